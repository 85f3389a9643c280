"""Radar operators of the hot path — host-side mirror of the reference module
``mm_masking/radar_utils.py`` (same function names, positional order and
argument meaning) with the arithmetic running in the hand-written gfx950
kernels of libmmk_hip.so (csrc/mmk_radar.hip) through the C ABI.

There is no CPU fallback: every kernel-backed function needs a HIP device and
the built library, and raises otherwise.  Tensors handed over on the CPU (the
reference runs these functions inside DataLoader workers,
icp_weight_dataset.py:336-352) are moved to the current HIP device and the
result is returned on the caller's device.

Reference line numbers are given per function (radar_utils.py:<lines>).
"""
import ctypes

import numpy as np
import torch

from . import _lib

__all__ = ["load_pc_from_file", "load_radar", "cfar_mask", "extract_pc", "extract_pc_padded", "extract_weights",
           "extract_weights_polar", "polar_target_from_pts", "extract_bev_from_pts", "mean_peaks_parallel_fast", "pol_2_cart", "radar_polar_to_cartesian",
           "radar_polar_to_cartesian_diff", "radar_cartesian_to_polar", "mask_polar_scan", "point_to_cart_idx",
           "form_cart_range_angle_grid", "form_polar_range_grid", "scan_times", "deskew_pc"]


def _hip_device(t):
    if t.is_cuda:
        return t.device
    if not torch.cuda.is_available():
        raise _lib.MmkError("radar_utils needs an MI355X/HIP device: the operators are HIP kernels with no CPU path")
    return torch.device("cuda", torch.cuda.current_device())


def _back(out, like):
    return out if like.is_cuda else out.to(like.device)


def _sized_workspace(size_fn, device, *dims):
    """The workspace, at least as large as the entry's own ``*_ws_bytes(*dims)`` asks."""
    return _lib.workspace(int(size_fn(*dims)), device, "radar")


def _remember(ctx, *inputs):
    """For the backward: the dtype and device the gradient of each input goes back in, and its shape (None: a number)."""
    ctx.like = [(t.dtype, t.device, tuple(t.shape)) if torch.is_tensor(t) else None for t in inputs]


def _grads_back(ctx, grads, n_rest):
    """``grads`` (None: not computed) in their inputs' dtype and on their device, then None for the ``n_rest`` constants."""
    return tuple(None if g is None else g.to(device=like[1], dtype=like[0]) for g, like in zip(grads, ctx.like)) + (None,) * n_rest


# ----------------------------------------------------------------------------- host-only helpers
def load_pc_from_file(file_path, to_type=None, to_device="cpu"):
    """radar_utils.py:10-18: float32 x 6 per point."""
    pc = np.fromfile(file_path, dtype=np.float32)
    pc = torch.from_numpy(pc.reshape((len(pc) // 6, 6))).to(to_device)
    return pc if to_type is None else pc.type(to_type)


def load_radar(raw_img):
    """radar_utils.py:20-27: Navtech PNG rows -> (fft f32 (A,R), azimuths f64 (A,), timestamps i64 (A,))."""
    raw = np.asarray(raw_img)
    timestamps = np.frombuffer(raw[:, :8].tobytes(), dtype=np.int64) * 1000
    azimuths = np.frombuffer(raw[:, 8:10].tobytes(), dtype=np.uint16) * (2 * np.pi / 5600)
    fft_data = np.divide(raw[:, 11:], 255.0, dtype=np.float32)
    return fft_data, azimuths, timestamps


def form_cart_range_angle_grid(cart_resolution=0.2384, cart_pixel_width=640, dtype=None, device="cpu"):
    """radar_utils.py:399-419.  Evaluated with the same PyTorch CPU ops as the
    reference (so the constant grid is bit-identical to the reference's on the
    same host), then moved to ``device``."""
    if (cart_pixel_width % 2) == 0:
        cart_min_range = (cart_pixel_width / 2 - 0.5) * cart_resolution
    else:
        cart_min_range = cart_pixel_width / 2 * cart_resolution
    kw = {} if dtype is None else {"dtype": dtype}
    coords = torch.linspace(-cart_min_range, cart_min_range, cart_pixel_width, **kw)
    Y, X = torch.meshgrid(coords, -1 * coords, indexing="xy")
    sample_range = torch.sqrt(Y * Y + X * X)
    sample_angle = torch.arctan2(Y, X)
    sample_angle = sample_angle + torch.where(sample_angle < 0, 2.0 * torch.pi, 0.0)
    return sample_range.to(device), sample_angle.to(device)


def form_polar_range_grid(polar_resolution=0.2384, polar_pixel_shape=(400, 3360), dtype=None, device="cpu"):
    """radar_utils.py:421-438."""
    polar_range = (polar_pixel_shape[1] - 1) * polar_resolution
    kw = {} if dtype is None else {"dtype": dtype}
    range_coords = torch.linspace(0.0, polar_range, polar_pixel_shape[1], **kw).to(device)
    return range_coords.unsqueeze(0).expand(polar_pixel_shape[0], -1)


_grid_cache = {}


def _device_grids(width, device):
    key = (width, device.type, device.index)
    g = _grid_cache.get(key)
    if g is None:
        # the reference ignores cart_resolution when it builds the grid (radar_utils.py:276)
        r, a = form_cart_range_angle_grid(cart_pixel_width=width, dtype=torch.float32)
        g = (r.contiguous().to(device), a.contiguous().to(device))
        _grid_cache[key] = g
    return g


def point_to_cart_idx(pc, cart_resolution=0.2384, cart_pixel_width=640, min_to_plus_1=False):
    """radar_utils.py:374-397 (tiny elementwise host logic; the kernels fuse it)."""
    grid_pc_u = -pc[:, :, 0] / cart_resolution
    grid_pc_v = pc[:, :, 1] / cart_resolution
    if min_to_plus_1:
        grid_pc = torch.stack((grid_pc_v, grid_pc_u), axis=2)
        return grid_pc / (cart_pixel_width - 1) * 2
    grid_pc = torch.stack((grid_pc_u, grid_pc_v), axis=2)
    return grid_pc + cart_pixel_width / 2


def mean_peaks_parallel_fast(arr, diff, steep_fact):
    """radar_utils.py:167-185.  Stand-alone elementwise form kept for API parity;
    ``extract_pc`` does not call it (the marker rule is fused into the HIP
    extraction kernels)."""
    res = torch.zeros_like(arr)
    zero_detect = (1 - torch.tanh(steep_fact * arr)) if diff else (arr == 0)
    res[:, :, :-1] = arr[:, :, :-1] * zero_detect[:, :, 1:] + arr[:, :, 1:] * zero_detect[:, :, :-1]
    return res


def pol_2_cart(pointcloud):
    """radar_utils.py:187-195."""
    rho, phi = pointcloud[:, 0], pointcloud[:, 1]
    return torch.stack((rho * torch.cos(phi), rho * torch.sin(phi), torch.zeros_like(rho)), axis=1)


def radar_polar_to_cartesian(*args, **kwargs):
    """radar_utils.py:197-256 (cv2.remap based).  Never called on the reference's
    train path: outside the hot-path scope."""
    raise NotImplementedError("radar_polar_to_cartesian (cv2) is dead code upstream and out of scope; "
                              "use radar_polar_to_cartesian_diff")


def _cart_to_polar_geometry(azimuths, radar_resolution, polar_pixel_shape, dev):
    """sin / cos of the azimuths and the range coordinates, formed on the host with the reference's own torch CPU calls."""
    az = azimuths.detach().to(device="cpu", dtype=torch.float64)
    rc = form_polar_range_grid(polar_resolution=radar_resolution, polar_pixel_shape=polar_pixel_shape, dtype=torch.float64,
                               device="cpu")[0]
    return torch.sin(az).to(dev).contiguous(), torch.cos(az).to(dev).contiguous(), rc.contiguous().to(dev)


def _cart_to_polar_forward(x, s_az, c_az, rc, cart_resolution):
    B, H, W = x.shape
    A, R = s_az.shape[1], rc.shape[0]
    out = torch.empty(B, A, R, dtype=torch.float64, device=x.device)
    _lib.check(_lib.lib().mmk_cart_to_polar(_lib.ptr(x), _lib.ptr(s_az), _lib.ptr(c_az), _lib.ptr(rc), B, A, R, H, W,
                                            float(cart_resolution), _lib.ptr(out), _lib.stream_ptr(x.device)))
    return out


class _CartToPolar(torch.autograd.Function):
    """radar_cartesian_to_polar with the gradient autograd takes through the F.grid_sample at radar_utils.py:370 with
    respect to the image (mmk_cart_to_polar_bwd).  The operator is linear in the image; the azimuths and both resolutions
    are constants."""

    @staticmethod
    def forward(ctx, cart, dev, s_az, c_az, rc, radar_resolution, cart_resolution):
        x = cart.detach().to(dev).contiguous()
        out = _cart_to_polar_forward(x, s_az, c_az, rc, cart_resolution)
        ctx.save_for_backward(s_az, c_az, rc)
        ctx.args = (tuple(x.shape), float(radar_resolution), float(cart_resolution))
        _remember(ctx, cart)
        return _back(out, cart)

    @staticmethod
    def backward(ctx, g):
        s_az, c_az, rc = ctx.saved_tensors
        (B, H, W), radar_resolution, cart_resolution = ctx.args
        A, R = s_az.shape[1], rc.shape[0]
        dev = s_az.device
        g = g.detach().to(device=dev, dtype=torch.float64).contiguous()
        L = _lib.lib()
        ws = _sized_workspace(L.mmk_cart_to_polar_bwd_ws_bytes, dev, B, A, R, H, W)
        gx = torch.empty(B, H, W, dtype=torch.float64, device=dev)
        _lib.check(L.mmk_cart_to_polar_bwd(_lib.ptr(g), _lib.ptr(s_az), _lib.ptr(c_az), _lib.ptr(rc), B, A, R, H, W,
                                           radar_resolution, cart_resolution, _lib.ptr(gx), _lib.ptr(ws), ws.numel(),
                                           _lib.stream_ptr(dev)))
        return _grads_back(ctx, (gx,), 6)


def radar_cartesian_to_polar(cart, azimuths, radar_resolution, cart_resolution=0.2384, polar_pixel_shape=(400, 3360)):
    """radar_utils.py:338-372.  (B,H,W) fp64 + (B,A) -> (B,A,R) fp64, bit-identical to the reference.
    As upstream, only an fp64 image is accepted: the reference casts its sampling grid to double (:370)
    and ``F.grid_sample`` raises ``RuntimeError`` on the dtype mismatch for anything else — same error here
    (a caller with an fp32 mask writes ``mask.double()``).
    sin / cos of the azimuths and the range coordinates are formed on the host with the reference's own
    torch CPU calls (B*A + R numbers); products, divisions and the bilinear gather run in the HIP kernel.
    The result is differentiable in ``cart`` (the gradient comes back in fp64 on its device); the azimuths
    and the resolutions are constants."""
    if cart.dtype != torch.float64:
        raise RuntimeError("expected scalar type Float but found Double" if cart.dtype == torch.float32 else
                           "expected scalar type %s but found Double" % str(cart.dtype).replace("torch.", "").capitalize())
    dev = _hip_device(cart)
    B, H, W = cart.shape
    A, R = int(polar_pixel_shape[0]), int(polar_pixel_shape[1])
    if azimuths.shape != (B, A):
        raise ValueError("azimuths must be (B, %d) (got %s)" % (A, tuple(azimuths.shape)))
    s_az, c_az, rc = _cart_to_polar_geometry(azimuths, radar_resolution, polar_pixel_shape, dev)
    if torch.is_grad_enabled() and cart.requires_grad:
        return _CartToPolar.apply(cart, dev, s_az, c_az, rc, radar_resolution, cart_resolution)
    x = cart.detach().to(dev).contiguous()
    return _back(_cart_to_polar_forward(x, s_az, c_az, rc, cart_resolution), cart)


def _mask_polar_scan_forward(x, m, s_az, c_az, rc, cart_resolution):
    B, A, R = x.shape
    out = torch.empty_like(x)
    _lib.check(_lib.lib().mmk_mask_polar_scan(_lib.ptr(x), _lib.ptr(m), _lib.ptr(s_az), _lib.ptr(c_az), _lib.ptr(rc), B, A, R,
                                              m.shape[1], m.shape[2], float(cart_resolution), _lib.ptr(out),
                                              _lib.stream_ptr(x.device)))
    return out


class _MaskPolarScan(torch.autograd.Function):
    """mask_polar_scan with the gradients autograd takes through ``radar_cartesian_to_polar(mask.double()).float() * scan``
    (mmk_mask_polar_scan_bwd): grad_scan = g * fl32(P) with P recomputed, grad_mask the fixed-point adjoint of the gather
    applied to fl32(g * scan).  The azimuths and both resolutions are constants."""

    @staticmethod
    def forward(ctx, scan, mask, dev, s_az, c_az, rc, radar_resolution, cart_resolution):
        x, m = _lib.dev_f32(scan, dev), _lib.dev_f32(mask, dev)
        out = _mask_polar_scan_forward(x, m, s_az, c_az, rc, cart_resolution)
        ctx.save_for_backward(x, m, s_az, c_az, rc)
        ctx.args = (float(radar_resolution), float(cart_resolution))
        _remember(ctx, scan, mask)
        return _back(out, scan)

    @staticmethod
    def backward(ctx, g):
        x, m, s_az, c_az, rc = ctx.saved_tensors
        radar_resolution, cart_resolution = ctx.args
        (B, A, R), (H, W) = x.shape, m.shape[1:]
        dev = x.device
        g = _lib.dev_f32(g, dev)
        want_scan, want_mask = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        L = _lib.lib()
        ws = _sized_workspace(L.mmk_mask_polar_scan_bwd_ws_bytes, dev, B, A, R, H, W) if want_mask else None
        gx = torch.empty_like(x) if want_scan else None
        gm = torch.empty_like(m) if want_mask else None
        _lib.check(L.mmk_mask_polar_scan_bwd(_lib.ptr(g), _lib.ptr(x), _lib.ptr(m), _lib.ptr(s_az), _lib.ptr(c_az), _lib.ptr(rc),
                                             B, A, R, H, W, radar_resolution, cart_resolution, _lib.ptr(gx), _lib.ptr(gm),
                                             _lib.ptr(ws), ws.numel() if want_mask else 0, _lib.stream_ptr(dev)))
        return _grads_back(ctx, (gx, gm), 6)


def mask_polar_scan(scan, mask, azimuths, radar_resolution, cart_resolution=0.2384):
    """The Cartesian mask applied to the polar scan, the masked scan of icp_weight_policy.py:266:
    ``radar_cartesian_to_polar(mask.double(), azimuths, radar_resolution, cart_resolution, scan.shape[1:]).float() * scan``
    in one kernel, bit for bit, without the fp64 polar image of the mask.  (B,A,R) scan + (B,H,W) mask + (B,A) azimuths ->
    (B,A,R) fp32, on the scan's device.  Differentiable in ``scan`` and in ``mask`` (each gradient comes back in its input's
    dtype and on its device; only the halves that are needed are computed); the azimuths and the resolutions are constants."""
    assert scan.ndim == 3 and mask.ndim == 3, "scan must be (B,A,R) and mask (B,H,W)"
    dev = _hip_device(scan)
    B, A, R = scan.shape
    if mask.shape[0] != B:
        raise ValueError("mask must be (%d, H, W) (got %s)" % (B, tuple(mask.shape)))
    if azimuths.shape != (B, A):
        raise ValueError("azimuths must be (B, %d) (got %s)" % (A, tuple(azimuths.shape)))
    s_az, c_az, rc = _cart_to_polar_geometry(azimuths, radar_resolution, (A, R), dev)
    if torch.is_grad_enabled() and (scan.requires_grad or mask.requires_grad):
        return _MaskPolarScan.apply(scan, mask, dev, s_az, c_az, rc, radar_resolution, cart_resolution)
    out = _mask_polar_scan_forward(_lib.dev_f32(scan, dev), _lib.dev_f32(mask, dev), s_az, c_az, rc, cart_resolution)
    return _back(out, scan)


# ----------------------------------------------------------------------------- R2
def cfar_cols(n_range, res, width=101, minr=2.0, maxr=80.0, guard=5):
    """Window half width and column range of radar_utils.py:34-39."""
    width = width + 1 if width % 2 == 0 else width
    w2 = width // 2
    mincol = max(0, int(minr / res + w2 + guard + 1))
    maxcol = min(n_range, int(maxr / res - w2 - guard))
    return w2, mincol, maxcol


def _cfar_forward(x, cols, a, b, diff, steep_fact):
    """Thresholds that are numbers go to mmk_cfar_mask; device tensors (both, of equal length) go to mmk_cfar_mask_p."""
    B, A, R = x.shape
    w2, guard, mincol, maxcol = cols
    out = torch.empty_like(x)
    head = (_lib.ptr(x), B, A, R, w2, guard, mincol, max(mincol, maxcol))
    tail = (1 if diff else 0, float(steep_fact), _lib.ptr(out), _lib.stream_ptr(x.device))
    if torch.is_tensor(a):
        _lib.check(_lib.lib().mmk_cfar_mask_p(*head, _lib.ptr(a), _lib.ptr(b), 1 if a.numel() > 1 else 0, *tail))
    else:
        _lib.check(_lib.lib().mmk_cfar_mask(*head, float(a), float(b), *tail))
    return out


class _CfarMask(torch.autograd.Function):
    """cfar_mask(diff=True) with the gradient autograd takes through radar_utils.py:29-69 (mmk_cfar_mask_bwd): tanh's
    slope on the cells hardshrink keeps, directly and through the GO-CFAR threshold into the winning window."""

    @staticmethod
    def forward(ctx, raw_scans, dev, cols, a_thresh, b_thresh, steep_fact):
        x = _lib.dev_f32(raw_scans, dev)
        out = _cfar_forward(x, cols, a_thresh, b_thresh, True, steep_fact)
        ctx.save_for_backward(x)
        ctx.args = (cols, float(a_thresh), float(b_thresh), float(steep_fact))
        _remember(ctx, raw_scans)
        return _back(out, raw_scans)

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        (w2, guard, mincol, maxcol), a_thresh, b_thresh, steep_fact = ctx.args
        B, A, R = x.shape
        g = _lib.dev_f32(g, x.device)
        gx = torch.empty_like(x)
        _lib.check(_lib.lib().mmk_cfar_mask_bwd(_lib.ptr(x), _lib.ptr(g), B, A, R, w2, guard, mincol, max(mincol, maxcol),
                                                a_thresh, b_thresh, steep_fact, _lib.ptr(gx), _lib.stream_ptr(x.device)))
        return _grads_back(ctx, (gx,), 5)


def _cfar_threshold_sizes(a_thresh, b_thresh, B):
    """Number of values the kernels read per threshold (1: shared by the batch, B: one per scan) for thresholds of which
    at least one is a tensor.  Shapes are checked here, before anything touches the device."""
    n = 1
    for name, v in (("a_thresh", a_thresh), ("b_thresh", b_thresh)):
        if not torch.is_tensor(v):
            continue
        shape = tuple(v.shape)
        if shape not in ((), (1,), (B,), (B, 1, 1)):
            raise ValueError("%s must be a number or a tensor of shape (), (1,), (%d,) or (%d, 1, 1) (got %s)"
                             % (name, B, B, shape))
        n = max(n, v.numel())
    return n


def _cfar_threshold_dev(v, n, dev):
    """A threshold as n contiguous fp32 values on the device; a number or a single value is broadcast there."""
    if torch.is_tensor(v):
        t = v.detach().to(device=dev, dtype=torch.float32).reshape(-1)
        return t.expand(n).contiguous() if t.numel() != n else t.contiguous()
    return torch.full((n,), float(v), dtype=torch.float32, device=dev)


class _CfarMaskP(torch.autograd.Function):
    """cfar_mask(diff=True) with tensor thresholds (mmk_cfar_mask_p / mmk_cfar_mask_bwd_p): the scan's gradient of _CfarMask
    and the gradients autograd takes through ``thres = a_thresh * stat + b_thresh`` (radar_utils.py:56) with respect to the
    two thresholds, per scan or summed over the batch as the thresholds' shapes ask."""

    @staticmethod
    def forward(ctx, raw_scans, a_thresh, b_thresh, dev, cols, steep_fact, n):
        x = _lib.dev_f32(raw_scans, dev)
        a, b = _cfar_threshold_dev(a_thresh, n, dev), _cfar_threshold_dev(b_thresh, n, dev)
        out = _cfar_forward(x, cols, a, b, True, steep_fact)
        ctx.save_for_backward(x, a, b)
        ctx.args = (cols, float(steep_fact))
        _remember(ctx, raw_scans, a_thresh, b_thresh)
        return _back(out, raw_scans)

    @staticmethod
    def backward(ctx, g):
        x, a, b = ctx.saved_tensors
        (w2, guard, mincol, maxcol), steep_fact = ctx.args
        B, A, R = x.shape
        dev = x.device
        g = _lib.dev_f32(g, dev)
        L = _lib.lib()
        gx = torch.empty_like(x) if ctx.needs_input_grad[0] else None       # NULL: the kernel stops after its first pass
        ga, gb = torch.empty_like(a), torch.empty_like(b)
        ws = _sized_workspace(L.mmk_cfar_mask_bwd_p_ws_bytes, dev, B, A)
        _lib.check(L.mmk_cfar_mask_bwd_p(_lib.ptr(x), _lib.ptr(g), B, A, R, w2, guard, mincol, max(mincol, maxcol), _lib.ptr(a),
                                         _lib.ptr(b), 1 if a.numel() > 1 else 0, steep_fact, _lib.ptr(gx), _lib.ptr(ga),
                                         _lib.ptr(gb), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev)))
        grads = []
        for need, like, val in zip(ctx.needs_input_grad, ctx.like, (gx, ga, gb)):
            if need and val.numel() != int(np.prod(like[2])):               # a single value broadcast over the scans
                val = val.sum()
            grads.append(val.reshape(like[2]) if need else None)
        return _grads_back(ctx, grads, 4)


def cfar_mask(raw_scans, res, width=101, minr=2.0, maxr=80.0, guard=5,
              a_thresh=1.0, b_thresh=0.09, diff=True, steep_fact=10.0):
    """GO-CFAR mask, radar_utils.py:29-69.  (B,A,R) fp32 -> (B,A,R) fp32.  With ``diff=True`` the mask is
    differentiable in ``raw_scans`` (the gradient comes back in its dtype and on its device); with ``diff=False`` it
    does not require grad, as upstream (torch.where of constants).

    ``a_thresh`` and ``b_thresh`` are Python numbers or, as upstream's ``a_thresh * stat + b_thresh`` (:56) allows, tensors of
    shape (), (1,), (B,) or (B,1,1): one value for the batch or one per scan.  Tensors are read on the device (no host
    synchronisation; a number mixed with a tensor is broadcast there), and with ``diff=True`` each one that requires grad
    receives its gradient in its own shape, dtype and on its device.  Any other shape raises ``ValueError``."""
    assert raw_scans.ndim == 3, "raw_scans must be 3D"
    tensors = torch.is_tensor(a_thresh) or torch.is_tensor(b_thresh)
    n = _cfar_threshold_sizes(a_thresh, b_thresh, raw_scans.shape[0]) if tensors else 0
    dev = _hip_device(raw_scans)
    w2, mincol, maxcol = cfar_cols(raw_scans.shape[2], res, width, minr, maxr, guard)
    cols = (w2, guard, mincol, maxcol)
    if diff and torch.is_grad_enabled() and any(torch.is_tensor(t) and t.requires_grad for t in (raw_scans, a_thresh, b_thresh)):
        if tensors:
            return _CfarMaskP.apply(raw_scans, a_thresh, b_thresh, dev, cols, steep_fact, n)
        return _CfarMask.apply(raw_scans, dev, cols, a_thresh, b_thresh, steep_fact)
    if tensors:
        a_thresh, b_thresh = _cfar_threshold_dev(a_thresh, n, dev), _cfar_threshold_dev(b_thresh, n, dev)
    return _back(_cfar_forward(_lib.dev_f32(raw_scans, dev), cols, a_thresh, b_thresh, diff, steep_fact), raw_scans)


# ----------------------------------------------------------------------------- R3 + R4
def _peaks_forward(m, res, az, tm, Tab, diff, steep_fact, max_pts, with_times=False):
    """(pc, cnt) from mmk_extract_peaks or, ``with_times``, (pc, cnt, t) from mmk_extract_peaks_t."""
    B, A, R = m.shape
    dev = m.device
    L = _lib.lib()
    ws = _sized_workspace(L.mmk_extract_peaks_workspace_bytes, dev, B, A, R, int(max_pts))
    pc = torch.empty(B, int(max_pts), 3, dtype=torch.float32, device=dev)
    cnt = torch.empty(B, dtype=torch.int32, device=dev)
    args = (_lib.ptr(m), B, A, R, float(res), _lib.ptr(az), _lib.ptr(tm), _lib.ptr(Tab), 1 if diff else 0, float(steep_fact),
            int(max_pts), _lib.ptr(pc), _lib.ptr(cnt), _lib.ptr(ws), ws.numel())
    if not with_times:
        _lib.check(L.mmk_extract_peaks(*args, _lib.stream_ptr(dev)))
        return pc, cnt
    t = torch.empty(B, int(max_pts), dtype=torch.float32, device=dev)
    _lib.check(L.mmk_extract_peaks_t(*args, _lib.ptr(t), _lib.stream_ptr(dev)))
    return pc, cnt, t


class _ExtractPeaks(torch.autograd.Function):
    """extract_pc_padded with the gradient autograd takes through radar_utils.py:71-106 / :167-185 with respect to the
    mask (mmk_extract_peaks_bwd).  The marker set, its order and its pairing are constants; so are the azimuths and T_ab,
    and the per-point times (``with_times``) are a non-differentiable output."""

    @staticmethod
    def forward(ctx, thres_mask, m, res, az, tm, Tab, diff, steep_fact, max_pts, with_times=False):
        out = _peaks_forward(m, res, az, tm, Tab, diff, steep_fact, max_pts, with_times)
        ctx.save_for_backward(m, az, Tab)
        ctx.args = (float(res), 1 if diff else 0, float(steep_fact), int(max_pts))
        _remember(ctx, thres_mask)
        ctx.mark_non_differentiable(*out[1:])
        return out

    @staticmethod
    def backward(ctx, gpc, *_rest):
        m, az, Tab = ctx.saved_tensors
        res, diff, steep_fact, max_pts = ctx.args
        B, A, R = m.shape
        dev = m.device
        gpc = _lib.dev_f32(gpc, dev)
        L = _lib.lib()
        ws = _sized_workspace(L.mmk_extract_peaks_bwd_workspace_bytes, dev, B, A, R, max_pts)
        gm = torch.empty_like(m)
        _lib.check(L.mmk_extract_peaks_bwd(_lib.ptr(m), B, A, R, res, _lib.ptr(az), _lib.ptr(Tab), diff, steep_fact, max_pts,
                                           _lib.ptr(gpc), _lib.ptr(gm), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev)))
        return _grads_back(ctx, (gm,), 9)


def extract_pc_padded(thres_mask, res, azimuth_angles, azimuth_times, max_pts, T_ab=None, diff=True,
                      steep_fact=10.0, return_times=False):
    """Batched form of ``extract_pc``: zero-padded (B,max_pts,3) cloud in the
    reference's azimuth-major order plus the per-item point count (int32 (B,)),
    with no host synchronisation.  This is the layout the dataset hands to the
    policy (icp_weight_dataset.py:379-381).  The cloud is differentiable in
    ``thres_mask`` for both values of ``diff`` (the gradient comes back in the mask's
    dtype and on its device); ``azimuth_angles``, ``azimuth_times`` and ``T_ab`` are
    constants, and the count is a non-differentiable int32 tensor.

    ``return_times=True`` returns ``(pc, cnt, t)``: ``t`` (B,max_pts) fp32 is the time of every point, the mean of its two
    markers' ``azimuth_times`` (the column the reference's pair mean forms at :97 and pol_2_cart drops), 0 in the padding
    rows, in the unit of ``azimuth_times`` (``scan_times`` gives seconds relative to the scan's reference time).  It is a
    constant, never differentiated; ``T_ab`` does not enter it.  ``azimuth_times=None`` is then a ``ValueError``."""
    if return_times and azimuth_times is None:
        raise ValueError("extract_pc_padded: return_times=True needs azimuth_times")
    dev = _hip_device(thres_mask)
    m = _lib.dev_f32(thres_mask, dev)
    az = _lib.dev_f32(azimuth_angles, dev)
    tm = _lib.dev_f32(azimuth_times, dev) if azimuth_times is not None else None
    Tab = _lib.dev_f32(T_ab, dev).reshape(-1, 16) if T_ab is not None else None
    if torch.is_grad_enabled() and thres_mask.requires_grad:
        return _ExtractPeaks.apply(thres_mask, m, res, az, tm, Tab, diff, steep_fact, max_pts, bool(return_times))
    return _peaks_forward(m, res, az, tm, Tab, diff, steep_fact, max_pts, bool(return_times))


def scan_times(az_times, unit=1e-6, ref="mid"):
    """The azimuth stamps of a scan as (B,A) fp32 seconds relative to the scan's reference time: what ``deskew_pc`` reads
    through ``extract_pc_padded(..., return_times=True)``.  ``az_times`` (B,A) holds stamps in multiples of ``unit``
    seconds, integers or floats of any size (epoch stamps included: the subtraction runs in fp64 before the cast).  ``ref``
    names the reference time of each row: "mid" = (min + max) / 2 of its stamps, "first" = min, "last" = max -- min and max,
    so that a row rolled by the augmentation keeps its reference.  Stays on the device of ``az_times``."""
    if ref not in ("mid", "first", "last"):
        raise ValueError("scan_times: ref must be 'mid', 'first' or 'last' (got %r)" % (ref,))
    if az_times.ndim != 2:
        raise ValueError("scan_times: az_times must be (B, A) (got %s)" % (tuple(az_times.shape),))
    t = az_times.detach().to(torch.float64)
    lo, hi = t.amin(dim=1, keepdim=True), t.amax(dim=1, keepdim=True)
    t0 = lo if ref == "first" else hi if ref == "last" else lo + (hi - lo) / 2
    return ((t - t0) * float(unit)).to(torch.float32)


# ----------------------------------------------------------------------------- D1
class _DeskewPoints(torch.autograd.Function):
    """deskew_pc with its hand-derived gradients (mmk_deskew_points_bwd): grad_pc = R^T g per point, grad_twist the ordered
    fp64 sum of the points' shares.  Only the halves that are needed are computed; the times are constants."""

    @staticmethod
    def forward(ctx, pc, twist, dev, t):
        p, w = _lib.dev_f32(pc, dev), _lib.dev_f32(twist, dev)
        out = _deskew_forward(p, t, w)
        ctx.save_for_backward(p, t, w)
        _remember(ctx, pc, twist)
        return _back(out, pc)

    @staticmethod
    def backward(ctx, g):
        p, t, w = ctx.saved_tensors
        B, N = t.shape
        dev = p.device
        g = _lib.dev_f32(g, dev)
        want_pc, want_twist = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        L = _lib.lib()
        ws = _sized_workspace(L.mmk_deskew_points_bwd_workspace_bytes, dev, B, N) if want_twist else None
        gp = torch.empty_like(p) if want_pc else None
        gw = torch.empty_like(w) if want_twist else None
        _lib.check(L.mmk_deskew_points_bwd(_lib.ptr(p), _lib.ptr(t), _lib.ptr(w), B, N, _lib.ptr(g), _lib.ptr(gp), _lib.ptr(gw),
                                           _lib.ptr(ws), ws.numel() if want_twist else 0, _lib.stream_ptr(dev)))
        return _grads_back(ctx, (gp, gw), 2)


def _deskew_forward(p, t, w):
    B, N = t.shape
    out = torch.empty_like(p)
    _lib.check(_lib.lib().mmk_deskew_points(_lib.ptr(p), _lib.ptr(t), _lib.ptr(w), B, N, _lib.ptr(out), _lib.stream_ptr(p.device)))
    return out


def deskew_pc(pc, t, twist):
    """Constant-twist motion compensation of a scan cloud (absent upstream, whose ``filtered_pc`` arrives
    compensated, icp_weight_dataset.py:331-332).  ``pc`` (B,N,3), ``t`` (B,N) the points' times in seconds relative to the
    scan's reference time (``extract_pc_padded(..., return_times=True)`` of ``scan_times``), ``twist`` (B,6) = (v; omega), the
    sensor's body-frame velocity in m/s and rad/s, translation first, constant over the scan.  Point i moves to
    ``Exp(t_i twist) p_i``, where it would have been measured from the sensor's pose at the reference time; evaluated per
    point in fp64 with one rounding per output.  A row of ``pc`` that is exactly (0, 0, 0) is padding and stays 0.  A zero
    twist and a zero time return the input bits; a planar twist keeps z = 0.  Differentiable in ``pc`` and ``twist`` (each
    gradient comes back in its input's dtype and on its device; the twist's is an ordered fp64 sum, equal bits in every
    run); ``t`` is a constant."""
    if pc.ndim != 3 or pc.shape[2] != 3:
        raise ValueError("deskew_pc: pc must be (B, N, 3) (got %s)" % (tuple(pc.shape),))
    B, N = pc.shape[0], pc.shape[1]
    if tuple(t.shape) != (B, N):
        raise ValueError("deskew_pc: t must be (%d, %d) (got %s)" % (B, N, tuple(t.shape)))
    if tuple(twist.shape) != (B, 6):
        raise ValueError("deskew_pc: twist must be (%d, 6) (got %s)" % (B, tuple(twist.shape)))
    if B < 1 or N < 1:
        raise ValueError("deskew_pc: empty cloud %s" % (tuple(pc.shape),))
    dev = _hip_device(pc)
    tt = _lib.dev_f32(t, dev)
    if torch.is_grad_enabled() and (pc.requires_grad or twist.requires_grad):
        return _DeskewPoints.apply(pc, twist, dev, tt)
    return _back(_deskew_forward(_lib.dev_f32(pc, dev), tt, _lib.dev_f32(twist, dev)), pc)


def extract_pc(thres_mask, res, azimuth_angles, azimuth_times, T_ab=None, diff=True, steep_fact=10.0):
    """radar_utils.py:71-106: Python list of ragged (n_i,3) clouds (one host sync
    to read the counts, as the reference's ``nonzero`` implies).  When ``thres_mask``
    requires grad the clouds are slices of the padded cloud that keep its graph, so a
    loss on a list element reaches the mask; the azimuths and ``T_ab`` are constants."""
    B, A, R = thres_mask.shape
    cap = (A * (R - 1) + 1) // 2
    cap = min(cap, 1 << 20)
    pc, cnt = extract_pc_padded(thres_mask, res, azimuth_angles, azimuth_times, cap, T_ab=T_ab, diff=diff,
                                steep_fact=steep_fact)
    counts = cnt.cpu().tolist()
    return [_back(pc[b, :min(n, cap)].clone(), thres_mask) for b, n in enumerate(counts)]


# ----------------------------------------------------------------------------- R5
def _polar_to_cart_forward(x, az, W, radar_resolution, interpolate_crossover, fix_wobble):
    B, A, R = x.shape
    rg, ag = _device_grids(W, x.device)
    out = torch.empty(B, W, W, dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().mmk_polar_to_cart(_lib.ptr(x), _lib.ptr(az), _lib.ptr(rg), _lib.ptr(ag), B, A, R, W,
                                            float(radar_resolution), 1 if interpolate_crossover else 0,
                                            1 if fix_wobble else 0, _lib.ptr(out), _lib.stream_ptr(x.device)))
    return out


class _PolarToCart(torch.autograd.Function):
    """radar_polar_to_cartesian_diff with the gradient autograd takes through the F.grid_sample at radar_utils.py:334 and
    the wrap rows of :318 with respect to the polar image (mmk_polar_to_cart_bwd).  The operator is linear in the image;
    the azimuths, the pixel grid and the resolution are constants."""

    @staticmethod
    def forward(ctx, fft_data, dev, az, W, radar_resolution, interpolate_crossover, fix_wobble):
        x = _lib.dev_f32(fft_data, dev)
        out = _polar_to_cart_forward(x, az, W, radar_resolution, interpolate_crossover, fix_wobble)
        ctx.save_for_backward(az)
        ctx.args = (tuple(x.shape), W, float(radar_resolution), 1 if interpolate_crossover else 0, 1 if fix_wobble else 0)
        _remember(ctx, fft_data)
        return _back(out, fft_data)

    @staticmethod
    def backward(ctx, g):
        (az,) = ctx.saved_tensors
        (B, A, R), W, radar_resolution, crossover, wobble = ctx.args
        dev = az.device
        g = _lib.dev_f32(g, dev)
        rg, ag = _device_grids(W, dev)
        L = _lib.lib()
        ws = _sized_workspace(L.mmk_polar_to_cart_bwd_ws_bytes, dev, B, A, R, W)
        gx = torch.empty(B, A, R, dtype=torch.float32, device=dev)
        _lib.check(L.mmk_polar_to_cart_bwd(_lib.ptr(g), _lib.ptr(az), _lib.ptr(rg), _lib.ptr(ag), B, A, R, W, radar_resolution,
                                           crossover, wobble, _lib.ptr(gx), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev)))
        return _grads_back(ctx, (gx,), 6)


def radar_polar_to_cartesian_diff(fft_data, azimuths, radar_resolution, cart_resolution=0.2384, cart_pixel_width=640,
                                  interpolate_crossover=True, fix_wobble=True):
    """radar_utils.py:258-336.  (B,A,R) + (B,A) -> (B,W,W).  As upstream, the
    pixel grid is built with the default 0.2384 m resolution whatever
    ``cart_resolution`` says (radar_utils.py:276).  The image is differentiable in ``fft_data`` (the gradient comes
    back in its dtype and on its device); the azimuths are constants."""
    dev = _hip_device(fft_data)
    az = _lib.dev_f32(azimuths, dev)
    W = int(cart_pixel_width)
    if torch.is_grad_enabled() and fft_data.requires_grad:
        return _PolarToCart.apply(fft_data, dev, az, W, radar_resolution, interpolate_crossover, fix_wobble)
    x = _lib.dev_f32(fft_data, dev)
    return _back(_polar_to_cart_forward(x, az, W, radar_resolution, interpolate_crossover, fix_wobble), fft_data)


def _polar_to_cart_pair(img_a, img_b, azimuths, radar_resolution, cart_pixel_width=640):
    """radar_polar_to_cartesian_diff of two images that share their azimuths (the FFT and the CFAR
    image of a scan, icp_weight_dataset.py:350-352) in one launch: same values as two calls."""
    dev = _hip_device(img_a)
    a, b = _lib.dev_f32(img_a, dev), _lib.dev_f32(img_b, dev)
    az = _lib.dev_f32(azimuths, dev)
    assert a.shape == b.shape
    B, A, R = a.shape
    W = int(cart_pixel_width)
    rg, ag = _device_grids(W, dev)
    out_a = torch.empty(B, W, W, dtype=torch.float32, device=dev)
    out_b = torch.empty(B, W, W, dtype=torch.float32, device=dev)
    _lib.check(_lib.lib().mmk_polar_to_cart_pair(_lib.ptr(a), _lib.ptr(b), _lib.ptr(az), _lib.ptr(rg), _lib.ptr(ag), B, A, R, W,
                                                 float(radar_resolution), 1, 1, _lib.ptr(out_a), _lib.ptr(out_b),
                                                 _lib.stream_ptr(dev)))
    return _back(out_a, img_a), _back(out_b, img_b)


# ----------------------------------------------------------------------------- R9
class _SampleWeights(torch.autograd.Function):
    """Bilinear gather of the mask at the scan points; backward is the
    scatter-add into the 4 taps (what autograd does for F.grid_sample at
    radar_utils.py:126) and, when the points require grad, the bilinear slope at
    each point (mmk_sample_weights_bwd_pc)."""

    @staticmethod
    def forward(ctx, mask, pc, cart_resolution, cart_pixel_width=640):
        B, H, W = mask.shape
        N, cols = pc.shape[1], pc.shape[2]
        out = torch.empty(B, N, dtype=torch.float32, device=mask.device)
        _lib.check(_lib.lib().mmk_sample_weights_fwd(_lib.ptr(mask, torch.float32, "mask"), _lib.ptr(pc), B, N, cols,
                                                     H, W, int(cart_pixel_width), float(cart_resolution), _lib.ptr(out),
                                                     _lib.stream_ptr(mask.device)))
        ctx.save_for_backward(pc, mask if ctx.needs_input_grad[1] else None)
        ctx.shape = (B, H, W)
        ctx.cres = float(cart_resolution)
        ctx.cw = int(cart_pixel_width)
        return out

    @staticmethod
    def backward(ctx, gw):
        pc, mask = ctx.saved_tensors
        B, H, W = ctx.shape
        gw = gw.contiguous().float()
        gmask = torch.empty(B, H, W, dtype=torch.float32, device=gw.device)
        ws = _sized_workspace(_lib.lib().mmk_sample_weights_bwd_ws_bytes, gw.device, B, pc.shape[1])
        _lib.check(_lib.lib().mmk_sample_weights_bwd(_lib.ptr(gw), _lib.ptr(pc), B, pc.shape[1], pc.shape[2], H, W, ctx.cw, ctx.cres,
                                                     _lib.ptr(gmask), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(gw.device)))
        gpc = None
        if ctx.needs_input_grad[1]:
            gpc = torch.empty_like(pc)
            _lib.check(_lib.lib().mmk_sample_weights_bwd_pc(_lib.ptr(gw), _lib.ptr(mask), _lib.ptr(pc), B, pc.shape[1], pc.shape[2],
                                                            H, W, ctx.cw, ctx.cres, _lib.ptr(gpc), _lib.stream_ptr(gw.device)))
        return gmask, gpc, None, None


class _WeightStats(torch.autograd.Function):
    """The statistics of extract_weights (radar_utils.py:130-138) in one pass (mmk_weight_stats).
    Only diff_mean_num_non0 carries a gradient (d/dw of sum(0.5 tanh(5w) + 0.5) / B over real points)."""

    @staticmethod
    def forward(ctx, weights, pc):
        B, N = weights.shape
        part = torch.empty(B * 8, dtype=torch.float32, device=weights.device)
        out = torch.empty(8, dtype=torch.float32, device=weights.device)
        w = weights.contiguous()
        _lib.check(_lib.lib().mmk_weight_stats(_lib.ptr(w), _lib.ptr(pc), B, N, pc.shape[2], _lib.ptr(part), _lib.ptr(out),
                                               _lib.stream_ptr(weights.device)))
        ctx.save_for_backward(w, pc)
        diff = out[0].clone()
        ctx.mark_non_differentiable(out)
        return diff, out

    @staticmethod
    def backward(ctx, g_diff, _g_stats):
        if g_diff is None:
            return None, None
        w, pc = ctx.saved_tensors
        real = ~((pc[:, :, 0] == 0.0) & (pc[:, :, 1] == 0.0))
        t = torch.tanh(5 * w)
        return g_diff * (2.5 / w.shape[0]) * (1 - t * t) * real, None


def _sample_with_stats(mask, scan_pc, sample):
    """What both extract_weights return, plus the raw statistics vector of mmk_weight_stats (the policy takes its
    mean_all_pts from it); ``sample(m, pc, dev)`` gives the weights of the device copies of the mask and the points."""
    dev = _hip_device(mask)
    m = mask if (mask.is_cuda and mask.dtype == torch.float32 and mask.is_contiguous()) else \
        mask.to(device=dev, dtype=torch.float32).contiguous()
    pc = scan_pc.to(device=dev, dtype=torch.float32).contiguous()      # not detached: differentiable in x, y
    weights = sample(m, pc, dev)
    diff_mean_num_non0, st = _WeightStats.apply(weights, pc)
    if not mask.is_cuda:
        weights = weights.to(mask.device)
    return (weights, diff_mean_num_non0, st[1], st[2], st[3], st[4]), st


def _extract_weights_stats(mask, scan_pc):
    """extract_weights plus the raw statistics vector."""
    # point_to_cart_idx's defaults (0.2384 m, 640 px) whatever the mask's shape: radar_utils.py:112
    return _sample_with_stats(mask, scan_pc, lambda m, pc, dev: _SampleWeights.apply(m, pc, 0.2384, 640))


def extract_weights(mask, scan_pc):
    """radar_utils.py:108-140 -> (weights (B,N), diff_mean_num_non0, mean_num_non0,
    mean_w, max_w, min_w).  The statistics are the reference's, formed over the real points in one
    fused pass (no boolean indexing, no host sync).  The weights are differentiable in ``mask`` and, as
    F.grid_sample is in its grid, in the x and y columns of ``scan_pc`` (its other columns and the fake
    (0, 0) rows get 0); diff_mean_num_non0 is differentiable through the weights."""
    return _extract_weights_stats(mask, scan_pc)[0]


class _SampleWeightsPolar(torch.autograd.Function):
    """Bilinear gather of a polar mask at the scan points' own ranges and angles (mmk_sample_weights_polar_fwd); backward is
    the ordered scatter-add into the taps with the crossover rows folded onto their data rows (mmk_sample_weights_polar_bwd)
    and, when the points require grad, the slope at each point chained through its range and angle
    (mmk_sample_weights_polar_bwd_pc).  The azimuths, the resolution and the two flags are constants."""

    @staticmethod
    def forward(ctx, mask, pc, az, radar_resolution, interpolate_crossover, fix_wobble):
        B, A, R = mask.shape
        N, cols = pc.shape[1], pc.shape[2]
        out = torch.empty(B, N, dtype=torch.float32, device=mask.device)
        args = (float(radar_resolution), 1 if interpolate_crossover else 0, 1 if fix_wobble else 0)
        _lib.check(_lib.lib().mmk_sample_weights_polar_fwd(_lib.ptr(mask, torch.float32, "mask"), _lib.ptr(pc), _lib.ptr(az), B, N,
                                                           cols, A, R, *args, _lib.ptr(out), _lib.stream_ptr(mask.device)))
        ctx.save_for_backward(pc, az, mask if ctx.needs_input_grad[1] else None)
        ctx.shape = (B, A, R)
        ctx.args = args
        return out

    @staticmethod
    def backward(ctx, gw):
        pc, az, mask = ctx.saved_tensors
        B, A, R = ctx.shape
        N, cols = pc.shape[1], pc.shape[2]
        gw = gw.contiguous().float()
        L = _lib.lib()
        gmask = None
        if ctx.needs_input_grad[0]:
            gmask = torch.empty(B, A, R, dtype=torch.float32, device=gw.device)
            ws = _sized_workspace(L.mmk_sample_weights_polar_bwd_ws_bytes, gw.device, B, N)
            _lib.check(L.mmk_sample_weights_polar_bwd(_lib.ptr(gw), _lib.ptr(pc), _lib.ptr(az), B, N, cols, A, R, *ctx.args,
                                                      _lib.ptr(gmask), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(gw.device)))
        gpc = None
        if ctx.needs_input_grad[1]:
            gpc = torch.empty_like(pc)
            _lib.check(L.mmk_sample_weights_polar_bwd_pc(_lib.ptr(gw), _lib.ptr(mask), _lib.ptr(pc), _lib.ptr(az), B, N, cols, A, R,
                                                         *ctx.args, _lib.ptr(gpc), _lib.stream_ptr(gw.device)))
        return gmask, gpc, None, None, None, None


def _extract_weights_polar_stats(mask, scan_pc, azimuths, radar_resolution, interpolate_crossover=True, fix_wobble=True):
    """extract_weights_polar plus the raw statistics vector of mmk_weight_stats, as _extract_weights_stats."""
    if mask.ndim != 3 or scan_pc.ndim != 3 or scan_pc.shape[0] != mask.shape[0]:
        raise ValueError("mask must be (B,A,R) and scan_pc (B,N,>=2) (got %s and %s)" % (tuple(mask.shape), tuple(scan_pc.shape)))
    if tuple(azimuths.shape) != (mask.shape[0], mask.shape[1]):
        raise ValueError("azimuths must be (B, %d) (got %s)" % (mask.shape[1], tuple(azimuths.shape)))
    return _sample_with_stats(mask, scan_pc, lambda m, pc, dev: _SampleWeightsPolar.apply(
        m, pc, _lib.dev_f32(azimuths, dev), radar_resolution, interpolate_crossover, fix_wobble))


def extract_weights_polar(mask, scan_pc, azimuths, radar_resolution, interpolate_crossover=True, fix_wobble=True):
    """extract_weights for a POLAR mask (B,A,R): every point reads the mask where it lies in the polar image -- its range
    and its angle against the item's azimuth table ``azimuths`` (B,A), ascending, on the host or the device -- with the
    sampling arithmetic of ``radar_polar_to_cartesian_diff`` (radar_utils.py:276-323; the two flags are its flags), so a
    point at the centre of a pixel of the 0.2384 m Cartesian grid gets what that function writes to the pixel.  Absent
    upstream, whose extract_weights samples any mask with the Cartesian grid's normalisation (kept as is in
    ``extract_weights``).  Returns extract_weights' 6-tuple, the statistics from the same fused pass.  The weights are
    differentiable in ``mask`` and in the x and y columns of ``scan_pc`` (its other columns and the fake (0, 0) rows get 0);
    the azimuths are constants."""
    return _extract_weights_polar_stats(mask, scan_pc, azimuths, radar_resolution, interpolate_crossover, fix_wobble)[0]


def polar_target_from_pts(pc, azimuths, radar_resolution, polar_pixel_shape=(400, 3360)):
    """The map-point BCE target in a polar mask's own geometry:
    ``radar_cartesian_to_polar(extract_bev_from_pts(pc).double(), azimuths, radar_resolution, polar_pixel_shape=...)`` as
    fp32 -- the reference's 640 x 640 raster of the points resampled onto the (A,R) grid, a soft target in [0, 1].  The
    reference has no such target (its polar network cannot form the map-point loss); composing the two pinned operators is
    this build's choice.  (B,M,>=2) + (B,A) -> (B,A,R) fp32, no gradient."""
    with torch.no_grad():
        bev = extract_bev_from_pts(pc)
        return radar_cartesian_to_polar(bev.double(), azimuths, radar_resolution, polar_pixel_shape=polar_pixel_shape).float()


# ----------------------------------------------------------------------------- R10
def extract_bev_from_pts(pc, cart_pixel_width=640):
    """radar_utils.py:142-165.  (B,M,>=2) -> (B,W,W) binary image."""
    dev = _hip_device(pc)
    p = _lib.dev_f32(pc, dev)
    B, M, cols = p.shape
    W = int(cart_pixel_width)
    bev = torch.empty(B, W, W, dtype=torch.float32, device=dev)
    _lib.check(_lib.lib().mmk_bev_raster(_lib.ptr(p), B, M, cols, W, 0.2384, _lib.ptr(bev), _lib.stream_ptr(dev)))
    return _back(bev.to(pc.dtype) if pc.dtype.is_floating_point else bev, pc)
