"""``dICP.ICP.ICP`` — batched differentiable ICP, MI355X implementation.

Keeps the call contract the reference relies on
(mm_masking/icp_weight_policy.py:54-55,281-288; mm_masking/icp_weight_dataset.py:59-61):

    ICP(icp_type='pt2pt'|'pt2pl', config_path=<yaml>, differentiable=True|False,
        max_iterations=int, tolerance=float)
    .target_pad_val
    .icp(source (B,N,3), target (B,M,6|3), T_init=(B,4,4), weight=(B,N),
         trim_dist=5.0, loss_fn={"name": "cauchy"|"huber"|"geman_mcclure"|"welsch", "metric": k}, dim=2|3)
        -> {"T": (B,4,4)}

``geman_mcclure`` (rho = c c, c = 1 / (1 + r2 / k^2)) and ``welsch`` (rho = exp(-(r2 / k^2))) are absent upstream: the two
strongly redescending kernels.  They go through every path Cauchy and Huber have, and their metric
may be a number or a tensor like Cauchy's (below).

pt2pl takes its normals from the target's columns 3..5; with ``parameters.target_normals:
estimate`` in the YAML an xyz-only target gets them from ``normals.estimate_normals`` per call.

The arithmetic (nearest neighbour, trim + robust weights, Jacobian accumulation,
Gauss-Newton solve, SE(2)/SE(3) update, and the reverse sweep that yields
dL/dweight) runs in the HIP kernels of csrc/mmk_icp.hip through the C ABI
(include/mmk.h); this file only owns buffers and the autograd hook.  The spec
is DESIGN.md §3; upstream dICP's source is absent, so it is OUR spec — see
"parity unpinned" there.  ``T`` maps source -> target (p_t ~ T p_s) and is
iterated from ``T_init``.

Differentiable (``differentiable=True``, grad enabled) in ``weight``, ``T_init``,
``source`` and ``target`` (xyz and, for pt2pl, the normals): ``T`` requires grad
when any of them does, and each one that does gets its gradient in its own dtype
and on its own device.  As in autograd through the unrolled iterations, the
correspondences, the hard trim gate, the freeze decisions and the non-positive-definite
fallback are constants.  With ``parameters.trim: tanh`` in the YAML (or ``icp.trim = "tanh"``)
the gate is ``0.5 - 0.5 tanh(tanh_steepness (d - trim_dist))`` and is differentiated in
the points like every other factor of a point's weight.  Entries outside the arithmetic get exactly 0: source z for
dim 2, target columns dim..2, the normals for pt2pt (columns >= 3 + dim for pt2pl)
and targets that never were a correspondent.  The clouds' adjoints come from
``mmk_icp_backward_points``; without them the backward is ``mmk_icp_backward``.

The robust scale ``loss_fn["metric"]``, ``trim_dist`` and the instance's ``tanh_steepness`` may each be a number or a
tensor of shape ``()``, ``(1,)`` (one value for the batch) or ``(B,)`` (one per pair); any other shape is a ValueError
before the device is touched.  With numbers only, the call is the one it always was.  With a tensor among them the call
goes through ``mmk_icp_forward_hp`` / ``mmk_icp_backward_hp`` (DESIGN.md §3 I3'', I7''): the three values are put into one
device array (numbers are broadcast there), nothing is read back, and a call whose tensors hold the values of a number call
is bit-identical to it.  Each tensor that requires grad gets its gradient in its own shape, dtype and device -- a shared
value the sum over the pairs -- and ``T`` requires grad when one of them does.  The hard gate gives ``trim_dist`` and the
steepness exactly 0, no robust loss gives the metric exactly 0.  A tensor cannot be validated on the host without a
synchronisation: the kernels raise ``MMK_ICP_STATUS_BAD_HYPER`` for a value the call uses that is non-finite or out of
range (metric > 0 under a robust loss, trim_dist >= 0, steepness > 0 under the tanh gate), and the next ICP call, or
``check_errors()``, turns it into an MmkError.  Nothing here keeps a learned value in range, and ``tolerance`` and
``target_pad_val`` get no gradient.

Soft correspondences (``parameters.correspondence: softmin`` in the YAML, or ``icp.correspondence = "softmin"``; DESIGN.md §3
I2', I3''', I7'''): a differentiable call -- ``differentiable=True`` with grad enabled -- matches every source point to a
VIRTUAL target row, the soft-min over its ``softmin_k`` (2..8, default 4) nearest target rows with temperature
``softmin_temp`` (m^2, default 0.25): a_j = softmax_j(-(d_j - d_0) / temp), row = sum_j a_j row_j, for pt2pl the normal
columns too, which are NOT renormalised.  The backward differentiates the a_j in the points, so a gradient can tell a point
that it would be better served by the neighbour next to its correspondent; which k rows are the neighbours stays a constant
(the temperature's gradient: below).  The search of such a call is always the exact k-NN through the grid: ``nn_search``
is ignored there.  Any other call of the instance (``differentiable=False``, or under ``torch.no_grad()``) keeps nearest
correspondences, bit for bit -- upstream's split, as with the gate.  ``trim: tanh`` combines with it; a tensor
hyper-parameter does not (ValueError before the device is touched), and the target needs at least ``softmin_k`` rows.
``correspondence: nearest``, or the keys absent, is the call it always was.

``icp.softmin_temp`` may also be a floating-point tensor of shape ``()``, ``(1,)`` (one temperature for the batch) or
``(B,)`` (one per pair); any other shape, or an integer dtype, is a ValueError before the device is touched.  The call then
goes through ``mmk_icp_forward_soft_t`` / ``mmk_icp_backward_soft_t`` (DESIGN.md §3 I3⁗, I7⁗): the kernels read tau on the
device with the expression they always had, so a tensor that holds the fp32 value of a number call gives that call's bits.
A tensor that requires grad gets its gradient in its own shape, dtype and device -- a shared value the fp64 sum of the pairs'
rows, rounded once -- and ``T`` requires grad when it does; a differentiable call in which nothing requires grad runs the
state-less soft forward with the device tau.  A tensor is not validated on the host: a non-finite or <= 0 value raises
``MMK_ICP_STATUS_BAD_HYPER`` as the other device-resident values do, and nothing here keeps a learned temperature positive.
A call that is not differentiable keeps nearest correspondences and does not look at the tensor.  The refusals above hold
with a tensor temperature too.
"""
import ctypes
import os

import torch
import yaml

from .. import _lib
from .normals import with_normals

_DEFAULT_CFG = os.path.join(os.path.dirname(os.path.abspath(__file__)), "config", "dICP_config.yaml")

_ws_cache = {}


def _workspace(nbytes, device):
    """Scratch of the ICP kernels, one buffer per (device, stream): calls enqueued on different streams
    (e.g. micro-batches overlapped on side streams) must not share scratch."""
    key = (device.index, torch.cuda.current_stream(device).cuda_stream)
    buf = _ws_cache.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(int(nbytes), dtype=torch.uint8, device=device)
        _ws_cache[key] = buf
    return buf


def _state_buffers(p, device, soft=None):
    K, B, N = p.max_iter, p.B, p.N
    per_point = () if soft is None else (soft.k,)          # soft correspondences: k neighbours per point, in key order
    return {
        "idx": torch.empty((K if p.save_state else 1, B, N) + per_point, dtype=torch.int32, device=device),
        "T": torch.empty((K + 1, B, 16), dtype=torch.float32, device=device),
        "delta": torch.empty((K, B, 6), dtype=torch.float64, device=device),
        "A": torch.empty((K, B, 36), dtype=torch.float64, device=device),
        "active": torch.empty((K + 1, B), dtype=torch.int32, device=device),
    }


ICP_STATUS_UNARMED_KEY = _lib.CONSTANTS["MMK_ICP_STATUS_UNARMED_KEY"]
ICP_STATUS_BAD_HYPER = _lib.CONSTANTS["MMK_ICP_STATUS_BAD_HYPER"]


class _StatusWatch:
    """Device-side error flags of the ICP kernels, checked WITHOUT synchronising the step: every forward call enqueues a
    4-byte copy of its status word into a pinned host slot behind its kernels (mmk_icp_status) plus an event; the slots
    whose event has completed are examined at the next ICP call (and by ``check(wait=True)``).  A raised flag is an
    internal error of the library (a nearest-neighbour key that no search kernel wrote) and becomes an MmkError instead
    of a silently clamped correspondence."""

    def __init__(self):
        self.pending = []           # (event, pinned int32 tensor)
        self.free = []

    def watch(self, p, ws, dev):
        L = _lib.lib()
        slot = self.free.pop() if self.free else torch.zeros(1, dtype=torch.int32).pin_memory()
        _lib.check(L.mmk_icp_status(ctypes.byref(p), _lib.ptr(ws), ws.numel(), ctypes.c_void_p(slot.data_ptr()),
                                    _lib.stream_ptr(dev)))
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(dev))
        self.pending.append((ev, slot))

    def check(self, wait=False):
        keep = []
        bad = 0
        for ev, slot in self.pending:
            if wait:
                ev.synchronize()
            if ev.query():
                bad |= int(slot[0])
                self.free.append(slot)
            else:
                keep.append((ev, slot))
        self.pending = keep
        if bad & ICP_STATUS_UNARMED_KEY:
            raise _lib.MmkError("dICP: a source row reached the accumulation stage with a nearest-neighbour key that no search "
                                "kernel wrote (MMK_ICP_STATUS_UNARMED_KEY) -- internal error, the poses of that call are invalid")
        if bad & ICP_STATUS_BAD_HYPER:
            raise _lib.MmkError("dICP: a device-resident hyper-parameter of an ICP call (loss_fn['metric'], trim_dist, "
                                "tanh_steepness or softmin_temp given as a tensor) was non-finite or out of range: the metric "
                                "must be > 0, trim_dist >= 0, the steepness > 0, softmin_temp > 0 (MMK_ICP_STATUS_BAD_HYPER); "
                                "the poses of that call are what the arithmetic gave with it")
        if bad:
            raise _lib.MmkError("dICP: the ICP kernels raised status bits 0x%x" % bad)


_status = _StatusWatch()


def check_errors(wait=True):
    """Raise if any ICP call so far raised a device-side error flag (``wait``: first wait for the calls in flight)."""
    _status.check(wait=wait)


HYPER_NAMES = ("loss_fn['metric']", "trim_dist", "tanh_steepness")      # the columns of the device array `hyper`


def _hyper_sizes(values, B):
    """Validate the three values (number, or tensor of shape (), (1,) or (B,)) without touching the device.  Returns None
    when all are numbers, else whether the device array takes one row per pair."""
    per_pair, any_tensor = False, False
    for name, v in zip(HYPER_NAMES, values):
        if isinstance(v, torch.Tensor):
            any_tensor = True
            if tuple(v.shape) not in ((), (1,), (B,)):
                raise ValueError("%s must be a number or a tensor of shape (), (1,) or (B,) = (%d,) (got shape %s)"
                                 % (name, B, tuple(v.shape)))
            if not (v.is_floating_point()):
                raise ValueError("%s: a tensor must have a floating-point dtype (got %s)" % (name, v.dtype))
            per_pair = per_pair or (v.ndim == 1 and v.shape[0] == B and B > 1)
    return per_pair if any_tensor else None


def _temp_size(temp, B):
    """Validate a tensor ``softmin_temp`` (shape (), (1,) or (B,), floating point) without touching the device.  Returns
    whether the device array takes one value per pair."""
    if tuple(temp.shape) not in ((), (1,), (B,)):
        raise ValueError("softmin_temp must be a number or a tensor of shape (), (1,) or (B,) = (%d,) (got shape %s)"
                         % (B, tuple(temp.shape)))
    if not temp.is_floating_point():
        raise ValueError("softmin_temp: a tensor must have a floating-point dtype (got %s)" % (temp.dtype,))
    return temp.ndim == 1 and temp.shape[0] == B and B > 1


def _temp_array(temp, per_pair, B, dev):
    """(1 | B,) fp32 on the device; nothing is read back."""
    return temp.detach().to(device=dev, dtype=torch.float32).reshape(-1).expand(B if per_pair else 1).contiguous()


def _hyper_array(values, per_pair, B, dev):
    """(1 | B, 3) fp32 on the device: tensors moved / cast, numbers broadcast there; nothing is read back."""
    n = B if per_pair else 1
    cols = []
    for v in values:
        if isinstance(v, torch.Tensor):
            cols.append(v.detach().to(device=dev, dtype=torch.float32).reshape(-1).expand(n))
        else:
            cols.append(torch.full((n,), float(v), dtype=torch.float32, device=dev))
    return torch.stack(cols, dim=1).contiguous()


def _forward(p, src, tgt, weight, T_init, hyper=None, per_pair=False, soft=None, temp=None):
    """``temp``: the (1 | B,) device temperature of a soft call (``per_pair`` then is its stride), mmk_icp_forward_soft_t."""
    L = _lib.lib()
    dev = src.device
    _status.check()
    nbytes = L.mmk_icp_workspace_bytes(ctypes.byref(p)) if soft is None else L.mmk_icp_soft_workspace_bytes(ctypes.byref(p), ctypes.byref(soft))
    if nbytes == 0:
        raise _lib.MmkError("libmmk_hip: %s" % L.mmk_last_error().decode(errors="replace"))
    ws = _workspace(nbytes, dev)
    st = _state_buffers(p, dev, soft)
    T_out = torch.empty(p.B, 4, 4, dtype=torch.float32, device=dev)
    iters = ctypes.c_int(0)
    args = [ctypes.byref(p), _lib.ptr(src, torch.float32, "source"), _lib.ptr(tgt, torch.float32, "target"),
            _lib.ptr(weight, torch.float32, "weight"), _lib.ptr(T_init, torch.float32, "T_init"), _lib.ptr(T_out),
            _lib.ptr(st["idx"]), _lib.ptr(st["T"]), _lib.ptr(st["delta"]), _lib.ptr(st["A"]), _lib.ptr(st["active"])]
    entry = L.mmk_icp_forward
    if hyper is not None:
        entry = L.mmk_icp_forward_hp
        args += [_lib.ptr(hyper), 1 if per_pair else 0]
    elif soft is not None and temp is not None:
        entry = L.mmk_icp_forward_soft_t
        args += [ctypes.byref(soft), _lib.ptr(temp), 1 if per_pair else 0]
    elif soft is not None:
        entry = L.mmk_icp_forward_soft
        args += [ctypes.byref(soft)]
    _lib.check(entry(*args, _lib.ptr(ws), ws.numel(), ctypes.byref(iters), _lib.stream_ptr(dev)))
    _status.watch(p, ws, dev)
    return T_out, st, iters.value


def _backward(ctx, grad_T, hyper, per_pair, need_h, soft=None, temp=None):
    """The reverse sweep of the autograd functions -> (gw, gT0, gs, gt, gh); ``hyper`` None: a call with numbers only,
    ``need_h``: a hyper-parameter gradient is asked for.  mmk_icp_backward on the cached workspace when neither a cloud nor
    a hyper-parameter is involved; else mmk_icp_backward_points (no ``hyper``) or mmk_icp_backward_hp, whose scratch holds
    per-point rows and fixed-point sums for the target as well and is sized per call, not cached.  ``soft``: the call had
    soft correspondences -- mmk_icp_backward_soft, with or without the clouds; with ``temp``, the device temperature,
    mmk_icp_backward_soft_t, and gh is then (B,) = dL/dtau per pair when ``need_h``."""
    weight, src, tgt, idx, T_hist, delta, A, active = ctx.saved_tensors[:8]
    p = ctx.p
    L = _lib.lib()
    dev = src.device
    gT = grad_T.contiguous().float()
    gw = torch.empty(p.B, p.N, dtype=torch.float32, device=dev)
    gT0 = torch.empty(p.B, 4, 4, dtype=torch.float32, device=dev)
    need_src, need_tgt = ctx.needs_input_grad[2], ctx.needs_input_grad[3]
    state = [ctypes.byref(p)] + [_lib.ptr(t) for t in (src, tgt, weight, idx, T_hist, delta, A, active, gT, gw, gT0)]
    if hyper is None and soft is None and not (need_src or need_tgt):
        ws = _workspace(L.mmk_icp_workspace_bytes(ctypes.byref(p)), dev)
        _lib.check(L.mmk_icp_backward(*state, _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev)))
        return gw, gT0, None, None, None
    if soft is not None and temp is not None:
        entry, nbytes = L.mmk_icp_backward_soft_t, L.mmk_icp_backward_soft_t_workspace_bytes(
            state[0], ctypes.byref(soft), 1 if need_tgt else 0, 1 if need_h else 0)
    elif soft is not None:
        entry, nbytes = L.mmk_icp_backward_soft, L.mmk_icp_backward_soft_workspace_bytes(state[0], ctypes.byref(soft), 1 if need_tgt else 0)
    elif hyper is None:
        entry, nbytes = L.mmk_icp_backward_points, L.mmk_icp_backward_points_workspace_bytes(state[0], 1 if need_tgt else 0)
    else:
        entry, nbytes = L.mmk_icp_backward_hp, L.mmk_icp_backward_hp_workspace_bytes(state[0], 1 if need_tgt else 0, 1)
    ws = torch.empty(int(nbytes), dtype=torch.uint8, device=dev)
    gs = torch.empty(p.B, p.N, 3, dtype=torch.float32, device=dev) if need_src else None
    gt = torch.empty(p.B, p.M, p.tgt_cols, dtype=torch.float32, device=dev) if need_tgt else None
    gh = torch.empty((p.B,) if temp is not None else (p.B, 3), dtype=torch.float32, device=dev) if need_h else None
    extra = [] if hyper is None else [_lib.ptr(hyper), 1 if per_pair else 0, _lib.ptr(gh)]
    if soft is not None:
        extra = [ctypes.byref(soft)]
        if temp is not None:
            extra += [_lib.ptr(temp), 1 if per_pair else 0, _lib.ptr(gh)]
    _lib.check(entry(*state, _lib.ptr(gs), _lib.ptr(gt), *extra, _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev)))
    return gw, gT0, gs, gt, gh


class _IcpFunction(torch.autograd.Function):
    """Autograd hook: forward = K unrolled iterations in HIP, backward = the
    hand-derived reverse sweep (no autograd graph through the iterations)."""
    last_active = None

    @staticmethod
    def forward(ctx, weight, T_init, src, tgt, p):
        T_out, st, _ = _forward(p, src, tgt, weight, T_init)
        _IcpFunction.last_active = st["active"]      # (K+1,B): pairs still iterating (measurement: bench.py)
        ctx.p = p
        ctx.save_for_backward(weight, src, tgt, st["idx"], st["T"], st["delta"], st["A"], st["active"])
        return T_out

    @staticmethod
    def backward(ctx, grad_T):
        return _backward(ctx, grad_T, None, False, False)[:4] + (None,)


class _IcpSoftFunction(torch.autograd.Function):
    """_IcpFunction for a call with soft correspondences (mmk_icp_forward_soft / mmk_icp_backward_soft): the saved
    correspondences are (K,B,N,k)."""

    @staticmethod
    def forward(ctx, weight, T_init, src, tgt, p, soft):
        T_out, st, _ = _forward(p, src, tgt, weight, T_init, soft=soft)
        _IcpFunction.last_active = st["active"]
        ctx.p, ctx.soft = p, soft
        ctx.save_for_backward(weight, src, tgt, st["idx"], st["T"], st["delta"], st["A"], st["active"])
        return T_out

    @staticmethod
    def backward(ctx, grad_T):
        return _backward(ctx, grad_T, None, False, False, soft=ctx.soft)[:4] + (None, None)


class _IcpSoftTempFunction(torch.autograd.Function):
    """_IcpSoftFunction with the temperature on the device (mmk_icp_forward_soft_t / mmk_icp_backward_soft_t): ``tau`` is
    the tensor as given; when it requires grad it gets the pair sums of I7⁗ -- its own row each for a (B,) tensor, their
    fp64 sum, rounded once, for a shared one."""

    @staticmethod
    def forward(ctx, weight, T_init, src, tgt, tau, p, soft, per_pair):
        temp = _temp_array(tau, per_pair, p.B, src.device)
        T_out, st, _ = _forward(p, src, tgt, weight, T_init, per_pair=per_pair, soft=soft, temp=temp)
        _IcpFunction.last_active = st["active"]
        ctx.p, ctx.soft, ctx.per_pair = p, soft, per_pair
        ctx.meta = (tuple(tau.shape), tau.dtype, tau.device)
        ctx.save_for_backward(weight, src, tgt, st["idx"], st["T"], st["delta"], st["A"], st["active"], temp)
        return T_out

    @staticmethod
    def backward(ctx, grad_T):
        need_t = ctx.needs_input_grad[4]
        gw, gT0, gs, gt, gh = _backward(ctx, grad_T, None, ctx.per_pair, need_t, soft=ctx.soft, temp=ctx.saved_tensors[8])
        gtau = None
        if need_t:
            shape, dtype, device = ctx.meta
            g = gh if ctx.per_pair else gh.double().sum()       # a shared value: the sum over the pairs, rounded once
            gtau = g.to(device=device, dtype=dtype).reshape(shape)
        return gw, gT0, gs, gt, gtau, None, None, None


class _IcpHpFunction(torch.autograd.Function):
    """_IcpFunction for a call with device-resident hyper-parameters (mmk_icp_forward_hp / mmk_icp_backward_hp): `values` are
    the metric, trim_dist and the steepness as given (tensor or number); a tensor among them that requires grad gets the
    pair sums of I7'' -- its own row each for a (B,) tensor, their fp64 sum for a shared one."""

    @staticmethod
    def forward(ctx, weight, T_init, src, tgt, v_k, v_c, v_s, p, per_pair):
        values = (v_k, v_c, v_s)
        hyper = _hyper_array(values, per_pair, p.B, src.device)
        T_out, st, _ = _forward(p, src, tgt, weight, T_init, hyper, per_pair)
        _IcpFunction.last_active = st["active"]
        ctx.p, ctx.per_pair = p, per_pair
        ctx.meta = [(tuple(v.shape), v.dtype, v.device) if isinstance(v, torch.Tensor) else None for v in values]
        ctx.save_for_backward(weight, src, tgt, st["idx"], st["T"], st["delta"], st["A"], st["active"], hyper)
        return T_out

    @staticmethod
    def backward(ctx, grad_T):
        p = ctx.p
        need_h = ctx.needs_input_grad[4:7]
        gw, gT0, gs, gt, gh = _backward(ctx, grad_T, ctx.saved_tensors[8], ctx.per_pair, any(need_h))
        gv = [None, None, None]
        for c in range(3):
            if need_h[c]:
                shape, dtype, device = ctx.meta[c]
                g = gh[:, c]
                if not (len(shape) == 1 and shape[0] == p.B and ctx.per_pair):
                    g = g.double().sum()             # a shared value: the sum over the pairs, rounded once
                gv[c] = g.to(device=device, dtype=dtype).reshape(shape)
        return gw, gT0, gs, gt, gv[0], gv[1], gv[2], None, None


class ICP:
    NN_SEARCH_OVERRIDE = None      # tests / benchmarks: force "brute" or "grid" for every instance

    def __init__(self, icp_type="pt2pl", config_path=None, differentiable=True, max_iterations=100, tolerance=1e-12):
        if icp_type not in _lib.ICP_TYPES:
            raise ValueError("icp_type must be 'pt2pt' or 'pt2pl' (got %r)" % (icp_type,))
        self.icp_type = icp_type
        self.differentiable = bool(differentiable)
        self.max_iterations = int(max_iterations)
        self.tolerance = float(tolerance)
        # The reference's path is CWD-relative and the upstream YAML is absent:
        # fall back to the built-in defaults instead of raising.
        cfg = {}
        for path in (config_path, _DEFAULT_CFG):
            if path and os.path.isfile(path):
                with open(path, "r") as f:
                    cfg = (yaml.safe_load(f) or {}).get("dICP", {}) or {}
                break
        self.config_path = config_path
        self.target_pad_val = float(cfg.get("target_pad_val", 1000.0))
        self.check_every = int((cfg.get("parameters") or {}).get("check_every", 8))
        # "brute": the exhaustive LDS-tiled scan; "grid": exact search through a uniform grid
        # (identical correspondences, ~100x fewer distance evaluations)
        self.nn_search = ICP.NN_SEARCH_OVERRIDE or str((cfg.get("parameters") or {}).get("nn_search", "brute"))
        if self.nn_search not in _lib.NN_METHODS:
            raise ValueError("dICP config: nn_search must be 'brute' or 'grid' (got %r)" % (self.nn_search,))
        # pt2pl with an xyz-only target: "given" refuses it (the normals are the caller's), "estimate" computes them per
        # call with normals.estimate_normals (k = normals_k, the call's dim, viewpoint = origin, pad_val = target_pad_val)
        self.target_normals = str((cfg.get("parameters") or {}).get("target_normals", "given"))
        if self.target_normals not in ("given", "estimate"):
            raise ValueError("dICP config: target_normals must be 'given' or 'estimate' (got %r)" % (self.target_normals,))
        self.normals_k = int((cfg.get("parameters") or {}).get("normals_k", 16))
        if not 3 <= self.normals_k <= 32:
            raise ValueError("dICP config: normals_k must be in 3..32 (got %r)" % (self.normals_k,))
        # the trim gate: "hard" keep = d2 < trim_dist^2 (a constant of the backward), "tanh" the soft gate
        # keep = 0.5 - 0.5 tanh(tanh_steepness (d - trim_dist)), differentiated in the points (DESIGN.md §3 I3', I7')
        self.trim = str((cfg.get("parameters") or {}).get("trim", "hard"))
        self.tanh_steepness = float((cfg.get("parameters") or {}).get("tanh_steepness", 10.0))
        self._trim_steep()
        # the correspondences of a differentiable call: "nearest" the single nearest target row (a constant of the
        # backward), "softmin" the soft-min over the softmin_k nearest rows at temperature softmin_temp (DESIGN.md §3
        # I2', I3''', I7'''); every other call keeps "nearest"
        self.correspondence = str((cfg.get("parameters") or {}).get("correspondence", "nearest"))
        self.softmin_k = (cfg.get("parameters") or {}).get("softmin_k", 4)
        self.softmin_temp = (cfg.get("parameters") or {}).get("softmin_temp", 0.25)
        self._softmin()
        self.last_state = None
        self.last_iterations = None

    def _soft_gate(self):
        """Whether the instance's gate is the tanh one (attributes are assignable: validated at every use)."""
        if self.trim not in ("hard", "tanh"):
            raise ValueError("dICP config: trim must be 'hard' or 'tanh' (got %r)" % (self.trim,))
        return self.trim == "tanh"

    def _trim_steep(self):
        """mmk_icp_params.trim_steep of the instance's gate, validated like ``trim``."""
        soft = self._soft_gate()
        steep = float(self.tanh_steepness)
        if not (steep > 0.0 and steep != float("inf")):
            raise ValueError("dICP config: tanh_steepness must be a finite number > 0 (got %r)" % (self.tanh_steepness,))
        return steep if soft else 0.0

    def _softmin(self):
        """mmk_icp_soft of the instance's correspondences, or None for "nearest" (attributes are assignable: validated at
        every use)."""
        if self.correspondence not in ("nearest", "softmin"):
            raise ValueError("dICP config: correspondence must be 'nearest' or 'softmin' (got %r)" % (self.correspondence,))
        k, temp = self.softmin_k, self.softmin_temp
        if isinstance(k, bool) or not isinstance(k, int) or not 2 <= k <= 8:
            raise ValueError("dICP config: softmin_k must be an integer in 2..8 (got %r)" % (k,))
        if isinstance(temp, torch.Tensor):
            # shape and dtype are validated against the call's B (_temp_size), the values on the device (the status flag);
            # the struct carries a placeholder that passes its validation and is not read
            return _lib.IcpSoft(k=k, temp=1.0) if self.correspondence == "softmin" else None
        if isinstance(temp, bool) or not isinstance(temp, (int, float)) or not (0.0 < float(temp) < float("inf")):
            raise ValueError("dICP config: softmin_temp must be a finite number > 0 (got %r)" % (temp,))
        return _lib.IcpSoft(k=k, temp=float(temp)) if self.correspondence == "softmin" else None

    def _params(self, B, N, M, tgt_cols, dim, loss_fn, trim_dist, save_state, on_device=False):
        """``on_device``: the metric, trim_dist and the steepness travel in the device array of the _hp entries; the struct
        then carries placeholders for the first two and only the gate's MODE in trim_steep."""
        name = None if loss_fn is None else loss_fn.get("name")
        if name not in _lib.LOSSES:
            raise ValueError("unknown loss_fn name %r" % (name,))
        if on_device:
            loss_k, trim_dist = 1.0, 0.0
            if isinstance(self.tanh_steepness, torch.Tensor):       # (no host validation of a tensor: the device flag replaces it)
                steep = 1.0 if self._soft_gate() else 0.0
            else:
                steep = self._trim_steep()
        else:
            loss_k, steep = float(1.0 if loss_fn is None else loss_fn.get("metric", 1.0)), self._trim_steep()
        return _lib.IcpParams(B=B, N=N, M=M, tgt_cols=tgt_cols, dim=dim, icp_type=_lib.ICP_TYPES[self.icp_type],
                              loss=_lib.LOSSES[name], loss_k=loss_k,
                              trim_dist=float(trim_dist), tolerance=self.tolerance, max_iter=self.max_iterations,
                              save_state=1 if save_state else 0,
                              check_every=0 if save_state else self.check_every,
                              nn_method=_lib.NN_METHODS[self.nn_search], trim_steep=steep)

    def icp(self, source, target, T_init=None, weight=None, trim_dist=5.0, loss_fn=None, dim=3):
        if source.ndim != 3 or source.shape[-1] != 3:
            raise ValueError("source must be (B,N,3)")
        if target.ndim != 3 or target.shape[-1] not in (3, 6):
            raise ValueError("target must be (B,M,3) or (B,M,6)")
        estimate = self.icp_type == "pt2pl" and target.shape[-1] != 6 and self.target_normals == "estimate"
        if self.icp_type == "pt2pl" and target.shape[-1] != 6 and not estimate:
            raise ValueError("pt2pl needs target normals: target must be (B,M,6)")
        if dim not in (2, 3):
            raise ValueError("dim must be 2 or 3")
        values = (1.0 if loss_fn is None else loss_fn.get("metric", 1.0), trim_dist, self.tanh_steepness)
        per_pair = _hyper_sizes(values, source.shape[0])            # None: numbers only, the call it always was
        soft = self._softmin()
        if not (self.differentiable and torch.is_grad_enabled()):
            soft = None                                             # only a differentiable call has soft correspondences
        if soft is not None and per_pair is not None:
            raise ValueError("correspondence='softmin' does not combine with a tensor hyper-parameter (%s given as a tensor)"
                             % ", ".join(n for n, v in zip(HYPER_NAMES, values) if isinstance(v, torch.Tensor)))
        tau = self.softmin_temp if soft is not None and isinstance(self.softmin_temp, torch.Tensor) else None
        tau_per_pair = False if tau is None else _temp_size(tau, source.shape[0])
        if soft is not None and target.shape[1] < soft.k:
            raise ValueError("correspondence='softmin' needs a target of at least softmin_k = %d rows (got %d)"
                             % (soft.k, target.shape[1]))
        if source.is_cuda:
            dev = source.device
        elif torch.cuda.is_available():
            dev = torch.device("cuda", torch.cuda.current_device())
        else:
            raise _lib.MmkError("dICP.ICP needs an MI355X/HIP device: the ICP is a set of HIP kernels with no CPU path")
        out_device = source.device
        # not detached: autograd undoes the move / cast for the clouds' gradients
        src = source.to(device=dev, dtype=torch.float32).contiguous()
        tgt = target.to(device=dev, dtype=torch.float32).contiguous()
        if estimate:
            # constants, like the map itself: the target's gradient flows through xyz only
            tgt = with_normals(tgt, k=self.normals_k, dim=dim, pad_val=self.target_pad_val).contiguous()
        B, N, _ = src.shape
        M = tgt.shape[1]
        if T_init is None:
            T0 = torch.eye(4, dtype=torch.float32, device=dev).repeat(B, 1, 1)
        else:
            T0 = T_init.to(device=dev, dtype=torch.float32).contiguous()
        w = None
        if weight is not None:
            w = weight.to(device=dev, dtype=torch.float32).contiguous()
        need_grad = self.differentiable and torch.is_grad_enabled() and (
            (w is not None and w.requires_grad) or T0.requires_grad or src.requires_grad or tgt.requires_grad or
            any(isinstance(v, torch.Tensor) and v.requires_grad for v in values) or (tau is not None and tau.requires_grad))
        p = self._params(B, N, M, tgt.shape[-1], dim, loss_fn, trim_dist, save_state=need_grad, on_device=per_pair is not None)
        if soft is not None:
            p.nn_method = _lib.NN_METHODS["grid"]                   # the k-NN goes through the grid; nn_search is ignored
        if need_grad:
            if w is None:
                w = torch.ones(B, N, dtype=torch.float32, device=dev)
            if tau is not None:
                T = _IcpSoftTempFunction.apply(w, T0, src, tgt, tau, p, soft, tau_per_pair)
            elif soft is not None:
                T = _IcpSoftFunction.apply(w, T0, src, tgt, p, soft)
            elif per_pair is None:
                T = _IcpFunction.apply(w, T0, src, tgt, p)
            else:
                T = _IcpHpFunction.apply(w, T0, src, tgt, values[0], values[1], values[2], p, per_pair)
            self.last_iterations = p.max_iter
        else:
            with torch.no_grad():
                hyper = None if per_pair is None else _hyper_array(values, per_pair, B, dev)
                temp = None if tau is None else _temp_array(tau, tau_per_pair, B, dev)
                T, st, iters = _forward(p, src, tgt, None if w is None else w.detach(), T0.detach(), hyper,
                                        bool(per_pair) if tau is None else tau_per_pair, soft, temp)
            self.last_state = st
            self.last_iterations = iters
        return {"T": T if T.device == out_device else T.to(out_device)}
