"""Trainer-side pieces of the hot path — mirror of the step-level functions of the
reference driver ``mm_masking/train_icp_weights.py``:

  train_policy            :22-69     one pass of zero_grad -> forward -> loss -> backward -> step
  validate_policy         :71-177    inference path (no_grad, ICP_alg_inference)
  eval_training_loss      :179-253   rot + trans + optional BCE mask losses
  eval_validation_loss    :255-273
  generate_baseline       :275-344   override-mask baselines (U-Net bypassed)
  default_params          :354-410   the hard-coded ``params`` dict
  fit                     :486-596   the epoch loop (best_policy.pt / epoch_N.pt), plus resume

Neptune logging, figures and checkpoint upload (observability SaaS) are out of
scope.  What the reference's Dataset/DataLoader does per item on the CPU
(CFAR, polar -> Cartesian; icp_weight_dataset.py:182-200,336-352) is done here
per batch on the GPU by ``prepare_batch`` — the synthetic pipeline has no vtr3
point extractor, so the scan cloud comes from cfar_mask + extract_pc.
"""
import time

import torch

from . import _lib
from . import radar_utils as ru
from . import synthetic
from .icp_weight_policy import LearnICPWeightPolicy, _check_batch


def default_params(device=None):
    """The reference's params (train_icp_weights.py:354-410) with BASELINE.json's
    configuration of the ICP (pt2pl + Huber) as optional overrides."""
    if device is None:
        device = torch.device("cuda" if torch.cuda.is_available() else "cpu")
    return {
        "device": device, "float_type": torch.float32, "gt_eye": True, "pos_std": 2.0, "rot_std": 0.6,
        "z_std": 0.0, "tilt_std": 0.0, "pose_loss": "se2",
        "log_transform": False, "normalize": ["minmax"], "batch_size_train": 16, "batch_size_test": 32,
        "icp_type": "pt2pt", "learning_rate": 1e-4, "leaky": False, "dropout": 0.05, "batch_norm": False,
        "init_weights": True, "a_thresh": 1.0, "b_thresh": 0.09, "loss_icp_rot_weight": 1.0,
        "loss_icp_trans_weight": 1.0, "loss_fft_mask_weight": 0.0, "loss_map_pts_mask_weight": 1.0,
        "loss_cfar_mask_weight": 0.0, "num_pts_weight": 0.0, "optimizer": "adam", "icp_loss_only_iter": -1,
        "max_iter": 10, "network_input_type": "cartesian", "network_output_type": "cartesian",
        "binary_inference": False, "norm_weights": True, "fft_input": True, "cfar_input": False,
        "range_input": False, "num_epochs": 30,
    }


def loss_weights_from(params):
    """train_icp_weights.py:414-417."""
    return {"icp_rot": params["loss_icp_rot_weight"], "icp_trans": params["loss_icp_trans_weight"],
            "fft": params["loss_fft_mask_weight"], "mask_pts": params["loss_map_pts_mask_weight"],
            "cfar": params["loss_cfar_mask_weight"], "num_pts": params["num_pts_weight"]}


def prepare_batch(raw, params, max_loc_pts=5120, polar_res=0.0596):
    """GPU counterpart of ICPWeightDataset.__getitem__ (icp_weight_dataset.py:323-362)
    for synthetic input: GO-CFAR -> blob centres -> zero-padded scan cloud, and
    polar -> Cartesian for the FFT and CFAR images (kept polar for a polar network).  ``raw`` holds device tensors
    fft_polar (B,400,3360), azimuths (B,400), az_times (B,400), map_pc (B,M,6),
    T_init, T_gt.  Returns the reference's dict-of-dicts batch; with params["mask_target"] == "scan" its ``loc_data`` also
    carries fft_polar, azimuths and az_times (what the policy's scan mode reads), with params["polar_sampling"] the azimuths
    (what the polar sampler and the polar map-point target read).  With params["motion_comp"] ``raw`` also holds velocity
    (B,6): raw_pc stays the image-frame cloud, filtered_pc is that cloud de-skewed with the twist (radar_utils.deskew_pc), and
    loc_data carries velocity."""
    motion = bool(params.get("motion_comp", False))
    if motion and (raw.get("velocity") is None or raw.get("az_times") is None):
        raise ValueError("motion_comp needs raw['velocity'] (B,6) and raw['az_times'] (synthetic.make_pair with vel_std or "
                         "yawrate_std > 0)")
    fft = raw["fft_polar"]
    az = raw["azimuths"]
    cfar = ru.cfar_mask(fft, polar_res, a_thresh=params["a_thresh"], b_thresh=params["b_thresh"], diff=False)
    if motion:
        # the reference's split (icp_weight_dataset.py:331-332,377-381): raw_pc lies where the image shows it and samples the
        # mask, which is distorted like the image; filtered_pc is the motion-compensated cloud that goes to ICP
        seconds = ru.scan_times(raw["az_times"], params.get("motion_time_unit", 1e-6), params.get("motion_ref", "mid"))
        pc, _, t = ru.extract_pc_padded(cfar, polar_res, az, seconds, max_loc_pts, diff=False, return_times=True)
        filtered = ru.deskew_pc(pc, t, raw["velocity"])
    else:
        pc, _ = ru.extract_pc_padded(cfar, polar_res, az, raw["az_times"], max_loc_pts, diff=False)
        filtered = pc
    if params.get("network_input_type", "cartesian") == "cartesian":    # icp_weight_dataset.py:350-352
        fft_img, cfar_img = ru._polar_to_cart_pair(fft, cfar, az, polar_res)     # one pass, shared coordinates
    else:                                                               # polar network: images stay (400,3360)
        fft_img, cfar_img = fft, cfar
    loc_data = {"raw_pc": pc, "filtered_pc": filtered, "fft_data": fft_img, "fft_cfar": cfar_img, "timestamp": 0}
    if motion:
        loc_data["velocity"] = raw["velocity"]
    if params.get("mask_target") == "scan":
        loc_data.update({"fft_polar": fft, "azimuths": az, "az_times": raw["az_times"]})
    if params.get("polar_sampling"):
        loc_data["azimuths"] = az
    map_data = {"pc": raw["map_pc"], "timestamp": 0}
    T_data = {"T_ml_init": raw["T_init"], "T_ml_gt": raw["T_gt"]}
    return {"loc_data": loc_data, "map_data": map_data, "transforms": T_data}


_CONST_CACHE = {}


def _const(kind, device, dtype):
    """Read-only constants (a (1,) zero, the 4x4 identity) built once per device and dtype: the reference creates them
    afresh in every call (train_icp_weights.py:183-188,195), which costs a fill launch each per training step."""
    key = (kind, device, dtype)
    t = _CONST_CACHE.get(key)
    if t is None:
        t = torch.zeros(1, dtype=dtype, device=device) if kind == "zero" else torch.eye(4, dtype=dtype, device=device)
        _CONST_CACHE[key] = t
    return t


# ----------------------------------------------------------------------------- loss terms as single launches (HIP tensors)
def _on_hip_f32(*tensors):
    """What the loss kernels take: fp32 tensors on a HIP device (anything else keeps the PyTorch expression)."""
    return all(t.is_cuda and t.dtype == torch.float32 for t in tensors)


class _PoseLossFn(torch.autograd.Function):
    """(loss_rot, loss_trans) of train_icp_weights.py:192-200 in one launch, their gradient w.r.t. T_pred in another
    (csrc/mmk_loss.hip) -- through PyTorch the two terms and their backward were ~25 launches of 2-5 us.  ``T_gt=None`` is
    the gt_eye form.  Against a ground-truth pose (gt_eye=False) the device takes a fp64 4x4 inverse per pair instead of
    torch.inverse, which synchronises with the host, and ~15 launches of matmul / norm / mean; T_gt gets no gradient."""

    @staticmethod
    def forward(ctx, T_pred, T_gt=None):
        L = _lib.lib()
        T = T_pred.contiguous().float()
        saved = (T,) if T_gt is None else (T, _lib.dev_f32(T_gt, T.device))
        if T_gt is not None and saved[1].shape != T.shape:
            raise ValueError("T_gt %s does not match T_pred %s" % (tuple(saved[1].shape), tuple(T.shape)))
        out = torch.empty(2, dtype=torch.float32, device=T.device)
        fwd = L.mmk_pose_loss_fwd if T_gt is None else L.mmk_pose_loss_gt_fwd
        _lib.check(fwd(*map(_lib.ptr, saved), T.shape[0], _lib.ptr(out), _lib.stream_ptr(T.device)))
        ctx.save_for_backward(*saved)
        return out[0], out[1]

    @staticmethod
    def backward(ctx, g_rot, g_trans):
        L = _lib.lib()
        saved = ctx.saved_tensors
        T = saved[0]
        gT = torch.empty_like(T)
        grads = [None if g is None else g.contiguous().float() for g in (g_rot, g_trans)]
        bwd = L.mmk_pose_loss_bwd if len(saved) == 1 else L.mmk_pose_loss_gt_bwd
        _lib.check(bwd(*map(_lib.ptr, saved), T.shape[0], *map(_lib.ptr, grads), _lib.ptr(gT), _lib.stream_ptr(T.device)))
        return gT, None


_PoseLossGtFn = _PoseLossFn         # (T_pred, T_gt): the name its tests call


class _PoseLossSe3Fn(torch.autograd.Function):
    """(loss_rot, loss_trans) of pose_loss="se3" -- the batch means of the geodesic rotation angle and of the 3-D translation
    norm of xi = T_pred T_gt^-1 - I (_se3_terms) -- in one launch, their gradient w.r.t. T_pred in another (csrc/mmk_loss.hip).
    ``T_gt=None`` is the gt_eye form; T_gt gets no gradient.  A None incoming gradient is a NULL pointer (a zero weight)."""

    @staticmethod
    def forward(ctx, T_pred, T_gt=None):
        T = T_pred.contiguous().float()
        Tg = None if T_gt is None else _lib.dev_f32(T_gt, T.device)
        if Tg is not None and Tg.shape != T.shape:
            raise ValueError("T_gt %s does not match T_pred %s" % (tuple(Tg.shape), tuple(T.shape)))
        out = torch.empty(2, dtype=torch.float32, device=T.device)
        _lib.check(_lib.lib().mmk_pose_loss_se3_fwd(_lib.ptr(T), _lib.ptr(Tg), T.shape[0], _lib.ptr(out), _lib.stream_ptr(T.device)))
        ctx.save_for_backward(T, Tg)
        ctx.set_materialize_grads(False)            # a term that is not used arrives as None, not as a tensor of zeros
        return out[0], out[1]

    @staticmethod
    def backward(ctx, g_rot, g_trans):
        T, Tg = ctx.saved_tensors
        gT = torch.empty_like(T)
        grads = [None if g is None else g.contiguous().float() for g in (g_rot, g_trans)]
        _lib.check(_lib.lib().mmk_pose_loss_se3_bwd(_lib.ptr(T), _lib.ptr(Tg), T.shape[0], *map(_lib.ptr, grads), _lib.ptr(gT),
                                                    _lib.stream_ptr(T.device)))
        return gT, None


def _shape_mismatch(x, t):
    return ValueError("Using a target size (%s) that is different to the input size (%s) is deprecated. "
                      "Please ensure they have the same size." % (tuple(t.shape), tuple(x.shape)))


def fft_threshold_mask(fft_data):
    """torch.where(fft > 3 * mean_{H,W}(fft), 1, 0) per image of a fp32 (B,H,W) HIP tensor (train_icp_weights.py:204-206,
    312-316) in three launches (csrc/mmk_loss.hip)."""
    L = _lib.lib()
    f = fft_data.contiguous()
    B = f.shape[0]
    ws = torch.empty(int(L.mmk_fft_threshold_ws_bytes(B)), dtype=torch.uint8, device=f.device)
    out = torch.empty_like(f)
    _lib.check(L.mmk_fft_threshold_mask(_lib.ptr(f, torch.float32, "fft_data"), B, f.numel() // B, _lib.ptr(ws), ws.numel(),
                                        _lib.ptr(out), _lib.stream_ptr(f.device)))
    return out


class _BceMeanFn(torch.autograd.Function):
    """torch.nn.BCELoss()(mask, target) (mean reduction, logs clamped at -100) as one pass + an ordered final sum, and its
    gradient as one pass (csrc/mmk_loss.hip); deterministic.  (An input outside [0, 1] gives NaN here where torch raises.)
    ``from_fft``: ``target`` is the fft, and both passes compute the 0/1 target of each element from it and its image's
    threshold -- _bce_mean(mask, fft_threshold_mask(fft)) without the target tensor, the same bits as the two calls."""

    @staticmethod
    def forward(ctx, mask, target, from_fft=False):
        L = _lib.lib()
        x, t = mask.contiguous().float(), target.contiguous().float()
        if x.shape != t.shape:
            raise _shape_mismatch(x, t)
        if from_fft:
            B = t.shape[0]
            ws = torch.empty(int(L.mmk_fft_threshold_ws_bytes(B)), dtype=torch.uint8, device=x.device)
            thr = torch.empty(B, dtype=torch.float32, device=x.device)     # a tensor of its own: the backward keeps it
            out = torch.empty((), dtype=torch.float32, device=x.device)
            _lib.check(L.mmk_bce_fft_threshold_fwd(_lib.ptr(x), _lib.ptr(t), B, t.numel() // B, _lib.ptr(ws), ws.numel(),
                                                   _lib.ptr(thr), _lib.ptr(out), _lib.stream_ptr(x.device)))
        else:
            ws = _lib.workspace(int(L.mmk_bce_ws_bytes()), x.device, "loss")
            thr = None
            out = torch.empty((), dtype=torch.float32, device=x.device)
            _lib.check(L.mmk_bce_mean_fwd(_lib.ptr(x), _lib.ptr(t), x.numel(), _lib.ptr(ws), ws.numel(), _lib.ptr(out),
                                          _lib.stream_ptr(x.device)))
        ctx.save_for_backward(x, t, thr)
        return out

    @staticmethod
    def backward(ctx, g):
        L = _lib.lib()
        x, t, thr = ctx.saved_tensors
        gx = torch.empty_like(x)
        g = g.contiguous().float()
        if thr is None:
            _lib.check(L.mmk_bce_mean_bwd(_lib.ptr(x), _lib.ptr(t), x.numel(), _lib.ptr(g), _lib.ptr(gx), _lib.stream_ptr(x.device)))
        else:
            B = t.shape[0]
            _lib.check(L.mmk_bce_fft_threshold_bwd(_lib.ptr(x), _lib.ptr(t), B, t.numel() // B, _lib.ptr(thr), _lib.ptr(g),
                                                   _lib.ptr(gx), _lib.stream_ptr(x.device)))
        return gx, None, None


class _BceFftThresholdFn(_BceMeanFn):
    """_BceMeanFn(mask, fft_data, from_fft=True) under the name of the fft term."""

    @staticmethod
    def forward(ctx, mask, fft_data):
        return _BceMeanFn.forward(ctx, mask, fft_data, True)


def _bce_mean(mask, target):
    """mask_criterion(mask, target) of the reference (torch.nn.BCELoss, train_icp_weights.py:180): the fused kernels on a HIP
    device, PyTorch's own on the CPU (host-logic tests)."""
    if _on_hip_f32(mask):
        return _BceMeanFn.apply(mask, target)
    return torch.nn.BCELoss()(mask, target)


def _fft_target(fft_data):
    """The fft term's target and generate_baseline's override mask (train_icp_weights.py:204-206, 312-316)."""
    if _on_hip_f32(fft_data):
        return fft_threshold_mask(fft_data)
    mean_azimuth = torch.mean(fft_data, dim=(1, 2), keepdim=True)
    return torch.where(fft_data > 3.0 * mean_azimuth, torch.ones_like(fft_data), torch.zeros_like(fft_data))


def _map_pts_target(model, batch_scan, batch_map, device):
    """The map-point target of the BCE term and of generate_baseline's override mask: the reference's 640 x 640 raster
    (train_icp_weights.py:209,318), or, for a policy with params["polar_sampling"], that raster in the polar mask's own
    geometry (ru.polar_target_from_pts with the scan's azimuths)."""
    pc = batch_map["pc"].to(device)
    if not getattr(model, "polar_sampling", False):
        return ru.extract_bev_from_pts(pc)
    _check_batch("polar", batch_scan, ("azimuths",))
    return ru.polar_target_from_pts(pc, batch_scan["azimuths"], model.res, tuple(batch_scan["fft_data"].shape[1:]))


def _xi_wedge(T_pred, T_gt, gt_eye):
    """xi = T_pred T_gt^-1 - I of both loss functions (train_icp_weights.py:192-196, 256-260), T_gt = I with gt_eye."""
    eye = _const("eye", T_pred.device, T_pred.dtype)
    if gt_eye:
        return T_pred - eye
    return torch.matmul(T_pred, torch.inverse(T_gt)) - eye


POSE_LOSSES = ("se2", "se3")


def _check_pose_loss(pose_loss):
    if pose_loss not in POSE_LOSSES:
        raise ValueError("pose_loss must be one of %s, got %r" % (", ".join(map(repr, POSE_LOSSES)), pose_loss))


def _xi_wedge_se3(T_pred, T_gt, gt_eye):
    """xi = T_pred T_gt^-1 - I as the kernels form it, (T_pred - T_gt) T_gt^-1: exactly zero for T_pred = T_gt, where _xi_wedge's
    product leaves rounding noise -- harmless to the planar terms' values, but theta and r are norms, and the gradient of a norm
    at rounding noise is a unit vector of noise instead of the zero it has at zero."""
    if gt_eye:
        return T_pred - _const("eye", T_pred.device, T_pred.dtype)
    return torch.matmul(T_pred - T_gt, torch.inverse(T_gt))


def _se3_terms(xi):
    """(theta, r) per pair of pose_loss="se3" from xi (B,4,4): v = half the skew part of the rotation block (the axis times
    sin(theta) of a rotation), c = 1 + trace / 2 (its cos(theta)), theta = atan2(||v||, c) in [0, pi], the geodesic angle, and
    r = ||xi[0:3,3]||.  A yaw-only pose has theta = asin|T[1,0]|, so small planar errors keep the scale of the "se2" terms."""
    v = 0.5 * torch.stack((xi[:, 2, 1] - xi[:, 1, 2], xi[:, 0, 2] - xi[:, 2, 0], xi[:, 1, 0] - xi[:, 0, 1]), dim=1)
    s = torch.linalg.vector_norm(v, dim=1)
    c = 1 + 0.5 * (xi[:, 0, 0] + xi[:, 1, 1] + xi[:, 2, 2])
    return torch.atan2(s, c), torch.linalg.vector_norm(xi[:, 0:3, 3], dim=1)


def _pose_terms(T_pred, T_gt, gt_eye, pose_loss="se2"):
    """(loss_rot, loss_trans): one launch each way for fp32 HIP tensors (csrc/mmk_loss.hip; against T_gt without torch.inverse,
    so without a host synchronisation), the reference's expression otherwise.  ``pose_loss="se3"``: the batch means of
    _se3_terms, which see all six components of the error, instead of the reference's planar |xi[1,0]| and ||xi[0:2,3]||."""
    _check_pose_loss(pose_loss)
    if _on_hip_f32(T_pred) and (gt_eye or T_gt.dtype == torch.float32):
        fn = _PoseLossFn if pose_loss == "se2" else _PoseLossSe3Fn
        return fn.apply(T_pred) if gt_eye else fn.apply(T_pred, T_gt)
    if pose_loss == "se3":
        theta, r = _se3_terms(_xi_wedge_se3(T_pred, T_gt, gt_eye))
        return theta.mean(), r.mean()
    xi_wedge = _xi_wedge(T_pred, T_gt, gt_eye)
    xi_r = xi_wedge[:, 0:2, 3]
    xi_theta = xi_wedge[:, 1, 0].unsqueeze(-1)
    return torch.norm(xi_theta, dim=1).mean(), torch.norm(xi_r, dim=1).mean()


# (term, its key in loss_weights) in the reference's order of summation
_LOSS_TERMS = (("rot", "icp_rot"), ("trans", "icp_trans"), ("fft", "fft"), ("mask_pts", "mask_pts"), ("cfar", "cfar"),
               ("num_pts", "num_pts"))


def eval_training_loss(T_pred, mask, num_non0, batch_T_gt, batch_scan, batch_map, model, loss_weights=[],
                       icp_loss_only_iter=0, gt_eye=True, epoch=0, pose_loss="se2"):
    """train_icp_weights.py:179-253.  Same values and shapes as the reference's expression
    ``w_rot * loss_rot + ... + w_num * loss_num_pts`` (a term that is switched off is a (1,) zero there, so the sum has
    shape (1,) whenever one is); the switched-off terms are not multiplied and added on the GPU, though: they are a
    shared constant zero (x + 0 = x bit for bit), which takes ~20 two-microsecond launches out of a training step."""
    _check_pose_loss(pose_loss)
    mask_criterion = _bce_mean
    zero = _const("zero", T_pred.device, T_pred.dtype)
    terms = {}
    want_pose = loss_weights["icp_rot"] > 0.0 or loss_weights["icp_trans"] > 0.0
    if want_pose:
        terms["rot"], terms["trans"] = _pose_terms(T_pred, batch_T_gt, gt_eye, pose_loss)
    if icp_loss_only_iter <= 0 or (icp_loss_only_iter > 0 and epoch < icp_loss_only_iter) or \
            (loss_weights["icp_rot"] <= 0 and loss_weights["icp_trans"] <= 0):
        if loss_weights["fft"] > 0.0:
            fft_data = batch_scan["fft_data"].to(mask.device)
            if _on_hip_f32(mask, fft_data):
                terms["fft"] = _BceFftThresholdFn.apply(mask, fft_data)     # the target is never written
            else:
                terms["fft"] = mask_criterion(mask, _fft_target(fft_data))
        if loss_weights["cfar"] > 0.0:
            terms["cfar"] = mask_criterion(mask, batch_scan["fft_cfar"].to(mask.device))
        if loss_weights["mask_pts"] > 0.0:
            map_pts_mask = _map_pts_target(model, batch_scan, batch_map, mask.device)
            terms["mask_pts"] = mask_criterion(mask, map_pts_mask)
        if loss_weights["num_pts"] > 0.0:
            terms["num_pts"] = model.mean_all_pts - num_non0

    loss = None
    loss_components = {}
    for name, wkey in _LOSS_TERMS:
        if name not in terms:
            loss_components[name] = zero
            continue
        w = loss_weights[wkey]
        # (a weight of exactly 1 -- the reference's defaults for the pose and map-point terms -- is not multiplied on the GPU:
        # 1.0 * x = x bit for bit, and the product and its backward were two ~5 us launches per term)
        t = terms[name] if (isinstance(w, (int, float)) and float(w) == 1.0) else w * terms[name]
        loss_components[name] = t.detach()
        loss = t if loss is None else loss + t
    if loss is None:
        loss = zero.clone()
    elif len(terms) < len(_LOSS_TERMS) and loss.dim() == 0:     # a term is off: the reference's sum has its (1,) zero in it
        loss = loss.reshape(1)
    return loss, loss_components


def eval_validation_loss(T_pred, batch_T_gt, gt_eye=True, pose_loss="se2"):
    """train_icp_weights.py:255-273 -> [||(theta,x,y)||, |theta|, ||(x,y)||] batch means.  gt_eye=False on a HIP device:
    one launch (csrc/mmk_loss.hip) instead of torch.inverse, which synchronises with the host; the result carries no gradient,
    so a T_pred that needs one (the reference only calls this under no_grad) keeps the PyTorch expression.
    ``pose_loss="se3"``: [sqrt(theta^2 + r^2), theta, r] batch means of _se3_terms, one launch on a HIP device in both forms."""
    _check_pose_loss(pose_loss)
    if pose_loss == "se3":
        if _on_hip_f32(T_pred) and (gt_eye or batch_T_gt.dtype == torch.float32) and \
                not (torch.is_grad_enabled() and T_pred.requires_grad):
            T = T_pred.detach().contiguous()
            Tg = None if gt_eye else _lib.dev_f32(batch_T_gt, T.device)
            out = torch.empty(3, dtype=torch.float32, device=T.device)
            _lib.check(_lib.lib().mmk_val_metric_se3(_lib.ptr(T), _lib.ptr(Tg), T.shape[0], _lib.ptr(out), _lib.stream_ptr(T.device)))
            return out
        theta, r = _se3_terms(_xi_wedge_se3(T_pred, batch_T_gt, gt_eye))
        full = torch.linalg.vector_norm(torch.stack((theta, r), dim=1), dim=1)     # (a zero subgradient at theta = r = 0)
        return torch.hstack((full.mean(), theta.mean(), r.mean()))
    if not gt_eye and _on_hip_f32(T_pred) and batch_T_gt.dtype == torch.float32 and \
            not (torch.is_grad_enabled() and T_pred.requires_grad):
        T = T_pred.detach().contiguous()
        Tg = _lib.dev_f32(batch_T_gt, T.device)
        out = torch.empty(3, dtype=torch.float32, device=T.device)
        _lib.check(_lib.lib().mmk_val_metric(_lib.ptr(T), _lib.ptr(Tg), T.shape[0], _lib.ptr(out), _lib.stream_ptr(T.device)))
        return out
    xi_wedge = _xi_wedge(T_pred, batch_T_gt, gt_eye)
    xi_r = xi_wedge[:, 0:2, 3]
    xi_theta = xi_wedge[:, 1, 0].unsqueeze(-1)
    xi_stack = torch.cat((xi_theta, xi_r), dim=1)
    return torch.hstack((torch.norm(xi_stack, dim=1).mean(), torch.norm(xi_theta, dim=1).mean(),
                         torch.norm(xi_r, dim=1).mean()))


def _unpack(batch, device):
    """(batch_scan, batch_map, T_init, T_gt) of a batch of the reference's dict-of-dicts form, the poses on ``device``."""
    batch_T = batch["transforms"]
    batch_T_gt = batch_T["T_ml_gt"].to(device)
    return batch["loc_data"], batch["map_data"], batch_T["T_ml_init"].to(device), batch_T_gt


def train_step(model, batch, opt, loss_weights, device, gt_eye=True, epoch=None, icp_loss_only_iter=0,
               grad_sync=None, pose_loss="se2"):
    """Body of the reference's batch loop (train_icp_weights.py:31-58).  ``grad_sync``
    (optional callable) is where a data-parallel job all-reduces the gradients."""
    _check_pose_loss(pose_loss)
    # (not _unpack: the ground-truth pose of a host-resident batch is copied after the forward, as it always was)
    batch_scan, batch_map, batch_T = batch["loc_data"], batch["map_data"], batch["transforms"]
    batch_T_init = batch_T["T_ml_init"].to(device)
    if grad_sync is not None and hasattr(grad_sync, "zero_grad"):
        grad_sync.zero_grad()           # keeps the flat gradient buffer attached
    else:
        opt.zero_grad()
    T_pred, mask, num_non0 = model(batch_scan, batch_map, batch_T_init)
    batch_T_gt = batch_T["T_ml_gt"].to(device)
    loss, loss_comp = eval_training_loss(T_pred, mask, num_non0, batch_T_gt, batch_scan, batch_map, model,
                                         loss_weights=loss_weights, icp_loss_only_iter=icp_loss_only_iter,
                                         gt_eye=gt_eye, epoch=epoch, pose_loss=pose_loss)
    loss.backward()
    if grad_sync is not None:
        grad_sync()
    opt.step()
    return loss.detach(), loss_comp


def train_policy(model, iterator, opt, loss_weights=[], device="cpu", epoch=None, icp_loss_only_iter=0, gt_eye=True,
                 grad_sync=None, pose_loss="se2"):
    """train_icp_weights.py:22-69."""
    _check_pose_loss(pose_loss)
    model.train()
    loss_hist = 0.0
    loss_comp_hist = []
    n = 0
    for batch in iterator:
        loss, loss_comp = train_step(model, batch, opt, loss_weights, device, gt_eye=gt_eye, epoch=epoch,
                                     icp_loss_only_iter=icp_loss_only_iter, grad_sync=grad_sync, pose_loss=pose_loss)
        loss_hist += loss
        loss_comp_hist.append(loss_comp)
        n += 1
    mean_loss = loss_hist / n
    mean_loss_comp = {k: sum(d[k] for d in loss_comp_hist) / len(loss_comp_hist) for k in loss_comp_hist[0]}
    _check_device_errors(device)
    return mean_loss, mean_loss_comp


def _check_device_errors(device):
    """The ICP kernels report internal errors through a status word that is examined without synchronising the step (at the next
    ICP call: dICP/ICP.py).  At the end of a pass nothing follows, so wait for the calls in flight and raise here: a flagged
    call's poses must not reach a checkpoint or a reported metric unnoticed (one synchronisation per epoch)."""
    if torch.device(device).type == "cuda":
        import importlib
        icp_mod = importlib.import_module(__package__ + ".dICP.ICP")     # the module (the package re-exports the class under its name)
        icp_mod.check_errors(wait=True)


def validate_policy(model, iterator, gt_eye=True, device="cpu", binary=False, neptune_run=None, epoch=None, pose_loss="se2"):
    """train_icp_weights.py:71-177 (without the Neptune figures)."""
    _check_pose_loss(pose_loss)
    model.eval()
    val_acc = torch.zeros((1, 3), device=device)
    mean_num_pc, mean_w, max_w, min_w = 0.0, 0.0, 0.0, 1000.0
    n = 0
    with torch.no_grad():
        for batch in iterator:
            batch_scan, batch_map, batch_T_init, batch_T_gt = _unpack(batch, device)
            T_pred, mask, _ = model(batch_scan, batch_map, batch_T_init, binary=binary)
            mean_num_pc += model.mean_num_pts
            max_w = model.max_w if model.max_w > max_w else max_w
            min_w = model.min_w if model.min_w < min_w else min_w
            mean_w += model.mean_w
            val_acc += eval_validation_loss(T_pred, batch_T_gt, gt_eye=gt_eye, pose_loss=pose_loss)
            n += 1
    _check_device_errors(device)
    return val_acc / n, mean_num_pc / n, mean_w / n, max_w, min_w


def generate_baseline(model, iterator, baseline_type="train", device="cpu",
                      loss_weights={"icp": 1.0, "fft": 0.0, "mask_pts": 0.0, "cfar": 0.0}, binary=False, gt_eye=True,
                      pose_loss="se2"):
    """train_icp_weights.py:275-344: ICP with a fixed (non-learned) mask."""
    _check_pose_loss(pose_loss)
    model.train() if baseline_type == "train" else model.eval()
    loss_init_hist, loss_ones_hist = [], []
    with torch.no_grad():
        for batch in iterator:
            batch_scan, batch_map, batch_T_init, batch_T_gt = _unpack(batch, device)
            fft_data = batch_scan["fft_data"].to(device)
            if loss_weights.get("cfar", 0.0) > 0.0:
                ones_mask = batch_scan["fft_cfar"].to(device)
            elif loss_weights.get("fft", 0.0) > 0.0:
                ones_mask = _fft_target(fft_data)
            elif loss_weights.get("mask_pts", 0.0) > 0.0:
                ones_mask = _map_pts_target(model, batch_scan, batch_map, device)
            else:
                ones_mask = torch.ones_like(fft_data)
            T_pred_ones, mask_ones, num_non0 = model(batch_scan, batch_map, batch_T_init, binary=binary,
                                                     override_mask=ones_mask)
            if baseline_type == "train":
                li, _ = eval_training_loss(batch_T_init, mask_ones, num_non0, batch_T_gt, batch_scan, batch_map, model,
                                           loss_weights=loss_weights, gt_eye=gt_eye, pose_loss=pose_loss)
                lo, _ = eval_training_loss(T_pred_ones, mask_ones, num_non0, batch_T_gt, batch_scan, batch_map, model,
                                           loss_weights=loss_weights, gt_eye=gt_eye, pose_loss=pose_loss)
            else:
                li = eval_validation_loss(batch_T_init, batch_T_gt, gt_eye=gt_eye, pose_loss=pose_loss)[0]
                lo = eval_validation_loss(T_pred_ones, batch_T_gt, gt_eye=gt_eye, pose_loss=pose_loss)[0]
            loss_init_hist.append(float(li))
            loss_ones_hist.append(float(lo))
    _check_device_errors(device)
    return sum(loss_init_hist) / len(loss_init_hist), sum(loss_ones_hist) / len(loss_ones_hist)


def make_optimizer(policy, params):
    """train_icp_weights.py:462-465."""
    if params["optimizer"] == "adam":
        # the same update rule; on the GPU all 46 tensors in one launch instead of seven foreach passes
        fused = all(p.is_cuda for p in policy.parameters())
        return torch.optim.Adam(policy.parameters(), lr=params["learning_rate"], fused=fused)
    return torch.optim.SGD(policy.parameters(), lr=params["learning_rate"], nesterov=True, momentum=1.0)


# ----------------------------------------------------------------------------- epoch loop + resume
def save_checkpoint(path, policy, opt, epoch, best_norm):
    """Everything a run needs to continue where it stopped (absent upstream, which saves the
    state_dict only: train_icp_weights.py:534-537,577-578): parameters, optimizer state, the epoch
    that finished, the best validation norm so far and the policy's dropout-seed counter.  Tensors,
    numbers and plain containers only, so it loads with ``weights_only=True``."""
    torch.save({"model": policy.state_dict(), "optimizer": opt.state_dict(), "epoch": int(epoch),
                "best_norm": float(best_norm), "policy_step": int(getattr(policy, "_step", 0))}, path)


def load_checkpoint(path, policy, opt=None, map_location=None):
    """Restores what ``save_checkpoint`` wrote; a bare state_dict file (the reference's
    ``best_policy.pt`` / ``epoch_N.pt``) loads the parameters only.  -> (next epoch, best_norm)."""
    ck = torch.load(path, map_location=map_location, weights_only=True)
    if "model" not in ck:
        policy.load_state_dict(ck)
        return 0, None
    policy.load_state_dict(ck["model"])
    if opt is not None:
        opt.load_state_dict(ck["optimizer"])
    policy._step = int(ck.get("policy_step", 0))
    return int(ck["epoch"]) + 1, float(ck["best_norm"])


def fit(policy, training_iterator, validation_iterator, opt, params, checkpoint_dir, loss_weights=None,
        start_epoch=0, best_norm=None, grad_sync=None, is_main=True, log=print):
    """The reference's epoch loop (train_icp_weights.py:486-596) without Neptune: baselines, a
    validation before training, then per epoch train_policy -> validate_policy, ``best_policy.pt`` when
    the total validation norm improves (or at epoch 0), ``epoch_N.pt`` every epoch (both bare
    state_dicts, as upstream), and finally a validation of the best policy.  Additionally writes
    ``resume.pt`` (save_checkpoint) every epoch; pass ``start_epoch`` / ``best_norm`` from
    ``load_checkpoint`` to continue a run.  Returns a history dict.

    Multi-rank jobs: every rank calls fit() with iterators of the SAME length (baselines, validation and training
    forwards may each hold the global min-max collective); ``is_main`` only gates the files that are written."""
    import os
    dev = params["device"]
    lw = loss_weights if loss_weights is not None else loss_weights_from(params)
    pose_loss = params.get("pose_loss", "se2")
    _check_pose_loss(pose_loss)
    if is_main:
        os.makedirs(checkpoint_dir, exist_ok=True)
    best_path = os.path.join(checkpoint_dir, "best_policy.pt")
    hist = {"loss": [], "loss_comp": [], "acc": [], "epoch_train_time": [], "epoch_val_time": []}

    def validate(epoch=None):
        return _rank_mean(validate_policy(policy, validation_iterator, epoch=epoch, device=dev, binary=params["binary_inference"],
                                          gt_eye=params["gt_eye"], pose_loss=pose_loss)[0])
    if start_epoch == 0:
        hist["train_baseline"] = generate_baseline(policy, training_iterator, baseline_type="train", device=dev, binary=False,
                                                   loss_weights=lw, gt_eye=params["gt_eye"], pose_loss=pose_loss)
        hist["val_baseline"] = generate_baseline(policy, validation_iterator, baseline_type="val", device=dev,
                                                 binary=params["binary_inference"], gt_eye=params["gt_eye"],
                                                 pose_loss=pose_loss)
        avg_norm = validate(epoch=-1)
        best_norm = float(avg_norm[0, 0])
        log("Norm before training: %.6f" % best_norm)
    for epoch in range(start_epoch, params["num_epochs"]):
        tic = time.time()
        mean_loss, mean_loss_comp = train_policy(policy, training_iterator, opt, lw, device=dev, epoch=epoch,
                                                 icp_loss_only_iter=params["icp_loss_only_iter"], gt_eye=params["gt_eye"],
                                                 grad_sync=grad_sync, pose_loss=pose_loss)
        mean_loss = float(mean_loss)
        t_train = time.time() - tic
        tic = time.time()
        avg_norm = validate(epoch)
        t_val = time.time() - tic
        total = float(avg_norm[0, 0])
        if total < best_norm or epoch == 0:
            best_norm = total
            if is_main:
                torch.save(policy.state_dict(), best_path)
        if is_main:
            torch.save(policy.state_dict(), os.path.join(checkpoint_dir, "epoch_{}.pt".format(epoch)))
            save_checkpoint(os.path.join(checkpoint_dir, "resume.pt"), policy, opt, epoch, best_norm)
        hist["loss"].append(mean_loss)
        hist["loss_comp"].append({k: float(v) for k, v in mean_loss_comp.items()})
        hist["acc"].append([float(v) for v in avg_norm[0]])
        hist["epoch_train_time"].append(t_train)
        hist["epoch_val_time"].append(t_val)
        log("EPOCH %d  loss %.5f  norm %.5f  best %.5f  (train %.1f s, val %.1f s)" % (epoch, mean_loss, total, best_norm,
                                                                                      t_train, t_val))
    hist["best_norm"] = best_norm
    # Final validation of the best policy (train_icp_weights.py:577-596), on EVERY rank of a multi-rank job: a forward
    # may hold a collective (the global min-max normalisation), so a validation that only the main rank entered would
    # hang or pair with another rank's next collective.  The main rank reads best_policy.pt and its weights are
    # broadcast, so the ranks end the run with identical (best) parameters.
    from .ddp import dist, job_size
    multi = job_size() > 1
    have_best = is_main and os.path.exists(best_path)
    if multi:
        flag = torch.tensor([1.0 if have_best else 0.0], device=dev)
        dist.all_reduce(flag, op=dist.ReduceOp.MAX)
        have_best = bool(flag.item() > 0)
    if have_best:
        if is_main and os.path.exists(best_path):
            policy.load_state_dict(torch.load(best_path, map_location=dev, weights_only=True))
        if multi:
            src = _main_rank(is_main, dev)
            for t in policy.state_dict().values():
                dist.broadcast(t, src=src)
        hist["final_acc"] = [float(v) for v in validate()[0]]
    return hist


def _rank_mean(t):
    """Mean over the ranks of a data-parallel job (identity in a single process): each rank validates its own shard of the
    validation set, and the reference selects its best policy on the WHOLE set (train_icp_weights.py:534-537) -- with equal
    shard sizes the mean of the shard means.  Every rank then takes the same best-policy decisions."""
    from .ddp import dist, job_size
    if job_size() == 1:
        return t
    t = t.clone()
    dist.all_reduce(t, op=dist.ReduceOp.SUM)
    return t / job_size()


def _main_rank(is_main, dev):
    """The rank that passed is_main=True (the lowest one, should several have): found with one MIN all-reduce."""
    from .ddp import dist, job_size
    t = torch.tensor([float(dist.get_rank()) if is_main else float(job_size())], device=dev)
    dist.all_reduce(t, op=dist.ReduceOp.MIN)
    return int(t.item())


class SyntheticIterator:
    """Stands in for DataLoader(ICPWeightDataset): yields ``n_batches`` prepared
    batches of ``batch_size`` pairs; pair indices are strided by world size so
    that ranks draw disjoint pairs of one seeded stream."""

    def __init__(self, params, batch_size, n_batches, rank=0, world_size=1, dataset_type="train", max_loc_pts=5120,
                 m_valid=20000, m_pad=20480, start=0, density="survey"):
        self.params, self.bs, self.nb, self.density = params, batch_size, n_batches, density
        self.rank, self.ws, self.kind = rank, world_size, dataset_type
        self.max_loc_pts, self.m_valid, self.m_pad, self.start = max_loc_pts, m_valid, m_pad, start

    def __len__(self):
        return self.nb

    def raw_batch(self, i):
        first = self.start + i * self.bs * self.ws
        idx = [first + self.rank + j * self.ws for j in range(self.bs)]
        return synthetic.make_batch(idx, device=self.params["device"], m_valid=self.m_valid, m_pad=self.m_pad,
                                    dataset_type=self.kind, pos_std=self.params["pos_std"],
                                    rot_std=self.params["rot_std"], density=self.density,
                                    z_std=self.params.get("z_std", 0.0), tilt_std=self.params.get("tilt_std", 0.0))

    def __iter__(self):
        for i in range(self.nb):
            yield prepare_batch(self.raw_batch(i), self.params, self.max_loc_pts)
