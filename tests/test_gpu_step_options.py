"""The non-default options of the training step on the hand-written kernels: pose terms against a ground-truth pose
(gt_eye=False) and the validation metric without torch.inverse, the fft-threshold mask loss without a target tensor, and
standardisation folded into the first layer (train_icp_weights.py:192-207,255-273, icp_weight_policy.py:156-159)."""
import os

import numpy as np
import pytest
import torch

from mm_masking_amd import _lib, synthetic, unet_hip
from mm_masking_amd import train_icp_weights as trn
from mm_masking_amd.icp_weight_policy import LearnICPWeightPolicy

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


# ----------------------------------------------------------------------------- pose terms against a ground-truth pose
def _poses(B, kind, g):
    """fp32 (B,4,4) ground-truth poses: random SE(2) / SE(3) ("se"), the same with an orthonormality defect ~1e-7 ("defect")."""
    T = torch.zeros(B, 4, 4, dtype=torch.float64)
    T[:, 3, 3] = 1.0
    for b in range(B):
        if b % 2 == 0:                                   # SE(2) in the plane, as the radar poses
            th = float(torch.rand(1, generator=g)) * 6.0 - 3.0
            T[b, :2, :2] = torch.tensor([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
            T[b, 2, 2] = 1.0
        else:
            q, r = torch.linalg.qr(torch.randn(3, 3, generator=g, dtype=torch.float64))
            q = q * torch.sign(torch.diagonal(r))
            if torch.det(q) < 0:
                q[:, 0] = -q[:, 0]
            T[b, :3, :3] = q
        T[b, :3, 3] = 20.0 * torch.randn(3, generator=g, dtype=torch.float64)
    if kind == "defect":
        T[:, :3, :3] += 1e-7 * torch.randn(B, 3, 3, generator=g, dtype=torch.float64)
    return T.float()


def _ref_pose_terms(Tp, Tg, w_rot, w_trans):
    """fp64 autograd of the reference's expression: xi = T_pred T_gt^-1 - I, torch.norm over xi[1,0] and (xi[0,3], xi[1,3])."""
    T = Tp.double().clone().requires_grad_(True)
    xi = torch.matmul(T, torch.inverse(Tg.double())) - torch.eye(4, dtype=torch.float64)
    rot = torch.norm(xi[:, 1, 0].unsqueeze(-1), dim=1).mean()
    trans = torch.norm(xi[:, 0:2, 3], dim=1).mean()
    (w_rot * rot + w_trans * trans).backward()
    return rot.item(), trans.item(), T.grad


@pytest.mark.parametrize("kind", ["se", "defect"])
@pytest.mark.parametrize("B", [1, 5, 32, 70])
def test_pose_terms_gt_match_fp64_autograd(B, kind):
    g = torch.Generator().manual_seed(1000 * B + len(kind))
    Tg = _poses(B, kind, g)
    Tp = Tg.clone()
    Tp[:, :3, :] += 0.05 * torch.randn(B, 3, 4, generator=g)
    same = B > 1                                         # pair 0 predicts the ground truth exactly: a zero gradient
    if same:
        Tp[0] = Tg[0]
    w_rot, w_trans = float(torch.rand(1, generator=g)) + 0.5, float(torch.rand(1, generator=g)) + 0.5
    rot_r, trans_r, g_r = _ref_pose_terms(Tp, Tg, w_rot, w_trans)
    Tpd = Tp.to(DEV).requires_grad_(True)
    rot, trans = trn._PoseLossGtFn.apply(Tpd, Tg.to(DEV))
    (w_rot * rot + w_trans * trans).backward()
    np.testing.assert_allclose([rot.item(), trans.item()], [rot_r, trans_r], rtol=1e-5)
    got = Tpd.grad.cpu().double()
    assert torch.all(got[:, 2:] == 0)
    k = 1 if same else 0
    if same:
        assert torch.all(got[0] == 0), got[0]
    np.testing.assert_allclose(got[k:].numpy(), g_r[k:].numpy(), rtol=1e-4, atol=1e-6 * float(g_r.abs().max()))
    # the validation metric of the same pairs (eval_validation_loss, :255-273)
    with torch.no_grad():
        v = trn.eval_validation_loss(Tp.to(DEV), Tg.to(DEV), gt_eye=False)
    xi = torch.matmul(Tp.double(), torch.inverse(Tg.double())) - torch.eye(4, dtype=torch.float64)
    xs = torch.stack((xi[:, 1, 0], xi[:, 0, 3], xi[:, 1, 3]), dim=1)
    want = [xs.norm(dim=1).mean().item(), xs[:, 0].abs().mean().item(), xs[:, 1:].norm(dim=1).mean().item()]
    np.testing.assert_allclose(v.cpu().numpy(), want, rtol=1e-5)


def test_pose_terms_gt_golden(golden_dir):
    """The reference's own values on tests/golden/losses.npz: the validation 3-vector with gt_eye=False, the pose terms and their
    gradient (fp64 autograd of the reference's expression on the golden poses)."""
    gz = np.load(os.path.join(golden_dir, "losses.npz"), allow_pickle=False)
    Tp, Tg = torch.from_numpy(gz["T_pred"]).float(), torch.from_numpy(gz["T_gt"]).float()
    out = torch.empty(3, dtype=torch.float32, device=DEV)
    Tpd, Tgd = Tp.to(DEV).contiguous(), Tg.to(DEV).contiguous()
    _lib.check(_lib.lib().mmk_val_metric(_lib.ptr(Tpd), _lib.ptr(Tgd), Tp.shape[0], _lib.ptr(out), _lib.stream_ptr(DEV)))
    np.testing.assert_allclose(out.cpu().numpy(), gz["val_gt"], rtol=1e-5)
    # T_gt = NULL is the identity: the gt_eye 3-vector
    _lib.check(_lib.lib().mmk_val_metric(_lib.ptr(Tpd), None, Tp.shape[0], _lib.ptr(out), _lib.stream_ptr(DEV)))
    np.testing.assert_allclose(out.cpu().numpy(), gz["val_eye"], rtol=1e-5)
    rot_r, trans_r, g_r = _ref_pose_terms(Tp, Tg, 0.7, 1.3)
    T = Tpd.clone().requires_grad_(True)
    rot, trans = trn._PoseLossGtFn.apply(T, Tgd)
    (0.7 * rot + 1.3 * trans).backward()
    np.testing.assert_allclose([rot.item(), trans.item()], [rot_r, trans_r], rtol=1e-5)
    np.testing.assert_allclose(T.grad.cpu().double().numpy(), g_r.numpy(), rtol=1e-4, atol=1e-7)


def test_gt_step_options_do_not_synchronise_with_the_host():
    """eval_training_loss(gt_eye=False) with the fft term, its backward and eval_validation_loss(gt_eye=False) enqueue work
    only: torch.inverse (a host synchronisation) is gone from all three."""
    g = torch.Generator().manual_seed(11)
    B, H, W = 4, 64, 96
    Tg = _poses(B, "se", g).to(DEV)
    Tp = (Tg + 0.01 * torch.randn(B, 4, 4, generator=g).to(DEV)).requires_grad_(True)
    mask = (torch.rand(B, H, W, generator=g) * 0.98 + 0.01).to(DEV).requires_grad_(True)
    fft = (-torch.log(torch.rand(B, H, W, generator=g))).to(DEV)
    lw = {"icp_rot": 1.0, "icp_trans": 2.0, "fft": 0.5, "mask_pts": 0.0, "cfar": 0.0, "num_pts": 0.0}
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        loss, comp = trn.eval_training_loss(Tp, mask, None, Tg, {"fft_data": fft}, None, None, loss_weights=lw, gt_eye=False)
        loss.backward()
        with torch.no_grad():
            v = trn.eval_validation_loss(Tp.detach(), Tg, gt_eye=False)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert torch.isfinite(loss).all() and torch.isfinite(v).all()
    assert Tp.grad is not None and mask.grad is not None and float(comp["fft"]) > 0


# ----------------------------------------------------------------------------- fft-threshold mask loss
def _fft_inputs():
    """Inputs whose threshold splits the image: synthetic radar (polar, full size), sparse exponential peaks, sizes that are
    not multiples of four (images that straddle the float4 groups), and one of 1 054 778 float4 groups and a tail of one
    element: more than one pass of the 2048 x 256 lanes of the BCE forward and of the 4096 x 256 of its backward and the mask."""
    g = torch.Generator().manual_seed(7)
    radar = synthetic.make_batch([3, 4], device=DEV, m_valid=3000, m_pad=3072, density="sparse")["fft_polar"]
    peaks = torch.rand(3, 640, 640, generator=g) ** 40
    odd = -torch.log(torch.rand(3, 33, 7, generator=g))
    odd2 = -torch.log(torch.rand(5, 37, 41, generator=g))
    big = -torch.log(torch.rand(3, 1201, 1171, generator=g))
    return {"radar": radar, "peaks": peaks.to(DEV), "odd": odd.to(DEV), "odd2": odd2.to(DEV), "big": big.to(DEV)}


@pytest.fixture(scope="module")
def fft_inputs():
    return _fft_inputs()


@pytest.mark.parametrize("name", ["radar", "peaks", "odd", "odd2", "big"])
def test_fft_threshold_mask_and_fused_bce(fft_inputs, name):
    fft = fft_inputs[name].contiguous()
    B = fft.shape[0]
    m = trn.fft_threshold_mask(fft)
    mean = torch.mean(fft, dim=(1, 2), keepdim=True)
    thr = 3.0 * mean
    want = torch.where(fft > thr, torch.ones_like(fft), torch.zeros_like(fft))
    frac = float(want.mean())
    assert 0.0 < frac < 0.5, frac                               # the threshold splits the image
    diff = m != want
    # the per-image mean is an ordered fp64 sum rounded to fp32, torch's a fp32 tree: they may differ by an ulp, which moves
    # the threshold by a few ulp -- only elements that close to it may be classified differently
    near = (fft - thr).abs() <= 2 * torch.finfo(torch.float32).eps * thr.abs()
    n_diff, n_near = int(diff.sum()), int(near.sum())
    print("%s: %d of %d elements above 3 x mean, %d differ from torch (%d within 2 ulp of the threshold)"
          % (name, int(want.sum()), want.numel(), n_diff, n_near))
    assert not bool((diff & ~near).any())
    assert set(torch.unique(m).tolist()) <= {0.0, 1.0}
    # the fused loss and gradient are the BCE on that mask, bit for bit
    g = torch.Generator().manual_seed(B)
    x = (torch.rand(fft.shape, generator=g) * 0.98 + 0.01).to(DEV)
    xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    la = trn._BceFftThresholdFn.apply(xa, fft)
    lb = trn._bce_mean(xb, m)
    assert la.shape == lb.shape == ()
    assert torch.equal(la.detach(), lb.detach()), (la.item(), lb.item())
    (0.37 * la).backward()
    (0.37 * lb).backward()
    assert torch.equal(xa.grad, xb.grad)
    # the same bits on a second evaluation
    xc = x.clone().requires_grad_(True)
    lc = trn._BceFftThresholdFn.apply(xc, fft)
    (0.37 * lc).backward()
    assert torch.equal(lc.detach(), la.detach()) and torch.equal(xc.grad, xa.grad)
    assert torch.equal(trn.fft_threshold_mask(fft), m)
    # and torch.nn.BCELoss on the torch target, where the two targets agree
    # (beyond one pass of the grid against the formula in fp64 on the CPU: BCELoss's own fp32 summation error is not measured)
    if n_diff == 0 and name == "big":
        xd, td = x.cpu().double(), want.cpu().double()
        ref = -(td * torch.log(xd).clamp(min=-100.0) + (1.0 - td) * torch.log(1.0 - xd).clamp(min=-100.0)).mean().item()
        np.testing.assert_allclose(la.item(), ref, rtol=2e-6)
    elif n_diff == 0:
        np.testing.assert_allclose(la.item(), torch.nn.BCELoss()(x, want).item(), rtol=2e-6)
    with pytest.raises(ValueError):
        trn._BceFftThresholdFn.apply(xa, fft[..., :-1].contiguous())


def test_fft_term_of_the_training_loss_uses_the_fused_kernels(fft_inputs):
    fft = fft_inputs["peaks"]
    x = (torch.rand(fft.shape, generator=torch.Generator().manual_seed(2)) * 0.98 + 0.01).to(DEV).requires_grad_(True)
    Tp = torch.eye(4, device=DEV).repeat(fft.shape[0], 1, 1)
    lw = {"icp_rot": 0.0, "icp_trans": 0.0, "fft": 0.25, "mask_pts": 0.0, "cfar": 0.0, "num_pts": 0.0}
    loss, comp = trn.eval_training_loss(Tp, x, None, Tp, {"fft_data": fft}, None, None, loss_weights=lw)
    assert loss.grad_fn is not None
    ref = 0.25 * trn._bce_mean(x.detach(), trn.fft_threshold_mask(fft))
    assert torch.equal(comp["fft"].reshape(()), ref)


# ----------------------------------------------------------------------------- standardisation
@pytest.mark.parametrize("C", [1, 2, 3, 4])
def test_channel_meanstd_matches_fp64(C):
    g = torch.Generator().manual_seed(C)
    shapes = [(2, C, 96, 128), (3, C, 33, 7)]
    for shp in shapes:
        x = torch.rand(shp, generator=g)
        for c in range(C):                                     # channels of different offsets and spreads
            x[:, c] = x[:, c] ** (c + 1) * (10.0 ** (c - 1)) + 3.0 * c
        pre = unet_hip.channel_meanstd(x.to(DEV).contiguous()).cpu().double()
        xd = x.double().transpose(0, 1).reshape(C, -1)
        np.testing.assert_allclose(pre[:, 0].numpy(), xd.mean(dim=1).numpy(), rtol=1e-6)
        np.testing.assert_allclose(pre[:, 1].numpy(), (1.0 / xd.std(dim=1, unbiased=True)).numpy(), rtol=1e-6)
    # a constant channel: 1 / std = inf, as the reference's division by zero
    x = torch.rand(2, 2, 40, 40, generator=g)
    x[:, 1] = 0.25
    pre = unet_hip.channel_meanstd(x.to(DEV)).cpu()
    assert pre[1, 0].item() == 0.25 and pre[1, 1].item() == float("inf")
    assert torch.isfinite(pre[0]).all()


def test_standardize_policy_folds_into_the_first_layer(monkeypatch):
    """normalize=["standardize"] on the HIP path: no normalised copy of the input (torch.std is never called) and the same
    mask and parameter gradients as the normalised input with pre=None, within the bf16 bounds of test_gpu_policy.py."""
    params = trn.default_params(DEV)
    params.update({"dropout": 0.0, "normalize": ["standardize"], "cfar_input": True, "range_input": True})
    torch.manual_seed(21)
    model = LearnICPWeightPolicy(params).to(DEV)
    model.train()
    g = torch.Generator().manual_seed(9)
    B, H = 2, 640
    fft = (torch.rand(B, H, H, generator=g) ** 6).to(DEV)
    cfar = (torch.rand(B, H, H, generator=g) > 0.95).float().to(DEV)
    scan = {"fft_data": fft, "fft_cfar": cfar, "raw_pc": torch.zeros(B, 4, 3, device=DEV)}
    gsel = torch.randn(B, H, H, generator=g).to(DEV)

    def no_std(*a, **k):
        raise AssertionError("torch.std called: the standardisation was not folded into the first layer")
    with monkeypatch.context() as mp:
        mp.setattr(torch, "std", no_std)
        a = model(scan, {"pc": torch.zeros(B, 4, 6, device=DEV)}, None, mask_only=True)
        (a * gsel).sum().backward()
    ga = [p.grad.detach().clone() for p in model.parameters()]
    model.zero_grad(set_to_none=True)
    raw_in = model._network_input(fft, cfar, normalize=False)
    net_in = model._normalize_channels(raw_in)
    b = unet_hip.unet_mask(model, net_in.contiguous().float(), True, model._step, norm=model.norm_weights, pre=None)
    (b * gsel).sum().backward()
    gb = [p.grad.detach() for p in model.parameters()]
    dm = (a - b).abs().max().item()
    num = sum(float(((x - y).double() ** 2).sum()) for x, y in zip(ga, gb))
    den = sum(float((y.double() ** 2).sum()) for y in gb)
    cos = torch.nn.functional.cosine_similarity(ga[0].flatten().double(), gb[0].flatten().double(), dim=0).item()
    print("standardize folded vs normalised copy: mask max |diff| %.2e, gradients relative L2 %.2e, encoder.0.0 cosine %.6f"
          % (dm, (num / den) ** 0.5, cos))
    assert dm < 5e-3
    assert (num / den) ** 0.5 < 0.059
    assert cos > 0.9


# ----------------------------------------------------------------------------- the whole step
def test_gt_fft_standardize_step_is_bit_reproducible():
    """A training step with gt_eye=False, the fft term on the polar network and standardisation, run twice from the same seed
    and state: the same loss and parameters, bit for bit (no float atomics on any of the new paths)."""
    B = 8
    params = trn.default_params(DEV)
    params.update({"icp_type": "pt2pl", "icp_loss_fn": {"name": "huber", "metric": 1.0}, "max_iter": 10, "dropout": 0.05,
                   "gt_eye": False, "loss_fft_mask_weight": 1.0, "loss_map_pts_mask_weight": 0.0,
                   "normalize": ["standardize"], "network_input_type": "polar", "network_output_type": "polar"})
    raw = synthetic.make_batch(list(range(4100, 4100 + B)), device=DEV)
    rng = np.random.default_rng(5)
    raw["T_gt"] = torch.from_numpy(np.stack([synthetic.se3_exp(np.r_[rng.normal(0, 0.3, 2), 0.0, 0.0, 0.0, rng.normal(0, 0.02)])
                                             for _ in range(B)]).astype(np.float32)).to(DEV)
    lw = trn.loss_weights_from(params)
    runs = []
    for rep in range(2):
        torch.manual_seed(77)
        model = LearnICPWeightPolicy(params).to(DEV)
        model.train()
        opt = trn.make_optimizer(model, params)
        out = []
        for step in range(2):
            batch = trn.prepare_batch(raw, params, max_loc_pts=5120)
            loss, comp = trn.train_step(model, batch, opt, lw, DEV, gt_eye=False)
            assert float(comp["fft"]) > 0 and float(comp["rot"]) > 0
            out.append((loss.clone(), [p.detach().clone() for p in model.parameters()]))
        runs.append(out)
    for step in range(2):
        (l0, p0), (l1, p1) = runs[0][step], runs[1][step]
        assert torch.isfinite(l0).all()
        assert torch.equal(l0, l1), (step, float(l0), float(l1))
        for a, b in zip(p0, p1):
            assert torch.equal(a, b), step
