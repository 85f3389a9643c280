"""The SE(3) pose terms (pose_loss="se3", csrc/mmk_loss.hip: mmk_pose_loss_se3_fwd / _bwd, mmk_val_metric_se3) on the GPU against
the fp64 PyTorch expression on the same fp32 inputs: values, gradients, exact zeros, determinism, argument errors, the untouched
planar default, and one training step end to end.  Cases and references: pose_cases.py.

Tolerances: rtol 1e-6 (gradients: atol 1e-9 beside it), the values test_gpu_losses.py uses for the planar kernels against PyTorch.
The kernels evaluate in fp64 and round once to fp32 (2^-24 = 6e-8 relative), which leaves more than a decade of margin.

Row 3 of grad_T: xi's last row is read by neither term, so G's row 3 and with it row 3 of grad_T = G T_gt^-T is zero in both
forms (fp64 autograd gives the same zeros, pose_cases.reference).  What the SE(3) terms add over the planar ones is row 2."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

from mm_masking_amd import _lib, synthetic
from mm_masking_amd import train_icp_weights as trn

import pose_cases as pc
import support
from support import DEV

pytestmark = pytest.mark.gpu
FORMS = [False, True]                            # with_gt: T_gt None (the gt_eye form) / given
_LW = {"icp_rot": 0.7, "icp_trans": 1.0, "fft": 0.0, "mask_pts": 0.0, "cfar": 0.0, "num_pts": 0.0}


def _dev_batch(B, with_gt):
    Tp, Tg = pc.batch(B)
    return Tp.to(DEV), (Tg.to(DEV) if with_gt else None)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _direct(name, T, Tg, n_out):
    """One ctypes call of a forward entry point."""
    out = torch.empty(n_out, dtype=torch.float32, device=DEV)
    _lib.check(getattr(_lib.lib(), name)(_lib.ptr(T), _lib.ptr(Tg), T.shape[0], _lib.ptr(out), _lib.stream_ptr(DEV)))
    return out


def _direct_bwd(T, Tg, g_rot, g_trans):
    gT = torch.full_like(T, float("nan"))
    g = [None if v is None else torch.tensor([v], dtype=torch.float32, device=DEV) for v in (g_rot, g_trans)]
    _lib.check(_lib.lib().mmk_pose_loss_se3_bwd(_lib.ptr(T), _lib.ptr(Tg), T.shape[0], _lib.ptr(g[0]), _lib.ptr(g[1]), _lib.ptr(gT),
                                                _lib.stream_ptr(DEV)))
    return gT


@pytest.mark.parametrize("with_gt", FORMS)
@pytest.mark.parametrize("B", pc.BATCH_SIZES)
def test_forward_and_metric_match_fp64(B, with_gt):
    T, Tg = _dev_batch(B, with_gt)
    ref = pc.reference(B, with_gt)
    rot, trans = trn._PoseLossSe3Fn.apply(T) if Tg is None else trn._PoseLossSe3Fn.apply(T, Tg)
    got2 = np.array([rot.item(), trans.item()])
    with torch.no_grad():
        got3 = trn.eval_validation_loss(T, Tg, gt_eye=not with_gt, pose_loss="se3")
    print("B %d T_gt %s: |err| out2 %s out3 %s" % (B, with_gt, np.abs(got2 - ref["out2"]), np.abs(got3.cpu().numpy() - ref["out3"])))
    np.testing.assert_allclose(got2, ref["out2"], rtol=1e-6)
    np.testing.assert_allclose(got3.cpu().numpy(), ref["out3"], rtol=1e-6)
    # the same launches by hand, and again: identical bits
    for _ in range(2):
        assert torch.equal(_bits(_direct("mmk_pose_loss_se3_fwd", T, Tg, 2)), _bits(torch.stack((rot, trans))))
        assert torch.equal(_bits(_direct("mmk_val_metric_se3", T, Tg, 3)), _bits(got3))


@pytest.mark.parametrize("with_gt", FORMS)
@pytest.mark.parametrize("B", pc.BATCH_SIZES)
def test_grad_T_matches_fp64_autograd(B, with_gt):
    T, Tg = _dev_batch(B, with_gt)
    ref = pc.reference(B, with_gt)
    Ta = T.clone().requires_grad_(True)
    rot, trans = trn._PoseLossSe3Fn.apply(Ta) if Tg is None else trn._PoseLossSe3Fn.apply(Ta, Tg)
    (pc.G_ROT * rot + pc.G_TRANS * trans).backward()
    got = Ta.grad.cpu().numpy()
    print("B %d T_gt %s: max |grad - ref| %.3e (max |ref| %.3e)" % (B, with_gt, np.abs(got - ref["grad"]).max(), np.abs(ref["grad"]).max()))
    np.testing.assert_allclose(got, ref["grad"], rtol=1e-6, atol=1e-9)
    assert np.all(got[:, 3, :] == 0)
    for b in (i for i in range(B) if i % len(pc.NAMES) in pc.GENERIC_ROWS):
        assert np.abs(got[b, 2, :]).max() > 1e-3 / B, b                # row 2: what the planar terms leave at zero
    # each term alone: a None upstream gradient (autograd) and a NULL pointer (by hand)
    for term, key in ((0, "grad_rot"), (1, "grad_trans")):
        Tb = T.clone().requires_grad_(True)
        out = trn._PoseLossSe3Fn.apply(Tb) if Tg is None else trn._PoseLossSe3Fn.apply(Tb, Tg)
        out[term].backward()
        np.testing.assert_allclose(Tb.grad.cpu().numpy(), ref[key], rtol=1e-6, atol=1e-9)
        by_hand = _direct_bwd(T, Tg, *((1.0, None) if term == 0 else (None, 1.0)))
        assert torch.equal(_bits(by_hand), _bits(Tb.grad))
    # determinism
    assert torch.equal(_bits(_direct_bwd(T, Tg, pc.G_ROT, pc.G_TRANS)), _bits(_direct_bwd(T, Tg, pc.G_ROT, pc.G_TRANS)))
    assert torch.equal(_bits(_direct_bwd(T, Tg, pc.G_ROT, pc.G_TRANS)), _bits(Ta.grad))


@pytest.mark.parametrize("B", [5, 65])
def test_equal_poses_give_zero_bits(B):
    """T_pred == T_gt (a T_gt that is not orthonormal among them): outputs, metric and grad_T are all-zero bit patterns; so is the
    identity in the gt_eye form."""
    Tp, Tg = (t.to(DEV) for t in pc.equal_batch(B))
    eye = torch.eye(4, device=DEV).repeat(B, 1, 1)
    for T, G in ((Tp, Tg), (eye, None), (eye, eye.clone())):
        assert torch.count_nonzero(_bits(_direct("mmk_pose_loss_se3_fwd", T, G, 2))) == 0
        assert torch.count_nonzero(_bits(_direct("mmk_val_metric_se3", T, G, 3))) == 0
        assert torch.count_nonzero(_bits(_direct_bwd(T, G, pc.G_ROT, pc.G_TRANS))) == 0


def test_argument_errors():
    L = _lib.lib()
    T, _ = _dev_batch(5, False)
    out, null, st = torch.empty(16 * 5, dtype=torch.float32, device=DEV), ctypes.c_void_p(0), _lib.stream_ptr(DEV)
    err = _lib.CONSTANTS["MMK_ERR_ARG"]
    for B, Tp, o, word in ((0, _lib.ptr(T), _lib.ptr(out), b"B"), (-3, _lib.ptr(T), _lib.ptr(out), b"B"),
                           (5, null, _lib.ptr(out), b"T_pred"), (5, _lib.ptr(T), null, b"NULL")):
        assert L.mmk_pose_loss_se3_fwd(Tp, null, B, o, st) == err and word in L.mmk_last_error()
        assert L.mmk_val_metric_se3(Tp, null, B, o, st) == err and word in L.mmk_last_error()
        assert L.mmk_pose_loss_se3_bwd(Tp, null, B, null, null, o, st) == err and word in L.mmk_last_error()
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match="pose_loss"):
        trn.eval_training_loss(T, None, None, T, {}, {}, None, loss_weights=_LW, pose_loss="so3")
    with pytest.raises(ValueError, match="does not match"):
        trn._PoseLossSe3Fn.apply(T, T[:3])


@pytest.mark.parametrize("gt_eye", [True, False])
def test_default_is_untouched_and_se3_dispatches_to_the_kernel(gt_eye):
    """pose_loss="se2" and no keyword: the same bits of the loss, of its components and of T_pred.grad.  pose_loss="se3" through
    _pose_terms / eval_training_loss / eval_validation_loss: the bits of a direct call of the new entry points."""
    T, Tg = _dev_batch(65, True)
    runs = []
    for kw in ({}, {"pose_loss": "se2"}, {"pose_loss": "se3"}):
        Ta = T.clone().requires_grad_(True)
        loss, comp = trn.eval_training_loss(Ta, None, None, Tg, {}, {}, None, loss_weights=_LW, gt_eye=gt_eye, **kw)
        loss.backward()
        runs.append((loss.detach(), comp["rot"], comp["trans"], Ta.grad))
    for a, b in zip(runs[0], runs[1]):
        assert torch.equal(_bits(a), _bits(b))
    assert not torch.equal(runs[0][3], runs[2][3])
    assert torch.equal(_bits(trn.eval_validation_loss(T, Tg, gt_eye=gt_eye)), _bits(trn.eval_validation_loss(T, Tg, gt_eye=gt_eye, pose_loss="se2")))
    G = None if gt_eye else Tg
    rot, trans = trn._pose_terms(T, Tg, gt_eye, pose_loss="se3")
    direct = _direct("mmk_pose_loss_se3_fwd", T, G, 2)
    assert torch.equal(_bits(torch.stack((rot, trans))), _bits(direct))
    assert torch.equal(_bits(runs[2][2]), _bits(direct[1])) and torch.equal(_bits(runs[2][1]), _bits(0.7 * direct[0]))
    assert torch.equal(_bits(runs[2][3]), _bits(_direct_bwd(T, G, 0.7, 1.0)))
    assert torch.equal(_bits(trn.eval_validation_loss(T, Tg, gt_eye=gt_eye, pose_loss="se3")), _bits(_direct("mmk_val_metric_se3", T, G, 3)))
    # a T_pred that needs a gradient keeps the PyTorch expression in eval_validation_loss
    Ta = T.clone().requires_grad_(True)
    v = trn.eval_validation_loss(Ta, Tg, gt_eye=gt_eye, pose_loss="se3")
    assert v.requires_grad
    np.testing.assert_allclose(v.detach().cpu().numpy(), _direct("mmk_val_metric_se3", T, G, 3).cpu().numpy(), rtol=1e-5)


def test_train_step_se3_end_to_end():
    """One training step of the 6-DoF configuration (icp_dim = 3, point-to-plane) from 6-DoF initial poses with the SE(3) terms
    as the only loss, at the reduced sizes of test_gpu_policy.py (B = 2, sparse scenes, 3 072-row maps, 2 048 scan rows): the
    returned loss is the PyTorch expression on the step's own T_pred, and every parameter gets a finite gradient."""
    raw = synthetic.make_batch([0, 1], device=DEV, m_valid=3000, m_pad=3072, density="sparse", dim=3, z_std=0.5, tilt_std=0.1)
    assert float(raw["T_init"][:, 2, 3].abs().min()) > 0
    model = support.policy(DEV, 3, train=True, icp_dim=3, icp_type="pt2pl")
    params = support.policy_params(DEV, icp_dim=3, icp_type="pt2pl")
    batch = trn.prepare_batch(raw, params, max_loc_pts=2048)
    opt = trn.make_optimizer(model, params)
    lw = dict(trn.loss_weights_from(params), mask_pts=0.0)
    seen = []
    hook = model.register_forward_hook(lambda mod, args, out: seen.append(out[0].detach().clone()))
    loss, comp = trn.train_step(model, batch, opt, lw, DEV, pose_loss="se3")
    hook.remove()
    assert len(seen) == 1 and seen[0].shape == (2, 4, 4)
    rot, trans, _ = pc.expression(seen[0].cpu(), None)
    print("loss %.9g, expression %.9g (rot %.9g, trans %.9g)" % (loss.item(), (rot + trans).item(), rot.item(), trans.item()))
    np.testing.assert_allclose(loss.item(), (rot + trans).item(), rtol=1e-6)
    np.testing.assert_allclose([comp["rot"].item(), comp["trans"].item()], [rot.item(), trans.item()], rtol=1e-6)
    grads = [p.grad for p in model.parameters()]
    assert all(g is not None and bool(torch.isfinite(g).all()) for g in grads)
    assert any(float(g.abs().max()) > 0 for g in grads)
    importlib.import_module("mm_masking_amd.dICP.ICP").check_errors(wait=True)
