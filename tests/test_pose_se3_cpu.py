"""CPU-only: the SE(3) pose terms (pose_loss="se3") on their PyTorch-expression path -- the closed-form gradient the kernel
evaluates against fp64 autograd, the exact zeros, the gap to the planar terms on a pure roll -- and the host pieces of the 6-DoF
supervision: the pose_loss keyword, the 6-DoF initial poses of sample_T_init and synthetic.make_pair, the three entry points in
the header.  The cases are in pose_cases.py."""
import math
import re

import numpy as np
import pytest
import torch

from mm_masking_amd import _lib, synthetic
from mm_masking_amd import train_icp_weights as trn
from mm_masking_amd.icp_weight_dataset import sample_T_init

import pose_cases as pc
from support import header, n_args


@pytest.mark.parametrize("with_gt", [False, True])
def test_closed_form_gradient_matches_autograd(with_gt):
    """The closed form of include/mmk.h against fp64 autograd of the PyTorch expression on the whole pose set (both in fp64:
    1e-12 absolute), for both terms together and for each alone."""
    B = len(pc.NAMES)
    Tp, Tg = pc.batch(B)
    ref = pc.reference(B, with_gt)
    for g_rot, g_trans, key in ((pc.G_ROT, pc.G_TRANS, "grad"), (1.0, 0.0, "grad_rot"), (0.0, 1.0, "grad_trans")):
        got = pc.closed_form_grad(Tp, Tg if with_gt else None, g_rot, g_trans).numpy()
        print("max |closed form - autograd| (%s, T_gt %s): %.3e" % (key, with_gt, np.abs(got - ref[key]).max()))
        np.testing.assert_allclose(got, ref[key], rtol=0, atol=1e-12)
    assert np.all(ref["grad"][:, 3, :] == 0)                           # xi's last row is not read
    for b in pc.GENERIC_ROWS:
        assert np.abs(ref["grad"][b, 2, :]).max() > 1e-3               # ... and row 2, which the planar terms leave at zero, is


def test_exact_zeros():
    """At the identity the gradient is exactly zero (theta = atan2(0, 1), the norms' subgradient at zero), and T_pred == T_gt
    gives (0, 0) and a zero gradient exactly: xi is formed as (T_pred - T_gt) T_gt^-1."""
    eye = torch.eye(4).repeat(3, 1, 1).requires_grad_(True)
    rot, trans = trn._pose_terms(eye, None, True, pose_loss="se3")
    assert rot.item() == 0.0 and trans.item() == 0.0
    (pc.G_ROT * rot + pc.G_TRANS * trans).backward()
    assert torch.count_nonzero(eye.grad) == 0
    assert torch.count_nonzero(pc.closed_form_grad(eye.detach(), None, pc.G_ROT, pc.G_TRANS)) == 0
    Tp, Tg = pc.equal_batch(5)
    Tp.requires_grad_(True)
    rot, trans = trn._pose_terms(Tp, Tg, False, pose_loss="se3")
    assert rot.item() == 0.0 and trans.item() == 0.0
    (pc.G_ROT * rot + pc.G_TRANS * trans).backward()
    assert torch.count_nonzero(Tp.grad) == 0
    assert torch.count_nonzero(pc.closed_form_grad(Tp.detach(), Tg, pc.G_ROT, pc.G_TRANS)) == 0
    assert torch.count_nonzero(trn.eval_validation_loss(Tp.detach(), Tg, gt_eye=False, pose_loss="se3")) == 0
    v = trn.eval_validation_loss(torch.eye(4).repeat(3, 1, 1), None, gt_eye=True, pose_loss="se3")
    assert v.shape == (3,) and torch.count_nonzero(v) == 0


def test_roll_is_invisible_to_se2_and_seen_by_se3():
    """The gap this closes: a pose that is wrong by a pure roll of 0.1 rad has planar terms of exactly (0, 0) and an "se3"
    rotation term of 0.1; a yaw-only pose's theta is asin|T[1,0]|, so small planar errors keep the scale of loss_rot."""
    cases = {n: torch.from_numpy(T)[None] for n, T, _ in pc.pose_set()}
    roll, yaw = cases["roll"], cases["yaw"]
    for gt_eye in (True, False):
        Tg = torch.eye(4)[None]
        rot2, trans2 = trn._pose_terms(roll, Tg, gt_eye)
        assert rot2.item() == 0.0 and trans2.item() == 0.0
        rot3, trans3 = trn._pose_terms(roll, Tg, gt_eye, pose_loss="se3")
        assert abs(rot3.item() - 0.1) < 1e-6 and trans3.item() == 0.0
        assert trn.eval_validation_loss(roll, Tg, gt_eye=gt_eye)[0].item() == 0.0
        assert abs(trn.eval_validation_loss(roll, Tg, gt_eye=gt_eye, pose_loss="se3")[0].item() - 0.1) < 1e-6
        rot_yaw, _ = trn._pose_terms(yaw, Tg, gt_eye, pose_loss="se3")
        assert abs(rot_yaw.item() - math.asin(abs(yaw[0, 1, 0].item()))) < 1e-6
        assert abs(rot_yaw.item() - 0.4) < 1e-6


def test_metric_is_the_norm_of_both_terms():
    Tp, Tg = pc.batch(len(pc.NAMES))
    theta, r = trn._se3_terms(pc.xi_f64(Tp, Tg))
    v = trn.eval_validation_loss(Tp.double(), Tg.double(), gt_eye=False, pose_loss="se3")
    np.testing.assert_allclose(v.numpy(), [torch.sqrt(theta ** 2 + r ** 2).mean().item(), theta.mean().item(), r.mean().item()],
                               rtol=1e-14)
    assert 0.0 <= theta.min().item() and theta.max().item() <= math.pi
    assert abs(theta[pc.NAMES.index("near_pi")].item() - (math.pi - 1e-3)) < 1e-6


def test_unknown_pose_loss_raises():
    T = torch.eye(4)[None]
    lw = {"icp_rot": 1.0, "icp_trans": 1.0, "fft": 0.0, "mask_pts": 0.0, "cfar": 0.0, "num_pts": 0.0}
    with pytest.raises(ValueError, match="pose_loss"):
        trn.eval_training_loss(T, None, None, T, {}, {}, None, loss_weights=lw, pose_loss="se4")
    with pytest.raises(ValueError, match="pose_loss"):
        trn.eval_validation_loss(T, T, pose_loss="SE3")
    with pytest.raises(ValueError, match="pose_loss"):
        trn.train_step(None, None, None, lw, "cpu", pose_loss="planar")      # before the batch or the device is touched
    with pytest.raises(ValueError, match="pose_loss"):
        trn.train_policy(None, [], None, pose_loss="")
    for fn in (trn.validate_policy, trn.generate_baseline):
        with pytest.raises(ValueError, match="pose_loss"):
            fn(None, [], pose_loss="")
    p = trn.default_params(torch.device("cpu"))
    assert (p["pose_loss"], p["z_std"], p["tilt_std"]) == ("se2", 0.0, 0.0)
    loss, comp = trn.eval_training_loss(T, None, None, T, {}, {}, None, loss_weights=lw, pose_loss="se3")
    assert loss.item() == 0.0 and comp["rot"].item() == 0.0


@pytest.mark.parametrize("kind", ["train", "validation"])
def test_sample_T_init_at_zero_std_keeps_its_bits(kind):
    def draw(**kw):
        return sample_T_init(kind, 2.0, 0.6, generator=torch.Generator().manual_seed(5), np_rng=np.random.default_rng(5), **kw)
    assert torch.equal(draw(), draw(z_std=0.0, tilt_std=0.0))
    assert not torch.equal(draw(), draw(z_std=0.5, tilt_std=0.1))


def test_sample_T_init_six_dof():
    """z_std = 0.5, tilt_std = 0.1.  Training: the six uniforms the planar call draws, each scaled by its std (x, y and yaw as
    before).  Otherwise: z, roll, pitch drawn after phi, x, y, so those three are the planar call's."""
    g = torch.Generator().manual_seed(9)
    u = (2 * torch.rand((6, 1), generator=g.clone_state()) - 1).reshape(6)
    xi = (u * torch.tensor([2.0, 2.0, 0.5, 0.1, 0.1, 0.6])).double().numpy()
    planar = (u * torch.tensor([2.0, 2.0, 0.0, 0.0, 0.0, 0.6])).double().numpy()
    T = sample_T_init("train", 2.0, 0.6, generator=g.clone_state(), z_std=0.5, tilt_std=0.1)
    assert torch.equal(T, torch.tensor(synthetic.se3_exp(xi), dtype=torch.float32))
    assert torch.equal(sample_T_init("train", 2.0, 0.6, generator=g.clone_state()),
                       torch.tensor(synthetic.se3_exp(planar), dtype=torch.float32))
    assert np.array_equal(xi[[0, 1, 5]], planar[[0, 1, 5]])
    assert 0 < abs(xi[2]) <= 0.5 and np.all(np.abs(xi[3:5]) > 0) and np.all(np.abs(xi[3:5]) <= 0.1)
    assert T[2, 3] != 0 and T[2, 0] != 0 and T[2, 1] != 0
    # e_z tilts by at most ||(roll, pitch)|| <= sqrt(2) tilt_std
    assert math.hypot(T[2, 0].item(), T[2, 1].item()) <= math.sin(math.sqrt(2) * 0.1) + 1e-6

    r = np.random.default_rng(9)
    phi, x, y = r.normal(0.0, 0.6), r.normal(0.0, 2.0), r.normal(0.0, 2.0)
    z, roll, pitch = r.normal(0.0, 0.5), r.normal(0.0, 0.1), r.normal(0.0, 0.1)
    Tv = sample_T_init("validation", 2.0, 0.6, np_rng=np.random.default_rng(9), z_std=0.5, tilt_std=0.1)
    assert torch.equal(Tv, torch.tensor(synthetic.se3_exp([x, y, z, roll, pitch, phi]), dtype=torch.float32))
    assert torch.equal(sample_T_init("validation", 2.0, 0.6, np_rng=np.random.default_rng(9)),
                       torch.tensor(synthetic.se3_exp([x, y, 0, 0, 0, phi]), dtype=torch.float32))
    assert Tv[2, 3] != 0 and Tv[2, 0] != 0 and Tv[2, 1] != 0
    # only z: roll and pitch are not drawn
    r = np.random.default_rng(9)
    phi, x, y, z = r.normal(0.0, 0.6), r.normal(0.0, 2.0), r.normal(0.0, 2.0), r.normal(0.0, 0.5)
    assert torch.equal(sample_T_init("validation", 2.0, 0.6, np_rng=np.random.default_rng(9), z_std=0.5),
                       torch.tensor(synthetic.se3_exp([x, y, z, 0, 0, phi]), dtype=torch.float32))


@pytest.mark.parametrize("kind", ["train", "validation"])
def test_make_pair_six_dof_changes_T_init_only(kind):
    kw = dict(m_valid=500, m_pad=512, density="sparse", dim=3, dataset_type=kind)
    base = synthetic.make_pair(7, **kw)
    zero = synthetic.make_pair(7, z_std=0.0, tilt_std=0.0, **kw)
    six = synthetic.make_pair(7, z_std=0.5, tilt_std=0.1, **kw)
    assert set(base) == set(six) == set(zero)
    for k in base:
        assert np.array_equal(base[k], zero[k]), k
        assert np.array_equal(base[k], six[k]) == (k != "T_init"), k
    # T_init = Exp of the planar pair's (x, y, yaw), recovered from its T_init, and of (z, roll, pitch) from the stream of their own
    extra = np.random.default_rng([synthetic.BASE_SEED + 7, 6])
    extra = (extra.uniform(-1, 1, 3) if kind == "train" else extra.normal(0, 1, 3)) * np.array([0.5, 0.1, 0.1])
    T0 = base["T_init"].astype(np.float64)
    yaw = math.atan2(T0[1, 0], T0[0, 0])
    V = (synthetic.se3_exp([1, 0, 0, 0, 0, yaw])[:2, 3], synthetic.se3_exp([0, 1, 0, 0, 0, yaw])[:2, 3])
    x, y = np.linalg.solve(np.stack(V, axis=1), T0[:2, 3])
    want = synthetic.se3_exp([x, y, extra[0], extra[1], extra[2], yaw])
    np.testing.assert_allclose(six["T_init"], want, rtol=0, atol=2e-6)            # (fp32 storage of both poses)
    assert six["T_init"][2, 3] != 0 and six["T_init"][2, 0] != 0 and six["T_init"][2, 1] != 0
    if kind == "train":
        assert np.all(np.abs(extra) <= [0.5, 0.1, 0.1])
        assert math.hypot(six["T_init"][2, 0], six["T_init"][2, 1]) <= math.sin(math.sqrt(2) * 0.1) + 1e-6


def test_synthetic_iterator_forwards_the_stds():
    p = trn.default_params(torch.device("cpu"))
    p.update({"z_std": 0.5, "tilt_std": 0.1})
    it = trn.SyntheticIterator(p, 1, 1, m_valid=500, m_pad=512, density="sparse")
    want = synthetic.make_pair(0, m_valid=500, m_pad=512, density="sparse", z_std=0.5, tilt_std=0.1)["T_init"]
    assert np.array_equal(it.raw_batch(0)["T_init"][0].numpy(), want) and want[2, 3] != 0


def test_header_declares_the_se3_entry_points():
    """(Fails without the feature.)"""
    hdr = header()
    for name, n in (("mmk_pose_loss_se3_fwd", 5), ("mmk_pose_loss_se3_bwd", 7), ("mmk_val_metric_se3", 5)):
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert n_args(hdr, name) == n
        assert name in _lib.EXPORTED and len(_lib.EXPORTED[name][1]) == n
    assert _lib.CONSTANTS["MMK_VERSION"] == 502                          # additions only
