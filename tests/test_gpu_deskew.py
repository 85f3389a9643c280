"""GPU: the motion compensation on the device -- the per-point times of mmk_extract_peaks_t against the numpy pairing of
tests/deskew_ref.py, mmk_deskew_points / mmk_deskew_points_bwd against the fp64 restatement there, the policy's and the batch
builder's motion_comp paths against the flag-off paths and the manual composition of the public operators, and the pose that
inference ICP finds for a moving scan with and without the compensation."""
import math

import numpy as np
import pytest
import torch

from mm_masking_amd import radar_utils as ru
from mm_masking_amd import synthetic
from mm_masking_amd import train_icp_weights as trn

import deskew_ref as dr
from radar_cases import A64, B64, RES, scene64  # noqa: F401  (scene64: a module fixture)
from support import DEV, dev, load_golden, policy

pytestmark = pytest.mark.gpu


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


# ----------------------------------------------------------------------------- 1. the per-point times
def _row_times(B, A, seed):
    """Distinct row times that are not monotone: a permutation of the multiples of 625 us, relative to mid-scan."""
    g = torch.Generator().manual_seed(seed)
    stamps = torch.stack([torch.randperm(A, generator=g) for _ in range(B)]).to(torch.float32) * 625.0
    return ru.scan_times(stamps)


def _time_cases(golden_dir):
    g = load_golden(golden_dir, "radar_peaks.npz")
    hard, soft, az = g["mask"].astype(np.float32), g["soft_mask"].astype(np.float32), g["az"]
    n_hard = max(g["pc0"].shape[0], g["pc1"].shape[0])
    rng = np.random.default_rng(3)
    ragged = np.zeros((3, 12, 300), dtype=np.float32)                  # blobs of 1..4 cells, a different number per item
    for b, nblob in enumerate((5, 40, 17)):
        for _ in range(nblob):
            a, c, w = rng.integers(0, 12), rng.integers(2, 290), rng.integers(1, 5)
            ragged[b, a, c:c + w] = 1.0
    az12 = np.sort(rng.uniform(0, 2 * math.pi, (3, 12)).astype(np.float32), axis=1)
    # a blob that reaches the last column leaves ONE marker (column R - 1 holds none): rows 2 and 7 of item 0 and row 4 of
    # item 1 have an odd number, so pairs straddle two rows, and item 1's last marker stays unpaired
    odd = np.zeros((2, 10, 64), dtype=np.float32)
    odd[0, 1, 5:8] = odd[0, 2, 10:12] = odd[0, 2, 60:64] = odd[0, 4, 3:9] = odd[0, 7, 58:64] = odd[0, 9, 20:22] = 1.0
    odd[1, 0, 30:33] = odd[1, 4, 61:64] = odd[1, 5, 7:9] = odd[1, 8, 40:44] = 1.0
    az10 = np.sort(rng.uniform(0, 2 * math.pi, (2, 10)).astype(np.float32), axis=1)
    return {"golden": (hard, az, False, 512), "golden_soft": (soft, az, True, 512), "truncated": (hard, az, False, n_hard // 2),
            "ragged": (ragged, az12, False, 64), "empty": (np.zeros((2, 8, 1400), dtype=np.float32), az, False, 16),
            "odd_rows": (odd, az10, False, 8), "odd_rows_truncated": (odd, az10, False, 2)}


@pytest.mark.parametrize("name", ["golden", "golden_soft", "truncated", "ragged", "empty", "odd_rows", "odd_rows_truncated"])
def test_point_times_equal_the_pairing(golden_dir, name):
    mask, az, diff, max_pts = _time_cases(golden_dir)[name]
    B, A, _ = mask.shape
    tm = _row_times(B, A, 17)
    assert all(len(set(row.tolist())) == A for row in tm) and (tm[:, 1:] < tm[:, :-1]).any()
    want_t, want_n = dr.point_times_ref(mask, tm.numpy(), RES, max_pts, diff=diff)
    m, azd, tmd = dev(mask), dev(az), tm.to(DEV)
    pc0, cnt0 = ru.extract_pc_padded(m, RES, azd, tmd, max_pts, diff=diff)
    pc, cnt, t = ru.extract_pc_padded(m, RES, azd, tmd, max_pts, diff=diff, return_times=True)
    print("TIMES %-18s counts %s of %d rows" % (name, cnt.cpu().tolist(), max_pts))
    assert cnt.cpu().tolist() == want_n.tolist()
    assert t.dtype == torch.float32 and t.shape == (B, max_pts) and np.array_equal(t.cpu().numpy().view(np.uint32), want_t.view(np.uint32))
    assert same_bits(pc, pc0) and torch.equal(cnt, cnt0)
    if name == "truncated":
        assert want_n.max() > max_pts
    if name == "empty":
        assert want_n.tolist() == [0, 0] and torch.count_nonzero(t).item() == 0
    if name.startswith("odd_rows"):
        assert want_n.tolist() == [5, 3]                                       # 10 and 7 markers
        if max_pts == 8:                                                       # item 0's third pair: rows 2 and 4
            assert t[0, 2].item() == ((tm[0, 2] + tm[0, 4]) / 2).item() and (t[0, 5:] == 0).all() and (t[1, 3:] == 0).all()
    # T_ab moves the points, not the times; under autograd the times are a constant
    T_ab = torch.eye(4, device=DEV).repeat(B, 1, 1)
    T_ab[:, 0, 3] = 1.5
    mg = m.clone().requires_grad_(True)
    pc2, cnt2, t2 = ru.extract_pc_padded(mg, RES, azd, tmd, max_pts, T_ab=T_ab, diff=diff, return_times=True)
    assert same_bits(t2, t) and not t2.requires_grad and not cnt2.requires_grad and pc2.requires_grad
    pc2.sum().backward()
    assert mg.grad is not None and torch.isfinite(mg.grad).all()


def test_times_need_the_azimuth_times():
    with pytest.raises(ValueError, match="return_times"):
        ru.extract_pc_padded(torch.zeros(1, 4, 16, device=DEV), RES, torch.zeros(1, 4, device=DEV), None, 8, return_times=True)


# ----------------------------------------------------------------------------- 2. the operator
FWD_REL = 2.0 ** -23          # one fp32 rounding of the fp64 value (2^-24), doubled for the device's fp64 sin / cos
TWIST_REL = 2.0 ** -22        # the same plus the fp64 sum's N 2^-53 sum|terms| (< 6e-9 of the result, test_deskew_cpu.py)


def _rel(got, ref, scale_axes=None):
    got, ref = got.detach().cpu().double().numpy(), np.asarray(ref, dtype=np.float64)
    scale = np.abs(ref).max() if scale_axes is None else np.abs(ref).max(axis=scale_axes, keepdims=True)
    return float((np.abs(got - ref) / scale).max())


@pytest.mark.parametrize("B, N", dr.SHAPES)
def test_operator_against_the_restatement(B, N):
    names = list(dr.TWISTS)
    for kind in dr.KINDS:
        pc, t, tw, G = dr.operator_case(B, N, kind)
        want, want_gp, want_gw, _ = dr.deskew_ref_grads(pc, t, tw, G)
        p, w = dev(pc).requires_grad_(True), dev(tw).requires_grad_(True)
        td, Gd = dev(t), dev(G)
        out = ru.deskew_pc(p, td, w)
        assert out.dtype == torch.float32 and out.shape == (B, N, 3)
        out.backward(Gd)
        r = (_rel(out, want), _rel(p.grad, want_gp), _rel(w.grad, want_gw, scale_axes=1))
        print("DESKEW B %2d N %4d %-7s out %.2e  grad_pc %.2e  grad_twist %.2e  (of 2^-23 = 1.19e-7, 2^-22 = 2.38e-7)" % ((B, N, kind) + r))
        assert r[0] <= FWD_REL and r[1] <= FWD_REL and r[2] <= TWIST_REL, (kind, r)
        # each gradient alone, the forward without a graph, and a second run: the same bits
        p1 = dev(pc).requires_grad_(True)
        o1 = ru.deskew_pc(p1, td, dev(tw))
        o1.backward(Gd)
        w2 = dev(tw).requires_grad_(True)
        o2 = ru.deskew_pc(dev(pc), td, w2)
        o2.backward(Gd)
        o3 = ru.deskew_pc(dev(pc), td, dev(tw))
        assert o3.grad_fn is None and same_bits(o1, out) and same_bits(o2, out) and same_bits(o3, out)
        assert same_bits(p1.grad, p.grad) and same_bits(w2.grad, w.grad)
        p4, w4 = dev(pc).requires_grad_(True), dev(tw).requires_grad_(True)
        ru.deskew_pc(p4, td, w4).backward(Gd)
        assert same_bits(p4.grad, p.grad) and same_bits(w4.grad, w.grad)
        # structure: padding rows, a zero twist, a zero time, a planar twist
        pad = (dev(pc) == 0).all(-1)
        assert int(pad.sum()) == (2 * B if N >= 8 else 0)
        assert (out[pad] == 0).all() and (p.grad[pad] == 0).all()
        item = [kind] * B if kind != "mixed" else [names[b % len(names)] for b in range(B)]
        for b, n in enumerate(item):
            if n == "zero":
                assert same_bits(out[b], dev(pc)[b])
            if n == "planar":
                assert (out[b, :, 2] == 0).all() and (p.grad[b, :, 2] == Gd[b, :, 2] * (~pad[b])).all()
        if N >= 8:
            assert (td[:, N // 4] == 0).all() and same_bits(out[:, N // 4], dev(pc)[:, N // 4])


def test_padding_rows_do_not_reach_the_twist():
    """A padding row's incoming gradient and time are never read into the sum: changing them leaves grad_twist's bits."""
    pc, t, tw, G = dr.operator_case(3, 257, "mixed")
    pad = (pc == 0).all(-1)
    G2, t2 = G.copy(), t.copy()
    G2[pad], t2[pad] = 1e6, 0.1
    grads = []
    for tt, GG in ((t, G), (t2, G2)):
        w = dev(tw).requires_grad_(True)
        ru.deskew_pc(dev(pc), dev(tt), w).backward(dev(GG))
        grads.append(w.grad)
    assert same_bits(*grads)


def test_operator_dtypes_and_devices():
    pc, t, tw, G = dr.operator_case(1, 65, "sixdof")
    p = torch.from_numpy(pc).double().requires_grad_(True)                   # a CPU fp64 cloud, an fp16-free device twist
    w = dev(tw).requires_grad_(True)
    out = ru.deskew_pc(p, torch.from_numpy(t), w)
    assert out.device.type == "cpu" and out.dtype == torch.float32
    out.backward(torch.from_numpy(G))
    assert p.grad.dtype == torch.float64 and p.grad.device.type == "cpu" and w.grad.dtype == torch.float32 and w.grad.is_cuda
    ref = ru.deskew_pc(dev(pc), dev(t), dev(tw))
    assert same_bits(out.to(DEV), ref)
    with torch.no_grad():
        assert ru.deskew_pc(dev(pc).requires_grad_(True), dev(t), dev(tw)).grad_fn is None


# ----------------------------------------------------------------------------- 3. the policy and the batch builder
def _moving(scan, velocity):
    stamps = (torch.arange(A64, dtype=torch.float32) * 7800.0)[None].repeat(B64, 1)       # a 0.25 s scan of 32 azimuths
    return dict(scan, az_times=stamps, velocity=velocity)


def _step(model, scan, mp, T0, G):
    model.train()
    model.zero_grad(set_to_none=True)
    T, mask, _ = model(scan, mp, T0)
    (T * G).sum().backward()
    return T.detach(), [q.grad.detach().clone() for q in model.parameters()]


def test_policy_flag_with_zero_velocity_equals_flag_off(scene64):
    scan, mp, T0, G = scene64
    batch = _moving(scan, torch.zeros(B64, 6, device=DEV))
    T_off, g_off = _step(policy(DEV, 3, dropout=0.0, mask_target="scan"), batch, mp, T0, G)
    T_on, g_on = _step(policy(DEV, 3, dropout=0.0, mask_target="scan", motion_comp=True), batch, mp, T0, G)
    assert same_bits(T_on, T_off) and any(g.abs().max() > 0 for g in g_off)
    assert len(g_on) == len(g_off) and all(torch.equal(a, b) for a, b in zip(g_on, g_off))


def test_policy_equals_the_manual_composition(scene64):
    scan, mp, T0, G = scene64
    twist = torch.tensor([[3.0, -1.0, 0.0, 0.0, 0.0, 0.2], [-2.0, 1.5, 0.0, 0.0, 0.0, -0.3]])
    vel = twist.to(DEV).requires_grad_(True)
    batch = _moving(scan, vel)
    model = policy(DEV, 3, dropout=0.0, mask_target="scan", motion_comp=True)
    T, through = _step(model, batch, mp, T0, G)
    v_through = vel.grad.detach().clone()
    T_plain, _ = _step(policy(DEV, 3, dropout=0.0, mask_target="scan"), batch, mp, T0, G)
    assert not torch.equal(T, T_plain)                                        # the compensation moves the pose

    model.zero_grad(set_to_none=True)
    vel2 = twist.to(DEV).requires_grad_(True)
    mask = model(batch, mp, T0, mask_only=True)
    masked = ru.mask_polar_scan(batch["fft_polar"], mask, batch["azimuths"], model.res)
    m = ru.cfar_mask(masked, model.res, a_thresh=model.a_thres, b_thresh=model.b_thres, diff=True)
    seconds = ru.scan_times(batch["az_times"].to(DEV), 1e-6, "mid")
    cloud, cnt, t = ru.extract_pc_padded(m, model.res, batch["azimuths"].to(DEV), seconds, max_pts=scan["raw_pc"].shape[1],
                                         diff=True, return_times=True)
    assert cnt.min() >= 8 and t.abs().max() > 0.1
    fixed = ru.deskew_pc(cloud, t, vel2)
    assert not torch.equal(fixed, cloud)
    T2 = model.icp(fixed, mp["pc"], T0, None)
    assert same_bits(T2, T)
    (T2 * G).sum().backward()
    manual = [q.grad.detach() for q in model.parameters()]
    assert any(g.abs().max() > 0 for g in through) and all(torch.equal(a, b) for a, b in zip(through, manual))
    assert v_through.abs().max() > 0 and torch.isfinite(v_through).all() and same_bits(vel2.grad, v_through)
    # the statistics keep reading the raw cloud; evaluation runs the inference ICP on the same de-skewed cloud
    model.eval()
    with torch.no_grad():
        Te, _, _ = model(batch, mp, T0)
        assert same_bits(Te, model.icp(fixed.detach(), mp["pc"], T0, None))


def test_policy_needs_velocity_and_times_on_the_device_too(scene64):
    scan, mp, T0, _ = scene64
    model = policy(DEV, 3, dropout=0.0, mask_target="scan", motion_comp=True)
    batch = _moving(scan, torch.zeros(B64, 6, device=DEV))
    for key in ("velocity", "az_times"):
        with pytest.raises(ValueError, match=key):
            model({k: v for k, v in batch.items() if k != key}, mp, T0)


# ----------------------------------------------------------------------------- 4. prepare_batch and the pose, end to end
# Of pairs 0..11, the two with the fastest drawn twists (14.8 and 12.8 m/s; yaw rates -0.08 and 0.21 rad/s) among those whose
# T_init lies within 0.15 rad of the truth (3, 8 and 9): from further away (pair 4: 0.50 rad) the inference ICP does not reach
# the pose even for the static scene, and the three errors would all be T_init's own.
PAIRS = [3, 9]


@pytest.fixture(scope="module")
def batches():
    params = trn.default_params(DEV)
    params.update({"icp_type": "pt2pl", "icp_loss_fn": {"name": "huber", "metric": 1.0}})
    moving = synthetic.make_batch(PAIRS, device=DEV, vel_std=12.0, yawrate_std=0.3)
    static = synthetic.make_batch(PAIRS, device=DEV)
    return params, moving, static


def test_prepare_batch_splits_raw_and_filtered(batches):
    params, moving, _ = batches
    plain = trn.prepare_batch(moving, params)["loc_data"]
    assert plain["raw_pc"] is plain["filtered_pc"] and "velocity" not in plain
    flagged = trn.prepare_batch(moving, dict(params, motion_comp=True))["loc_data"]
    assert same_bits(flagged["raw_pc"], plain["raw_pc"]) and same_bits(flagged["velocity"], moving["velocity"])
    assert not torch.equal(flagged["filtered_pc"], flagged["raw_pc"])
    real = ~(plain["raw_pc"] == 0).all(-1)
    shift = (flagged["filtered_pc"] - flagged["raw_pc"]).norm(dim=-1)
    assert (shift[~real] == 0).all() and 0.5 < shift[real].max() < 0.125 * 16 + 0.3 * 0.125 * 200
    assert "az_times" not in flagged and "az_times" in trn.prepare_batch(moving, dict(params, motion_comp=True, mask_target="scan"))["loc_data"]
    for k in ("fft_data", "fft_cfar"):
        assert same_bits(flagged[k], plain[k])


def _planar_errors(T):
    T = T.detach().cpu().double()
    return T[:, :2, 3].norm(dim=1).numpy(), torch.atan2(T[:, 1, 0], T[:, 0, 0]).abs().numpy()


def test_compensated_pose_end_to_end(batches):
    """Pairs 3 and 9 seen by a moving sensor (vel_std 12, yawrate_std 0.3) and by a standing one, prepare_batch, then the
    inference ICP (pt2pl, Huber, 50 iterations) from T_init; T_gt = I, so the planar error is the pose's own translation
    and yaw.  The compensated cloud must localise as the static twin does, within a factor 2 (the occlusion pattern of a
    moving viewpoint differs) plus ten times the pose-parity bound (1 cm, 1 mrad); the uncompensated cloud must do worse."""
    params, moving, static = batches
    model = policy(DEV, 0, **{k: params[k] for k in ("icp_type", "icp_loss_fn")}).eval()
    flagged = trn.prepare_batch(moving, dict(params, motion_comp=True))
    twin = trn.prepare_batch(static, params)
    with torch.no_grad():
        runs = {"static": model.icp(twin["loc_data"]["filtered_pc"], twin["map_data"]["pc"], static["T_init"], None),
                "compensated": model.icp(flagged["loc_data"]["filtered_pc"], flagged["map_data"]["pc"], moving["T_init"], None),
                "uncompensated": model.icp(flagged["loc_data"]["raw_pc"], flagged["map_data"]["pc"], moving["T_init"], None)}
    err = {k: _planar_errors(T) for k, T in runs.items()}
    for k, (tr, rot) in err.items():
        print("POSE %-13s translation %s m, yaw %s rad" % (k, np.round(tr, 4).tolist(), np.round(rot, 5).tolist()))
    assert err["static"][0].max() < 0.5 and err["static"][1].max() < 0.05      # the static twins localise: the comparison means something
    for i in range(len(PAIRS)):
        for q, extra in ((0, 0.01), (1, 0.001)):
            assert err["compensated"][q][i] <= 2 * err["static"][q][i] + extra, (PAIRS[i], q, err)
            assert err["uncompensated"][q][i] > err["compensated"][q][i], (PAIRS[i], q, err)
