"""CPU: the motion compensation without a device -- the ABI of its entries and their host-side checks, the restatement of
tests/deskew_ref.py against torch.linalg.matrix_exp with its identities as bits, the cancellation figure that the GPU test's
grad_twist tolerance rests on, scan_times, the ValueErrors of the policy and the batch builder, what make_pair's new
arguments change, and the point-to-map distance of a moving scan before and after the de-skew."""
import ctypes

import numpy as np
import pytest
import torch

from mm_masking_amd import _lib, synthetic
from mm_masking_amd import radar_utils as ru
from mm_masking_amd import train_icp_weights as trn
from oracle import radar_ref as R

import deskew_ref as dr
from support import header, n_args, policy

NULL = ctypes.c_void_p(0)
FAKE = ctypes.c_void_p(4096)          # never dereferenced: every call below fails on the host before any launch
RES = 0.0596


@pytest.fixture(scope="module")
def L():
    _lib.build()
    return _lib.lib()


# ----------------------------------------------------------------------------- the ABI
def test_entries_are_declared_exported_and_bound(L):
    hdr = header()
    for name, arity in (("mmk_extract_peaks_t", 17), ("mmk_deskew_points", 7), ("mmk_deskew_points_bwd_workspace_bytes", 2),
                        ("mmk_deskew_points_bwd", 11)):
        assert hasattr(L, name) and name in _lib.EXPORTED
        assert len(_lib.EXPORTED[name][1]) == n_args(hdr, name) == arity, name
    assert n_args(hdr, "mmk_extract_peaks_t") == n_args(hdr, "mmk_extract_peaks") + 1
    assert _lib.CONSTANTS["MMK_VERSION"] == 502 == L.mmk_version()            # additions only


def test_host_side_checks_raise_without_a_launch(L):
    need = L.mmk_extract_peaks_workspace_bytes(1, 4, 16, 8)
    peaks = (FAKE, 1, 4, 16, RES, FAKE, FAKE, NULL, 0, 10.0, 8, FAKE, FAKE, FAKE)
    assert L.mmk_extract_peaks_t(*peaks, need, NULL, NULL) == -1 and b"mmk_extract_peaks_t" in L.mmk_last_error()    # no out_time
    assert L.mmk_extract_peaks_t(FAKE, 1, 4, 16, RES, FAKE, NULL, NULL, 0, 10.0, 8, FAKE, FAKE, FAKE, need, FAKE, NULL) == -1   # no times
    assert L.mmk_extract_peaks_t(*peaks, need - 1, FAKE, NULL) == -3
    assert L.mmk_last_error() == b"mmk_extract_peaks_t: workspace too small (%d < %d)" % (need - 1, need)
    assert L.mmk_extract_peaks_t(FAKE, 1, 4, 1, RES, FAKE, FAKE, NULL, 0, 10.0, 8, FAKE, FAKE, FAKE, need, FAKE, NULL) == -1
    assert L.mmk_last_error() == b"mmk_extract_peaks_t: bad shape"
    assert L.mmk_extract_peaks(*peaks, need - 1, NULL) == -3                                   # the shared path names its entry
    assert L.mmk_last_error() == b"mmk_extract_peaks: workspace too small (%d < %d)" % (need - 1, need)

    assert L.mmk_deskew_points(NULL, FAKE, FAKE, 1, 4, FAKE, NULL) == -1 and b"NULL" in L.mmk_last_error()
    assert L.mmk_deskew_points(FAKE, FAKE, FAKE, 1, 4, NULL, NULL) == -1
    assert L.mmk_deskew_points(FAKE, FAKE, FAKE, 0, 4, FAKE, NULL) == -1 and b"bad shape" in L.mmk_last_error()
    assert L.mmk_deskew_points(FAKE, FAKE, FAKE, 1, 0, FAKE, NULL) == -1
    assert L.mmk_deskew_points_bwd_workspace_bytes(0, 4) == 0 and L.mmk_deskew_points_bwd_workspace_bytes(1, 0) == 0
    # one fp64 partial of six per block of 256 points and item, in whole 256-byte units
    assert L.mmk_deskew_points_bwd_workspace_bytes(1, 256) == 256 and L.mmk_deskew_points_bwd_workspace_bytes(1, 257) == 256
    assert L.mmk_deskew_points_bwd_workspace_bytes(32, 5120) == 32 * 20 * 6 * 8
    need = L.mmk_deskew_points_bwd_workspace_bytes(3, 1000)
    bwd = (FAKE, FAKE, FAKE, 3, 1000, FAKE)
    assert L.mmk_deskew_points_bwd(*bwd, FAKE, FAKE, FAKE, need - 1, NULL) == -3
    assert L.mmk_last_error() == b"mmk_deskew_points_bwd: workspace too small (%d < %d)" % (need - 1, need)
    assert L.mmk_deskew_points_bwd(*bwd, FAKE, FAKE, NULL, 0, NULL) == -3                      # grad_twist needs the workspace
    assert L.mmk_deskew_points_bwd(*bwd, NULL, NULL, FAKE, need, NULL) == -1 and b"neither" in L.mmk_last_error()
    assert L.mmk_deskew_points_bwd(FAKE, FAKE, FAKE, 3, 1000, NULL, FAKE, FAKE, FAKE, need, NULL) == -1
    assert L.mmk_deskew_points_bwd(FAKE, NULL, FAKE, 3, 1000, FAKE, FAKE, FAKE, FAKE, need, NULL) == -1


def test_python_argument_checks():
    pc, t, tw = torch.zeros(2, 5, 3), torch.zeros(2, 5), torch.zeros(2, 6)
    for bad in ((pc[:, :, :2], t, tw), (pc, t[:, :4], tw), (pc, t, tw[:1]), (pc, t, tw[:, :5]), (pc[:, :0], t[:, :0], tw)):
        with pytest.raises(ValueError, match="deskew_pc"):
            ru.deskew_pc(*bad)
    with pytest.raises(ValueError, match="return_times"):
        ru.extract_pc_padded(torch.zeros(1, 4, 16), RES, torch.zeros(1, 4), None, 8, return_times=True)
    assert "deskew_pc" in ru.__all__ and "scan_times" in ru.__all__
    if not torch.cuda.is_available():
        with pytest.raises(_lib.MmkError):                                    # HIP only, like its neighbours
            ru.deskew_pc(pc, t, tw)


# ----------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("scale", [1.0, 1e-3, 0.0])
def test_restatement_agrees_with_matrix_exp(scale):
    rng = np.random.default_rng(5)
    pc = torch.from_numpy(rng.uniform(-70, 70, (2, 400, 3)))
    t = torch.from_numpy(rng.uniform(-0.125, 0.125, (2, 400)))
    tw = (torch.tensor([dr.TWISTS["sixdof"], dr.TWISTS["fast"]], dtype=torch.float64) * scale).requires_grad_(True)
    th2 = ((t[..., None] * tw.detach()[:, None, 3:]) ** 2).sum(-1)
    if scale == 1.0:
        assert (th2 < dr.SERIES_CUT).any() and (th2 >= dr.SERIES_CUT).any()     # both branches in one call
    p1 = pc.clone().requires_grad_(True)
    out = dr.deskew_ref(p1, t, tw)
    G = torch.from_numpy(rng.normal(0, 1, out.shape))
    gp, gw = torch.autograd.grad(out, (p1, tw), G)
    tw2, p2 = tw.detach().clone().requires_grad_(True), pc.clone().requires_grad_(True)
    want = dr.matrix_exp_ref(p2, t, tw2)
    gp2, gw2 = torch.autograd.grad(want, (p2, tw2), G)
    for name, got, ref in (("value", out, want), ("grad_pc", gp, gp2), ("grad_twist", gw, gw2)):
        err = (got - ref).abs().max().item() / ref.abs().max().item()
        print("RESTATEMENT scale %g %-10s err/scale = %.2e (scale %.3e)" % (scale, name, err, ref.abs().max().item()))
        assert err <= 1e-10, (name, err)


def test_restatement_identities_hold_as_bits():
    pc, t, tw, _ = dr.operator_case(3, 257, "mixed")
    names = list(dr.TWISTS)
    out = dr.deskew_ref(dr.f64(pc), dr.f64(t), dr.f64(tw)).to(torch.float32).numpy()
    zero, planar = names.index("zero"), names.index("planar")
    assert np.array_equal(out[zero].view(np.uint32), pc[zero].view(np.uint32))                # twist = 0: the input bits
    col = 257 // 4
    assert (t[:, col] == 0).all() and np.array_equal(out[:, col].view(np.uint32), pc[:, col].view(np.uint32))   # s = 0
    assert (out[planar, :, 2] == 0).all() and np.abs(out[planar, :, :2] - pc[planar, :, :2]).max() > 0.1      # planar: z = 0
    pad = (pc == 0).all(-1)
    assert pad.sum() == 3 * 2 and (out[pad] == 0).all()                                      # padding stays padding ...
    moved = np.abs(out - pc).max(-1)
    assert (moved[~pad & (t != 0) & (np.arange(3)[:, None] != zero)] > 0).all()
    _, gp, gw, terms = dr.deskew_ref_grads(pc, t, tw, np.ones_like(pc))
    assert (gp[pad] == 0).all() and (terms[pad] == 0).all() and np.abs(gw).min() > 0          # ... and takes no gradient


def test_cancellation_figure_of_the_gradient_cases():
    """sum_i |s_i (u_bar_i; w_bar_i)| over the points and the six components of an item, over max |grad_twist| of the item:
    how much larger than the result the summed terms are.  The device sums them in fp64, so its error is bounded by
    N 2^-53 times this figure relative to the result; below 1e4 that is 5 120 * 1.1e-16 * 1e4 = 6e-9, far inside the 2^-22 the GPU
    test allows.  Measured: the largest figure over all cases is printed (about 4e2 at 5 120 points)."""
    worst = 0.0
    for B, N in dr.SHAPES:
        for kind in dr.KINDS:
            pc, t, tw, G = dr.operator_case(B, N, kind)
            _, _, gw, terms = dr.deskew_ref_grads(pc, t, tw, G)
            fig = np.abs(terms).sum((1, 2)) / np.abs(gw).max(1)
            worst = max(worst, fig.max())
            assert np.isfinite(fig).all() and fig.max() < 1e4, (B, N, kind, fig)
    print("CANCELLATION largest sum|terms| / max|grad_twist| = %.3e" % worst)


# ----------------------------------------------------------------------------- scan_times
def test_scan_times_on_epoch_stamps_and_on_a_rolled_row():
    base = 1_697_000_000_000_000                                                # microseconds since the epoch: 2^50.6
    stamps = torch.tensor([[base + 625 * a for a in range(400)], [base + 7 + 625 * a for a in range(400)]], dtype=torch.int64)
    mid = ru.scan_times(stamps)
    assert mid.dtype == torch.float32 and mid.shape == (2, 400)
    want = (((np.arange(400) - 199.5) * 625.0) * 1e-6).astype(np.float32)
    assert np.array_equal(mid[0].numpy(), want) and np.array_equal(mid[1].numpy(), want)    # fp64 subtraction, then the cast
    assert np.array_equal(ru.scan_times(stamps, ref="first")[0].numpy(), ((np.arange(400) * 625.0) * 1e-6).astype(np.float32))
    assert np.array_equal(ru.scan_times(stamps, ref="last")[1].numpy(), (((np.arange(400) - 399) * 625.0) * 1e-6).astype(np.float32))
    rolled = torch.roll(stamps, 137, dims=1)                                    # the augmentation rolls the rows of a scan
    assert torch.equal(ru.scan_times(rolled), torch.roll(mid, 137, dims=1))
    # synthetic's fp32 stamps; another unit; the generator's own rule
    syn = torch.from_numpy((np.arange(400, dtype=np.float32) * 625.0)[None])
    assert np.array_equal(ru.scan_times(syn)[0].numpy(), want)
    assert np.array_equal(ru.scan_times(syn, unit=1e-3)[0].numpy(), (((np.arange(400) - 199.5) * 625.0) * 1e-3).astype(np.float32))
    assert np.array_equal(synthetic.scan_seconds(syn[0].numpy()).astype(np.float32), want)
    with pytest.raises(ValueError, match="ref"):
        ru.scan_times(syn, ref="centre")
    with pytest.raises(ValueError, match="B, A"):
        ru.scan_times(syn[0])


# ----------------------------------------------------------------------------- the policy and the batch builder
def test_policy_and_builder_value_errors():
    model = policy("cpu", 0, mask_target="scan", motion_comp=True, unet_backend="torch")
    assert model.motion_comp and model.motion_time_unit == 1e-6 and model.motion_ref == "mid"
    plain = policy("cpu", 0, mask_target="scan", unet_backend="torch")
    assert plain.motion_comp is False
    with pytest.raises(ValueError, match="motion_ref"):
        policy("cpu", 0, motion_comp=True, motion_ref="centre")
    times, vel = torch.zeros(1, 400), torch.zeros(1, 6)
    # (raised before anything else of the batch is read: the batches below hold nothing the forward could move to a device)
    with pytest.raises(ValueError, match="velocity"):
        model({"az_times": times}, {}, None)
    with pytest.raises(ValueError, match="az_times"):
        model({"velocity": vel}, {}, None)
    with pytest.raises(ValueError, match="az_times"):
        model({"velocity": vel, "az_times": None}, {}, None)
    params = trn.default_params("cpu")
    params["motion_comp"] = True
    with pytest.raises(ValueError, match="velocity"):
        trn.prepare_batch({"az_times": times}, params)
    with pytest.raises(ValueError, match="velocity"):
        trn.prepare_batch({"velocity": vel}, params)


# ----------------------------------------------------------------------------- synthetic pairs
@pytest.fixture(scope="module")
def pairs():
    static = synthetic.make_pair(3, dataset_type="test")
    moving = synthetic.make_pair(3, dataset_type="test", velocity=(12.0, 0.5, 0.0, 0.0, 0.0, 0.3))
    return static, moving


def test_make_pair_at_std_zero_and_above(pairs):
    static, moving = pairs
    again = synthetic.make_pair(3, dataset_type="test", vel_std=0.0, yawrate_std=0.0)
    assert list(again) == list(static) == ["fft_polar", "azimuths", "az_times", "map_pc", "T_init", "T_gt"]
    for k in static:
        assert again[k].dtype == static[k].dtype and np.array_equal(again[k], static[k]), k
    assert static["fft_polar"].shape == (400, 3360) and "velocity" not in static
    for kw in ({"dataset_type": "test"}, {"dataset_type": "train"}):
        drawn = synthetic.make_pair(3, vel_std=12.0, yawrate_std=0.3, **kw)
        ref = static if kw["dataset_type"] == "test" else synthetic.make_pair(3, **kw)
        assert drawn["velocity"].dtype == np.float32 and drawn["velocity"].shape == (6,)
        assert (drawn["velocity"][2:5] == 0).all() and (drawn["velocity"][[0, 1, 5]] != 0).all()          # a planar twist
        if kw["dataset_type"] == "train":
            assert np.abs(drawn["velocity"][:2]).max() <= 12.0 and abs(drawn["velocity"][5]) <= 0.3
        r7 = np.random.default_rng([synthetic.BASE_SEED + 3, 7])
        d = r7.uniform(-1, 1, 3) if kw["dataset_type"] == "train" else r7.normal(0, 1, 3)
        assert np.array_equal(drawn["velocity"], np.array([12 * d[0], 12 * d[1], 0, 0, 0, 0.3 * d[2]], dtype=np.float32))
        for k in ("azimuths", "az_times", "map_pc", "T_init", "T_gt"):
            assert np.array_equal(drawn[k], ref[k]), k
        assert not np.array_equal(drawn["fft_polar"], ref["fft_polar"])
    for k in ("azimuths", "az_times", "map_pc", "T_init", "T_gt"):
        assert np.array_equal(moving[k], static[k]), k
    assert np.array_equal(moving["velocity"], np.array([12, 0.5, 0, 0, 0, 0.3], dtype=np.float32))
    only_yaw = synthetic.make_pair(3, dataset_type="test", yawrate_std=0.3)
    assert (only_yaw["velocity"][:5] == 0).all() and only_yaw["velocity"][5] != 0


def _map_distance(cloud, map_xy):
    d = torch.cat([torch.cdist(c, map_xy).min(dim=1).values for c in torch.from_numpy(cloud[:, :2].astype(np.float32)).split(1024)])
    return d.numpy()


def test_point_to_map_distance(pairs):
    """Pair 3 seen by a sensor that moves with (12, 0.5, 0, 0, 0, 0.3) and by one that stands still: the distance from every
    extracted point (oracle cfar_mask / extract_pc, diff=False) to its nearest map point.  Measured:
        static scene             4 461 points, median 0.124 m, 78.8 % within 0.3 m
        moving, as extracted     4 452 points, median 0.367 m, 41.2 % within 0.3 m
        moving, de-skewed        4 452 points, median 0.113 m, 83.1 % within 0.3 m
    (The de-skewed cloud lies a little closer than the static one: a moving pole lights the azimuth NEAREST its bearing,
    a static one the first azimuth at or beyond it, as the generator always did.)  Required: the de-skewed median within
    1.25 x the static scene's (the occlusion pattern differs between a moving and a fixed viewpoint), and the raw median at
    least twice the de-skewed one."""
    static, moving = pairs
    map_xy = torch.from_numpy(static["map_pc"][:20000, :2].copy())
    fig = {}
    for name, pair in (("static", static), ("moving", moving)):
        mask = R.cfar_mask(pair["fft_polar"][None], RES, diff=False)
        cloud = R.extract_pc(mask, RES, pair["azimuths"][None], pair["az_times"][None], diff=False)[0]
        fig[name] = (cloud, mask)
    cloud, mask = fig["moving"]
    seconds = ru.scan_times(torch.from_numpy(moving["az_times"][None]))
    t, cnt = dr.point_times_ref(mask, seconds.numpy(), RES, 8192)
    assert cnt[0] == len(cloud) and np.abs(t[0, :cnt[0]]).max() <= 0.125 and np.abs(t[0, :cnt[0]]).max() > 0.12
    fixed = dr.deskew_ref(dr.f64(cloud[None]), dr.f64(t[:, :cnt[0]]), dr.f64(moving["velocity"][None]))[0].to(torch.float32).numpy()
    med = {}
    for name, c in (("static", fig["static"][0]), ("raw", cloud), ("deskewed", fixed)):
        d = _map_distance(c, map_xy)
        med[name] = float(np.median(d))
        print("MAP DISTANCE %-9s %5d points, median %.3f m, %4.1f %% within 0.3 m" % (name, len(c), med[name], 100 * (d < 0.3).mean()))
    assert med["deskewed"] <= 1.25 * med["static"], med
    assert med["raw"] >= 2 * med["deskewed"], med
