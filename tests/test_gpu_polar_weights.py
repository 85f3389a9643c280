"""The polar-aware sampler on the GPU (radar_utils.extract_weights_polar, mmk_sample_weights_polar_*): values and both gradients
against the test-side restatement (tests/polar_weights_ref.py), the pixel-centre identity against the reference's golden
images, the adjoint identity, bit-reproducibility of the ordered scatter, a known answer, and the policy / training-step switch
params["polar_sampling"].

Tolerances (derived, not measured).  The only arithmetic the kernels do not share bit for bit with the restatement is sqrtf /
atan2f on the device against torch on the host (and grid_sample's own rounding of the tap weights, a few 2^-23).  An angle error
of k ulp of 2 pi moves v by k 2^-21 / min_step cells; with k = 16 that is `delta` (polar_weights_ref.position_error), which also
covers the range's ulp (R 2^-23 cells).  A weight is Lipschitz in the position with constant max|mask| per cell:
    |w - ref| <= delta max|mask| + 4 2^-23,      |grad_mask - ref| <= the same bound times max|gw|, per contributing tap.
grad_pc: the bilinear slopes are Lipschitz with constant 2 max|mask| per cell and are multiplied by du/drng = 1 / res and by
dv/dang / rng, on top of the project's 1e-5 max|ref| for the Cartesian kernel (test_gpu_point_grads.py):
    |grad_pc - ref| <= 1e-5 max|ref| + 2 max|mask| max|gw| delta (1 / res + dv / rng)   per point."""
import functools
import os

import numpy as np
import pytest
import torch

from mm_masking_amd import synthetic
from mm_masking_amd import radar_utils as ru
from mm_masking_amd import train_icp_weights as trn
from mm_masking_amd.icp_weight_policy import LearnICPWeightPolicy
from polar_weights_ref import azimuth_tables, polar_weights_ref, position_error, tap_counts
from radar_cases import RES
from support import DEV, policy_params

pytestmark = pytest.mark.gpu
N = 300
FLAGS = [(0, 0), (0, 1), (1, 0), (1, 1)]
FAKE_ROWS = (100, 255, 256, 299)            # both sides of the 256-thread block's edge, and the last row


def _points(az, A, R, seed):
    """(N, 3) fp32 points of one item, constructed from its azimuth table: every special case of the sampler at a fixed row,
    random interior points elsewhere.  Returns the points and the name -> rows dictionary."""
    rng = np.random.default_rng(seed)
    az = az.astype(np.float64)
    gap = 2 * np.pi - az[-1] + az[0]                      # between the last and the first azimuth, through 0
    rows = {}
    pts = np.zeros((N, 3))

    def put(name, i, r, a):
        pts[i, 0], pts[i, 1] = r * np.cos(a), r * np.sin(a)
        rows.setdefault(name, []).append(i)

    def r_of(u):
        return (u + 0.5) * RES                            # u = (rng - res / 2) / res

    put("beyond_last", 0, r_of(20.3), az[-1] + 0.2 * gap)
    put("beyond_last", 1, r_of(33.6), az[-1] + 0.1 * gap)
    put("below_first", 2, r_of(11.7), 0.4 * az[0])
    put("below_first", 3, r_of(50.2), 0.8 * az[0])
    for i, u in ((4, 25.4), (5, 60.7)):                   # exactly on +x: y = 0, ang = 0
        pts[i, 0], pts[i, 1] = r_of(u), 0.0
        rows.setdefault("on_plus_x", []).append(i)
    put("u_clamped", 6, 0.3 * RES / 2, az[3] + 0.4 * (az[4] - az[3]))
    put("u_clamped", 7, 0.8 * RES / 2, az[7] + 0.6 * (az[8] - az[7]))
    put("last_column", 8, r_of(R - 1 + 0.4), az[5] + 0.3 * (az[6] - az[5]))
    put("beyond_R", 9, r_of(R + 3.3), az[9] + 0.5 * (az[10] - az[9]))
    for i, y in ((10, 1.7), (11, -2.3)):                  # x = 0 alone: a real point at ang = pi / 2, 3 pi / 2
        pts[i, 0], pts[i, 1] = 0.0, y
        rows.setdefault("x_zero", []).append(i)
    for k in range(8):                                    # eight points inside one polar cell
        put("one_cell", 12 + k, r_of(30 + 0.1 + 0.1 * k), az[6] + (0.15 + 0.09 * k) * (az[7] - az[6]))
    put("wrap_fold", 20, r_of(40.5), az[-1] + 0.25 * gap)  # between the last and the first azimuth: taps on the wrap rows
    put("wrap_fold", 21, r_of(40.8), 0.6 * az[0])
    rows["fake"] = list(FAKE_ROWS)
    for i in range(22, N):
        if i in FAKE_ROWS:
            continue
        a, c = rng.integers(0, A - 1), rng.integers(0, R - 1)
        put("random", i, r_of(c + rng.uniform(0.05, 0.95)), az[a] + rng.uniform(0.05, 0.95) * (az[a + 1] - az[a]))
    pts[:, 2] = rng.normal(size=N)
    pts[list(FAKE_ROWS), :2] = 0.0
    return pts.astype(np.float32), rows


_CASES = {}


def _case(A, R):
    """Inputs of one mask shape (B = 2: a uniform and a wobbled table) and, per flag combination, the restatement's weights and
    gradients: computed once, shared by the tests, never modified."""
    if (A, R) in _CASES:
        return _CASES[(A, R)]
    az = azimuth_tables(A, 4000 + A)
    rng = np.random.default_rng(4100 + A)
    both = [_points(az[b], A, R, 4200 + 10 * A + b) for b in range(2)]
    pc = torch.from_numpy(np.stack([p for p, _ in both]))
    mask = torch.from_numpy(rng.uniform(0.0, 1.0, (2, A, R)).astype(np.float32))
    gw = torch.from_numpy(rng.normal(size=(2, N)).astype(np.float32))
    c = {"az": torch.from_numpy(az), "pc": pc, "mask": mask, "gw": gw, "rows": both[0][1], "ref": {}}
    for cross, wob in FLAGS:
        m, p = mask.clone().requires_grad_(True), pc.clone().requires_grad_(True)
        w, info = polar_weights_ref(m, p, c["az"], RES, bool(cross), bool(wob))
        (w * gw).sum().backward()
        c["ref"][(cross, wob)] = {"w": w.detach(), "gm": m.grad, "gpc": p.grad, "info": info}
    _CASES[(A, R)] = c
    return c


def _run(c, cross, wob, pc_grad=True):
    m = c["mask"].to(DEV).requires_grad_(True)
    p = c["pc"].to(DEV).requires_grad_(pc_grad)
    w = ru.extract_weights_polar(m, p, c["az"], RES, bool(cross), bool(wob))[0]
    (w * c["gw"].to(DEV)).sum().backward()
    return w.detach().cpu(), m.grad.cpu(), (p.grad.cpu() if pc_grad else None)


def test_points_are_constructed():
    """The generator's cases are where they are meant to be (the restatement's own positions, fp32)."""
    for A, R in ((16, 96), (50, 128)):
        c = _case(A, R)
        rows = c["rows"]
        for wob in (0, 1):
            i = c["ref"][(1, wob)]["info"]
            u, v = i["u"], i["v"]
            assert (c["pc"][:, rows["fake"], :2] == 0).all() and i["fake"].sum() == 2 * len(FAKE_ROWS)
            assert i["clamped"][:, rows["u_clamped"]].all() and i["clamped"].sum() == 4
            assert (torch.floor(u[:, rows["last_column"]]) == R - 1).all() and (u[:, rows["beyond_R"]] > R).all()
            assert (c["pc"][:, rows["on_plus_x"], 1] == 0).all() and (c["pc"][:, rows["x_zero"], 0] == 0).all()
            assert not i["fake"][:, rows["x_zero"]].any()
            if wob:
                cell = torch.floor(torch.stack([u[:, rows["one_cell"]], v[:, rows["one_cell"]]]))
                assert (cell == cell[:, :, :1]).all()
                # the table's ends gate the interpolation off: v = 0 or A - 1
                assert (v[:, rows["below_first"] + rows["on_plus_x"]] == 0).all() and (v[:, rows["beyond_last"]] == A - 1).all()
                assert i["gated"][:, rows["wrap_fold"]].all()
            else:                                         # the uniform step extrapolates onto the wrap rows
                assert (v[:, rows["below_first"] + rows["on_plus_x"] + rows["wrap_fold"][1:]] < 0).all()
                assert (v[:, rows["beyond_last"] + rows["wrap_fold"][:1]] > A - 1).all()


@pytest.mark.parametrize("A,R", [(16, 96), (50, 128)])
@pytest.mark.parametrize("cross,wob", FLAGS)
def test_values_and_gradients_against_restatement(A, R, cross, wob):
    """Measured worst ratios error / bound are printed (and recorded in the change's summary)."""
    c = _case(A, R)
    ref = c["ref"][(cross, wob)]
    info = ref["info"]
    w, gm, gpc = _run(c, cross, wob)
    delta = position_error(c["az"].numpy())
    M, G = float(c["mask"].abs().max()), float(c["gw"].abs().max())
    # weights
    tol_w = delta * M + 4 * 2.0 ** -23
    r_w = float((w - ref["w"]).abs().max()) / tol_w
    assert (w[:, list(FAKE_ROWS)] == 0).all()
    # grad_mask: the weights' bound times max|gw| per contributing tap.  The taps of a cell: the restatement's own (tap_counts,
    # reach 0), plus, for a point within 2 delta of a cell boundary (the gated rows of the wobble fix sit exactly on one), any
    # cell next to its taps: the last ulp of the position decides which of the two cells carries the weight <= delta.
    near = tap_counts(info, A, R, bool(cross), reach=1) > 0
    assert (gm[~near].view(torch.int32) == 0).all()                              # untouched cells: +0, bit for bit
    assert (ref["gm"][~near] == 0).all() and (~near).sum() > 0
    fu = (info["u"] - torch.round(info["u"])).abs()
    fv = (info["v"] - torch.round(info["v"])).abs()
    edge = (fu < 2 * delta) | (fv < 2 * delta)
    count = tap_counts(info, A, R, bool(cross)) + tap_counts(info, A, R, bool(cross), reach=1, select=edge)
    tol_gm = count * (tol_w * G)
    err_gm = (gm - ref["gm"]).abs()
    assert (err_gm[count == 0] == 0).all()
    r_gm = float((err_gm[count > 0] / tol_gm[count > 0]).max())
    # grad_pc
    assert (gpc[:, :, 2:] == 0).all() and (gpc[:, list(FAKE_ROWS)] == 0).all()
    smooth = ((fu >= 1e-3) | info["clamped"]) & ((fv >= 1e-3) | info["gated"]) & ~info["fake"]
    assert smooth.float().mean() > 0.9                                           # the generator keeps clear of the jumps
    if wob:                                                                      # (placed against the table the wobble fix reads)
        for name in ("u_clamped", "one_cell", "last_column", "beyond_R", "random", "beyond_last", "below_first", "on_plus_x"):
            assert smooth[:, c["rows"][name]].all(), name
    chain = 1.0 / RES + info["dv"] / info["rng"]
    tol_pc = 1e-5 * float(ref["gpc"].abs().max()) + 2 * M * G * delta * chain
    err_pc = (gpc[:, :, :2] - ref["gpc"][:, :, :2]).abs().amax(dim=2)
    r_pc = float((err_pc[smooth] / tol_pc[smooth]).max())
    assert float(ref["gpc"][:, :, :2].abs().max()) > 0
    print("polar weights %dx%d crossover %d wobble %d: error / bound  weights %.3f  grad_mask %.3f  grad_pc %.3f  (delta %.2e)"
          % (A, R, cross, wob, r_w, r_gm, r_pc, delta))
    assert r_w <= 1.0, r_w
    assert r_gm <= 1.0, r_gm
    assert r_pc <= 1.0, r_pc


@pytest.mark.parametrize("cross,wob", FLAGS)
def test_pixel_centre_identity_against_golden(golden_dir, cross, wob):
    """At the centres of the 32 x 32 grid of 0.2384 m pixels the sampler reads what the reference's
    radar_polar_to_cartesian_diff writes to the pixels (tests/golden/make_golden_polar_weights.py)."""
    g = np.load(os.path.join(golden_dir, "polar_weights.npz"), allow_pickle=False)
    W = int(g["pw_width"])
    half = (W / 2 - 0.5) * 0.2384
    coords = torch.linspace(-half, half, W)
    pts = torch.stack([(-coords)[:, None].expand(W, W), coords[None, :].expand(W, W)], dim=-1).reshape(1, -1, 2).expand(2, -1, -1)
    assert pts.shape[1] == 1024
    w = ru.extract_weights_polar(torch.from_numpy(g["pw_mask"]).to(DEV), pts.contiguous(), torch.from_numpy(g["pw_az"]),
                                 float(g["pw_res"]), bool(cross), bool(wob))[0]
    want = g["pw_cart_%d%d" % (cross, wob)]
    bound = position_error(g["pw_az"]) * float(g["pw_mask"].max()) + 4 * 2.0 ** -23
    err = np.abs(w.cpu().numpy().reshape(2, W, W) - want).max()
    print("pixel-centre identity crossover %d wobble %d: max |diff| %.2e (bound %.2e)" % (cross, wob, err, bound))
    assert err <= bound


@pytest.mark.parametrize("cross,wob", FLAGS)
def test_adjoint_identity(cross, wob):
    """The operator is linear in the mask: sum gw fwd(mask) = sum grad_mask mask, both in fp64, to 1e-6 relative."""
    c = _case(50, 128)
    w, gm, _ = _run(c, cross, wob, pc_grad=False)
    lhs = (c["gw"].double() * w.double()).sum().item()
    rhs = (gm.double() * c["mask"].double()).sum().item()
    print("adjoint identity crossover %d wobble %d: %.9g against %.9g" % (cross, wob, lhs, rhs))
    assert abs(lhs) > 1.0 and abs(lhs - rhs) <= 1e-6 * abs(lhs), (lhs, rhs)


def test_mask_gradient_is_reproducible():
    c = _case(16, 96)
    info = c["ref"][(1, 1)]["info"]
    cnt = tap_counts(info, 16, 96, True)                                         # the four taps of every real point
    assert int((cnt > 1).sum()) >= 100
    _, g1, _ = _run(c, 1, 1, pc_grad=False)
    _, g2, _ = _run(c, 1, 1, pc_grad=False)
    _, g3, _ = _run(c, 1, 1, pc_grad=True)
    assert torch.equal(g1, g2) and torch.equal(g1, g3)
    assert g1.abs().sum() > 0


def test_known_answer_and_what_the_cartesian_sampler_reads():
    """A block of ones in a polar mask: points at the centres of its interior cells weigh 1, points two cells outside 0 -- and
    extract_weights, which samples any mask with the Cartesian grid's normalisation, reads something else there."""
    A, R = 50, 128
    az = azimuth_tables(A, 4050)
    mask = torch.zeros(2, A, R)
    mask[:, 10:20, 40:80] = 1.0
    inside = [(r, c) for r in range(11, 19) for c in (41, 55, 77)]
    outside = [(8, 50), (21, 50), (15, 37), (15, 81), (8, 37), (21, 81)]
    pts = np.zeros((2, len(inside) + len(outside), 3), dtype=np.float32)
    for b in range(2):
        for i, (r, c) in enumerate(inside + outside):
            rng = (c + 0.5 + 0.5) * RES               # u = (rng - res / 2) / res = c + 0.5: between columns c and c + 1
            pts[b, i, 0], pts[b, i, 1] = rng * np.cos(float(az[b, r])), rng * np.sin(float(az[b, r]))
    pc = torch.from_numpy(pts)
    w = ru.extract_weights_polar(mask.to(DEV), pc, torch.from_numpy(az), RES)[0].cpu()
    n = len(inside)
    assert (w[:, :n] - 1.0).abs().max() <= 4 * 2.0 ** -23
    assert (w[:, n:] == 0).all()
    wc = ru.extract_weights(mask.to(DEV), pc)[0].cpu()
    assert not torch.allclose(wc[:, :n], torch.ones(2, n), atol=0.5)
    assert (wc[:, :n] - 1.0).abs().max() > 0.5


_policy_params = functools.partial(policy_params, DEV, dropout=0.0, network_input_type="polar", network_output_type="polar",
                                   icp_type="pt2pl", icp_loss_fn={"name": "huber", "metric": 1.0}, max_iter=5)


def test_policy_switch():
    """forward with params["polar_sampling"] weighs the points with extract_weights_polar of its own mask, bit for bit; its
    checks; and polar_sampling=False is the policy without the key."""
    A, R, n = 64, 128, 200
    raw = synthetic.make_batch([0, 1], device=DEV, m_valid=3000, m_pad=3072, density="sparse")
    fft = raw["fft_polar"][:, :A, :R].contiguous()
    az = torch.from_numpy(azimuth_tables(A, 4064)).to(DEV)
    rng = np.random.default_rng(4065)
    pc = np.zeros((2, n, 3), dtype=np.float32)
    rr, aa = rng.uniform(0.2, (R + 4) * RES, (2, n)), rng.uniform(0, 2 * np.pi, (2, n))
    pc[..., 0], pc[..., 1] = rr * np.cos(aa), rr * np.sin(aa)
    pc[:, -7:] = 0.0
    pc = torch.from_numpy(pc).to(DEV)
    loc = {"fft_data": fft, "fft_cfar": torch.zeros_like(fft), "raw_pc": pc, "filtered_pc": pc, "azimuths": az}
    mp = {"pc": raw["map_pc"]}
    seen = {}

    def build(**over):
        torch.manual_seed(7)
        m = LearnICPWeightPolicy(_policy_params(**over)).to(DEV)
        m.eval()
        m.icp = lambda scan_pc, map_pc, T_init, weights: (seen.__setitem__("w", weights), T_init)[1]
        return m

    with torch.no_grad():
        model = build(polar_sampling=True)
        T, mask, d = model(loc, mp, raw["T_init"])
        assert mask.shape == (2, A, R)
        want = ru.extract_weights_polar(mask, pc, az, model.res)
        assert torch.equal(seen["w"], want[0]) and torch.equal(d, want[1])
        assert torch.equal(model.mean_w, want[3]) and torch.equal(model.max_w, want[4]) and torch.equal(model.min_w, want[5])
        assert not torch.equal(seen["w"], ru.extract_weights(mask, pc)[0])
        with pytest.raises(KeyError, match="prepare_batch.*keep_polar=True"):
            model({k: v for k, v in loc.items() if k != "azimuths"}, mp, raw["T_init"])
        with pytest.raises(ValueError, match="override_mask"):
            model(loc, mp, raw["T_init"], override_mask=torch.ones(2, 640, 640, device=DEV))
        ones = torch.ones(2, A, R, device=DEV)
        To, mo, _ = model(loc, mp, raw["T_init"], override_mask=ones)            # generate_baseline's path
        assert torch.equal(mo, ones) and torch.equal(seen["w"], ru.extract_weights_polar(ones, pc, az, model.res)[0])
        # flag False = key absent
        outs = []
        for over in ({"polar_sampling": False}, {}):
            m2 = build(**over)
            T2, mask2, d2 = m2(loc, mp, raw["T_init"])
            outs.append((mask2, d2, seen["w"], m2.mean_w))
        assert all(torch.equal(a, b) for a, b in zip(*outs))
        assert torch.equal(outs[0][2], ru.extract_weights(outs[0][0], pc)[0])


def test_full_size_training_step_with_the_default_loss():
    """B = 2 at 400 x 3360 with the default loss weights (mask_pts = 1): with the flag the map-point term is the BCE against
    polar_target_from_pts and the step trains every parameter; without it the same call cannot form the loss."""
    raw = synthetic.make_batch([0, 1], device=DEV, m_valid=3000, m_pad=3072, density="sparse")
    params = _policy_params(polar_sampling=True, dropout=0.05)
    batch = trn.prepare_batch(raw, params, max_loc_pts=2048)
    assert batch["loc_data"]["azimuths"] is raw["azimuths"] and batch["loc_data"]["fft_data"].shape == (2, 400, 3360)
    assert "fft_polar" not in batch["loc_data"]
    lw = trn.loss_weights_from(params)
    assert lw["mask_pts"] == 1.0
    torch.manual_seed(3)
    model = LearnICPWeightPolicy(params).to(DEV)
    model.train()
    loc, mp, Ts = batch["loc_data"], batch["map_data"], batch["transforms"]
    T_pred, mask, n0 = model(loc, mp, Ts["T_ml_init"])
    assert mask.shape == (2, 400, 3360)
    loss, comp = trn.eval_training_loss(T_pred, mask, n0, Ts["T_ml_gt"], loc, mp, model, loss_weights=lw)
    assert torch.isfinite(loss).all()
    target = ru.polar_target_from_pts(mp["pc"], loc["azimuths"], model.res, (400, 3360))
    assert target.shape == (2, 400, 3360) and target.dtype == torch.float32
    assert float(target.min()) >= 0.0 and float(target.max()) <= 1.0 and float(target.max()) > 0.5
    assert torch.equal(comp["mask_pts"], trn._bce_mean(mask.detach(), target))
    loss.backward()
    for name, q in model.named_parameters():
        assert q.grad is not None and torch.isfinite(q.grad).all(), name
    assert sum(q.grad.abs().sum().item() for q in model.parameters()) > 0
    model.polar_sampling = False                         # the policy without the flag: (B,400,3360) against (B,640,640)
    with pytest.raises(ValueError, match="target size"):
        trn.eval_training_loss(T_pred.detach(), mask.detach(), n0.detach(), Ts["T_ml_gt"], loc, mp, model, loss_weights=lw)
