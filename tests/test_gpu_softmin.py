"""GPU: soft correspondences of the HIP dICP (mmk_icp_forward_soft / mmk_icp_backward_soft, mmk_knn_search; DESIGN.md §3 I2',
I3''', I7''') against the restatement tests/dicp_restatement.py: the stand-alone k-NN element for element, the forward and the
gradients of source, target, weight and T_init from both backward shapes, structural zeros, bit reproducibility, the nearest
limit against the hard call, the untouched `nearest` mode and the policy's params["icp_correspondence"].

The reference REPLAYS the neighbours of the GPU run (fixed_idx): device and host expf may differ in the last bit, and a
flipped near-tie of a later search must not turn that into a failure.  idx_hist[0], found before the first solve, is compared
bit for bit with the free-running reference.

Shapes (tests/dicp_cases.py): B = 2, 300 + 20 zero source rows (one full and one partial 256-thread block),
700 + 30 target_pad_val rows, K = 4, T_init shifted by 0.2 m, trim_dist 1.0, tau = 0.25 m^2, k in {4, 8}.  Every case asserts
on the reference's own values that the soft-min is awake (a_0 < 0.9 for 30 % at least of the real points in every iteration),
that 30 % of the real points pass the gate in every iteration, that Huber is past its knee for 30 % of them, and that no pair
froze.

Tolerances: pose 2e-6 absolute and gradients 2e-3 of the reference's largest magnitude, the bounds of
tests/test_gpu_point_grads.py.  The nearest limit's target gradient: the hard and the soft call add the same non-zero rows as
fixed point at resolutions max|row entry| 2^(cnt_bits - 62), cnt_bits <= 14, over at most 2^14 rows (2^-34 max|row entry| in
all) and round the sum to fp32 once (2^-24 relative, twice): asserted at 2^-22 |value| + 2^-30 max|value|, which leaves room
for row entries 16 times larger than the largest sum.

Measured on an MI355X (all cases, k = 4 and 8): pose within 6.8e-7 of the replay; gradients within 3.3e-5 of the reference's
largest magnitude (weight, pt2pt Huber dim 3; source 1.4e-5, target 1.2e-5, T_init 6.6e-6 at most); a_0 < 0.9 for 77 - 98 % of
the real points in every iteration, 73 - 100 % pass the gate, Huber past its knee for 65 % (pt2pl dim 2) and 40 % (pt2pt dim 3)
of them over the iterations; the nearest limit's target gradient differs from the hard call's by at most 2.8e-17.
"""
import numpy as np
import pytest
import torch

from mm_masking_amd import _lib
from mm_masking_amd.dICP.ICP import ICP
from oracle.dicp_ref import transform_points

from dicp_cases import (B, K, M, M_REAL, N, N_REAL, NAMES, SOFTMIN_CASES as CASES, SOFTMIN_IDS as IDS, SOFTMIN_TRIM as TRIM, TAU, TOL,
                        assert_softmin_awake, close, first_neighbours, gpu, inputs, nn_engine, reference)  # noqa: F401
from dicp_restatement import knn_ref_batch
from radar_cases import scene64  # noqa: F401  (the smallest scan-mode batch of the suite, a module fixture)
from support import DEV, policy

pytestmark = pytest.mark.gpu


def _knn_search(src, tgt, T, dim, k):
    """mmk_knn_search on device tensors -> idx (B,N,k) int32, d2 (B,N,k) fp32, on the host."""
    L = _lib.lib()
    Bq, Nq, Mq = src.shape[0], src.shape[1], tgt.shape[1]
    nbytes = L.mmk_knn_search_workspace_bytes(Bq, Nq, Mq, k)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    idx = torch.full((Bq, Nq, k), -7, dtype=torch.int32, device=DEV)
    d2 = torch.full((Bq, Nq, k), -7.0, dtype=torch.float32, device=DEV)
    _lib.check(L.mmk_knn_search(_lib.ptr(src), _lib.ptr(tgt), _lib.ptr(T), Bq, Nq, Mq, tgt.shape[2], dim, k, _lib.ptr(idx),
                                _lib.ptr(d2), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(DEV)))
    torch.cuda.synchronize()
    return idx.cpu(), d2.cpu()


# ----------------------------------------------------------------------------- 1. the stand-alone k-NN
def _knn_inputs(dim, n, m):
    rng = np.random.default_rng(100 + dim + n + m)
    tgt = np.zeros((2, m, 6), np.float32)
    tgt[..., :3] = rng.uniform(-20, 20, (2, m, 3)).astype(np.float32)
    if dim == 2:
        tgt[..., 2] = 0
    if m >= 112:
        tgt[:, 40, :3] = tgt[:, 5, :3]                           # duplicated rows: ties go to the lowest index
        tgt[:, 77, :3] = tgt[:, 5, :3]
        tgt[:, 100:112, 0] = rng.uniform(3.1, 3.9, (2, 12))     # twelve rows in one 2 m cell
        tgt[:, 100:112, 1] = rng.uniform(7.1, 7.9, (2, 12))
    src = np.zeros((2, n, 3), np.float32)
    src[...] = rng.uniform(-22, 22, (2, n, 3))
    if dim == 2:
        src[..., 2] = 0
    src[:, 0] = (300.0, -250.0, 0.0)                             # beyond +-128 m: the exhaustive path
    if n > 8:
        src[:, 1] = (45.0, 10.0, 0.0)                            # a dozen rings away from every row: settled by a late ring
        src[:, 2] = tgt[:, min(5, m - 1), :3] - np.array([0.25, -0.5, 0.0], np.float32)      # lands on the duplicated rows (pair 0: T is a shift)
        src[:, 3] = (3.5, 7.5, 0.0)                              # inside the crowded cell
        src[:, 4] = 0.0
    T = torch.eye(4).repeat(2, 1, 1)
    c, s = np.cos(0.03), np.sin(0.03)
    T[1, :2, :2] = torch.tensor([[c, -s], [s, c]], dtype=torch.float32)
    T[:, 0, 3], T[:, 1, 3] = 0.25, -0.5
    return torch.from_numpy(src), torch.from_numpy(tgt), T


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("n,m,k", [(257, 600, 4), (257, 600, 8), (1, 600, 8), (257, 8, 8), (257, 2, 2)])
def test_knn_search_matches_the_numpy_knn(dim, n, m, k):
    src, tgt, T = _knn_inputs(dim, n, m)
    idx, d2 = _knn_search(src.to(DEV), tgt.to(DEV), T.reshape(2, 16).contiguous().to(DEV), dim, k)
    p = torch.stack(transform_points(src, T, dim), dim=-1).numpy()
    ridx, rd2 = knn_ref_batch(p, tgt[..., :dim].numpy(), k, dim)
    assert np.array_equal(idx.numpy().astype(np.int64), ridx)
    assert np.array_equal(d2.numpy().view(np.int32), rd2.view(np.int32))
    if m >= 112 and n > 8:
        assert (rd2[:, 0, 0] > 128.0 ** 2).all()                                   # farther than GRID_RMAX rings reach
        assert (rd2[:, 1, 0] > 20.0 ** 2).all() and (rd2[:, 1, -1] < 33.0 ** 2).all()      # 10 .. 17 rings
        tie = idx[0, 2, :3].tolist()
        assert tie == [5, 40, 77] and d2[0, 2, 0] == d2[0, 2, 1] == d2[0, 2, 2]


# ----------------------------------------------------------------------------- 2. - 4. forward, gradients, zeros, run-to-run
@pytest.mark.parametrize("k", [4, 8])
@pytest.mark.parametrize("ci", range(len(CASES)), ids=IDS)
def test_softmin_matches_the_restatement(ci, k):
    case = CASES[ci]
    icp_type, _, dim, _, _ = case
    inp = inputs(case)
    run = gpu(case, inp, TRIM, softmin_k=k)
    assert run["fn"].startswith("_IcpSoftFunction") and tuple(run["idx"].shape) == (K, B, N, k)
    assert run["active"][:K].all()
    # forward: the first search is the free-running reference's; the pose is the replay's
    assert torch.equal(run["idx"][0].long(), first_neighbours(case, k))
    ref = reference(case, TRIM, fixed_idx=run["idx"], soft_k=k)
    assert_softmin_awake(case, ref)
    err = (run["T"].double() - ref["T"].double()).abs().max().item()
    print("POSE max abs diff = %.3e" % err)
    np.testing.assert_allclose(run["T"].numpy(), ref["T"].numpy(), atol=2e-6, rtol=0)
    # gradients: with the clouds (all four), without them (weight and T_init only)
    for name in NAMES:
        close(run["grads"][name], ref["grads"][name], name)
    two = gpu(case, inp, TRIM, need=("weight", "T_init"), softmin_k=k)
    assert torch.equal(two["T"], run["T"]) and torch.equal(two["idx"], run["idx"])
    assert two["grads"]["source"] is None and two["grads"]["target"] is None
    for name in ("weight", "T_init"):
        close(two["grads"][name], ref["grads"][name], name + " (no clouds)")
        assert torch.equal(two["grads"][name], run["grads"][name])
    # structural zeros
    gs, gt, gw = run["grads"]["source"], run["grads"]["target"], run["grads"]["weight"]
    if dim == 2:
        assert (gs[..., 2] == 0).all()
    assert (gt[..., dim:3] == 0).all()
    assert (gt[..., 3 + (dim if icp_type == "pt2pl" else 0):] == 0).all()
    for b in range(B):
        used = torch.zeros(M, dtype=torch.bool)
        used[run["idx"][:, b].reshape(-1).long()] = True
        assert (~used).any() and (gt[b, ~used] == 0).all()                       # targets never among any k
        assert (gt[b, M_REAL:] == 0).all()                                       # pad rows
        assert gt[b, used, :dim].abs().max() > 0
    assert (gs[:, N_REAL:] == 0).all()                                           # zero-weight rows
    assert torch.isfinite(gw).all() and torch.isfinite(gt).all() and torch.isfinite(gs).all()
    # run to run
    again = gpu(case, inp, TRIM, softmin_k=k)
    assert torch.equal(again["T"], run["T"]) and torch.equal(again["idx"], run["idx"])
    for name in NAMES:
        assert torch.equal(again["grads"][name], run["grads"][name]), name


# ----------------------------------------------------------------------------- 5. the nearest limit
@pytest.mark.parametrize("k", [4, 8])
@pytest.mark.parametrize("ci", [0, 1, 3], ids=[IDS[0], IDS[1], IDS[3]])
def test_nearest_limit_is_the_hard_grid_call(ci, k):
    case = CASES[ci]
    dim = case[2]
    inp = inputs(case)
    tau = 1e-12
    ICP.NN_SEARCH_OVERRIDE = "grid"
    try:
        hard = gpu(case, inp, TRIM)
    finally:
        ICP.NN_SEARCH_OVERRIDE = None
    soft = gpu(case, inp, TRIM, softmin_k=k, tau=tau)
    # the premise, on the device's own distances: (d_1 - d_0) / tau >= 120 on every real row of every iteration
    s, t = inp["x"][0].to(DEV), inp["x"][1].to(DEV)
    for it in range(K):
        idx, d2 = _knn_search(s, t, soft["T_hist"][it].contiguous().to(DEV), dim, k)
        assert torch.equal(idx, soft["idx"][it])
        gap = (d2[:, :N_REAL, 1].double() - d2[:, :N_REAL, 0].double()) / tau
        assert gap.min().item() >= 120, gap.min().item()
    assert torch.equal(soft["T"], hard["T"]) and torch.equal(soft["active"], hard["active"])
    assert torch.equal(soft["idx"][..., 0], hard["idx"])
    for name in ("weight", "source", "T_init"):
        assert torch.equal(soft["grads"][name], hard["grads"][name]), name
    a, b = soft["grads"]["target"].double(), hard["grads"]["target"].double()
    print("TARGET GRAD nearest limit: max abs diff %.3e (max %.3e)" % ((a - b).abs().max().item(), b.abs().max().item()))
    assert ((a - b).abs() <= 2.0 ** -22 * b.abs() + 2.0 ** -30 * b.abs().max()).all()


# ----------------------------------------------------------------------------- 6. correspondence: nearest
@pytest.mark.parametrize("ci", [1, 2], ids=[IDS[1], IDS[2]])
def test_nearest_is_bit_identical_to_a_call_that_never_mentions_it(nn_engine, ci, tmp_path):
    case = CASES[ci]
    inp = inputs(case)

    def by_attr(icp):
        icp.correspondence, icp.softmin_k, icp.softmin_temp = "nearest", 8, 1.0

    def by_yaml(icp):
        cfg = tmp_path / "dICP_config.yaml"
        cfg.write_text("dICP:\n  target_pad_val: 1000.0\n  parameters:\n    correspondence: nearest\n    softmin_k: 8\n    softmin_temp: 1.0\n")
        new = ICP(icp_type=icp.icp_type, config_path=str(cfg), differentiable=True, max_iterations=K, tolerance=TOL)
        assert (new.correspondence, new.softmin_k, new.nn_search) == ("nearest", 8, nn_engine)
        return new

    # the three backward entries: mmk_icp_backward (no clouds), mmk_icp_backward_points, mmk_icp_backward_hp (a tensor trim_dist)
    for need, trim in ((("weight", "T_init"), TRIM), (NAMES, TRIM), (NAMES, torch.tensor(TRIM))):
        plain = gpu(case, inp, trim, need=need)
        assert plain["fn"].startswith("_IcpHpFunction" if torch.is_tensor(trim) else "_IcpFunction")
        for configure in (by_attr, by_yaml):
            got = gpu(case, inp, trim, need=need, configure=configure)
            assert got["fn"] == plain["fn"]
            assert torch.equal(got["T"], plain["T"]) and torch.equal(got["idx"], plain["idx"]), configure.__name__
            assert torch.equal(got["active"], plain["active"])
            for name in need:
                assert torch.equal(got["grads"][name], plain["grads"][name]), (configure.__name__, name)
    soft = gpu(case, inp, TRIM, softmin_k=4)
    assert not torch.equal(soft["T"], plain["T"])                       # and the option is not a no-op
    # a call that is not differentiable keeps nearest correspondences, whatever the instance says
    icp = ICP(icp_type=case[0], differentiable=True, max_iterations=K, tolerance=TOL)
    x = [v.to(DEV) for v in inp["x"]]
    with torch.no_grad():
        T_plain = icp.icp(x[0], x[1], T_init=x[3], weight=x[2], trim_dist=TRIM, loss_fn=inp["loss_fn"], dim=case[2])["T"]
        icp.correspondence, icp.softmin_k, icp.softmin_temp = "softmin", 4, TAU
        T_soft = icp.icp(x[0], x[1], T_init=x[3], weight=x[2], trim_dist=TRIM, loss_fn=inp["loss_fn"], dim=case[2])["T"]
    assert torch.equal(T_plain, T_soft) and tuple(icp.last_state["idx"].shape) == (1, B, N)


def test_softmin_call_without_a_gradient_input_keeps_the_mode_and_the_pose():
    """differentiable=True with grad enabled but no input that requires grad: still soft correspondences, through the forward
    that saves no state (one (B,N,k) index buffer, the polled early exit), and the pose of the call that saves it."""
    case = CASES[1]
    inp = inputs(case)
    saved = gpu(case, inp, TRIM, softmin_k=4)
    icp = ICP(icp_type=case[0], differentiable=True, max_iterations=K, tolerance=TOL)
    icp.check_every = 2
    icp.correspondence, icp.softmin_k, icp.softmin_temp = "softmin", 4, TAU
    x = [v.to(DEV) for v in inp["x"]]
    T = icp.icp(x[0], x[1], T_init=x[3], weight=x[2], trim_dist=TRIM, loss_fn=inp["loss_fn"], dim=case[2])["T"]
    assert not T.requires_grad and tuple(icp.last_state["idx"].shape) == (1, B, N, 4)
    assert torch.equal(T.cpu(), saved["T"])
    assert torch.equal(icp.last_state["idx"][0].cpu(), saved["idx"][K - 1])


# ----------------------------------------------------------------------------- 7. the policy
def test_policy_softmin_trains_and_inference_stays_nearest(scene64):
    scan, mp, T0, G = scene64
    kw = dict(dropout=0.0, mask_target="scan")

    def step(model):
        model.train()
        T, _, _ = model(scan, mp, T0)
        (T * G).sum().backward()
        return T.detach(), [q.grad.detach().clone() if q.grad is not None else None for q in model.parameters()]

    soft_model, hard_model = policy(DEV, 3, icp_correspondence="softmin", **kw), policy(DEV, 3, **kw)
    assert soft_model.ICP_alg.correspondence == "softmin" and soft_model.ICP_alg_inference.correspondence == "nearest"
    T_soft, g_soft = step(soft_model)
    T_hard, g_hard = step(hard_model)
    assert torch.isfinite(T_soft).all() and not torch.equal(T_soft, T_hard)
    assert all(g is not None and torch.isfinite(g).all() for g in g_soft) and any(g.abs().max() > 0 for g in g_soft)
    assert any(not torch.equal(a, b) for a, b in zip(g_soft, g_hard))
    # evaluation: the inference instance keeps nearest correspondences -- the bits it gives today
    soft_model.eval(), hard_model.eval()
    with torch.no_grad():
        Te_soft, Te_hard = soft_model(scan, mp, T0)[0], hard_model(scan, mp, T0)[0]
    assert torch.equal(Te_soft, Te_hard)
