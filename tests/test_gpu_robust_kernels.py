"""GPU: the Geman-McClure and Welsch kernels of the HIP dICP (MMK_LOSS_GEMAN_MCCLURE, MMK_LOSS_WELSCH; DESIGN.md §3 I3, I7,
I7'') through every path Cauchy and Huber have, against the restatement tests/dicp_restatement.py: nearest correspondences on
both NN engines and both backward shapes, the device-resident scale and its gradient, soft correspondences with the
temperature a number and a tensor, the stand-alone accumulate stage, the status bit and the policy.

Shapes, inputs, ``close`` and the launch helper ``gpu`` are those of tests/dicp_cases.py (imported from it): B = 2, 300 + 20
zero source rows (one full and one partial 256-thread block), 700 + 30 target_pad_val rows, K = 4, T_init shifted by 0.2 m,
trim_dist 1.0.  In the per-pair runs pair 1 uses k x 1.3.

The reference REPLAYS the device's idx_hist: device and host expf may differ in the last bit, and a flipped near-tie of a later
search must not turn that into a failure.  idx_hist[0], found before any rho is evaluated, is compared bit for bit with the
free-running search.  The reference runs once per (case, correspondences, values) with the scale as a (B,N) leaf: its gradient
is every point's contribution summed over the iterations, the fp64 row sums g_b are the per-pair references and S_b = sum
|contributions|.

Conditions asserted on the reference's own values in every case: no pair froze; in every iteration at least 30 % of the real
points pass the gate (keep > 0.5) AND have 0.05 < rho < 0.95 (the kernel is neither off nor saturated); the scale's gradient
is awake, max_b |g_b| / S_b >= 0.03 (tests/test_gpu_icp_hyper.py's threshold).  tests/test_robust_kernels_cpu.py asserts the
same on the free run, without a GPU.

Tolerances: pose 2e-6 absolute, gradients 2e-3 of the reference's largest magnitude per input (tests/test_gpu_point_grads.py).
Equalities are exact.  The stage: |A - ref| and |b - ref| within 2^-22 of the sum of the terms' magnitudes with the gate taken
as 1 (tests/test_gpu_soft_trim.py's bound for the same stage).

No vector of a Cauchy or Huber call at these shapes is stored under tests/golden, so "unchanged ground" is what the existing
suite asserts, unmodified: this file generates no fixture from the code under test.

Measured on an MI355X (all six cases, both engines, soft correspondences over 4 and 8 rows): pose within 1.2e-6 of the replay
(soft correspondences; nearest: 3.0e-8); gradients within 2.8e-5 of the reference's largest magnitude for the four inputs
(weight 2.8e-5, source 2.6e-5, target 2.6e-5, T_init 1.7e-5, all with soft correspondences; nearest: 1.5e-6 at most), the scale k
within 6.7e-7, trim_dist 5.7e-7 and the steepness 1.4e-6 under the tanh gate, tau 6.2e-5.  Welsch sits with Geman-McClure: device
expf against torch.exp does not show at these bounds.  Band share per iteration 0.32 (pt2pl Welsch dim 2, first iteration) to
0.95; the scale's awake ratio max_b |g_b| / S_b 0.077 (pt2pt Geman-McClure dim 2, 8 soft rows) to 0.518, the smallest single
pair 0.036; the smallest step norm 0.0095 against the tolerance 1e-9.  The stage: |A - ref| and |b - ref| at 3.6e-16 and
1.1e-16 of the sum of the terms' magnitudes (bound 2.4e-7).  The policy's gradient of icp_metric (Welsch, 0.5) on scene64:
4.2714e-17 -- this scene's ICP converges to residuals near 0, which no weighting moves (tests/test_gpu_icp_hyper.py finds
1e-14 .. 1e-11 for Cauchy there).
"""
import ctypes

import numpy as np
import pytest
import torch

from mm_masking_amd import _lib
from mm_masking_amd.dICP.ICP import ICP, check_errors

from dicp_cases import (B, HARD_STEEP, K, M, M_REAL, N, N_REAL, NAMES, PER_PAIR_TAU, REAL, ROBUST_CASES as CASES, ROBUST_IDS as IDS,
                        ROBUST_TRIM as TRIM, K_MULT, TAU, TOL, assert_awake, close, first_neighbours, gpu, inputs, nn_engine,
                        reference, same)  # noqa: F401
from dicp_restatement import per_point_terms
from radar_cases import scene64  # noqa: F401  (the smallest scan-mode batch of the suite, a module fixture)
from support import DEV, policy

pytestmark = pytest.mark.gpu


def _pose(run, ref):
    err = (run["T"].double() - ref["T"].double()).abs().max().item()
    print("POSE max abs diff = %.3e" % err)
    np.testing.assert_allclose(run["T"].numpy(), ref["T"].numpy(), atol=2e-6, rtol=0)


def k_values(case, per_pair):
    """(k of pair 0, k of pair 1) as an fp32 tensor."""
    k0 = case[1][1]
    return torch.tensor([k0, k0 * K_MULT if per_pair else k0], dtype=torch.float32)


def _gpu_hp(case, inp, hyper, need, gate):
    return gpu(case, inp, hyper[1], need=need, gate=gate, k=hyper[0], steep=hyper[2])


def _hyper(case, ks, tensors):
    """The (k, trim_dist, steepness) triple and the gate of a launch with the scale on the device; ``tensors``: trim_dist and
    the steepness as (B,) tensors of the case's values (the tanh cases)."""
    steep = case[4]
    if steep > 0:
        if tensors:
            return [ks, torch.full((B,), TRIM), torch.full((B,), steep)], "tanh"
        return [ks, TRIM, steep], "tanh"
    return [ks, TRIM, HARD_STEEP], "hard"


# ----------------------------------------------------------------------------- 1. nearest correspondences
@pytest.mark.parametrize("ci", range(len(CASES)), ids=IDS)
def test_nearest_matches_the_restatement(nn_engine, ci):
    case = CASES[ci]
    icp_type, _, dim, _, _ = case
    inp = inputs(case)
    run = gpu(case, inp, TRIM)                                 # all four: mmk_icp_backward_points
    assert run["fn"].startswith("_IcpFunction") and tuple(run["idx"].shape) == (K, B, N) and run["active"][:K].all()
    free = reference(case, TRIM, differentiable=False)
    assert torch.equal(run["idx"][0].long(), free["hist"]["idx"][0].long())
    ref = reference(case, TRIM, fixed_idx=run["idx"])
    assert_awake(ref, "%s nearest" % IDS[ci])
    _pose(run, ref)
    for name in NAMES:
        close(run["grads"][name], ref["grads"][name], name)
    two = gpu(case, inp, TRIM, need=("weight", "T_init"))     # without the clouds: mmk_icp_backward
    assert torch.equal(two["T"], run["T"]) and torch.equal(two["idx"], run["idx"])
    assert two["grads"]["source"] is None and two["grads"]["target"] is None
    for name in ("weight", "T_init"):
        close(two["grads"][name], ref["grads"][name], name + " (no clouds)")
    # structural zeros
    gs, gt, gw = run["grads"]["source"], run["grads"]["target"], run["grads"]["weight"]
    if dim == 2:
        assert (gs[..., 2] == 0).all()
    assert (gt[..., dim:3] == 0).all()
    assert (gt[..., 3 + (dim if icp_type == "pt2pl" else 0):] == 0).all()
    for b in range(B):
        used = torch.zeros(M, dtype=torch.bool)
        used[run["idx"][:, b].reshape(-1).long()] = True
        assert (~used).any() and (gt[b, ~used] == 0).all()                       # targets never matched
        assert (gt[b, M_REAL:] == 0).all()                                       # pad rows
        assert gt[b, used, :dim].abs().max() > 0
    assert (gs[:, N_REAL:] == 0).all()                                           # zero-weight rows
    assert torch.isfinite(gw).all() and torch.isfinite(gt).all() and torch.isfinite(gs).all()
    # run to run
    again = gpu(case, inp, TRIM)
    same(again, run, NAMES)


# ----------------------------------------------------------------------------- 2. the scale on the device
@pytest.mark.parametrize("ci", range(len(CASES)), ids=IDS)
def test_device_scale_and_its_gradient(ci):
    case = CASES[ci]
    tanh = case[4] > 0
    inp = inputs(case)
    # a (B,) tensor with the number call's values gives the number call's bits
    plain = gpu(case, inp, TRIM)
    hyper, gate = _hyper(case, k_values(case, False), False)
    per = _gpu_hp(case, inp, hyper, need=NAMES + ("k",), gate=gate)
    assert per["fn"] == "_IcpHpFunctionBackward"
    same(per, plain, NAMES)
    # per-pair values against the restatement, the metric's gradient included; under the tanh gate trim_dist's and the
    # steepness's too
    ks = k_values(case, True)
    hyper, gate = _hyper(case, ks, True)
    need = NAMES + (("k", "trim_dist", "trim_steep") if tanh else ("k",))
    run = _gpu_hp(case, inp, hyper, need=need, gate=gate)
    assert run["active"][:K].all() and not torch.equal(run["T"][1], plain["T"][1])
    ref = reference(case, TRIM, fixed_idx=run["idx"], mult=(K_MULT, 1.0, 1.0))
    assert_awake(ref, "%s per-pair k" % IDS[ci])
    _pose(run, ref)
    for name in need:
        assert run["grads"][name].shape == ref["grads"][name].shape
        close(run["grads"][name], ref["grads"][name], name)
    two = _gpu_hp(case, inp, hyper, need=("weight", "T_init", "k"), gate=gate)      # the other backward shape
    same(two, run, ("weight", "T_init", "k"))
    # a shared value gets the fp32 rounding of the fp64 sum of the pairs' rows
    want = per["grads"]["k"].double().sum().float()
    for shape in ((), (1,)):
        hyper, gate = _hyper(case, k_values(case, False)[0].reshape(shape), False)
        shared = _gpu_hp(case, inp, hyper, need=NAMES + ("k",), gate=gate)
        same(shared, per, NAMES)
        assert shared["grads"]["k"].shape == shape and torch.equal(shared["grads"]["k"].reshape(()), want)
    again = _gpu_hp(case, inp, _hyper(case, ks, True)[0], need=need, gate=gate)
    same(again, run, need)


# ----------------------------------------------------------------------------- 3. soft correspondences
@pytest.mark.parametrize("k", [4, 8])
@pytest.mark.parametrize("ci", range(len(CASES)), ids=IDS)
def test_soft_correspondences_match_the_restatement(ci, k):
    case = CASES[ci]
    inp = inputs(case)
    free0 = first_neighbours(case, k)
    # tau a number
    run = gpu(case, inp, TRIM, softmin_k=k)
    assert run["fn"].startswith("_IcpSoftFunction") and tuple(run["idx"].shape) == (K, B, N, k) and run["active"][:K].all()
    assert torch.equal(run["idx"][0].long(), free0)
    ref = reference(case, TRIM, fixed_idx=run["idx"], soft_k=k)
    assert_awake(ref, "%s softmin k=%d tau=%g" % (IDS[ci], k, TAU))
    _pose(run, ref)
    for name in NAMES:
        close(run["grads"][name], ref["grads"][name], name)
    two = gpu(case, inp, TRIM, need=("weight", "T_init"), softmin_k=k)
    assert torch.equal(two["T"], run["T"]) and torch.equal(two["idx"], run["idx"])
    for name in ("weight", "T_init"):
        assert torch.equal(two["grads"][name], run["grads"][name])
    # tau a (B,) tensor
    ten = gpu(case, inp, TRIM, need=NAMES + ("tau",), softmin_k=k, tau=torch.tensor(PER_PAIR_TAU))
    assert ten["fn"] == "_IcpSoftTempFunctionBackward" and ten["active"][:K].all()
    assert torch.equal(ten["idx"][0].long(), free0)
    tref = reference(case, TRIM, fixed_idx=ten["idx"], soft_k=k, taus=PER_PAIR_TAU)
    assert_awake(tref, "%s softmin k=%d tau=%s" % (IDS[ci], k, PER_PAIR_TAU))
    _pose(ten, tref)
    for name in NAMES + ("tau",):
        assert ten["grads"][name].shape == tref["grads"][name].shape
        close(ten["grads"][name], tref["grads"][name], name)


# ----------------------------------------------------------------------------- 4. the stand-alone stage
def test_accumulate_stage_with_geman_mcclure():
    case = CASES[0]
    icp_type, (name, k0), dim, _, steep = case
    inp = inputs(case)
    L = _lib.lib()
    s, t, wt, T0 = (v.to(DEV).contiguous() for v in inp["x"])
    Tt = T0.reshape(B, 16).contiguous()
    icp = ICP(icp_type, differentiable=False, max_iterations=1, tolerance=0.0)
    p = icp._params(B, N, M, 6, dim, inp["loss_fn"], TRIM, save_state=False)
    assert p.loss == 3 and p.trim_steep == 0.0
    st = _lib.stream_ptr(DEV)
    Mpad = L.mmk_nn_padded_m(M)
    planar = torch.empty(B, dim, Mpad, dtype=torch.float32, device=DEV)
    _lib.check(L.mmk_pack_target(_lib.ptr(t), B, M, 6, dim, _lib.ptr(planar), st))
    ws = torch.empty(L.mmk_nn_workspace_bytes(B, N, M, dim), dtype=torch.uint8, device=DEV)
    idx = torch.empty(B, N, dtype=torch.int32, device=DEV)
    d2 = torch.empty(B, N, dtype=torch.float32, device=DEV)
    _lib.check(L.mmk_nn_search(_lib.ptr(s), _lib.ptr(planar), _lib.ptr(Tt), B, N, M, dim, _lib.ptr(idx), _lib.ptr(d2),
                               _lib.ptr(ws), ws.numel(), st))
    keys = (d2.view(torch.int32).to(torch.int64) << 32) | idx.to(torch.int64)
    n_part = L.mmk_icp_partials_count(ctypes.byref(p))
    nblk, nacc, P = (N + 255) // 256, (9 if dim == 2 else 27), (3 if dim == 2 else 6)
    assert n_part == B * nblk * nacc
    parts = torch.zeros(n_part, dtype=torch.float64, device=DEV)
    idx_out = torch.full((B, N), -7, dtype=torch.int32, device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    _lib.check(L.mmk_icp_accumulate(ctypes.byref(p), _lib.ptr(s), _lib.ptr(t), _lib.ptr(wt), _lib.ptr(Tt), _lib.ptr(keys),
                                    _lib.ptr(idx_out), _lib.ptr(parts), _lib.ptr(status), st))
    torch.cuda.synchronize()
    assert int(status.item()) == 0 and torch.equal(idx_out, idx)
    acc = parts.view(B, nblk, nacc).sum(dim=1).cpu()
    iu = torch.triu_indices(P, P)
    A = torch.zeros(B, P, P, dtype=torch.float64)
    A[:, iu[0], iu[1]] = acc[:, :P * (P + 1) // 2]
    A = torch.triu(A) + torch.triu(A, 1).transpose(1, 2)
    bvec = acc[:, P * (P + 1) // 2:]

    src, tgt, w, T0c = inp["x"]
    one = torch.ones(1, 1)
    J, e, wref, _, aux = per_point_terms(src, tgt, T0c, idx_out.cpu().long(), w, icp_type, name, one * k0, one * TRIM,
                                         one * HARD_STEEP, dim, False)
    band = float(((aux["keep"] > 0.5) & (aux["rho"] > 0.05) & (aux["rho"] < 0.95))[REAL].double().mean())
    assert band >= 0.30, band
    Jd, ed = J.double(), e.double()
    wJ = (wref[..., None, None] * J).double()
    A_ref = torch.einsum("bnrp,bnrq->bpq", wJ, Jd)
    A_ref = torch.triu(A_ref) + torch.triu(A_ref, 1).transpose(1, 2)
    b_ref = torch.einsum("bnrp,bnr->bp", wJ, ed)
    w_open = ((w * aux["rho"])[..., None, None] * J).double().abs()             # the gate taken as 1
    A_abs = torch.einsum("bnrp,bnrq->bpq", w_open, Jd.abs())
    A_abs = torch.triu(A_abs) + torch.triu(A_abs, 1).transpose(1, 2)
    b_abs = torch.einsum("bnrp,bnr->bp", w_open, ed.abs())
    bound = 2.0 ** -22
    ra = ((A - A_ref).abs() / A_abs.clamp_min(1e-300)).max().item()
    rb = ((bvec - b_ref).abs() / b_abs.clamp_min(1e-300)).max().item()
    print("STAGE %s: |A - ref| / sum|terms| = %.3e, |b - ref| / sum|terms| = %.3e (bound %.3e)" % (IDS[0], ra, rb, bound))
    assert ((A - A_ref).abs() <= bound * A_abs).all() and ((bvec - b_ref).abs() <= bound * b_abs).all()
    # Cauchy on the same keys gives other sums: the stage reads the code
    p.loss = 1
    parts1 = torch.zeros_like(parts)
    _lib.check(L.mmk_icp_accumulate(ctypes.byref(p), _lib.ptr(s), _lib.ptr(t), _lib.ptr(wt), _lib.ptr(Tt), _lib.ptr(keys),
                                    _lib.ptr(idx_out), _lib.ptr(parts1), _lib.ptr(status), st))
    torch.cuda.synchronize()
    assert not torch.equal(parts1, parts)


# ----------------------------------------------------------------------------- 5. the status bit
@pytest.mark.parametrize("name", ["geman_mcclure", "welsch"])
def test_bad_scale_on_the_device_raises_the_status_bit_and_nothing_else(name):
    case = CASES[0]
    inp = inputs(case)
    check_errors(wait=True)
    icp = ICP(icp_type=case[0], differentiable=False, max_iterations=2, tolerance=TOL)
    s, t, w, T0 = (v.to(DEV) for v in inp["x"])

    def call(k):
        return icp.icp(s, t, T_init=T0, weight=w, trim_dist=TRIM, loss_fn={"name": name, "metric": k}, dim=case[2])["T"]

    for bad in (torch.tensor(0.0, device=DEV), torch.tensor([0.5, float("nan")], device=DEV)):    # (one bad pair is enough)
        call(bad)
        with pytest.raises(_lib.MmkError, match="MMK_ICP_STATUS_BAD_HYPER"):
            check_errors(wait=True)
        good = call(torch.tensor(0.5, device=DEV))                  # a flag, not a fault: the next call is clean
        check_errors(wait=True)
        assert torch.isfinite(good).all()
        assert torch.equal(good, call(0.5))                         # and it is the number call
    for bad in (0.0, -1.0, float("nan")):                           # a number is refused on the host
        with pytest.raises((_lib.MmkError, ValueError), match="metric"):
            call(bad)
    check_errors(wait=True)


# ----------------------------------------------------------------------------- 7. the policy
def test_policy_learns_the_welsch_scale(scene64):
    """One training step with icp_loss_fn = Welsch at 0.5 and learn_icp=("metric",): a finite, non-zero gradient of
    icp_metric (printed; 4.2714e-17 on an MI355X); the inference instance runs with the same kernel and nearest
    correspondences."""
    scan, mp, T0, G = scene64
    kw = dict(dropout=0.0, mask_target="scan", icp_loss_fn={"name": "welsch", "metric": 0.5})
    model, plain = policy(DEV, 3, learn_icp=("metric",), **kw), policy(DEV, 3, **kw)
    assert [n for n, _ in model.named_parameters() if n.startswith("icp_")] == ["icp_metric"]
    model.train(), plain.train()
    T, _, _ = model(scan, mp, T0)
    Tp, _, _ = plain(scan, mp, T0)
    assert torch.isfinite(T).all() and torch.equal(T.detach(), Tp.detach())      # the pose without learn_icp, bit for bit
    (T * G).sum().backward()
    g = model.icp_metric.grad
    print("POLICY icp_metric = %.4f (welsch), grad %.4e" % (model.icp_metric.item(), g.item()))
    assert g.shape == () and g.is_cuda and torch.isfinite(g) and g != 0
    check_errors(wait=True)
    # evaluation: the inference instance, nearest correspondences, the same kernel and scale
    model.eval(), plain.eval()
    with torch.no_grad():
        Te, Tpe = model(scan, mp, T0)[0], plain(scan, mp, T0)[0]
    check_errors(wait=True)
    assert torch.isfinite(Te).all() and torch.equal(Te, Tpe)
    assert model.ICP_alg_inference.correspondence == "nearest" and model.icp_loss_fn["name"] == "welsch"
