"""GPU: the soft (tanh) trim gate of the HIP dICP (mmk_icp_params.trim_steep; DESIGN.md §3 I3', I7') against the restatement
tests/dicp_restatement.py: forward, the gradients of source, target, weight and T_init from both backward entries,
structural zeros, bit reproducibility, the untouched hard gate, the stand-alone accumulate stage, a coincident point and the
policy's params["icp_trim"].

The reference REPLAYS the correspondences of the GPU run (fixed_idx): device and host tanhf may differ in the last bit, and a
flipped near-tie of a later search must not turn that into a failure.  idx_hist[0], found before the first solve, is compared
bit for bit with the free-running reference.

Shapes: B = 2, 300 + 20 zero source rows (one full and one partial 256-thread block), 700 + 30 target_pad_val rows, K = 4.
Every case asserts on the reference's own values that the gate works in its band (0.05 < keep < 0.95 for a tenth at least of
the real points in every iteration), that Huber is past its knee for 30 % of them, and that no pair froze.

Tolerances: pose 2e-6 absolute and gradients 2e-3 of the reference's largest magnitude, the bounds of
tests/test_gpu_point_grads.py.  The accumulate stage: the gate of a point is off by at most 2^-23 absolutely (tanhf within 2
ulp of a value below 1, halved, plus the rounding of 0.5 - 0.5 th), every other factor is the same fp32 arithmetic, so an entry
of A or b differs by at most 2^-23 sum_i weight_i rho_i |J_m J_n| (|J_m e|); asserted at twice that, 2^-22, for the fp64 sums'
own rounding and the products' (weight keep) rho roundings that a different last bit of keep moves.

Measured on an MI355X (both engines, all cases): pose within 2.4e-7 of the replay; gradients within 9.4e-6 of the reference's
largest magnitude (pt2pl Huber, weight; every other case below 1e-6); the stage's A and b within 1.1e-8 of the sum of their
terms' magnitudes.
"""
import ctypes

import numpy as np
import pytest
import torch

from mm_masking_amd import _lib
from mm_masking_amd.dICP.ICP import ICP

from dicp_cases import (B, GATE_CASES as CASES, GATE_IDS as IDS, GATE_TRIM as TRIM, K, M, M_REAL, N, N_REAL, NAMES, REAL, TOL,
                        assert_gate_awake, close, gpu, inputs, nn_engine, reference)  # noqa: F401
from dicp_restatement import as_bn, band_share, per_point_terms
from radar_cases import scene64  # noqa: F401  (the smallest scan-mode batch of the suite, a module fixture)
from support import DEV, policy

pytestmark = pytest.mark.gpu


# ----------------------------------------------------------------------------- 1. - 4. forward, gradients, zeros, run-to-run
@pytest.mark.parametrize("ci", range(len(CASES)), ids=IDS)
def test_soft_gate_matches_the_restatement(nn_engine, ci):
    case = CASES[ci]
    icp_type, _, dim, _, _ = case
    inp = inputs(case)
    run = gpu(case, inp, TRIM)
    assert run["active"][:K].all()
    # 1. forward: the first search is the free-running reference's; the pose is the replay's
    assert torch.equal(run["idx"][0].long(), reference(case, TRIM, differentiable=False, K_=1)["hist"]["idx"][0].long())
    ref = reference(case, TRIM, fixed_idx=run["idx"])
    assert_gate_awake(case, ref)
    err = (run["T"].double() - ref["T"].double()).abs().max().item()
    print("POSE max abs diff = %.3e" % err)
    np.testing.assert_allclose(run["T"].numpy(), ref["T"].numpy(), atol=2e-6, rtol=0)
    # 2. gradients: mmk_icp_backward_points (all four), mmk_icp_backward (weight and T_init only)
    for name in NAMES:
        close(run["grads"][name], ref["grads"][name], name)
    two = gpu(case, inp, TRIM, need=("weight", "T_init"))
    assert torch.equal(two["T"], run["T"]) and torch.equal(two["idx"], run["idx"])
    assert two["grads"]["source"] is None and two["grads"]["target"] is None
    for name in ("weight", "T_init"):
        close(two["grads"][name], ref["grads"][name], name + " (mmk_icp_backward)")
        assert torch.equal(two["grads"][name], run["grads"][name])
    # 3. structural zeros, as with the hard gate
    gs, gt, gw = run["grads"]["source"], run["grads"]["target"], run["grads"]["weight"]
    if dim == 2:
        assert (gs[..., 2] == 0).all()
    assert (gt[..., dim:3] == 0).all()
    assert (gt[..., 3 + (dim if icp_type == "pt2pl" else 0):] == 0).all()
    for b in range(B):
        used = torch.zeros(M, dtype=torch.bool)
        for k in range(K):
            used[run["idx"][k, b].long()] = True
        assert (~used).any() and (gt[b, ~used] == 0).all()
        assert not used[M_REAL:].any() and (gt[b, M_REAL:] == 0).all()          # pad rows: never a correspondent
        assert gt[b, used, :dim].abs().max() > 0
    assert (gs[:, N_REAL:] == 0).all()                                           # zero-weight rows: nothing through omega
    assert torch.isfinite(gw).all()
    # 4. run to run
    again = gpu(case, inp, TRIM)
    assert torch.equal(again["T"], run["T"]) and torch.equal(again["idx"], run["idx"])
    for name in NAMES:
        assert torch.equal(again["grads"][name], run["grads"][name]), name


# ----------------------------------------------------------------------------- 5. gate off
@pytest.mark.parametrize("ci", [1, 2], ids=[IDS[1], IDS[2]])
def test_gate_off_is_bit_identical_to_a_call_that_never_mentions_it(nn_engine, ci, tmp_path):
    case = CASES[ci]
    inp = inputs(case)
    plain = gpu(case, inp, TRIM, gate=False)                                            # never mentions the option

    def hard_attr(icp):
        icp.trim, icp.tanh_steepness = "hard", 4.0

    def hard_yaml(icp):
        cfg = tmp_path / "dICP_config.yaml"
        cfg.write_text("dICP:\n  target_pad_val: 1000.0\n  parameters:\n    trim: hard\n    tanh_steepness: 4.0\n")
        new = ICP(icp_type=icp.icp_type, config_path=str(cfg), differentiable=True, max_iterations=K, tolerance=TOL)
        assert new.trim == "hard" and new.tanh_steepness == 4.0
        return new

    class ZeroSteep(ICP):                                               # trim_steep = 0 written into the struct by hand
        def _params(self, *a, **kw):
            p = super()._params(*a, **kw)
            p.trim_steep = 0.0
            return p

    def zero_steep(icp):
        new = ZeroSteep(icp_type=icp.icp_type, differentiable=True, max_iterations=K, tolerance=TOL)
        new.trim, new.tanh_steepness = "tanh", 4.0
        return new

    for configure in (hard_attr, hard_yaml, zero_steep):
        got = gpu(case, inp, TRIM, gate=False, configure=configure)
        assert torch.equal(got["T"], plain["T"]) and torch.equal(got["idx"], plain["idx"]), configure.__name__
        assert torch.equal(got["active"], plain["active"])
        for name in NAMES:
            assert torch.equal(got["grads"][name], plain["grads"][name]), (configure.__name__, name)
    soft = gpu(case, inp, TRIM)
    assert not torch.equal(soft["T"], plain["T"])                       # and the option is not a no-op


# ----------------------------------------------------------------------------- 6. the stand-alone stage
@pytest.mark.parametrize("ci", [1, 2], ids=[IDS[1], IDS[2]])
def test_accumulate_stage_with_the_soft_gate(ci):
    case = CASES[ci]
    icp_type, _, dim, _, steep = case
    inp = inputs(case)
    L = _lib.lib()
    s, t, wt, T0 = (v.to(DEV).contiguous() for v in inp["x"])
    Tt = T0.reshape(B, 16).contiguous()
    icp = ICP(icp_type, differentiable=False, max_iterations=1, tolerance=0.0)
    icp.trim, icp.tanh_steepness = "tanh", steep
    p = icp._params(B, N, M, 6, dim, inp["loss_fn"], TRIM, save_state=False)
    assert p.trim_steep == steep
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
    ic = idx_out.cpu().long()
    loss_name, loss_k = (None, 1.0) if case[1] is None else case[1]
    kk, cc, ss = (as_bn(v, B, torch.float32) for v in (loss_k, TRIM, steep))
    J, e, wref, _, aux = per_point_terms(src, tgt, T0c, ic, w, icp_type, loss_name, kk, cc, ss, dim, True)
    assert band_share(aux["keep"], REAL) >= 0.10
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
    print("STAGE %s: |A - ref| / sum|terms| = %.3e, |b - ref| / sum|terms| = %.3e (bound %.3e)" % (IDS[ci], ra, rb, bound))
    assert ((A - A_ref).abs() <= bound * A_abs).all() and ((bvec - b_ref).abs() <= bound * b_abs).all()
    # the hard gate on the same keys gives other sums: the stage reads the field
    p0 = icp._params(B, N, M, 6, dim, inp["loss_fn"], TRIM, save_state=False)
    p0.trim_steep = 0.0
    parts0 = torch.zeros_like(parts)
    _lib.check(L.mmk_icp_accumulate(ctypes.byref(p0), _lib.ptr(s), _lib.ptr(t), _lib.ptr(wt), _lib.ptr(Tt), _lib.ptr(keys),
                                    _lib.ptr(idx_out), _lib.ptr(parts0), _lib.ptr(status), st))
    torch.cuda.synchronize()
    assert not torch.equal(parts0, parts)


# ----------------------------------------------------------------------------- 7. a coincident point
@pytest.mark.parametrize("ci", [0, 1, 3], ids=[IDS[0], IDS[1], IDS[3]])
def test_coincident_point_keeps_every_gradient_finite(nn_engine, ci):
    case = CASES[ci]
    inp = inputs(case, coincident=True)
    run = gpu(case, inp, TRIM)
    assert (run["idx"][0][:, 5] == 11).all()                    # d == 0 in the first iteration
    for name in NAMES:
        g = run["grads"][name]
        assert torch.isfinite(g).all() and g.abs().max() > 0, name


# ----------------------------------------------------------------------------- 8. the policy
def test_policy_soft_gate_trains_and_inference_stays_hard(scene64):
    """mask_target="scan": one training step with params["icp_trim"] = "tanh".  The points of this scene lie 0.09 .. 0.15 m
    from their correspondents, so a trim distance of 0.12 m puts them inside the gate's band (steepness 10: |argument| < 0.4)."""
    scan, mp, T0, G = scene64
    kw = dict(dropout=0.0, mask_target="scan", icp_trim_dist=0.12)

    def step(model):
        model.train()
        T, _, _ = model(scan, mp, T0)
        (T * G).sum().backward()
        return T.detach(), [q.grad.detach().clone() for q in model.parameters()]

    soft_model, hard_model = policy(DEV, 3, icp_trim="tanh", **kw), policy(DEV, 3, **kw)
    assert soft_model.ICP_alg.trim == "tanh" and soft_model.ICP_alg_inference.trim == "hard"
    T_soft, g_soft = step(soft_model)
    T_hard, g_hard = step(hard_model)
    assert torch.isfinite(T_soft).all() and not torch.equal(T_soft, T_hard)
    assert all(torch.isfinite(g).all() for g in g_soft) and any(g.abs().max() > 0 for g in g_soft)
    assert any(not torch.equal(a, b) for a, b in zip(g_soft, g_hard))
    # evaluation: the inference instance keeps the hard gate
    soft_model.eval(), hard_model.eval()
    with torch.no_grad():
        Te_soft, Te_hard = soft_model(scan, mp, T0)[0], hard_model(scan, mp, T0)[0]
    assert torch.equal(Te_soft, Te_hard)
