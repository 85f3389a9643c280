"""CPU: the Geman-McClure and Welsch kernels of the dICP (DESIGN.md §3 I3, I7, I7'').  The host plumbing -- the two codes in the
header, the binding and the C ABI's parameter validation, dICP.ICP's mapping of the names, the policy's ``learn_icp=("metric",)``
-- and the restatement tests/dicp_restatement.py: its bits against oracle.dicp_ref's under the hard gate for the kernels the
oracle has, Geman-McClure as the bit-exact square of Cauchy, the closed forms of the new chains against fp64 autograd, fp64 finite
differences, and the awake figures of tests/test_gpu_robust_kernels.py's cases on the restatement's free run, so that a
drifting input fails here, without a GPU.

Awake figures of a run (``assert_awake`` of tests/dicp_cases.py): no pair froze; in every iteration at least 30 % of the real
points pass the gate and have 0.05 < rho < 0.95; the scale's gradient max_b |g_b| / S_b >= 0.03.  Free run, all six cases, nearest
correspondences with k = (k0, k0) and (k0, 1.3 k0), soft correspondences (4 and 8 rows) with tau = (0.25, 0.25) and (0.25, 0.4):
band share per iteration 0.32 (pt2pl Welsch dim 2, first iteration) to 0.95, the awake ratio's maximum over the pairs 0.077
(pt2pt Geman-McClure dim 2, 8 soft rows) to 0.518, the smallest single pair 0.036, the smallest step norm 0.0095 against the
tolerance 1e-9.  The figures are printed.
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from mm_masking_amd import _lib, synthetic
from mm_masking_amd.dICP.ICP import ICP

from oracle.dicp_ref import ICPRef

from dicp_cases import (K_MULT, NAMES, PER_PAIR_TAU, ROBUST_CASES as GPU_CASES, ROBUST_IDS as GPU_IDS, ROBUST_TRIM, TAU, TOL,
                        assert_awake, inputs, policy_params, reference)
from dicp_cases import K as GPU_K
from dicp_restatement import ICPRestatement, closed_form_r2bar, closed_form_sums, per_point_terms
from support import ROOT, icp_params
NEW = {"geman_mcclure": 3, "welsch": 4}
B, N, M, K = 2, 70, 160, 3
TRIM, STEEP = 0.6, 4.0


# ----------------------------------------------------------------------------- the C ABI
@pytest.fixture(scope="module")
def L():
    _lib.build()
    return _lib.lib()


def test_header_and_binding_name_the_two_codes(L):
    raw = open(os.path.join(ROOT, "include", "mmk.h")).read()
    for name, code in NEW.items():
        assert int(re.search(r"#define\s+MMK_LOSS_%s\s+(\d+)" % name.upper(), raw).group(1)) == code == _lib.LOSSES[name]
    assert _lib.LOSSES == {None: 0, "none": 0, "l2": 0, "cauchy": 1, "huber": 2, "geman_mcclure": 3, "welsch": 4}
    assert L.mmk_version() == 502 and ctypes.sizeof(_lib.IcpParams) == L.mmk_icp_params_bytes() == 60


def test_parameter_validation_accepts_the_new_codes_and_nothing_beyond(L):
    null, fake = ctypes.c_void_p(0), ctypes.c_void_p(4096)       # never dereferenced: every call fails before any launch
    iters = ctypes.c_int(0)

    def forward(p):
        return L.mmk_icp_forward(ctypes.byref(p), *([fake] * 10), fake, 1 << 30, ctypes.byref(iters), null)

    for code in NEW.values():
        for kw in ({}, {"trim_steep": 4.0}, {"dim": 3, "loss_k": 0.2}):
            p = icp_params(loss=code, **kw)
            r = ctypes.byref(p)
            assert L.mmk_icp_workspace_bytes(r) > 0 and L.mmk_icp_backward_points_workspace_bytes(r, 1) > 0
            assert L.mmk_icp_backward_hp_workspace_bytes(r, 1, 1) > 0 and L.mmk_icp_partials_count(r) > 0
            assert L.mmk_icp_workspace_bytes(r) == L.mmk_icp_workspace_bytes(ctypes.byref(icp_params(loss=1, **kw)))     # Cauchy's sizes
        for bad_k in (0.0, -0.5, float("nan")):
            p = icp_params(loss=code, loss_k=bad_k)
            assert L.mmk_icp_workspace_bytes(ctypes.byref(p)) == 0 and b"metric" in L.mmk_last_error()
            assert forward(p) == -1 and b"metric" in L.mmk_last_error()                                     # MMK_ERR_ARG
    for code in (5, -1):
        p = icp_params(loss=code)
        assert L.mmk_icp_workspace_bytes(ctypes.byref(p)) == 0 and b"bad loss" in L.mmk_last_error()
        assert forward(p) == -1 and ("bad loss %d" % code).encode() in L.mmk_last_error()
    assert int(re.search(r"#define\s+MMK_ERR_ARG\s+\((-?\d+)\)", open(os.path.join(ROOT, "include", "mmk.h")).read()).group(1)) == -1


# ----------------------------------------------------------------------------- dICP.ICP and the policy
def test_icp_maps_the_names_and_refuses_the_others():
    icp = ICP("pt2pl", differentiable=True, max_iterations=3)
    for name, code in NEW.items():
        p = icp._params(1, 8, 8, 6, 2, {"name": name, "metric": 0.25}, 1.0, True)
        assert p.loss == code and p.loss_k == 0.25
        p = icp._params(1, 8, 8, 6, 2, {"name": name, "metric": torch.tensor(0.25)}, torch.tensor(1.0), True, on_device=True)
        assert p.loss == code                                      # the metric may be a tensor, as Cauchy's
    for name in ("tukey", "gm", "geman-mcclure", "Welsch", "leclerc"):
        with pytest.raises(ValueError, match="unknown loss_fn name"):
            icp._params(1, 8, 8, 6, 2, {"name": name, "metric": 0.25}, 1.0, True)


def test_policy_learns_the_metric_of_the_new_kernels():
    from mm_masking_amd.icp_weight_policy import LearnICPWeightPolicy
    for name in NEW:
        m = LearnICPWeightPolicy(policy_params(icp_loss_fn={"name": name, "metric": 0.5}, learn_icp=("metric",)))
        assert [n for n, _ in m.named_parameters() if n.startswith("icp_")] == ["icp_metric"]
        assert m.icp_metric.item() == 0.5 and m.icp_metric.requires_grad
    for loss_fn in (None, {"name": "l2"}, {"name": "tukey", "metric": 1.0}):
        with pytest.raises(ValueError, match="robust loss.*'cauchy', 'huber', 'geman_mcclure' or 'welsch'"):
            LearnICPWeightPolicy(policy_params(icp_loss_fn=loss_fn, learn_icp=("metric",)))


# ----------------------------------------------------------------------------- the restatement
def _inputs(dim, noise):
    S, Tg = [], []
    for b in range(B):
        s, t, _ = synthetic.simple_cloud_pair(77 + dim + b, N, M, dim=dim, noise=noise, yaw=0.02 + 0.01 * b, trans=(0.6, -0.4 + 0.1 * b, 0.1))
        S.append(s), Tg.append(t)
    w = np.random.default_rng(2).uniform(0.2, 1.0, (B, N)).astype(np.float32)
    T0 = torch.eye(4).repeat(B, 1, 1)
    T0[:, 0, 3] += 0.2
    G = torch.from_numpy(np.random.default_rng(3).normal(size=(B, 4, 4)).astype(np.float32))
    return torch.from_numpy(np.stack(S)), torch.from_numpy(np.stack(Tg)), torch.from_numpy(w), T0, G


@pytest.mark.parametrize("loss", [None, ("cauchy", 0.5), ("huber", 0.1)], ids=["none", "cauchy", "huber"])
@pytest.mark.parametrize("icp_type,dim", [("pt2pt", 2), ("pt2pl", 2), ("pt2pt", 3), ("pt2pl", 3)])
def test_hard_gate_is_the_oracle_bit_for_bit(icp_type, dim, loss):
    """On the clouds of tests/dicp_cases.py (B = 2, 320 x 730, K = 4) with trim distances 0.6 and 1.0, the restatement with the
    hard gate returns what oracle.dicp_ref.ICPRef returns: T, num_iter, the histories of idx, T and delta and the gradients of
    source, target, weight and T_init, in every bit."""
    inp = inputs((icp_type, loss, dim, 0.15 if icp_type == "pt2pl" else 0.01, 0.0))
    for trim in (0.6, 1.0):
        outs = []
        for oracle in (True, False):
            x = [v.clone().requires_grad_(True) for v in inp["x"]]
            kw = dict(T_init=x[3], weight=x[2], trim_dist=trim, dim=dim)
            if oracle:
                out = ICPRef(icp_type, differentiable=True, max_iterations=GPU_K, tolerance=TOL).icp(x[0], x[1], loss_fn=inp["loss_fn"],
                                                                                                     **kw)
            else:
                out = ICPRestatement(icp_type, differentiable=True, max_iterations=GPU_K, tolerance=TOL, soft=False).icp(
                    x[0], x[1], loss_name=loss and loss[0], k=loss[1] if loss else 1.0, **kw)
            (out["T"] * inp["G"]).sum().backward()
            outs.append((out, x))
        (a, xa), (b, xb) = outs
        assert a["num_iter"] == b["num_iter"] == GPU_K and torch.equal(a["T"], b["T"])
        for name in ("idx", "T", "delta"):
            assert len(a["hist"][name]) == len(b["hist"][name])
            for p, q in zip(a["hist"][name], b["hist"][name]):
                assert torch.equal(p, q), (name, trim)
        for name, p, q in zip(NAMES, xa, xb):
            assert p.grad is not None and p.grad.abs().max() > 0 and torch.equal(p.grad, q.grad), (name, trim)


@pytest.mark.parametrize("icp_type,dim", [("pt2pt", 2), ("pt2pl", 3)])
def test_geman_mcclure_is_the_bit_exact_square_of_cauchy(icp_type, dim):
    src, tgt, w, T0, _ = _inputs(dim, 0.15)
    idx = ICPRestatement(icp_type, differentiable=False, max_iterations=1).icp(src, tgt, T_init=T0, weight=w, k=0.3, trim_dist=TRIM,
                                                                            loss_name="cauchy", dim=dim)["hist"]["idx"][0]
    one = torch.ones(1, 1)
    terms = {name: per_point_terms(src, tgt, T0, idx, w, icp_type, name, one * 0.3, one * TRIM, one * STEEP, dim, True)
             for name in ("cauchy", "geman_mcclure", "welsch")}
    c, gm, we = (terms[n][4] for n in ("cauchy", "geman_mcclure", "welsch"))
    assert torch.equal(c["r2"], gm["r2"]) and torch.equal(c["keep"], gm["keep"])            # the same residuals
    assert torch.equal(gm["rho"], c["rho"] * c["rho"])
    assert torch.equal(terms["geman_mcclure"][2], (w * c["keep"]) * (c["rho"] * c["rho"]))   # and the weights
    assert torch.equal(we["rho"], torch.exp(-(c["r2"] / ((one * 0.3) * (one * 0.3)))))
    share = ((c["rho"] > 0.05) & (c["rho"] < 0.95)).double().mean().item()
    assert share > 0.3, share                                                                # not a saturated comparison
    assert (gm["rho"] <= c["rho"]).all() and (gm["rho"] < c["rho"]).any()


FD_CASES = [("pt2pt", "geman_mcclure", 0.5, 2, 0.01, False), ("pt2pl", "welsch", 0.2, 2, 0.15, True),
            ("pt2pt", "welsch", 0.5, 3, 0.01, True), ("pt2pl", "geman_mcclure", 0.5, 3, 0.15, False)]
FD_IDS = ["%s-%s-d%d-%s" % (c[0], c[1], c[3], "tanh" if c[5] else "hard") for c in FD_CASES]


def _fixed_run(case, k_shape, dtype=torch.float64):
    """The restatement with fixed correspondences (a free fp32 run's) and per-pair scales (pair 1: x 1.3).  The tanh gate at
    TRIM; the hard gate at 5 m, where it keeps every point: a hard gate that trims most of 70 points leaves the 6 x 6 system of
    the dim-3 cases close to singular, and a finite difference then measures the fall-back of the solve, not a derivative."""
    icp_type, loss, k, dim, noise, soft = case
    trim = TRIM if soft else 5.0
    src, tgt, w, T0, G = _inputs(dim, noise)
    ks = torch.tensor([k, k * 1.3])
    free = ICPRestatement(icp_type, differentiable=False, max_iterations=K, tolerance=1e-12, soft=soft).icp(
        src, tgt, T_init=T0, weight=w, k=ks, trim_dist=trim, trim_steep=STEEP, loss_name=loss, dim=dim)
    fixed = free["hist"]["idx"]
    assert len(fixed) == K
    ref = ICPRestatement(icp_type, differentiable=True, max_iterations=K, tolerance=1e-12, soft=soft)

    def run(s, t, ww, T, kk):
        return ref.icp(s, t, T_init=T, weight=ww, k=kk, trim_dist=trim, trim_steep=STEEP, loss_name=loss, dim=dim, dtype=dtype,
                       fixed_idx=fixed)

    if k_shape == "BN":
        ks = ks[:, None].expand(B, N).contiguous()
    leaves = [v.to(dtype).clone().requires_grad_(True) for v in (src, tgt, w, T0, ks)]
    return run, leaves, G.to(dtype), fixed


@pytest.mark.parametrize("case", FD_CASES, ids=FD_IDS)
def test_closed_forms_match_autograd(case):
    """I7's r2bar line and I7'''s k̄_i for the two kernels, written out in numpy fp64 from (wbar, omega, keep, rho, r2), against
    autograd through the restatement in fp64: both are exact derivatives of the same expressions, so they agree to rounding
    -- 1e-12 of the largest magnitude (tests/test_softmin_temp_cpu.py's bound)."""
    icp_type, loss, _, _, _, soft = case
    run, leaves, G, _ = _fixed_run(case, "BN")
    out = run(*leaves)
    (out["T"] * G).sum().backward()
    kv = leaves[4].detach().numpy()
    got, ref = closed_form_sums(out["hist"], kv, TRIM if soft else 5.0, STEEP, loss, soft)[0], leaves[4].grad.numpy()
    scale = np.abs(ref).max()
    assert scale > 0 and np.abs(got - ref).max() <= 1e-12 * scale, (np.abs(got - ref).max(), scale)
    assert (np.abs(ref) > 1e-3 * scale).sum() >= 20             # and not a handful of points only (the hard gate trims many)
    if icp_type == "pt2pl" or not soft:                         # (pt2pt under the tanh gate: the gate reads the same d2)
        for t, act in zip(out["hist"]["terms"], out["hist"]["active"]):
            got, ref = closed_form_r2bar(t, act, kv, loss), t["r2_graph"].grad.numpy()
            scale = np.abs(ref).max()
            assert scale > 0 and np.abs(got - ref).max() <= 1e-12 * scale, (np.abs(got - ref).max(), scale)


@pytest.mark.parametrize("case", FD_CASES, ids=FD_IDS)
def test_finite_differences(case):
    """fp64 central differences of the restatement (fixed correspondences) in source, target xyz (and normals), weight, T_init
    and each pair's k against its autograd: step and bound of tests/test_icp_hyper_cpu.py's finite-difference test."""
    icp_type, loss, _, dim, _, soft = case
    run, leaves, G, fixed = _fixed_run(case, "B")

    def f(*a):
        with torch.no_grad():
            return (run(*a)["T"] * G).sum()

    out = run(*leaves)
    rho = torch.stack(out["hist"]["rho"])
    share = float(((rho > 0.05) & (rho < 0.95)).double().mean())
    assert share >= 0.3, share                                  # the kernel is neither off nor saturated
    (out["T"] * G).sum().backward()
    grads = [v.grad for v in leaves]
    assert all(torch.isfinite(g).all() for g in grads)
    used = torch.unique(torch.cat([ix[0].long() for ix in fixed]))
    checks = [(0, (b, i, c)) for b, i, c in ((0, 0, 0), (1, 17, 1), (0, 63, dim - 1))]
    for j in used[[0, len(used) // 2, -1]].tolist():
        checks += [(1, (0, j, c)) for c in range(dim)]
        if icp_type == "pt2pl":
            checks += [(1, (0, j, 3 + c)) for c in range(dim)]
    checks += [(2, (b, i)) for b, i in ((0, 0), (1, 17), (0, 63))]
    checks += [(3, (b, r, c)) for b, r, c in ((0, 0, 3), (1, 1, 3), (0, 0, 0), (1, 0, 1), (0, 1, 0), (1, 1, 1))]
    if dim == 3:
        checks += [(3, (0, r, c)) for r, c in ((2, 3), (2, 1), (0, 2))]
    checks += [(4, (b,)) for b in range(B)]
    eps, worst = 1e-6, 0.0
    for which, at in checks:
        ap = [v.detach().clone() for v in leaves]
        am = [v.detach().clone() for v in leaves]
        ap[which][at] += eps
        am[which][at] -= eps
        fd = (f(*ap) - f(*am)).item() / (2 * eps)
        g = grads[which][at].item()
        bound = 1e-5 * max(1e-3, abs(fd)) + 1e-8
        worst = max(worst, abs(fd - g) / bound)
        assert abs(fd - g) <= bound, (which, at, fd, g)
        if which == 4:
            assert g != 0.0, at
    print("FD %s: worst deviation %.2f of the bound, band share %.2f" % (FD_IDS[FD_CASES.index(case)], worst, share))


# ----------------------------------------------------------------------------- the GPU cases stay awake
@pytest.mark.parametrize("ci", range(len(GPU_CASES)), ids=GPU_IDS)
def test_gpu_cases_are_awake_on_the_free_run(ci):
    """tests/test_gpu_robust_kernels.py's cases on the restatement's free run (its own correspondences): every configuration
    that file replays keeps its conditions -- no pair froze, the band share, the scale's awake ratio."""
    case = GPU_CASES[ci]
    for mult in (1.0, K_MULT):
        assert_awake(reference(case, ROBUST_TRIM, mult=(mult, 1.0, 1.0)), "%s nearest k x %s" % (GPU_IDS[ci], (1.0, mult)))
    for soft_k in (4, 8):
        for taus in ((TAU, TAU), PER_PAIR_TAU):
            assert_awake(reference(case, ROBUST_TRIM, soft_k=soft_k, taus=taus),
                         "%s softmin %d tau %s" % (GPU_IDS[ci], soft_k, taus))
