"""GPU: the soft (tanh) trim gate of the HIP dICP (mmk_icp_params.trim_steep; DESIGN.md §3 I3', I7') against the restatement
tests/dicp_soft_trim_ref.py: forward, the gradients of source, target, weight and T_init from both backward entries,
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

from mm_masking_amd import _lib, synthetic
from mm_masking_amd.dICP.ICP import ICP

from dicp_soft_trim_ref import ICPSoftRef, band_share, per_point_terms

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

B, N_REAL, N_ZERO, M_REAL, M_PAD, K, TOL, TRIM = 2, 300, 20, 700, 30, 4, 1e-9, 0.6
N, M = N_REAL + N_ZERO, M_REAL + M_PAD

#        type     loss (k)          dim noise steepness
CASES = [("pt2pt", ("cauchy", 0.5), 2, 0.01, 4.0),
         ("pt2pl", ("huber", 0.1), 2, 0.15, 4.0),
         ("pt2pt", ("huber", 0.5), 3, 0.01, 4.0),
         ("pt2pl", ("cauchy", 0.5), 3, 0.15, 4.0),
         ("pt2pl", None, 2, 0.15, 4.0),
         ("pt2pt", None, 2, 0.01, 10.0)]
IDS = ["%s-%s-d%d-s%g" % (c[0], c[1][0] if c[1] else "none", c[2], c[4]) for c in CASES]
NAMES = ("source", "target", "weight", "T_init")


@pytest.fixture(params=["brute", "grid"])
def nn_engine(request):
    ICP.NN_SEARCH_OVERRIDE = request.param
    yield request.param
    ICP.NN_SEARCH_OVERRIDE = None


def _inputs(case, coincident=False):
    icp_type, loss, dim, noise, steep = case
    S, Tg = [], []
    for b in range(B):
        s, t, _ = synthetic.simple_cloud_pair(77 + dim + b, N_REAL, M_REAL, dim=dim, noise=noise, pad_n=N_ZERO, pad_m=M_PAD,
                                              yaw=0.02 + 0.01 * b, trans=(0.6, -0.4 + 0.1 * b, 0.1))
        S.append(s), Tg.append(t)
    src, tgt = np.stack(S), np.stack(Tg)
    w = np.random.default_rng(2).uniform(0.2, 1.0, (B, N)).astype(np.float32)
    w[:, N_REAL:] = 0.0
    T0 = torch.eye(4).repeat(B, 1, 1)
    if coincident:
        src[:, 5] = tgt[:, 11, :3]          # d == 0 under T_init = I
    else:
        T0[:, 0, 3] += 0.2
    G = torch.from_numpy(np.random.default_rng(3).normal(size=(B, 4, 4)).astype(np.float32))
    loss_fn = None if loss is None else {"name": loss[0], "metric": loss[1]}
    return {"x": [torch.from_numpy(src), torch.from_numpy(tgt), torch.from_numpy(w), T0], "G": G, "loss_fn": loss_fn}


def _gpu(case, inp, need=NAMES, configure=None):
    """One forward + backward of the HIP dICP: T, idx_hist (K,B,N), active_hist (K+1,B), gradients by name."""
    icp_type, _, dim, _, steep = case
    icp = ICP(icp_type=icp_type, differentiable=True, max_iterations=K, tolerance=TOL)
    if configure is None:
        icp.trim, icp.tanh_steepness = "tanh", steep
    else:
        icp = configure(icp) or icp
    x = [v.clone().to(DEV).requires_grad_(name in need) for name, v in zip(NAMES, inp["x"])]
    T = icp.icp(x[0], x[1], T_init=x[3], weight=x[2], trim_dist=TRIM, loss_fn=inp["loss_fn"], dim=dim)["T"]
    saved = T.grad_fn.saved_tensors                 # weight, src, tgt, idx, T_hist, delta, A, active
    (T * inp["G"].to(DEV)).sum().backward()
    torch.cuda.synchronize()
    grads = {name: (v.grad.cpu() if v.grad is not None else None) for name, v in zip(NAMES, x)}
    return {"T": T.detach().cpu(), "idx": saved[3].cpu(), "active": saved[7].cpu(), "grads": grads}


_ref_cache = {}


def _reference(ci, inp, idx_hist):
    """Autograd through the fp32 restatement replaying ``idx_hist``; computed once per (case, correspondences)."""
    key = (ci, idx_hist.numpy().tobytes())
    if key not in _ref_cache:
        icp_type, _, dim, _, steep = CASES[ci]
        leaves = [v.clone().requires_grad_(True) for v in inp["x"]]
        ref = ICPSoftRef(icp_type, differentiable=True, max_iterations=K, tolerance=TOL, trim_steep=steep)
        out = ref.icp(leaves[0], leaves[1], T_init=leaves[3], weight=leaves[2], trim_dist=TRIM, loss_fn=inp["loss_fn"], dim=dim,
                      fixed_idx=[idx_hist[k].long() for k in range(K)])
        (out["T"] * inp["G"]).sum().backward()
        _ref_cache[key] = {"T": out["T"].detach(), "hist": out["hist"], "num_iter": out["num_iter"],
                           "grads": {name: v.grad for name, v in zip(NAMES, leaves)}}
    return _ref_cache[key]


_free_cache = {}


def _free_idx0(ci, inp):
    """Correspondences of the first iteration of the free-running reference."""
    if ci not in _free_cache:
        icp_type, _, dim, _, steep = CASES[ci]
        ref = ICPSoftRef(icp_type, differentiable=False, max_iterations=1, tolerance=TOL, trim_steep=steep)
        out = ref.icp(inp["x"][0], inp["x"][1], T_init=inp["x"][3], weight=inp["x"][2], trim_dist=TRIM, loss_fn=inp["loss_fn"], dim=dim)
        _free_cache[ci] = out["hist"]["idx"][0]
    return _free_cache[ci]


def _close(g, ref, name, rel=2e-3):
    g, ref = g.detach().cpu().double().numpy(), ref.detach().double().numpy()
    scale = np.abs(ref).max()
    assert scale > 0, name
    err = np.abs(g - ref).max()
    print("GRAD %-7s err/scale = %.3e (scale %.3e)" % (name, err / scale, scale))
    assert err <= rel * scale, (name, err, scale)


def _assert_gate_is_awake(ci, ref):
    """Conditions on the reference's own values: no case passes with the gate or the Huber branch asleep."""
    loss = CASES[ci][1]
    real = torch.zeros(B, N, dtype=torch.bool)
    real[:, :N_REAL] = True
    assert ref["num_iter"] == K and all(bool(a.all()) for a in ref["hist"]["active"])          # all pairs active
    shares = [band_share(k, real) for k in ref["hist"]["keep"]]
    print("BAND SHARE per iteration: %s" % ["%.2f" % s for s in shares])
    assert min(shares) >= 0.10, shares
    if loss is not None and loss[0] == "huber":
        hub = [float(h[real].double().mean()) for h in ref["hist"]["huber_out"]]
        print("HUBER r > k share per iteration: %s" % ["%.2f" % s for s in hub])
        assert float(torch.stack(ref["hist"]["huber_out"])[:, real].double().mean()) >= 0.3, hub


# ----------------------------------------------------------------------------- 1. - 4. forward, gradients, zeros, run-to-run
@pytest.mark.parametrize("ci", range(len(CASES)), ids=IDS)
def test_soft_gate_matches_the_restatement(nn_engine, ci):
    case = CASES[ci]
    icp_type, _, dim, _, _ = case
    inp = _inputs(case)
    run = _gpu(case, inp)
    assert run["active"][:K].all()
    # 1. forward: the first search is the free-running reference's; the pose is the replay's
    assert torch.equal(run["idx"][0].long(), _free_idx0(ci, inp).long())
    ref = _reference(ci, inp, run["idx"])
    _assert_gate_is_awake(ci, ref)
    err = (run["T"].double() - ref["T"].double()).abs().max().item()
    print("POSE max abs diff = %.3e" % err)
    np.testing.assert_allclose(run["T"].numpy(), ref["T"].numpy(), atol=2e-6, rtol=0)
    # 2. gradients: mmk_icp_backward_points (all four), mmk_icp_backward (weight and T_init only)
    for name in NAMES:
        _close(run["grads"][name], ref["grads"][name], name)
    two = _gpu(case, inp, need=("weight", "T_init"))
    assert torch.equal(two["T"], run["T"]) and torch.equal(two["idx"], run["idx"])
    assert two["grads"]["source"] is None and two["grads"]["target"] is None
    for name in ("weight", "T_init"):
        _close(two["grads"][name], ref["grads"][name], name + " (mmk_icp_backward)")
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
    again = _gpu(case, inp)
    assert torch.equal(again["T"], run["T"]) and torch.equal(again["idx"], run["idx"])
    for name in NAMES:
        assert torch.equal(again["grads"][name], run["grads"][name]), name


# ----------------------------------------------------------------------------- 5. gate off
@pytest.mark.parametrize("ci", [1, 2], ids=[IDS[1], IDS[2]])
def test_gate_off_is_bit_identical_to_a_call_that_never_mentions_it(nn_engine, ci, tmp_path):
    case = CASES[ci]
    inp = _inputs(case)
    plain = _gpu(case, inp, configure=lambda icp: None)                 # never mentions the option

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
        got = _gpu(case, inp, configure=configure)
        assert torch.equal(got["T"], plain["T"]) and torch.equal(got["idx"], plain["idx"]), configure.__name__
        assert torch.equal(got["active"], plain["active"])
        for name in NAMES:
            assert torch.equal(got["grads"][name], plain["grads"][name]), (configure.__name__, name)
    soft = _gpu(case, inp)
    assert not torch.equal(soft["T"], plain["T"])                       # and the option is not a no-op


# ----------------------------------------------------------------------------- 6. the stand-alone stage
@pytest.mark.parametrize("ci", [1, 2], ids=[IDS[1], IDS[2]])
def test_accumulate_stage_with_the_soft_gate(ci):
    case = CASES[ci]
    icp_type, _, dim, _, steep = case
    inp = _inputs(case)
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
    loss_name = None if inp["loss_fn"] is None else inp["loss_fn"]["name"]
    loss_k = 1.0 if inp["loss_fn"] is None else inp["loss_fn"]["metric"]
    J, e, wref, _, aux = per_point_terms(src, tgt, T0c, ic, w, icp_type, loss_name, loss_k, TRIM, dim, steep)
    real = torch.zeros(B, N, dtype=torch.bool)
    real[:, :N_REAL] = True
    assert band_share(aux["keep"], real) >= 0.10
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
    inp = _inputs(case, coincident=True)
    run = _gpu(case, inp)
    assert (run["idx"][0][:, 5] == 11).all()                    # d == 0 in the first iteration
    for name in NAMES:
        g = run["grads"][name]
        assert torch.isfinite(g).all() and g.abs().max() > 0, name


# ----------------------------------------------------------------------------- 8. the policy
from test_gpu_mask_scan import scene64, _policy  # noqa: E402,F401  (the smallest scan-mode batch of the suite, as a fixture)


def test_policy_soft_gate_trains_and_inference_stays_hard(scene64):
    """mask_target="scan": one training step with params["icp_trim"] = "tanh".  The points of this scene lie 0.09 .. 0.15 m
    from their correspondents, so a trim distance of 0.12 m puts them inside the gate's band (steepness 10: |argument| < 0.4)."""
    scan, mp, T0, G = scene64
    kw = dict(mask_target="scan", icp_trim_dist=0.12)

    def step(model):
        model.train()
        T, _, _ = model(scan, mp, T0)
        (T * G).sum().backward()
        return T.detach(), [q.grad.detach().clone() for q in model.parameters()]

    soft_model, hard_model = _policy(icp_trim="tanh", **kw), _policy(**kw)
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
