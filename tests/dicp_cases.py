"""What the dICP tests share (soft gate, device hyper-parameters, soft-min, device temperature, robust kernels): shapes, the case
tables, the inputs, one launch of the HIP dICP, one run of the CPU restatement and the "is it awake" conditions -- a module of
the tests, not a test.  Nothing here touches a device at import; ``gpu`` names it when called.

Shapes: B = 2, 300 + 20 zero source rows (one full and one partial 256-thread block), 700 + 30 target_pad_val rows, K = 4,
T_init shifted by 0.2 m.  A case is (icp type, (loss, k) or None, dim, noise, tanh steepness -- 0: the hard gate); each table
has its trim distance.  In the per-pair runs pair 1 uses k x 1.3, trim_dist x 1.15, steepness x 0.8 (``MULT``; ``K_MULT`` where
only k differs) and the temperatures ``PER_PAIR_TAU``.

``reference`` runs the restatement ONCE per key with (B,N)-shaped leaves for k, trim_dist, the steepness and (soft
correspondences) tau: the gradient of such a leaf is every point's contribution summed over the iterations, its fp64 row sums
are the per-pair reference gradients g_b, and the awake condition of each parameter is made of it: max_b |g_b| / S_b >= 0.03
with S_b the sum of the magnitudes of pair b's contributions.  Leaves of equal values give the bits of a call with numbers
(tests/test_icp_hyper_cpu.py, tests/test_softmin_temp_cpu.py).
"""
import numpy as np
import torch

from mm_masking_amd import synthetic
from mm_masking_amd.dICP.ICP import ICP
from oracle.dicp_ref import transform_points

from dicp_restatement import ICPRestatement, band_share, knn_ref_batch, pair_sums, tau_leaf
from support import nn_engine  # noqa: F401  (a fixture, re-exported to the dICP test files)

B, N_REAL, N_ZERO, M_REAL, M_PAD, K, TOL = 2, 300, 20, 700, 30, 4, 1e-9
N, M = N_REAL + N_ZERO, M_REAL + M_PAD

NAMES = ("source", "target", "weight", "T_init")
HNAMES = ("k", "trim_dist", "trim_steep")
MULT = (1.3, 1.15, 0.8)             # pair 1's values over pair 0's
K_MULT = 1.3                        # pair 1's scale over pair 0's where only the scale differs
TAU = 0.25
PER_PAIR_TAU = (0.25, 0.4)
HARD_STEEP = 10.0                   # the instance's default steepness: not read under the hard gate

#             type     loss (k)          dim noise steepness
GATE_CASES = [("pt2pt", ("cauchy", 0.5), 2, 0.01, 4.0),
              ("pt2pl", ("huber", 0.1), 2, 0.15, 4.0),
              ("pt2pt", ("huber", 0.5), 3, 0.01, 4.0),
              ("pt2pl", ("cauchy", 0.5), 3, 0.15, 4.0),
              ("pt2pl", None, 2, 0.15, 4.0),
              ("pt2pt", None, 2, 0.01, 10.0)]
GATE_IDS = ["%s-%s-d%d-s%g" % (c[0], c[1][0] if c[1] else "none", c[2], c[4]) for c in GATE_CASES]
GATE_TRIM = 0.6

SOFTMIN_CASES = [("pt2pt", ("cauchy", 0.5), 2, 0.01, 0.0),
                 ("pt2pl", ("huber", 0.1), 2, 0.15, 0.0),
                 ("pt2pt", ("huber", 0.5), 3, 0.01, 0.0),
                 ("pt2pl", ("cauchy", 0.5), 3, 0.15, 0.0),
                 ("pt2pl", None, 2, 0.15, 4.0)]
SOFTMIN_IDS = ["%s-%s-d%d%s" % (c[0], c[1][0] if c[1] else "none", c[2], "-tanh" if c[4] else "") for c in SOFTMIN_CASES]
SOFTMIN_TRIM = 1.0

ROBUST_CASES = [("pt2pt", ("geman_mcclure", 0.5), 2, 0.01, 0.0),
                ("pt2pl", ("welsch", 0.2), 2, 0.15, 0.0),
                ("pt2pt", ("welsch", 0.5), 3, 0.01, 0.0),
                ("pt2pl", ("geman_mcclure", 0.5), 3, 0.15, 0.0),
                ("pt2pl", ("geman_mcclure", 0.2), 2, 0.15, 4.0),
                ("pt2pt", ("welsch", 0.5), 2, 0.01, 4.0)]
ROBUST_IDS = ["%s-%s-d%d%s" % (c[0], c[1][0], c[2], "-tanh" if c[4] else "") for c in ROBUST_CASES]
ROBUST_TRIM = 1.0

REAL = torch.zeros(B, N, dtype=torch.bool)
REAL[:, :N_REAL] = True


def inputs(case, coincident=False):
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


def policy_params(**kw):
    p = dict(icp_type="pt2pl", fft_input=True, cfar_input=False, range_input=False, network_input_type="cartesian",
             network_output_type="cartesian", device="cpu", max_iter=4, loss_icp_rot_weight=1.0, loss_icp_trans_weight=1.0,
             float_type=torch.float32, leaky=False, dropout=0.0, batch_norm=False, normalize="minmax", log_transform=False,
             a_thresh=1.0, b_thresh=0.09, gt_eye=True, norm_weights=True, init_weights=True, unet_backend="torch")
    p.update(kw)
    return p


def close(g, ref, name, rel=2e-3):
    g, ref = g.detach().cpu().double().numpy(), ref.detach().double().numpy()
    scale = np.abs(ref).max()
    assert scale > 0, name
    err = np.abs(g - ref).max()
    print("GRAD %-7s err/scale = %.3e (scale %.3e)" % (name, err / scale, scale))
    assert err <= rel * scale, (name, err, scale)


def same(a, b, names):
    assert torch.equal(a["T"], b["T"]) and torch.equal(a["idx"], b["idx"]) and torch.equal(a["active"], b["active"])
    for name in names:
        assert torch.equal(a["grads"][name], b["grads"][name]), name


# ----------------------------------------------------------------------------- the device
def gpu(case, inp, trim_dist, need=NAMES, gate=None, k=None, steep=None, softmin_k=None, tau=TAU, configure=None, K_=K, tol=TOL):
    """One forward + backward of the HIP dICP -> T, idx_hist, T_hist (K+1,B,16), active_hist (K+1,B), the gradients by name and
    the grad function's class name.

    ``gate``: "tanh" / "hard" with the steepness ``steep`` (the case's by default); None: "tanh" if the case has a steepness,
    else the instance as it is built; False: as it is built.  ``k``: the metric of the case's loss (a case without one hands it
    over under the name "l2": rho = 1); None: the case's own loss_fn.  ``softmin_k``: soft correspondences with the temperature
    ``tau``.  k, trim_dist, steep and tau are numbers or CPU tensors, which go to the device and require grad if named in
    ``need``.  ``configure(icp)`` has the last word on the instance and may return another one."""
    dev = torch.device("cuda:0")

    def on_device(name, v):
        return v.clone().to(dev).requires_grad_(name in need) if isinstance(v, torch.Tensor) else v

    icp = ICP(icp_type=case[0], differentiable=True, max_iterations=K_, tolerance=tol)
    if gate is None and case[4] > 0:
        gate = "tanh"
    h = {"k": on_device("k", k), "trim_dist": on_device("trim_dist", trim_dist),
         "trim_steep": on_device("trim_steep", case[4] if steep is None else steep), "tau": on_device("tau", tau)}
    if gate:
        icp.trim, icp.tanh_steepness = gate, h["trim_steep"]
    if softmin_k is not None:
        icp.correspondence, icp.softmin_k, icp.softmin_temp = "softmin", softmin_k, h["tau"]
    if configure is not None:
        icp = configure(icp) or icp
    loss_fn = inp["loss_fn"] if k is None else {"name": "l2" if case[1] is None else case[1][0], "metric": h["k"]}
    x = [v.clone().to(dev).requires_grad_(name in need) for name, v in zip(NAMES, inp["x"])]
    T = icp.icp(x[0], x[1], T_init=x[3], weight=x[2], trim_dist=h["trim_dist"], loss_fn=loss_fn, dim=case[2])["T"]
    assert T.requires_grad
    saved = T.grad_fn.saved_tensors                 # weight, src, tgt, idx, T_hist, delta, A, active(, hyper | temp)
    (T * inp["G"].to(dev)).sum().backward()
    torch.cuda.synchronize()
    grads = {name: (v.grad.cpu() if v.grad is not None else None) for name, v in zip(NAMES, x)}
    for n, v in h.items():
        grads[n] = None
        if isinstance(v, torch.Tensor) and v.grad is not None:
            assert v.grad.shape == v.shape and v.grad.dtype == v.dtype and v.grad.device == v.device
            grads[n] = v.grad.cpu()
    return {"T": T.detach().cpu(), "idx": saved[3].cpu(), "T_hist": saved[4].cpu(), "active": saved[7].cpu(), "grads": grads,
            "fn": type(T.grad_fn).__name__}


# ----------------------------------------------------------------------------- the restatement
_ref_cache = {}


def reference(case, trim, fixed_idx=None, mult=(1.0, 1.0, 1.0), soft_k=None, taus=(TAU, TAU), differentiable=True, K_=K):
    """Autograd through the fp32 restatement on ``inputs(case)``: nearest correspondences, or soft ones over ``soft_k`` rows
    with the per-pair temperatures ``taus``; ``fixed_idx`` (K, ...) is replayed, None runs free.  Pair 1's (k, trim_dist,
    steepness) are pair 0's times ``mult``.  Every hyper-parameter is a (B,N) leaf: ``points`` holds their gradients (None where
    the pose does not read the value), ``grads`` the fp64 row sums next to the four inputs' gradients, ``S`` tau's sum of
    magnitudes.  Computed once per key and left unchanged."""
    replay = None if fixed_idx is None else fixed_idx.numpy().tobytes()
    key = (case, trim, replay, tuple(mult), soft_k, tuple(taus), differentiable, K_)
    if key in _ref_cache:
        return _ref_cache[key]
    icp_type, loss, dim, _, steep = case
    inp = inputs(case)
    leaves = [v.clone().requires_grad_(differentiable) for v in inp["x"]]
    base = (1.0 if loss is None else loss[1], trim, steep if steep > 0 else HARD_STEEP)
    hl = {n: tau_leaf((v, v * m), N) for n, v, m in zip(HNAMES, base, mult)}
    ref = ICPRestatement(icp_type, differentiable=differentiable, max_iterations=K_, tolerance=TOL, soft=steep > 0)
    kw = dict(T_init=leaves[3], weight=leaves[2], k=hl["k"], trim_dist=hl["trim_dist"], trim_steep=hl["trim_steep"],
              loss_name=None if loss is None else loss[0], dim=dim,
              fixed_idx=None if fixed_idx is None else [fixed_idx[it].long() for it in range(K_)])
    if soft_k is None:
        out = ref.icp(leaves[0], leaves[1], **kw)
    else:
        hl["tau"] = tau_leaf(taus, N)
        out = ref.icp_soft(leaves[0], leaves[1], hl["tau"], softmin_k=soft_k, **kw)
    res = {"T": out["T"].detach(), "hist": out["hist"], "num_iter": out["num_iter"]}
    if differentiable:
        (out["T"] * inp["G"]).sum().backward()
        res["grads"] = {n: v.grad for n, v in zip(NAMES, leaves)}
        res["points"] = {n: (None if v.grad is None else v.grad.double()) for n, v in hl.items()}
        for n, p in res["points"].items():
            res["grads"][n] = None if p is None else p.sum(1)
        if soft_k is not None:
            res["S"] = pair_sums(hl["tau"].grad)[1]
    _ref_cache[key] = res
    return res


def first_neighbours(case, k):
    """Neighbours of the first iteration of a free run with soft correspondences."""
    x, dim = inputs(case)["x"], case[2]
    p = torch.stack(transform_points(x[0], x[3], dim), dim=-1)
    return torch.from_numpy(knn_ref_batch(p.numpy(), x[1][..., :dim].numpy(), k, dim)[0])


# ----------------------------------------------------------------------------- the awake conditions, on the reference's own values
def _assert_none_froze(ref):
    assert ref["num_iter"] == K and all(bool(a.all()) for a in ref["hist"]["active"])


def _assert_huber_past_its_knee(case, ref):
    if case[1] is not None and case[1][0] == "huber":
        hub = [float(h[REAL].double().mean()) for h in ref["hist"]["huber_out"]]
        print("HUBER r > k share per iteration: %s" % ["%.2f" % s for s in hub])
        assert float(torch.stack(ref["hist"]["huber_out"])[:, REAL].double().mean()) >= 0.3, hub


def assert_gate_awake(case, ref):
    """No case passes with a pair frozen or the gate or the Huber branch asleep."""
    _assert_none_froze(ref)
    shares = [band_share(k, REAL) for k in ref["hist"]["keep"]]
    print("BAND SHARE per iteration: %s" % ["%.2f" % s for s in shares])
    assert min(shares) >= 0.10, shares
    _assert_huber_past_its_knee(case, ref)


def assert_softmin_awake(case, ref):
    """No case passes with a pair frozen or the soft-min, the gate or the Huber branch asleep."""
    _assert_none_froze(ref)
    shared = [float((a[..., 0][REAL] < 0.9).double().mean()) for a in ref["hist"]["a"]]
    print("a_0 < 0.9 share per iteration: %s" % ["%.2f" % s for s in shared])
    assert min(shared) >= 0.30, shared
    passed = [float((kp[REAL] > 0.5).double().mean()) for kp in ref["hist"]["keep"]]
    print("GATE PASSED share per iteration: %s" % ["%.2f" % s for s in passed])
    assert min(passed) >= 0.30, passed
    _assert_huber_past_its_knee(case, ref)


def assert_hyper_awake(case, ref):
    """No parameter's gradient is the rounding noise of a cancellation: for each, some pair's |g_b| is at least 0.03 of the
    sum of the magnitudes of its per-point contributions."""
    for n in HNAMES:
        p = ref["points"][n]
        if p is None:
            assert n == "k" and case[1] is None
            continue
        ratios = (p.sum(1).abs() / p.abs().sum(1)).tolist()
        print("AWAKE %-10s |g_b| / S_b per pair: %s" % (n, ["%.3f" % r for r in ratios]))
        assert max(ratios) >= 0.03, (n, ratios)


def assert_tau_awake(ref, what):
    """The tau gradient is not the rounding noise of a cancellation: some pair's |g_b| is at least 0.03 of the sum of the
    magnitudes of its per-point contributions."""
    ratios = (ref["grads"]["tau"].abs() / ref["S"]).tolist()
    print("AWAKE tau %s: |g_b| / S_b per pair %s" % (what, ["%.3f" % r for r in ratios]))
    assert max(ratios) >= 0.03, ratios


def awake_figures(ref):
    """(smallest band share over the iterations, the scale's awake ratio per pair, smallest step norm) of a reference run."""
    h = ref["hist"]
    shares = [float(((kp > 0.5) & (rho > 0.05) & (rho < 0.95))[REAL].double().mean()) for kp, rho in zip(h["keep"], h["rho"])]
    p = ref["points"]["k"]
    ratios = (p.sum(1).abs() / p.abs().sum(1)).tolist()
    step = min(float(d.norm(dim=1).min()) for d in h["delta"])
    return shares, ratios, step


def assert_awake(ref, what):
    """No case passes with a pair frozen, the kernel off or saturated, or the scale's gradient asleep."""
    assert ref["num_iter"] == K and all(bool(a.all()) for a in ref["hist"]["active"]), what      # no pair froze
    shares, ratios, step = awake_figures(ref)
    print("AWAKE %s: band share per iteration %s, |g_b| / S_b per pair %s, smallest step %.4f"
          % (what, ["%.2f" % s for s in shares], ["%.3f" % r for r in ratios], step))
    assert min(shares) >= 0.30, (what, shares)
    assert max(ratios) >= 0.03, (what, ratios)
    return shares, ratios, step
