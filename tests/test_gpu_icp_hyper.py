"""GPU: the HIP dICP with its robust scale k, trim distance and steepness on the device, one value for the batch or one per
pair, and their gradients (mmk_icp_forward_hp / mmk_icp_backward_hp; DESIGN.md §3 I3'', I7'') against the restatement
tests/dicp_restatement.py.

Shapes, cases and replay discipline are those of tests/dicp_cases.py (imported from it): B = 2, 300 + 20 source rows,
700 + 30 target rows, K = 4, trim_dist 0.6, both NN engines; the reference replays the device's idx_hist.  In the per-pair
runs pair 1 uses k x 1.3, trim_dist x 1.15, steepness x 0.8.

The reference runs ONCE per (case, correspondences) with (B,N)-shaped leaves for the three parameters: the gradient of such a
leaf is every point's contribution (summed over the iterations), its fp64 row sums are the per-pair reference gradients, and
the "is this gradient awake" condition of each parameter is made of it -- max_b |g_b| / S_b >= 0.03 with S_b the sum of the
magnitudes of pair b's contributions -- next to the soft-trim test's own conditions (band share, Huber past its knee, no pair
frozen).  All are asserted on the reference's values and printed.

Tolerances: pose 2e-6 absolute, gradients 2e-3 of the reference's largest magnitude per parameter (``close`` of
tests/dicp_cases.py).  Equalities are exact: tensors holding the values of a float call give that call's bits; a shared value's
gradient is the fp32 rounding of the fp64 sum of the pairs' gradients; the hard gate gives trim_dist and the steepness 0, no robust loss
gives k 0, a pair's frozen iterations add 0; two runs agree in every bit.

Measured on an MI355X (both engines, all cases): pose within 2.4e-7 of the replay; gradients within 9.5e-6 of the reference's
largest magnitude (pt2pl Huber, weight); of the new ones k within 7.8e-6, trim_dist 2.0e-6, trim_steep 4.3e-6.  The awake ratio
max_b |g_b| / S_b: smallest 0.051 (pt2pl, no loss, dim 2, steepness); the smallest single entry 0.008 of its S.
"""
import numpy as np
import pytest
import torch

from mm_masking_amd import _lib
from mm_masking_amd.dICP.ICP import ICP, check_errors

import icp_freeze_cases as fz
from dicp_cases import (B, GATE_CASES as CASES, GATE_IDS as IDS, GATE_TRIM as TRIM, HNAMES, K, MULT, NAMES, TOL, assert_gate_awake,
                        assert_hyper_awake, close, gpu, inputs, nn_engine, reference, same)  # noqa: F401
from radar_cases import scene64  # noqa: F401  (the smallest scan-mode batch of the suite, a module fixture)
from support import DEV, policy

pytestmark = pytest.mark.gpu

ALL7 = NAMES + HNAMES


def _values(case, per_pair):
    """(k, trim_dist, steepness) of a case as floats (pair 0's) and as fp32 tensors: (B,) with pair 1 scaled, or equal."""
    base = (1.0 if case[1] is None else case[1][1], TRIM, case[4])
    m = MULT if per_pair else (1.0, 1.0, 1.0)
    return base, [torch.tensor([v, v * mm], dtype=torch.float32) for v, mm in zip(base, m)]


def _gpu(case, inp, hyper, need=ALL7, gate="tanh", **kw):
    """One forward + backward.  ``hyper``: (k, trim_dist, steepness), each a float or a CPU tensor."""
    return gpu(case, inp, hyper[1], need=need, gate=gate, k=hyper[0], steep=hyper[2], **kw)


# ----------------------------------------------------------------------------- 1. same values, same bits
@pytest.mark.parametrize("gate", ["tanh", "hard"])
@pytest.mark.parametrize("ci", range(len(CASES)), ids=IDS)
def test_tensors_with_a_float_calls_values_give_its_bits(nn_engine, ci, gate):
    case = CASES[ci]
    inp = inputs(case)
    base, vals = _values(case, False)
    for need in (NAMES, ("weight", "T_init")):                  # both backward shapes
        plain = _gpu(case, inp, base, need=need, gate=gate)
        assert plain["fn"] == "_IcpFunctionBackward"
        scalars = [torch.tensor(v, dtype=torch.float32) for v in base]
        for hyper in (scalars, vals, [scalars[0], base[1], vals[2]], [base[0], vals[1], base[2]]):
            for with_grad in (need, need + HNAMES):
                got = _gpu(case, inp, hyper, need=with_grad, gate=gate)
                assert got["fn"] == "_IcpHpFunctionBackward"
                same(got, plain, need)
                assert all(got["grads"][n] is None for n in NAMES if n not in need)


# ----------------------------------------------------------------------------- 2. - 5. per-pair values
@pytest.mark.parametrize("ci", range(len(CASES)), ids=IDS)
def test_per_pair_values_match_the_restatement(nn_engine, ci):
    case = CASES[ci]
    inp = inputs(case)
    _, vals = _values(case, True)
    run = _gpu(case, inp, vals)
    assert run["active"][:K].all()
    ref = reference(case, TRIM, fixed_idx=run["idx"], mult=MULT)
    assert_gate_awake(case, ref)
    assert_hyper_awake(case, ref)
    err = (run["T"].double() - ref["T"].double()).abs().max().item()
    print("POSE max abs diff = %.3e" % err)
    np.testing.assert_allclose(run["T"].numpy(), ref["T"].numpy(), atol=2e-6, rtol=0)
    # 2. the four existing gradients and the three new ones
    for name in ALL7:
        g = run["grads"][name]
        if name == "k" and case[1] is None:
            assert ref["grads"][name] is None and g.shape == (B,) and (g == 0).all()       # 4. no robust loss: exactly 0
            continue
        assert g.shape == ref["grads"][name].shape
        close(g, ref["grads"][name], name)
    # the other backward shape (no cloud requires grad): the same hyper-parameter gradients, bit for bit
    two = _gpu(case, inp, vals, need=("weight", "T_init") + HNAMES)
    same(two, run, ("weight", "T_init") + HNAMES)
    # a parameter alone, the others numbers of pair 0: still its own (B,) gradient
    base, _ = _values(case, False)
    if case[1] is not None:
        solo = _gpu(case, inp, [torch.tensor([base[0]] * B), base[1], base[2]], need=("k",))
        assert solo["grads"]["k"].shape == (B,) and solo["grads"]["k"].abs().min() > 0
    # 3. shared values: a scalar's gradient is the fp32 rounding of the fp64 sum of the pairs' gradients of the same values
    _, equal = _values(case, False)
    per = _gpu(case, inp, equal)
    for shape in ((), (1,)):
        shared = _gpu(case, inp, [v[0].reshape(shape) for v in equal])
        same(shared, per, NAMES)
        for n in HNAMES:
            want = per["grads"][n].double().sum().float()
            assert shared["grads"][n].shape == shape and torch.equal(shared["grads"][n].reshape(()), want), n
    # 4. the hard gate: trim_dist (and the steepness) exactly 0, k as before
    hard = _gpu(case, inp, vals, gate="hard")
    assert (hard["grads"]["trim_dist"] == 0).all() and (hard["grads"]["trim_steep"] == 0).all()
    assert hard["grads"]["trim_dist"].shape == (B,)
    if case[1] is not None:
        assert hard["grads"]["k"].abs().min() > 0
    # 5. run to run, all seven
    again = _gpu(case, inp, vals)
    same(again, run, ALL7)


# ----------------------------------------------------------------------------- 4. a frozen pair's frozen iterations
@pytest.mark.parametrize("gate", ["hard", "tanh"])
def test_frozen_iterations_contribute_exactly_zero(nn_engine, gate):
    """The staggered-freeze batch of tests/icp_freeze_cases.py (pt2pt, Cauchy, dim 2, K = 8): a pair that froze after n
    iterations has, in every bit, the gradients of a run that stops after n -- its frozen iterations added exactly 0."""
    icp_type, loss, dim = "pt2pt", "cauchy", 2
    src, tgt, w, T0, G = fz.inputs(dim)
    tol = fz.TOLERANCE[(icp_type, loss, dim)]
    inp = {"x": [torch.from_numpy(v) for v in (src, tgt, w, T0)], "G": torch.from_numpy(G)}
    case = (icp_type, (loss, fz.METRIC), dim, None, 4.0)
    # (the batch's own trim distance of 3 m saturates a tanh gate of steepness 4: 0.6 m keeps it, and its gradients, awake;
    # the restatement's free run freezes the pairs after 8 / 7 / 3 iterations with either)
    trim = fz.TRIM if gate == "hard" else 0.6
    vals = [torch.tensor([v, v * 1.1, v * 0.9], dtype=torch.float32) for v in (fz.METRIC, trim, 4.0)]
    need = ("source", "weight", "T_init") + HNAMES       # (not the target: its fixed-point resolution depends on K itself)
    full = _gpu(case, inp, vals, need=need, gate=gate, K_=fz.K, tol=tol)
    n_active = full["active"][:fz.K].sum(0)
    print("ACTIVE iterations per pair (%s gate): %s" % (gate, n_active.tolist()))
    frozen = [b for b in range(fz.B) if 1 <= int(n_active[b]) <= fz.K - 2]
    assert frozen, n_active                                      # some pair sat frozen through two iterations at least
    for b in frozen:
        short = _gpu(case, inp, vals, need=need, gate=gate, K_=int(n_active[b]), tol=tol)
        assert torch.equal(short["T"][b], full["T"][b])
        for n in need:
            assert torch.equal(short["grads"][n][b], full["grads"][n][b]), (n, b)
        assert full["grads"]["k"][b] != 0
        if gate == "tanh":
            assert full["grads"]["trim_dist"][b] != 0 and full["grads"]["trim_steep"][b] != 0


# ----------------------------------------------------------------------------- 6. the status bit
def test_bad_value_on_the_device_raises_the_status_bit_and_nothing_else():
    case = CASES[0]
    inp = inputs(case)
    base, _ = _values(case, False)
    check_errors(wait=True)
    icp = ICP(icp_type=case[0], differentiable=False, max_iterations=2, tolerance=TOL)
    icp.trim, icp.tanh_steepness = "tanh", base[2]
    s, t, w, T0 = (v.to(DEV) for v in inp["x"])

    def call(k, trim=TRIM):
        return icp.icp(s, t, T_init=T0, weight=w, trim_dist=trim, loss_fn={"name": "cauchy", "metric": k}, dim=case[2])["T"]

    call(torch.tensor(-1.0, device=DEV))
    with pytest.raises(_lib.MmkError, match="MMK_ICP_STATUS_BAD_HYPER"):
        check_errors(wait=True)
    good = call(torch.tensor(base[0], device=DEV))                  # a flag, not a fault: the next call is clean
    check_errors(wait=True)
    assert torch.isfinite(good).all()
    call(torch.tensor([base[0], float("nan")], device=DEV))         # one bad pair is enough
    with pytest.raises(_lib.MmkError, match="MMK_ICP_STATUS_BAD_HYPER"):
        check_errors(wait=True)
    icp.trim = "hard"                                               # a value the call does not use is not looked at
    icp.tanh_steepness = torch.tensor(-5.0, device=DEV)
    call(base[0])
    icp.icp(s, t, T_init=T0, weight=w, trim_dist=TRIM, loss_fn={"name": "l2", "metric": torch.tensor(-1.0, device=DEV)}, dim=case[2])
    check_errors(wait=True)


# ----------------------------------------------------------------------------- 7. the policy
def test_policy_learns_the_three_values(scene64):
    scan, mp, T0, G = scene64
    kw = dict(dropout=0.0, mask_target="scan", icp_trim="tanh", icp_trim_dist=0.12)
    names = ("icp_metric", "icp_trim_dist_p", "icp_tanh_steepness_p")
    model, plain = policy(DEV, 3, learn_icp=("metric", "trim_dist", "tanh_steepness"), **kw), policy(DEV, 3, **kw)
    assert [n for n, _ in model.named_parameters() if n.startswith("icp_")] == list(names)
    assert not any(n.startswith("icp_") for n, _ in plain.named_parameters())
    model.train(), plain.train()
    # This scene's ICP converges to a pose with residuals near 0, which no weighting moves: the three gradients are of the
    # order 1e-14 .. 1e-11 (printed below).  Adam's first step is lr * g / (|g| + eps), so with the default eps = 1e-8 it
    # would be lost in the rounding of the parameters; a negligible eps makes the step lr * sign(g) whatever the scale.
    opt = torch.optim.Adam(model.parameters(), lr=1e-2, eps=1e-30)
    T, _, _ = model(scan, mp, T0)
    Tp, _, _ = plain(scan, mp, T0)
    assert torch.equal(T.detach(), Tp.detach())                   # the same pose as without learn_icp, bit for bit
    (T * G).sum().backward()
    before = {n: getattr(model, n).detach().clone() for n in names}
    for n in names:
        g = getattr(model, n).grad
        print("POLICY %s = %.4f, grad %.4e" % (n, before[n].item(), g.item()))
        assert g.shape == () and g.is_cuda and torch.isfinite(g) and g != 0, n
    opt.step()
    check_errors(wait=True)
    for n in names:
        assert getattr(model, n).detach() != before[n], n
    # evaluation: the inference instance (hard gate) uses the stepped metric and trim distance
    model.eval()
    with torch.no_grad():
        Te = model(scan, mp, T0)[0]
    net = {k: v for k, v in model.state_dict().items() if not k.startswith("icp_")}           # the stepped U-Net
    stepped = policy(DEV, 3, icp_loss_fn={"name": "cauchy", "metric": model.icp_metric.item()}, **dict(kw, icp_trim_dist=model.icp_trim_dist_p.item()))
    unstepped = policy(DEV, 3, **kw)
    for m in (stepped, unstepped):
        m.load_state_dict(net)
        m.eval()
    with torch.no_grad():
        Ts, Tu = stepped(scan, mp, T0)[0], unstepped(scan, mp, T0)[0]
    assert torch.equal(Te, Ts) and not torch.equal(Te, Tu)
    assert model.ICP_alg_inference.trim == "hard"
