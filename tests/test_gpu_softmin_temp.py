"""GPU: the soft-min temperature of the HIP dICP on the device, one value for the batch or one per pair, and its gradient
(mmk_icp_forward_soft_t / mmk_icp_backward_soft_t; DESIGN.md §3 I3⁗, I7⁗) against the restatement
tests/dicp_restatement.py.

Shapes, cases, inputs and ``close`` are those of tests/dicp_cases.py (its soft-min table): B = 2, 300 + 20 source rows (one
full and one partial 256-thread block), 700 + 30 target rows, K = 4, its five cases, k in {4, 8}; the reference replays the
device's idx_hist.  The reference runs once per (case, k, temperatures, correspondences) with tau as a (B,N) leaf: the
gradient of that leaf is every point's contribution summed over the iterations, its fp64 row sums g_b are the per-pair
references, and S_b = sum |contributions| makes the awake condition max_b |g_b| / S_b >= 0.03 (tests/test_gpu_icp_hyper.py's
threshold), asserted on the reference's values and printed next to tests/test_gpu_softmin.py's conditions (``assert_softmin_awake``).

Tolerances: pose 2e-6 absolute, gradients 2e-3 of the reference's largest magnitude per input (tests/test_gpu_point_grads.py's
bounds).  Equalities are exact: a tensor holding a number call's fp32 value gives that call's bits (0.25, and 0.3, which fp32
does not represent); a shared value's gradient is the fp32 rounding of the fp64 sum of the pairs' rows; a pair's frozen
iterations add 0; two runs agree in every bit.

Frozen iterations: the pt2pl, Huber, dim 2 batch of tests/icp_freeze_cases.py with K = 8, its TRIM and METRIC, the hard gate,
k = 4, tau = (0.25, 0.275, 0.225), tolerance 3e-5 -- on the CPU restatement the pairs stay active for 4, 3 and 2 iterations
and every step norm of an active pair is at least 14x away from the tolerance.

The policy: scene64 of tests/radar_cases.py, icp_softmin_temp = POLICY_TAU (see there).

Measured on an MI355X (all cases, k = 4 and 8): pose within 6.8e-7 of the replay; gradients within 4.0e-5 of the reference's
largest magnitude for the four inputs (weight, pt2pt Huber dim 3; source 1.3e-5, target 1.8e-5, T_init 6.6e-6 at most) and
1.1e-4 for tau with (0.25, 0.4), 5.8e-4 with (0.25, 0.25) (pt2pl, no loss, dim 2, tanh gate, k = 8, where pair 1's sum
cancels to 0.009 of its S).  The awake ratio max_b |g_b| / S_b on the replayed neighbours: smallest 0.102 with (0.25, 0.4)
(smallest single pair 0.055), smallest 0.055 with (0.25, 0.25) (pt2pl, Cauchy, dim 3, k = 8) -- the free run's figures of
tests/test_softmin_temp_cpu.py.  a_0 < 0.9 for 83 - 99 % of the real points in every iteration, 73 - 100 % pass the gate.  The
frozen batch's pairs stay active for 4, 3 and 2 iterations on the device as well.  The policy's gradient of
icp_softmin_temp_p at 0.25: 1.7637e-01.
"""
import numpy as np
import pytest
import torch

from mm_masking_amd import _lib
from mm_masking_amd.dICP.ICP import ICP, check_errors

import icp_freeze_cases as fz
from dicp_cases import (B, K, N, NAMES, PER_PAIR_TAU as PER_PAIR, SOFTMIN_CASES as CASES, SOFTMIN_IDS as IDS, SOFTMIN_TRIM as TRIM, TOL,
                        assert_softmin_awake, assert_tau_awake, close, gpu, inputs, reference, same)
from radar_cases import scene64  # noqa: F401  (the smallest scan-mode batch of the suite, a module fixture)
from support import DEV, policy

pytestmark = pytest.mark.gpu

ALL5 = NAMES + ("tau",)
EQUAL = (0.25, 0.25)
CASE_K = [(ci, 4) for ci in range(len(CASES))] + [(ci, 8) for ci in range(len(CASES))]
CASE_K_IDS = ["%s-k%d" % (IDS[ci], k) for ci, k in CASE_K]
# icp_softmin_temp of the policy test: out of {0.25, 0.05, 1.0} the first at which the gradient of icp_softmin_temp_p on
# scene64 is not exactly 0 -- 0.25 gives 1.7637e-01 (printed by the test)
POLICY_TAU = 0.25


def _gpu(case, inp, k, tau, need=ALL5, trim=TRIM, **kw):
    """One forward + backward with soft correspondences.  ``tau``: a float or a CPU tensor."""
    return gpu(case, inp, trim, need=need, softmin_k=k, tau=tau, **kw)


# ----------------------------------------------------------------------------- 1. same value, same bits
@pytest.mark.parametrize("ci,k", [(ci, 4) for ci in range(len(CASES))] + [(1, 8), (3, 8)],
                         ids=["%s-k4" % i for i in IDS] + ["%s-k8" % IDS[1], "%s-k8" % IDS[3]])
def test_a_tensor_with_a_number_calls_value_gives_its_bits(ci, k):
    case = CASES[ci]
    inp = inputs(case)
    value = 0.3 if ci == 1 else 0.25                             # 0.3 is not representable: the tensor holds its fp32 rounding
    for need in (NAMES, ("weight", "T_init")):                  # both backward shapes
        plain = gpu(case, inp, TRIM, need=need, softmin_k=k, tau=value)
        assert plain["fn"] == "_IcpSoftFunctionBackward"
        for tau in (torch.tensor(value), torch.tensor([value]), torch.tensor([value] * B), torch.tensor(value, dtype=torch.float64)):
            for with_grad in (need, need + ("tau",)):
                got = _gpu(case, inp, k, tau, need=with_grad)
                assert got["fn"] == "_IcpSoftTempFunctionBackward"
                same(got, plain, need)
                assert all(got["grads"][n] is None for n in NAMES if n not in need)
                assert (got["grads"]["tau"] is not None) == ("tau" in with_grad)


# ----------------------------------------------------------------------------- 2. per-pair values against the restatement
@pytest.mark.parametrize("ci,k", CASE_K, ids=CASE_K_IDS)
def test_per_pair_values_match_the_restatement(ci, k):
    case = CASES[ci]
    inp = inputs(case)
    run = _gpu(case, inp, k, torch.tensor(PER_PAIR))
    assert tuple(run["idx"].shape) == (K, B, N, k) and run["active"][:K].all()
    ref = reference(case, TRIM, fixed_idx=run["idx"], soft_k=k, taus=PER_PAIR)
    assert_softmin_awake(case, ref)
    assert_tau_awake(ref, PER_PAIR)
    err = (run["T"].double() - ref["T"].double()).abs().max().item()
    print("POSE max abs diff = %.3e" % err)
    np.testing.assert_allclose(run["T"].numpy(), ref["T"].numpy(), atol=2e-6, rtol=0)
    for name in ALL5:
        assert run["grads"][name].shape == ref["grads"][name].shape
        close(run["grads"][name], ref["grads"][name], name)
    # the other backward shape (no cloud requires grad): the same temperature gradient, bit for bit
    two = _gpu(case, inp, k, torch.tensor(PER_PAIR), need=("weight", "T_init", "tau"))
    same(two, run, ("weight", "T_init", "tau"))
    # per-pair values are not equal values
    assert not torch.equal(run["T"][1], _gpu(case, inp, k, torch.tensor(EQUAL))["T"][1])


# ----------------------------------------------------------------------------- 3. a shared value
@pytest.mark.parametrize("ci,k", CASE_K, ids=CASE_K_IDS)
def test_shared_value_gets_the_sum_of_the_pairs(ci, k):
    case = CASES[ci]
    inp = inputs(case)
    per = _gpu(case, inp, k, torch.tensor(EQUAL))
    ref = reference(case, TRIM, fixed_idx=per["idx"], soft_k=k, taus=EQUAL)
    assert_tau_awake(ref, EQUAL)
    close(per["grads"]["tau"], ref["grads"]["tau"], "tau (equal values)")
    want = per["grads"]["tau"].double().sum().float()
    for shape in ((), (1,)):
        shared = _gpu(case, inp, k, torch.tensor(EQUAL[0]).reshape(shape))
        same(shared, per, NAMES)
        assert shared["grads"]["tau"].shape == shape and torch.equal(shared["grads"]["tau"].reshape(()), want)
    half = _gpu(case, inp, k, torch.tensor(EQUAL[0], dtype=torch.float64))           # the gradient in the tensor's own dtype
    assert half["grads"]["tau"].dtype == torch.float64 and half["grads"]["tau"] == per["grads"]["tau"].double().sum()


# ----------------------------------------------------------------------------- 4. only tau requires grad
@pytest.mark.parametrize("ci,k", [(0, 4), (3, 8)], ids=["%s-k4" % IDS[0], "%s-k8" % IDS[3]])
def test_only_tau_requires_grad(ci, k):
    case = CASES[ci]
    inp = inputs(case)
    full = _gpu(case, inp, k, torch.tensor(PER_PAIR))
    solo = _gpu(case, inp, k, torch.tensor(PER_PAIR), need=("tau",))             # (_gpu asserts T.requires_grad)
    assert all(solo["grads"][n] is None for n in NAMES)
    assert torch.equal(solo["T"], full["T"]) and torch.equal(solo["idx"], full["idx"])
    assert torch.equal(solo["grads"]["tau"], full["grads"]["tau"]) and solo["grads"]["tau"].abs().min() > 0
    again = _gpu(case, inp, k, torch.tensor(PER_PAIR))
    same(again, full, ALL5)
    # nothing requires grad: the state-less soft forward with the device tau, and the pose of the call that saves its state
    icp = ICP(icp_type=case[0], differentiable=True, max_iterations=K, tolerance=TOL)
    icp.correspondence, icp.softmin_k, icp.softmin_temp = "softmin", k, torch.tensor(PER_PAIR, device=DEV)
    x = [v.to(DEV) for v in inp["x"]]
    T = icp.icp(x[0], x[1], T_init=x[3], weight=x[2], trim_dist=TRIM, loss_fn=inp["loss_fn"], dim=case[2])["T"]
    assert not T.requires_grad and tuple(icp.last_state["idx"].shape) == (1, B, N, k)
    assert torch.equal(T.cpu(), full["T"])


# ----------------------------------------------------------------------------- 5. a frozen pair's frozen iterations
def test_frozen_iterations_contribute_exactly_zero():
    """A pair that froze after n iterations has, in every bit, the pose and the gradients -- tau's included -- of a run that
    stops after n: its frozen iterations added exactly 0.  (Not the target: its fixed-point resolution depends on K itself.)"""
    icp_type, loss, dim = "pt2pl", "huber", 2
    src, tgt, w, T0, G = fz.inputs(dim)
    inp = {"x": [torch.from_numpy(v) for v in (src, tgt, w, T0)], "G": torch.from_numpy(G), "loss_fn": fz.loss_dict(loss)}
    case = (icp_type, (loss, fz.METRIC), dim, None, 0.0)
    tau, tol, k = torch.tensor([0.25, 0.275, 0.225]), 3e-5, 4
    need = ("source", "weight", "T_init", "tau")
    full = _gpu(case, inp, k, tau, need=need, K_=fz.K, tol=tol, trim=fz.TRIM)
    n_active = full["active"][:fz.K].sum(0)
    print("ACTIVE iterations per pair: %s" % n_active.tolist())
    frozen = [b for b in range(fz.B) if 1 <= int(n_active[b]) <= fz.K - 2]
    assert frozen, n_active                                      # some pair sat frozen through two iterations at least
    for b in frozen:
        short = _gpu(case, inp, k, tau, need=need, K_=int(n_active[b]), tol=tol, trim=fz.TRIM)
        assert torch.equal(short["T"][b], full["T"][b])
        for n in need:
            assert torch.equal(short["grads"][n][b], full["grads"][n][b]), (n, b)
        assert full["grads"]["tau"][b] != 0


# ----------------------------------------------------------------------------- 6. the status bit
def test_bad_value_on_the_device_raises_the_status_bit_and_nothing_else():
    case = CASES[0]
    inp = inputs(case)
    check_errors(wait=True)
    icp = ICP(icp_type=case[0], differentiable=True, max_iterations=2, tolerance=TOL)
    icp.correspondence, icp.softmin_k = "softmin", 4
    s, t, w, T0 = (v.to(DEV) for v in inp["x"])

    def call(tau):
        icp.softmin_temp = tau
        return icp.icp(s, t, T_init=T0, weight=w, trim_dist=TRIM, loss_fn=inp["loss_fn"], dim=case[2])["T"]

    for bad in (torch.tensor(-1.0, device=DEV), torch.tensor([0.0], device=DEV), torch.tensor([0.25, float("nan")], device=DEV)):
        call(bad)                                                   # (one bad pair is enough)
        assert tuple(icp.last_state["idx"].shape) == (1, B, N, 4)   # the soft forward ran, within its bounds
        with pytest.raises(_lib.MmkError, match="MMK_ICP_STATUS_BAD_HYPER"):
            check_errors(wait=True)
        good = call(torch.tensor(0.25, device=DEV))                 # a flag, not a fault: the next call is clean
        check_errors(wait=True)
        assert torch.isfinite(good).all()
    with torch.no_grad():                                           # nearest correspondences: the tensor is not looked at
        call(torch.tensor(-1.0, device=DEV))
    check_errors(wait=True)
    assert tuple(icp.last_state["idx"].shape) == (1, B, N)


# ----------------------------------------------------------------------------- 7. the policy
def test_policy_learns_the_temperature(scene64):
    scan, mp, T0, G = scene64
    kw = dict(dropout=0.0, mask_target="scan", icp_correspondence="softmin", icp_softmin_temp=POLICY_TAU)
    model, plain, hard = policy(DEV, 3, learn_icp=("softmin_temp",), **kw), policy(DEV, 3, **kw), policy(DEV, 3, dropout=0.0, mask_target="scan")
    assert [n for n, _ in model.named_parameters() if n.startswith("icp_")] == ["icp_softmin_temp_p"]
    assert not any(n.startswith("icp_") for n, _ in plain.named_parameters())
    model.train(), plain.train()
    # (a negligible eps makes Adam's first step lr * sign(g) whatever the gradient's scale: tests/test_gpu_icp_hyper.py)
    opt = torch.optim.Adam(model.parameters(), lr=1e-2, eps=1e-30)
    T, _, _ = model(scan, mp, T0)
    Tp, _, _ = plain(scan, mp, T0)
    assert torch.equal(T.detach(), Tp.detach())                   # the same pose as without learn_icp, bit for bit
    (T * G).sum().backward()
    q = model.icp_softmin_temp_p
    before, g = q.detach().clone(), q.grad
    print("POLICY icp_softmin_temp_p = %.4f, grad %.4e" % (before.item(), g.item()))
    assert g.shape == () and g.is_cuda and torch.isfinite(g) and g != 0
    opt.step()
    check_errors(wait=True)
    assert q.detach() != before
    # evaluation: the inference instance keeps nearest correspondences -- the hard model's bits for the same U-Net
    hard.load_state_dict({k: v for k, v in model.state_dict().items() if not k.startswith("icp_")})
    model.eval(), hard.eval()
    with torch.no_grad():
        Te, Th = model(scan, mp, T0)[0], hard(scan, mp, T0)[0]
    assert torch.equal(Te, Th) and model.ICP_alg_inference.correspondence == "nearest"
