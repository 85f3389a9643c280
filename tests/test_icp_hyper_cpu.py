"""CPU: the dICP's device-resident, learnable robust scale k, trim distance and steepness (DESIGN.md §3 I3'', I7'').  The
restatement tests/dicp_restatement.py -- the same bits for equal values given as numbers or as tensors of any accepted shape,
the closed forms of I7'' against its autograd, fp64 finite differences per pair -- and the host plumbing: the _hp entries of
the C ABI and their argument checks, dICP.ICP's shape validation, the policy's params["learn_icp"]."""
import ctypes
import importlib
import os
import re

import numpy as np
import pytest
import torch

from mm_masking_amd import _lib, synthetic
from mm_masking_amd.dICP.ICP import ICP

icp_mod = importlib.import_module("mm_masking_amd.dICP.ICP")        # (the package re-exports the class under the module's name)

from dicp_cases import policy_params
from dicp_restatement import ICPRestatement, closed_form_sums
from support import ROOT, icp_params, n_args
B, N, M, K = 2, 70, 160, 3
TRIM, STEEP = 0.6, 4.0
#        type     loss      k    dim noise
CASES = [("pt2pt", "cauchy", 0.5, 2, 0.01),
         ("pt2pl", "huber", 0.1, 2, 0.15),
         ("pt2pt", "huber", 0.5, 3, 0.01),
         ("pt2pl", "cauchy", 0.5, 3, 0.15),
         ("pt2pl", None, 1.0, 2, 0.15)]
IDS = ["%s-%s-d%d" % (c[0], c[1] or "none", c[3]) for c in CASES]


def _inputs(case):
    _, _, _, dim, noise = case
    S, Tg = [], []
    for b in range(B):
        s, t, _ = synthetic.simple_cloud_pair(77 + dim + b, N, M, dim=dim, noise=noise, yaw=0.02 + 0.01 * b, trans=(0.6, -0.4 + 0.1 * b, 0.1))
        S.append(s), Tg.append(t)
    w = np.random.default_rng(2).uniform(0.2, 1.0, (B, N)).astype(np.float32)
    T0 = torch.eye(4).repeat(B, 1, 1)
    T0[:, 0, 3] += 0.2
    G = torch.from_numpy(np.random.default_rng(3).normal(size=(B, 4, 4)).astype(np.float32))
    return torch.from_numpy(np.stack(S)), torch.from_numpy(np.stack(Tg)), torch.from_numpy(w), T0, G


# ----------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("ci", range(len(CASES)), ids=IDS)
@pytest.mark.parametrize("soft", [True, False], ids=["soft", "hard"])
def test_plain_equal_values_are_the_soft_trim_restatement_bit_for_bit(ci, soft):
    """A number, a 0-d tensor, a (B,) tensor and a (B,N) tensor of equal value give the same bits."""
    icp_type, loss, k, dim, _ = CASES[ci]
    src, tgt, w, T0, G = _inputs(CASES[ci])
    new = ICPRestatement(icp_type, differentiable=True, max_iterations=K, tolerance=1e-9, soft=soft)
    leaves_o = [v.clone().requires_grad_(True) for v in (src, tgt, w, T0)]
    a = new.icp(leaves_o[0], leaves_o[1], T_init=leaves_o[3], weight=leaves_o[2], k=k, trim_dist=TRIM, trim_steep=STEEP, loss_name=loss,
                dim=dim)
    (a["T"] * G).sum().backward()
    for shape in ((), (B,), (B, N)):
        leaves_n = [v.clone().requires_grad_(True) for v in (src, tgt, w, T0)]
        hy = [torch.full(shape, v, dtype=torch.float32) for v in (k, TRIM, STEEP)]
        b = new.icp(leaves_n[0], leaves_n[1], T_init=leaves_n[3], weight=leaves_n[2], k=hy[0], trim_dist=hy[1], trim_steep=hy[2],
                    loss_name=loss, dim=dim)
        (b["T"] * G).sum().backward()
        assert a["num_iter"] == b["num_iter"] == K and torch.equal(a["T"], b["T"])
        for name in ("idx", "T", "delta", "keep", "A", "b", "huber_out"):
            for x, y in zip(a["hist"][name], b["hist"][name]):
                assert torch.equal(x, y), (name, shape)
        for x, y in zip(leaves_o, leaves_n):
            assert torch.equal(x.grad, y.grad), shape


def _fixed_run(case, soft, hyper_shape, dtype=torch.float64, mult=(1.3, 1.15, 0.8)):
    """The restatement with fixed correspondences (a free fp32 run's) and per-pair values: pair 1 scaled by ``mult``."""
    icp_type, loss, k, dim, _ = case
    src, tgt, w, T0, G = _inputs(case)
    vals = [torch.tensor([v, v * m]) for v, m in zip((k, TRIM, STEEP), mult)]
    free = ICPRestatement(icp_type, differentiable=False, max_iterations=K, tolerance=1e-12, soft=soft).icp(
        src, tgt, T_init=T0, weight=w, k=vals[0], trim_dist=vals[1], trim_steep=vals[2], loss_name=loss, dim=dim)
    fixed = free["hist"]["idx"]
    assert len(fixed) == K
    ref = ICPRestatement(icp_type, differentiable=True, max_iterations=K, tolerance=1e-12, soft=soft)

    def run(kk, cc, ss):
        return ref.icp(src, tgt, T_init=T0, weight=w, k=kk, trim_dist=cc, trim_steep=ss, loss_name=loss, dim=dim, dtype=dtype,
                       fixed_idx=fixed)

    if hyper_shape == "BN":
        vals = [v[:, None].expand(B, N).contiguous() for v in vals]
    leaves = [v.to(dtype).clone().requires_grad_(True) for v in vals]
    return run, leaves, G.to(dtype)


@pytest.mark.parametrize("ci", range(len(CASES)), ids=IDS)
@pytest.mark.parametrize("soft", [True, False], ids=["soft", "hard"])
def test_closed_forms_of_I7_match_autograd(ci, soft):
    """k̄_i, c̄_i, s̄_i of I7'' in numpy from (wbar, omega, keep, rho, r2, d, th) against autograd's gradient of (B,N)-shaped
    leaves of the restatement (fp64: agreement to rounding), and their pair sums against the gradient of (B,) leaves."""
    case = CASES[ci]
    loss = case[1]
    run, leaves, G = _fixed_run(case, soft, "BN")
    out = run(*leaves)
    if out["T"].requires_grad:
        (out["T"] * G).sum().backward()
    else:
        assert loss is None and not soft                 # hard gate, no robust loss: the pose does not read any of the three
    got = closed_form_sums(out["hist"], *(v.detach().numpy() for v in leaves), loss, soft)
    auto = [np.zeros((B, N)) if v.grad is None else v.grad.numpy() for v in leaves]
    for c, name in enumerate(("k", "trim_dist", "trim_steep")):
        scale = np.abs(auto[c]).max()
        if (name == "k" and loss is None) or (name != "k" and not soft):
            assert scale == 0 and (got[c] == 0).all(), name                  # the structural zeros
            continue
        assert scale > 0, name
        assert np.abs(got[c] - auto[c]).max() <= 1e-11 * scale, (name, np.abs(got[c] - auto[c]).max(), scale)
    run_b, leaves_b, _ = _fixed_run(case, soft, "B")
    T_b = run_b(*leaves_b)["T"]
    if T_b.requires_grad:
        (T_b * G).sum().backward()
    for c in range(3):
        if leaves_b[c].grad is not None:
            np.testing.assert_allclose(leaves_b[c].grad.numpy(), auto[c].sum(1), rtol=1e-9, atol=1e-12 * max(1.0, np.abs(auto[c]).sum()))
    if loss == "huber":                     # points on both sides of the knee, so both branches of k̄ are exercised
        out_share = float(torch.stack(out["hist"]["huber_out"]).double().mean())
        print("HUBER r > k share: %.2f" % out_share)
        assert 0.1 <= out_share <= 0.9, out_share


@pytest.mark.parametrize("ci", range(len(CASES)), ids=IDS)
def test_finite_differences_per_pair(ci):
    """fp64 central differences of the restatement (fixed correspondences, soft gate) in k, trim_dist and the steepness of
    each pair, against its autograd: bound and step of tests/test_soft_trim_cpu.py's finite-difference test."""
    case = CASES[ci]
    loss = case[1]
    run, leaves, G = _fixed_run(case, True, "B")
    out = run(*leaves)
    (out["T"] * G).sum().backward()
    if loss == "huber":
        share = float(torch.stack(out["hist"]["huber_out"]).double().mean())
        assert 0.1 <= share <= 0.9, share
    eps, worst = 1e-6, 0.0
    for c, name in enumerate(("k", "trim_dist", "trim_steep")):
        if name == "k" and loss is None:
            assert leaves[c].grad is None or (leaves[c].grad == 0).all()
            continue
        for b in range(B):
            ap = [v.detach().clone() for v in leaves]
            am = [v.detach().clone() for v in leaves]
            ap[c][b] += eps
            am[c][b] -= eps
            with torch.no_grad():
                fd = ((run(*ap)["T"] * G).sum() - (run(*am)["T"] * G).sum()).item() / (2 * eps)
            g = leaves[c].grad[b].item()
            bound = 1e-5 * max(1e-3, abs(fd)) + 1e-8
            worst = max(worst, abs(fd - g) / bound)
            assert abs(fd - g) <= bound, (name, b, fd, g)
            assert g != 0.0, (name, b)
    print("FD %s: worst deviation %.2f of the bound" % (IDS[ci], worst))


# ----------------------------------------------------------------------------- the C ABI
@pytest.fixture(scope="module")
def L():
    _lib.build()
    return _lib.lib()


def test_hp_entries_exist_and_older_sizes_are_unchanged(L):
    raw = open(os.path.join(ROOT, "include", "mmk.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name in ("mmk_icp_forward_hp", "mmk_icp_backward_hp_workspace_bytes", "mmk_icp_backward_hp"):
        assert hasattr(L, name) and name in _lib.EXPORTED, name
        assert n_args(hdr, name) == len(_lib.EXPORTED[name][1]), name
    assert n_args(hdr, "mmk_icp_forward_hp") == n_args(hdr, "mmk_icp_forward") + 2
    assert n_args(hdr, "mmk_icp_backward_hp") == n_args(hdr, "mmk_icp_backward_points") + 3
    assert int(re.search(r"#define\s+MMK_ICP_STATUS_BAD_HYPER\s+(\d+)", raw).group(1)) == icp_mod.ICP_STATUS_BAD_HYPER == 2
    assert ctypes.sizeof(_lib.IcpParams) == L.mmk_icp_params_bytes() == 60          # the struct did not grow
    for p in (icp_params(), icp_params(trim_steep=4.0), icp_params(N=1000, dim=3, nn_method=1)):
        r = ctypes.byref(p)
        base = L.mmk_icp_backward_points_workspace_bytes(r, 0)
        assert base == L.mmk_icp_workspace_bytes(r) > 0
        # without the array: the sizes of the older entries; with it: the block partials behind them, (K, B, nblk, 3) fp64
        assert L.mmk_icp_backward_hp_workspace_bytes(r, 0, 0) == base
        assert L.mmk_icp_backward_hp_workspace_bytes(r, 1, 0) == L.mmk_icp_backward_points_workspace_bytes(r, 1)
        extra = p.max_iter * p.B * ((p.N + 255) // 256) * 3 * 8
        for wt in (0, 1):
            got = L.mmk_icp_backward_hp_workspace_bytes(r, wt, 1) - L.mmk_icp_backward_points_workspace_bytes(r, wt)
            assert extra <= got <= extra + 256, (got, extra)


def test_hp_argument_errors(L):
    null, fake = ctypes.c_void_p(0), ctypes.c_void_p(4096)       # never dereferenced: every call fails before any launch
    iters = ctypes.c_int(0)
    p = icp_params()
    for per_pair in (2, -1):
        assert L.mmk_icp_forward_hp(ctypes.byref(p), *([fake] * 10), fake, per_pair, fake, 1 << 30, ctypes.byref(iters), null) == -1
        assert b"per_pair" in L.mmk_last_error()
        assert L.mmk_icp_backward_hp(ctypes.byref(p), *([fake] * 13), fake, per_pair, fake, fake, 1 << 30, null) == -1
        assert b"per_pair" in L.mmk_last_error()
    assert L.mmk_icp_backward_hp(ctypes.byref(p), *([fake] * 13), null, 0, fake, fake, 1 << 30, null) == -1
    assert b"grad_hyper needs hyper" in L.mmk_last_error()
    assert L.mmk_icp_backward_hp(ctypes.byref(p), *([fake] * 13), fake, 0, fake, fake, 64, null) == -1
    assert b"workspace too small" in L.mmk_last_error()
    assert L.mmk_icp_backward_hp(ctypes.byref(icp_params(save_state=0)), *([fake] * 13), fake, 0, fake, fake, 1 << 30, null) == -1
    assert b"save_state" in L.mmk_last_error()
    bad = icp_params(trim_steep=-1.0)
    assert L.mmk_icp_backward_hp_workspace_bytes(ctypes.byref(bad), 1, 1) == 0 and b"trim_steep" in L.mmk_last_error()
    assert L.mmk_icp_forward_hp(ctypes.byref(bad), *([fake] * 10), fake, 0, fake, 1 << 30, ctypes.byref(iters), null) == -1


# ----------------------------------------------------------------------------- dICP.ICP
def test_shape_validation_happens_before_the_device_is_touched(monkeypatch):
    monkeypatch.setattr(_lib, "lib", lambda: pytest.fail("the library was loaded"))
    src, tgt = torch.zeros(3, 8, 3), torch.zeros(3, 9, 3)
    icp = ICP("pt2pt", differentiable=True, max_iterations=2)
    for bad in (torch.ones(2), torch.ones(3, 1), torch.ones(1, 1), torch.ones(4), torch.ones(3, 8)):
        with pytest.raises(ValueError, match="trim_dist"):
            icp.icp(src, tgt, trim_dist=bad, dim=2)
        with pytest.raises(ValueError, match="metric"):
            icp.icp(src, tgt, loss_fn={"name": "cauchy", "metric": bad}, dim=2)
        icp.trim, icp.tanh_steepness = "tanh", bad
        with pytest.raises(ValueError, match="tanh_steepness"):
            icp.icp(src, tgt, dim=2)
        icp.trim, icp.tanh_steepness = "hard", 10.0
    with pytest.raises(ValueError, match="floating"):
        icp.icp(src, tgt, trim_dist=torch.ones(3, dtype=torch.int64), dim=2)
    assert icp_mod._hyper_sizes((1.0, 5.0, 10.0), 3) is None                    # numbers only: the call it always was
    assert icp_mod._hyper_sizes((torch.tensor(1.0), 5.0, 10.0), 3) is False
    assert icp_mod._hyper_sizes((1.0, torch.ones(1), 10.0), 3) is False
    assert icp_mod._hyper_sizes((1.0, torch.ones(1), torch.ones(3)), 3) is True
    assert icp_mod._hyper_sizes((1.0, torch.ones(1), 10.0), 1) is False         # B == 1: (1,) is the shared value
    h = icp_mod._hyper_array((torch.tensor([0.5, 0.7], dtype=torch.float64), 5, torch.tensor(4.0)), True, 2, torch.device("cpu"))
    assert h.dtype == torch.float32 and h.is_contiguous()
    assert torch.equal(h, torch.tensor([[0.5, 5.0, 4.0], [0.7, 5.0, 4.0]]))
    h = icp_mod._hyper_array((0.5, torch.tensor([5.0]), 4.0), False, 2, torch.device("cpu"))
    assert torch.equal(h, torch.tensor([[0.5, 5.0, 4.0]]))


def test_params_of_a_tensor_call_carry_only_the_gate_mode():
    icp = ICP("pt2pt", differentiable=True, max_iterations=3)
    icp.trim, icp.tanh_steepness = "tanh", torch.tensor(-3.0)      # (a tensor is not validated on the host: the device flag is)
    p = icp._params(1, 8, 8, 3, 2, {"name": "cauchy", "metric": torch.tensor(2.0)}, torch.tensor(1.0), True, on_device=True)
    assert p.trim_steep > 0 and p.loss == 1
    icp.trim = "hard"
    assert icp._params(1, 8, 8, 3, 2, None, torch.tensor(1.0), True, on_device=True).trim_steep == 0.0
    icp.trim, icp.tanh_steepness = "tanh", 2.5                       # a number among tensors keeps its host validation
    assert icp._params(1, 8, 8, 3, 2, None, torch.tensor(1.0), True, on_device=True).trim_steep == 2.5
    icp.tanh_steepness = -1.0
    with pytest.raises(ValueError, match="tanh_steepness"):
        icp._params(1, 8, 8, 3, 2, None, torch.tensor(1.0), True, on_device=True)


def test_status_bit_becomes_an_error_that_names_the_parameters():
    watch = icp_mod._StatusWatch()

    class Done:
        def synchronize(self):
            pass

        def query(self):
            return True

    watch.pending.append((Done(), torch.tensor([icp_mod.ICP_STATUS_BAD_HYPER], dtype=torch.int32)))
    with pytest.raises(_lib.MmkError, match="metric.*trim_dist.*tanh_steepness"):
        watch.check(wait=True)
    watch.check(wait=True)                                          # reported once


# ----------------------------------------------------------------------------- the policy
def test_policy_learn_icp_parameters_and_errors():
    from mm_masking_amd.icp_weight_policy import LearnICPWeightPolicy
    base = LearnICPWeightPolicy(policy_params())
    keys = list(base.state_dict().keys())
    assert len(list(base.parameters())) == 46 and base.learn_icp == ()
    assert not any(k.startswith("icp_") for k in keys)
    soft = LearnICPWeightPolicy(policy_params(icp_trim="tanh"))
    assert list(soft.state_dict().keys()) == keys
    m = LearnICPWeightPolicy(policy_params(icp_trim="tanh", icp_trim_dist=0.12, icp_tanh_steepness=7.0,
                                            icp_loss_fn={"name": "huber", "metric": 0.3},
                                            learn_icp=("metric", "trim_dist", "tanh_steepness")))
    new = ["icp_metric", "icp_trim_dist_p", "icp_tanh_steepness_p"]     # (a module's own parameters precede its children's)
    assert list(m.state_dict().keys()) == new + keys
    assert len(list(m.parameters())) == 49
    for name, v in (("icp_metric", 0.3), ("icp_trim_dist_p", 0.12), ("icp_tanh_steepness_p", 7.0)):
        q = getattr(m, name)
        assert isinstance(q, torch.nn.Parameter) and q.shape == () and q.dtype == torch.float32 and q.requires_grad
        assert q.item() == np.float32(v)
    only = LearnICPWeightPolicy(policy_params(learn_icp=("metric",)))              # the default Cauchy loss, hard gate
    assert list(only.state_dict().keys()) == ["icp_metric"] + keys and only.icp_metric.item() == 1.0
    for bad, msg in ((dict(learn_icp=("trim_dist",)), "icp_trim='tanh'"),
                     (dict(learn_icp=("tanh_steepness",)), "icp_trim='tanh'"),
                     (dict(learn_icp=("metric",), icp_loss_fn=None), "robust loss"),
                     (dict(learn_icp=("metric",), icp_loss_fn={"name": "l2"}), "robust loss"),
                     (dict(learn_icp=("tolerance",), icp_trim="tanh"), "unknown name")):
        with pytest.raises(ValueError, match=msg):
            LearnICPWeightPolicy(policy_params(**bad))


def test_policy_hands_the_parameters_to_the_right_instance():
    from mm_masking_amd.icp_weight_policy import LearnICPWeightPolicy
    m = LearnICPWeightPolicy(policy_params(icp_trim="tanh", learn_icp=("metric", "trim_dist", "tanh_steepness")))
    seen = []

    def fake(name):
        def icp(scan_pc, map_pc, T_init=None, weight=None, trim_dist=None, loss_fn=None, dim=None):
            seen.append((name, trim_dist, loss_fn["metric"]))
            return {"T": T_init}
        return icp

    m.ICP_alg.icp, m.ICP_alg_inference.icp = fake("train"), fake("infer")
    m.train()
    m.icp(None, None, torch.eye(4)[None], None)
    assert seen[-1][0] == "train" and seen[-1][1] is m.icp_trim_dist_p and seen[-1][2] is m.icp_metric
    assert m.ICP_alg.tanh_steepness is m.icp_tanh_steepness_p
    m.eval()
    m.icp(None, None, torch.eye(4)[None], None)
    name, c, k = seen[-1]
    assert name == "infer" and not c.requires_grad and not k.requires_grad
    assert c.data_ptr() == m.icp_trim_dist_p.data_ptr() and k.data_ptr() == m.icp_metric.data_ptr()     # the learned values
    assert m.ICP_alg_inference.trim == "hard" and not isinstance(m.ICP_alg_inference.tanh_steepness, torch.Tensor)
    assert m.icp_loss_fn["metric"] == 1.0                           # the configured dictionary is left alone
