"""CPU: the soft (tanh) trim gate of the dICP (DESIGN.md §3 I3', I7').  The restatement tests/dicp_restatement.py -- known
answers of the gate, its hard limit against oracle.dicp_ref, finite differences of its autograd in fp64 -- and the host
plumbing of the option: mmk_icp_params.trim_steep / mmk_icp_params_bytes, the argument checks, dICP.ICP's YAML keys and
attributes, and the policy's params["icp_trim"] / ["icp_tanh_steepness"]."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

from mm_masking_amd import _lib, synthetic
from mm_masking_amd.dICP.ICP import ICP
from oracle import dicp_ref

from dicp_restatement import ICPRestatement, band_share, soft_keep
from support import ROOT, icp_params, icp_yaml, policy_params


# ----------------------------------------------------------------------------- the gate itself
@pytest.mark.parametrize("dt", [torch.float32, torch.float64])
def test_gate_known_answers(dt):
    trim, steep = 0.6, 4.0
    # exactly one half at d == trim_dist (sqrt(fl(v v)) == v in IEEE arithmetic)
    for v in (trim, 2.0, 0.25, 1.5):
        d = torch.tensor([v], dtype=dt)
        assert soft_keep(d * d, v, steep).item() == 0.5
    # saturated once |steep (d - trim)| >= 20: exactly 1 inside, exactly 0 outside
    inside = torch.tensor([0.0, 0.5, 0.999], dtype=dt)            # trim 6, steep 4: arguments <= -20
    outside = torch.tensor([11.0, 12.5, 1400.0], dtype=dt)        # >= +20 (1400 m: a target_pad_val row)
    assert (soft_keep(inside * inside, 6.0, 4.0) == 1.0).all()
    assert (soft_keep(outside * outside, 6.0, 4.0) == 0.0).all()
    assert soft_keep(torch.tensor([5.0 ** 2], dtype=dt), 7.0, 10.0).item() == 1.0      # argument -20 itself
    assert soft_keep(torch.tensor([9.0 ** 2], dtype=dt), 7.0, 10.0).item() == 0.0      # argument +20 itself
    # monotone (non-increasing) in d, strictly inside the band
    d = torch.linspace(0.0, 8.0, 4001, dtype=dt)
    k = soft_keep(d * d, trim, steep)
    assert (k[1:] <= k[:-1]).all() and k[0] > 0.9 and k[-1] == 0.0
    band = (k > 0.05) & (k < 0.95)
    assert band.sum() > 100 and (k[1:][band[1:]] < k[:-1][band[1:]]).all()
    # finite, zero slope at a coincident point
    d2 = torch.zeros(3, dtype=dt, requires_grad=True)
    soft_keep(d2, trim, steep).sum().backward()
    assert (d2.grad == 0).all()


def _point_grad_inputs(dim, n=80, m=200):
    """The inputs of tests/test_point_grads_cpu.py::test_oracle_cloud_gradients_finite_difference."""
    src, tgt, _ = synthetic.simple_cloud_pair(40 + dim, n, m, dim=dim, yaw=0.03, trans=(0.5, -0.3, 0.1))
    w = torch.from_numpy(np.random.default_rng(3).uniform(0.2, 1.0, (1, n)))
    return torch.from_numpy(src)[None], torch.from_numpy(tgt)[None], w


@pytest.mark.parametrize("icp_type,dim", [("pt2pt", 2), ("pt2pl", 2), ("pt2pt", 3), ("pt2pl", 3)])
def test_gate_off_is_the_oracle_and_steep_gate_is_the_hard_gate(icp_type, dim):
    """trim_steep = 0: what oracle.dicp_ref.ICPRef returns, bit for bit.  Steepness 1e4 with no point within 1e-2 m of
    trim_dist: every gate is exactly 0 or 1, so poses and index histories are the hard oracle's, bit for bit."""
    src, tgt, w = _point_grad_inputs(dim)
    loss_fn, K = {"name": "cauchy", "metric": 1.0}, 3
    kw = dict(T_init=torch.eye(4)[None], weight=w.float(), dim=dim)
    loss = dict(loss_name=loss_fn["name"], k=loss_fn["metric"])
    for trim in (5.0,):               # the inputs' own setting
        hard = dicp_ref.ICPRef(icp_type, differentiable=True, max_iterations=K, tolerance=1e-12).icp(src, tgt, trim_dist=trim,
                                                                                                     loss_fn=loss_fn, **kw)
        off = ICPRestatement(icp_type, max_iterations=K, tolerance=1e-12, soft=False).icp(src, tgt, trim_dist=trim, **loss, **kw)
        steep = ICPRestatement(icp_type, max_iterations=K, tolerance=1e-12, soft=True).icp(src, tgt, trim_dist=trim, trim_steep=1e4,
                                                                                           **loss, **kw)
        d = torch.sqrt(torch.stack(steep["hist"]["d2"]))
        assert (d - trim).abs().min() >= 1e-2, float((d - trim).abs().min())
        kept = torch.stack(steep["hist"]["keep"])
        assert ((kept == 0) | (kept == 1)).all() and torch.equal(kept == 1, d < trim)
        for got in (off, steep):
            assert got["num_iter"] == hard["num_iter"] == K
            assert torch.equal(got["T"], hard["T"])
            for a, b in zip(got["hist"]["idx"] + got["hist"]["T"] + got["hist"]["delta"],
                            hard["hist"]["idx"] + hard["hist"]["T"] + hard["hist"]["delta"]):
                assert torch.equal(a, b)


@pytest.mark.parametrize("icp_type,dim", [("pt2pt", 2), ("pt2pl", 2), ("pt2pt", 3), ("pt2pl", 3)])
def test_soft_gate_gradients_finite_difference(icp_type, dim):
    """Autograd through the restatement (fp64, fixed correspondences) against central differences in source, target xyz (and
    normals), weight and T_init: recipe and bound of test_oracle_cloud_gradients_finite_difference.  One source point
    coincides with its correspondent (d == 0 at T_init = I); a fifth at least of the points of the K iterations sit in the
    gate's band (0.05 < keep < 0.95), so the check cannot pass on a saturated gate."""
    n, m, K = 80, 200, 3
    trim, steepness = 0.6, 4.0
    src, tgt, _ = synthetic.simple_cloud_pair(40 + dim, n, m, dim=dim, noise=0.1, yaw=0.03, trans=(0.5, -0.3, 0.1))
    src[5] = tgt[11, :3]
    src, tgt = torch.from_numpy(src)[None], torch.from_numpy(tgt)[None]
    w0 = torch.from_numpy(np.random.default_rng(3).uniform(0.2, 1.0, (1, n)))
    G = torch.from_numpy(np.random.default_rng(4).normal(size=(1, 4, 4)))
    loss_fn = {"name": "cauchy", "metric": 1.0}
    ref = ICPRestatement(icp_type, differentiable=True, max_iterations=K, tolerance=1e-12, soft=True)
    hyper = dict(k=loss_fn["metric"], trim_dist=trim, trim_steep=steepness, loss_name=loss_fn["name"], dim=dim)
    free = ref.icp(src, tgt, T_init=torch.eye(4)[None], weight=w0.float(), **hyper)
    fixed = free["hist"]["idx"]
    assert len(fixed) == K and int(fixed[0][0, 5]) == 11 and float(free["hist"]["d2"][0][0, 5]) == 0.0

    def run(s, t, w, T0):
        return ref.icp(s, t, T_init=T0, weight=w, dtype=torch.float64, fixed_idx=fixed, **hyper)

    def f(s, t, w, T0):
        return (run(s, t, w, T0)["T"] * G).sum()

    leaves = [src.double(), tgt.double(), w0.clone(), torch.eye(4, dtype=torch.float64)[None]]
    for v in leaves:
        v.requires_grad_(True)
    out = run(*leaves)
    real = torch.ones(1, n, dtype=torch.bool)
    shares = [band_share(k, real) for k in out["hist"]["keep"]]
    print("BAND SHARE %s dim %d: %s" % (icp_type, dim, ["%.2f" % v for v in shares]))
    share = band_share(torch.stack(out["hist"]["keep"]), real[None].expand(K, 1, n))       # over the points of all iterations
    assert share >= 0.2, (share, shares)
    assert float(out["hist"]["d2"][0][0, 5]) == 0.0
    (out["T"] * G).sum().backward()
    grads = [v.grad for v in leaves]
    assert all(torch.isfinite(g).all() for g in grads)
    gs, gt = grads[0][0], grads[1][0]
    used = torch.unique(torch.cat([ix[0].long() for ix in fixed]))
    if dim == 2:
        assert (gs[:, 2] == 0).all()
    assert (gt[:, dim:3] == 0).all() and (gt[:, 3 + (dim if icp_type == "pt2pl" else 0):] == 0).all()

    eps = 1e-6
    checks = [(0, (0, i, c)) for i, c in ((0, 0), (17, 1), (63, dim - 1))]
    for j in used[[0, len(used) // 2, -1]].tolist():
        checks += [(1, (0, j, c)) for c in range(dim)]
        if icp_type == "pt2pl":
            checks += [(1, (0, j, 3 + c)) for c in range(dim)]
    checks += [(2, (0, i)) for i in (0, 17, 63)]
    checks += [(3, (0, r, c)) for r, c in ((0, 3), (1, 3), (0, 0), (0, 1), (1, 0), (1, 1))]
    if dim == 3:
        checks += [(3, (0, r, c)) for r, c in ((2, 3), (2, 1), (0, 2))]
    worst = 0.0
    for which, at in checks:
        args_p = [v.detach().clone() for v in leaves]
        args_m = [v.detach().clone() for v in leaves]
        args_p[which][at] += eps
        args_m[which][at] -= eps
        fd = (f(*args_p) - f(*args_m)).item() / (2 * eps)
        g = grads[which][at].item()
        bound = 1e-5 * max(1e-3, abs(fd)) + 1e-8
        worst = max(worst, abs(fd - g) / bound)
        assert abs(fd - g) <= bound, (which, at, fd, g)
    print("FD %s dim %d: worst deviation %.2f of the bound" % (icp_type, dim, worst))


# ----------------------------------------------------------------------------- host plumbing
@pytest.fixture(scope="module")
def L():
    _lib.build()
    return _lib.lib()


def test_params_struct_and_new_symbol(L):
    assert icp_params().trim_steep == 0.0                       # keyword constructions that never mention it: the hard gate
    assert icp_params(trim_steep=4.0).trim_steep == 4.0
    assert _lib.IcpParams._fields_[-1][0] == "trim_steep"    # appended: every earlier field keeps its offset
    assert _lib.IcpParams.nn_method.offset + 4 == _lib.IcpParams.trim_steep.offset
    assert ctypes.sizeof(_lib.IcpParams) == L.mmk_icp_params_bytes()
    raw = open(os.path.join(ROOT, "include", "mmk.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    assert re.search(r"\bsize_t\s+mmk_icp_params_bytes\s*\(\s*void\s*\)", hdr)
    assert hasattr(L, "mmk_icp_params_bytes") and "mmk_icp_params_bytes" in _lib.EXPORTED
    struct = re.search(r"typedef struct \{([^}]*)\} mmk_icp_params;", hdr).group(1)
    names = re.findall(r"\b(?:int32_t|float)\s+(\w+)\s*;", struct)
    assert names == [f[0] for f in _lib.IcpParams._fields_]
    assert L.mmk_version() == int(re.search(r"#define\s+MMK_VERSION\s+(\d+)", raw).group(1))


@pytest.mark.parametrize("bad", [-1.0, float("nan"), float("inf"), -0.5])
def test_bad_trim_steep_is_an_argument_error(L, bad):
    p = icp_params(trim_steep=bad)
    null, fake = ctypes.c_void_p(0), ctypes.c_void_p(4096)       # never dereferenced: every call fails before any launch
    assert L.mmk_icp_workspace_bytes(ctypes.byref(p)) == 0 and b"trim_steep" in L.mmk_last_error()
    assert L.mmk_icp_backward_points_workspace_bytes(ctypes.byref(p), 1) == 0 and b"trim_steep" in L.mmk_last_error()
    assert L.mmk_icp_partials_count(ctypes.byref(p)) == 0
    iters = ctypes.c_int(0)
    calls = [
        lambda: L.mmk_icp_forward(ctypes.byref(p), *([fake] * 10), fake, 1 << 30, ctypes.byref(iters), null),
        lambda: L.mmk_icp_backward(ctypes.byref(p), *([fake] * 11), fake, 1 << 30, null),
        lambda: L.mmk_icp_backward_points(ctypes.byref(p), *([fake] * 13), fake, 1 << 30, null),
        lambda: L.mmk_icp_accumulate(ctypes.byref(p), *([fake] * 8), null),
        lambda: L.mmk_icp_solve_update(ctypes.byref(p), *([fake] * 7), null),
        lambda: L.mmk_icp_status(ctypes.byref(p), fake, 1 << 30, fake, null),
    ]
    for call in calls:
        L.mmk_icp_workspace_bytes(ctypes.byref(icp_params()))         # (a good call in between: the message below is the new one)
        assert call() == -1 and b"trim_steep" in L.mmk_last_error()
    good = icp_params(trim_steep=4.0)
    assert L.mmk_icp_workspace_bytes(ctypes.byref(good)) == L.mmk_icp_workspace_bytes(ctypes.byref(icp_params())) > 0
    assert (L.mmk_icp_backward_points_workspace_bytes(ctypes.byref(good), 1)
            == L.mmk_icp_backward_points_workspace_bytes(ctypes.byref(icp_params()), 1) > 0)


def test_icp_yaml_keys_and_attributes(tmp_path):
    for diff in (True, False):
        icp = ICP("pt2pt", differentiable=diff, max_iterations=3)
        assert icp.trim == "hard" and icp.tanh_steepness == 10.0              # the built-in YAML
        assert icp._params(1, 8, 8, 3, 2, None, 5.0, save_state=diff).trim_steep == 0.0
        icp.trim = "tanh"                                                      # assignable, like nn_search
        assert icp._params(1, 8, 8, 3, 2, None, 5.0, save_state=diff).trim_steep == 10.0
        icp.tanh_steepness = 2.5
        assert icp._params(1, 8, 8, 3, 2, None, 5.0, save_state=diff).trim_steep == 2.5
        icp.trim = "hard"
        assert icp._params(1, 8, 8, 3, 2, None, 5.0, save_state=diff).trim_steep == 0.0
        cfg = icp_yaml(tmp_path, "dICP:\n  target_pad_val: 1000.0\n  parameters:\n    trim: tanh\n    tanh_steepness: 4\n")
        icp = ICP("pt2pl", config_path=cfg, differentiable=diff)
        assert icp.trim == "tanh" and icp.tanh_steepness == 4.0
        assert icp._params(1, 8, 8, 6, 2, None, 5.0, save_state=diff).trim_steep == 4.0
    icp = ICP("pt2pt", config_path=icp_yaml(tmp_path, "dICP:\n  parameters:\n    trim: tanh\n"))
    assert icp.trim == "tanh" and icp.tanh_steepness == 10.0
    for text in ("    trim: soft\n", "    trim: tanh\n    tanh_steepness: 0\n", "    trim: tanh\n    tanh_steepness: -3.0\n",
                 "    tanh_steepness: 0.0\n", "    trim: tanh\n    tanh_steepness: .nan\n"):
        with pytest.raises(ValueError, match="trim|tanh_steepness"):
            ICP("pt2pt", config_path=icp_yaml(tmp_path, "dICP:\n  parameters:\n" + text))
    icp = ICP("pt2pt")
    icp.trim = "sigmoid"
    with pytest.raises(ValueError, match="trim"):
        icp._params(1, 8, 8, 3, 2, None, 5.0, save_state=True)
    icp.trim, icp.tanh_steepness = "tanh", 0.0
    with pytest.raises(ValueError, match="tanh_steepness"):
        icp._params(1, 8, 8, 3, 2, None, 5.0, save_state=True)


def test_policy_parameters_switch_the_training_instance_only():
    from mm_masking_amd.icp_weight_policy import LearnICPWeightPolicy

    params = functools.partial(policy_params, torch.device("cpu"), dropout=0.0, amp_dtype=torch.float32, unet_backend="torch")

    assert "icp_trim" not in params() and "icp_tanh_steepness" not in params()      # default_params stays as it is
    model = LearnICPWeightPolicy(params())
    assert (model.ICP_alg.trim, model.ICP_alg_inference.trim) == ("hard", "hard")
    model = LearnICPWeightPolicy(params(icp_trim="tanh"))
    assert (model.ICP_alg.trim, model.ICP_alg.tanh_steepness) == ("tanh", 10.0)
    assert model.ICP_alg._params(1, 8, 8, 6, 2, None, 5.0, save_state=True).trim_steep == 10.0
    assert model.ICP_alg_inference.trim == "hard"
    assert model.ICP_alg_inference._params(1, 8, 8, 6, 2, None, 5.0, save_state=False).trim_steep == 0.0
    model = LearnICPWeightPolicy(params(icp_trim="tanh", icp_tanh_steepness=3))
    assert model.ICP_alg._params(1, 8, 8, 6, 2, None, 5.0, save_state=True).trim_steep == 3.0
    assert model.ICP_alg_inference._params(1, 8, 8, 6, 2, None, 5.0, save_state=False).trim_steep == 0.0
    model = LearnICPWeightPolicy(params(icp_trim="hard", icp_tanh_steepness=3.0))
    assert model.ICP_alg._params(1, 8, 8, 6, 2, None, 5.0, save_state=True).trim_steep == 0.0
    for over in ({"icp_trim": "soft"}, {"icp_trim": None}, {"icp_trim": "tanh", "icp_tanh_steepness": 0.0},
                 {"icp_tanh_steepness": -1.0}, {"icp_tanh_steepness": float("nan")}, {"icp_tanh_steepness": float("inf")},
                 {"icp_tanh_steepness": "10"}):
        with pytest.raises(ValueError, match="icp_trim|icp_tanh_steepness"):
            LearnICPWeightPolicy(params(**over))
