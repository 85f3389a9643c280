"""CPU: the device-resident, learnable soft-min temperature of the dICP (DESIGN.md §3 I3⁗, I7⁗).  The host plumbing -- the
three C entries in the header and the binding, their argument checks, the older entries' sizes, dICP.ICP's validation of a
tensor ``softmin_temp``, the refused combinations, the policy's ``learn_icp=("softmin_temp",)`` -- and the restatement
tests/dicp_restatement.py: the bits of a number temperature for a tensor of equal values, the closed form of tau-bar
against fp64 autograd, and the awake ratios of the GPU test's cases on the restatement's free run, so that a drifting input
fails here, without a GPU.

Awake ratio of a run: max_b |g_b| / S_b, g_b the pair's tau gradient and S_b the sum of the magnitudes of its per-point
contributions; the threshold 0.03 is tests/test_gpu_icp_hyper.py's.  Free-running neighbours, shapes and soft-min cases of
tests/dicp_cases.py, all five cases, k in {4, 8}: with tau = (0.25, 0.4) the smallest max_b ratio is 0.10 and the
smallest single pair 0.055; with (0.25, 0.25) the smallest max_b ratio is 0.055 (pt2pl, Cauchy, dim 3, k = 8).
"""
import ctypes
import functools
import importlib

import numpy as np
import pytest
import torch

from mm_masking_amd import _lib
from mm_masking_amd.dICP.ICP import ICP

from dicp_cases import B, K, SOFTMIN_CASES as CASES, SOFTMIN_IDS as IDS, SOFTMIN_TRIM as TRIM, reference
from dicp_restatement import knn_ref_batch, soft_backward_closed_form, soft_rows
from support import header, icp_params, n_args, policy_params

icp_mod = importlib.import_module("mm_masking_amd.dICP.ICP")        # (the package re-exports the class under the module's name)
NEW = ("mmk_icp_forward_soft_t", "mmk_icp_backward_soft_t_workspace_bytes", "mmk_icp_backward_soft_t")


@pytest.fixture(scope="module")
def L():
    return _lib.lib()


_params = functools.partial(icp_params, N=300, M=64, icp_type=0, loss=0, tolerance=1e-9, max_iter=3, trim_steep=0.0)


# ----------------------------------------------------------------------------- the C ABI
def test_entries_exist_and_older_sizes_are_unchanged(L):
    hdr = header()
    for name in NEW:
        assert hasattr(L, name) and name in _lib.EXPORTED, name
        assert n_args(hdr, name) == len(_lib.EXPORTED[name][1]), name
    assert n_args(hdr, "mmk_icp_forward_soft_t") == n_args(hdr, "mmk_icp_forward_soft") + 2          # temp, per_pair
    assert n_args(hdr, "mmk_icp_backward_soft_t") == n_args(hdr, "mmk_icp_backward_soft") + 3       # + grad_temp
    assert L.mmk_version() == 502 and ctypes.sizeof(_lib.IcpParams) == L.mmk_icp_params_bytes() == 60
    assert ctypes.sizeof(_lib.IcpSoft) == 8
    for p in (_params(), _params(N=1000, dim=3, icp_type=1, max_iter=5)):
        for k in (4, 8):
            r, s = ctypes.byref(p), ctypes.byref(_lib.IcpSoft(k=k, temp=1.0))
            for wt in (0, 1):
                old = L.mmk_icp_backward_soft_workspace_bytes(r, s, wt)
                assert old > 0 and L.mmk_icp_backward_soft_t_workspace_bytes(r, s, wt, 0) == old
                # with grad_temp: the block partials behind the older parts, (K, B, nblk) fp64
                extra = p.max_iter * p.B * ((p.N + 255) // 256) * 8
                got = L.mmk_icp_backward_soft_t_workspace_bytes(r, s, wt, 1) - old
                assert got > 0 and got % 256 == 0 and extra <= got <= extra + 256, (got, extra)
    p = _params()
    for k, temp in ((1, 1.0), (9, 1.0), (4, 0.0), (4, float("nan"))):          # the struct's own validation still holds
        assert L.mmk_icp_backward_soft_t_workspace_bytes(ctypes.byref(p), ctypes.byref(_lib.IcpSoft(k=k, temp=temp)), 1, 1) == 0
    assert L.mmk_icp_backward_soft_t_workspace_bytes(ctypes.byref(p), None, 1, 1) == 0


def test_argument_errors(L):
    null, fake = ctypes.c_void_p(0), ctypes.c_void_p(4096)       # never dereferenced: every call fails before any launch
    iters = ctypes.c_int(0)
    p, ok = _params(), _lib.IcpSoft(k=4, temp=1.0)
    r, s = ctypes.byref(p), ctypes.byref(ok)
    for per_pair in (2, -1):
        assert L.mmk_icp_forward_soft_t(r, *([fake] * 10), s, fake, per_pair, fake, 1 << 30, ctypes.byref(iters), null) == -1
        assert b"per_pair" in L.mmk_last_error()
        assert L.mmk_icp_backward_soft_t(r, *([fake] * 13), s, fake, per_pair, fake, fake, 1 << 30, null) == -1
        assert b"per_pair" in L.mmk_last_error()
    assert L.mmk_icp_backward_soft_t(r, *([fake] * 13), s, null, 0, fake, fake, 1 << 30, null) == -1
    assert b"grad_temp needs temp" in L.mmk_last_error()
    need = L.mmk_icp_backward_soft_t_workspace_bytes(r, s, 1, 1)
    for have in (64, need - 1, L.mmk_icp_backward_soft_workspace_bytes(r, s, 1)):          # (the last: the size without grad_temp)
        assert L.mmk_icp_backward_soft_t(r, *([fake] * 13), s, fake, 1, fake, fake, have, null) == -1
        assert b"workspace too small" in L.mmk_last_error()
    assert L.mmk_icp_backward_soft_t(r, *([fake] * 13), s, fake, 1, fake, null, 1 << 30, null) == -1     # no workspace at all
    assert L.mmk_icp_backward_soft_t(ctypes.byref(_params(save_state=0)), *([fake] * 13), s, fake, 0, fake, fake, 1 << 30, null) == -1
    assert b"save_state" in L.mmk_last_error()
    for k, temp in ((1, 1.0), (4, -1.0)):
        bad = ctypes.byref(_lib.IcpSoft(k=k, temp=temp))
        assert L.mmk_icp_forward_soft_t(r, *([fake] * 10), bad, fake, 0, fake, 1 << 30, ctypes.byref(iters), null) == -1
        assert b"soft" in L.mmk_last_error()
        assert L.mmk_icp_backward_soft_t(r, *([fake] * 13), bad, fake, 0, fake, fake, 1 << 30, null) == -1


# ----------------------------------------------------------------------------- dICP.ICP
def _soft_icp(temp):
    icp = ICP("pt2pt", differentiable=True)
    icp.correspondence, icp.softmin_temp = "softmin", temp
    return icp


def test_tensor_shape_and_dtype_are_validated_before_the_device_is_touched():
    src, tgt = torch.zeros(2, 6, 3), torch.zeros(2, 9, 3)
    for shape in ((3,), (2, 1), (1, 1), (0,)):
        with pytest.raises(ValueError, match=r"softmin_temp must be a number or a tensor of shape \(\), \(1,\) or \(B,\) = \(2,\)"):
            _soft_icp(torch.full(shape, 0.25)).icp(src, tgt, dim=2)
    for dtype in (torch.int32, torch.int64, torch.bool):
        with pytest.raises(ValueError, match="softmin_temp: a tensor must have a floating-point dtype"):
            _soft_icp(torch.ones((), dtype=dtype)).icp(src, tgt, dim=2)
    for bad in (0.0, -1.0, float("nan"), float("inf"), True, "1"):                 # a number is validated on the host as before
        with pytest.raises(ValueError, match="softmin_temp"):
            _soft_icp(bad).icp(src, tgt, dim=2)
    s = _soft_icp(torch.tensor([0.25, 0.4]))._softmin()
    assert (s.k, s.temp) == (4, 1.0)                            # the struct carries a placeholder that passes its validation
    assert icp_mod._temp_size(torch.tensor(0.25), 2) is False and icp_mod._temp_size(torch.tensor([0.25]), 2) is False
    assert icp_mod._temp_size(torch.tensor([0.25, 0.4], dtype=torch.float64), 2) is True
    assert icp_mod._temp_size(torch.tensor([0.25]), 1) is False                   # B = 1: (1,) is the shared value
    if not torch.cuda.is_available():
        # a tensor's VALUES are not looked at on the host: a good shape goes on and wants its device
        for temp in (torch.tensor(0.25), torch.tensor([-1.0]), torch.tensor([0.25, float("nan")], dtype=torch.float64)):
            with pytest.raises(_lib.MmkError, match="HIP device"):
                _soft_icp(temp).icp(src, tgt, dim=2)
        # a call that is not differentiable keeps nearest correspondences and does not look at the tensor
        with torch.no_grad(), pytest.raises(_lib.MmkError, match="HIP device"):
            _soft_icp(torch.ones(5, 5, dtype=torch.int32)).icp(src, tgt, dim=2)


def test_refused_combinations_are_still_refused_with_a_tensor_temperature():
    src, tgt = torch.zeros(1, 6, 3), torch.zeros(1, 9, 3)
    for temp in (0.25, torch.tensor(0.25), torch.tensor(0.25, requires_grad=True)):
        icp = _soft_icp(temp)
        for kw in ({"trim_dist": torch.tensor(1.0)}, {"loss_fn": {"name": "cauchy", "metric": torch.tensor([0.5])}}):
            with pytest.raises(ValueError, match="tensor hyper-parameter"):
                icp.icp(src, tgt, dim=2, **kw)
        icp.tanh_steepness, icp.trim = torch.tensor(4.0), "tanh"
        with pytest.raises(ValueError, match="tensor hyper-parameter"):
            icp.icp(src, tgt, dim=2)
        icp.tanh_steepness = 4.0
        with pytest.raises(ValueError, match="at least softmin_k"):
            icp.icp(src, torch.zeros(1, 3, 3), dim=2)


def test_status_message_names_the_temperature():
    watch = icp_mod._StatusWatch()

    class Done:
        def synchronize(self):
            pass

        def query(self):
            return True

    watch.pending.append((Done(), torch.tensor([icp_mod.ICP_STATUS_BAD_HYPER], dtype=torch.int32)))
    with pytest.raises(_lib.MmkError, match="softmin_temp.*MMK_ICP_STATUS_BAD_HYPER"):
        watch.check(wait=True)


# ----------------------------------------------------------------------------- the policy
def test_policy_keys():
    from mm_masking_amd.icp_weight_policy import LearnICPWeightPolicy

    params = functools.partial(policy_params, torch.device("cpu"), dropout=0.0, amp_dtype=torch.float32, unet_backend="torch")

    for over in ({"learn_icp": ("softmin_temp",)}, {"learn_icp": "softmin_temp"},
                 {"learn_icp": ("softmin_temp",), "icp_correspondence": "nearest"}):
        with pytest.raises(ValueError, match="'softmin_temp' needs icp_correspondence='softmin'"):
            LearnICPWeightPolicy(params(**over))
    for temp in (0.25, 1.0):
        model = LearnICPWeightPolicy(params(icp_correspondence="softmin", icp_softmin_temp=temp, learn_icp=("softmin_temp",)))
        assert [n for n, _ in model.named_parameters() if n.startswith("icp_")] == ["icp_softmin_temp_p"]
        q = model.icp_softmin_temp_p
        assert q.shape == () and q.dtype == torch.float32 and q.requires_grad and q.item() == np.float32(temp)
        assert model.ICP_alg.softmin_temp == temp               # the instance reads the parameter in train() mode, in icp()
        assert model.ICP_alg_inference.correspondence == "nearest" and model.ICP_alg_inference._softmin() is None
    assert not any(n.startswith("icp_") for n, _ in LearnICPWeightPolicy(params(icp_correspondence="softmin")).named_parameters())
    # soft-min with any of the other three names stays the ValueError it is, also next to the new name
    for learn in (("trim_dist",), ("softmin_temp", "trim_dist"), ("metric", "softmin_temp"), "tanh_steepness"):
        with pytest.raises(ValueError, match="icp_correspondence='softmin' does not combine with learn_icp"):
            LearnICPWeightPolicy(params(icp_correspondence="softmin", icp_trim="tanh", learn_icp=learn))
    with pytest.raises(ValueError, match="unknown name"):
        LearnICPWeightPolicy(params(learn_icp=("softmin_tau",)))


# ----------------------------------------------------------------------------- the restatement
def test_equal_values_give_the_bits_of_the_number_restatement():
    rng = np.random.default_rng(11)
    for dim, with_normals, tau in ((2, False, 0.25), (3, True, 0.3)):
        tgt = torch.from_numpy(rng.uniform(-2, 2, (2, 120, 6)).astype(np.float32))
        p = torch.from_numpy(rng.uniform(-2, 2, (2, 40, dim)).astype(np.float32))
        idx = torch.from_numpy(knn_ref_batch(p.numpy(), tgt.numpy(), 5, dim)[0])
        P = [p[..., c] for c in range(dim)]
        want = soft_rows(tgt, P, idx, tau, dim, with_normals)
        got = soft_rows(tgt, P, idx, torch.full((2, 40), tau, dtype=torch.float32), dim, with_normals)
        for a, b in zip(got, want):
            assert torch.equal(a, b)


@pytest.mark.parametrize("dim,with_normals", [(2, False), (2, True), (3, False), (3, True)])
def test_closed_form_of_tau_bar_against_autograd(dim, with_normals):
    """I7⁗ in numpy (soft_backward_closed_form's tau-bar) against autograd through soft_rows, fp64, with a temperature of its own per
    point: both are exact derivatives of the same expression, so they agree to rounding -- 1e-12 of the largest magnitude."""
    rng = np.random.default_rng(14 + dim)
    N_, M_, k = 30, 200, 5
    tgt = torch.from_numpy(rng.uniform(-2, 2, (1, M_, 6)))
    p = torch.from_numpy(rng.uniform(-2, 2, (1, N_, dim)))
    tau = torch.from_numpy(rng.uniform(0.15, 0.5, (1, N_))).requires_grad_(True)
    idx = torch.from_numpy(knn_ref_batch(p.float().numpy(), tgt.float().numpy(), k, dim)[0])
    virt, a, d = soft_rows(tgt, [p[..., c] for c in range(dim)], idx, tau, dim, with_normals)
    assert ((a > 0.01) & (a < 0.99)).double().mean() > 0.5      # the weights are spread: the soft-min is awake
    vbar = torch.from_numpy(rng.normal(size=(1, N_, 6)))
    (virt * vbar).sum().backward()
    got = soft_backward_closed_form(tgt.numpy()[0], p.numpy()[0], idx.numpy()[0], tau.detach().numpy()[0], dim, with_normals,
                                    vbar.numpy()[0])[2]
    ref = tau.grad.numpy()[0]
    scale = np.abs(ref).max()
    assert scale > 0 and np.abs(got - ref).max() <= 1e-12 * scale, (np.abs(got - ref).max(), scale)
    assert (np.abs(ref) > 1e-3 * scale).mean() > 0.5            # and not a handful of points only


@pytest.mark.parametrize("k", [4, 8])
@pytest.mark.parametrize("ci", range(len(CASES)), ids=IDS)
def test_tau_gradient_of_the_gpu_cases_is_awake_on_the_free_run(ci, k):
    """The cases of tests/test_gpu_softmin_temp.py on the restatement's free run (its own neighbours): for the per-pair
    temperatures (0.25, 0.4) and the equal ones (0.25, 0.25), some pair's |g_b| is at least 0.03 of the sum of the magnitudes
    of its per-point contributions, and no pair froze."""
    for taus in ((0.25, 0.4), (0.25, 0.25)):
        out = reference(CASES[ci], TRIM, soft_k=k, taus=taus)
        assert out["num_iter"] == K and all(bool(a.all()) for a in out["hist"]["active"])
        g, S = out["grads"]["tau"], out["S"]
        ratios = (g.abs() / S).tolist()
        print("AWAKE tau %s k %d: |g_b| / S_b per pair %s" % (taus, k, ["%.3f" % r for r in ratios]))
        assert len(ratios) == B and torch.isfinite(g).all() and max(ratios) >= 0.03, ratios
