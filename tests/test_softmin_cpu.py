"""CPU: soft correspondences of the dICP (DESIGN.md §3 I2', I3''', I7''').  The host plumbing of the option -- the new C
entries in the header and the binding, the pinned version and struct size, the argument checks, dICP.ICP's YAML keys and
attributes, the policy's keys, the refused combinations -- and the restatement tests/dicp_restatement.py: its k-NN, the
nearest limit of its soft loop against its nearest loop bit for bit, the closed forms of I7''' against its autograd, and fp64
finite differences of source, target, weight and T_init."""
import ctypes
import functools
import re

import numpy as np
import pytest
import torch

from mm_masking_amd import _lib, synthetic
from mm_masking_amd.dICP.ICP import ICP

from dicp_restatement import ICPRestatement, knn_ref, knn_ref_batch, soft_backward_closed_form, soft_rows
from knn_normals_ref import nn_dist_f32
from support import header, icp_params, n_args, policy_params

NEW = ("mmk_icp_soft_workspace_bytes", "mmk_icp_forward_soft", "mmk_icp_backward_soft_workspace_bytes", "mmk_icp_backward_soft",
       "mmk_knn_search_workspace_bytes", "mmk_knn_search")


@pytest.fixture(scope="module")
def L():
    return _lib.lib()


_params = functools.partial(icp_params, B=1, N=8, M=16, icp_type=0, loss=0, tolerance=1e-9, max_iter=2, trim_steep=0.0)


# ----------------------------------------------------------------------------- the C ABI
def test_header_and_binding_carry_the_new_entries(L):
    hdr = header()
    for name in NEW:
        arity = n_args(hdr, name)
        assert name in _lib.EXPORTED, name
        assert arity == len(_lib.EXPORTED[name][1]), (name, arity, len(_lib.EXPORTED[name][1]))
        assert hasattr(L, name)
    m = re.search(r"typedef struct \{\s*int32_t k;\s*float temp;\s*\} mmk_icp_soft;", hdr)
    assert m and ctypes.sizeof(_lib.IcpSoft) == 8 and [f[0] for f in _lib.IcpSoft._fields_] == ["k", "temp"]


def test_version_and_struct_size_are_pinned(L):
    assert L.mmk_version() == 502
    assert ctypes.sizeof(_lib.IcpParams) == L.mmk_icp_params_bytes() == 60


BAD_SOFT = [(1, 0.25), (0, 0.25), (-3, 0.25), (9, 0.25), (4, 0.0), (4, -0.25), (4, float("nan")), (4, float("inf")), (4, -float("inf"))]


def test_argument_checks(L):
    p = _params()
    ok = _lib.IcpSoft(k=4, temp=0.25)
    plain = L.mmk_icp_workspace_bytes(ctypes.byref(p))
    fwd = L.mmk_icp_soft_workspace_bytes(ctypes.byref(p), ctypes.byref(ok))
    assert plain > 0 and fwd > plain and fwd % 256 == 0
    # nn_method is ignored: the search always goes through the grid
    assert fwd == L.mmk_icp_soft_workspace_bytes(ctypes.byref(_params(nn_method=1)), ctypes.byref(ok))
    b0 = L.mmk_icp_backward_soft_workspace_bytes(ctypes.byref(p), ctypes.byref(ok), 0)
    b1 = L.mmk_icp_backward_soft_workspace_bytes(ctypes.byref(p), ctypes.byref(ok), 1)
    assert b0 == fwd and b1 > b0 and b1 % 256 == 0
    # k rows per point in the target part: it grows with k
    b1_8 = L.mmk_icp_backward_soft_workspace_bytes(ctypes.byref(p), ctypes.byref(_lib.IcpSoft(k=8, temp=0.25)), 1)
    assert b1_8 > b1
    null = ctypes.c_void_p(0)
    for k, temp in BAD_SOFT + [(8, 0.25)]:                     # the last: M = 7 < k = 8
        q = _params(M=7) if (k, temp) == (8, 0.25) else p
        s = _lib.IcpSoft(k=k, temp=temp)
        assert L.mmk_icp_soft_workspace_bytes(ctypes.byref(q), ctypes.byref(s)) == 0, (k, temp)
        assert L.mmk_icp_backward_soft_workspace_bytes(ctypes.byref(q), ctypes.byref(s), 1) == 0, (k, temp)
        rc = L.mmk_icp_forward_soft(ctypes.byref(q), *([null] * 10), ctypes.byref(s), null, 0, None, null)
        assert rc == -1, (k, temp, rc)                         # MMK_ERR_ARG, before any pointer is looked at
        assert b"soft" in L.mmk_last_error()
        rc = L.mmk_icp_backward_soft(ctypes.byref(q), *([null] * 13), ctypes.byref(s), null, 0, null)
        assert rc == -1, (k, temp, rc)
    assert L.mmk_icp_soft_workspace_bytes(ctypes.byref(_params(M=8)), ctypes.byref(_lib.IcpSoft(k=8, temp=0.25))) > 0     # M == k
    assert L.mmk_icp_soft_workspace_bytes(ctypes.byref(p), None) == 0
    # the stand-alone search
    assert L.mmk_knn_search_workspace_bytes(2, 10, 16, 4) > 0 and L.mmk_knn_search_workspace_bytes(2, 10, 4, 4) > 0
    for B, N, M, k in ((2, 10, 16, 1), (2, 10, 16, 9), (2, 10, 3, 4), (0, 10, 16, 4), (2, 0, 16, 4)):
        assert L.mmk_knn_search_workspace_bytes(B, N, M, k) == 0, (B, N, M, k)
    one = ctypes.c_void_p(8)                                   # never dereferenced: the argument checks come first
    assert L.mmk_knn_search(one, one, one, 2, 10, 3, 3, 2, 4, one, one, one, 1 << 20, null) == -1
    assert L.mmk_knn_search(one, one, one, 2, 10, 16, 3, 2, 9, one, one, one, 1 << 20, null) == -1
    assert L.mmk_knn_search(one, one, one, 2, 10, 16, 3, 2, 4, one, one, null, 0, null) == -3          # MMK_ERR_WORKSPACE


# ----------------------------------------------------------------------------- dICP.ICP and the policy
def test_yaml_keys_and_attributes(tmp_path):
    icp = ICP("pt2pt")
    assert (icp.correspondence, icp.softmin_k, icp.softmin_temp) == ("nearest", 4, 0.25) and icp._softmin() is None
    cfg = tmp_path / "dICP_config.yaml"
    cfg.write_text("dICP:\n  target_pad_val: 1000.0\n  parameters:\n    correspondence: softmin\n    softmin_k: 8\n    softmin_temp: 1.0\n")
    icp = ICP("pt2pl", config_path=str(cfg))
    assert (icp.correspondence, icp.softmin_k, icp.softmin_temp) == ("softmin", 8, 1.0)
    s = icp._softmin()
    assert (s.k, s.temp) == (8, 1.0)
    cfg.write_text("dICP:\n  parameters:\n    nn_search: grid\n")
    assert ICP("pt2pt", config_path=str(cfg)).correspondence == "nearest"           # keys absent: the call it always was
    for body in ("correspondence: soft", "correspondence: softmin\n    softmin_k: 1", "softmin_k: 9", "softmin_k: 4.0",
                 "softmin_temp: 0.0", "softmin_temp: -1.0", "softmin_temp: .nan", "softmin_temp: .inf"):
        cfg.write_text("dICP:\n  parameters:\n    %s\n" % body)
        with pytest.raises(ValueError, match="correspondence|softmin_k|softmin_temp"):
            ICP("pt2pt", config_path=str(cfg))
    icp = ICP("pt2pt")
    icp.correspondence, icp.softmin_k = "softmin", 12                               # attributes are validated at every use
    with pytest.raises(ValueError, match="softmin_k"):
        icp.icp(torch.zeros(1, 4, 3), torch.zeros(1, 20, 3), dim=2)


def test_refused_combinations_raise_before_the_device_is_touched():
    icp = ICP("pt2pt", differentiable=True)
    icp.correspondence = "softmin"
    src, tgt = torch.zeros(1, 6, 3), torch.zeros(1, 9, 3)
    for kw in ({"trim_dist": torch.tensor(1.0)}, {"loss_fn": {"name": "cauchy", "metric": torch.tensor([0.5])}}):
        with pytest.raises(ValueError, match="tensor hyper-parameter"):
            icp.icp(src, tgt, dim=2, **kw)
    icp.tanh_steepness, icp.trim = torch.tensor(4.0), "tanh"
    with pytest.raises(ValueError, match="tensor hyper-parameter"):
        icp.icp(src, tgt, dim=2)
    icp.tanh_steepness = 4.0
    with pytest.raises(ValueError, match="at least softmin_k"):                     # M >= k
        icp.icp(src, torch.zeros(1, 3, 3), dim=2)
    if not torch.cuda.is_available():
        # a call the mode does not apply to goes the old way, which wants its device -- not a ValueError of this option
        with torch.no_grad(), pytest.raises(_lib.MmkError, match="HIP device"):
            icp.icp(src, tgt, dim=2, trim_dist=torch.tensor(1.0))
        with pytest.raises(_lib.MmkError, match="HIP device"):
            icp.icp(src, tgt, dim=2)                                                # trim: tanh with softmin is supported


def test_policy_keys():
    from mm_masking_amd.icp_weight_policy import LearnICPWeightPolicy

    params = functools.partial(policy_params, torch.device("cpu"), dropout=0.0, amp_dtype=torch.float32, unet_backend="torch")

    assert not any(k in params() for k in ("icp_correspondence", "icp_softmin_k", "icp_softmin_temp"))
    model = LearnICPWeightPolicy(params())
    assert (model.ICP_alg.correspondence, model.ICP_alg_inference.correspondence) == ("nearest", "nearest")
    model = LearnICPWeightPolicy(params(icp_correspondence="softmin"))
    assert (model.ICP_alg.correspondence, model.ICP_alg.softmin_k, model.ICP_alg.softmin_temp) == ("softmin", 4, 0.25)
    assert model.ICP_alg_inference.correspondence == "nearest" and model.ICP_alg_inference._softmin() is None
    model = LearnICPWeightPolicy(params(icp_correspondence="softmin", icp_softmin_k=8, icp_softmin_temp=1.0, mask_target="scan",
                                        icp_trim="tanh"))
    s = model.ICP_alg._softmin()
    assert (s.k, s.temp, model.ICP_alg.trim) == (8, 1.0, "tanh") and model.ICP_alg_inference.correspondence == "nearest"
    for over in ({"icp_correspondence": "soft"}, {"icp_correspondence": None}, {"icp_softmin_k": 1}, {"icp_softmin_k": 9},
                 {"icp_softmin_k": 4.0}, {"icp_softmin_temp": 0.0}, {"icp_softmin_temp": float("nan")}, {"icp_softmin_temp": "1"},
                 {"icp_correspondence": "softmin", "icp_trim": "tanh", "learn_icp": ("trim_dist",)}):
        with pytest.raises(ValueError, match="icp_correspondence|softmin_k|softmin_temp"):
            LearnICPWeightPolicy(params(**over))


# ----------------------------------------------------------------------------- the restatement
def _clouds(dim, n=60, m=150, pad_n=6, pad_m=8, B=2, noise=0.05):
    S, Tg = [], []
    for b in range(B):
        s, t, _ = synthetic.simple_cloud_pair(50 + dim + b, n, m, dim=dim, noise=noise, pad_n=pad_n, pad_m=pad_m, yaw=0.02 + 0.01 * b,
                                              trans=(0.4, -0.3 + 0.1 * b, 0.1))
        S.append(s), Tg.append(t)
    src, tgt = np.stack(S), np.stack(Tg)
    w = np.random.default_rng(2).uniform(0.2, 1.0, src.shape[:2]).astype(np.float32)
    w[:, n:] = 0.0
    return torch.from_numpy(src), torch.from_numpy(tgt), torch.from_numpy(w)


def test_knn_ref_is_sorted_exact_and_breaks_ties_to_the_lowest_index():
    rng = np.random.default_rng(0)
    tgt = rng.uniform(-5, 5, (40, 3)).astype(np.float32)
    tgt[17] = tgt[3]                                            # duplicated rows: a tie
    tgt[29] = tgt[3]
    q = np.concatenate([tgt[3:4] + np.float32(0.01), rng.uniform(-5, 5, (6, 3)).astype(np.float32)])
    for dim in (2, 3):
        idx, d2 = knn_ref(q, tgt, 5, dim)
        assert list(idx[0, :3]) == [3, 17, 29] and d2[0, 0] == d2[0, 1] == d2[0, 2]
        for i in range(len(q)):
            d = nn_dist_f32(tgt, q[i], dim)
            assert (np.diff(d2[i]) >= 0).all() and np.array_equal(d2[i], d[idx[i]])
            assert d2[i, -1] <= np.delete(d, idx[i]).min()
    src, t2, _ = _clouds(2)
    i1, _ = knn_ref_batch(src[..., :2].numpy(), t2[..., :2].numpy(), 4, 2)
    from oracle import _clib
    i0, _ = _clib.nn_search(src[..., :2].contiguous().numpy(), np.ascontiguousarray(t2[..., :2].numpy()))
    assert np.array_equal(i1[..., 0], i0)                       # slot 0 is the correspondent the hard searches return


@pytest.mark.parametrize("icp_type,dim,loss", [("pt2pt", 2, ("cauchy", 0.5)), ("pt2pl", 3, ("huber", 0.1)), ("pt2pl", 2, None)])
def test_nearest_limit_of_the_restatement_is_the_hard_restatement_bit_for_bit(icp_type, dim, loss):
    """tau so small that (d_1 - d_0) / tau >= 120 on every real row of every iteration (asserted): every e_j beyond slot 0
    underflows to exactly 0, the virtual row is the correspondent, and the pose is the nearest loop's bit for bit.  (The zero
    source rows share one point and may tie; they carry weight 0.)"""
    src, tgt, w = _clouds(dim)
    n_real = 60
    T0 = torch.eye(4).repeat(2, 1, 1)
    T0[:, 0, 3] += 0.1
    K, tau = 3, 1e-9
    ref = ICPRestatement(icp_type, differentiable=False, max_iterations=K, tolerance=1e-9)
    kw = dict(T_init=T0, weight=w, trim_dist=1.0, loss_name=loss and loss[0], k=loss[1] if loss else 1.0, dim=dim)
    a = ref.icp_soft(src, tgt, tau, softmin_k=4, **kw)
    b = ref.icp(src, tgt, **kw)
    assert a["num_iter"] == b["num_iter"] == K
    for it in range(K):
        d = a["hist"]["d"][it][:, :n_real].double()
        assert ((d[..., 1] - d[..., 0]) / tau >= 120).all()
        assert (a["hist"]["a"][it][:, :n_real, 0] == 1).all() and (a["hist"]["a"][it][:, :n_real, 1:] == 0).all()
        assert torch.equal(a["hist"]["idx"][it][..., 0], b["hist"]["idx"][it].long())
        assert torch.equal(a["hist"]["T"][it + 1], b["hist"]["T"][it + 1])
    assert torch.equal(a["T"], b["T"])
    # and away from the limit the mode is not a no-op
    c = ref.icp_soft(src, tgt, 0.25, softmin_k=4, **kw)
    assert not torch.equal(c["T"], b["T"])
    assert (c["hist"]["a"][0][:, :n_real, 0] < 0.9).any()          # some points do share their weight among neighbours


@pytest.mark.parametrize("dim,with_normals", [(2, False), (2, True), (3, False), (3, True)])
def test_closed_forms_of_the_backward_against_autograd(dim, with_normals):
    """I7''' in numpy (tests/dicp_restatement.py::soft_backward_closed_form) against autograd through soft_rows, fp64: both
    are exact derivatives of the same expression, so they agree to rounding -- 1e-12 of the largest magnitude."""
    rng = np.random.default_rng(4 + dim)
    N, M, k, tau = 30, 200, 5, 0.25                              # N k < M: some target is nobody's neighbour
    tgt = torch.from_numpy(rng.uniform(-2, 2, (1, M, 6))).requires_grad_(True)
    p = torch.from_numpy(rng.uniform(-2, 2, (1, N, dim))).requires_grad_(True)
    idx = torch.from_numpy(knn_ref_batch(p.detach().float().numpy(), tgt.detach().float().numpy(), k, dim)[0])
    virt, a, _ = soft_rows(tgt, [p[..., c] for c in range(dim)], idx, tau, dim, with_normals)
    assert ((a > 0.01) & (a < 0.99)).double().mean() > 0.5      # the weights are spread: the softmin is awake
    vbar = torch.from_numpy(rng.normal(size=(1, N, 6)))
    (virt * vbar).sum().backward()
    gt, pbar, _ = soft_backward_closed_form(tgt.detach().numpy()[0], p.detach().numpy()[0], idx.numpy()[0], tau, dim, with_normals,
                                            vbar.numpy()[0])
    for name, got, ref in (("target", gt, tgt.grad.numpy()[0]), ("p", pbar, p.grad.numpy()[0])):
        scale = np.abs(ref).max()
        assert scale > 0 and np.abs(got - ref).max() <= 1e-12 * scale, (name, np.abs(got - ref).max(), scale)
    used = np.zeros(M, bool)
    used[idx.numpy().ravel()] = True
    assert (~used).any() and (gt[~used] == 0).all() and (gt[:, dim:3] == 0).all()
    if not with_normals:
        assert (gt[:, 3:] == 0).all()


@pytest.mark.parametrize("icp_type,dim,loss,steep,tau", [("pt2pt", 2, ("cauchy", 0.5), 0.0, 0.25), ("pt2pl", 3, ("huber", 0.1), 4.0, 2.0)])
def test_fp64_finite_differences(icp_type, dim, loss, steep, tau):
    """Autograd of the fp64 restatement (neighbours replayed) against central differences along random directions of source,
    target (xyz and normals), weight and T_init.  h = 1e-6: truncation ~ h^2 |f'''| ~ 1e-12, rounding ~ 2^-52 |L| / h ~ 1e-9,
    against directional derivatives of 1e-2 .. 1: asserted at 1e-5 of the analytic value (+ 1e-8).  (The 90 targets of the dim 3
    cloud lie about a metre apart: tau = 2 m^2 there, so that the weights are shared as they are at 0.25 in dim 2.)"""
    src, tgt, w = _clouds(dim, n=40, m=90, pad_n=0, pad_m=0, B=1, noise=0.08)
    K, k, trim = 2, 4, 5.0                           # the hard gate (steep 0) keeps every point: no FD across it
    T0 = torch.eye(4, dtype=torch.float64).repeat(1, 1, 1)
    T0[:, 0, 3] += 0.1
    hyper = dict(softmin_k=k, trim_dist=trim, trim_steep=steep, loss_name=loss[0], k=loss[1], dim=dim)
    G = torch.from_numpy(np.random.default_rng(3).normal(size=(1, 4, 4)))
    free = ICPRestatement(icp_type, differentiable=False, max_iterations=K, tolerance=1e-12, soft=steep > 0).icp_soft(
        src, tgt, tau, T_init=T0, weight=w, **hyper)
    fixed = [i.clone() for i in free["hist"]["idx"]]
    assert (free["hist"]["a"][0][..., 0] < 0.9).double().mean() >= 0.3
    ref = ICPRestatement(icp_type, differentiable=True, max_iterations=K, tolerance=1e-12, soft=steep > 0)

    def L(x):
        out = ref.icp_soft(x[0], x[1], tau, T_init=x[3], weight=x[2], dtype=torch.float64, fixed_idx=fixed, **hyper)
        return (out["T"] * G).sum()

    x0 = [src.double(), tgt.double(), w.double(), T0]
    leaves = [v.clone().requires_grad_(True) for v in x0]
    L(leaves).backward()
    rng = np.random.default_rng(9)
    h = 1e-6
    for n, name in enumerate(("source", "target", "weight", "T_init")):
        g = leaves[n].grad
        assert g is not None and g.abs().max() > 0, name
        for _ in range(3):
            v = torch.from_numpy(rng.normal(size=tuple(x0[n].shape)))
            if name == "source" and dim == 2:
                v[..., 2] = 0
            if name == "target":
                v[..., dim:3] = 0
                v[..., 3 + (dim if icp_type == "pt2pl" else 0):] = 0
            if name == "T_init":
                v[:, 3, :] = 0
                if dim == 2:
                    v[:, 2, :] = 0
                    v[:, :, 2] = 0
            with torch.no_grad():
                xp = [t.clone() for t in x0]
                xm = [t.clone() for t in x0]
                xp[n] += h * v
                xm[n] -= h * v
                fd = (L(xp) - L(xm)).item() / (2 * h)
            an = (g * v).sum().item()
            assert abs(fd - an) <= 1e-5 * abs(an) + 1e-8, (name, fd, an)
    # structural zeros of the reference itself
    if dim == 2:
        assert (leaves[0].grad[..., 2] == 0).all()
    assert (leaves[1].grad[..., dim:3] == 0).all()
