"""CPU: the C ABI of the radar front end's gradients (mmk_cfar_mask_bwd, mmk_extract_peaks_bwd) -- declared, exported,
host-side argument and workspace checks (no launch) -- and the golden fixture itself (tests/golden/radar_grads.npz): the
conditions its generator asserts, re-asserted on the stored arrays, and the stored gradients against central finite
differences of an fp64 restatement of the forward along two random directions."""
import ctypes
import os
import re

import numpy as np
import pytest

from mm_masking_amd import _lib
from radar_cases import RES
from support import ROOT, load_golden

NEW = ("mmk_cfar_mask_bwd", "mmk_extract_peaks_bwd", "mmk_extract_peaks_bwd_workspace_bytes")


@pytest.fixture(scope="module")
def L():
    _lib.build()
    return _lib.lib()


@pytest.fixture(scope="module")
def gold(golden_dir):
    return load_golden(golden_dir, "radar_grads.npz")


def test_new_entries_declared_and_exported(L):
    raw_hdr = open(os.path.join(ROOT, "include", "mmk.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", raw_hdr, flags=re.S)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(L, name) and name in _lib.EXPORTED, name
    assert L.mmk_version() == int(re.search(r"#define\s+MMK_VERSION\s+(\d+)", raw_hdr).group(1))


def test_cfar_bwd_argument_checks(L):
    null, fake = ctypes.c_void_p(0), ctypes.c_void_p(4096)     # never dereferenced: every call fails on the host before a launch

    def call(raw=fake, g=fake, out=fake, B=1, A=2, R=1400, w2=50, guard=5, mincol=89, maxcol=1287):
        return L.mmk_cfar_mask_bwd(raw, g, B, A, R, w2, guard, mincol, maxcol, 1.0, 0.09, 10.0, out, null)

    for kw in ({"raw": null}, {"g": null}, {"out": null}):
        assert call(**kw) == -1 and b"NULL" in L.mmk_last_error()
    assert call(B=0) == -1 and b"3D" in L.mmk_last_error()
    assert call(w2=0) == -1 and b"window" in L.mmk_last_error()
    assert call(mincol=54) == -1 and b"column range" in L.mmk_last_error()
    assert call(maxcol=1401) == -1 and b"column range" in L.mmk_last_error()
    assert call(R=14000, maxcol=1287) == -1 and b"LDS" in L.mmk_last_error()


def test_extract_peaks_bwd_workspace_and_argument_checks(L):
    null, fake = ctypes.c_void_p(0), ctypes.c_void_p(4096)
    B, A, R, P = 2, 12, 400, 26
    fwd = L.mmk_extract_peaks_workspace_bytes(B, A, R, P)
    need = L.mmk_extract_peaks_bwd_workspace_bytes(B, A, R, P)
    assert need >= fwd + B * 2 * P * 4                          # the forward's arrays + one gradient per marker slot
    assert L.mmk_extract_peaks_bwd_workspace_bytes(0, A, R, P) == 0 and L.mmk_extract_peaks_bwd_workspace_bytes(B, A, R, 0) == 0

    def call(mask=fake, az=fake, gpc=fake, gm=fake, ws=fake, nbytes=need, R=R, P=P):
        return L.mmk_extract_peaks_bwd(mask, B, A, R, RES, az, null, 1, 10.0, P, gpc, gm, ws, nbytes, null)

    for kw in ({"mask": null}, {"az": null}, {"gpc": null}, {"gm": null}):
        assert call(**kw) == -1 and b"NULL" in L.mmk_last_error()
    assert call(R=1) == -1 and b"shape" in L.mmk_last_error()
    assert call(P=0) == -1 and b"shape" in L.mmk_last_error()
    assert call(nbytes=need - 1) == -3 and b"workspace" in L.mmk_last_error()
    assert call(ws=null) == -3 and b"workspace" in L.mmk_last_error()
    assert call(R=20000, nbytes=1 << 30) == -1 and b"LDS" in L.mmk_last_error()


# ----------------------------------------------------------------------------- the fixture
def _cfar_kw(gold, tag):
    if tag == 0:
        return dict(width=101, guard=5, steep=10.0, a_th=1.0, b_th=0.09)
    w, g, s, a, b = gold["ca_params1"]
    return dict(width=int(w), guard=int(g), steep=float(s), a_th=float(a), b_th=float(b))


def _cfar_f64(x, width, guard, steep, a_th, b_th, minr=2.0, maxr=80.0):
    """fp64 restatement of cfar_mask(diff=True): m_raw, the mask, and the two window sums (NaN outside the column range)."""
    R = x.shape[-1]
    w2 = width // 2
    mincol = max(0, int(minr / RES + w2 + guard + 1))
    maxcol = min(R, int(maxr / RES - w2 - guard))
    cs = np.concatenate([np.zeros(x.shape[:-1] + (1,)), np.cumsum(x, axis=-1)], axis=-1)
    c = np.arange(mincol, maxcol)
    left, right = np.full(x.shape, np.nan), np.full(x.shape, np.nan)
    left[..., c] = cs[..., c - guard] - cs[..., c - w2 - guard]
    right[..., c] = cs[..., np.minimum(R, c + w2 + guard + 1)] - cs[..., np.minimum(R, c + guard + 1)]
    th = np.full(x.shape, 1000.0)
    th[..., c] = a_th * np.maximum(left[..., c], right[..., c]) / w2 + b_th
    m_raw = 0.5 * np.tanh(steep * (x - th) + 2.5) + 0.5
    return m_raw, np.where(np.abs(m_raw) > 0.99, m_raw, 0.0), left, right


@pytest.mark.parametrize("name,tags", [("ca_raw", (0, 1)), ("ch_raw", (0,))])
def test_fixture_conditions_cfar(gold, name, tags):
    raw = gold[name].astype(np.float64)
    for tag in tags:
        kw = _cfar_kw(gold, tag)
        m_raw, mask, left, right = _cfar_f64(raw, **kw)
        assert (np.abs(m_raw - 0.99) > 1e-4).all()              # no gate within a tanh ulp of flipping
        kept = mask != 0
        assert kept.any()
        l32, r32 = left.astype(np.float32).astype(np.float64), right.astype(np.float32).astype(np.float64)
        with np.errstate(invalid="ignore"):
            d = np.abs(l32 - r32)
            assert not (kept & (d > 0) & (d < 1e-4)).any()      # a winner never hangs on the last bit of a window sum
        if name == "ca_raw":
            assert (kept[2] & (l32[2] == r32[2])).any()         # exact ties on kept cells of the empty field
        if name == "ch_raw":
            assert (10.0 * RES * np.nonzero(kept)[2] * 0.99 > 10).all()


def test_fixture_conditions_peaks(gold):
    mask = gold["pk_mask"]
    assert (10.0 * RES * np.nonzero(mask)[2] * 0.99 > 10).all()
    assert (gold["pk_nmark"] % 2 == 0).all() and (gold["pk_nmark"] == 2 * gold["pk_n10"]).all()
    rows = [np.nonzero(_markers(mask[b], True)[0].reshape(mask.shape[1], -1))[0] for b in range(2)]
    assert (rows[0][0::2] != rows[0][1::2]).any()               # pairs that straddle two azimuth rows
    assert (mask[:, 5] == 0).all()


def _directional(f, x, d, eps):
    return (f(x + eps * d) - f(x - eps * d)) / (2 * eps)


@pytest.mark.parametrize("tag", [0, 1])
def test_cfar_golden_gradient_against_finite_differences(gold, tag):
    """<grad, d> against the central difference of sum(G * mask) along d.  At an exact tie the central difference of
    max(l, r) is the mean of the two slopes: torch.maximum's half-and-half."""
    kw = _cfar_kw(gold, tag)
    x, G, grad = gold["ca_raw"].astype(np.float64), gold["ca_G"].astype(np.float64), gold["ca_grad%d" % tag].astype(np.float64)
    keep = _cfar_f64(x, **kw)[1] != 0                           # the gate is the forward's decision: a constant
    f = lambda y: (G * np.where(keep, _cfar_f64(y, **kw)[0], 0.0)).sum()
    rng = np.random.default_rng(5 + tag)
    for _ in range(2):
        d = rng.normal(size=x.shape)
        fd, an = _directional(f, x, d, 1e-7), (grad * d).sum()
        assert abs(fd - an) <= 2e-5 * np.abs(grad * d).sum(), (fd, an)


def _markers(mask, diff, steep=10.0, z_hard=None):
    """Marker values per flattened cell and a = res j m, in the dtype of ``mask``.  ``z_hard``: the (a == 0) factor of
    diff=False taken from another (the unperturbed) mask: the reference multiplies by a bool tensor, a constant."""
    a = (mask.dtype.type(RES) * np.arange(mask.shape[-1], dtype=mask.dtype)) * mask
    if diff:
        z = 1 - np.tanh(mask.dtype.type(steep) * a)
    else:
        z = (a == 0).astype(mask.dtype) if z_hard is None else z_hard
    v = np.zeros_like(a)
    v[..., :-1] = a[..., :-1] * z[..., 1:] + a[..., 1:] * z[..., :-1]
    return v.reshape(-1), a


@pytest.mark.parametrize("diff,use_T", [(True, False), (True, True), (False, False), (False, True)])
def test_peaks_golden_gradient_against_finite_differences(gold, diff, use_T):
    """The marker set, its order and its pairing are the unperturbed forward's (constants, as under autograd); the marker
    VALUES move with the mask."""
    tag = "%d%d" % (int(diff), int(use_T))
    mask, az, T_ab = gold["pk_mask"].astype(np.float64), gold["pk_az"].astype(np.float64), gold["pk_T_ab"].astype(np.float64)
    G, grad, n = gold["pk_G" + tag].astype(np.float64), gold["pk_grad" + tag].astype(np.float64), gold["pk_n" + tag]
    B, A, R = mask.shape
    # the marker set as the reference finds it: in fp32, where tanh(steep a) saturates to 1 inside a blob
    where = [np.flatnonzero(_markers(gold["pk_mask"][b], diff)[0]) for b in range(B)]
    z_hard = [(_markers(mask[b], False)[1] == 0).astype(np.float64) for b in range(B)]

    def cloud(m, b):
        v = _markers(m[b], diff, z_hard=z_hard[b])[0][where[b]]
        phi_m = np.repeat(az[b], R)[where[b]]
        rho, phi = (v[1::2] + v[0::2]) / 2, (phi_m[1::2] + phi_m[0::2]) / 2
        p = np.stack([rho * np.cos(phi), rho * np.sin(phi), np.zeros_like(rho)], 1)
        return p @ T_ab[b, :3, :3].T + T_ab[b, :3, 3] if use_T else p

    for b in range(B):
        assert len(where[b]) == 2 * n[b]
        np.testing.assert_allclose(cloud(mask, b), gold["pk_pc" + tag][b, :n[b]], atol=2e-5)
    f = lambda m: sum((cloud(m, b) * G[b, :n[b]]).sum() for b in range(B))
    rng = np.random.default_rng(9)
    for _ in range(2):
        d = rng.normal(size=mask.shape)
        fd, an = _directional(f, mask, d, 1e-7), (grad * d).sum()
        assert abs(fd - an) <= 2e-5 * np.abs(grad * d).sum(), (fd, an)


def test_chain_golden_gradient_against_finite_differences(gold):
    """scan -> CFAR -> peaks -> zero padding -> extract_weights -> dICP -> sum(T * G), restated in fp64 with the constants of
    the fp32 forward (gates, marker set and pairing, correspondences), against the stored fp32 gradient.  The bound is the
    dICP backward's own ceiling for fp32 against fp64 arithmetic (2e-3, tests/test_gpu_point_grads.py), taken of
    sum |grad_i d_i|."""
    import torch
    import torch.nn.functional as F
    from oracle import dicp_ref
    x0, az, G = gold["ch_raw"].astype(np.float64), gold["ch_az"].astype(np.float64), torch.from_numpy(gold["ch_G"]).double()
    B, A, R = x0.shape
    npad, K, n = int(gold["ch_npad"]), int(gold["ch_iters"]), gold["ch_n"]
    kw = _cfar_kw(gold, 0)
    keep = _cfar_f64(x0, **kw)[1] != 0
    mask32 = np.where(keep, _cfar_f64(x0, **kw)[0], 0.0).astype(np.float32)
    where = [np.flatnonzero(_markers(mask32[b], True)[0]) for b in range(B)]
    assert [len(w) for w in where] == (2 * n).tolist()
    wmask = torch.from_numpy(gold["ch_mu"].astype(np.float64)[:, :, None] * gold["ch_mv"].astype(np.float64)[:, None, :])
    tgt = torch.from_numpy(gold["ch_map"])
    loss_fn = {"name": "huber", "metric": 1.0}
    ref = dicp_ref.ICPRef("pt2pl", differentiable=False, max_iterations=K, tolerance=1e-9)
    fixed = ref.icp(torch.from_numpy(gold["ch_cloud"]), tgt, weight=torch.from_numpy(gold["ch_w"]), trim_dist=5.0, loss_fn=loss_fn,
                    dim=2)["hist"]["idx"]

    def f(x):
        m = np.where(keep, _cfar_f64(x, **kw)[0], 0.0)
        cloud = np.zeros((B, npad, 3))
        for b in range(B):
            v = _markers(m[b], True)[0][where[b]]
            phi_m = np.repeat(az[b], R)[where[b]]
            rho, phi = (v[1::2] + v[0::2]) / 2, (phi_m[1::2] + phi_m[0::2]) / 2
            cloud[b, :n[b], 0], cloud[b, :n[b], 1] = rho * np.cos(phi), rho * np.sin(phi)
        c = torch.from_numpy(cloud)
        grid = torch.stack((c[:, :, 1] / 0.2384, -c[:, :, 0] / 0.2384), dim=2) / 639 * 2      # point_to_cart_idx(min_to_plus_1)
        grid[(c[:, :, 0] == 0) & (c[:, :, 1] == 0)] = -100.0
        w = F.grid_sample(wmask[:, None], grid[:, :, None], mode="bilinear", padding_mode="zeros", align_corners=True)[:, 0, :, 0]
        T = ref.icp(c, tgt.double(), T_init=torch.eye(4, dtype=torch.float64).repeat(B, 1, 1), weight=w, trim_dist=5.0,
                    loss_fn=loss_fn, dim=2, dtype=torch.float64, fixed_idx=fixed)["T"]
        return (T * G).sum().item(), T

    np.testing.assert_allclose(f(x0)[1].numpy(), gold["ch_T"], atol=2e-6)
    grad = gold["ch_grad"].astype(np.float64)
    rng = np.random.default_rng(13)
    for _ in range(2):
        d = rng.normal(size=x0.shape)
        fd, an = (f(x0 + 1e-6 * d)[0] - f(x0 - 1e-6 * d)[0]) / 2e-6, (grad * d).sum()
        print("chain fd %.6e analytic %.6e scale %.3e" % (fd, an, np.abs(grad * d).sum()))
        assert abs(fd - an) <= 2e-3 * np.abs(grad * d).sum(), (fd, an)
