"""CPU: the C ABI of the two resamplers' adjoints (mmk_polar_to_cart_bwd, mmk_cart_to_polar_bwd and their *_ws_bytes) --
declared, exported, host-side argument and workspace checks (no launch) -- and the golden fixture itself
(tests/golden/resample_grads.npz): both operators are linear in the image, so a stored (G, grad) pair must satisfy
<G, F(X)> = <grad, X> for ANY image X, with F the numpy restatement of the forward (oracle/radar_ref.py).

Tolerance of the identity: F is evaluated in the operator's own precision (fp32 / fp64) and the stored gradient is the
reference's sum in that precision, so the two sides differ by rounding only.  Relative to sum |G| F(|X|), measured here over
all cases and both random images (the three sums exactly rounded, math.fsum):  polar -> Cartesian (fp32) worst 2.2e-8,
Cartesian -> polar (fp64) worst 4.9e-18;  bounds 4 x: 8.8e-8 and 2.0e-17.
"""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from mm_masking_amd import _lib
from oracle import radar_ref
from support import ROOT, load_golden

NEW = ("mmk_polar_to_cart_bwd", "mmk_polar_to_cart_bwd_ws_bytes", "mmk_cart_to_polar_bwd", "mmk_cart_to_polar_bwd_ws_bytes")
PC_VARIANTS = ({}, {"fix_wobble": False}, {"interpolate_crossover": False})
PC_ADJOINT_REL = 8.8e-8
CP_ADJOINT_REL = 2.0e-17


@pytest.fixture(scope="module")
def L():
    _lib.build()
    return _lib.lib()


@pytest.fixture(scope="module")
def gold(golden_dir):
    return load_golden(golden_dir, "resample_grads.npz")


def test_new_entries_declared_and_exported(L):
    raw_hdr = open(os.path.join(ROOT, "include", "mmk.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", raw_hdr, flags=re.S)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(L, name) and name in _lib.EXPORTED, name
    assert L.mmk_version() == int(re.search(r"#define\s+MMK_VERSION\s+(\d+)", raw_hdr).group(1))


def test_polar_to_cart_bwd_workspace_and_argument_checks(L):
    null, fake = ctypes.c_void_p(0), ctypes.c_void_p(4096)     # never dereferenced: every call fails on the host before a launch
    B, A, R, W = 2, 24, 96, 72
    need = L.mmk_polar_to_cart_bwd_ws_bytes(B, A, R, W)
    assert need >= B * A * R * 8 + B * 4                        # a 64-bit sum per cell + the item's max |g|
    assert L.mmk_polar_to_cart_bwd_ws_bytes(0, A, R, W) == 0 and L.mmk_polar_to_cart_bwd_ws_bytes(B, 1, R, W) == 0
    sizes = [L.mmk_polar_to_cart_bwd_ws_bytes(b, A, R, W) for b in (1, 2, 3, 8, 32)]
    assert sizes == sorted(sizes) and sizes[0] < sizes[-1]

    def call(g=fake, az=fake, rg=fake, ag=fake, out=fake, ws=fake, nbytes=need, A=A, R=R):
        return L.mmk_polar_to_cart_bwd(g, az, rg, ag, B, A, R, W, 0.1, 1, 1, out, ws, nbytes, null)

    for kw in ({"g": null}, {"az": null}, {"rg": null}, {"ag": null}, {"out": null}):
        assert call(**kw) == -1 and b"NULL" in L.mmk_last_error()
    assert call(A=1) == -1 and b"bad shape" in L.mmk_last_error()
    assert call(R=1) == -1 and b"bad shape" in L.mmk_last_error()
    assert call(A=16385, nbytes=1 << 40) == -1 and b"too many azimuths" in L.mmk_last_error()
    assert call(nbytes=need - 1) == -3 and b"workspace" in L.mmk_last_error()
    assert call(ws=null) == -3 and b"workspace" in L.mmk_last_error()


def test_cart_to_polar_bwd_workspace_and_argument_checks(L):
    null, fake = ctypes.c_void_p(0), ctypes.c_void_p(4096)
    B, A, R, H, W = 2, 16, 120, 40, 48
    need = L.mmk_cart_to_polar_bwd_ws_bytes(B, A, R, H, W)
    assert need >= B * 4                                        # the sums are formed in grad_cart: only the item's max |g|
    assert L.mmk_cart_to_polar_bwd_ws_bytes(0, A, R, H, W) == 0 and L.mmk_cart_to_polar_bwd_ws_bytes(B, A, R, 1, W) == 0
    sizes = [L.mmk_cart_to_polar_bwd_ws_bytes(b, A, R, H, W) for b in (1, 2, 64, 65, 1000)]
    assert sizes == sorted(sizes) and sizes[0] < sizes[-1]

    def call(g=fake, s=fake, c=fake, rc=fake, out=fake, ws=fake, nbytes=need, A=A, H=H, W=W, rres=0.1):
        return L.mmk_cart_to_polar_bwd(g, s, c, rc, B, A, R, H, W, rres, 0.3, out, ws, nbytes, null)

    for kw in ({"g": null}, {"s": null}, {"c": null}, {"rc": null}, {"out": null}):
        assert call(**kw) == -1 and b"NULL" in L.mmk_last_error()
    assert call(H=1) == -1 and b"bad shape" in L.mmk_last_error()
    assert call(W=1) == -1 and b"bad shape" in L.mmk_last_error()
    assert call(A=65536) == -1 and b"too many azimuths" in L.mmk_last_error()
    assert call(rres=0.0) == -1 and b"positive" in L.mmk_last_error()
    assert call(nbytes=need - 1) == -3 and b"workspace" in L.mmk_last_error()
    assert call(ws=null) == -3 and b"workspace" in L.mmk_last_error()


# ----------------------------------------------------------------------------- the fixture pins itself
def _adjoint_gap(G, grad, X, FX, FabsX):
    # (math.fsum: the exactly rounded sum of the fp64 products, whatever the order numpy would add them in)
    lhs = math.fsum((G.astype(np.float64) * FX.astype(np.float64)).ravel())
    rhs = math.fsum((grad.astype(np.float64) * X.astype(np.float64)).ravel())
    scale = math.fsum((np.abs(G).astype(np.float64) * FabsX.astype(np.float64)).ravel())
    assert scale > 0
    return abs(lhs - rhs) / scale


@pytest.mark.parametrize("key", ["pc_a", "pc_b"])
@pytest.mark.parametrize("tag", [0, 1, 2])
def test_polar_to_cart_golden_gradient_is_the_adjoint(gold, key, tag):
    az, G, grad = gold[key + "_az"], gold[key + "_G"], gold["%s_grad%d" % (key, tag)]
    R, W = (int(v) for v in gold[key + "_shape"])
    res = float(gold[key + "_res"])
    F = lambda X: radar_ref.radar_polar_to_cartesian_diff(X, az, res, cart_pixel_width=W, **PC_VARIANTS[tag])
    rng = np.random.default_rng(31 + tag)
    for _ in range(2):
        X = rng.normal(size=grad.shape).astype(np.float32)
        gap = _adjoint_gap(G, grad, X, F(X), F(np.abs(X)))
        print("ADJOINT %s variant %d gap / scale = %.3e" % (key, tag, gap))
        assert gap <= PC_ADJOINT_REL, (key, tag, gap)
    if tag == 2:                                                # without the wrap rows the first and last azimuth lose taps
        assert not np.array_equal(grad, gold[key + "_grad0"])


def test_cart_to_polar_golden_gradient_is_the_adjoint(gold):
    az, G, grad = gold["cp_a_az"], gold["cp_a_G"], gold["cp_a_grad"]
    A, R = (int(v) for v in gold["cp_a_shape"])
    assert grad.dtype == np.float64
    F = lambda X: radar_ref.radar_cartesian_to_polar(X, az, 0.1, cart_resolution=0.3, polar_pixel_shape=(A, R))
    rng = np.random.default_rng(37)
    for _ in range(2):
        X = rng.normal(size=grad.shape)
        gap = _adjoint_gap(G, grad, X, F(X), F(np.abs(X)))
        print("ADJOINT cp_a gap / scale = %.3e" % gap)
        assert gap <= CP_ADJOINT_REL, gap
    assert (grad == 0).mean() > 0.4 and np.abs(grad).max() > 0   # pixels no ray touches


def test_chain_fixture_is_consistent(gold, golden_dir):
    base = load_golden(golden_dir, "radar_grads.npz")
    B, A, R = base["ch_raw"].shape
    assert gold["ch_fix_idx"].max() < B * A * R and len(gold["ch_fix_idx"]) == len(gold["ch_fix_val"])
    assert gold["ch_grad_c"].shape == (B, 640, 640) and gold["ch_grad_p"].shape == gold["ch_p"].shape == (B, A, 160)
    assert (gold["ch_n"] <= int(base["ch_npad"])).all()
    for b in range(B):
        assert np.abs(gold["ch_grad_c"][b]).max() > 0 and np.abs(gold["ch_grad_p"][b]).max() > 0
