"""CPU: the C ABI of the input-image gradient (mmk_conv_first_dgrad, mmk_input_norm_bwd, mmk_unet_backward_input) -- declared,
exported, host-side argument checks (no launch) -- and the CPU mirror of the policy against the reference's golden input
gradients (tests/golden/input_grads.npz)."""
import ctypes
import re

import pytest
import torch

from mm_masking_amd import _lib

import input_grad_cases as igc
from support import header, n_args

NEW = ("mmk_conv_first_dgrad_ws_bytes", "mmk_conv_first_dgrad", "mmk_input_norm_bwd", "mmk_unet_backward_input")
NULL = ctypes.c_void_p(0)
FAKE = ctypes.c_void_p(4096)          # never dereferenced: every call below fails on the host before any launch
ERR_ARG = -1


@pytest.fixture(scope="module")
def L():
    _lib.build()
    return _lib.lib()


def test_new_entries_declared_and_exported(L):
    hdr = header()
    for name in NEW:
        assert hasattr(L, name) and name in _lib.EXPORTED, name
        assert n_args(hdr, name) == len(_lib.EXPORTED[name][1]), name         # the binding has the header's arity
    assert L.mmk_version() == int(re.search(r"#define\s+MMK_VERSION\s+(\d+)", hdr).group(1))
    for mode, val in (("NONE", None), ("MINMAX", "minmax"), ("STANDARDIZE", "standardize")):
        assert int(re.search(r"#define\s+MMK_NORM_%s\s+(\d+)" % mode, hdr).group(1)) == _lib.NORM_MODES[val]


def test_conv_first_dgrad_argument_checks(L):
    need = L.mmk_conv_first_dgrad_ws_bytes(3)
    # per channel (S1, S2, #min, #max) in fp64: the totals + one set per block
    assert need >= 3 * 4 * 8 * 2 and L.mmk_conv_first_dgrad_ws_bytes(1) < need <= L.mmk_conv_first_wgrad_ws_bytes(3)

    def call(g=FAKE, cin=3, W=FAKE, x=FAKE, pre=FAKE, mm=FAKE, B=2, H=32, Wd=32, gx=FAKE, ws=FAKE, nbytes=need):
        return L.mmk_conv_first_dgrad(g, cin, W, x, pre, mm, B, H, Wd, gx, ws, nbytes, NULL)

    for kw in ({"g": NULL}, {"W": NULL}, {"gx": NULL}, {"x": NULL}, {"pre": NULL}):
        assert call(**kw) == ERR_ARG and b"NULL" in L.mmk_last_error(), kw
    assert call(ws=NULL) == ERR_ARG and b"workspace" in L.mmk_last_error()        # tie counts without statistics
    assert call(cin=0) == ERR_ARG and b"cin" in L.mmk_last_error()
    assert call(cin=5) == ERR_ARG and b"cin" in L.mmk_last_error()
    assert call(H=0) == ERR_ARG
    assert call(nbytes=need - 1) == ERR_ARG and b"workspace too small" in L.mmk_last_error()


def test_input_norm_bwd_argument_checks(L):
    need = L.mmk_conv_first_dgrad_ws_bytes(2)

    def call(gx=FAKE, x=FAKE, cin=2, pre=FAKE, mm=FAKE, mode=1, B=2, H=32, Wd=32, ws=FAKE, nbytes=need):
        return L.mmk_input_norm_bwd(gx, x, cin, pre, mm, mode, B, H, Wd, ws, nbytes, NULL)

    assert call(mode=3) == ERR_ARG and b"mode" in L.mmk_last_error()
    assert call(mode=-1) == ERR_ARG and b"mode" in L.mmk_last_error()
    for kw in ({"gx": NULL}, {"x": NULL}, {"pre": NULL}, {"mm": NULL}, {"ws": NULL}):
        assert call(**kw) == ERR_ARG and b"NULL" in L.mmk_last_error(), kw
    assert call(mode=2, mm=NULL, nbytes=need - 1) == ERR_ARG and b"workspace too small" in L.mmk_last_error()
    assert call(cin=5) == ERR_ARG and b"cin" in L.mmk_last_error()
    assert call(mode=0, x=NULL, pre=NULL, mm=NULL, ws=NULL, nbytes=0) == 0          # nothing to add: no launch


def test_unet_backward_input_argument_checks(L):
    pp = (ctypes.c_void_p * 46)(*[4096] * 46)

    def desc(cin=1, pre=4096):
        return _lib.UNetDesc(B=1, H=32, W=32, cin=cin, x=4096, pre=pre, params=pp, workspace=4096, workspace_bytes=1 << 30, mask=4096)

    def call(d, gx=FAKE, mode=1, mm=FAKE):
        return L.mmk_unet_backward_input(ctypes.byref(d) if d is not None else None, FAKE, pp, gx, mode, mm, FAKE, 1 << 30, None, NULL)

    assert call(None) == ERR_ARG and b"NULL" in L.mmk_last_error()
    assert call(desc(), gx=NULL) == ERR_ARG and b"NULL" in L.mmk_last_error()
    assert call(desc(cin=0)) == ERR_ARG and b"cin" in L.mmk_last_error()
    assert call(desc(cin=5)) == ERR_ARG and b"cin" in L.mmk_last_error()
    assert call(desc(), mode=7) == ERR_ARG and b"mode" in L.mmk_last_error()
    assert call(desc(), mm=NULL) == ERR_ARG and b"minmax" in L.mmk_last_error()
    assert call(desc(pre=None), mode=2) == ERR_ARG and b"pre" in L.mmk_last_error()


MEASURED = {"n1": 0.0, "n3": 0.0}       # max |fft.grad - golden| / max |golden| of this mirror where the fixture was generated:
#                                         bit-identical (so is x 1.3); the bound below is the stated 1e-5, which leaves room for
#                                         another torch build's convolution order


@pytest.mark.parametrize("tag", ["n1", "n3"])
def test_cpu_mirror_input_grad_matches_reference(golden_dir, tag):
    """unet_backend="torch" on the CPU: fft.grad (and cfar.grad) of the policy reproduce the reference module's to 1e-5 of the
    largest value (the same fp32 torch operators in the same order; measured: MEASURED)."""
    g = igc.load_golden(golden_dir)
    dev = torch.device("cpu")
    model = igc.golden_model(g, tag, dev, unet_backend="torch")
    mask, gx, gcfar = igc.golden_input_grads(g, tag, model, dev)
    want = torch.from_numpy(g["gx_" + tag])
    assert (mask - torch.from_numpy(g["mask_" + tag])).abs().max() < 1e-5
    err = ((gx - want).abs().max() / want.abs().max()).item()
    print("cpu mirror %s: max |fft.grad - golden| / max |golden| = %.3g" % (tag, err))
    assert gx.dtype == want.dtype and gx.shape == want.shape
    assert err <= 1e-5, err
    if tag == "n3":
        wc = torch.from_numpy(g["gcfar_" + tag])
        errc = ((gcfar - wc).abs().max() / wc.abs().max()).item()
        print("cpu mirror %s: max |cfar.grad - golden| / max |golden| = %.3g" % (tag, errc))
        assert errc <= 1e-5, errc
    else:
        assert gcfar is None
