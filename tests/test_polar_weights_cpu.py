"""CPU: the C ABI of the polar-aware sampler (mmk_sample_weights_polar_*) -- declared, exported, bound, host-side argument checks
(no launch) -- the policy's constructor checks for params["polar_sampling"], and the test-side restatement against the golden
images of the reference's radar_polar_to_cartesian_diff at the pixel centres."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

from mm_masking_amd import _lib
from mm_masking_amd import radar_utils as ru
from mm_masking_amd import train_icp_weights as trn
from mm_masking_amd.icp_weight_policy import LearnICPWeightPolicy
from polar_weights_ref import azimuth_tables, polar_weights_ref, position_error
from support import policy_params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mmk_sample_weights_polar_fwd", "mmk_sample_weights_polar_bwd_ws_bytes", "mmk_sample_weights_polar_bwd",
       "mmk_sample_weights_polar_bwd_pc")


@pytest.fixture(scope="module")
def L():
    _lib.build()
    return _lib.lib()


def test_new_entries_declared_exported_and_bound(L):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mmk.h")).read(), flags=re.S)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(L, name) and name in _lib.EXPORTED, name
    assert L.mmk_version() == 502
    assert "extract_weights_polar" in ru.__all__ and "polar_target_from_pts" in ru.__all__


def test_workspace_bytes(L):
    ws = [L.mmk_sample_weights_polar_bwd_ws_bytes(2, n) for n in (1, 300, 301, 5120)]
    assert ws[0] > 0 and all(a < b for a, b in zip(ws, ws[1:]))
    assert L.mmk_sample_weights_polar_bwd_ws_bytes(2, 300) == L.mmk_sample_weights_bwd_ws_bytes(2, 300)     # a function of (B, N)
    assert L.mmk_sample_weights_polar_bwd_ws_bytes(0, 300) == 0 and L.mmk_sample_weights_polar_bwd_ws_bytes(2, 0) == 0


NULL = ctypes.c_void_p(0)
FAKE = ctypes.c_void_p(4096)          # never dereferenced: every call below fails on the host before any launch
GOOD = dict(B=1, N=4, cols=3, A=16, R=96, res=0.0596)


def _fwd(L, mask=FAKE, pc=FAKE, az=FAKE, out=FAKE, **kw):
    s = dict(GOOD, **kw)
    return L.mmk_sample_weights_polar_fwd(mask, pc, az, s["B"], s["N"], s["cols"], s["A"], s["R"], s["res"], 1, 1, out, NULL)


def _bwd(L, gw=FAKE, pc=FAKE, az=FAKE, gm=FAKE, ws=FAKE, nbytes=None, **kw):
    s = dict(GOOD, **kw)
    nbytes = L.mmk_sample_weights_polar_bwd_ws_bytes(max(s["B"], 1), max(s["N"], 1)) if nbytes is None else nbytes
    return L.mmk_sample_weights_polar_bwd(gw, pc, az, s["B"], s["N"], s["cols"], s["A"], s["R"], s["res"], 1, 1, gm, ws, nbytes, NULL)


def _bwd_pc(L, gw=FAKE, mask=FAKE, pc=FAKE, az=FAKE, gpc=FAKE, **kw):
    s = dict(GOOD, **kw)
    return L.mmk_sample_weights_polar_bwd_pc(gw, mask, pc, az, s["B"], s["N"], s["cols"], s["A"], s["R"], s["res"], 1, 1, gpc, NULL)


@pytest.mark.parametrize("call,pointers", [(_fwd, ("mask", "pc", "az", "out")), (_bwd, ("gw", "pc", "az", "gm", "ws")),
                                           (_bwd_pc, ("gw", "mask", "pc", "az", "gpc"))])
def test_argument_checks(L, call, pointers):
    for name in pointers:
        assert call(L, **{name: NULL}) == -1 and b"NULL" in L.mmk_last_error(), name
    for bad in ({"cols": 1}, {"A": 1}, {"R": 1}, {"B": 0}, {"N": 0}, {"B": -1}, {"N": -3}):
        assert call(L, **bad) == -1 and b"shape" in L.mmk_last_error(), bad
    assert call(L, A=16385) == -1 and b"azimuths" in L.mmk_last_error()          # 64 KiB of LDS hold 16384 floats
    assert call(L, res=0.0) == -1 and b"radar_resolution" in L.mmk_last_error()


def test_workspace_too_small(L):
    need = L.mmk_sample_weights_polar_bwd_ws_bytes(GOOD["B"], GOOD["N"])
    assert _bwd(L, nbytes=need - 1) == -1 and b"workspace" in L.mmk_last_error()
    assert _bwd(L, nbytes=0) == -1 and b"workspace" in L.mmk_last_error()


_policy_params = functools.partial(policy_params, torch.device("cpu"), unet_backend="torch")


def test_policy_constructor_checks():
    with pytest.raises(ValueError, match="polar"):
        LearnICPWeightPolicy(_policy_params(polar_sampling=True))                                  # a Cartesian network
    with pytest.raises(ValueError, match="weights"):
        LearnICPWeightPolicy(_policy_params(polar_sampling=True, network_input_type="polar", mask_target="scan"))
    m = LearnICPWeightPolicy(_policy_params(polar_sampling=True, network_input_type="polar"))
    assert m.polar_sampling is True
    assert LearnICPWeightPolicy(_policy_params(network_input_type="polar")).polar_sampling is False
    assert LearnICPWeightPolicy(_policy_params(polar_sampling=False)).polar_sampling is False
    assert "polar_sampling" not in trn.default_params(torch.device("cpu"))


def test_policy_forward_checks_on_the_host():
    """Without the azimuths: KeyError naming where they come from; on a CPU device: MmkError (no CPU path)."""
    m = LearnICPWeightPolicy(_policy_params(polar_sampling=True, network_input_type="polar"))
    scan = {"fft_data": torch.rand(1, 32, 64), "fft_cfar": torch.zeros(1, 32, 64), "raw_pc": torch.rand(1, 8, 3)}
    with pytest.raises(KeyError, match="prepare_batch.*keep_polar=True"):
        m(scan, {"pc": torch.zeros(1, 4, 6)}, None)
    scan["azimuths"] = torch.from_numpy(azimuth_tables(32, 1)[:1])
    with pytest.raises(_lib.MmkError, match="HIP device"):
        m(scan, {"pc": torch.zeros(1, 4, 6)}, None)


@pytest.mark.parametrize("cross,wob", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_restatement_reproduces_the_golden_at_pixel_centres(golden_dir, cross, wob):
    """The test-side reference at the centres of the 32 x 32 grid of 0.2384 m pixels against the reference's own
    radar_polar_to_cartesian_diff: the GPU tests compare the kernels with this restatement."""
    g = np.load(os.path.join(golden_dir, "polar_weights.npz"), allow_pickle=False)
    W = int(g["pw_width"])
    half = (W / 2 - 0.5) * 0.2384
    coords = torch.linspace(-half, half, W)
    pts = torch.stack([(-coords)[:, None].expand(W, W), coords[None, :].expand(W, W)], dim=-1).reshape(1, -1, 2).expand(2, -1, -1)
    w, _ = polar_weights_ref(torch.from_numpy(g["pw_mask"]), pts, torch.from_numpy(g["pw_az"]), float(g["pw_res"]), bool(cross),
                             bool(wob))
    want = g["pw_cart_%d%d" % (cross, wob)]
    bound = position_error(g["pw_az"]) * float(g["pw_mask"].max()) + 4 * 2.0 ** -23
    assert np.abs(w.reshape(2, W, W).numpy() - want).max() <= bound
    assert (want == 0).any() and ((w.reshape(2, W, W).numpy() == 0) == (want == 0)).all()         # the corners beyond the last bin
