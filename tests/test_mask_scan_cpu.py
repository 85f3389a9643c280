"""CPU: the mask applied to the scan (mmk_mask_polar_scan, mmk_mask_polar_scan_bwd and its *_ws_bytes; radar_utils.mask_polar_scan;
LearnICPWeightPolicy's mask_target) -- what can be checked without a device: the entries are declared and exported, their
host-side argument and workspace checks (no launch), the policy's key, and the golden fixture itself
(tests/golden/mask_scan.npz, written by tests/golden/make_golden_mask_scan.py).

Tolerance of the forward against oracle/radar_ref.py evaluated on this host: 2^-23 absolute.  Mask and scan are below 1, so
the output is below 1; the fixture may come from a host whose sin / cos differ in the last fp64 bit, which can move the one
fp32 rounding of the polar mask by an ulp (at most 2^-24 below 1) before the product with a scan value below 1.
"""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

from mm_masking_amd import _lib
from oracle import radar_ref
from support import ROOT, load_golden, policy_params

NEW = ("mmk_mask_polar_scan", "mmk_mask_polar_scan_bwd", "mmk_mask_polar_scan_bwd_ws_bytes")
FWD_ABS = 2.0 ** -23


@pytest.fixture(scope="module")
def L():
    _lib.build()
    return _lib.lib()


@pytest.fixture(scope="module")
def gold(golden_dir):
    return load_golden(golden_dir, "mask_scan.npz")


def test_new_entries_declared_and_exported(L):
    raw_hdr = open(os.path.join(ROOT, "include", "mmk.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", raw_hdr, flags=re.S)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(L, name) and name in _lib.EXPORTED, name
    assert L.mmk_version() == int(re.search(r"#define\s+MMK_VERSION\s+(\d+)", raw_hdr).group(1))
    from mm_masking_amd import radar_utils as ru
    from mm_masking_amd.dropin import radar_utils as dropin
    assert "mask_polar_scan" in ru.__all__ and dropin.mask_polar_scan is ru.mask_polar_scan


def test_forward_argument_checks(L):
    null, fake = ctypes.c_void_p(0), ctypes.c_void_p(4096)     # never dereferenced: every call fails on the host before a launch
    B, A, R, H, W = 2, 16, 120, 40, 48

    def call(scan=fake, mask=fake, s=fake, c=fake, rc=fake, out=fake, B=B, A=A, H=H, W=W, cres=0.3):
        return L.mmk_mask_polar_scan(scan, mask, s, c, rc, B, A, R, H, W, cres, out, null)

    for kw in ({"scan": null}, {"mask": null}, {"s": null}, {"c": null}, {"rc": null}, {"out": null}):
        assert call(**kw) == -1 and b"mmk_mask_polar_scan: NULL" in L.mmk_last_error()
    for kw in ({"H": 1}, {"W": 1}, {"B": 65536}, {"A": 65536}, {"B": 0}):
        assert call(**kw) == -1 and b"mmk_mask_polar_scan: bad shape" in L.mmk_last_error()
    assert call(cres=0.0) == -1 and b"mmk_mask_polar_scan: cart_resolution must be positive" in L.mmk_last_error()


def test_backward_workspace_and_argument_checks(L):
    null, fake = ctypes.c_void_p(0), ctypes.c_void_p(4096)
    B, A, R, H, W = 2, 16, 120, 40, 48
    need = L.mmk_mask_polar_scan_bwd_ws_bytes(B, A, R, H, W)
    assert need >= B * H * W * 8 + B * 4                        # a 64-bit sum per pixel + the item's max
    assert L.mmk_mask_polar_scan_bwd_ws_bytes(0, A, R, H, W) == 0 and L.mmk_mask_polar_scan_bwd_ws_bytes(B, A, R, 1, W) == 0
    sizes = [L.mmk_mask_polar_scan_bwd_ws_bytes(b, A, R, H, W) for b in (1, 2, 3, 8, 32)]
    assert sizes == sorted(sizes) and sizes[0] < sizes[-1]

    def call(g=fake, scan=fake, mask=fake, s=fake, c=fake, rc=fake, gs=fake, gm=fake, ws=fake, nbytes=need, B=B, A=A, H=H, W=W,
             rres=0.1, cres=0.3):
        return L.mmk_mask_polar_scan_bwd(g, scan, mask, s, c, rc, B, A, R, H, W, rres, cres, gs, gm, ws, nbytes, null)

    for kw in ({"g": null}, {"scan": null}, {"mask": null}, {"s": null}, {"c": null}, {"rc": null}):
        assert call(**kw) == -1 and b"mmk_mask_polar_scan_bwd: NULL" in L.mmk_last_error()
    for kw in ({"H": 1}, {"W": 1}, {"B": 65536}, {"A": 65536}):
        assert call(**kw) == -1 and b"mmk_mask_polar_scan_bwd: bad shape" in L.mmk_last_error()
    for kw in ({"rres": 0.0}, {"cres": -1.0}):
        assert call(**kw) == -1 and b"mmk_mask_polar_scan_bwd: resolutions must be positive" in L.mmk_last_error()
    assert call(nbytes=need - 1) == -3 and b"mmk_mask_polar_scan_bwd: workspace" in L.mmk_last_error()
    assert call(ws=null) == -3 and b"mmk_mask_polar_scan_bwd: workspace" in L.mmk_last_error()
    assert call(gs=null, nbytes=need - 1) == -3                 # grad_mask alone still needs the workspace
    assert call(gs=null, gm=null, ws=null, nbytes=0) == 0       # nothing asked for: nothing launched


# ----------------------------------------------------------------------------- the fixture
def _polar_mask(gold, key):
    A, R = (int(v) for v in gold[key + "_shape"])
    rres, cres = (float(v) for v in gold[key + "_res"])
    return radar_ref.radar_cartesian_to_polar(gold[key + "_mask"].astype(np.float64), gold[key + "_az"], rres,
                                              cart_resolution=cres, polar_pixel_shape=(A, R))


@pytest.mark.parametrize("key", ["ms_a", "ms_b"])
def test_golden_forward_is_the_host_restatement(gold, key):
    y = _polar_mask(gold, key).astype(np.float32) * gold[key + "_scan"]
    assert y.dtype == np.float32 and gold[key + "_y"].dtype == np.float32
    err = np.abs(y.astype(np.float64) - gold[key + "_y"]).max()
    print("FORWARD %s max abs diff = %.3e" % (key, err))
    assert err <= FWD_ABS
    assert gold[key + "_mask"].max() < 1 and gold[key + "_scan"].max() < 1 and gold[key + "_mask"].min() > 0


def _tap_mass(gold, key):
    """d sum(P) / d mask on the host: the tap weights of radar_ref.radar_cartesian_to_polar's coordinates, added per pixel."""
    A, R = (int(v) for v in gold[key + "_shape"])
    rres, cres = (float(v) for v in gold[key + "_res"])
    B, H, W = gold[key + "_mask"].shape
    az = torch.as_tensor(gold[key + "_az"])
    rc = torch.linspace(0.0, (R - 1) * rres, R, dtype=torch.float64).numpy()
    s, c = torch.sin(az).numpy(), torch.cos(az).numpy()
    ix = (((s[:, :, None] * rc) / cres / (W - 1) * 2 + 1.0) / 2.0) * (W - 1)
    iy = (((-(c[:, :, None] * rc) / cres) / (H - 1) * 2 + 1.0) / 2.0) * (H - 1)
    x0, y0 = np.floor(ix), np.floor(iy)
    wx, wy = ix - x0, iy - y0
    mass = np.zeros((B, H, W))
    bidx = np.broadcast_to(np.arange(B)[:, None, None], ix.shape)
    for dy, dx, w in ((0, 0, (1 - wy) * (1 - wx)), (0, 1, (1 - wy) * wx), (1, 0, wy * (1 - wx)), (1, 1, wy * wx)):
        yi, xi = y0.astype(np.int64) + dy, x0.astype(np.int64) + dx
        ok = (xi >= 0) & (xi < W) & (yi >= 0) & (yi < H)
        np.add.at(mass, (bidx[ok], yi[ok], xi[ok]), w[ok])
    return mass


def test_fixture_conditions_hold(gold):
    mass = _tap_mass(gold, "ms_a")
    B, A, R = gold["ms_a_scan"].shape
    assert mass.max() > 10 and mass.sum() / (B * A * R) < 0.9 and (mass != 0).mean() < 0.6
    assert gold["ms_a_notap"].mean() >= 0.10
    assert np.array_equal(gold["ms_a_notap"], _polar_mask({**gold, "ms_a_mask": np.ones_like(gold["ms_a_mask"])}, "ms_a") == 0)
    # pixels no ray touches receive nothing; cells without a tap give and receive nothing
    assert (gold["ms_a_grad_mask"][mass == 0] == 0).all() and (gold["ms_a_grad_mask"] == 0).mean() > 0.4
    for key in ("ms_a", "ms_b"):
        assert (gold[key + "_y"][gold[key + "_notap"]] == 0).all() and (gold[key + "_grad_scan"][gold[key + "_notap"]] == 0).all()
        assert np.abs(gold[key + "_grad_mask"]).max() > 0 and np.abs(gold[key + "_grad_scan"]).max() > 0
    # ms_b: more than one 256-thread block per ray with a ragged tail; the rays leave the image after 128-180 cells
    B, A, R = gold["ms_b_scan"].shape
    assert R > 256 and R % 256 != 0
    first_out = gold["ms_b_notap"][0].argmax(axis=1)
    assert (first_out >= 120).all() and (first_out <= 190).all()


def test_chain_fixture_is_consistent(gold, golden_dir):
    base = np.load(os.path.join(golden_dir, "radar_grads.npz"))
    rg = np.load(os.path.join(golden_dir, "resample_grads.npz"))
    B = base["ch_raw"].shape[0]
    assert gold["ms_ch_n"].tolist() == rg["ch_n"].tolist()      # the same front end: the same cloud
    assert np.array_equal(gold["ms_ch_cloud"], rg["ch_cloud"])
    assert gold["ms_ch_grad_mask"].shape == (B, 640, 640) and gold["ms_ch_grad_mask"].dtype == np.float32
    assert gold["ms_ch_T"].shape == (B, 4, 4) and not np.array_equal(gold["ms_ch_T"], rg["ch_T"])     # unweighted ICP
    for b in range(B):
        assert np.abs(gold["ms_ch_grad_mask"][b]).max() > 0
    assert os.path.getsize(os.path.join(golden_dir, "mask_scan.npz")) < 600 * 1024


# ----------------------------------------------------------------------------- the policy's key
_params = functools.partial(policy_params, torch.device("cpu"))


def _cpu_batch(B=1, H=32, A=8, R=40, polar=True):
    scan = {"fft_data": torch.rand(B, H, H), "fft_cfar": torch.zeros(B, H, H), "raw_pc": torch.zeros(B, 4, 3),
            "filtered_pc": torch.zeros(B, 4, 3)}
    if polar:
        scan.update({"fft_polar": torch.rand(B, A, R), "azimuths": torch.rand(B, A).sort(dim=1).values * 6})
    return scan, {"pc": torch.zeros(B, 4, 6)}, torch.eye(4).repeat(B, 1, 1)


def test_mask_target_values():
    from mm_masking_amd.icp_weight_policy import LearnICPWeightPolicy
    with pytest.raises(ValueError, match="mask_target"):
        LearnICPWeightPolicy(_params(mask_target="bogus"))
    absent, weights, scan = (LearnICPWeightPolicy(_params(**kw)) for kw in ({}, {"mask_target": "weights"}, {"mask_target": "scan"}))
    assert absent.mask_target == "weights" and weights.mask_target == "weights" and scan.mask_target == "scan"
    assert list(absent.state_dict().keys()) == list(weights.state_dict().keys()) == list(scan.state_dict().keys())


def test_scan_mode_refuses_a_cpu_device_and_a_batch_without_the_scan():
    from mm_masking_amd.icp_weight_policy import LearnICPWeightPolicy
    model = LearnICPWeightPolicy(_params(mask_target="scan", unet_backend="torch"))
    scan, mp, T0 = _cpu_batch()
    with pytest.raises(_lib.MmkError, match="mask_target='scan'"):
        model(scan, mp, T0)
    for key in ("fft_polar", "azimuths"):
        short = {k: v for k, v in scan.items() if k != key}
        with pytest.raises(KeyError, match=key):
            model(short, mp, T0)


def test_prepare_batch_and_finish_batch_defaults_leave_the_batch_alone():
    import inspect
    from mm_masking_amd import icp_weight_dataset as ds
    assert inspect.signature(ds.finish_batch).parameters["keep_polar"].default is False
    assert inspect.signature(ds.DeviceLoader.__init__).parameters["keep_polar"].default is False
