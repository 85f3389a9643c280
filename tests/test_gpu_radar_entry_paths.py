"""The radar entries that share one launch path give the same bits, on every side of the host layer's choices of kernel.

Through the C ABI directly; B = 2 so that a stride error shows in the second item.  No tolerance anywhere: every comparison
is torch.equal, between two entries that must run the same arithmetic or between two runs of one entry.

  CFAR      mmk_cfar_mask == mmk_cfar_mask_p (one pair for the batch) == mmk_cfar_mask_p (one equal pair per scan), both values of
            diff; mmk_cfar_mask_bwd's grad_raw == mmk_cfar_mask_bwd_p's; the latter's grad_a / grad_b with and without grad_raw.
            R: 3412 | 3413 the last and the first row on either side of the persistent kernel's 40 KB of LDS, 4096 | 4097 of the
            backward's 8 cells per thread, 5500 the first size class that needs the raised dynamic-LDS limit, 600 a short row.
  peaks     the backward places the forward's points: a gradient on one point reaches that point's row alone.
  samplers  the ordered scatter of the Cartesian and of the polar sampler from a workspace of exactly *_ws_bytes, twice.
  adjoints  the three fixed-point scatters from an exact-size workspace, twice; mmk_mask_polar_scan_bwd without grad_mask.
  pair      mmk_polar_to_cart_pair(x, y) == mmk_polar_to_cart(x), mmk_polar_to_cart(y).
(The return codes and texts of a short workspace need no device: tests/test_*_cpu.py.)
"""
import ctypes
import math

import pytest
import torch

from mm_masking_amd import _lib
from mm_masking_amd import radar_utils as ru

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
B = 2
NULL = ctypes.c_void_p(0)
P = _lib.ptr


def _run(name, *args):
    _lib.check(getattr(_lib.lib(), name)(*args, _lib.stream_ptr(DEV)))
    torch.cuda.synchronize()


def _exact_ws(name, *dims):
    """A workspace of exactly the entry's own size, and that size."""
    n = int(getattr(_lib.lib(), name)(*dims))
    assert n > 0
    return torch.empty(n, dtype=torch.uint8, device=DEV), n


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ----------------------------------------------------------------------------- CFAR
CFAR_A, W2, GUARD, MINCOL = 3, 50, 5, 56
A_TH, B_TH, STEEP = 1.0, 0.09, 10.0


def _cfar_inputs(R):
    """Uniform noise plus a few spikes per row: cells on both sides of the gate, windows won on the left and on the right."""
    g = _gen(100 + R)
    raw = torch.rand(B, CFAR_A, R, generator=g) * 0.2
    cols = torch.randint(MINCOL, R - MINCOL, (B, CFAR_A, 12), generator=g)
    raw.scatter_add_(2, cols, torch.rand(B, CFAR_A, 12, generator=g) * 0.5 + 0.4)
    return raw.to(DEV).contiguous(), torch.randn(B, CFAR_A, R, generator=g).to(DEV).contiguous()


def _thresholds(n):
    return torch.full((n,), A_TH, device=DEV), torch.full((n,), B_TH, device=DEV)


@pytest.mark.parametrize("R", [600, 3412, 3413, 4096, 4097, 5500])
def test_cfar_value_and_pointer_thresholds_give_the_same_bits(R):
    raw, gmask = _cfar_inputs(R)
    shape = (P(raw), B, CFAR_A, R, W2, GUARD, MINCOL, R - MINCOL)
    for diff in (0, 1):
        by_value = torch.empty_like(raw)
        _run("mmk_cfar_mask", *shape, A_TH, B_TH, diff, STEEP, P(by_value))
        for per_scan in (0, 1):
            a, b = _thresholds(B if per_scan else 1)
            by_pointer = torch.empty_like(raw)
            _run("mmk_cfar_mask_p", *shape, P(a), P(b), per_scan, diff, STEEP, P(by_pointer))
            assert torch.equal(by_value, by_pointer), (diff, per_scan)
        kept = by_value[:, :, MINCOL:R - MINCOL].ne(0).float().mean().item()
        assert 0.0 < kept < 1.0, (diff, kept)

    shape = (P(raw), P(gmask)) + shape[1:]
    gx = torch.empty_like(raw)
    _run("mmk_cfar_mask_bwd", *shape, A_TH, B_TH, STEEP, P(gx))
    assert bool(torch.isfinite(gx).all()) and bool(gx.reshape(B, -1).abs().amax(dim=1).gt(0).all())
    ws, nbytes = _exact_ws("mmk_cfar_mask_bwd_p_ws_bytes", B, CFAR_A)
    for per_scan in (0, 1):
        a, b = _thresholds(B if per_scan else 1)
        out = []
        for with_gx in (True, False):
            gxp, ga, gb = torch.empty_like(raw) if with_gx else None, torch.empty_like(a), torch.empty_like(b)
            _run("mmk_cfar_mask_bwd_p", *shape, P(a), P(b), per_scan, STEEP, P(gxp), P(ga), P(gb), P(ws), nbytes)
            out.append((gxp, ga, gb))
        assert torch.equal(out[0][0], gx), per_scan
        assert torch.equal(out[0][1], out[1][1]) and torch.equal(out[0][2], out[1][2]), per_scan
        assert bool(out[0][1].ne(0).all()) and bool(out[0][2].ne(0).all())


# ----------------------------------------------------------------------------- peaks
def test_peaks_backward_places_the_forwards_points():
    A, R, res = 5, 64, 0.5
    max_pts = (A * (R - 1) + 1) // 2                                 # every marker pair of a scan fits: nothing is truncated
    # blobs of ones strictly inside the rows: a rising and a falling marker each, so every point lies in one row
    blobs = [[[(10, 14)], [(5, 9), (40, 47)], [], [(30, 31)], [(12, 20), (50, 60)]],
             [[(8, 12), (33, 35)], [], [(20, 29)], [(45, 52)], [(6, 7)]]]
    mask = torch.zeros(B, A, R)
    for b in range(B):
        for a in range(A):
            for lo, hi in blobs[b][a]:
                mask[b, a, lo:hi] = 1.0
    mask = mask.to(DEV)
    az = (torch.linspace(0.2, 5.8, A).repeat(B, 1) + torch.tensor([[0.0], [0.05]])).to(DEV).contiguous()
    pc, cnt = torch.empty(B, max_pts, 3, device=DEV), torch.empty(B, dtype=torch.int32, device=DEV)
    ws, nbytes = _exact_ws("mmk_extract_peaks_workspace_bytes", B, A, R, max_pts)
    _run("mmk_extract_peaks", P(mask), B, A, R, res, P(az), NULL, NULL, 1, STEEP, max_pts, P(pc), P(cnt), P(ws), nbytes)
    rows_of = [[a for a in range(A) for _ in blobs[b][a]] for b in range(B)]
    assert cnt.tolist() == [len(r) for r in rows_of]

    b, k = 1, 3                                                     # the second item's fourth point
    row = rows_of[b][k]
    assert abs(math.atan2(pc[b, k, 1].item(), pc[b, k, 0].item()) % (2 * math.pi) - az[b, row].item()) < 1e-5
    gpc = torch.zeros_like(pc)
    gpc[b, k] = torch.tensor([0.7, -1.3, 0.0])
    ws, nbytes = _exact_ws("mmk_extract_peaks_bwd_workspace_bytes", B, A, R, max_pts)
    runs = []
    for _ in range(2):
        gm = torch.full_like(mask, float("nan"))
        ws.zero_()
        _run("mmk_extract_peaks_bwd", P(mask), B, A, R, res, P(az), NULL, 1, STEEP, max_pts, P(gpc), P(gm), P(ws), nbytes)
        runs.append(gm)
    assert torch.equal(runs[0], runs[1])
    touched = runs[0].ne(0)
    assert bool(touched[b, row].any())
    touched[b, row] = False
    assert not bool(touched.any())


# ----------------------------------------------------------------------------- samplers
N, COLS = 300, 3


def _points(seed, reach):
    """(B, N, 3) points within `reach` metres of the sensor; every seventh row is a fake (0, 0) point."""
    pc = (torch.rand(B, N, COLS, generator=_gen(seed)) * 2 - 1) * reach
    pc[:, ::7, :2] = 0.0
    return pc.to(DEV).contiguous()


def _twice(name, out_shape, ws_name, ws_dims, args_before, args_after=()):
    """An ordered scatter from an exact-size workspace of arbitrary content, twice: the same bits, and something in them."""
    ws, nbytes = _exact_ws(ws_name, *ws_dims)
    runs = []
    for fill in (0, 255):
        ws.fill_(fill)
        out = torch.full(out_shape, float("nan"), device=DEV)
        _run(name, *args_before, P(out), *args_after, P(ws), nbytes)
        runs.append(out)
    assert torch.equal(runs[0], runs[1]), name
    assert bool(torch.isfinite(runs[0]).all()) and bool(runs[0].reshape(B, -1).abs().amax(dim=1).gt(0).all()), name
    return runs[0]


def test_cartesian_sampler_backward_from_an_exact_workspace():
    H = Wd = 32
    pc = _points(5, 0.5 * Wd * 0.5)
    gw = torch.randn(B, N, generator=_gen(6)).to(DEV)
    _twice("mmk_sample_weights_bwd", (B, H, Wd), "mmk_sample_weights_bwd_ws_bytes", (B, N),
           (P(gw), P(pc), B, N, COLS, H, Wd, Wd, 0.5))


def test_polar_sampler_backward_from_an_exact_workspace():
    A, R, res = 16, 24, 0.5
    pc = _points(7, 0.9 * R * res)
    gw = torch.randn(B, N, generator=_gen(8)).to(DEV)
    az = _azimuths(A)
    _twice("mmk_sample_weights_polar_bwd", (B, A, R), "mmk_sample_weights_polar_bwd_ws_bytes", (B, N),
           (P(gw), P(pc), P(az), B, N, COLS, A, R, res, 1, 1))


# ----------------------------------------------------------------------------- scatter adjoints and the pair
SW, SA, SR = 16, 8, 12                                               # W = H, A, R
RRES, CRES = 0.2, 0.2384


def _azimuths(A):
    """(B, A) ascending azimuths over the circle, the second item's wobbling a little."""
    az = torch.arange(A, dtype=torch.float32) * (2 * math.pi / A) + 0.01
    return torch.stack([az, az + 0.02 * torch.sin(3 * az)]).to(DEV).contiguous()


def _polar_geometry():
    az = _azimuths(SA).double()
    rc = (torch.arange(SR, dtype=torch.float64) * RRES).to(DEV)
    return torch.sin(az).contiguous(), torch.cos(az).contiguous(), rc


def test_polar_to_cart_adjoint_from_an_exact_workspace():
    g = torch.randn(B, SW, SW, generator=_gen(11)).to(DEV)
    az, (rg, ag) = _azimuths(SA), ru._device_grids(SW, DEV)
    _twice("mmk_polar_to_cart_bwd", (B, SA, SR), "mmk_polar_to_cart_bwd_ws_bytes", (B, SA, SR, SW),
           (P(g), P(az), P(rg), P(ag), B, SA, SR, SW, RRES, 1, 1))


def test_cart_to_polar_adjoint_from_an_exact_workspace():
    g = torch.randn(B, SA, SR, generator=_gen(12), dtype=torch.float64).to(DEV)
    s, c, rc = _polar_geometry()
    ws, nbytes = _exact_ws("mmk_cart_to_polar_bwd_ws_bytes", B, SA, SR, SW, SW)
    runs = []
    for fill in (0, 255):
        ws.fill_(fill)
        out = torch.full((B, SW, SW), float("nan"), dtype=torch.float64, device=DEV)     # the sums are formed in the output itself
        _run("mmk_cart_to_polar_bwd", P(g), P(s), P(c), P(rc), B, SA, SR, SW, SW, RRES, CRES, P(out), P(ws), nbytes)
        runs.append(out)
    assert torch.equal(runs[0], runs[1])
    assert bool(torch.isfinite(runs[0]).all()) and bool(runs[0].reshape(B, -1).abs().amax(dim=1).gt(0).all())


def test_mask_polar_scan_adjoint_with_and_without_grad_mask():
    gen = _gen(13)
    g, scan = torch.randn(B, SA, SR, generator=gen).to(DEV), torch.rand(B, SA, SR, generator=gen).to(DEV)
    mask = torch.rand(B, SW, SW, generator=gen).to(DEV)
    s, c, rc = _polar_geometry()
    head = (P(g), P(scan), P(mask), P(s), P(c), P(rc), B, SA, SR, SW, SW, RRES, CRES)
    gs = torch.full_like(scan, float("nan"))
    _twice("mmk_mask_polar_scan_bwd", (B, SW, SW), "mmk_mask_polar_scan_bwd_ws_bytes", (B, SA, SR, SW, SW), head + (P(gs),))
    alone = torch.full_like(scan, float("nan"))
    _run("mmk_mask_polar_scan_bwd", *head, P(alone), NULL, NULL, 0)
    assert torch.equal(alone, gs) and bool(gs.reshape(B, -1).abs().amax(dim=1).gt(0).all())


def test_polar_to_cart_pair_equals_two_single_calls():
    gen = _gen(14)
    x, y = torch.rand(B, SA, SR, generator=gen).to(DEV), torch.rand(B, SA, SR, generator=gen).to(DEV)
    az, (rg, ag) = _azimuths(SA), ru._device_grids(SW, DEV)
    shape = (P(az), P(rg), P(ag), B, SA, SR, SW, RRES, 1, 1)
    one = [torch.full((B, SW, SW), float("nan"), device=DEV) for _ in range(2)]
    two = [torch.full((B, SW, SW), float("nan"), device=DEV) for _ in range(2)]
    _run("mmk_polar_to_cart", P(x), *shape, P(one[0]))
    _run("mmk_polar_to_cart", P(y), *shape, P(one[1]))
    _run("mmk_polar_to_cart_pair", P(x), P(y), *shape, P(two[0]), P(two[1]))
    assert torch.equal(one[0], two[0]) and torch.equal(one[1], two[1])
    assert bool(one[0].reshape(B, -1).amax(dim=1).gt(0).all()) and not torch.equal(one[0], one[1])
