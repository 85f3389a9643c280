"""CPU: the forward edge fixture of the radar front end (tests/golden/radar_edges.npz, written by
tests/golden/make_golden_radar_edges.py) -- the conditions its generator asserts, re-asserted on the stored arrays; the numpy
oracle (oracle/radar_ref.py) against every stored output of the reference; and the host-side refusals of the longest CFAR row
and of the shortest extractor row (no launch).

Oracle against the reference's stored outputs, measured on the build host (bound in brackets):
    CFAR hard mask, 8 cases                         equal        [equal]
    CFAR soft mask, 8 cases                         6.0e-8       [2e-5]
    clouds, hard (pk0, pk2..pk5, with / without T)  2.4e-7       [3e-5]
    clouds, soft (pks)                              2.4e-7       [3e-5]
    resampler, tables from 0 / short / wobbly       2.3e-6 / 1.9e-6 / 2.5e-6   [5e-6]
    weights, 640 x 640 and 40 x 96                  6.0e-8       [2e-5]
    BEV                                             equal        [equal]

What the reference does at the edges, pinned here on the stored arrays:
  * pk0 (the issue's (1, 3, 13) mask): markers at cells 0, 2, 9 | 4, 5 | 1, 3, 4, 6, 10 of its three rows, ten in all, five
    points, of which two pair markers of different rows (the blob that reaches column 12 of row 0 never closes)
  * pk1 (R = 2, one marker per item): the reference pairs index lists of lengths 0 and 1, which broadcasts to an EMPTY cloud;
    it raises only from three markers on.  oracle.radar_ref.extract_pc raises on every odd count
  * resampler: a pixel reads zero padding alone once its range coordinate u = rng / res - 0.5 reaches R, that is from
    (R + 0.5) res on; between (R - 0.5) res and (R + 0.5) res it keeps the tap of the last bin.  With the wobble fix a pixel
    above the last azimuth is clamped to the last row (c3 = A - 1, delta = 0) and is NOT zero, with and without the crossover rows
"""
import ctypes

import numpy as np
import pytest

from mm_masking_amd import _lib
from oracle import radar_ref
from radar_edge_cases import (CF_RES, EW_MASKS, LAST_R, PC_CASES, PC_TABLES, PC_VARIANTS, PEAK_HARD, PEAK_SOFT, SOFT_STEEP,
                              assert_cfar_conditions, assert_peak_conditions, assert_table_conditions, beyond_range,
                              bev_pixel_index, cf_sets, ew_mask, ew_pixel_index, marker_rows, off_grid, peak_case,
                              pixel_range_angle)
from support import load_golden


@pytest.fixture(scope="module")
def L():
    _lib.build()
    return _lib.lib()


@pytest.fixture(scope="module")
def gold(golden_dir):
    return load_golden(golden_dir, "radar_edges.npz")


# ----------------------------------------------------------------------------- CFAR
@pytest.mark.parametrize("tag,kw", cf_sets())
def test_cfar_conditions_and_oracle(gold, tag, kw):
    raw = gold["cf_raw"]
    R = raw.shape[2]
    th64, (w2, guard, mincol, maxcol) = assert_cfar_conditions(raw, CF_RES, **kw)
    assert mincol == w2 + guard + 1 and maxcol == (R if tag[1] == "b" else int(80.0 / CF_RES - w2 - guard))
    th32 = radar_ref.cfar_threshold(raw, CF_RES, **{k: v for k, v in kw.items() if k != "steep_fact"})
    assert np.abs(th32[:, :, mincol:maxcol] - th64).max() < 4e-7 and (th32[:, :, :mincol] == 1000).all()
    hard = gold["cf_hard" + tag].astype(np.float32)
    assert np.array_equal(radar_ref.cfar_mask(raw, CF_RES, diff=False, **kw), hard)
    err = np.abs(radar_ref.cfar_mask(raw, CF_RES, diff=True, **kw) - gold["cf_soft" + tag]).max()
    print("oracle vs fixture: cf_soft%s %.3e" % (tag, err))
    assert err <= 2e-5
    assert 0 < hard[:, :, mincol:maxcol].mean() < 1 and hard[:, :, mincol].any()
    if tag[1] == "b":                                               # kept cells whose right window is cut, and cut to nothing
        assert hard[:, :, -(w2 + guard):].any() and hard[:, :, -(guard + 1):].any()


# ----------------------------------------------------------------------------- extractor
@pytest.mark.parametrize("name", PEAK_HARD + PEAK_SOFT)
def test_peaks_conditions_and_oracle(gold, name):
    c = peak_case(gold, name)
    n = assert_peak_conditions(name, dict(mask=c["mask"], res=c["res"], diff=c["diff"], steep=SOFT_STEEP))
    assert np.array_equal(n, c["nmark"]) and np.array_equal(n // 2, c["n"])
    if name == "pk1":
        assert c["pc"] is None and (c["n"] == 0).all()
        with pytest.raises(RuntimeError):
            radar_ref.extract_pc(c["mask"], c["res"], c["az"], c["tm"], diff=False)
        return
    for key, T in (("pc", None), ("pcT", c["T_ab"])):
        want = radar_ref.extract_pc(c["mask"], c["res"], c["az"], c["tm"], T_ab=T, diff=c["diff"], steep_fact=SOFT_STEEP)
        for b, w in enumerate(want):
            assert w.shape[0] == c["n"][b] and (c[key][b, c["n"][b]:] == 0).all()
            err = np.abs(w - c[key][b, :c["n"][b]]).max()
            print("oracle vs fixture: %s %s item %d %.3e" % (name, key, b, err))
            assert err <= 3e-5


def test_peaks_edge_behaviour_of_the_reference(gold):
    c = peak_case(gold, "pk0")
    rows = marker_rows(c["mask"], c["res"], False)[0]
    assert rows.tolist() == [0, 0, 0, 1, 1, 2, 2, 2, 2, 2] and c["n"].tolist() == [5]
    assert (rows[0::2] != rows[1::2]).sum() == 2                    # the open blob of row 0 shifts the pairing across two row ends
    np.testing.assert_allclose(np.hypot(*c["pc"][0, 0, :2]), (0.5 + 1.0) / 2, atol=1e-6)     # cell 0 has range 0: marker 0 = cell 1
    assert gold["pk4_nmark"].tolist() == [64] and gold["pk3_mask"].shape == (1, 300, 8) and gold["pk2_mask"].shape[2] % 4 == 1
    open_end = peak_case(gold, "pk5")
    assert open_end["mask"][0, -1, -1] == 1 and open_end["nmark"][0] % 2 == 0
    soft = peak_case(gold, "pks")
    assert marker_rows(soft["mask"], soft["res"], True)[0].tolist() == [0] * 7 + [1] * 5 + [2] * 2


# ----------------------------------------------------------------------------- resampler
@pytest.mark.parametrize("ci", range(len(PC_CASES)))
def test_resampler_conditions_and_oracle(gold, ci):
    A, R, res, W = PC_CASES[ci]
    img = gold["pc%d_img" % ci]
    assert img.shape == (2, A, R)
    zero, edge = beyond_range(W, R, res)
    _, ang = pixel_range_angle(W)
    if ci < 2:
        assert zero.sum() >= 20 and edge.any()                      # (the 17-pixel image lies inside the last bin altogether)
    for kind in PC_TABLES:
        az = gold["pc%d_az_%s" % (ci, kind)]
        assert_table_conditions(az)
        assert not np.array_equal(az[0], az[1]) and ((az[:, 0] == 0).all() if kind == "zero" else (az[:, 0] > 0).all())
        for vi, kw in enumerate(PC_VARIANTS):
            cart = gold["pc%d_cart_%s%d" % (ci, kind, vi)]
            err = np.abs(radar_ref.radar_polar_to_cartesian_diff(img, az, res, cart_pixel_width=W, **kw) - cart).max()
            print("oracle vs fixture: pc%d %s %d %.3e" % (ci, kind, vi, err))
            assert err <= 5e-6
            assert (cart[:, zero] == 0).all() and (ci == 2 or (cart[:, edge] != 0).any())
            if kind == "short" and kw.get("fix_wobble", True):      # above the last azimuth: clamped to the last row, not padded
                above = ang > az.astype(np.float64).max() + 1e-3
                assert above.any() and (cart[:, above & ~zero] != 0).any()


# ----------------------------------------------------------------------------- sampler and rasteriser
@pytest.mark.parametrize("tag", sorted(EW_MASKS))
def test_weights_conditions_and_oracle(gold, tag):
    pts, mask = gold["ew_pts"], ew_mask(tag)
    assert int(gold["ew_seed_" + tag]) == EW_MASKS[tag][3]
    out = radar_ref.extract_weights(mask, pts)
    on = ~off_grid(*ew_pixel_index(pts, *mask.shape[1:]))
    assert on.sum() >= 8 and np.array_equal(out[0][on], gold["ew_w_" + tag][on])     # on the grid: the oracle agrees exactly
    err = np.abs(out[0] - gold["ew_w_" + tag]).max()
    print("oracle vs fixture: ew_w_%s %.3e" % (tag, err))
    assert err <= 2e-5
    np.testing.assert_allclose([float(v) for v in out[1:]], gold["ew_stats_" + tag], rtol=1e-5, atol=2e-5)
    iy, ix = ew_pixel_index(pts, *mask.shape[1:])
    H, W = mask.shape[1:]
    at = lambda i, v: np.abs(i - v) < 1e-3                                             # (the fp32 points are a few 1e-6 off)
    assert (at(iy, H - 1) & at(ix, W - 1)).any() and (at(iy, 0) & at(ix, 0)).any()    # the corners of the last row and column
    assert ((iy > -1) & (iy < 0)).any() and ((iy > H - 1) & (iy < H)).any()          # half a pixel outside: two taps padded
    assert ((ix > W - 1) & (ix < W)).any() and (tag == "s" or (iy < -1).any())         # and more than a pixel outside (of 640 x 640)
    w = gold["ew_w_" + tag]
    fake = (pts[:, :, 0] == 0) & (pts[:, :, 1] == 0)
    assert fake.sum() == 2 and (w[fake] == 0).all() and ((pts[:, :, 0] == 0) & ~fake).any() and (w[~fake] != 0).sum() >= 16


def test_bev_conditions_and_oracle(gold):
    pts = gold["bev_pts"]
    want = np.zeros((2, 640, 640), np.float32)
    j = gold["bev_nz_idx"].astype(np.int64)
    want[j[0], j[1], j[2]] = 1.0
    assert np.array_equal(radar_ref.extract_bev_from_pts(pts), want)                  # every point, on and off the grid
    iu, iv = bev_pixel_index(pts)
    assert ((iu > -1) & (iu < 0)).any() and ((iv > -1) & (iv < 0)).any()
    assert ((iu > 639) & (iu < 640)).any() and ((iv > 639) & (iv < 640)).any()
    assert (iu == np.round(iu)).any() and (want[:, 320, 320] == 0).all()              # floor and ceil coincide; the centre is cleared
    fl = np.floor(np.stack([iu, iv], -1)).astype(int)
    assert any((fl[0, a] == fl[0, b]).all() for a in range(fl.shape[1]) for b in range(a))   # two points on one pixel
    assert ((np.ceil(iu) == 320) & (np.ceil(iv) == 320) & (iu != 320)).any()         # a point that sends an index to the centre


# ----------------------------------------------------------------------------- refusals on the host
def test_longest_cfar_row_and_shortest_extractor_row(L):
    """R = 13648 does not fit the row buffer; R = 13647 is admitted.  A call that is admitted launches, so the admission is
    shown on the one CFAR entry that checks something after cfar_args (the four entries share it): mmk_cfar_mask_bwd_p stops
    at its missing workspace instead.  tests/test_gpu_radar_edges.py runs R = 13647 through the other entries."""
    null, fake = ctypes.c_void_p(0), ctypes.c_void_p(4096)          # never dereferenced: every call fails on the host before a launch
    R = LAST_R + 1
    assert L.mmk_cfar_mask(fake, 2, 3, R, 50, 5, 89, R - 55, 1.0, 0.09, 1, 10.0, fake, null) == -1
    assert b"does not fit" in L.mmk_last_error()
    assert L.mmk_cfar_mask_bwd(fake, fake, 2, 3, R, 50, 5, 89, R - 55, 1.0, 0.09, 10.0, fake, null) == -1
    assert b"does not fit" in L.mmk_last_error()
    for r, code, text in ((R, -1, b"does not fit"), (LAST_R, -3, b"workspace")):
        assert L.mmk_cfar_mask_bwd_p(fake, fake, 2, 3, r, 50, 5, 89, r - 55, fake, fake, 1, 10.0, fake, fake, fake, null, 0, null) == code
        assert text in L.mmk_last_error()
    assert L.mmk_extract_peaks(fake, 1, 1, 1, 0.5, fake, null, null, 0, 10.0, 4, fake, fake, fake, 1 << 20, null) == -1
    assert b"shape" in L.mmk_last_error()
