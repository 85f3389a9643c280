"""What tests/test_radar_edges_cpu.py and tests/test_gpu_radar_edges.py share: the case tables of tests/golden/radar_edges.npz,
the fixture conditions of its generator, the conditioned CFAR scans of the launch classes and of the persistent walk, and the
fp64 restatement of the CFAR scan gradient -- a module of the tests, not a test.  Nothing here touches a device.

The restatement (``cfar_scan_grad_f64``, in radar_cases.threshold_grads_f64's notation): with k_c, t_c and stat_c as there,
kL_c = k_c where the left window of c won, kR_c = k_c where the right one did (half of k_c in both on an exact tie),
    gx_i = k_i - (a / w2) (sum of kL_c over c in [i + g + 1, i + w2 + g + 1)  +  sum of kR_c over c in [i - w2 - g, i - g)),
the ranges cut to [0, R): cell i lies in the left window of the former cells and in the right window of the latter.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from make_golden_radar_edges import (CF_RES, EW_MASKS, PC_CASES, PC_TABLES, PC_VARIANTS, PX, assert_cfar_conditions,  # noqa: E402,F401
                                     assert_peak_conditions, assert_table_conditions, bev_pixel_index, cf_sets, ew_mask,
                                     ew_pixel_index, marker_counts, nudge_cfar, off_grid, pixel_range_angle)
from make_golden_radar_grads import CFAR_SETS, cfar_terms  # noqa: E402,F401
from radar_cases import RES  # noqa: E402

PEAK_HARD = ("pk0", "pk1", "pk2", "pk3", "pk4", "pk5")
PEAK_SOFT = ("pks",)
SOFT_STEEP = 10.0

# CFAR launch classes: a short row | 3412, 3413 either side of the persistent kernel's 40 KB of LDS | 4097 the backward's first
# row beyond eight cells per thread | 5461 the first row whose 12 R + 8 bytes need the raised dynamic-LDS limit | 13647 the last
# row cfar_args admits
LAUNCH_R = (600, 3412, 3413, 4097, 5461, 13647)
GRAD_R = (5461, 13647)
LAST_R = 13647
WALK_SHAPE = (6, 200, 256)
WALK_PAIRS = ((1.0, 0.09), (1.2, 0.12), (0.8, 0.07), (1.5, 0.05), (0.6, 0.15), (1.1, 0.10))


def peak_case(gold, name):
    """A case of the fixture as extract_pc's arguments: the mask as fp32, the tables, the poses and the stored clouds."""
    c = {k: gold["%s_%s" % (name, k)] for k in ("mask", "az", "tm", "T_ab", "nmark", "n")}
    c["mask"], c["res"], c["diff"] = c["mask"].astype(np.float32), float(gold[name + "_res"]), name in PEAK_SOFT
    for k in ("pc", "pcT"):
        c[k] = gold.get("%s_%s" % (name, k))
    return c


def marker_rows(mask, res, diff):
    """Per item, the azimuth row of every marker in the reference's order (flattened azimuth-major)."""
    _, v = marker_counts(mask, res, diff, SOFT_STEEP)
    return [np.nonzero(v[b])[0] for b in range(mask.shape[0])]


def point_times(mask, res, diff, tm):
    """Per item, the fp32 expression (t1 + t0) / 2 of every marker pair; a last unpaired marker gives no point."""
    out = []
    for b, rows in enumerate(marker_rows(mask, res, diff)):
        rows = rows[:2 * (len(rows) // 2)]
        out.append((tm[b][rows[1::2]] + tm[b][rows[0::2]]) / np.float32(2.0))
    return out


def conditioned_scan(seed, shape, res, sets, step=37):
    """test_gpu_cfar_params._conditioned_scan's noise and three-cell returns, here across the whole row up to its last window,
    changed by the generator's nudge_cfar() until every fixture condition holds under every keyword set of ``sets``."""
    rng = np.random.default_rng(seed)
    raw = rng.random(shape, dtype=np.float32) * np.float32(0.04)
    for c in range(150 % step + step, shape[2] - 3, step):
        raw[:, :, c:c + 3] += rng.uniform(0.1, 0.4, shape[:2] + (3,)).astype(np.float32)
    return nudge_cfar(raw, res, sets)


def launch_scan(R):
    """(raw (2, 3, R), keywords): maxr = R res, so that the windows of the last cells of [mincol, maxcol) reach the row's end."""
    kw = {"maxr": R * RES}
    return conditioned_scan(500 + R, (2, 3, R), RES, (kw,)), kw


def walk_scan():
    """(raw (6, 200, 256) at res 0.5, one keyword set per scan): six different threshold pairs, minr = 0 and maxr = 1e6 so that
    the column range runs from w2 + guard + 1 to the row's end."""
    sets = [{"minr": 0.0, "maxr": 1e6, "a_thresh": a, "b_thresh": b} for a, b in WALK_PAIRS]
    rng = np.random.default_rng(77)
    raw = rng.random(WALK_SHAPE, dtype=np.float32) * np.float32(0.04)
    for c in range(10, WALK_SHAPE[2] - 3, 23):
        raw[:, :, c:c + 3] += rng.uniform(0.1, 0.4, WALK_SHAPE[:2] + (3,)).astype(np.float32)
    for i, kw in enumerate(sets):                                   # each scan is conditioned under its own pair
        raw[i:i + 1] = nudge_cfar(raw[i:i + 1], CF_RES, (kw,))
    return raw, sets


def cfar_scan_grad_f64(raw, G, res, **kw):
    """Gradient of sum(mask * G) with respect to the scan in fp64 (see the module docstring); the gate comes from the fp64
    m_raw, the winner from the fp32-rounded window sums, as the fixture conditions make both safe."""
    m_raw, left, right, (w2, guard, mincol, maxcol) = cfar_terms(raw, res=res, **kw)
    steep, a = float(kw.get("steep_fact", 10.0)), float(kw.get("a_thresh", 1.0))
    R = raw.shape[-1]
    t = 2.0 * m_raw - 1.0
    k = np.where(m_raw > 0.99, np.asarray(G, dtype=np.float64) * 0.5 * steep * (1.0 - t * t), 0.0)
    inr = np.zeros(R, bool)
    inr[mincol:maxcol] = True
    with np.errstate(invalid="ignore"):
        kL = np.where(inr & (left > right), k, np.where(inr & (left == right), 0.5 * k, 0.0))
        kR = np.where(inr & (right > left), k, np.where(inr & (left == right), 0.5 * k, 0.0))
    zero = np.zeros(raw.shape[:-1] + (1,))
    PL, PR = (np.concatenate([zero, np.cumsum(v, axis=-1)], axis=-1) for v in (kL, kR))
    i = np.arange(R)
    sl = PL[..., np.minimum(R, i + w2 + guard + 1)] - PL[..., np.minimum(R, i + guard + 1)]
    sr = PR[..., np.maximum(0, i - guard)] - PR[..., np.maximum(0, i - w2 - guard)]
    return k - (a / w2) * (sl + sr)


def beyond_range(W, R, res):
    """Pixels of the W x W image whose every tap is zero padding: the range coordinate u = rng / res - 0.5 of
    radar_utils.py:288 is at least R, with a margin of 1e-3 bins; and the pixels one bin inside that edge, u in [R - 1, R),
    which keep the tap of the last bin alone."""
    rng, _ = pixel_range_angle(W)
    u = rng / res - 0.5
    return u > R + 1e-3, (u > R - 1 + 1e-3) & (u < R - 1e-3)
