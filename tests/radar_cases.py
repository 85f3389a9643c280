"""What several radar and policy test files share: the range resolution, the 64 x 64 scan-mode scene, non-uniform azimuths, the
golden chain's inputs, the CFAR parameter sets and the cases and fp64 restatement of the learnable GO-CFAR thresholds -- a
module of the tests, not a test.  Nothing here touches a device at import; ``scene64`` does when a test requests it.

The restatement (``threshold_grads_f64``, for shapes that have no golden value):
    ga = - sum over the kept cells c of [mincol, maxcol) of k_c stat_c,      gb = - sum of k_c,
    k_c = G_c 0.5 steep (1 - t_c^2),  t_c = tanh(steep (x_c - a stat_c - b) + 2.5),  stat_c = max(left_c, right_c) / w2,
with kept_c = (0.5 t_c + 0.5 > 0.99), as autograd takes them through radar_utils.py:56-65 of the reference.  Its scale is the
same sum with |G|: every term then has one sign.
"""
import math
import os
import sys

import numpy as np
import pytest
import torch

from support import DEV, load_golden

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from make_golden_radar_grads import cfar_terms  # noqa: E402

RES = 0.0596


def wobbly_azimuths(seed):
    """One ascending table of 400 azimuths that is far from uniform: steps between 0.2 and 1.8 of the mean step."""
    g = torch.Generator().manual_seed(seed)
    steps = (0.2 + 1.6 * torch.rand(400, generator=g, dtype=torch.float64)) * (2 * math.pi / 400)
    az = 0.004 + torch.cumsum(steps, 0) * (2 * math.pi - 0.02) / steps.sum()
    return az[None]


def cfar_kw(gold, tag):
    """cfar_mask keywords of parameter set ``tag`` of radar_grads.npz (0: the defaults)."""
    if tag == 0:
        return {}
    w, g, s, a, b = gold["ca_params1"]
    return {"width": int(w), "guard": int(g), "steep_fact": float(s), "a_thresh": float(a), "b_thresh": float(b)}


def chain_inputs(golden_dir):
    """The golden chain's inputs: radar_grads.npz's scan with resample_grads.npz's changes applied, and the mask factors."""
    base, rg = load_golden(golden_dir, "radar_grads.npz"), load_golden(golden_dir, "resample_grads.npz")
    raw = base["ch_raw"].copy()
    raw.reshape(-1)[rg["ch_fix_idx"]] = rg["ch_fix_val"]
    return {"raw": raw, "az": base["ch_az"], "map": base["ch_map"], "G": base["ch_G"], "npad": int(base["ch_npad"]),
            "iters": int(base["ch_iters"]), "cu": rg["ch_cu"], "cv": rg["ch_cv"]}


# ----------------------------------------------------------------------------- the policy at 64 x 64
B64, H64, A64, R64, NP64 = 2, 64, 32, 200, 128


@pytest.fixture(scope="module")
def scene64():
    """A 32 x 200 polar scan whose only detections lie between GO-CFAR's first column (89) and the edge of a 64 x 64 Cartesian
    image (range cell 128 on the axes, 181 in the corners): one three-cell blob per azimuth at cells 95..122, the map = the
    blob centres moved by a small rigid offset, with radial normals."""
    from mm_masking_amd import radar_utils as ru
    g = torch.Generator().manual_seed(11)
    az = ((torch.arange(A64, dtype=torch.float64) + 0.5) * (2 * math.pi / A64))[None].repeat(B64, 1)
    az = az + 0.02 * (torch.rand(B64, A64, generator=g, dtype=torch.float64) - 0.5)
    polar = 0.02 * torch.rand(B64, A64, R64, generator=g)
    col = torch.zeros(B64, A64, dtype=torch.long)
    for b in range(B64):
        for a in range(A64):
            c = 95 + (7 * a + 13 * b) % 28
            col[b, a] = c
            polar[b, a, c - 1:c + 2] = torch.tensor([0.55, 0.7, 0.55])
    rho = (col.double() * RES).float()
    x, y = rho * torch.cos(az.float()), rho * torch.sin(az.float())
    nrm = torch.stack((torch.cos(az.float()), torch.sin(az.float()), torch.zeros(B64, A64)), dim=2)
    pts = torch.stack((x + 0.10, y - 0.06, torch.zeros(B64, A64)), dim=2)
    map_pc = torch.cat((torch.cat((pts, nrm), dim=2), torch.cat((pts + 0.03 * nrm, nrm), dim=2)), dim=1)
    polar, azd = polar.to(DEV), az.float().to(DEV)
    raw_pc, cnt = ru.extract_pc_padded(ru.cfar_mask(polar, RES, diff=False), RES, azd, torch.zeros_like(azd), NP64, diff=False)
    assert cnt.min() >= 8 and cnt.max() <= NP64
    scan = {"fft_data": ru.radar_polar_to_cartesian_diff(polar, azd, RES, cart_pixel_width=H64), "fft_cfar": torch.zeros(B64, H64, H64, device=DEV),
            "raw_pc": raw_pc, "filtered_pc": raw_pc, "fft_polar": polar, "azimuths": az}          # azimuths on the host: no sync
    return scan, {"pc": map_pc.to(DEV)}, torch.eye(4, device=DEV).repeat(B64, 1, 1), torch.randn(B64, 4, 4, generator=g).to(DEV)


# ----------------------------------------------------------------------------- the learnable GO-CFAR thresholds
CASES = ["0s", "0p", "1s", "1p"]


def load_fixture(golden_dir):
    """cfar_params.npz plus the inputs it shares with radar_grads.npz (the scans with the fixture's own changes applied)."""
    g, base = load_golden(golden_dir, "cfar_params.npz"), load_golden(golden_dir, "radar_grads.npz")
    for pre, src in (("cp", "ca_raw"), ("cc", "ch_raw")):
        raw = base[src].copy()
        raw.reshape(-1)[g[pre + "_fix_idx"]] = g[pre + "_fix_val"]
        g[pre + "_raw"] = raw
    g["cp_G"] = base["ca_G"]
    for k in ("ch_az", "ch_map", "ch_mu", "ch_mv", "ch_G", "ch_npad", "ch_iters", "ca_grad0", "ca_grad1"):
        g[k] = base[k]
    return g


def geom_of(gold, key):
    """Window geometry and steepness of a case's parameter set, as cfar_mask keywords."""
    if key[0] == "0":
        return {}
    w, g, s = gold["cp_geom1"]
    return {"width": int(w), "guard": int(g), "steep_fact": float(s)}


def per_scan_values(gold, key, B):
    """The thresholds of a case as (B,) fp64 arrays holding the stored fp32 numbers."""
    a, b = gold["cp_a" + key], gold["cp_b" + key]
    return np.broadcast_to(a.astype(np.float64), (B,)), np.broadcast_to(b.astype(np.float64), (B,))


def threshold_grads_f64(raw, G, a, b, res=RES, **geom):
    """(ga, gb) per scan in fp64 for the scans ``raw`` (B,A,R) with per-scan thresholds ``a``, ``b`` (B,).  m_raw, the column
    range and the gate come from the generator's cfar_terms; the window statistic is formed here in fp64."""
    B = raw.shape[0]
    ga, gb = np.zeros(B), np.zeros(B)
    G = np.asarray(G, dtype=np.float64)
    steep = float(geom.get("steep_fact", 10.0))
    for i in range(B):
        m_raw, _, _, (w2, guard, mincol, maxcol) = cfar_terms(raw[i], res=res, a_thresh=float(a[i]), b_thresh=float(b[i]), **geom)
        x = raw[i].astype(np.float64)
        R = x.shape[-1]
        cs = np.concatenate([np.zeros(x.shape[:-1] + (1,)), np.cumsum(x, axis=-1)], axis=-1)
        c = np.arange(mincol, maxcol)
        left = cs[..., c - guard] - cs[..., c - w2 - guard]
        right = cs[..., np.minimum(R, c + w2 + guard + 1)] - cs[..., np.minimum(R, c + guard + 1)]
        stat = np.maximum(left, right) / w2
        t = 2.0 * m_raw[..., c] - 1.0
        k = np.where(m_raw[..., c] > 0.99, G[i][..., c] * 0.5 * steep * (1.0 - t * t), 0.0)
        ga[i], gb[i] = -(k * stat).sum(), -k.sum()
    return ga, gb
