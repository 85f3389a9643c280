"""Test-side reference of the polar-aware sampler (radar_utils.extract_weights_polar): a torch restatement of its arithmetic,
written for this project from the operator's definition, evaluated on the CPU from searchsorted, gather, cat and
F.grid_sample(align_corners=True, padding_mode="zeros"), so that autograd yields the gradient in the mask and in the points.
Imports nothing from oracle/ and nothing of the reference."""
import math

import numpy as np
import torch
import torch.nn.functional as F


def azimuth_tables(A, seed):
    """(2, A) fp32, ascending, inside (0, 2 pi): row 0 uniform ((k + 0.5) steps), row 1 encoder-quantised (5600 counts per
    turn) with a wobble of +-0.2 of a step per azimuth."""
    rng = np.random.default_rng(seed)
    k = np.arange(A)
    uniform = (k + 0.5) * (2 * np.pi / A)
    counts = np.round((k + 0.5 + rng.uniform(-0.2, 0.2, A)) * 5600 / A)
    wobbled = counts * (2 * np.pi / 5600)
    az = np.stack([uniform, wobbled]).astype(np.float32)
    assert (np.diff(az, axis=1) > 0).all() and az.min() > 0 and az.max() < 2 * np.pi
    return az


def polar_weights_ref(mask, pc, az, res, interpolate_crossover=True, fix_wobble=True, dtype=torch.float32):
    """weights (B,N) of mask (B,A,R) at the points pc (B,N,>=2) with the azimuth tables az (B,A), and a dict with the
    sampling position (u, v before the crossover row's shift), the clamp of u and the gate of v's interpolation.  Differentiable
    in mask and pc (fake rows get a zero gradient: they are replaced before the arithmetic and masked after it)."""
    mask, pc, az = mask.to(dtype), pc.to(dtype), az.to(dtype)
    B, A, R = mask.shape
    x, y = pc[..., 0], pc[..., 1]
    fake = (x == 0) & (y == 0)
    xs = torch.where(fake, torch.ones_like(x), x)
    rng = torch.sqrt(y * y + xs * xs)
    ang = torch.atan2(y, xs)
    ang = ang + torch.where(ang < 0, 2.0 * math.pi, 0.0).to(dtype)
    u = (rng - res / 2) / res
    if fix_wobble:
        c3 = torch.searchsorted(az.contiguous(), ang.detach().contiguous())       # first i with az[i] >= ang
        c3 = torch.where(c3 == A, c3 - 1, c3)
        c2 = c3 - 1
        c2 = torch.where(c2 < 0, c2 + 1, c2)
        a3, a2 = torch.gather(az, 1, c3), torch.gather(az, 1, c2)
        df = ang - a3
        live = (df < 0) & (c3 > 0)
        delta = ((df * (df < 0).to(dtype)) * (c3 > 0).to(dtype)) / ((a3 - a2) + 1e-14)
        v = c3.to(dtype) + delta
        dv = torch.where(live, 1.0 / ((a3 - a2) + 1e-14), torch.zeros_like(a3))
    else:
        step = (az[:, -1:] - az[:, :1]) / (A - 1)
        v = (ang - az[:, :1]) / step
        live = torch.ones_like(fake)
        dv = (1.0 / step).expand_as(v)
    clamped = u < 0
    u = torch.where(clamped, torch.zeros_like(u), u)
    info = {"u": u.detach(), "v": v.detach(), "clamped": clamped, "gated": ~live, "fake": fake, "rng": rng.detach(), "dv": dv.detach()}
    img = mask
    if interpolate_crossover:
        img = torch.cat([mask[:, -1:], mask, mask[:, :1]], dim=1)
        v = v + 1.0
    rows = img.shape[1]
    gx = u / (R - 1) * 2.0 - 1.0
    gy = v / (rows - 1) * 2.0 - 1.0
    grid = torch.stack([gx, gy], dim=-1).unsqueeze(1)
    w = F.grid_sample(img.unsqueeze(1), grid, mode="bilinear", padding_mode="zeros", align_corners=True)[:, 0, 0]
    return torch.where(fake, torch.zeros_like(w), w), info


def position_error(az):
    """Bound on the error of a sampling position, in cells: sqrtf / atan2f on the device against torch on the host are the only
    arithmetic not shared bit for bit; an angle error of k ulp of 2 pi (2^-21) moves v by k 2^-21 / min_step; k = 16."""
    return 16 * 2.0 ** -21 / float(np.diff(np.asarray(az, dtype=np.float64), axis=1).min())


def tap_counts(info, A, R, wrap, reach=0, select=None):
    """(B,A,R) fp32: how many of the real points (of those in the (B,N) bool ``select``, if given) have the cell inside the
    block of cells from (floor(v) - reach, floor(u) - reach) to (floor(v) + 1 + reach, floor(u) + 1 + reach), rows folded as
    the crossover rows fold them.  reach = 0: the point's four taps as the restatement places them; reach = 1: every cell a
    tap can fall on whatever the last ulp of the position."""
    B, N = info["u"].shape
    count = torch.zeros(B, A, R)
    u0, v0 = torch.floor(info["u"].double()).long(), torch.floor(info["v"].double()).long()
    for b in range(B):
        real = ~info["fake"][b] if select is None else (~info["fake"][b] & select[b])
        for dr in range(-reach, 2 + reach):
            r = v0[b][real] + dr
            r = torch.remainder(r, A) if wrap else r
            for dc in range(-reach, 2 + reach):
                c = u0[b][real] + dc
                ok = (r >= 0) & (r < A) & (c >= 0) & (c < R)
                count[b].index_put_((r[ok], c[ok]), torch.ones(int(ok.sum())), accumulate=True)
    return count
