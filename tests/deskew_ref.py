"""The CPU restatement of the motion compensation and of the per-point times, and the cases the CPU and the
GPU test of the operator share -- a module of the tests, not a test; only test_deskew_cpu.py and test_gpu_deskew.py import it.
Nothing here touches a device.

``deskew_ref`` is the normative arithmetic in fp64 torch with plain autograd: per point, from the fp32 inputs,
    w = s omega, u = s v, th2 = w.w, A = sin th / th, B = (1 - cos th) / th2, C = (th - sin th) / th^3
    (th2 < 1e-4: their Taylor series to th^6), p' = p + A (w x p) + B w x (w x p) + u + B (w x u) + C w x (w x u),
a row of the cloud that is exactly (0, 0, 0) being padding (output 0, no gradient).  The caller rounds to fp32.

``point_times_ref`` restates the marker pairing of the reference's extract_pc (radar_utils.py:88-97) in numpy and keeps the
third column of its pair mean: the time of point k is (times[row of marker 2k+1] + times[row of marker 2k]) / 2 in fp32.
"""
import numpy as np
import torch

SERIES_CUT = 1e-4


def _cross(a, b):
    ax, ay, az = a.unbind(-1)
    bx, by, bz = b.unbind(-1)
    return torch.stack((ay * bz - az * by, az * bx - ax * bz, ax * by - ay * bx), dim=-1)


def coefficients(th2):
    """(A, B, C) of th2 (fp64): the series below the cut, the closed forms above it."""
    small = th2 < SERIES_CUT
    x = torch.where(small, th2, torch.zeros_like(th2))
    x2 = x * x
    x3 = x2 * x
    As = ((1.0 - x / 6.0) + x2 / 120.0) - x3 / 5040.0
    Bs = ((0.5 - x / 24.0) + x2 / 720.0) - x3 / 40320.0
    Cs = ((1.0 / 6.0 - x / 120.0) + x2 / 5040.0) - x3 / 362880.0
    y = torch.where(small, torch.ones_like(th2), th2)              # (the unused branch stays finite, and so does its gradient)
    th = torch.sqrt(y)
    s, c = torch.sin(th), torch.cos(th)
    return (torch.where(small, As, s / th), torch.where(small, Bs, (1.0 - c) / y), torch.where(small, Cs, (th - s) / (y * th)))


def deskew_ref(pc, t, twist):
    """p' (B,N,3) fp64 of pc (B,N,3), t (B,N) and twist (B,6) -- or (B,N,6), one copy of the twist per point, whose gradient
    then holds every point's own share of the twist's.  Inputs: fp64 tensors (holding fp32 values), any of which may
    require grad."""
    tw = twist if twist.ndim == 3 else twist[:, None, :]
    s = t[..., None]
    u, w = s * tw[..., :3], s * tw[..., 3:]
    A, B, C = (k[..., None] for k in coefficients((w * w).sum(-1)))
    a1 = _cross(w, pc)
    a2 = _cross(w, a1)
    b1 = _cross(w, u.expand_as(pc))
    b2 = _cross(w, b1)
    out = ((((pc + A * a1) + B * a2) + u) + B * b1) + C * b2
    pad = (pc.detach() == 0).all(-1, keepdim=True)
    return torch.where(pad, torch.zeros_like(out), out)


def f64(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float32).astype(np.float64))


def deskew_ref_grads(pc, t, twist, G):
    """(out, grad_pc, grad_twist, terms) in fp64 numpy for fp32 numpy inputs: terms (B,N,6) are the points' shares
    s_i (u_bar_i; w_bar_i), grad_twist their sum over the points."""
    p = f64(pc).requires_grad_(True)
    tw = f64(twist)[:, None, :].expand(-1, p.shape[1], -1).clone().requires_grad_(True)
    out = deskew_ref(p, f64(t), tw)
    out.backward(f64(G))
    terms = tw.grad.numpy()
    return out.detach().numpy(), p.grad.numpy(), terms.sum(1), terms


def matrix_exp_ref(pc, t, twist):
    """Exp(t_i twist) p_i through torch.linalg.matrix_exp of the 4x4 twist matrix, fp64 (no padding rule)."""
    B, N = t.shape
    xi = t[..., None] * twist[:, None, :]                          # (B,N,6)
    v, w = xi[..., :3], xi[..., 3:]
    M = torch.zeros(B, N, 4, 4, dtype=torch.float64)
    M[..., 0, 1], M[..., 0, 2], M[..., 1, 2] = -w[..., 2], w[..., 1], -w[..., 0]
    M[..., 1, 0], M[..., 2, 0], M[..., 2, 1] = w[..., 2], -w[..., 1], w[..., 0]
    M[..., :3, 3] = v
    E = torch.linalg.matrix_exp(M)
    return (E[..., :3, :3] @ pc[..., None])[..., 0] + E[..., :3, 3]


# ----------------------------------------------------------------------------- the operator's cases
# name -> the twist (v; omega) of an item.  With |s| <= 0.125 s the series cut th = 0.01 lies at |s| = 0.01 / |omega|:
#   sixdof  |omega| = 0.31: points on both sides of the cut        planar  the same in the plane
#   fast    |omega| = 3.1:  th up to 0.39, nearly every point above the cut
#   slow    |omega| = 0.05: th <= 0.00625, every point below the cut
TWISTS = {"sixdof": (12.0, 0.5, -0.3, 0.05, -0.04, 0.3), "planar": (12.0, 0.5, 0.0, 0.0, 0.0, 0.3), "zero": (0.0,) * 6,
          "fast": (-4.0, 7.0, 0.6, 1.0, -0.8, 2.8), "slow": (3.0, -9.0, 0.2, 0.03, 0.02, -0.035)}
SHAPES = [(B, N) for B in (1, 3) for N in (1, 63, 64, 65, 256, 257, 1000)] + [(32, 5120)]
KINDS = ["sixdof", "planar", "zero", "fast", "slow", "mixed"]


def operator_case(B, N, kind, seed=0):
    """fp32 numpy (pc, t, twist, G).  ``mixed``: the items cycle through the five twists.  Planar items lie in z = 0.  Rows
    N // 3 and N // 2 of every item are interior zero (padding) rows when N >= 8, and t holds an exact 0 at row N // 4."""
    rng = np.random.default_rng([seed, B, N, KINDS.index(kind)])
    names = [kind] * B if kind != "mixed" else [list(TWISTS)[b % len(TWISTS)] for b in range(B)]
    twist = np.array([TWISTS[n] for n in names], dtype=np.float32)
    pc = rng.uniform(-70.0, 70.0, (B, N, 3)).astype(np.float32)
    pc[:, :, 2] = rng.uniform(-1.0, 1.0, (B, N)).astype(np.float32)
    for b, n in enumerate(names):
        if n == "planar":
            pc[b, :, 2] = 0.0
    t = rng.uniform(-0.125, 0.125, (B, N)).astype(np.float32)
    if N >= 8:
        pc[:, N // 3] = 0.0
        pc[:, N // 2] = 0.0
        t[:, N // 4] = 0.0
    G = rng.normal(0.0, 1.0, (B, N, 3)).astype(np.float32)
    return pc, t, twist, G


# ----------------------------------------------------------------------------- the per-point times
def point_times_ref(mask, times, res, max_pts, diff=False, steep_fact=10.0):
    """(t (B,max_pts) fp32, cnt (B,) int) of the masks (B,A,R) and the row times (B,A): markers where
    mean_peaks_parallel_fast of res * j * mask is not 0 (radar_utils.py:74,167-185), in row-major order (nonzero, :88),
    paired (2k, 2k+1) -- the unpaired last marker of an odd count is dropped, as the kernels drop it -- and the pair's two
    row times averaged in fp32 (:97).  cnt counts the pairs; rows at or beyond it, and pairs beyond max_pts, give 0."""
    mask = np.asarray(mask, dtype=np.float32)
    times = np.asarray(times, dtype=np.float32)
    B, A, R = mask.shape
    arr = (np.float32(res) * np.arange(R).astype(np.float32))[None, None, :] * mask
    z = (np.float32(1.0) - np.tanh(np.float32(steep_fact) * arr)) if diff else (arr == 0).astype(np.float32)
    peaks = np.zeros_like(arr)
    peaks[:, :, :-1] = arr[:, :, :-1] * z[:, :, 1:] + arr[:, :, 1:] * z[:, :, :-1]
    out, cnt = np.zeros((B, max_pts), dtype=np.float32), np.zeros(B, dtype=np.int64)
    for b in range(B):
        nz = np.nonzero(peaks[b].reshape(-1))[0]
        n = len(nz) // 2
        even, odd = nz[0:2 * n:2], nz[1:2 * n:2]
        tk = (times[b][odd // R] + times[b][even // R]) / np.float32(2.0)
        cnt[b] = n
        out[b, :min(n, max_pts)] = tk[:max_pts]
    return out, cnt
