"""Test-side restatement of DESIGN.md §3 N1 (exact k-NN PCA normals) in numpy: what ``mmk_knn_normals`` must return.

Distances are the kernel's ``nn_dist`` on the fp32 inputs: fp32 differences, ``fmaf(dy, dy, dx * dx)`` (then
``fmaf(dz, dz, .)``), restated through fp64 (a product of two fp32 values is exact in fp64; the one sum is rounded to
fp64 and then to fp32, which can differ from a single rounding only when the fp64 sum lands within 2^-29 relative of an
fp32 tie -- not on any input of the tests, whose k / k+1 gaps are asserted).  Neighbours: stable sort by (d2, index),
padding rows excluded, radius applied as an fp32 compare.  Centroid, covariance, ``numpy.linalg.eigh`` and the
orientation rule in fp64.

Besides the results, two numbers per point that say how well-posed its answer is:
  * ``knn_gap``: (d_{k+1} - d_k) / d_{k+1} of the squared distances (1 when there is no k+1-th candidate);
  * ``eig_gap``: (lambda_2 - lambda_min) / trace, lambda_2 the second-smallest eigenvalue (0 for a zero trace).
"""
import numpy as np


def nn_dist_f32(pts, q, dim):
    """fp32 squared distances of the rows ``pts`` (M,>=dim) to ``q``, bit for bit as the kernels' nn_dist()."""
    t = pts[:, :dim].astype(np.float32)
    d = t - q[:dim].astype(np.float32)[None, :]                     # fp32 differences
    sq = (d[:, 0] * d[:, 0]).astype(np.float32)                      # dx * dx, rounded
    out = (d[:, 1].astype(np.float64) * d[:, 1].astype(np.float64) + sq.astype(np.float64)).astype(np.float32)
    if dim == 3:
        out = (d[:, 2].astype(np.float64) * d[:, 2].astype(np.float64) + out.astype(np.float64)).astype(np.float32)
    return out


def knn_normals_ref(points, k, dim, max_radius=None, pad_val=None, viewpoint=None):
    """points (M,cols) of ONE cloud -> dict(normals (M,3) f64, curvature (M,), count (M,) int32, nbr_idx (M,k) int32,
    knn_gap (M,), eig_gap (M,))."""
    pts = np.asarray(points, dtype=np.float32)
    M = pts.shape[0]
    pad = np.zeros(M, bool)
    if pad_val is not None and pad_val > 0:
        pad = (np.abs(pts[:, :dim]) >= np.float32(pad_val)).any(axis=1)
    v = np.zeros(3) if viewpoint is None else np.asarray(viewpoint, dtype=np.float32).astype(np.float64)
    valid = np.flatnonzero(~pad)
    normals = np.zeros((M, 3))
    curvature = np.zeros(M)
    count = np.zeros(M, np.int32)
    nbr = np.full((M, k), -1, np.int32)
    knn_gap = np.ones(M)
    eig_gap = np.zeros(M)
    r2 = None if not max_radius or max_radius <= 0 else np.float32(max_radius) * np.float32(max_radius)
    for i in valid:
        d2 = nn_dist_f32(pts[valid], pts[i], dim)
        order = np.lexsort((valid, d2))                              # ascending d2, ties to the lowest index
        if r2 is not None:
            order = order[~(d2[order] > r2)]
        keep = order[:k]
        c = len(keep)
        count[i] = c
        nbr[i, :c] = valid[keep]
        if len(order) > k:
            a, b = float(d2[order[k - 1]]), float(d2[order[k]])
            knn_gap[i] = (b - a) / b if b > 0 else 0.0
        if c < 3:
            continue
        x = pts[valid[keep], :dim].astype(np.float64)
        mean = x.sum(axis=0) / c
        dx = x - mean
        cov = dx.T @ dx / c
        lam, vec = np.linalg.eigh(cov)                               # ascending
        tr = lam.sum()
        eig_gap[i] = (lam[1] - lam[0]) / tr if tr > 0 else 0.0
        n = np.zeros(3)
        n[:dim] = vec[:, 0]
        n /= np.linalg.norm(n)
        if np.dot(n[:dim], v[:dim] - pts[i, :dim].astype(np.float64)) < 0:
            n = -n
        normals[i] = n
        curvature[i] = max(lam[0], 0.0) / tr if tr > 0 else 0.0
    return {"normals": normals, "curvature": curvature, "count": count, "nbr_idx": nbr, "knn_gap": knn_gap, "eig_gap": eig_gap}


def knn_normals_ref_batch(points, k, dim, max_radius=None, pad_val=None, viewpoint=None):
    """(B,M,cols) -> the same dict with a leading batch axis; viewpoint (B,3), (3,) or None."""
    points = np.asarray(points)
    outs = []
    for b in range(points.shape[0]):
        vp = None if viewpoint is None else (np.asarray(viewpoint)[b] if np.asarray(viewpoint).ndim == 2 else viewpoint)
        outs.append(knn_normals_ref(points[b], k, dim, max_radius, pad_val, vp))
    return {key: np.stack([o[key] for o in outs]) for key in outs[0]}


def lattice_line(n=12, x=3.0):
    """n rows (x, j, 0), j = 0..n-1: every neighbourhood lies on the line x = const."""
    return np.stack([np.full(n, x), np.arange(n, dtype=np.float64), np.zeros(n)], axis=1).astype(np.float32)


def lattice_plane(n=8, z=5.0):
    """n*n rows (i, j, z): every neighbourhood lies in the plane z = const."""
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    return np.stack([i.ravel(), j.ravel(), np.full(n * n, z)], axis=1).astype(np.float32)
