"""Test-side restatement of the voxel filter in numpy, written from the specification alone: the cell of
a row is the fp32 product x * fp32(1 / voxel) floored, the occupied cells are kept in a dictionary in row order (so the
output order is the order of first appearance), means are fp64 and the mean normal is re-normalised in fp64.  The GPU
tests (test_gpu_voxel.py) compare mmk_voxel_downsample with it; test_voxel_cpu.py pins its known answers."""
import numpy as np


def cell_inverse(voxel):
    """What the host forms once: (float)(1.0 / (double)voxel), voxel an fp32 number."""
    return np.float32(1.0 / float(np.float32(voxel)))


def valid_rows(points, dim, pad_val):
    p = np.asarray(points, np.float32)
    return np.isfinite(p).all(axis=1) & (np.abs(p[:, :dim]) < np.float32(pad_val)).all(axis=1)


def voxel_ref(points, voxel, dim=3, pad_val=1000.0, max_out=None, mode="centroid", normals=None):
    """One cloud (M,cols) -> dict: ``count`` (occupied cells), ``out`` (max_out,cols) fp64 (centroid: the fp64 means, the
    normal columns divided by their fp64 length, 0 where it is 0; first: the first member's fp32 values; pad_val in the
    rows from min(count, max_out) on), ``n`` and ``first`` (max_out,), ``voxel_of`` (M,), ``vmax`` (the largest |value| of a
    valid row, what the fixed-point resolution is relative to)."""
    p = np.ascontiguousarray(points, np.float32)
    M, cols = p.shape
    max_out = M if max_out is None else int(max_out)
    normals = (cols == 6) if normals is None else bool(normals)
    valid = valid_rows(p, dim, pad_val)
    cells = np.floor(p[:, :dim] * cell_inverse(voxel))              # fp32 product, fp32 floor
    rank, members = {}, []
    voxel_of = np.full(M, -1, np.int32)
    for i in np.nonzero(valid)[0]:
        key = tuple(int(c) for c in cells[i])
        r = rank.get(key)
        if r is None:
            r = rank[key] = len(members)
            members.append([])
        members[r].append(int(i))
        voxel_of[i] = r
    out = np.full((max_out, cols), float(np.float32(pad_val)), np.float64)
    n = np.zeros(max_out, np.int32)
    first = np.full(max_out, -1, np.int32)
    for r, rows in enumerate(members[:max_out]):
        n[r], first[r] = len(rows), rows[0]
        if mode == "first":
            out[r] = p[rows[0]].astype(np.float64)
            continue
        out[r] = p[rows].astype(np.float64).sum(axis=0) / len(rows)
        if normals:
            length = np.sqrt((out[r, 3:6] ** 2).sum())
            out[r, 3:6] = out[r, 3:6] / length if length > 0 else 0.0
    vmax = float(np.abs(p[valid]).max()) if valid.any() else 0.0
    return {"count": len(members), "out": out, "n": n, "first": first, "voxel_of": voxel_of, "vmax": vmax}


def voxel_ref_batch(points, voxel, **kw):
    """(B,M,cols) -> the dictionary of voxel_ref with a leading batch axis."""
    res = [voxel_ref(p, voxel, **kw) for p in points]
    return {k: np.stack([np.asarray(r[k]) for r in res]) for k in res[0]}
