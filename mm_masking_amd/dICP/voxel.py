"""Voxel-grid downsampling of point clouds on the device.

``voxel_downsample`` is V1 of DESIGN.md §3: one output row per occupied cell of a uniform grid of edge ``voxel``, in the
order in which the cells first appear in the cloud, either the centroid of the cell's rows (every column, the normals
re-normalised) or a copy of its first row.  It is the other half of "raw xyz -> ICP target" beside
``normals.estimate_normals``: upstream the maps arrive voxel-filtered from vtr3.  The arithmetic runs in the kernels of
csrc/mmk_cloud.hip through ``mmk_voxel_downsample`` (include/mmk.h); this file only owns buffers.

No gradient: the output is detached.
"""
import math

import numpy as np
import torch

from .. import _lib

MAX_CELLS = 2.0 ** 20          # cells per half axis: pad_val / voxel may not exceed it (three indices pack into one key)


def _check_args(points, voxel, dim, pad_val, max_out, mode, normals):
    """The checked (max_out, normals) of a call; ValueError for anything mmk_voxel_downsample would refuse."""
    if not torch.is_tensor(points) or points.ndim != 3:
        raise ValueError("points must be a (B,M,cols) tensor")
    B, M, cols = points.shape
    if B < 1 or M < 1:
        raise ValueError("points must hold at least one cloud of at least one row")
    if dim not in (2, 3):
        raise ValueError("dim must be 2 or 3 (got %r)" % (dim,))
    if not dim <= cols <= 8:
        raise ValueError("points has %d columns, dim = %d needs between %d and 8" % (cols, dim, dim))
    for name, v in (("voxel", voxel), ("pad_val", pad_val)):
        if isinstance(v, bool) or not isinstance(v, (int, float, np.floating, np.integer)) or not math.isfinite(v) or not v > 0:
            raise ValueError("%s must be a finite number > 0 (got %r)" % (name, v))
    vox32 = np.float32(voxel)
    if not vox32 > 0 or not np.isfinite(np.float32(pad_val)):
        raise ValueError("voxel and pad_val must be fp32 numbers > 0 (got %r, %r)" % (voxel, pad_val))
    inv = np.float32(1.0 / float(vox32))
    if not np.float32(pad_val) * inv <= np.float32(MAX_CELLS):
        raise ValueError("pad_val / voxel = %g exceeds 2^20 cells: use a larger voxel or a smaller pad_val"
                         % (float(pad_val) / float(voxel)))
    if mode not in _lib.VOXEL_MODES:
        raise ValueError("mode must be 'centroid' or 'first' (got %r)" % (mode,))
    if normals is None:
        normals = cols == 6
    if normals not in (True, False, 0, 1):
        raise ValueError("normals must be None, True or False (got %r)" % (normals,))
    if normals and cols < 6:
        raise ValueError("normals=True needs at least 6 columns (xyz | normal), points has %d" % cols)
    if max_out is None:
        max_out = M
    if isinstance(max_out, bool) or int(max_out) != max_out or int(max_out) < 1:
        raise ValueError("max_out must be an integer >= 1 (got %r)" % (max_out,))
    return int(max_out), bool(normals)


def voxel_downsample(points, voxel, dim=3, pad_val=1000.0, max_out=None, mode="centroid", normals=None, return_info=False):
    """``(out, count)``: ``out`` (B,max_out,cols) fp32 and ``count`` (B,) int32, both on the device of ``points``
    (B,M,cols), dim <= cols <= 8.

    A row is valid when all its values are finite and its first ``dim`` coordinates lie inside ``(-pad_val, pad_val)``;
    its cell is ``floor(x * fp32(1 / voxel))`` per coordinate (``dim = 2`` ignores z).  ``out`` holds one row per
    occupied cell in the order of first appearance -- ``mode="centroid"``: the mean of the cell's rows in every column,
    independent of the order of the rows down to the bit; with ``normals`` (default: ``cols == 6``) columns 3..5 are the
    mean normal re-normalised, exactly 0 where it vanishes; ``mode="first"``: a copy of the cell's first row -- followed by
    padding rows of ``pad_val``.  ``count`` is the number of occupied cells and stays on the device (nothing
    synchronises); it may exceed ``max_out`` (default M), the first ``max_out`` cells are then kept.  ``return_info``: also
    ``n`` (B,max_out) int32 members per output row (0 in padding), ``first`` (B,max_out) int32 lowest member index (-1)
    and ``voxel_of`` (B,M) int32 rank of every row's cell (-1 for padding rows; ranks >= max_out are reported too).
    """
    max_out, normals = _check_args(points, voxel, dim, pad_val, max_out, mode, normals)
    if not points.is_cuda:
        raise _lib.MmkError("voxel_downsample needs an MI355X/HIP device: the voxel filter is a HIP kernel with no CPU path")
    L = _lib.lib()
    dev = points.device
    pts = _lib.dev_f32(points, dev)
    B, M, cols = pts.shape
    out = torch.empty(B, max_out, cols, dtype=torch.float32, device=dev)
    count = torch.empty(B, dtype=torch.int32, device=dev)
    n = first = voxel_of = None
    if return_info:
        n = torch.empty(B, max_out, dtype=torch.int32, device=dev)
        first = torch.empty(B, max_out, dtype=torch.int32, device=dev)
        voxel_of = torch.empty(B, M, dtype=torch.int32, device=dev)
    ws = torch.empty(int(L.mmk_voxel_downsample_workspace_bytes(B, M, cols, max_out)), dtype=torch.uint8, device=dev)
    _lib.check(L.mmk_voxel_downsample(_lib.ptr(pts, torch.float32, "points"), B, M, cols, int(dim), float(voxel), float(pad_val),
                                      _lib.VOXEL_MODES[mode], int(normals), max_out, _lib.ptr(out), _lib.ptr(count), _lib.ptr(n),
                                      _lib.ptr(first), _lib.ptr(voxel_of), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev)))
    if return_info:
        return out, count, n, first, voxel_of
    return out, count
