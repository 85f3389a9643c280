"""Target normals for point-to-plane ICP, estimated on the device.

``estimate_normals`` is the exact k-nearest-neighbour PCA of DESIGN.md §3 (N1): for every row of a cloud the k nearest
valid rows of the same cloud (the ICP's own distance and tie rule, through the ICP's uniform grid), the eigenvector of
the smallest eigenvalue of their covariance, turned towards a viewpoint.  It produces the normals columns of the map
tensor (mm_masking/icp_weight_dataset.py:395-398), which upstream come out of vtr3 pose graphs.  The arithmetic runs in
``knn_normals_kernel`` of csrc/mmk_icp.hip through ``mmk_knn_normals`` (include/mmk.h); this file only owns buffers.

No gradient: the normals are constants, as the map is.
"""
import torch

from .. import _lib


def _check_args(points, k, dim):
    if points.ndim != 3:
        raise ValueError("points must be (B,M,cols)")
    if dim not in (2, 3):
        raise ValueError("dim must be 2 or 3 (got %r)" % (dim,))
    if int(k) != k or not 3 <= int(k) <= 32:
        raise ValueError("k must be in 3..32 (got %r)" % (k,))
    if points.shape[-1] < dim:
        raise ValueError("points has %d columns, dim = %d needs at least %d" % (points.shape[-1], dim, dim))
    if points.shape[0] < 1 or points.shape[1] < 1:
        raise ValueError("points must hold at least one cloud of at least one row")


def estimate_normals(points, k=16, dim=3, max_radius=None, pad_val=None, viewpoint=None, return_info=False):
    """Normals (B,M,3) fp32 of ``points`` (B,M,cols >= dim), on the input's device.

    ``k`` in 3..32 neighbours (the row itself included); ``max_radius`` drops neighbours farther away; rows with a
    |coordinate| >= ``pad_val`` are padding (never neighbours, zero outputs); ``viewpoint`` (B,3) or (3,) is what the
    normals face (default: the origin).  Rows with fewer than 3 neighbours get the zero normal, which is inert in
    pt2pl.  ``return_info``: also ``curvature`` (B,M) fp32 = lambda_min / sum(lambda), ``count`` (B,M) int32 and
    ``nbr_idx`` (B,M,k) int32 in (distance, index) order, -1 in unused slots.
    """
    _check_args(points, k, dim)
    if not points.is_cuda:
        raise _lib.MmkError("estimate_normals needs an MI355X/HIP device: the k-NN PCA is a HIP kernel with no CPU path")
    L = _lib.lib()
    dev = points.device
    pts = _lib.dev_f32(points, dev)
    B, M, cols = pts.shape
    vp = None
    if viewpoint is not None:
        vp = torch.as_tensor(viewpoint, dtype=torch.float32).to(dev)
        if vp.ndim == 1:
            vp = vp.reshape(1, 3).expand(B, 3)
        if tuple(vp.shape) != (B, 3):
            raise ValueError("viewpoint must be (B,3) or (3,)")
        vp = vp.contiguous()
    normals = torch.empty(B, M, 3, dtype=torch.float32, device=dev)
    curv = cnt = nbr = None
    if return_info:
        curv = torch.empty(B, M, dtype=torch.float32, device=dev)
        cnt = torch.empty(B, M, dtype=torch.int32, device=dev)
        nbr = torch.empty(B, M, int(k), dtype=torch.int32, device=dev)
    ws = torch.empty(int(L.mmk_knn_normals_workspace_bytes(B, M)), dtype=torch.uint8, device=dev)
    _lib.check(L.mmk_knn_normals(_lib.ptr(pts, torch.float32, "points"), B, M, cols, int(dim), int(k),
                                 float(max_radius) if max_radius else 0.0, float(pad_val) if pad_val else 0.0,
                                 _lib.ptr(vp), _lib.ptr(normals), _lib.ptr(curv), _lib.ptr(cnt), _lib.ptr(nbr),
                                 _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev)))
    if return_info:
        return normals, curv, cnt, nbr
    return normals


def with_normals(points, **kw):
    """(B,M,6) = xyz | estimated normal: the six-column target of ``ICP('pt2pl').icp``.  Keyword arguments are
    ``estimate_normals``'s.  A cloud with two columns gets z = 0.  The xyz columns are ``points``' own (their gradient
    flows); the normals are constants."""
    kw.pop("return_info", None)
    n = estimate_normals(points.detach(), **kw)
    xyz = points.to(device=n.device, dtype=torch.float32)[..., :3]
    if xyz.shape[-1] < 3:
        xyz = torch.cat((xyz, torch.zeros(xyz.shape[:-1] + (3 - xyz.shape[-1],), dtype=xyz.dtype, device=xyz.device)), dim=-1)
    return torch.cat((xyz, n), dim=-1)
