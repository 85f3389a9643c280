"""CPU restatement of the dICP with soft correspondences (DESIGN.md §3 I2', I3''', I7''') -- a module of the tests, not a test.

``knn_ref`` is I2' in numpy: the k target rows with the smallest I2 distance to a transformed source point, in key order
(ascending d, ties to the lowest index), with the distance expression of tests/knn_normals_ref.py (``nn_dist_f32``: the
kernels' fmaf form, bit for bit).  No row is special: ``target_pad_val`` rows are simply far away.

``soft_rows`` is I3''': per point, in the dtype of the clouds (fp32 normative: torch rounds every operation on its own),

    d_j = I2's expression, recomputed from the rows;  e_j = exp(-(d_j - d_0) / tau);  S = sum_j e_j in slot order;
    a_j = e_j / S;  row~ = sum_j a_j row_j in slot order (xyz; for pt2pl the normal columns too, NOT renormalised).

The fused multiply-add of I2 is restated through fp64 (a product of two fp32 values is exact there; the sum is rounded to
fp64 and then to fp32 -- the caveat of tests/knn_normals_ref.py), and stays differentiable; in fp64 it is the plain
expression.

``ICPSoftminRef`` is tests/dicp_soft_trim_ref.py's ICPSoftRef with the k-NN and the virtual row: the same loop around the
oracle's helpers (transform_points, normal_equations, solve_spd, se_exp) and that module's per_point_terms, which reads the
virtual rows as a target of one row per point.  ``fixed_idx`` (K,B,N,k) replays neighbours; autograd through it is the
reference of the hand-derived backward (which k rows are the neighbours is a constant there too).  ``hist`` carries per
iteration ``idx`` (B,N,k), ``a`` (B,N,k), ``d`` (B,N,k), and ICPSoftRef's ``keep`` / ``huber_out``.
"""
import numpy as np
import torch

from oracle.dicp_ref import normal_equations, se_exp, solve_spd, transform_points

from dicp_soft_trim_ref import per_point_terms
from knn_normals_ref import nn_dist_f32


def knn_ref(p, tgt, k, dim):
    """p (N,dim) fp32 queries, tgt (M,>=dim) -> idx (N,k) int64, d2 (N,k) fp32, in key order."""
    p = np.asarray(p, dtype=np.float32)
    tgt = np.asarray(tgt, dtype=np.float32)
    rows = np.arange(tgt.shape[0])
    idx = np.zeros((p.shape[0], k), np.int64)
    d2 = np.zeros((p.shape[0], k), np.float32)
    for i in range(p.shape[0]):
        d = nn_dist_f32(tgt, p[i], dim)
        order = np.lexsort((rows, d))[:k]                      # ascending d, ties to the lowest index
        idx[i], d2[i] = order, d[order]
    return idx, d2


def knn_ref_batch(p, tgt, k, dim):
    out = [knn_ref(p[b], tgt[b], k, dim) for b in range(p.shape[0])]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def _dist(Q, P, dim):
    """I2's expression for coordinate lists Q[c] (B,N,k) and P[c] (B,N,1), differentiable."""
    dt = Q[0].dtype
    dx, dy = Q[0] - P[0], Q[1] - P[1]
    if dt == torch.float32:
        d = (dy.double() * dy.double() + (dx * dx).double()).float()
        if dim == 3:
            dz = Q[2] - P[2]
            d = (dz.double() * dz.double() + d.double()).float()
        return d
    d = dy * dy + dx * dx
    if dim == 3:
        dz = Q[2] - P[2]
        d = dz * dz + d
    return d


def soft_rows(tgt, P, idx, tau, dim, with_normals):
    """tgt (B,M,cols), P list of dim (B,N) coordinates, idx (B,N,k) -> virtual rows (B,N,6), a (B,N,k), d (B,N,k)."""
    dt = tgt.dtype
    B, N, k = idx.shape
    flat = idx.reshape(B, N * k).long()
    cols = list(range(dim)) + ([3 + c for c in range(dim)] if with_normals else [])
    G = {c: torch.gather(tgt[..., c], 1, flat).reshape(B, N, k) for c in cols}
    d = _dist([G[c] for c in range(dim)], [P[c].unsqueeze(-1) for c in range(dim)], dim)
    e = torch.exp(-(d - d[..., :1]) / torch.tensor(tau, dtype=dt))
    S = e[..., 0]
    for j in range(1, k):
        S = S + e[..., j]
    a = e / S.unsqueeze(-1)
    zero = torch.zeros(B, N, dtype=dt)
    out = []
    for c in range(6):
        if c not in G:
            out.append(zero)
            continue
        v = a[..., 0] * G[c][..., 0]
        for j in range(1, k):
            v = v + a[..., j] * G[c][..., j]
        out.append(v)
    return torch.stack(out, dim=-1), a, d


class ICPSoftminRef:
    """ICPSoftRef with soft correspondences: k neighbours, temperature tau (m^2); trim_steep 0 is the hard gate."""

    def __init__(self, icp_type="pt2pt", differentiable=True, max_iterations=100, tolerance=1e-12, k=4, tau=0.25, trim_steep=0.0):
        assert icp_type in ("pt2pt", "pt2pl") and 2 <= k <= 8 and tau > 0
        self.icp_type = icp_type
        self.differentiable = differentiable
        self.max_iterations = int(max_iterations)
        self.tolerance = float(tolerance)
        self.k, self.tau, self.trim_steep = int(k), float(tau), float(trim_steep)

    def icp(self, source, target, T_init=None, weight=None, trim_dist=5.0, loss_fn=None, dim=3, dtype=torch.float32,
            fixed_idx=None):
        src = source.to(dtype)
        tgt = target.to(dtype)
        B, N, _ = src.shape
        assert tgt.shape[1] >= self.k
        if self.icp_type == "pt2pl" and tgt.shape[-1] < 6:
            raise ValueError("pt2pl needs target normals: target must be (B,M,6)")
        Tk = torch.eye(4, dtype=dtype).repeat(B, 1, 1) if T_init is None else T_init.to(dtype)
        omega = torch.ones(B, N, dtype=dtype) if weight is None else weight.to(dtype)
        loss_name = None if loss_fn is None else loss_fn.get("name")
        loss_k = 1.0 if loss_fn is None else float(loss_fn.get("metric", 1.0))
        tgt_np = np.ascontiguousarray(tgt[..., :dim].detach().float().numpy())
        own = torch.arange(N).expand(B, N)                      # the virtual target has one row per point
        active = torch.ones(B, dtype=torch.bool)
        hist = {"idx": [], "a": [], "d": [], "T": [Tk.detach().clone()], "delta": [], "active": [], "keep": [], "huber_out": []}
        with torch.set_grad_enabled(self.differentiable and torch.is_grad_enabled()):
            for it in range(self.max_iterations):
                if not bool(active.any()):
                    break
                if fixed_idx is not None:
                    idx = fixed_idx[it].long()
                else:
                    p = torch.stack(transform_points(src.detach(), Tk.detach(), dim), dim=-1)
                    idx = torch.from_numpy(knn_ref_batch(p.float().numpy(), tgt_np, self.k, dim)[0])
                P = transform_points(src, Tk, dim)
                virt, a, d = soft_rows(tgt, P, idx, self.tau, dim, self.icp_type == "pt2pl")
                J, e, w, _, aux = per_point_terms(src, virt, Tk, own, omega, self.icp_type, loss_name, loss_k, trim_dist, dim,
                                                  self.trim_steep)
                A, b = normal_equations(J, e, w)
                delta, ok = solve_spd(A, b)
                delta = torch.where(active[:, None], delta, torch.zeros_like(delta))
                E = se_exp(delta, dim)
                Tn = (E @ Tk.double()).to(dtype)
                Tk = torch.where(active[:, None, None], Tn, Tk)
                hist["idx"].append(idx.clone())
                hist["a"].append(a.detach().clone())
                hist["d"].append(d.detach().clone())
                hist["delta"].append(delta.detach().clone())
                hist["active"].append(active.clone())
                hist["T"].append(Tk.detach().clone())
                hist["keep"].append(aux["keep"])
                hist["huber_out"].append(torch.sqrt(aux["r2"]) > loss_k)
                conv = delta.detach().norm(dim=1) < self.tolerance
                active = active & ~conv
        return {"T": Tk, "hist": hist, "num_iter": len(hist["delta"])}


def soft_backward_closed_form(tgt, p, idx, tau, dim, with_normals, vbar):
    """I7''' in numpy, fp64: the adjoint vbar (N,6) of the virtual rows of ONE pair -> (grad_tgt (M,cols), pbar (N,dim)), the
    target rows' gradient and the softmin's share of the points' adjoint.  tgt (M,cols), p (N,dim), idx (N,k)."""
    tgt, p, vbar = np.asarray(tgt, np.float64), np.asarray(p, np.float64), np.asarray(vbar, np.float64)
    N, k = idx.shape
    gt = np.zeros_like(tgt)
    pbar = np.zeros((N, dim))
    for i in range(N):
        q = tgt[idx[i], :dim]
        diff = q - p[i]
        d = (diff * diff).sum(axis=1)
        e = np.exp(-(d - d[0]) / tau)
        a = e / e.sum()
        abar = q @ vbar[i, :dim]
        if with_normals:
            abar = abar + tgt[idx[i], 3:3 + dim] @ vbar[i, 3:3 + dim]
        m = 0.0
        for l in range(k):
            m += a[l] * abar[l]
        zbar = a * (abar - m)
        dbar = -zbar / tau
        for j in range(k):
            h = 2.0 * dbar[j] * diff[j]
            gt[idx[i, j], :dim] += a[j] * vbar[i, :dim] + h
            if with_normals:
                gt[idx[i, j], 3:3 + dim] += a[j] * vbar[i, 3:3 + dim]
            pbar[i] -= h
    return gt, pbar
