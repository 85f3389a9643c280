"""CPU restatement of the dICP with the soft (tanh) trim gate of DESIGN.md §3 I3' -- a module of the tests, not a test.

``per_point_terms`` is oracle.dicp_ref.per_point_terms with one more argument, ``trim_steep``:

    0     the hard gate  keep = d2 < trim_dist^2                                   (I3, the oracle's own lines)
    > 0   the soft gate  d = sqrt(d2); th = tanh(trim_steep (d - trim_dist)); keep = 0.5 - 0.5 th      (I3')

in the dtype of the clouds (fp32 normative: torch rounds every operation on its own), with w = (weight keep) rho as before.
The square root is guarded like the oracle's Huber branch (sqrt of 1 where d2 == 0, the value put back as 0), so autograd
stays finite at a coincident point and gives it no gradient through the gate -- the `d > 0 ? ... : 0` of I7'.

``ICPSoftRef`` is oracle.dicp_ref.ICPRef's loop around it, built from the oracle's own helpers (transform_points,
normal_equations, solve_spd, se_exp, _clib.nn_search, the fixed_idx replay and the dtype switch); with trim_steep = 0 it
returns what ICPRef returns, bit for bit.  ``hist`` also carries per iteration ``keep`` (B,N) and, for Huber, ``huber_out``
(B,N): r > k.
"""
import numpy as np
import torch

from oracle import _clib
from oracle.dicp_ref import normal_equations, se_exp, solve_spd, transform_points


def soft_keep(d2, trim_dist, trim_steep):
    """I3': the gate of squared distances d2 (any float dtype), autograd-safe at d2 == 0."""
    dt = d2.dtype
    pos = d2 > 0
    d = torch.where(pos, torch.sqrt(torch.where(pos, d2, torch.ones_like(d2))), torch.zeros_like(d2))
    th = torch.tanh(torch.tensor(trim_steep, dtype=dt) * (d - torch.tensor(trim_dist, dtype=dt)))
    return 0.5 - 0.5 * th


def per_point_terms(src, tgt, Tk, idx, omega, icp_type, loss_name, loss_k, trim_dist, dim, trim_steep=0.0):
    """Stages I1, I3 / I3', I4 for given correspondences -> J (B,N,nr,p), e (B,N,nr), w (B,N), p (B,N,dim), aux (keep, rho)."""
    dt = src.dtype
    P = transform_points(src, Tk, dim)
    px, py = P[0], P[1]
    if dim == 3:
        pz = P[2]
    idx64 = idx.long()
    Q = [torch.gather(tgt[..., c], 1, idx64) for c in range(dim)]
    Ev = [Q[c] - P[c] for c in range(dim)]
    d2 = Ev[0] * Ev[0] + Ev[1] * Ev[1]
    if dim == 3:
        d2 = d2 + Ev[2] * Ev[2]
    if trim_steep > 0:
        keep = soft_keep(d2, trim_dist, trim_steep)
    else:
        trim = torch.tensor(trim_dist, dtype=dt)
        keep = (d2 < trim * trim).to(dt)
    one = torch.ones_like(px)
    zero = torch.zeros_like(px)
    if icp_type == "pt2pl":
        Nn = [torch.gather(tgt[..., 3 + c], 1, idx64) for c in range(dim)]
        e = Nn[0] * Ev[0] + Nn[1] * Ev[1]
        if dim == 3:
            e = e + Nn[2] * Ev[2]
        r2 = e * e
        if dim == 2:
            Jrows = [[Nn[0], Nn[1], Nn[1] * px - Nn[0] * py]]
        else:
            Jrows = [[Nn[0], Nn[1], Nn[2],
                      py * Nn[2] - pz * Nn[1], pz * Nn[0] - px * Nn[2], px * Nn[1] - py * Nn[0]]]
        erows = [e]
    else:
        r2 = d2
        if dim == 2:
            Jrows = [[one, zero, -py], [zero, one, px]]
        else:
            Jrows = [[one, zero, zero, zero, pz, -py],
                     [zero, one, zero, -pz, zero, px],
                     [zero, zero, one, py, -px, zero]]
        erows = Ev
    k = torch.tensor(loss_k, dtype=dt)
    if loss_name == "cauchy":
        rho = 1.0 / (1.0 + r2 / (k * k))
    elif loss_name == "huber":
        rr = torch.sqrt(r2.detach())
        r_safe = torch.sqrt(torch.where(r2 > 0, r2, torch.ones_like(r2)))
        rho = torch.where(rr <= k, one, k / r_safe)
    elif loss_name in ("l2", "none", None):
        rho = one
    else:
        raise ValueError("unknown loss_fn name %r" % (loss_name,))
    w = (omega * keep) * rho
    J = torch.stack([torch.stack(row, dim=-1) for row in Jrows], dim=-2)
    e = torch.stack(erows, dim=-1)
    aux = {"keep": keep.detach(), "rho": rho.detach(), "r2": r2.detach(), "d2": d2.detach()}
    return J, e, w, torch.stack(P, dim=-1), aux


class ICPSoftRef:
    """oracle.dicp_ref.ICPRef with the gate of ``trim_steep`` (0: hard)."""

    def __init__(self, icp_type="pt2pt", differentiable=True, max_iterations=100, tolerance=1e-12, trim_steep=0.0):
        assert icp_type in ("pt2pt", "pt2pl")
        self.icp_type = icp_type
        self.differentiable = differentiable
        self.max_iterations = int(max_iterations)
        self.tolerance = float(tolerance)
        self.trim_steep = float(trim_steep)

    def icp(self, source, target, T_init=None, weight=None, trim_dist=5.0, loss_fn=None, dim=3, dtype=torch.float32,
            fixed_idx=None):
        src = source.to(dtype)
        tgt = target.to(dtype)
        B, N, _ = src.shape
        if self.icp_type == "pt2pl" and tgt.shape[-1] < 6:
            raise ValueError("pt2pl needs target normals: target must be (B,M,6)")
        Tk = torch.eye(4, dtype=dtype).repeat(B, 1, 1) if T_init is None else T_init.to(dtype)
        omega = torch.ones(B, N, dtype=dtype) if weight is None else weight.to(dtype)
        loss_name = None if loss_fn is None else loss_fn.get("name")
        loss_k = 1.0 if loss_fn is None else float(loss_fn.get("metric", 1.0))
        tgt_xy = np.ascontiguousarray(tgt[..., :dim].detach().float().numpy())
        active = torch.ones(B, dtype=torch.bool)
        hist = {"idx": [], "T": [Tk.detach().clone()], "delta": [], "active": [], "keep": [], "huber_out": [], "A": [], "b": [], "d2": []}
        with torch.set_grad_enabled(self.differentiable and torch.is_grad_enabled()):
            for k in range(self.max_iterations):
                if not bool(active.any()):
                    break
                if fixed_idx is not None:
                    idx = fixed_idx[k]
                else:
                    p = torch.stack(transform_points(src.detach(), Tk.detach(), dim), dim=-1)
                    idx_np, _ = _clib.nn_search(p.float().numpy(), tgt_xy)
                    idx = torch.from_numpy(idx_np)
                J, e, w, _, aux = per_point_terms(src, tgt, Tk, idx, omega, self.icp_type, loss_name, loss_k, trim_dist, dim,
                                                  self.trim_steep)
                A, b = normal_equations(J, e, w)
                delta, ok = solve_spd(A, b)
                delta = torch.where(active[:, None], delta, torch.zeros_like(delta))
                E = se_exp(delta, dim)
                Tn = (E @ Tk.double()).to(dtype)
                Tk = torch.where(active[:, None, None], Tn, Tk)
                hist["idx"].append(idx.clone())
                hist["delta"].append(delta.detach().clone())
                hist["active"].append(active.clone())
                hist["T"].append(Tk.detach().clone())
                hist["keep"].append(aux["keep"])
                hist["huber_out"].append(torch.sqrt(aux["r2"]) > loss_k)
                hist["d2"].append(aux["d2"])
                hist["A"].append(A.detach().clone())
                hist["b"].append(b.detach().clone())
                conv = delta.detach().norm(dim=1) < self.tolerance
                active = active & ~conv
        return {"T": Tk, "hist": hist, "num_iter": len(hist["delta"])}


def band_share(keep, real, lo=0.05, hi=0.95):
    """Share of the real points (boolean ``real`` (B,N)) whose gate lies strictly between lo and hi."""
    k = keep[real]
    return float(((k > lo) & (k < hi)).double().mean())
