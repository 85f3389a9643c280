"""CPU restatement of the dICP with the robust scale k, the trim distance and the gate's steepness as TENSORS (DESIGN.md §3
I3'', I7'') -- a module of the tests, not a test.

It is tests/dicp_soft_trim_ref.py with ``k``, ``trim_dist`` and ``trim_steep`` broadcastable to (B,N): a 0-d tensor (shared by
the batch), (B,) (one value per pair) or (B,N) (one LEAF per point, whose gradient is that point's contribution to its pair's
sum -- what the tests' "is the gradient awake" conditions are made of).  Autograd reaches all three.  The gate's MODE is a
constant of the instance (``soft``), as it is a constant of the launch on the device; in hard mode the steepness is not read.

The arithmetic is the soft-trim restatement's line for line (same operations in the same order in the clouds' dtype), and the
loop is built from the oracle's helpers the same way, so with plain equal values ``ICPHyperRef`` returns what ``ICPSoftRef``
returns, bit for bit (tests/test_icp_hyper_cpu.py).  ``hist`` carries what ICPSoftRef's does and, per iteration, ``terms``:
the point's weight ``w`` (in the graph, gradient retained: w.grad is I7's wbar) and detached ``omega, keep, rho, r2, d, th``
-- the quantities the closed forms of I7'' start from.
"""
import numpy as np
import torch

from oracle import _clib
from oracle.dicp_ref import normal_equations, se_exp, solve_spd, transform_points


def as_bn(v, B, dtype):
    """A hyper-parameter as a tensor broadcastable to (B,N): () -> (1,1), (B,) or (1,) -> (B,1) / (1,1), (B,N) as it is."""
    v = v if isinstance(v, torch.Tensor) else torch.tensor(float(v))
    v = v.to(dtype)
    if v.ndim == 0:
        return v.reshape(1, 1)
    if v.ndim == 1:
        assert v.shape[0] in (1, B)
        return v[:, None]
    assert v.ndim == 2 and v.shape[0] == B
    return v


def per_point_terms(src, tgt, Tk, idx, omega, icp_type, loss_name, k, trim, steep, dim, soft):
    """Stages I1, I3'' and I4 for given correspondences; k, trim, steep are (B|1, N|1) tensors of the clouds' dtype."""
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
    if soft:
        pos = d2 > 0
        d = torch.where(pos, torch.sqrt(torch.where(pos, d2, torch.ones_like(d2))), torch.zeros_like(d2))
        th = torch.tanh(steep * (d - trim))
        keep = 0.5 - 0.5 * th
    else:
        d, th = torch.zeros_like(d2), torch.zeros_like(d2)
        keep = (d2 < trim * trim).to(d2.dtype)
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
    aux = {"keep": keep.detach(), "rho": rho.detach(), "r2": r2.detach(), "d2": d2.detach(), "d": d.detach(), "th": th.detach(),
           "omega": omega.detach()}
    return J, e, w, torch.stack(P, dim=-1), aux


class ICPHyperRef:
    """dicp_soft_trim_ref.ICPSoftRef with tensor hyper-parameters; ``soft`` selects the gate."""

    def __init__(self, icp_type="pt2pt", differentiable=True, max_iterations=100, tolerance=1e-12, soft=False):
        assert icp_type in ("pt2pt", "pt2pl")
        self.icp_type = icp_type
        self.differentiable = differentiable
        self.max_iterations = int(max_iterations)
        self.tolerance = float(tolerance)
        self.soft = bool(soft)

    def icp(self, source, target, T_init=None, weight=None, k=1.0, trim_dist=5.0, trim_steep=10.0, loss_name=None, dim=3,
            dtype=torch.float32, fixed_idx=None):
        src = source.to(dtype)
        tgt = target.to(dtype)
        B, N, _ = src.shape
        if self.icp_type == "pt2pl" and tgt.shape[-1] < 6:
            raise ValueError("pt2pl needs target normals: target must be (B,M,6)")
        Tk = torch.eye(4, dtype=dtype).repeat(B, 1, 1) if T_init is None else T_init.to(dtype)
        omega = torch.ones(B, N, dtype=dtype) if weight is None else weight.to(dtype)
        kk, cc, ss = as_bn(k, B, dtype), as_bn(trim_dist, B, dtype), as_bn(trim_steep, B, dtype)
        tgt_xy = np.ascontiguousarray(tgt[..., :dim].detach().float().numpy())
        active = torch.ones(B, dtype=torch.bool)
        hist = {"idx": [], "T": [Tk.detach().clone()], "delta": [], "active": [], "keep": [], "huber_out": [], "A": [], "b": [], "d2": [],
                "terms": []}
        grad_on = self.differentiable and torch.is_grad_enabled()
        with torch.set_grad_enabled(grad_on):
            for it in range(self.max_iterations):
                if not bool(active.any()):
                    break
                if fixed_idx is not None:
                    idx = fixed_idx[it]
                else:
                    p = torch.stack(transform_points(src.detach(), Tk.detach(), dim), dim=-1)
                    idx_np, _ = _clib.nn_search(p.float().numpy(), tgt_xy)
                    idx = torch.from_numpy(idx_np)
                J, e, w, _, aux = per_point_terms(src, tgt, Tk, idx, omega, self.icp_type, loss_name, kk, cc, ss, dim, self.soft)
                if grad_on and w.requires_grad:
                    w.retain_grad()
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
                hist["huber_out"].append(torch.sqrt(aux["r2"]) > kk.detach())
                hist["d2"].append(aux["d2"])
                hist["A"].append(A.detach().clone())
                hist["b"].append(b.detach().clone())
                hist["terms"].append(dict(aux, w=w))
                conv = delta.detach().norm(dim=1) < self.tolerance
                active = active & ~conv
        return {"T": Tk, "hist": hist, "num_iter": len(hist["delta"])}


def closed_form_sums(hist, k, trim_dist, trim_steep, loss_name, soft):
    """I7'' written out in numpy (fp64) from the quantities of ``hist["terms"]`` after a backward pass: the per-point adjoints
    (k̄_i, c̄_i, s̄_i) summed over the iterations -> three (B,N) arrays.  k, trim_dist, trim_steep: arrays broadcastable to (B,N)."""
    k, c, s = (np.asarray(v, np.float64) for v in (k, trim_dist, trim_steep))
    out = None
    for t, act in zip(hist["terms"], hist["active"]):
        wg = t["w"].grad if t["w"].grad is not None else torch.zeros_like(t["w"])
        wbar = wg.double().numpy() * act.numpy()[:, None]                   # (a frozen pair: exactly 0)
        omega, keep, rho, r2, d, th = (t[n].double().numpy() for n in ("omega", "keep", "rho", "r2", "d", "th"))
        rhobar = (wbar * omega) * keep
        if loss_name == "cauchy":
            kbar = rhobar * (2.0 * r2 * rho * rho) / (k * (k * k))
        elif loss_name == "huber":
            r = np.sqrt(r2)
            kbar = np.where(r > k, rhobar / np.where(r > 0, r, 1.0), 0.0)
        else:
            kbar = np.zeros_like(wbar)
        if soft:
            keepbar = (wbar * omega) * rho
            g = 0.5 * (1.0 - th * th)
            cbar, sbar = keepbar * (s * g), keepbar * (-g * (d - c))
        else:
            cbar, sbar = np.zeros_like(wbar), np.zeros_like(wbar)
        cur = np.stack([kbar, cbar, sbar])
        out = cur if out is None else out + cur
    return out
