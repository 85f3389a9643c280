"""CPU restatement of the dICP with the Geman-McClure and Welsch kernels next to Cauchy and Huber (DESIGN.md §3 I3, I7, I7'')
-- a module of the tests, not a test.

``per_point_terms`` is tests/dicp_hyper_ref.py's with two more branches, every operation rounded on its own in the clouds' dtype:

    geman_mcclure:  c = 1 / (1 + r2 / (k k))  (Cauchy's expression),  rho = c c
    welsch:         rho = exp(-(r2 / (k k)))

``k``, ``trim_dist`` and ``trim_steep`` are broadcastable to (B,N) as there: a 0-d tensor, (B,) or a (B,N) LEAF whose gradient
is every point's contribution to its pair's sum.  With ``cauchy``, ``huber`` or no loss ``ICPRobustRef.icp`` returns what
``ICPHyperRef.icp`` returns, bit for bit (tests/test_robust_kernels_cpu.py).

Two loops, both built from the oracle's helpers the way the sibling restatements are:

  ``icp``       nearest correspondences (the oracle's search, or ``fixed_idx`` (K,B,N) replayed);
  ``icp_soft``  soft correspondences: the virtual rows of tests/dicp_softmin_temp_ref.py's ``soft_rows_t`` (``tau`` a (B,N)
                tensor that stays in the graph) fed to the same ``per_point_terms`` with ``own = arange(N)``; the search is the
                numpy k-NN, or ``fixed_idx`` (K,B,N,k) replayed.

``hist`` carries per iteration ``idx, delta, active, T, A, b, keep, rho, r2, d2, huber_out``, the point's weight ``w`` (in the
graph, gradient retained: w.grad is I7's wbar), ``terms`` (ICPHyperRef's, what the closed forms start from, and ``r2_graph``:
r2 in the graph with its gradient retained -- I7's r2bar wherever the gate does not read the same tensor, i.e. for pt2pl and
under the hard gate) and, for the soft loop, ``a`` and ``d``.

``closed_form_kbar`` and ``closed_form_r2bar`` are the new chains of I7 / I7'' written out in numpy, fp64.
"""
import numpy as np
import torch

from oracle import _clib
from oracle.dicp_ref import normal_equations, se_exp, solve_spd, transform_points

from dicp_hyper_ref import as_bn
from dicp_softmin_ref import knn_ref_batch
from dicp_softmin_temp_ref import soft_rows_t

ROBUST = ("cauchy", "huber", "geman_mcclure", "welsch")


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
    elif loss_name == "geman_mcclure":
        c = 1.0 / (1.0 + r2 / (k * k))
        rho = c * c
    elif loss_name == "welsch":
        rho = torch.exp(-(r2 / (k * k)))
    elif loss_name in ("l2", "none", None):
        rho = one
    else:
        raise ValueError("unknown loss_fn name %r" % (loss_name,))
    w = (omega * keep) * rho
    J = torch.stack([torch.stack(row, dim=-1) for row in Jrows], dim=-2)
    e = torch.stack(erows, dim=-1)
    aux = {"keep": keep.detach(), "rho": rho.detach(), "r2": r2.detach(), "d2": d2.detach(), "d": d.detach(), "th": th.detach(),
           "omega": omega.detach(), "r2_graph": r2}
    return J, e, w, torch.stack(P, dim=-1), aux


class ICPRobustRef:
    """dicp_hyper_ref.ICPHyperRef with the two kernels, and the same loop over soft correspondences; ``soft`` selects the gate."""

    def __init__(self, icp_type="pt2pt", differentiable=True, max_iterations=100, tolerance=1e-12, soft=False):
        assert icp_type in ("pt2pt", "pt2pl")
        self.icp_type = icp_type
        self.differentiable = differentiable
        self.max_iterations = int(max_iterations)
        self.tolerance = float(tolerance)
        self.soft = bool(soft)

    def _run(self, src, tgt, T_init, weight, k, trim_dist, trim_steep, loss_name, dim, dtype, rows):
        """The Gauss-Newton loop.  ``rows(it, src, tgt, Tk)`` -> (the rows per_point_terms gathers from, its idx, what ``hist``
        records as idx, extra hist entries)."""
        B, N, _ = src.shape
        if self.icp_type == "pt2pl" and tgt.shape[-1] < 6:
            raise ValueError("pt2pl needs target normals: target must be (B,M,6)")
        Tk = torch.eye(4, dtype=dtype).repeat(B, 1, 1) if T_init is None else T_init.to(dtype)
        omega = torch.ones(B, N, dtype=dtype) if weight is None else weight.to(dtype)
        kk, cc, ss = as_bn(k, B, dtype), as_bn(trim_dist, B, dtype), as_bn(trim_steep, B, dtype)
        active = torch.ones(B, dtype=torch.bool)
        hist = {"idx": [], "T": [Tk.detach().clone()], "delta": [], "active": [], "keep": [], "rho": [], "r2": [], "w": [],
                "huber_out": [], "A": [], "b": [], "d2": [], "terms": [], "a": [], "d": []}
        grad_on = self.differentiable and torch.is_grad_enabled()
        with torch.set_grad_enabled(grad_on):
            for it in range(self.max_iterations):
                if not bool(active.any()):
                    break
                table, idx, idx_rec, extra = rows(it, src, tgt, Tk)
                J, e, w, _, aux = per_point_terms(src, table, Tk, idx, omega, self.icp_type, loss_name, kk, cc, ss, dim, self.soft)
                if grad_on and w.requires_grad:
                    w.retain_grad()
                    if aux["r2_graph"].requires_grad:
                        aux["r2_graph"].retain_grad()
                A, b = normal_equations(J, e, w)
                delta, ok = solve_spd(A, b)
                delta = torch.where(active[:, None], delta, torch.zeros_like(delta))
                E = se_exp(delta, dim)
                Tn = (E @ Tk.double()).to(dtype)
                Tk = torch.where(active[:, None, None], Tn, Tk)
                hist["idx"].append(idx_rec.clone())
                hist["delta"].append(delta.detach().clone())
                hist["active"].append(active.clone())
                hist["T"].append(Tk.detach().clone())
                for name in ("keep", "rho", "r2", "d2"):
                    hist[name].append(aux[name])
                hist["w"].append(w)
                hist["huber_out"].append(torch.sqrt(aux["r2"]) > kk.detach())
                hist["A"].append(A.detach().clone())
                hist["b"].append(b.detach().clone())
                hist["terms"].append(dict(aux, w=w))
                for name, v in extra.items():
                    hist[name].append(v.detach().clone())
                conv = delta.detach().norm(dim=1) < self.tolerance
                active = active & ~conv
        return {"T": Tk, "hist": hist, "num_iter": len(hist["delta"])}

    def icp(self, source, target, T_init=None, weight=None, k=1.0, trim_dist=5.0, trim_steep=10.0, loss_name=None, dim=3,
            dtype=torch.float32, fixed_idx=None):
        """Nearest correspondences; ``fixed_idx``: a list of (B,N) index tensors, one per iteration, replayed."""
        src, tgt = source.to(dtype), target.to(dtype)
        tgt_xy = np.ascontiguousarray(tgt[..., :dim].detach().float().numpy())

        def rows(it, src_, tgt_, Tk):
            if fixed_idx is not None:
                idx = fixed_idx[it]
            else:
                p = torch.stack(transform_points(src_.detach(), Tk.detach(), dim), dim=-1)
                idx = torch.from_numpy(_clib.nn_search(p.float().numpy(), tgt_xy)[0])
            return tgt_, idx, idx, {}

        return self._run(src, tgt, T_init, weight, k, trim_dist, trim_steep, loss_name, dim, dtype, rows)

    def icp_soft(self, source, target, tau, softmin_k=4, T_init=None, weight=None, k=1.0, trim_dist=5.0, trim_steep=10.0,
                 loss_name=None, dim=3, dtype=torch.float32, fixed_idx=None):
        """Soft correspondences over the ``softmin_k`` nearest rows with the temperatures ``tau`` (B,N); ``fixed_idx``: a list
        of (B,N,softmin_k) index tensors replayed."""
        src, tgt = source.to(dtype), target.to(dtype)
        B, N, _ = src.shape
        assert tgt.shape[1] >= softmin_k
        tau = tau.to(dtype)
        tgt_np = np.ascontiguousarray(tgt[..., :dim].detach().float().numpy())
        own = torch.arange(N).expand(B, N)                      # the virtual target has one row per point

        def rows(it, src_, tgt_, Tk):
            if fixed_idx is not None:
                idx = fixed_idx[it].long()
            else:
                p = torch.stack(transform_points(src_.detach(), Tk.detach(), dim), dim=-1)
                idx = torch.from_numpy(knn_ref_batch(p.float().numpy(), tgt_np, softmin_k, dim)[0])
            virt, a, d = soft_rows_t(tgt_, transform_points(src_, Tk, dim), idx, tau, dim, self.icp_type == "pt2pl")
            return virt, own, idx, {"a": a, "d": d}

        return self._run(src, tgt, T_init, weight, k, trim_dist, trim_steep, loss_name, dim, dtype, rows)


def _rhobar(t, act):
    wg = t["w"].grad if t["w"].grad is not None else torch.zeros_like(t["w"])
    wbar = wg.double().numpy() * act.numpy()[:, None]                       # (a frozen pair: exactly 0)
    return (wbar * t["omega"].double().numpy()) * t["keep"].double().numpy()


def closed_form_kbar(hist, k, loss_name):
    """I7'' for the two kernels in numpy (fp64) from ``hist["terms"]`` after a backward pass: the per-point k̄_i summed over
    the iterations -> (B,N).  k: an array broadcastable to (B,N)."""
    k = np.asarray(k, np.float64)
    k2 = k * k
    out = 0.0
    for t, act in zip(hist["terms"], hist["active"]):
        rhobar, rho, r2 = _rhobar(t, act), t["rho"].double().numpy(), t["r2"].double().numpy()
        if loss_name == "geman_mcclure":
            c = 1.0 / (1.0 + r2 / k2)
            out = out + rhobar * ((4.0 * r2 * (c * rho)) / (k * k2))
        elif loss_name == "welsch":
            out = out + rhobar * ((2.0 * r2 * rho) / (k * k2))
        else:
            raise ValueError(loss_name)
    return out


def closed_form_r2bar(t, act, k, loss_name):
    """I7's r2bar line for the two kernels in numpy (fp64) for ONE iteration's ``terms`` -> (B,N)."""
    k = np.asarray(k, np.float64)
    k2 = k * k
    rhobar, rho, r2 = _rhobar(t, act), t["rho"].double().numpy(), t["r2"].double().numpy()
    if loss_name == "geman_mcclure":
        c = 1.0 / (1.0 + r2 / k2)
        return rhobar * (-(2.0 * (c * rho)) / k2)
    if loss_name == "welsch":
        return rhobar * (-rho / k2)
    raise ValueError(loss_name)
