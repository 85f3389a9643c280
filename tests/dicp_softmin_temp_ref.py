"""CPU restatement of the dICP's soft correspondences with the temperature as a differentiable input (DESIGN.md §3 I3⁗,
I7⁗) -- a module of the tests, not a test.

``soft_rows_t`` is tests/dicp_softmin_ref.py's ``soft_rows`` with ``tau`` a (B,N) tensor that stays in the graph (that one
wraps a float in ``torch.tensor(...)``, which cuts it).  The expression is I3''' unchanged, every operation rounded on its
own in the dtype of the clouds:

    e_j = exp(-(d_j - d_0) / tau_i);  S = sum_j e_j in slot order;  a_j = e_j / S;  row~ = sum_j a_j row_j in slot order.

With every tau_i of a pair equal to a float it has soft_rows' bits (tests/test_softmin_temp_cpu.py asserts it).

``ICPSoftminTempRef`` is ICPSoftminRef's loop with that function.  ``tau`` is given per call: a (B,N) LEAF broadcast from
the per-pair values, so that its gradient is every point's contribution summed over the iterations; ``pair_sums`` turns
that into the per-pair references g_b (fp64 row sums) and S_b = sum |contributions|, which feeds the awake condition
max_b |g_b| / S_b >= 0.03 of tests/test_gpu_icp_hyper.py.

``temp_bar_closed_form`` is I7⁗ in numpy, fp64, for one pair and one iteration: from the adjoint of the virtual rows,

    z̄_j = a_j (ā_j - m);   u = sum_j z̄_j (d_j - d_0) in slot order (slot 0 adds exactly 0);   tau-bar_i = u / (tau * tau).
"""
import numpy as np
import torch

from oracle.dicp_ref import normal_equations, se_exp, solve_spd, transform_points

from dicp_soft_trim_ref import per_point_terms
from dicp_softmin_ref import ICPSoftminRef, _dist, knn_ref_batch


def soft_rows_t(tgt, P, idx, tau, dim, with_normals):
    """tgt (B,M,cols), P list of dim (B,N) coordinates, idx (B,N,k), tau (B,N) in the clouds' dtype -> virtual rows (B,N,6),
    a (B,N,k), d (B,N,k)."""
    dt = tgt.dtype
    assert tau.dtype == dt and tuple(tau.shape) == tuple(idx.shape[:2])
    B, N, k = idx.shape
    flat = idx.reshape(B, N * k).long()
    cols = list(range(dim)) + ([3 + c for c in range(dim)] if with_normals else [])
    G = {c: torch.gather(tgt[..., c], 1, flat).reshape(B, N, k) for c in cols}
    d = _dist([G[c] for c in range(dim)], [P[c].unsqueeze(-1) for c in range(dim)], dim)
    e = torch.exp(-(d - d[..., :1]) / tau.unsqueeze(-1))
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


def tau_leaf(per_pair, N, dtype=torch.float32):
    """(B,) values -> the (B,N) leaf of ICPSoftminTempRef.icp."""
    t = torch.as_tensor(per_pair, dtype=dtype).reshape(-1)
    return t[:, None].expand(t.shape[0], N).contiguous().requires_grad_(True)


def pair_sums(leaf_grad):
    """The (B,N) gradient of a tau leaf -> (g_b, S_b): fp64 row sums and the sums of the magnitudes."""
    p = leaf_grad.double()
    return p.sum(1), p.abs().sum(1)


class ICPSoftminTempRef(ICPSoftminRef):
    """ICPSoftminRef whose temperature is the call's ``tau`` (B,N) tensor; the instance's own tau is not used."""

    def icp(self, source, target, tau, T_init=None, weight=None, trim_dist=5.0, loss_fn=None, dim=3, dtype=torch.float32,
            fixed_idx=None):
        src = source.to(dtype)
        tgt = target.to(dtype)
        B, N, _ = src.shape
        assert tgt.shape[1] >= self.k
        if self.icp_type == "pt2pl" and tgt.shape[-1] < 6:
            raise ValueError("pt2pl needs target normals: target must be (B,M,6)")
        tau = tau.to(dtype)
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
                virt, a, d = soft_rows_t(tgt, P, idx, tau, dim, self.icp_type == "pt2pl")
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


def temp_bar_closed_form(tgt, p, idx, tau, dim, with_normals, vbar):
    """I7⁗ in numpy, fp64: the adjoint vbar (N,6) of the virtual rows of ONE pair -> tau-bar per point (N,).  tgt (M,cols),
    p (N,dim), idx (N,k); tau a float or (N,)."""
    tgt, p, vbar = np.asarray(tgt, np.float64), np.asarray(p, np.float64), np.asarray(vbar, np.float64)
    N, k = idx.shape
    tau = np.broadcast_to(np.asarray(tau, np.float64), (N,))
    out = np.zeros(N)
    for i in range(N):
        q = tgt[idx[i], :dim]
        diff = q - p[i]
        d = (diff * diff).sum(axis=1)
        e = np.exp(-(d - d[0]) / tau[i])
        a = e / e.sum()
        abar = q @ vbar[i, :dim]
        if with_normals:
            abar = abar + tgt[idx[i], 3:3 + dim] @ vbar[i, 3:3 + dim]
        m = 0.0
        for l in range(k):
            m += a[l] * abar[l]
        zbar = a * (abar - m)
        u = 0.0
        for j in range(k):
            u += zbar[j] * (d[j] - d[0])
        out[i] = u / (tau[i] * tau[i])
    return out
