"""CPU restatement of the dICP with everything the HIP dICP offers beyond oracle.dicp_ref (DESIGN.md §3 I2', I3 - I3⁗,
I7 - I7⁗) -- a module of the tests, not a test.

``per_point_terms`` is oracle.dicp_ref.per_point_terms with the trim gate hard (I3: keep = d2 < trim^2) or soft (I3': d =
sqrt(d2); th = tanh(steep (d - trim)); keep = 0.5 - 0.5 th, the square root guarded like the oracle's Huber branch so that
autograd stays finite at a coincident point), and four robust kernels:

    cauchy:         rho = 1 / (1 + r2 / (k k))           huber:   rho = 1 if r <= k else k / r
    geman_mcclure:  c = 1 / (1 + r2 / (k k)), rho = c c   welsch:  rho = exp(-(r2 / (k k)))

``k``, ``trim`` and ``steep`` are tensors broadcastable to (B,N) in the clouds' dtype, every operation is rounded on its own
(fp32 normative), and w = (weight keep) rho as in the oracle.  The GPU tests compare with these bits in places, so no
expression here is reordered or fused.

``knn_ref`` is I2' in numpy: the k target rows with the smallest I2 distance to a transformed source point, in key order
(ascending d, ties to the lowest index), with the distance expression of tests/knn_normals_ref.py (``nn_dist_f32``: the
kernels' fmaf form, bit for bit).  No row is special: ``target_pad_val`` rows are simply far away.

``soft_rows`` is I3''' / I3⁗: per point, in the dtype of the clouds,

    d_j = I2's expression, recomputed from the rows;  e_j = exp(-(d_j - d_0) / tau_i);  S = sum_j e_j in slot order;
    a_j = e_j / S;  row~ = sum_j a_j row_j in slot order (xyz; for pt2pl the normal columns too, NOT renormalised).

The fused multiply-add of I2 is restated through fp64 (a product of two fp32 values is exact there; the sum is rounded to
fp64 and then to fp32 -- the caveat of tests/knn_normals_ref.py) and stays differentiable; in fp64 it is the plain expression.
``tau`` is a (B,N) tensor that stays in the graph, or a number.

``ICPRestatement`` is oracle.dicp_ref.ICPRef's loop around these, built from the oracle's own helpers (transform_points,
normal_equations, solve_spd, se_exp, the fixed_idx replay and the dtype switch).  The gate's MODE is a constant of the
instance (``soft``), as it is a constant of the launch on the device; in hard mode the steepness is not read.  The
hyper-parameters are given per call: a number, a 0-d tensor (shared by the batch), (B,) (one value per pair) or (B,N) (one
LEAF per point, whose gradient is that point's contribution to its pair's sum -- what the tests' "is the gradient awake"
conditions are made of).  Equal values give equal bits in every form (tests/test_icp_hyper_cpu.py), and with the hard gate
``icp`` returns what the oracle returns, bit for bit (tests/test_robust_kernels_cpu.py).

  ``icp``       nearest correspondences (the oracle's search, or ``fixed_idx`` (K,B,N) replayed);
  ``icp_soft``  soft correspondences: the virtual rows of ``soft_rows`` fed to the same ``per_point_terms`` as a target of one
                row per point; the search is the numpy k-NN, or ``fixed_idx`` (K,B,N,k) replayed.  Autograd through a replay is
                the reference of the hand-derived backward (which rows are the neighbours is a constant there too).

``hist`` carries per iteration ``idx, delta, active, T, A, b, keep, rho, r2, d2, huber_out`` (r > k), the point's weight ``w``
(in the graph, gradient retained: w.grad is I7's wbar), ``terms`` (w and detached ``omega, keep, rho, r2, d2, d, th``, what the
closed forms start from, and ``r2_graph``: r2 in the graph with its gradient retained -- I7's r2bar wherever the gate does not
read the same tensor, i.e. for pt2pl and under the hard gate) and, for the soft loop, ``a`` and ``d``.

``tau_leaf`` makes the (B,N) leaf of per-pair values; ``pair_sums`` turns such a leaf's gradient into the per-pair references
g_b (fp64 row sums) and S_b = sum |contributions|, which feed the awake condition max_b |g_b| / S_b >= 0.03.

The closed forms, numpy fp64: ``closed_form_sums`` (I7'': k-bar, c-bar, s-bar per point), ``closed_form_r2bar`` (I7's r2bar line
of Geman-McClure and Welsch) and ``soft_backward_closed_form`` (I7''' and I7⁗: from the adjoint of the virtual rows,

    z̄_j = a_j (ā_j - m);  d̄_j = -z̄_j / tau;  u = sum_j z̄_j (d_j - d_0) in slot order (slot 0 adds exactly 0);
    tau-bar_i = u / (tau tau)).
"""
import numpy as np
import torch

from oracle import _clib
from oracle.dicp_ref import normal_equations, se_exp, solve_spd, transform_points

from knn_normals_ref import nn_dist_f32

ROBUST = ("cauchy", "huber", "geman_mcclure", "welsch")


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


def soft_keep(d2, trim_dist, trim_steep):
    """I3': the gate of squared distances d2 (any float dtype), autograd-safe at d2 == 0."""
    dt = d2.dtype
    pos = d2 > 0
    d = torch.where(pos, torch.sqrt(torch.where(pos, d2, torch.ones_like(d2))), torch.zeros_like(d2))
    th = torch.tanh(torch.tensor(trim_steep, dtype=dt) * (d - torch.tensor(trim_dist, dtype=dt)))
    return 0.5 - 0.5 * th


def band_share(keep, real, lo=0.05, hi=0.95):
    """Share of the real points (boolean ``real`` (B,N)) whose gate lies strictly between lo and hi."""
    k = keep[real]
    return float(((k > lo) & (k < hi)).double().mean())


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
    """tgt (B,M,cols), P list of dim (B,N) coordinates, idx (B,N,k), tau a number or (B,N) in the clouds' dtype -> virtual rows
    (B,N,6), a (B,N,k), d (B,N,k)."""
    dt = tgt.dtype
    B, N, k = idx.shape
    if not isinstance(tau, torch.Tensor):
        tau = torch.full((B, N), float(tau), dtype=dt)
    assert tau.dtype == dt and tuple(tau.shape) == (B, N)
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
    """(B,) values -> a (B,N) leaf: its gradient is every point's contribution to its pair's sum."""
    t = torch.as_tensor(per_pair, dtype=dtype).reshape(-1)
    return t[:, None].expand(t.shape[0], N).contiguous().requires_grad_(True)


def pair_sums(leaf_grad):
    """The (B,N) gradient of such a leaf -> (g_b, S_b): fp64 row sums and the sums of the magnitudes."""
    p = leaf_grad.double()
    return p.sum(1), p.abs().sum(1)


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


class ICPRestatement:
    """oracle.dicp_ref.ICPRef with tensor hyper-parameters, four robust kernels, the gate of ``soft`` and, in ``icp_soft``, soft
    correspondences."""

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
        """Soft correspondences over the ``softmin_k`` nearest rows with the temperatures ``tau`` (a number, or (B,N));
        ``fixed_idx``: a list of (B,N,softmin_k) index tensors replayed."""
        src, tgt = source.to(dtype), target.to(dtype)
        B, N, _ = src.shape
        assert 2 <= softmin_k <= min(8, tgt.shape[1])
        tau = tau.to(dtype) if isinstance(tau, torch.Tensor) else tau
        tgt_np = np.ascontiguousarray(tgt[..., :dim].detach().float().numpy())
        own = torch.arange(N).expand(B, N)                      # the virtual target has one row per point

        def rows(it, src_, tgt_, Tk):
            if fixed_idx is not None:
                idx = fixed_idx[it].long()
            else:
                p = torch.stack(transform_points(src_.detach(), Tk.detach(), dim), dim=-1)
                idx = torch.from_numpy(knn_ref_batch(p.float().numpy(), tgt_np, softmin_k, dim)[0])
            virt, a, d = soft_rows(tgt_, transform_points(src_, Tk, dim), idx, tau, dim, self.icp_type == "pt2pl")
            return virt, own, idx, {"a": a, "d": d}

        return self._run(src, tgt, T_init, weight, k, trim_dist, trim_steep, loss_name, dim, dtype, rows)


def _wbar(t, act):
    wg = t["w"].grad if t["w"].grad is not None else torch.zeros_like(t["w"])
    return wg.double().numpy() * act.numpy()[:, None]                       # (a frozen pair: exactly 0)


def _rhobar(t, act):
    return (_wbar(t, act) * t["omega"].double().numpy()) * t["keep"].double().numpy()


def closed_form_sums(hist, k, trim_dist, trim_steep, loss_name, soft):
    """I7'' written out in numpy (fp64) from the quantities of ``hist["terms"]`` after a backward pass: the per-point adjoints
    (k̄_i, c̄_i, s̄_i) summed over the iterations -> three (B,N) arrays.  k, trim_dist, trim_steep: arrays broadcastable to (B,N)."""
    k, c, s = (np.asarray(v, np.float64) for v in (k, trim_dist, trim_steep))
    k2 = k * k
    out = None
    for t, act in zip(hist["terms"], hist["active"]):
        wbar, rhobar = _wbar(t, act), _rhobar(t, act)
        omega, rho, r2, d, th = (t[n].double().numpy() for n in ("omega", "rho", "r2", "d", "th"))
        if loss_name == "cauchy":
            kbar = rhobar * (2.0 * r2 * rho * rho) / (k * (k * k))
        elif loss_name == "huber":
            r = np.sqrt(r2)
            kbar = np.where(r > k, rhobar / np.where(r > 0, r, 1.0), 0.0)
        elif loss_name == "geman_mcclure":
            cau = 1.0 / (1.0 + r2 / k2)
            kbar = rhobar * ((4.0 * r2 * (cau * rho)) / (k * k2))
        elif loss_name == "welsch":
            kbar = rhobar * ((2.0 * r2 * rho) / (k * k2))
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


def soft_backward_closed_form(tgt, p, idx, tau, dim, with_normals, vbar):
    """I7''' and I7⁗ in numpy, fp64: the adjoint vbar (N,6) of the virtual rows of ONE pair -> (grad_tgt (M,cols),
    pbar (N,dim), taubar (N,)): the target rows' gradient, the softmin's share of the points' adjoint and tau-bar per point.
    tgt (M,cols), p (N,dim), idx (N,k); tau a float or (N,)."""
    tgt, p, vbar = np.asarray(tgt, np.float64), np.asarray(p, np.float64), np.asarray(vbar, np.float64)
    N, k = idx.shape
    tau = np.broadcast_to(np.asarray(tau, np.float64), (N,))
    gt = np.zeros_like(tgt)
    pbar = np.zeros((N, dim))
    taubar = np.zeros(N)
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
        dbar = -zbar / tau[i]
        u = 0.0
        for j in range(k):
            h = 2.0 * dbar[j] * diff[j]
            gt[idx[i, j], :dim] += a[j] * vbar[i, :dim] + h
            if with_normals:
                gt[idx[i, j], 3:3 + dim] += a[j] * vbar[i, 3:3 + dim]
            pbar[i] -= h
            u += zbar[j] * (d[j] - d[0])
        taubar[i] = u / (tau[i] * tau[i])
    return gt, pbar, taubar
