"""The dICP entries that share one launch sequence give the same bits, for every <DIM, TYPE> instantiation and both searches.

One table: (pt2pt | pt2pl) x (dim 2 | 3) x (brute | grid), through the C ABI directly.  N = 300 is two accumulation blocks with
the second partial, M = 700 pads to 1024 so that the coarse-seed pass runs on the first iteration, and with B = 2 a stride
error shows in the second pair.  No tolerance anywhere: every comparison is torch.equal.

  forward      mmk_icp_forward  ==  mmk_icp_forward_hp with a (1,3) array holding the same three values
  backward     mmk_icp_backward  ==  mmk_icp_backward_points (NULL clouds)  ==  mmk_icp_backward_hp (hyper NULL, NULL clouds)
  with clouds  mmk_icp_backward_points  ==  mmk_icp_backward_hp (hyper NULL), and their grad_weight / grad_T_init are the above
"""
import ctypes
import functools

import pytest
import torch

from mm_masking_amd import _lib
from support import DEV, icp_params, pair_batch

pytestmark = pytest.mark.gpu
B, N, M, K = 2, 300, 700, 3
METRIC, TRIM = 1.0, 5.0
STATE = ("idx_hist", "T_hist", "delta_hist", "A_hist", "active_hist")
CASES = [(t, d, nn) for t, d in (("pt2pt", 2), ("pt2pl", 2), ("pt2pt", 3), ("pt2pl", 3)) for nn in ("brute", "grid")]


@functools.lru_cache(maxsize=None)
def _inputs(dim):
    """Seeded clouds, weights, start poses and the upstream gradient of a dim: made once, never written."""
    src, tgt, _ = pair_batch(B, N, M, dim, seed=31 + dim)
    g = torch.Generator().manual_seed(7 + dim)
    T0 = torch.eye(4).repeat(B, 1, 1)
    T0[:, 0, 3] += 0.2
    x = {"source": torch.from_numpy(src), "target": torch.from_numpy(tgt), "weight": torch.rand(B, N, generator=g) * 0.8 + 0.2,
         "T_init": T0, "grad_T": torch.randn(B, 4, 4, generator=g)}
    return {k: v.to(DEV).contiguous() for k, v in x.items()}


def _params(icp_type, dim, nn):
    return icp_params(B=B, N=N, M=M, dim=dim, icp_type=_lib.ICP_TYPES[icp_type], loss=_lib.LOSSES["huber"], loss_k=METRIC,
                      trim_dist=TRIM, tolerance=1e-9, max_iter=K, nn_method=_lib.NN_METHODS[nn], trim_steep=0.0)


def _forward(p, x, hyper):
    """mmk_icp_forward (hyper None) or mmk_icp_forward_hp with the shared array `hyper` -> T_out and the saved state."""
    L = _lib.lib()
    out = {"T_out": torch.zeros(B, 4, 4, device=DEV),
           "idx_hist": torch.zeros(K, B, N, dtype=torch.int32, device=DEV),
           "T_hist": torch.zeros(K + 1, B, 16, device=DEV),
           "delta_hist": torch.zeros(K, B, 6, dtype=torch.float64, device=DEV),
           "A_hist": torch.zeros(K, B, 36, dtype=torch.float64, device=DEV),
           "active_hist": torch.zeros(K + 1, B, dtype=torch.int32, device=DEV)}
    ws = torch.empty(L.mmk_icp_workspace_bytes(ctypes.byref(p)), dtype=torch.uint8, device=DEV)
    iters = ctypes.c_int(0)
    args = [ctypes.byref(p)] + [_lib.ptr(x[k]) for k in ("source", "target", "weight", "T_init")]
    args += [_lib.ptr(out[k]) for k in ("T_out",) + STATE]
    tail = [_lib.ptr(ws), ws.numel(), ctypes.byref(iters), _lib.stream_ptr(DEV)]
    if hyper is None:
        _lib.check(L.mmk_icp_forward(*args, *tail))
    else:
        _lib.check(L.mmk_icp_forward_hp(*args, _lib.ptr(hyper), 0, *tail))
    torch.cuda.synchronize()
    assert iters.value == K
    return out


def _backward(entry, p, x, state, clouds):
    """One of the three backward entries on the saved `state`; `clouds`: with both cloud outputs, else NULL for them."""
    L = _lib.lib()
    out = {"grad_weight": torch.zeros(B, N, device=DEV), "grad_T_init": torch.zeros(B, 4, 4, device=DEV)}
    if clouds:
        out["grad_source"], out["grad_target"] = torch.zeros(B, N, 3, device=DEV), torch.zeros(B, M, 6, device=DEV)
    P = ctypes.byref(p)
    args = [P] + [_lib.ptr(x[k]) for k in ("source", "target", "weight")] + [_lib.ptr(state[k]) for k in STATE]
    args += [_lib.ptr(x["grad_T"]), _lib.ptr(out["grad_weight"]), _lib.ptr(out["grad_T_init"])]
    cl = [_lib.ptr(out.get("grad_source")), _lib.ptr(out.get("grad_target"))]
    null, st = ctypes.c_void_p(0), _lib.stream_ptr(DEV)
    if entry == "backward":
        assert not clouds
        ws = torch.empty(L.mmk_icp_workspace_bytes(P), dtype=torch.uint8, device=DEV)
        _lib.check(L.mmk_icp_backward(*args, _lib.ptr(ws), ws.numel(), st))
    elif entry == "points":
        ws = torch.empty(L.mmk_icp_backward_points_workspace_bytes(P, int(clouds)), dtype=torch.uint8, device=DEV)
        _lib.check(L.mmk_icp_backward_points(*args, *cl, _lib.ptr(ws), ws.numel(), st))
    else:
        ws = torch.empty(L.mmk_icp_backward_hp_workspace_bytes(P, int(clouds), 0), dtype=torch.uint8, device=DEV)
        _lib.check(L.mmk_icp_backward_hp(*args, *cl, null, 0, null, _lib.ptr(ws), ws.numel(), st))
    torch.cuda.synchronize()
    return out


def entry_path_outputs(icp_type, dim, nn):
    """Every output of every entry path of one case, by name."""
    p, x = _params(icp_type, dim, nn), _inputs(dim)
    hyper = torch.tensor([[METRIC, TRIM, 0.0]], dtype=torch.float32, device=DEV)
    res = {"forward": _forward(p, x, None), "forward_hp": _forward(p, x, hyper)}
    state = res["forward"]
    for entry in ("backward", "points", "hp"):
        res[entry] = _backward(entry, p, x, state, clouds=False)
    for entry in ("points", "hp"):
        res[entry + "+clouds"] = _backward(entry, p, x, state, clouds=True)
    return res


def _same(a, b, names, what):
    for k in names:
        assert torch.equal(a[k], b[k]), (what, k)


@pytest.mark.parametrize("icp_type,dim,nn", CASES, ids=["%s-dim%d-%s" % c for c in CASES])
def test_entry_paths_give_the_same_bits(icp_type, dim, nn):
    r = entry_path_outputs(icp_type, dim, nn)
    _same(r["forward"], r["forward_hp"], ("T_out",) + STATE, "forward vs forward_hp")
    pose = ("grad_weight", "grad_T_init")
    _same(r["backward"], r["points"], pose, "backward vs backward_points, NULL clouds")
    _same(r["backward"], r["hp"], pose, "backward vs backward_hp, hyper NULL, NULL clouds")
    _same(r["points+clouds"], r["hp+clouds"], pose + ("grad_source", "grad_target"), "backward_points vs backward_hp, clouds")
    _same(r["backward"], r["points+clouds"], pose, "backward vs backward_points, clouds")
    # the case is awake: the pairs iterate to the end, and every gradient is finite and not identically zero per pair
    assert bool(r["forward"]["active_hist"][:K].ne(0).all())
    for k, g in r["points+clouds"].items():
        assert bool(torch.isfinite(g).all()) and bool(g.reshape(B, -1).abs().amax(dim=1).gt(0).all()), k
