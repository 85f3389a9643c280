"""GPU: the HIP dICP's reverse sweep through FROZEN pairs (||delta|| < tolerance: the pose is carried forward, the later
iterations do nothing) and through DEGENERATE pairs (A not positive definite: delta = 0, no dependence), against autograd
through the CPU restatement.  The shared cases and the conditions that make them meaningful are in tests/icp_freeze_cases.py.

Every gradient is compared PER PAIR, max|got_b - ref_b| <= 2e-3 * max|ref_b| (the dICP backward's ceiling), so
that a wrong pair cannot hide behind a pair with a larger gradient.  Each comparison prints its ratios before it asserts
(pytest -s: lines "PER-PAIR RATIO ..." and "DEGENERATE ..."); DESIGN.md 6b says what has been measured."""
import ctypes

import numpy as np
import pytest
import torch

import icp_freeze_cases as fc
from mm_masking_amd import _lib
from mm_masking_amd.dICP.ICP import ICP
from support import DEV, nn_engine  # noqa: F401  (nn_engine: a fixture)

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _both_engines(nn_engine):  # noqa: F811
    """Every test of this file runs with both nearest-neighbour engines."""


def _leaves(arrays, need, with_weight=True, pairs=slice(None)):
    src, tgt, w, T0, G = arrays
    x = {"source": torch.from_numpy(src[pairs]).to(DEV), "target": torch.from_numpy(tgt[pairs]).to(DEV),
         "weight": torch.from_numpy(w[pairs]).to(DEV) if with_weight else None, "T_init": torch.from_numpy(T0[pairs]).to(DEV)}
    for name in need:
        x[name].requires_grad_(True)
    return x, torch.from_numpy(G[pairs]).to(DEV)


def _run(c, x, n_iter):
    icp = ICP(icp_type=c["icp_type"], differentiable=True, max_iterations=n_iter, tolerance=c["tol"])
    return icp.icp(x["source"], x["target"], T_init=x["T_init"], weight=x["weight"], trim_dist=fc.TRIM,
                   loss_fn=fc.loss_dict(c["loss"]), dim=c["dim"])["T"]


def _check_forward_state(c, T, n_iter):
    """active_hist is the oracle's schedule; frozen (k, b): delta exactly 0 and the pose carried forward bit for bit; active
    (k, b): the oracle's correspondences; pose within 2e-6.  -> active (n_iter, B) bool."""
    idx, T_hist, delta, _, active = (t.cpu().numpy() for t in T.grad_fn.saved_tensors[3:8])     # after weight, src, tgt
    want = c["active"]
    n_pairs, n_pts = want.shape[1], c["arrays"][0].shape[1]
    # (the order of _IcpFunction's save_for_backward is a private detail: say so if it ever changes)
    assert idx.dtype == np.int32 and idx.shape == (n_iter, n_pairs, n_pts), "saved_tensors[3] is not idx_hist"
    assert T_hist.dtype == np.float32 and T_hist.shape == (n_iter + 1, n_pairs, 16), "saved_tensors[4] is not T_hist"
    assert delta.dtype == np.float64 and delta.shape == (n_iter, n_pairs, 6), "saved_tensors[5] is not delta_hist"
    assert active.dtype == np.int32 and active.shape == (n_iter + 1, n_pairs), "saved_tensors[7] is not active_hist"
    np.testing.assert_array_equal(active[:n_iter], want)
    for k in range(n_iter):
        for b in range(want.shape[1]):
            if want[k, b]:
                np.testing.assert_array_equal(idx[k, b], c["hist"]["idx"][k][b].numpy(), err_msg="iteration %d pair %d" % (k, b))
            else:
                assert (delta[k, b] == 0).all(), (k, b)
                assert T_hist[k + 1, b].tobytes() == T_hist[k, b].tobytes(), (k, b)
    np.testing.assert_allclose(T.detach().cpu().numpy(), c["T"].numpy(), atol=2e-6)
    return want.astype(bool)


def _compare(c, grads, names, label, pairs=None):
    for name in names:
        ratios = fc.pair_ratios(grads[name], c["grads"][name])
        print("PER-PAIR RATIO %s %s/%s/dim%d %s %s: %s" % (label, c["icp_type"], c["loss"], c["dim"], ICP.NN_SEARCH_OVERRIDE, name,
                                                           " ".join("%.3e" % r for r in ratios)))
    for name in names:
        fc.assert_close_per_pair(grads[name], c["grads"][name], name, pairs=pairs)


@pytest.mark.parametrize("icp_type,loss,dim", fc.CASES)
def test_frozen_pairs_gradients_match_autograd_per_pair(icp_type, loss, dim):
    """Three pairs that freeze at different iterations of K = 8 (training builds its ICP with tolerance 1e-5, so frozen
    iterations are in every well-converged batch): forward state against the oracle, the four gradients per pair, and two
    backward runs over the same saved state bit-identical."""
    c = fc.frozen_case(icp_type, loss, dim)
    x, G = _leaves(c["arrays"], fc.INPUTS)
    T = _run(c, x, fc.K)
    frozen = ~_check_forward_state(c, T, fc.K)
    assert frozen.any() and not frozen[0].any()
    order = list(fc.INPUTS)
    runs = [torch.autograd.grad((T * G).sum(), [x[n] for n in order], retain_graph=True) for _ in range(2)]
    for name, a, b in zip(order, *runs):
        assert torch.equal(a, b), name
    _compare(c, dict(zip(order, runs[0])), order, "frozen")


def test_backward_never_reads_idx_rows_of_frozen_iterations():
    """Through the C ABI: mmk_icp_forward(save_state=1) leaves the idx_hist rows of frozen (k, b) unwritten (the Python side
    allocates the buffer uninitialised); mmk_icp_backward_points and mmk_icp_backward give the same bits whatever those rows
    hold.  The rows are overwritten with OTHER VALID indices in [0, M) only, so that even a kernel that did read them could
    not leave the target."""
    c = fc.frozen_case("pt2pl", "huber", 2)
    src, tgt, w, T0, G = (torch.from_numpy(a).to(DEV) for a in c["arrays"])
    B, N, M, K = src.shape[0], src.shape[1], tgt.shape[1], fc.K
    icp = ICP("pt2pl", differentiable=True, max_iterations=K, tolerance=c["tol"])
    p = icp._params(B, N, M, 6, 2, fc.loss_dict("huber"), fc.TRIM, save_state=True)
    L = _lib.lib()
    st = _lib.stream_ptr(DEV)
    ws = torch.empty(L.mmk_icp_workspace_bytes(ctypes.byref(p)), dtype=torch.uint8, device=DEV)
    idx = torch.zeros(K, B, N, dtype=torch.int32, device=DEV)           # (a valid index wherever the forward writes nothing)
    T_hist = torch.empty(K + 1, B, 16, device=DEV)
    delta = torch.empty(K, B, 6, dtype=torch.float64, device=DEV)
    A = torch.empty(K, B, 36, dtype=torch.float64, device=DEV)
    active = torch.empty(K + 1, B, dtype=torch.int32, device=DEV)
    T_out = torch.empty(B, 16, device=DEV)
    _lib.check(L.mmk_icp_forward(ctypes.byref(p), _lib.ptr(src), _lib.ptr(tgt), _lib.ptr(w), _lib.ptr(T0), _lib.ptr(T_out),
                                 _lib.ptr(idx), _lib.ptr(T_hist), _lib.ptr(delta), _lib.ptr(A), _lib.ptr(active), _lib.ptr(ws),
                                 ws.numel(), None, st))
    torch.cuda.synchronize()
    act = active[:K].cpu().numpy()
    np.testing.assert_array_equal(act, c["active"])
    assert (act == 0).sum() >= 2
    np.testing.assert_allclose(T_out.view(B, 4, 4).cpu().numpy(), c["T"].numpy(), atol=2e-6)

    def backward(idx_t):
        state = [_lib.ptr(t) for t in (src, tgt, w, idx_t, T_hist, delta, A, active, G)]
        gw, gT0 = torch.empty(B, N, device=DEV), torch.empty(B, 16, device=DEV)
        gs, gt = torch.empty(B, N, 3, device=DEV), torch.empty(B, M, 6, device=DEV)
        wp = torch.empty(L.mmk_icp_backward_points_workspace_bytes(ctypes.byref(p), 1), dtype=torch.uint8, device=DEV)
        _lib.check(L.mmk_icp_backward_points(ctypes.byref(p), *state, _lib.ptr(gw), _lib.ptr(gT0), _lib.ptr(gs), _lib.ptr(gt),
                                             _lib.ptr(wp), wp.numel(), st))
        gw2, gT02 = torch.empty(B, N, device=DEV), torch.empty(B, 16, device=DEV)
        _lib.check(L.mmk_icp_backward(ctypes.byref(p), *state, _lib.ptr(gw2), _lib.ptr(gT02), _lib.ptr(ws), ws.numel(), st))
        torch.cuda.synchronize()
        return {"weight": gw, "T_init": gT0, "source": gs, "target": gt, "weight (mmk_icp_backward)": gw2,
                "T_init (mmk_icp_backward)": gT02}

    first = backward(idx)
    other = idx.clone()
    fill = ((7919 * torch.arange(N, dtype=torch.int64) + 13) % M).to(torch.int32).to(DEV)
    n_changed = 0
    for k in range(K):
        for b in range(B):
            if act[k, b] == 0:
                other[k, b] = (fill + 101 * (k * B + b)) % M
                n_changed += int((other[k, b] != idx[k, b]).sum())
    assert n_changed > 0 and int(other.min()) >= 0 and int(other.max()) < M
    second = backward(other)
    for name in first:
        assert torch.isfinite(first[name]).all() and first[name].abs().max() > 0, name
        assert torch.equal(first[name], second[name]), name
    # and the state as the forward left it gives the oracle's gradients
    _compare(c, {n: first[n].view(c["grads"][n].shape) for n in fc.INPUTS}, fc.INPUTS, "C ABI")


@pytest.mark.parametrize("icp_type,loss,dim", fc.DEGENERATE_CASES)
def test_degenerate_pairs_stay_inert_in_the_backward(icp_type, loss, dim):
    """tolerance 0, so nothing freezes and the 'A is not positive definite -> delta = 0, no dependence' branch of the
    reverse sweep runs with the pair ACTIVE: pair 0 has only zero weights, pair 2 has every point beyond trim_dist (T_init
    moved by 100 m), pair 1 is ordinary and must not notice its neighbours."""
    c = fc.degenerate_case(icp_type, loss, dim)
    n_iter = fc.K_DEGENERATE
    x, G = _leaves(c["arrays"], fc.INPUTS)
    T = _run(c, x, n_iter)
    assert _check_forward_state(c, T, n_iter).all()
    delta = T.grad_fn.saved_tensors[5]
    (T * G).sum().backward()
    grads = {name: x[name].grad for name in fc.INPUTS}
    for b in (0, 2):
        assert torch.equal(T[b].detach(), x["T_init"][b].detach()), b
        assert (delta[:, b] == 0).all(), b
        for name in ("weight", "source", "target"):
            assert (grads[name][b] == 0).all(), (name, b)
        print("DEGENERATE %s/%s/dim%d %s pair %d: grad_T_init bit-equal to G: %s" % (
            icp_type, loss, dim, ICP.NN_SEARCH_OVERRIDE, b, bool(torch.equal(grads["T_init"][b], G[b]))))
    _compare(c, grads, ["T_init"], "degenerate")
    _compare(c, grads, ["source", "target", "weight"], "degenerate", pairs=[1])
    # the ordinary pair alone, B = 1: the same bits
    x1, G1 = _leaves(c["arrays"], fc.INPUTS, pairs=slice(1, 2))
    T1 = _run(c, x1, n_iter)
    (T1 * G1).sum().backward()
    assert torch.equal(T1[0].detach(), T[1].detach())
    for name in fc.INPUTS:
        assert torch.equal(x1[name].grad[0], grads[name][1]), name


def test_weight_none_with_gradients_elsewhere():
    """weight=None while T_init and the clouds require grad (frozen pt2pl / huber / dim 2 case): the same bits as an explicit
    all-ones weight that does not require grad, and the oracle's gradients per pair."""
    c = fc.frozen_case("pt2pl", "huber", 2, with_weight=False)
    need = ("source", "target", "T_init")
    out = []
    for with_weight in (False, True):                  # c["arrays"] carries the all-ones weight
        x, G = _leaves(c["arrays"], need, with_weight=with_weight)
        assert with_weight == (x["weight"] is not None) and (x["weight"] is None or not x["weight"].requires_grad)
        T = _run(c, x, fc.K)
        frozen = ~_check_forward_state(c, T, fc.K)
        assert frozen.any()
        (T * G).sum().backward()
        out.append((T.detach(), {name: x[name].grad for name in need}))
    assert torch.equal(out[0][0], out[1][0])
    for name in need:
        assert torch.equal(out[0][1][name], out[1][1][name]), name
    _compare(c, out[0][1], need, "weight=None")
