"""GPU: gradients with respect to the point clouds -- the HIP dICP's dL/dsource and dL/dtarget (mmk_icp_backward_points)
against autograd through the CPU restatement, and extract_weights' dL/dscan_pc (mmk_sample_weights_bwd_pc) against
PyTorch's grid_sample autograd; which inputs get gradients, structural zeros, run-to-run bit equality, and that the
weight / pose gradients and the policy's parameter gradients do not change when the clouds also require grad."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from mm_masking_amd import _lib, synthetic
from mm_masking_amd import radar_utils as ru
from mm_masking_amd.dICP.ICP import ICP
from oracle import dicp_ref
from support import DEV, nn_engine, pair_batch  # noqa: F401  (nn_engine: a fixture)

pytestmark = pytest.mark.gpu


def _close(g, ref, name, rel=2e-3):
    g, ref = g.detach().cpu().double().numpy(), ref.detach().double().numpy()
    scale = np.abs(ref).max()
    assert scale > 0, name
    err = np.abs(g - ref).max()
    assert err <= rel * scale, (name, err, scale)


CASES = [("pt2pt", "cauchy", 2), ("pt2pl", "huber", 2), ("pt2pt", "huber", 3), ("pt2pl", "cauchy", 3), ("pt2pl", None, 2)]


@pytest.mark.parametrize("icp_type,loss,dim", CASES)
def test_cloud_gradients_match_autograd(nn_engine, icp_type, loss, dim):
    """All four inputs require grad: source, target (xyz + normals), weight and T_init gradients against autograd through
    the CPU restatement; zero-padded source rows and target_pad_val target rows included."""
    B, n, m, K = 2, 900, 2500, 5
    src, tgt, _ = pair_batch(B, n, m, dim, pad_n=60, pad_m=40, seed=77 + dim)
    rng = np.random.default_rng(2)
    w0 = rng.uniform(0.2, 1.0, (B, n + 60)).astype(np.float32)
    w0[:, n:] = 0.0
    loss_fn = None if loss is None else {"name": loss, "metric": 0.5}
    G = torch.from_numpy(rng.normal(size=(B, 4, 4)).astype(np.float32))
    T0 = torch.eye(4).repeat(B, 1, 1)
    T0[:, 0, 3] += 0.2

    leaves_ref = [torch.from_numpy(x).requires_grad_(True) for x in (src, tgt, w0)] + [T0.clone().requires_grad_(True)]
    ref = dicp_ref.ICPRef(icp_type, differentiable=True, max_iterations=K, tolerance=1e-9)
    out = ref.icp(leaves_ref[0], leaves_ref[1], T_init=leaves_ref[3], weight=leaves_ref[2], trim_dist=3.0, loss_fn=loss_fn, dim=dim)
    (out["T"] * G).sum().backward()

    leaves = [x.detach().to(DEV).requires_grad_(True) for x in leaves_ref]
    icp = ICP(icp_type=icp_type, differentiable=True, max_iterations=K, tolerance=1e-9)
    T = icp.icp(leaves[0], leaves[1], T_init=leaves[3], weight=leaves[2], trim_dist=3.0, loss_fn=loss_fn, dim=dim)["T"]
    (T * G.to(DEV)).sum().backward()
    np.testing.assert_allclose(T.detach().cpu().numpy(), out["T"].detach().numpy(), atol=2e-6)
    for name, g, r in zip(("source", "target", "weight", "T_init"), leaves, leaves_ref):
        _close(g.grad, r.grad, name)


@pytest.mark.parametrize("which", [("source",), ("target",), ("source", "target"), ("source", "target", "weight", "T_init")])
def test_gradients_go_exactly_to_the_inputs_that_require_them(nn_engine, which):
    B, n, m = 2, 600, 1500
    src, tgt, _ = pair_batch(B, n, m, 2, seed=5)
    x = {"source": torch.from_numpy(src).to(DEV), "target": torch.from_numpy(tgt).to(DEV),
         "weight": torch.rand(B, n, device=DEV) + 0.1, "T_init": torch.eye(4, device=DEV).repeat(B, 1, 1)}
    for k in which:
        x[k].requires_grad_(True)
    icp = ICP("pt2pl", differentiable=True, max_iterations=4, tolerance=1e-9)
    T = icp.icp(x["source"], x["target"], T_init=x["T_init"], weight=x["weight"], trim_dist=5.0,
                loss_fn={"name": "huber", "metric": 1.0}, dim=2)["T"]
    assert T.requires_grad
    (T[:, :2, 3].sum() + T[:, 1, 0].sum()).backward()
    for k, t in x.items():
        if k in which:
            assert t.grad is not None and t.grad.shape == t.shape and torch.isfinite(t.grad).all() and t.grad.abs().max() > 0, k
        else:
            assert t.grad is None, k


def test_cloud_gradients_in_the_callers_dtype_and_device(nn_engine):
    """CPU fp64 clouds: the gradients come back as CPU fp64 -- the device fp32 gradients, converted."""
    B, n, m = 2, 500, 1200
    src, tgt, _ = pair_batch(B, n, m, 2, seed=9)
    w = torch.rand(B, n, generator=torch.Generator().manual_seed(1)) + 0.1
    loss_fn = {"name": "cauchy", "metric": 1.0}
    grads = []
    for dev, dt in ((torch.device("cpu"), torch.float64), (DEV, torch.float32)):
        s = torch.from_numpy(src).to(dev, dt).requires_grad_(True)
        t = torch.from_numpy(tgt).to(dev, dt).requires_grad_(True)
        icp = ICP("pt2pl", differentiable=True, max_iterations=4, tolerance=1e-9)
        T = icp.icp(s, t, weight=w.to(dev, dt), trim_dist=5.0, loss_fn=loss_fn, dim=2)["T"]
        assert T.device.type == dev.type
        T[:, :2, 3].sum().backward()
        assert s.grad.dtype == dt and t.grad.dtype == dt and s.grad.device.type == dev.type and t.grad.device.type == dev.type
        grads.append((s.grad, t.grad))
    assert torch.equal(grads[0][0], grads[1][0].cpu().double()) and torch.equal(grads[0][1], grads[1][1].cpu().double())


@pytest.mark.parametrize("icp_type,dim", [("pt2pt", 2), ("pt2pl", 2), ("pt2pt", 3), ("pt2pl", 3)])
def test_structural_zeros(nn_engine, icp_type, dim):
    B, n, m, K = 2, 700, 1800, 4
    src, tgt, _ = pair_batch(B, n, m, dim, pad_n=20, pad_m=50, seed=21)
    s = torch.from_numpy(src).to(DEV).requires_grad_(True)
    t = torch.from_numpy(tgt).to(DEV).requires_grad_(True)
    icp = ICP(icp_type, differentiable=True, max_iterations=K, tolerance=1e-9)
    T = icp.icp(s, t, weight=torch.rand(B, n + 20, device=DEV) + 0.1, trim_dist=5.0, loss_fn={"name": "cauchy", "metric": 1.0},
                dim=dim)["T"]
    idx, active = T.grad_fn.saved_tensors[3], T.grad_fn.saved_tensors[7]
    (T * torch.randn(B, 4, 4, device=DEV)).sum().backward()
    gs, gt = s.grad, t.grad
    if dim == 2:
        assert (gs[..., 2] == 0).all()
    assert (gt[..., dim:3] == 0).all()
    assert (gt[..., 3 + (dim if icp_type == "pt2pl" else 0):] == 0).all()
    for b in range(B):
        used = torch.zeros(t.shape[1], dtype=torch.bool, device=DEV)
        for k in range(K):
            if active[k, b]:
                used[idx[k, b].long()] = True
        assert (~used).any() and (gt[b, ~used] == 0).all()
        assert not used[m:].any()                      # target_pad_val rows are never a correspondent
        assert gt[b, used, :dim].abs().max() > 0


def _hot_target_case():
    """pt2pt, Cauchy: 4 096 source points within 0.5 m of one isolated target, every other target beyond the trim distance."""
    rng = np.random.default_rng(12)
    M, n = 2000, 4096
    tgt = np.zeros((1, M, 3), np.float32)
    tgt[0, 0] = [10.0, -5.0, 0.0]
    ang = rng.uniform(0, 2 * np.pi, M - 1)
    rad = rng.uniform(30.0, 60.0, M - 1)
    tgt[0, 1:, 0], tgt[0, 1:, 1] = 10.0 + rad * np.cos(ang), -5.0 + rad * np.sin(ang)
    src = np.zeros((1, n, 3), np.float32)
    r, a = 0.45 * np.sqrt(rng.uniform(0, 1, n)), rng.uniform(0, 2 * np.pi, n)
    src[0, :, 0], src[0, :, 1] = 10.0 + r * np.cos(a), -5.0 + r * np.sin(a)
    w = rng.uniform(0.2, 1.0, (1, n)).astype(np.float32)
    return src, tgt, w


def test_hot_target_matches_oracle_and_backward_is_reproducible(nn_engine):
    src, tgt, w = _hot_target_case()
    K, loss_fn = 5, {"name": "cauchy", "metric": 1.0}
    G = torch.from_numpy(np.random.default_rng(3).normal(size=(1, 4, 4)).astype(np.float32))
    sr, tr = torch.from_numpy(src).requires_grad_(True), torch.from_numpy(tgt).requires_grad_(True)
    ref = dicp_ref.ICPRef("pt2pt", differentiable=True, max_iterations=K, tolerance=1e-9)
    out = ref.icp(sr, tr, weight=torch.from_numpy(w), trim_dist=5.0, loss_fn=loss_fn, dim=2)
    (out["T"] * G).sum().backward()
    runs = []
    for rep in range(2):
        s = torch.from_numpy(src).to(DEV).requires_grad_(True)
        t = torch.from_numpy(tgt).to(DEV).requires_grad_(True)
        wg = torch.from_numpy(w).to(DEV).requires_grad_(True)
        icp = ICP("pt2pt", differentiable=True, max_iterations=K, tolerance=1e-9)
        T = icp.icp(s, t, weight=wg, trim_dist=5.0, loss_fn=loss_fn, dim=2)["T"]
        assert (T.grad_fn.saved_tensors[3] == 0).all()          # every point of every iteration on target 0
        (T * G.to(DEV)).sum().backward()
        runs.append((s.grad, t.grad, wg.grad))
    for a, b in zip(runs[0], runs[1]):
        assert torch.equal(a, b)
    _close(runs[0][0], sr.grad, "source")
    _close(runs[0][1], tr.grad, "target")
    assert (runs[0][1][0, 1:] == 0).all()


def test_backward_is_bit_reproducible(nn_engine):
    B, n, m = 3, 1200, 3000
    src, tgt, _ = pair_batch(B, n, m, 2, pad_n=200, seed=33)
    w = torch.rand(B, n + 200, generator=torch.Generator().manual_seed(2)).to(DEV)
    runs = []
    for rep in range(2):
        x = [torch.from_numpy(src).to(DEV), torch.from_numpy(tgt).to(DEV), w.clone(), torch.eye(4, device=DEV).repeat(B, 1, 1)]
        for v in x:
            v.requires_grad_(True)
        icp = ICP("pt2pl", differentiable=True, max_iterations=6, tolerance=1e-9)
        T = icp.icp(x[0], x[1], T_init=x[3], weight=x[2], trim_dist=5.0, loss_fn={"name": "huber", "metric": 1.0}, dim=2)["T"]
        T[:, :2, 3].sum().backward()
        runs.append([v.grad for v in x])
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_weight_and_pose_gradients_untouched_by_cloud_gradients(nn_engine):
    """weight.grad and T_init.grad are the same bits whether or not the clouds also require grad, and the new entry with
    NULL point outputs is bit-identical to mmk_icp_backward."""
    B, n, m, dim = 2, 800, 2000, 2
    src, tgt, _ = pair_batch(B, n, m, dim, pad_n=40, seed=51)
    w = torch.rand(B, n + 40, generator=torch.Generator().manual_seed(5)).to(DEV)
    loss_fn = {"name": "huber", "metric": 1.0}
    grads = []
    for clouds in (False, True):
        s, t = torch.from_numpy(src).to(DEV).requires_grad_(clouds), torch.from_numpy(tgt).to(DEV).requires_grad_(clouds)
        wg, T0 = w.clone().requires_grad_(True), torch.eye(4, device=DEV).repeat(B, 1, 1).requires_grad_(True)
        icp = ICP("pt2pl", differentiable=True, max_iterations=5, tolerance=1e-9)
        T = icp.icp(s, t, T_init=T0, weight=wg, trim_dist=5.0, loss_fn=loss_fn, dim=dim)["T"]
        saved = T.grad_fn.saved_tensors                # weight, src, tgt, idx, T_hist, delta, A, active
        (T * torch.arange(16.0, device=DEV).reshape(4, 4)).sum().backward()
        grads.append((wg.grad, T0.grad))
    assert torch.equal(grads[0][0], grads[1][0]) and torch.equal(grads[0][1], grads[1][1])

    p = icp._params(B, n + 40, m, 6, dim, loss_fn, 5.0, save_state=True)
    L = _lib.lib()
    gT = torch.randn(B, 4, 4, device=DEV)
    st = _lib.stream_ptr(DEV)
    outs = []
    for new in (False, True):
        gw, gT0 = torch.empty(B, n + 40, device=DEV), torch.empty(B, 4, 4, device=DEV)
        args = [_lib.ptr(v) for v in (saved[1], saved[2], saved[0]) + tuple(saved[3:8]) + (gT, gw, gT0)]
        if new:
            ws = torch.empty(L.mmk_icp_backward_points_workspace_bytes(ctypes.byref(p), 0), dtype=torch.uint8, device=DEV)
            null = ctypes.c_void_p(0)
            _lib.check(L.mmk_icp_backward_points(ctypes.byref(p), *args, null, null, _lib.ptr(ws), ws.numel(), st))
        else:
            ws = torch.empty(L.mmk_icp_workspace_bytes(ctypes.byref(p)), dtype=torch.uint8, device=DEV)
            _lib.check(L.mmk_icp_backward(ctypes.byref(p), *args, _lib.ptr(ws), ws.numel(), st))
        torch.cuda.synchronize()
        outs.append((gw, gT0))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


def _ref_extract_weights(mask, pc):
    """radar_utils.py:108-128 on the CPU: point_to_cart_idx(min_to_plus_1=True), fake rows at -100, grid_sample."""
    gu = -pc[:, :, 0] / 0.2384
    gv = pc[:, :, 1] / 0.2384
    grid = torch.stack((gv, gu), dim=2) / (640 - 1) * 2
    fake = (pc[:, :, 0] == 0.0) & (pc[:, :, 1] == 0.0)
    grid = torch.where(fake[..., None], torch.full_like(grid, -100.0), grid)
    w = F.grid_sample(mask.unsqueeze(1), grid.unsqueeze(2), mode="bilinear", padding_mode="zeros", align_corners=True)
    return w.squeeze(1).squeeze(-1)


@pytest.mark.parametrize("H,W", [(640, 640), (400, 3360), (40, 96)])
def test_extract_weights_point_gradient(H, W):
    g = torch.Generator().manual_seed(H + W)
    B, N = 2, 3000
    mask = torch.rand(B, H, W, generator=g)
    pc = torch.zeros(B, N, 3)
    pc[:, :, :2] = (torch.rand(B, N, 2, generator=g) - 0.5) * 170.0        # +-85 m: some beyond the image (76 m)
    pc[:, :, 2] = torch.rand(B, N, generator=g)
    k = torch.arange(-300, 300, 12, dtype=torch.float32)
    pc[:, :50, 1] = (k + 0.5) * 0.2384                                      # on pixel edges (640-pixel grid)
    pc[:, 50:100, 0] = -(k + 0.5) * 0.2384
    pc[:, 100:104, :2] = torch.tensor([[0.0, 319.5 * 0.2384], [0.0, -319.5 * 0.2384],      # on the image border
                                       [319.5 * 0.2384, 0.0], [-319.5 * 0.2384, 1.0]])
    pc[:, 104:110, :2] = torch.tensor([[500.0, 0.0], [0.0, -500.0], [80.0, 80.0], [-77.0, 0.5], [0.5, 76.5], [-76.3, -76.3]])
    pc[:, 110:130, :2] = 0.0                                                # fake rows (z != 0 does not matter)
    pc[:, 130, 0] = 0.0                                                     # x == 0 alone is a real point
    gw = torch.randn(B, N, generator=g)

    m_ref, p_ref = mask.clone().requires_grad_(True), pc.clone().requires_grad_(True)
    (_ref_extract_weights(m_ref, p_ref) * gw).sum().backward()

    m_g, p_g = mask.to(DEV).requires_grad_(True), pc.to(DEV).requires_grad_(True)
    (ru.extract_weights(m_g, p_g)[0] * gw.to(DEV)).sum().backward()
    gp = p_g.grad.cpu()
    scale = p_ref.grad.abs().max()
    assert scale > 0
    assert (gp - p_ref.grad).abs().max() <= 1e-5 * scale, float((gp - p_ref.grad).abs().max() / scale)
    assert (gp[..., 2] == 0).all() and (gp[:, 110:130] == 0).all()
    # the mask gradient is the same bits as without point gradients
    m2 = mask.to(DEV).requires_grad_(True)
    (ru.extract_weights(m2, pc.to(DEV))[0] * gw.to(DEV)).sum().backward()
    assert torch.equal(m_g.grad, m2.grad)


def test_policy_passes_gradients_to_the_clouds():
    """LearnICPWeightPolicy: raw_pc gets its gradient through the weights, filtered_pc and the map through the ICP; the loss
    and every parameter gradient are the same bits as without cloud gradients (dropout 0)."""
    from mm_masking_amd.icp_weight_policy import LearnICPWeightPolicy
    from mm_masking_amd.train_icp_weights import default_params, eval_training_loss, loss_weights_from, prepare_batch
    params = default_params(DEV)
    params.update({"icp_type": "pt2pl", "icp_loss_fn": {"name": "huber", "metric": 1.0}, "dropout": 0.0, "max_iter": 4})
    raw = synthetic.make_batch([0, 1], device=DEV, m_valid=3000, m_pad=3072, density="sparse")
    batch = prepare_batch(raw, params, max_loc_pts=2048)

    def run(clouds):
        torch.manual_seed(0)
        model = LearnICPWeightPolicy(params).to(DEV)
        model.train()
        scan, mp = dict(batch["loc_data"]), dict(batch["map_data"])
        pcs = [scan["raw_pc"].clone(), scan["filtered_pc"].clone(), mp["pc"].clone()]
        for v in pcs:
            v.requires_grad_(clouds)
        scan["raw_pc"], scan["filtered_pc"], mp["pc"] = pcs
        T_pred, mask, num_non0 = model(scan, mp, batch["transforms"]["T_ml_init"])
        loss, _ = eval_training_loss(T_pred, mask, num_non0, batch["transforms"]["T_ml_gt"], scan, mp, model,
                                     loss_weights=loss_weights_from(params))
        loss.backward()
        return loss.detach(), [p.grad for p in model.parameters()], pcs

    loss0, g0, _ = run(False)
    loss1, g1, pcs = run(True)
    assert torch.equal(loss0, loss1)
    assert len(g0) == len(g1) and all((a is None and b is None) or torch.equal(a, b) for a, b in zip(g0, g1))
    for name, v in zip(("raw_pc", "filtered_pc", "map_pc"), pcs):
        assert v.grad is not None and torch.isfinite(v.grad).all() and v.grad.abs().max() > 0, name
