"""Batch-norm variant of the mask U-Net (params["batch_norm"], icp_weight_policy.py:108-113) on the hand-written
kernels: the BatchNorm kernels against torch's, and the whole network against the reference module's golden mask,
per-tensor gradient vectors and running statistics (tests/golden/make_golden_r2.py, tag n)."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from mm_masking_amd import train_icp_weights as trn
from mm_masking_amd import unet_hip_bn as ub
from mm_masking_amd.icp_weight_policy import LearnICPWeightPolicy
from support import DEV, _Q, nchw

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("B,H,W,C,drop", [(2, 24, 40, 8, 0.0), (3, 17, 23, 32, 0.2), (2, 9, 11, 256, 0.0)])
def test_bn_kernels_against_torch(B, H, W, C, drop):
    g = torch.Generator().manual_seed(C)
    a32 = F.relu(torch.randn(B, C, H, W, generator=g) * 1.5 + 0.3)
    a = a32.permute(0, 2, 3, 1).contiguous().to(torch.bfloat16).to(DEV)
    bn = torch.nn.BatchNorm2d(C).to(DEV)
    with torch.no_grad():
        bn.weight.copy_(torch.rand(C, generator=g) + 0.5)
        bn.bias.copy_(torch.randn(C, generator=g) * 0.2)
    ref = torch.nn.BatchNorm2d(C).to(DEV)
    ref.load_state_dict(bn.state_dict())
    bn.train(), ref.train()
    y, stat, affine = ub._bn_forward(a, bn, bn.weight.detach(), bn.bias.detach(), True, drop, 5)
    ar = a.float().permute(0, 3, 1, 2).requires_grad_(True)
    yr = ref(ar)
    keep = (y.float() != 0) | (torch.signbit(y.float()))            # dropped = +0.0
    scale = ub.uh.dropout_scale(drop)
    want = (yr.permute(0, 2, 3, 1) * scale).detach()
    assert (keep.float().mean().item() > 0.99) if drop == 0 else abs(keep.float().mean().item() - (1 - drop)) < 0.03
    assert ((y.float() - want)[keep]).abs().max().item() < 0.03 + 0.01 * want.abs().max().item()          # bf16 output
    np.testing.assert_allclose(bn.running_mean.cpu().numpy(), ref.running_mean.cpu().numpy(), rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(bn.running_var.cpu().numpy(), ref.running_var.cpu().numpy(), rtol=1e-4, atol=1e-5)
    assert int(bn.num_batches_tracked) == 1
    # backward: gradient w.r.t. the conv pre-activation z (a = relu(z)), dgamma, dbeta
    gd = torch.randn(B, H, W, C, generator=g).to(torch.bfloat16).to(DEV)
    dgamma, dbeta = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
    gz = ub._bn_backward(gd, y, scale, a, stat, affine, bn.weight.detach(), 0.0, dgamma, dbeta, False)
    gy = gd.float() * keep.float() * scale
    yr.backward(gy.permute(0, 3, 1, 2))
    want_gz = (ar.grad * (ar > 0)).permute(0, 2, 3, 1)
    assert (gz.float() - want_gz).abs().max().item() < 0.03 + 0.01 * want_gz.abs().max().item()
    np.testing.assert_allclose(dgamma.cpu().numpy(), ref.weight.grad.cpu().numpy(), rtol=2e-3, atol=2e-3 * float(ref.weight.grad.abs().max()))
    np.testing.assert_allclose(dbeta.cpu().numpy(), ref.bias.grad.cpu().numpy(), rtol=2e-3, atol=2e-3 * float(ref.bias.grad.abs().max()))
    # evaluation mode: running statistics
    bn.eval(), ref.eval()
    y2, stat2, _ = ub._bn_forward(a, bn, bn.weight.detach(), bn.bias.detach(), False)
    assert stat2 is None
    assert (y2.float() - ref(a.float().permute(0, 3, 1, 2)).permute(0, 2, 3, 1)).abs().max().item() < 0.03 + 0.01 * float(y2.float().abs().max())


def _bn_train(a, bn_w, bn_b, eps=1e-5):
    mean = a.mean(dim=(0, 2, 3), keepdim=True)
    var = a.var(dim=(0, 2, 3), unbiased=False, keepdim=True)
    return (a - mean) / torch.sqrt(var + eps) * bn_w.view(1, -1, 1, 1) + bn_b.view(1, -1, 1, 1)


@pytest.mark.parametrize("B,H,W,drop,leaky", [(2, 64, 64, 0.0, False), (3, 96, 64, 0.1, False), (2, 64, 96, 0.05, True)])
def test_batch_norm_network_on_pinned_activations(B, H, W, drop, leaky):
    """The whole batch-norm network, layer by layer on the tensors the HIP path itself stored (so that bf16
    differences do not compound through 22 BatchNorms over a handful of pixels), then every parameter gradient
    against autograd through an fp32 graph whose forward values are pinned to the HIP activations (the technique
    of test_gpu_unet_kernels.py::test_unet_hip_backward_exact_on_pinned_activations)."""
    p = trn.default_params(DEV)
    p.update({"dropout": drop, "batch_norm": True, "leaky": leaky, "norm_weights": False})
    torch.manual_seed(5)
    model = LearnICPWeightPolicy(p).to(DEV)
    model.train()
    with torch.no_grad():       # non-trivial affine parameters
        for m_ in model.modules():
            if isinstance(m_, torch.nn.BatchNorm2d):
                m_.weight.uniform_(0.5, 1.5)
                m_.bias.uniform_(-0.3, 0.3)
    g = torch.Generator().manual_seed(1)
    x = torch.rand(B, 1, H, W, generator=g).to(DEV)
    gsel = torch.randn(B, H, W, generator=g).to(DEV)
    slope = 0.1 if leaky else 0.0
    ub.uh.DEBUG = {}
    try:
        out = ub.unet_mask(model, x, training=True, seed=3, norm=False, slope=slope)
        (out * gsel).sum().backward()
        fwd = ub.uh.DEBUG["fwd_bn"]
    finally:
        ub.uh.DEBUG = None
    got = {n: q.grad.clone() for n, q in model.named_parameters()}
    model.zero_grad()
    act = (lambda t: F.leaky_relu(t, 0.1)) if leaky else F.relu
    sd_scale = ub.uh.dropout_scale(drop)
    blocks = list(model.encoder) + list(model.decoder)
    q = _Q.apply

    def pin(ref, mine_nhwc):
        mine = nchw(mine_nhwc)
        return q(ref + (mine - ref).detach())

    def conv(t, m):
        return F.conv2d(t, m.weight.to(torch.bfloat16).float(), m.bias, padding=1)

    def run_block(k, key, xin):
        x1, x2, aA, yA, aB, d, sA, afA, sB, afB = fwd["saved"][key]
        blk = blocks[k]
        zA = conv(xin, blk[0])
        aA_ref = act(zA)
        assert (aA_ref - nchw(aA)).abs().max().item() < 0.03 + 0.01 * aA_ref.abs().max().item(), (key, "conv A")
        # activation factor taken from the stored tensor, as the HIP adjoint does
        fA = torch.where(nchw(aA) > 0, 1.0, slope) if leaky else (nchw(aA) > 0).float()
        aA_p = q(zA * fA + (nchw(aA) - zA * fA).detach())
        yA_ref = _bn_train(aA_p, blk[2].weight, blk[2].bias)
        assert (yA_ref - nchw(yA)).abs().max().item() < 0.04 + 0.01 * yA_ref.abs().max().item(), (key, "BN A")
        yA_p = pin(yA_ref, yA)
        zB = conv(yA_p, blk[3])
        aB_ref = act(zB)
        assert (aB_ref - nchw(aB)).abs().max().item() < 0.03 + 0.01 * aB_ref.abs().max().item(), (key, "conv B")
        fB = torch.where(nchw(aB) > 0, 1.0, slope) if leaky else (nchw(aB) > 0).float()
        aB_p = q(zB * fB + (nchw(aB) - zB * fB).detach())
        yB_ref = _bn_train(aB_p, blk[5].weight, blk[5].bias)
        keep = ((nchw(d) != 0) | torch.signbit(nchw(d))).float()
        d_ref = yB_ref * keep * sd_scale
        assert ((d_ref - nchw(d)).abs() * keep).max().item() < 0.05 + 0.01 * d_ref.abs().max().item(), (key, "BN B")
        return pin(d_ref, d)

    xb = x.to(torch.bfloat16).float()
    t = [run_block(0, ("e", 0), xb)]
    for i in range(1, 6):
        t.append(F.max_pool2d(run_block(i, ("e", i), t[i - 1]), 2, 2))
    cur = t[5]
    for j in range(5):
        skip = t[4 - j]
        u = q(F.interpolate(cur, size=skip.shape[2:], mode="bilinear", align_corners=True))
        u = pin(u, fwd["saved"][("d", j, 0)][0])
        d1 = run_block(6 + j, ("d", j, 0), u)
        cur = run_block(6 + j, ("d", j, 1), torch.cat([skip, d1], 1))
    fl = model.final_layer[0]
    ref = torch.sigmoid(F.conv2d(cur, fl.weight.to(torch.bfloat16).float(), fl.bias)).squeeze(1)
    assert (out - ref).abs().max().item() < 2e-3
    (ref * gsel).sum().backward()
    worst = (0.0, None)
    for n, qp in model.named_parameters():
        rel = ((got[n] - qp.grad).norm() / (qp.grad.norm() + 1e-12)).item()
        if rel > worst[0]:
            worst = (rel, n)
    assert worst[0] < 0.08, worst


def test_batch_norm_network_golden(golden_dir):
    gv = np.load(os.path.join(golden_dir, "unet_grads.npz"), allow_pickle=False)
    p = trn.default_params(DEV)
    p.update({"dropout": 0.0, "batch_norm": True})
    torch.manual_seed(1234)
    model = LearnICPWeightPolicy(p).to(DEV)
    model.train()
    assert list(model.state_dict().keys()) == [str(k) for k in gv["sd_names_n"]]         # checkpoint compatibility
    H = 64
    xin = np.random.default_rng(99).uniform(0.01, 1, size=(2, H, H)).astype(np.float32)
    scan = {"fft_data": torch.from_numpy(xin), "fft_cfar": torch.zeros(2, H, H), "raw_pc": torch.zeros(2, 4, 3)}
    m = model(scan, {"pc": torch.zeros(2, 4, 6)}, None, mask_only=True)
    # At 64 x 64 and B = 2 the deep BatchNorms normalise over 8..128 values, some channels nearly dead
    # (variance ~1e-4 at random init): an element that is 0.02 in fp32 and 0 in bf16 moves its normalised value
    # by O(1), and 22 such layers follow each other -- the fp32 golden mask cannot be reproduced by a bf16
    # network here (the CPU mirror reproduces it to 2e-6: tests/test_policy_cpu.py).  What is compared with the
    # golden: the first block (statistics over 8 192 values) and the bookkeeping; the kernels and the whole
    # schedule are checked layer by layer in test_batch_norm_network_on_pinned_activations.
    gsel = torch.from_numpy(np.random.default_rng(97).normal(size=(2, H, H)).astype(np.float32)).to(DEV)
    (m * gsel).sum().backward()
    names = [str(n) for n in gv["names_n"]]
    assert names == [k for k, _ in model.named_parameters()]
    assert all(q.grad is not None and torch.isfinite(q.grad).all() for q in model.parameters())
    assert float((m.detach().cpu() - torch.from_numpy(gv["mask_n"])).abs().mean()) < 0.25
    sd = model.state_dict()
    np.testing.assert_allclose(sd["encoder.0.2.running_mean"].cpu().numpy(), gv["rm_enc0_n"], rtol=2e-2, atol=2e-3)
    np.testing.assert_allclose(sd["encoder.0.2.running_var"].cpu().numpy(), gv["rv_enc0_n"], rtol=2e-2, atol=2e-3)
    assert int(sd["decoder.4.5.num_batches_tracked"]) == int(gv["nbt_dec4b_n"]) == 2
    # evaluation mode runs on the running statistics, and a training step with dropout + leaky works end to end
    model.eval()
    with torch.no_grad():
        me = model(scan, {"pc": torch.zeros(2, 4, 6)}, None, mask_only=True)
    assert torch.isfinite(me).all() and float(me.max()) == pytest.approx(1.0, abs=1e-6)
    p2 = dict(p, dropout=0.1, leaky=True)
    m2 = LearnICPWeightPolicy(p2).to(DEV)
    m2.train()
    out = m2(scan, {"pc": torch.zeros(2, 4, 6)}, None, mask_only=True)
    out.sum().backward()
    assert all(q.grad is not None and torch.isfinite(q.grad).all() for q in m2.parameters())
