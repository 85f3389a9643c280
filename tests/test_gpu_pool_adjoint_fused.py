"""The max-pool adjoint inside its consumers (ReLU network): every kernel that can stage its gradient operand from the pooled
gradient and the arg-max codes (mmk_conv_bwd_fused_pooled, mmk_conv3x3_wgrad_partial_pooled, mmk_conv_desc.x1_pool_arg) against
the standalone mmk_maxpool2_bwd_arg launch followed by the plain entry point, and the whole backward pass against the
switch-selected standalone path (MMK_UNET_POOL_ADJOINT=0).  Everything is bit-equality: the select is exact."""
import pytest
import torch

from mm_masking_amd import unet_hip as uh
from support import DEV, policy

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
SCALES = [1.0, 1.0 / 0.95]


def _operands(B, H, W, C, seed):
    """A ReLU-like activation x (B,H,W,C), a pooled gradient gy (B,H/2,W/2,C) and the codes of a pre-pool tensor with ties
    (values on a coarse grid), all-zero windows and negative maxima, so that both bits of a code and every position occur."""
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(B, H, W, C, generator=g) * 0.7).clamp_min(0).to(DEV).to(BF16)
    pre = (torch.randn(B, H, W, C, generator=g) * 1.5).round() * 0.5           # ties; about a third of the windows' maxima <= 0
    pre[:, :, :, 0::5] = pre[:, :, :, 0::5].clamp_max(0)                        # channels whose maxima are never positive
    pre[:, :, :, 3::7] = -pre[:, :, :, 3::7].abs() - 0.5                        # ... and strictly negative ones
    pre = pre.to(DEV).to(BF16)
    _, arg = uh.maxpool2_arg(pre)
    gy = (torch.randn(B, H // 2, W // 2, C, generator=g) * 0.3).to(DEV).to(BF16)
    codes = arg.int()
    seen = set(torch.unique(torch.cat([codes & 15, codes >> 4])).tolist())
    assert seen >= {0, 4, 5, 6, 7}, seen                                        # not positive, and positive at each of the 4 positions
    return x, gy, arg


def _eq16(a, b):
    return torch.equal(a.view(torch.int16), b.view(torch.int16))


def _eq32(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def _reduced(part, cout, cin):
    db = torch.zeros(cout, dtype=torch.float32, device=DEV)
    dW = uh.wgrad_unpack_batch([(part, cout, cin, db)])[0]
    return dW, db


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("B,H,W", [(2, 18, 70), (2, 17, 35)])
def test_bwd_fused16_pooled_bit_identical(B, H, W, scale):
    """conv_bwd_fused_kernel<16, 16> (encoder block 1): data gradient and partial slices, and a second application that
    accumulates into the slices."""
    C = 16
    x, gy, arg = _operands(B, H, W, C, 100 + H)
    w = (torch.randn(C, C, 3, 3, generator=torch.Generator().manual_seed(3)) / C).to(DEV)
    wpt = uh.pack_weights(w, transposed=True)
    ns = uh.wgrad_slices(C, C, C, B, H, W)
    assert ns > 0
    gz = uh.maxpool2_bwd_arg(arg, gy, H, W, scale)
    ref_dx, ref_part = torch.empty_like(x), uh.partial_buffer(ns, C, C, DEV)
    uh.conv_bwd_fused(x, gz, wpt, 1.0, ref_dx, ref_part)
    dx, part = torch.full_like(x, 7.0), torch.full_like(ref_part, 3.0)
    uh.conv_bwd_fused(x, gy, wpt, 1.0, dx, part, g_pool_arg=arg, g_pool_scale=scale)
    torch.cuda.synchronize()
    assert _eq16(dx, ref_dx)
    assert _eq32(part, ref_part)
    for p, q in zip(_reduced(part, C, C), _reduced(ref_part, C, C)):
        assert _eq32(p, q)
    uh.conv_bwd_fused(x, gz, wpt, 1.0 / 0.95, ref_dx, ref_part, accumulate=True)
    uh.conv_bwd_fused(x, gy, wpt, 1.0 / 0.95, dx, part, accumulate=True, g_pool_arg=arg, g_pool_scale=scale)
    torch.cuda.synchronize()
    assert _eq16(dx, ref_dx)
    assert _eq32(part, ref_part)


# (channels, B, H, W): the ring kernel and conv3x3_wgrad_kernel<32, 32>; the 8-wave kernels at 64 channels (80- and 48-pixel tile
# rows), at 128 (two output-channel groups of the weight gradient, 4-row tiles) and at 256 (two groups of the data gradient)
CONSUMERS = [(32, 2, 18, 70), (32, 2, 17, 35),
             (64, 2, 20, 88), (64, 2, 9, 83), (64, 2, 20, 44),
             (128, 1, 12, 40), (256, 1, 7, 20)]


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("C,B,H,W", CONSUMERS)
def test_data_gradient_pooled_bit_identical(C, B, H, W, scale):
    """mmk_conv3x3 with x1_pool_arg (conv3x3_ring_kernel<32, 32>, conv3x3_deep_kernel): the ReLU-source form the driver uses,
    and the accumulating form."""
    x, gy, arg = _operands(B, H, W, C, 200 + C + H)
    g = torch.Generator().manual_seed(5)
    w = (torch.randn(C, C, 3, 3, generator=g) / (3 * C ** 0.5)).to(DEV)
    acc0 = (torch.randn(B, H, W, C, generator=g) * 0.2).to(DEV).to(BF16)
    wpt = uh.pack_weights(w, transposed=True)
    gz = uh.maxpool2_bwd_arg(arg, gy, H, W, scale)
    ref = uh.conv3x3(gz, wpt, C, relu_src=x, scale=1.0)
    out = torch.full_like(x, 7.0)
    uh.conv3x3(gy, wpt, C, out=out, relu_src=x, scale=1.0, x1_pool_arg=arg, x1_pool_scale=scale, hw=(H, W))
    ref_acc, out_acc = acc0.clone(), acc0.clone()
    uh.conv3x3(gz, wpt, C, out=ref_acc, accumulate=True)
    uh.conv3x3(gy, wpt, C, out=out_acc, accumulate=True, x1_pool_arg=arg, x1_pool_scale=scale, hw=(H, W))
    torch.cuda.synchronize()
    assert float(ref.float().abs().sum()) > 0
    assert _eq16(out, ref)
    assert _eq16(out_acc, ref_acc)


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("C,B,H,W", CONSUMERS)
def test_weight_gradient_pooled_bit_identical(C, B, H, W, scale):
    """mmk_conv3x3_wgrad_partial_pooled (conv3x3_wgrad_kernel<32, 32>, conv3x3_wgrad_deep_kernel): the partial slices, a second
    application that accumulates, and the reduced dW / db."""
    x, gy, arg = _operands(B, H, W, C, 300 + C + H)
    ns = uh.wgrad_slices(C, C, C, B, H, W)
    assert ns > 0
    gz = uh.maxpool2_bwd_arg(arg, gy, H, W, scale)
    ref_part = uh.partial_buffer(ns, C, C, DEV)
    uh.conv3x3_wgrad_partial(x, gz, C, ref_part)
    part = torch.full_like(ref_part, 3.0)
    uh.conv3x3_wgrad_partial(x, gy, C, part, g_pool_arg=arg, g_pool_scale=scale)
    torch.cuda.synchronize()
    assert float(ref_part.abs().sum()) > 0
    assert _eq32(part, ref_part)
    for p, q in zip(_reduced(part, C, C), _reduced(ref_part, C, C)):
        assert _eq32(p, q)
    uh.conv3x3_wgrad_partial(x, gz, C, ref_part, accumulate=True)
    uh.conv3x3_wgrad_partial(x, gy, C, part, accumulate=True, g_pool_arg=arg, g_pool_scale=scale)
    torch.cuda.synchronize()
    assert _eq32(part, ref_part)


def test_pooled_input_refused_where_no_kernel_stages_it():
    """A layer without pooled staging is an error, not a quiet other path."""
    from mm_masking_amd import _lib
    x, gy, arg = _operands(1, 16, 32, 16, 9)
    w = torch.randn(16, 16, 3, 3, generator=torch.Generator().manual_seed(1)).to(DEV)
    with pytest.raises(_lib.MmkError):
        uh.conv3x3(gy, uh.pack_weights(w, transposed=True), 16, relu_src=x, x1_pool_arg=arg, hw=(16, 32))
    x8 = x[..., :8].contiguous()
    with pytest.raises(_lib.MmkError):
        uh.conv3x3_wgrad_partial(x8, gy, 16, uh.partial_buffer(uh.wgrad_slices(16, 8, 8, 1, 16, 32), 16, 8, DEV), g_pool_arg=arg)


@pytest.mark.parametrize("drop", [0.0, 0.05])
@pytest.mark.parametrize("B,H,W", [(3, 64, 160), (1, 50, 210)])
def test_unet_backward_pooled_adjoint_bit_identical(B, H, W, drop, monkeypatch):
    """mmk_unet_backward: all 46 gradients with the adjoint inside the consumers == with the standalone launch on every level
    (MMK_UNET_POOL_ADJOINT=0), and == a second run.  (1, 50, 210) reaches odd sizes: 25 x 105 at level 1, 3 x 13 at level 4."""
    model = policy(DEV, 11, dropout=drop, amp_dtype=torch.float32, unet_backend="torch")
    model.train()
    g = torch.Generator().manual_seed(1)
    x = torch.rand(B, 1, H, W, generator=g).to(DEV)
    gsel = torch.randn(B, H, W, generator=g).to(DEV)

    def grads():
        model.zero_grad()
        out = uh.unet_mask(model, x, training=True, seed=5)
        (out * gsel).sum().backward()
        torch.cuda.synchronize()
        return [p.grad.clone() for p in uh.param_list(model)]

    monkeypatch.delenv("MMK_UNET_POOL_ADJOINT", raising=False)
    fused, again = grads(), grads()
    monkeypatch.setenv("MMK_UNET_POOL_ADJOINT", "0")
    alone = grads()
    assert len(fused) == 46
    assert all(bool(torch.isfinite(p).all()) for p in fused) and float(fused[2].abs().sum()) > 0     # (encoder block 1 got a gradient)
    for k, (p, q, r) in enumerate(zip(fused, again, alone)):
        assert _eq32(p, q), k
        assert _eq32(p, r), k
