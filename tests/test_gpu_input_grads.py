"""The gradient of the mask U-Net with respect to its input image: the first layer's data-gradient kernel
(mmk_conv_first_dgrad) and the adjoint of the folded normalisation (mmk_input_norm_bwd) against their fp64 definitions, the
three autograd nodes (python / native driver, BatchNorm network) against each other and against the reference module's
golden input gradients (tests/golden/input_grads.npz), and the behaviour of the policy around them."""
import numpy as np
import pytest
import torch

from mm_masking_amd import _lib, synthetic
from mm_masking_amd import train_icp_weights as trn
from mm_masking_amd import unet_hip as uh
from mm_masking_amd import unet_hip_bn as ub
from mm_masking_amd.icp_weight_policy import LearnICPWeightPolicy

import input_grad_cases as igc
from support import DEV, policy

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16

# fp32 sums of at most 288 products (8 output channels x 9 taps x 4 input channels) in a fixed order, one more rounding for the
# reciprocal scale: 1e-5 of the largest element
KERNEL_TOL = 1e-5
# tiled form (W % 4 == 0; 35 x 36: an odd height with it) and the any-width form (33 x 37)
SIZES = [(32, 32), (33, 37), (40, 100), (35, 36)]


def _rand_case(B, cin, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    gz = torch.randn(B, H, W, 8, generator=g).to(BF16)
    w = torch.randn(8, cin, 3, 3, generator=g) * 0.3
    x = torch.rand(B, cin, H, W, generator=g)
    return gz, w, x


def _model(cin=1, dropout=0.0, leaky=False, bn=False, normalize="minmax", norm_weights=True, seed=17, **extra):
    return policy(DEV, seed, train=True, dropout=dropout, leaky=leaky, cfar_input=cin >= 2, range_input=cin >= 3, batch_norm=bn,
                  normalize=[normalize], norm_weights=norm_weights, **extra)


def _pre(x, mode):
    """(pre, input_norm) of unet_mask for normalisation ``mode`` of x."""
    if mode == "minmax":
        pre, mm = uh.channel_minmax(x, return_minmax=True)
        return pre, ("minmax", mm)
    if mode == "standardize":
        return uh.channel_meanstd(x), ("standardize", None)
    return None, None


# ----------------------------------------------------------------------------- 1. the kernel against its definition
@pytest.mark.parametrize("H,W", SIZES)
@pytest.mark.parametrize("cin", [1, 2, 3, 4])
def test_conv_first_dgrad_matches_the_definition(cin, H, W):
    """grad_x = rscale_c * conv2d_input(gz, W) (fp64, CPU) with the (offset, reciprocal scale) pairs as constants; every border,
    both forms of the kernel."""
    gz, w, _ = _rand_case(2, cin, H, W, seed=100 * cin + H)
    pre = torch.stack((torch.linspace(-0.5, 0.5, cin), torch.linspace(0.7, 2.9, cin)), dim=1).contiguous()
    want = igc.first_layer_input_grad_ref(gz, w) * pre[:, 1].double().view(1, cin, 1, 1)
    gx, ws = uh.conv_first_dgrad(gz.to(DEV), w.to(DEV), pre=pre.to(DEV))
    assert ws is None and gx.shape == (2, cin, H, W) and gx.dtype == torch.float32
    err = ((gx.cpu().double() - want).abs().max() / want.abs().max()).item()
    print("conv_first_dgrad cin=%d %dx%d: max error / max |grad_x| = %.3g" % (cin, H, W, err))
    assert err <= KERNEL_TOL, err
    # pre = NULL: rscale 1; and the tensor is overwritten, not added to
    gx1, _ = uh.conv_first_dgrad(gz.to(DEV), w.to(DEV))
    want1 = igc.first_layer_input_grad_ref(gz, w)
    assert ((gx1.cpu().double() - want1).abs().max() / want1.abs().max()).item() <= KERNEL_TOL
    gx2, _ = uh.conv_first_dgrad(gz.to(DEV), w.to(DEV))
    assert torch.equal(gx1, gx2)                 # gather form, fixed order: bit-reproducible


# ----------------------------------------------------------------------------- 2. known answer
@pytest.mark.parametrize("H,W", [(40, 100), (33, 37)])
@pytest.mark.parametrize("cin", [1, 3])
def test_conv_first_dgrad_known_answer(cin, H, W):
    """One non-zero pixel of gz (1.0 in one channel): grad_x is rscale * W[co] laid out around it -- the tap (ky, kx) at
    (y - 1 + ky, x - 1 + kx), clipped at the image border -- bit for bit, and exactly 0 elsewhere."""
    g = torch.Generator().manual_seed(7)
    w = torch.randn(8, cin, 3, 3, generator=g)
    pre = torch.stack((torch.zeros(cin), torch.linspace(1.5, 2.5, cin)), dim=1).contiguous()
    spots = [(0, 0, 0, 0), (1, H - 1, W - 1, 7), (0, 0, W // 2 + 1, 3), (1, H // 2, 0, 5), (0, H - 1, 5, 1), (1, H // 2 + 1, W // 2 + 2, 6),
             (0, 1, W - 2, 2)]          # corners, the four edges, interior (odd and even rows / columns)
    for b, y, x, co in spots:
        gz = torch.zeros(2, H, W, 8, dtype=BF16)
        gz[b, y, x, co] = 1.0
        want = torch.zeros(2, cin, H, W)
        for ky in range(3):
            for kx in range(3):
                yy, xx = y - 1 + ky, x - 1 + kx
                if 0 <= yy < H and 0 <= xx < W:
                    want[b, :, yy, xx] = w[co, :, ky, kx] * pre[:, 1]
        gx, _ = uh.conv_first_dgrad(gz.to(DEV), w.to(DEV), pre=pre.to(DEV))
        assert torch.equal(gx.cpu(), want), (b, y, x, co)


# ----------------------------------------------------------------------------- 3. the normalisation's adjoint
def _tied_image(B, cin, H, W, seed):
    """With two channels or more, channel 0 is binary (a CFAR mask: every element is tied with an extremum); every other
    channel is random with the maximum and the minimum planted twice each, in different images."""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(B, cin, H, W, generator=g) * 0.8 + 0.1
    for c in range(cin):
        if c == 0 and cin >= 2:
            x[:, 0] = (x[:, 0] > 0.75).float()
        else:
            x[0, c, 3, 4] = x[1, c, H - 1, W - 1] = 0.96875
            x[0, c, 0, 0] = x[1, c, 7, 9] = 0.03125
    return x


# error of grad_x against the fp64 autograd reference, relative to its largest element (for min-max an extremum's share, 19 to
# 100 times the median element).  Expected scale: the fp32 rounding of S1, S2 and of the reciprocal scale, about 1e-6.
# Measured on an MI355X, worst of cin 1..4 in both forms: min-max 3.13e-7, standardize 3.78e-7; bound = measured x 1.3.
NORM_TOL = {"minmax": 4.1e-7, "standardize": 4.9e-7}


@pytest.mark.parametrize("H,W", [(40, 100), (33, 37)])
@pytest.mark.parametrize("cin", [1, 2, 3, 4])
@pytest.mark.parametrize("mode", ["minmax", "standardize"])
def test_input_norm_adjoint_matches_autograd(mode, cin, H, W):
    """conv_first_dgrad + input_norm_bwd against CPU fp64 autograd through _normalize_channels and the fp64 convolution:
    every channel count in the tiled (40 x 100) and the any-width (33 x 37) form."""
    B = 2
    x = _tied_image(B, cin, H, W, seed=31)
    gz, w, _ = _rand_case(B, cin, H, W, seed=32)
    want = igc.first_layer_input_grad_ref(gz, w, x, mode)
    xd = x.to(DEV)
    pre, in_norm = _pre(xd, mode)
    gx = uh.first_layer_input_grad(xd, gz.to(DEV), w.to(DEV), pre, in_norm)
    err = ((gx.cpu().double() - want).abs().max() / want.abs().max()).item()
    print("input_norm_bwd %s cin=%d %dx%d: max error / max |grad_x| = %.3g (largest / median element %.1f)"
          % (mode, cin, H, W, err, (want.abs().max() / want.abs().median()).item()))
    assert err <= NORM_TOL[mode], err
    # the statistics the pass summed, against fp64
    g_n = igc.first_layer_input_grad_ref(gz, w)
    x_n = igc.normalize_channels(x.double(), mode)
    _, ws = uh.conv_first_dgrad(gz.to(DEV), w.to(DEV), x=xd, pre=pre, minmax=in_norm[1], stats=True)
    st = ws[:4 * cin].cpu().view(cin, 4)
    for c in range(cin):
        s1, s2 = g_n[:, c].sum().item(), (g_n[:, c] * x_n[:, c]).sum().item()
        scale = g_n[:, c].abs().sum().item()
        assert abs(st[c, 0].item() - s1) <= 1e-6 * scale and abs(st[c, 1].item() - s2) <= 1e-6 * scale, (c, st[c], s1, s2)
        if mode == "minmax":
            assert st[c, 2].item() == (x[:, c] == x[:, c].min()).sum().item()
            assert st[c, 3].item() == (x[:, c] == x[:, c].max()).sum().item()
            if not (c == 0 and cin >= 2):
                assert st[c, 2].item() == 2 and st[c, 3].item() == 2


@pytest.mark.parametrize("H,W", [(40, 100), (33, 37)])
@pytest.mark.parametrize("cin", [1, 2, 3, 4])
def test_minmax_tie_share_is_equal_bit_for_bit(cin, H, W):
    """The extremum's gradient is shared evenly among the tied elements: with the data term cleared, every element equal to
    the minimum (maximum) holds the same bits, the share is total / count, and nothing else is touched."""
    x = _tied_image(2, cin, H, W, seed=41)
    gz, w, _ = _rand_case(2, cin, H, W, seed=42)
    xd = x.to(DEV)
    pre, (_, mm) = _pre(xd, "minmax")
    gx, ws = uh.conv_first_dgrad(gz.to(DEV), w.to(DEV), x=xd, pre=pre, minmax=mm, stats=True)
    gx.zero_()
    uh.input_norm_bwd(gx, xd, pre, "minmax", mm, ws)
    gx, st, r = gx.cpu(), ws[:4 * cin].cpu().view(cin, 4), pre.cpu()[:, 1].double()
    for c in range(cin):
        lo, hi = x[:, c] == x[:, c].min(), x[:, c] == x[:, c].max()
        assert (gx[:, c][~(lo | hi)] == 0).all()
        for sel, total, cnt in ((lo, r[c] * (st[c, 1] - st[c, 0]), st[c, 2]), (hi, -r[c] * st[c, 1], st[c, 3])):
            v = gx[:, c][sel]
            assert v.numel() == int(cnt.item()) >= 2
            assert (v.view(torch.int32) == v.view(torch.int32)[0]).all()
            assert v[0].item() == np.float32((total / cnt).item())


# ----------------------------------------------------------------------------- 4. the whole network, pinned
@pytest.mark.parametrize("cin,leaky,mode,H,W", [(1, False, "minmax", 64, 64), (3, True, "standardize", 64, 64), (2, False, "none", 50, 84)])
def test_network_input_grad_on_its_own_first_gradient(cin, leaky, mode, H, W):
    """grad_x of the network equals the fp64 recomputation from the kernel's own gradient of the first pre-activation
    (the python driver's DEBUG hook): the new code apart from the bf16 noise of the 33 layers behind it."""
    model = _model(cin, leaky=leaky)
    g = torch.Generator().manual_seed(5)
    x = (torch.rand(2, cin, H, W, generator=g) + 0.05).to(DEV).requires_grad_(True)
    gsel = torch.randn(2, H, W, generator=g).to(DEV)
    pre, in_norm = _pre(x.detach(), mode)
    uh.DEBUG = {}
    try:
        m = uh.unet_mask(model, x, training=True, seed=3, norm=True, pre=pre, slope=0.1 if leaky else 0.0, driver="python",
                         input_norm=in_norm)
        (m * gsel).sum().backward()
        gz_a0 = uh.DEBUG["gz_a0"].clone()
    finally:
        uh.DEBUG = None
    assert gz_a0.shape == (2, H, W, 8) and gz_a0.dtype == BF16
    want = igc.first_layer_input_grad_ref(gz_a0, model.encoder[0][0].weight, x, mode)
    err = ((x.grad.cpu().double() - want).abs().max() / want.abs().max()).item()
    print("network grad_x vs fp64 from its own gz_a0 (cin=%d, %s): %.3g" % (cin, mode, err))
    assert want.abs().max() > 0 and err <= KERNEL_TOL, err


# ----------------------------------------------------------------------------- 5. drivers and variants
@pytest.mark.parametrize("cin,leaky,bn,norm,mode", [(1, False, False, True, "minmax"), (3, True, False, False, "standardize"),
                                                    (1, False, False, False, "none"), (3, False, False, True, "minmax"),
                                                    (1, False, True, True, "minmax"), (3, True, True, False, "standardize")])
def test_drivers_agree_and_repeat_bit_for_bit(cin, leaky, bn, norm, mode):
    """native and python drivers (the BatchNorm network: its one schedule) give torch.equal input gradients, and so do two
    runs of each; dropout 0.05 in training mode with the deterministic seed schedule."""
    model = _model(cin, dropout=0.05, leaky=leaky, bn=bn)
    g = torch.Generator().manual_seed(11)
    x0 = (torch.rand(2, cin, 64, 64, generator=g) + 0.05).to(DEV)
    gsel = torch.randn(2, 64, 64, generator=g).to(DEV)
    pre, in_norm = _pre(x0, mode)
    slope = 0.1 if leaky else 0.0
    got = []
    for drv in (("bn", "bn") if bn else ("python", "native", "python", "native")):
        if bn:       # (the running statistics move with every training pass; the batch statistics the pass uses do not)
            x = x0.clone().requires_grad_(True)
            m = ub.unet_mask(model, x, training=True, seed=9, norm=norm, pre=pre, slope=slope, input_norm=in_norm)
        else:
            x = x0.clone().requires_grad_(True)
            m = uh.unet_mask(model, x, training=True, seed=9, norm=norm, pre=pre, slope=slope, driver=drv, input_norm=in_norm)
        model.zero_grad(set_to_none=True)
        (m * gsel).sum().backward()
        assert x.grad is not None and x.grad.shape == x.shape
        assert torch.isfinite(x.grad).all() and x.grad.abs().max() > 0
        got.append(x.grad.clone())
    for other in got[1:]:
        assert torch.equal(got[0], other)


# ----------------------------------------------------------------------------- 6. against the reference's golden
# relative L2 error / cosine of the input gradients against the reference module's fp32 CPU vectors.  The per-pixel gradient
# does not average the bf16 noise of the 33 layers as a parameter gradient does, so the parameters' 5.9 % / 6.2 % do not carry
# over.  Measured on an MI355X (deterministic: dropout is off), relative L2 / cosine: n1 fft 0.0496 / 0.9988; n3 fft 0.0509 /
# 0.9987, cfar 0.0602 / 0.9982.  Bounds = measured with 30 % of margin on the error (relative L2 x 1.3, 1 - cosine x 1.3), the
# convention of test_unet_hip_backend_golden.  A cosine below 0.8 would mean a bug, not noise.
GOLDEN_BOUND = {"n1": {"fft": (0.0645, 0.9984)}, "n3": {"fft": (0.0662, 0.9983), "cfar": (0.0783, 0.9977)}}   # (relative L2 max, cosine min)


# the forward mask against the reference's, as test_unet_hip_backend_golden checks it (forward kernels this gradient does not
# touch; the same figures come out when the images do not require grad).  Measured on an MI355X, largest error: n1 0.00051,
# n3 0.0089 (3.5 % of the pixels beyond the 4e-3 of that test's standardised 3-channel case).  n3 feeds the network raw
# logarithms, up to |log 1e-6| = 13.8 and a range channel of 4.46 .. 4.68 that bf16 resolves in steps of 0.031: rounding the
# input alone moves the fp32 mirror's mask by 1.8e-3 (n1: 1e-4), before any of the 33 bf16 layers.  Bounds = measured x 1.3.
MASK_ATOL = {"n1": 6.7e-4, "n3": 1.16e-2}


def _rel_cos(got, want):
    got, want = got.double().reshape(-1), want.double().reshape(-1)
    return ((got - want).norm() / want.norm()).item(), (got @ want / (got.norm() * want.norm())).item()


@pytest.mark.parametrize("tag", ["n1", "n3"])
def test_input_grad_against_the_reference_golden(golden_dir, tag):
    g = igc.load_golden(golden_dir)
    model = igc.golden_model(g, tag, DEV)
    assert model.unet_backend == "hip"
    mask, gx, gcfar = igc.golden_input_grads(g, tag, model, DEV)
    assert gx is not None
    mask_err = float(np.abs(mask.cpu().numpy() - g["mask_" + tag]).max())
    print("mask vs the reference's (%s): max error %.5f" % (tag, mask_err))
    pairs = [("fft", gx, g["gx_" + tag])] + ([("cfar", gcfar, g["gcfar_" + tag])] if tag == "n3" else [])
    res = {}
    for name, got, want in pairs:
        res[name] = _rel_cos(got.cpu(), torch.from_numpy(want))
        print("input gradient vs the reference's (%s, %s): relative L2 %.4f, cosine %.4f" % (tag, name, res[name][0], res[name][1]))
    assert mask_err <= MASK_ATOL[tag], mask_err
    for name, (rel, cos) in res.items():
        assert cos > 0.8, (name, cos)                # below this: a bug, not bf16 noise
        rel_max, cos_min = GOLDEN_BOUND[tag][name]
        assert rel < rel_max and cos > cos_min, (name, rel, cos)


# ----------------------------------------------------------------------------- 7. behaviour
@pytest.mark.parametrize("normalize,cin", [("minmax", 1), ("standardize", 3), ("none", 1)])
def test_step_without_input_grad_is_unchanged(normalize, cin):
    """A leaf that requires grad changes nothing else: the mask and all 46 parameter gradients are bit-equal to the call on
    a plain tensor (the path the training step takes), and so is the mask under torch.no_grad()."""
    g = torch.Generator().manual_seed(3)
    fft = torch.rand(2, 64, 64, generator=g) + 0.05
    cfar = (torch.rand(2, 64, 64, generator=g) > 0.9).float()
    gsel = torch.randn(2, 64, 64, generator=g).to(DEV)
    res = []
    for leaf in (False, True):
        model = _model(cin, dropout=0.05, normalize=normalize, seed=23)
        if cin >= 3:
            model.range_mask = model.range_mask[:64, :64].contiguous()
        f = fft.clone().to(DEV).requires_grad_(leaf)
        scan = {"fft_data": f, "fft_cfar": cfar.to(DEV), "raw_pc": torch.zeros(2, 4, 3)}
        m = model(scan, {"pc": torch.zeros(2, 4, 6)}, None, mask_only=True)
        (m * gsel).sum().backward()
        res.append((m.detach().clone(), [p.grad.clone() for p in model.parameters()], f.grad))
        if leaf:
            with torch.no_grad():
                model._step = 0
                m2 = model(scan, {"pc": torch.zeros(2, 4, 6)}, None, mask_only=True)
            assert torch.equal(m2, res[0][0])
    (m0, g0, x0), (m1, g1, x1) = res
    assert x0 is None and x1 is not None and torch.isfinite(x1).all() and x1.abs().max() > 0
    assert torch.equal(m0, m1)
    assert len(g0) == len(g1) == 46
    for a, b in zip(g0, g1):
        assert torch.equal(a, b)


def test_input_grad_dtype_device_and_polar_size():
    """The gradient arrives in the input's dtype and on its device (an fp64 tensor on the GPU through unet_mask, a CPU leaf
    through the policy), and the odd polar size 50 x 84 runs on every node."""
    model = _model(1)
    g = torch.Generator().manual_seed(9)
    x = torch.rand(3, 1, 50, 84, generator=g, dtype=torch.float64).to(DEV).requires_grad_(True)
    for drv in ("native", "python"):
        x.grad = None
        pre, in_norm = _pre(x.detach().float(), "minmax")
        uh.unet_mask(model, x, training=True, seed=1, norm=True, pre=pre, driver=drv, input_norm=in_norm).sum().backward()
        assert x.grad.dtype == torch.float64 and x.grad.device == x.device and x.grad.shape == x.shape
        assert torch.isfinite(x.grad).all() and x.grad.abs().max() > 0
    mb = _model(1, bn=True)
    xb = torch.rand(3, 1, 50, 84, generator=g).to(DEV).requires_grad_(True)
    ub.unet_mask(mb, xb, training=True, seed=1, norm=True).sum().backward()
    assert xb.grad.dtype == torch.float32 and torch.isfinite(xb.grad).all() and xb.grad.abs().max() > 0
    leaf = torch.rand(2, 64, 64, generator=g).requires_grad_(True)                   # on the host
    scan = {"fft_data": leaf, "fft_cfar": torch.zeros(2, 64, 64), "raw_pc": torch.zeros(2, 4, 3)}
    model(scan, {"pc": torch.zeros(2, 4, 6)}, None, mask_only=True).sum().backward()
    assert leaf.grad.device.type == "cpu" and leaf.grad.dtype == torch.float32 and leaf.grad.abs().max() > 0


def test_input_norm_argument_checks():
    model = _model(1)
    x = torch.rand(1, 1, 32, 32, device=DEV)
    with pytest.raises(_lib.MmkError, match="unknown mode"):
        uh.unet_mask(model, x, True, 1, pre=uh.channel_minmax(x), input_norm=("zscore", None))
    with pytest.raises(_lib.MmkError, match="raw"):
        uh.unet_mask(model, x, True, 1, pre=uh.channel_minmax(x), input_norm=("minmax", None))
    with pytest.raises(_lib.MmkError, match="pre"):
        uh.unet_mask(model, x, True, 1, input_norm=("standardize", None))


def test_global_minmax_input_grad_is_refused(tmp_path):
    """Extrema reduced over the ranks (here: the forced collective of a one-rank group): the cross-rank gradient is out of
    scope, so an input that requires grad is refused -- before any collective is issued; a plain tensor still runs."""
    import torch.distributed as dist
    model = _model(1, global_minmax=True)
    leaf = torch.rand(2, 32, 32, device=DEV).requires_grad_(True)
    batch_map = {"pc": torch.zeros(2, 4, 6)}

    def scan(t):
        return {"fft_data": t, "fft_cfar": torch.zeros(2, 32, 32), "raw_pc": torch.zeros(2, 4, 3)}

    dist.init_process_group("gloo", init_method="file://%s" % (tmp_path / "rendezvous"), rank=0, world_size=1)
    uh.FORCE_COLLECTIVES = True
    try:
        with pytest.raises(_lib.MmkError, match="reduced over the ranks"):
            model(scan(leaf), batch_map, None, mask_only=True)
        with torch.no_grad():            # nothing asks for the gradient: the collective path as before
            model(scan(leaf), batch_map, None, mask_only=True)
        model(scan(leaf.detach()), batch_map, None, mask_only=True)
    finally:
        uh.FORCE_COLLECTIVES = False
        dist.destroy_process_group()
    model(scan(leaf), batch_map, None, mask_only=True).sum().backward()          # per-rank extrema: fine
    assert leaf.grad is not None and leaf.grad.abs().max() > 0


# ----------------------------------------------------------------------------- 8. the chain
def test_pose_loss_reaches_the_radar_image():
    """loss(T).backward() through dICP, extract_weights and the mask leaves a finite, non-zero fft_data.grad (the small
    shape of test_gpu_policy.py::test_train_step_matches_cpu_port)."""
    raw = synthetic.make_batch([0, 1], device=DEV, m_valid=3000, m_pad=3072, density="sparse")
    params = trn.default_params(DEV)
    params.update({"dropout": 0.0, "icp_type": "pt2pl", "icp_loss_fn": {"name": "huber", "metric": 1.0}, "max_iter": 5})
    batch = trn.prepare_batch(raw, params, max_loc_pts=2048)
    torch.manual_seed(1234)
    model = LearnICPWeightPolicy(params).to(DEV)
    model.train()
    loc = dict(batch["loc_data"])
    fft = loc["fft_data"].detach().clone().requires_grad_(True)
    loc["fft_data"] = fft
    T, mask, _ = model(loc, batch["map_data"], raw["T_init"])
    loss = ((T - raw["T_gt"]) ** 2).sum()
    loss.backward()
    assert fft.grad is not None and fft.grad.shape == fft.shape and fft.grad.dtype == fft.dtype
    assert torch.isfinite(fft.grad).all() and fft.grad.abs().max() > 0
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in model.parameters())
