"""Every kernel that draws a dropout mask, pinned bit for bit to the host restatement of the hash (tests/dropout_ref.py):
WHICH elements are dropped, not just how many.  Element index = pixel * COUT + channel (+ hash_base), COUT = the layer's.

Input kinds
  ones      x = 1, weights 1 at the centre tap of w[co, co % cin]: every accumulator is exactly 1, so the whole output is, as
            bits, where(keep, bf16(1 / keep), +0.0).  Run without bias and with a zero bias tensor (the bias-in-LDS path).
  positive  x in [0.5, 1.5], weights >= 0, bias > 0: nothing is zero by itself, so the zero pattern is the mask exactly; on kept
            elements y_drop is compared with the same launch without dropout, y_nodrop * (1 / keep) -- see _check_values.
  signed    the paths that store a kept zero as -0.0 (slope > 0, bn_apply): inputs of both signs with exact zeros;
            dropped <=> bits == 0x0000 in both directions, and the same value check.

Which kernel each case reaches (read off dispatch_conv / dispatch_conv_deep / launch_conv_ring_epi, csrc/mmk_unet.hip):

  case                                         kernel                                               mask code
  8->8, 16->8                                  conv3x3_ring_kernel<.., C8>                          dropout_keep4 on pixel * 8, lanes permuted
  8->16, 16->16, 16->32, 32->32, 32->16        conv3x3_ring_kernel<CK, CM, RD, EPI=0, POOL=0>       dropout_words + pk_keep_mask
  16->8|8 (split output)                       the same (o2.C != 0 keeps it off the C8 epilogue)    ... index over COUT = 16, stores over 8
  16->16 accumulating into zeros               conv3x3_ring_kernel<.., EPI=1>                       dropout_keep4 (scalar form)
  16->16, 32->32 + pool_out                    conv3x3_ring_kernel<.., POOL=1>                      dropout_keep4 (scalar form)
  16->16, 32->32 + pool_out + pool_arg         conv3x3_ring_kernel<.., POOL=2>                      dropout_words + pk_keep_mask
  8->64, 16->64                                conv3x3_kernel<CK, 64>                               dropout_scale4
  8->8, 16->16, 32->32 with slope              conv3x3_kernel<CK, CM, LK>                           dropout_scale4 + drop_leaky
  64->64, 32->64, 64->32, 64->32|32            conv3x3_deep_kernel<BM, NT, R_FWD, WRES> (resident)  packed, threshold word rebuilt locally
  128->128, 256->128, 64->128, 64->192         conv3x3_deep_kernel<128, NT, R_FWD> (streamed)       the same
  64+64->64 (concatenated input)               conv3x3_deep_kernel<64, NT, R_FWD> (4 chunks: streamed)
  128->16                                      conv3x3_deep_kernel<16, NT> generic role             dropout_scale4
  64->64, 128->128 with slope                  conv3x3_deep_kernel<BM, NT, LK>                      dropout_scale4 + drop_leaky
  B = 32: (80, 128->64), (40, 256->128)        own kernel on images 0..24, then <32, NT, SUBW, R_FWD> on 25..31 with hash_base
  bn_apply C = 8, 32, 256                      bn_apply_kernel                                      dropout_scale4 on e * 8, e * 8 + 4
  (.., 9, 20) and (.., 17, 33) rows take the 3-tile-wide deep variant (W <= 48), (2, 12, 80) the 5-tile-wide one.

No expected number in this file comes from a kernel: masks and scales are dropout_ref's, the value bound is derived below."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import dropout_ref as dr
from mm_masking_amd import _lib
from mm_masking_amd import unet_hip as uh
from support import DEV, policy

pytestmark = pytest.mark.gpu
P = 0.05                   # the benchmarked probability (thr = 3277)
SEED = 0x5EED5


def _bits(t):
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def _f64(t):
    return t.float().cpu().numpy().astype(np.float64)


def _bf16_bits(v):
    """bits of bf16(v), round to nearest even, v an fp32 scalar"""
    return int(torch.tensor([float(v)], dtype=torch.float32).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)[0])


@functools.lru_cache(maxsize=None)
def _centre_weights(cin, cout):
    w = torch.zeros(cout, cin, 3, 3)
    for co in range(cout):
        w[co, co % cin, 1, 1] = 1.0
    return uh.pack_weights(w.to(DEV))


def _inputs(kind, cin, cout, B, H, W, want_bias):
    """(x, packed weights, bias or None) of one input kind; deterministic"""
    g = torch.Generator().manual_seed(1000 * cin + cout + H)
    if kind == "ones":
        x = torch.ones(B, H, W, cin, dtype=uh.BF16, device=DEV)
        return x, _centre_weights(cin, cout), (torch.zeros(cout, device=DEV) if want_bias else None)
    if kind == "positive":
        x = (torch.rand(B, H, W, cin, generator=g) + 0.5).to(uh.BF16).to(DEV)
        w = (torch.rand(cout, cin, 3, 3, generator=g) / (4.5 * cin)).to(DEV)
        return x, uh.pack_weights(w), (torch.rand(cout, generator=g) + 0.1).to(DEV)
    assert kind == "signed"
    x = torch.randn(B, H, W, cin, generator=g)
    x[torch.rand(B, H, W, cin, generator=g) < 0.1] = 0.0            # exact zeros: kept ones must come out as -0.0
    return x.to(uh.BF16).to(DEV), _centre_weights(cin, cout), None


def _check_ones(y, keep, p, what=""):
    want = np.where(keep, np.uint16(_bf16_bits(dr.params(p).inv_keep)), np.uint16(0))
    got = _bits(y)
    bad = got != want
    assert not bad.any(), "%s: %d of %d elements differ from where(keep, bf16(1/keep), +0.0); first at %s" % (
        what, bad.sum(), bad.size, tuple(np.argwhere(bad)[0]))


def _check_zero_pattern(y, keep, what=""):
    zero = _bits(y) == 0
    assert not (zero & keep).any(), "%s: %d kept elements are stored as +0.0" % (what, (zero & keep).sum())
    assert not (~zero & ~keep).any(), "%s: %d dropped elements are not +0.0" % (what, (~zero & ~keep).sum())


def _check_values(y_drop, y_nodrop, keep, p, what=""):
    """On kept elements |y_drop - y_nodrop k| <= 2^-7 |y_nodrop| k, k = 1 / keep in fp32.  Both tensors are bf16 roundings of the
    same fp32 value v (times k): y_nodrop = v (1 + a), y_drop = v k (1 + b), |a|, |b| <= 2^-9 (half an ulp of an 8-bit
    significand; the fp32 roundings of v k and of the folded bias k are 2^-24 and vanish beside it).  So
    |y_drop - y_nodrop k| = |v| k |b - a| <= 2^-8 |v| k <= 2^-8 |y_nodrop| k / (1 - 2^-9): 2^-7 |y_nodrop| k leaves a factor 2."""
    k = float(dr.params(p).inv_keep)
    a, b = _f64(y_drop)[keep], _f64(y_nodrop)[keep] * k
    err = np.abs(a - b)
    bound = 2.0 ** -7 * np.abs(b)
    assert (err <= bound).all(), "%s: kept values off by up to %g of y_nodrop / keep (bound 2^-7)" % (
        what, (err / np.maximum(np.abs(b), 1e-30)).max())


def _conv(x, wp, cout, bias, p, seed, **kw):
    return uh.conv3x3(x, wp, cout, bias=bias, relu=True, drop_p=p, seed=seed, **kw)


def _check_conv(cin, cout, B, H, W, kinds=("ones", "ones+bias", "positive"), slope=0.0, p=P, seed=SEED, x2_at=None, split=None):
    keep = dr.keep_mask(seed, (B, H, W, cout), p)
    for kind in kinds:
        x, wp, bias = _inputs(kind.split("+")[0], cin, cout, B, H, W, kind.endswith("+bias"))
        kw = {"slope": slope}
        xa = x
        if x2_at is not None:
            xa, kw["x2"] = x[..., :x2_at].contiguous(), x[..., x2_at:].contiguous()
        what = "%d->%d (%d,%d,%d) %s" % (cin, cout, B, H, W, kind)

        def run(pp):
            y = _conv(xa, wp, cout, bias, pp, seed, split=split, **kw)
            return torch.cat(y, dim=3) if split is not None else y

        y = run(p)
        if kind.startswith("ones"):
            _check_ones(y, keep, p, what)
        else:
            _check_zero_pattern(y, keep, what)
            _check_values(y, run(0.0), keep, p, what)
            if kind == "signed":          # the case the -0.0 convention exists for really occurs: kept exact zeros
                zin = (_f64(x) == 0.0)[..., [co % cin for co in range(cout)]]
                assert (zin & keep).sum() > 10 and (_bits(y)[zin & keep] == 0x8000).all(), what


RING_SHAPES = [(3, 17, 33), (2, 9, 31)]
DEEP_SHAPES = [(3, 9, 20), (2, 12, 80)]


@pytest.mark.parametrize("cin,cout", [(8, 8), (16, 8)])
def test_ring_c8_epilogue(cin, cout):
    _check_conv(cin, cout, 3, 17, 33)


@pytest.mark.parametrize("B,H,W", RING_SHAPES)
@pytest.mark.parametrize("cin,cout", [(8, 16), (16, 16), (16, 32), (32, 32), (32, 16)])
def test_ring_packed(cin, cout, B, H, W):
    _check_conv(cin, cout, B, H, W)


def test_ring_scalar_form_with_epilogue_operand():
    """Dropout with an accumulate target (the ABI allows it) takes the ring kernel's EPI variant, whose forward epilogue is
    the scalar one: accumulating into zeros leaves the dropout result itself."""
    B, H, W, c = 3, 17, 33, 16
    keep = dr.keep_mask(SEED, (B, H, W, c), P)
    x, wp, _ = _inputs("ones", c, c, B, H, W, False)
    y = _conv(x, wp, c, None, P, SEED, out=torch.zeros(B, H, W, c, dtype=uh.BF16, device=DEV), accumulate=True)
    _check_ones(y, keep, P, "16->16 accumulate")
    x, wp, bias = _inputs("positive", c, c, B, H, W, True)
    z = lambda: torch.zeros(B, H, W, c, dtype=uh.BF16, device=DEV)
    y = _conv(x, wp, c, bias, P, SEED, out=z(), accumulate=True)
    _check_zero_pattern(y, keep, "16->16 accumulate, positive")
    _check_values(y, _conv(x, wp, c, bias, 0.0, SEED, out=z(), accumulate=True), keep, P)


def _pool_windows(a, Hp, Wp):
    """(B,H,W,C) -> (B,Hp,Wp,C,4): the 2x2 windows of the floor-rounded pooling, positions in scan order"""
    B, _, _, C = a.shape
    return a[:, :2 * Hp, :2 * Wp].reshape(B, Hp, 2, Wp, 2, C).transpose(0, 1, 3, 5, 2, 4).reshape(B, Hp, Wp, C, 4)


@pytest.mark.parametrize("c,B,H,W", [(16, 3, 37, 51), (32, 2, 25, 42)])
def test_ring_fused_pooling(c, B, H, W):
    assert uh.pool_fusable(c, c, B, H, W)
    Hp, Wp = H // 2, W // 2
    keep = dr.keep_mask(SEED, (B, H, W, c), P)
    kw = _pool_windows(keep, Hp, Wp)
    kbits = np.uint16(_bf16_bits(dr.params(P).inv_keep))
    want_pool = np.where(kw.any(-1), kbits, np.uint16(0))
    # arg-max code: first kept position in scan order | 1 << 2, 0 for an all-dropped window (every kept value is the same
    # maximum); channel c sits in bits 4 (c & 1) of byte c / 2 (include/mmk.h: mmk_conv_desc.pool_arg)
    code = np.where(kw.any(-1), kw.argmax(-1) | 4, 0).astype(np.uint8)
    want_arg = code[..., 0::2] | (code[..., 1::2] << 4)
    for with_bias in (False, True):
        x, wp, bias = _inputs("ones", c, c, B, H, W, with_bias)
        # pool_out: the scalar epilogue; the full-resolution tensor is written as well
        pooled = torch.full((B, Hp, Wp, c), float("nan"), dtype=uh.BF16, device=DEV)
        y = _conv(x, wp, c, bias, P, SEED, pool_out=pooled)
        _check_ones(y, keep, P, "%d->%d pool_out, full resolution" % (c, c))
        assert np.array_equal(_bits(pooled), want_pool)
        # pool_out + pool_arg: the packed epilogue; only the pooled tensor and the codes are written
        pooled2 = torch.full((B, Hp, Wp, c), float("nan"), dtype=uh.BF16, device=DEV)
        arg = torch.full((B, Hp, Wp, c // 2), 0xEE, dtype=torch.uint8, device=DEV)
        assert _conv(x, wp, c, bias, P, SEED, pool_out=pooled2, pool_arg=arg) is None
        assert np.array_equal(_bits(pooled2), want_pool)
        assert np.array_equal(arg.cpu().numpy(), want_arg)
    # positive: mask / value pairing of the scalar epilogue, and the pooled tensor = window maximum of the checked tensor
    x, wp, bias = _inputs("positive", c, c, B, H, W, True)
    pooled = torch.full((B, Hp, Wp, c), float("nan"), dtype=uh.BF16, device=DEV)
    y = _conv(x, wp, c, bias, P, SEED, pool_out=pooled)
    _check_zero_pattern(y, keep, "pool_out, positive")
    _check_values(y, _conv(x, wp, c, bias, 0.0, SEED), keep, P, "pool_out, positive")
    assert np.array_equal(_f64(pooled), _pool_windows(_f64(y), Hp, Wp).max(-1))
    pooled2 = torch.full((B, Hp, Wp, c), float("nan"), dtype=uh.BF16, device=DEV)
    arg = torch.empty(B, Hp, Wp, c // 2, dtype=torch.uint8, device=DEV)
    _conv(x, wp, c, bias, P, SEED, pool_out=pooled2, pool_arg=arg)
    assert torch.equal(pooled2, pooled)
    win = _pool_windows(_f64(y), Hp, Wp)
    code = (win.argmax(-1) | np.where(win.max(-1) > 0, 4, 0)).astype(np.uint8)
    assert np.array_equal(arg.cpu().numpy(), code[..., 0::2] | (code[..., 1::2] << 4))


@pytest.mark.parametrize("cin,cout", [(8, 64), (16, 64)])
def test_thin_kernel_wide_output(cin, cout):
    _check_conv(cin, cout, 3, 17, 33)


@pytest.mark.parametrize("c", [8, 16, 32])
def test_thin_kernel_leaky(c):
    _check_conv(c, c, 3, 17, 33, kinds=("signed",), slope=0.1)


@pytest.mark.parametrize("B,H,W", DEEP_SHAPES)
@pytest.mark.parametrize("cin,cout", [(64, 64), (32, 64), (64, 32), (128, 128), (256, 128), (64, 128), (64, 192)])
def test_deep_forward_role(cin, cout, B, H, W):
    _check_conv(cin, cout, B, H, W)


def test_deep_forward_role_concatenated_input():
    _check_conv(128, 64, 3, 9, 20, x2_at=64)


@pytest.mark.parametrize("B,H,W", DEEP_SHAPES)
def test_deep_generic_role(B, H, W):
    _check_conv(128, 16, B, H, W)


@pytest.mark.parametrize("B,H,W", DEEP_SHAPES)
@pytest.mark.parametrize("c", [64, 128])
def test_deep_leaky(c, B, H, W):
    _check_conv(c, c, B, H, W, kinds=("signed",), slope=0.1)


@pytest.mark.parametrize("cin,cout,B,H,W", [(16, 16, 3, 17, 33), (64, 64, 3, 9, 20), (64, 64, 2, 12, 80)])
def test_split_outputs_index_runs_over_the_layers_cout(cin, cout, B, H, W):
    _check_conv(cin, cout, B, H, W, split=cout // 2)


def _deep_rounds(B, H, W, cout, BM, NT):
    """dispatch_conv_deep's tile arithmetic (csrc/mmk_unet.hip: deep_rounds): rounds of the persistent grid, tiles per image,
    blocks per XCD"""
    TH = 4 if BM >= 128 else 8
    tpi = -(-W // (NT * 16)) * -(-H // TH)
    groups = -(-cout // BM)
    nb = max(1, 32 // groups)
    return -(-((B * tpi + 7) // 8) // nb), tpi, nb


@pytest.mark.parametrize("H,cin,cout", [(80, 128, 64), (40, 256, 128)])
def test_deep_sub_batch_split_continues_the_index(H, cin, cout):
    """The shapes of test_conv_deep_sub_batch_split_bit_identical: the launch is split by images and the second launch's
    element index must continue at hash_base = images in front * H * W * COUT -- checked against the definition over the
    whole batch, not against the unsplit launch."""
    B, BM, NT = 32, min(cout, 128), 3 if H <= 48 else 5
    rounds, tpi, nb = _deep_rounds(B, H, H, cout, BM, NT)
    Bm = (8 * nb) // tpi
    assert rounds == 2 and 1 <= Bm < B                     # the split's own condition: two rounds, Bm images fill the first
    assert _deep_rounds(Bm, H, H, cout, BM, NT)[0] == 1 and _deep_rounds(B - Bm, H, H, cout, 32, NT)[0] == 1
    keep = dr.keep_mask(SEED, (B, H, H, cout), P)
    x, wp, _ = _inputs("ones", cin, cout, B, H, H, False)
    y = _conv(x, wp, cout, None, P, SEED)
    assert float(y[-1].float().abs().sum()) > 0              # the images of the second launch were written
    _check_ones(y[:Bm], keep[:Bm], P, "images of the first launch")
    _check_ones(y[Bm:], keep[Bm:], P, "images of the second launch (hash_base)")


def _bn_apply(a, affine, p, seed, y=None):
    B, H, W, C = a.shape
    y = torch.empty_like(a) if y is None else y
    _lib.check(_lib.lib().mmk_bn_apply(ctypes.c_void_p(a.data_ptr()), B * H * W, C, ctypes.c_void_p(affine.data_ptr()), float(p),
                                       int(seed) & 0xFFFFFFFF, ctypes.c_void_p(y.data_ptr()), _lib.stream_ptr(a.device)))
    return y


@pytest.mark.parametrize("C", [8, 32, 256])
def test_bn_apply(C):
    B, H, W = 3, 17, 23
    g = torch.Generator().manual_seed(C)
    a = torch.randn(B, H, W, C, generator=g)
    a[torch.rand(B, H, W, C, generator=g) < 0.1] = 0.0
    a = a.to(uh.BF16).to(DEV)
    affine = torch.stack((torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.3), dim=1)
    affine[0::2, 1] = 0.0                                  # no shift on the even channels: a zero input gives an exact zero there
    affine = affine.contiguous().to(DEV)
    keep = dr.keep_mask(SEED, (B, H, W, C), P)
    y = _bn_apply(a, affine, P, SEED)
    _check_zero_pattern(y, keep, "bn_apply C=%d" % C)
    _check_values(y, _bn_apply(a, affine, 0.0, SEED), keep, P, "bn_apply C=%d" % C)
    zin = _f64(a) == 0.0
    zin[..., 1::2] = False
    assert (zin & keep).sum() > 10 and (_bits(y)[zin & keep] == 0x8000).all()


@pytest.mark.parametrize("c,B", [(8, 22), (16, 11)])
def test_group_numbers_from_2_to_the_24(c, B):
    """Element 2^26 (group 2^24, where the term i & 0xff000000 of the hash starts to matter) lies inside the last two images of
    these tensors, which are what the benchmark's B = 32, 640 x 640 thin layers reach from image 21 on."""
    H = W = 640
    per_image = H * W * c
    base = (B - 2) * per_image
    assert base < (1 << 26) < base + 2 * per_image and B * per_image < (1 << 31)
    x = torch.ones(B, H, W, c, dtype=uh.BF16, device=DEV)
    y = _conv(x, _centre_weights(c, c), c, None, P, SEED)
    del x
    keep = dr.keep_mask(SEED, (2, H, W, c), P, base=base)
    _check_ones(y[B - 2:], keep, P, "%d->%d, images %d and %d of %d" % (c, c, B - 2, B - 1, B))


# ---------------------------------------------------------------------------------------------- edge thresholds
# (2, 40, 80), ones.  Seeds picked on the CPU so that both extreme draws occur at least three times among the case's elements.
EDGE_SHAPE = (2, 40, 80)
EDGE_SEED = {8: 440, 16: 96, 64: 11}
EDGE_PATHS = [("ring packed", 16, 16), ("ring c8", 8, 8), ("deep R_FWD", 64, 64), ("deep generic", 128, 16), ("thin kernel", 8, 64),
              ("bn_apply", 64, 64)]


def _edge_run(name, cin, cout, p, seed):
    B, H, W = EDGE_SHAPE
    if name == "bn_apply":
        a = torch.ones(B, H, W, cout, dtype=uh.BF16, device=DEV)
        affine = torch.tensor([[1.0, 0.0]] * cout, device=DEV)
        return _bn_apply(a, affine, p, seed)
    x, wp, _ = _inputs("ones", cin, cout, B, H, W, False)
    return _conv(x, wp, cout, None, p, seed)


@pytest.mark.parametrize("name,cin,cout", EDGE_PATHS)
def test_edge_probabilities(name, cin, cout):
    B, H, W = EDGE_SHAPE
    seed = EDGE_SEED[cout]
    d = dr.draws(seed, B * H * W * cout).reshape(B, H, W, cout)
    assert (d == -32768).sum() >= 3 and (d == 32767).sum() >= 3
    # p = 1 / 65536: only the draw -32768 is dropped
    p = 1.0 / 65536
    assert dr.params(p).thr == 1
    _check_ones(_edge_run(name, cin, cout, p, seed), d != -32768, p, name + " thr = 1")
    # p = 0.5
    assert dr.params(0.5).thr == 32768
    _check_ones(_edge_run(name, cin, cout, 0.5, seed), d >= 0, 0.5, name + " thr = 32768")
    # p = 65535 / 65536: only the draw 32767 is kept, scaled by 65536
    p = 65535.0 / 65536
    assert dr.params(p).thr == 65535 and dr.params(p).inv_keep == 65536.0 and _bf16_bits(65536.0) == 0x4780
    _check_ones(_edge_run(name, cin, cout, p, seed), d == 32767, p, name + " thr = 65535")
    # p = 1e-6 quantises to thr = 0: dropout is off, also for the draw -32768
    assert dr.params(1e-6).thr == 0
    y0 = _edge_run(name, cin, cout, 0.0, seed)
    assert (_bits(y0) == 0x3F80).all()
    assert np.array_equal(_bits(_edge_run(name, cin, cout, 1e-6, seed)), _bits(y0)), name + " thr = 0"


def test_probability_that_quantises_to_everything_dropped_is_refused():
    """p = 1 - 1e-6 passes p < 1 but rounds to thr = 65536 (nothing kept, 1 / keep infinite): the three entries that take a
    dropout probability name it in an argument error before anything is launched."""
    p = 1.0 - 1e-6
    assert dr.params(p).thr == 65536
    B, H, W = 2, 16, 32
    x, wp, _ = _inputs("ones", 16, 16, B, H, W, False)
    y = torch.full((B, H, W, 16), 7.0, dtype=uh.BF16, device=DEV)
    with pytest.raises(_lib.MmkError, match="mmk_conv3x3: dropout probability"):
        _conv(x, wp, 16, None, p, 1, out=y)
    with pytest.raises(_lib.MmkError, match="mmk_bn_apply: dropout probability"):
        _bn_apply(x, torch.tensor([[1.0, 0.0]] * 16, device=DEV), p, 1, y=y)
    torch.cuda.synchronize()
    assert (_bits(y) == _bf16_bits(7.0)).all()
    model = policy(DEV, 11, dropout=0.05)
    model.dropout = p
    model.train()
    with pytest.raises(_lib.MmkError, match="mmk_unet_forward: dropout probability"):
        uh.unet_mask(model, torch.rand(1, 1, 32, 32, device=DEV), training=True, seed=1, driver="native")


# ---------------------------------------------------------------------------------------------- the network's seed schedule
def _layer_tensors(fwd):
    """the 16 stored post-dropout tensors in launch order"""
    out = [fwd["enc"]["e%d" % i][1] for i in range(6)]
    for j in range(5):
        out += [fwd["dec"][j][2], fwd["dec"][j][4]]
    return out


def _check_schedule(tensors, step_seed, exact, p=P):
    """exact: dropped <=> +0.0 (the networks that store a kept zero as -0.0).  Otherwise (ReLU network, where a zero may also be
    a ReLU zero): every host-dropped element is +0.0 -- and, so that this cannot pass on a wrong seed, the mask of the
    neighbouring seed must be violated by at least 1 % of ITS dropped elements on every layer of >= 4096 elements."""
    assert len(tensors) == 16
    for k, t in enumerate(tensors, start=1):
        keep = dr.keep_mask(dr.layer_seed(step_seed, k), tuple(t.shape), p)
        zero = _bits(t) == 0
        assert zero[~keep].all(), "layer %d: %d dropped elements are not +0.0" % (k, (~zero[~keep]).sum())
        if exact:
            assert not zero[keep].any(), "layer %d: %d kept elements are +0.0" % (k, zero[keep].sum())
        elif t.numel() >= 4096:
            other = ~dr.keep_mask(dr.layer_seed(step_seed, k) + 1, tuple(t.shape), p)
            viol = (~zero[other]).mean()
            assert viol >= 0.01, "layer %d: the control mask (seed + 1) is violated by only %.4f of its dropped elements" % (k, viol)


@pytest.mark.parametrize("slope", [0.0, 0.1])
@pytest.mark.parametrize("driver", ["python", "native"])
@pytest.mark.parametrize("B,H,W", [(2, 64, 64), (1, 50, 84)])
def test_network_seed_schedule(B, H, W, driver, slope):
    model = policy(DEV, 11, dropout=P)
    model.train()
    x = torch.rand(B, 1, H, W, generator=torch.Generator().manual_seed(3)).to(DEV)
    uh.DEBUG = {}
    try:
        uh.unet_mask(model, x, training=True, seed=9, slope=slope, driver=driver)
        tensors = _layer_tensors(uh.DEBUG["fwd"])
    finally:
        uh.DEBUG = None
    _check_schedule(tensors, 9, exact=slope > 0)


def test_policy_advances_the_step_seed():
    """Two consecutive training forwards of the policy draw with _step and _step + 1 (first layer's mask of both)."""
    model = policy(DEV, 11, dropout=P)
    assert model.unet_backend == "hip"
    model.train()
    g = torch.Generator().manual_seed(4)
    scan = {"fft_data": torch.rand(2, 64, 64, generator=g), "fft_cfar": torch.rand(2, 64, 64, generator=g), "raw_pc": torch.zeros(2, 4, 3)}
    first = []
    for _ in range(2):
        uh.DEBUG = {}
        try:
            model(scan, {"pc": torch.zeros(2, 4, 6)}, None, mask_only=True)
            first.append((model._step, uh.DEBUG["fwd"]["enc"]["e0"][1]))
        finally:
            uh.DEBUG = None
    assert first[1][0] == first[0][0] + 1
    for step, t in first:
        assert t.numel() >= 4096
        zero = _bits(t) == 0
        assert zero[~dr.keep_mask(dr.layer_seed(step, 1), tuple(t.shape), P)].all()
        for wrong in (step - 1, step + 1):            # the other pass's seed does not fit
            assert (~zero[~dr.keep_mask(dr.layer_seed(wrong, 1), tuple(t.shape), P)]).mean() >= 0.01


@pytest.mark.parametrize("slope", [0.0, 0.1])
def test_batch_norm_network_seed_schedule(slope):
    """The BatchNorm network draws in bn_apply behind each block's second BatchNorm, same schedule; it stores a kept zero as
    -0.0 whatever the activation, so the zero pattern is the mask exactly."""
    from mm_masking_amd import unet_hip_bn as ub
    model = policy(DEV, 11, dropout=P, batch_norm=True, leaky=slope > 0, norm_weights=False)
    model.train()
    x = torch.rand(2, 1, 64, 64, generator=torch.Generator().manual_seed(3)).to(DEV)
    uh.DEBUG = {}
    try:
        ub.unet_mask(model, x, training=True, seed=9, slope=slope)
        saved = uh.DEBUG["fwd_bn"]["saved"]
    finally:
        uh.DEBUG = None
    tensors = [saved[("e", i)][5] for i in range(6)]
    for j in range(5):
        tensors += [saved[("d", j, 0)][5], saved[("d", j, 1)][5]]
    _check_schedule(tensors, 9, exact=True)
