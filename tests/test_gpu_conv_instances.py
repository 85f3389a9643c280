"""Every kernel instance the convolution dispatch of csrc/mmk_unet.hip can launch (tests/conv_cases.py: instance_of and the
class lists), at the smallest shapes where its tile logic has an edge, against the fp64 reference of tests/conv_ref.py under
the error bound derived there -- no tolerance in this file comes from an observed error.

Guard bands: every output, partial-slice buffer and accumulate target is a view inside a larger buffer with 4 KiB of a fixed
byte pattern on both sides, which must come back unchanged; outputs that are not accumulate targets start as NaN and must come
back finite; every input is a view between 4 KiB bands of bf16 NaN, so that a halo read outside the tensor which reaches the
arithmetic shows up as NaN.  The bands are part of the same allocation: a stray access lands in them instead of faulting.

Each case prints `RATIO <family> <case> <largest |got - ref| / bound>`; run with -s to collect them."""
import ctypes
import re

import numpy as np
import pytest
import torch

import conv_cases as cc
import conv_ref as cr
from mm_masking_amd import _lib
from mm_masking_amd import unet_hip as uh

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
BF16 = torch.bfloat16
F64 = torch.float64
BAND = 4096


def _pattern(lo, hi):
    return torch.tensor([lo, hi] * (BAND // 2), dtype=torch.uint8, device=DEV)


class Guarded:
    """A tensor of `shape` between two BAND-byte bands.  out=False: an input (bands of bf16 NaN, 0x7FC0); out=True: an output
    (bands 0xA55A; the tensor itself NaN unless `init` gives its content)."""

    def __init__(self, init=None, shape=None, dtype=BF16, out=False):
        if init is not None:
            shape, dtype = tuple(init.shape), init.dtype
        nbytes = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size()
        self.pat = _pattern(0x5A, 0xA5) if out else _pattern(0xC0, 0x7F)
        self.buf = torch.empty(2 * BAND + nbytes, dtype=torch.uint8, device=DEV)
        self.buf[:BAND] = self.pat
        self.buf[BAND + nbytes:] = self.pat
        self.t = self.buf[BAND:BAND + nbytes].view(dtype).view(shape)
        assert self.t.data_ptr() % 16 == 0
        if init is not None:
            self.t.copy_(init)
        else:
            self.t.fill_(float("nan"))
        self.nbytes = nbytes

    def intact(self):
        return torch.equal(self.buf[:BAND], self.pat) and torch.equal(self.buf[BAND + self.nbytes:], self.pat)


def _family(inst):
    d = inst[-1]
    if isinstance(d, cc.Deep):
        if d.SUBW:
            return "deep_subw"
        if d.POOLG:
            return "deep_poolg"
        return "deep_leaky" if d.LK else "deep_role%d" % d.ROLE
    if isinstance(d, cc.Thin):
        return "thin_" + d.path
    return "wgrad_deep" if isinstance(d, cc.WgradDeep) else "wgrad_thin"


def _report(c, ratio):
    print("RATIO %s %s %.4f" % (_family(cc.instance_of(c)), c.name, ratio))


def _run_conv(c):
    """The case through mmk_conv3x3 with every operand guarded: (output (B,H,W,COUT) bf16 on the device, list of Guarded)."""
    o = cc.shared(c)
    c1 = c.cin if c.c1 is None else c.c1
    o1 = c.cout if c.o1 is None else c.o1
    x1 = Guarded(o["x"][..., :c1])
    x2 = Guarded(o["x"][..., c1:]) if c1 < c.cin else None
    arg = Guarded(o["arg"]) if c.pooled else None
    wp = uh.pack_weights((o["wt"] if c.transposed else o["w"]).to(DEV), transposed=c.transposed)
    halves = ((0, o1), (o1, c.cout))
    srcs = [Guarded(o["src"][..., lo:hi]) if s else None for s, (lo, hi) in zip(c.src, halves)]
    outs = [None if hi == lo else
            (Guarded(o["base"][..., lo:hi], out=True) if a else Guarded(shape=(c.B, c.H, c.W, hi - lo), out=True))
            for a, (lo, hi) in zip(c.acc, halves)]
    t = lambda g: None if g is None else g.t
    uh.conv3x3(x1.t, wp, c.cout, bias=o["bias"].to(DEV) if c.bias else None, x2=t(x2), relu=c.relu, drop_p=c.drop_p, seed=cc.SEED,
               out=outs[0].t, out2=t(outs[1]), split=o1 if o1 < c.cout else None, relu_src=t(srcs[0]), scale=c.scale[0],
               relu_src2=t(srcs[1]), scale2=c.scale[1], accumulate=c.acc[0], accumulate2=c.acc[1], slope=c.slope,
               x1_pool_arg=t(arg), x1_pool_scale=c.pool_scale, hw=(c.H, c.W) if c.pooled else None)
    torch.cuda.synchronize()
    got = torch.cat([g.t for g in outs if g is not None], dim=3)
    return got, [g for g in [x1, x2, arg] + srcs + outs if g is not None]


def _check_conv(c, got, guards, ref):
    assert all(g.intact() for g in guards), "guard band changed: " + c.name
    assert bool(torch.isfinite(got.float()).all()), "NaN reached the output: " + c.name
    ratio, outside = cr.worst(got.to(ref.y.device), ref.y, ref.S, 9 * c.cin)
    _report(c, ratio)
    assert outside == 0, (c.name, cc.instance_of(c), "elements outside the bound: %d, largest ratio %.3f" % (outside, ratio))
    if ref.keep is not None and c.slope > 0:            # LeakyReLU network: a dropped element is +0.0, a kept zero -0.0
        assert torch.equal(got.view(torch.int16).to(ref.keep.device) == 0, ~ref.keep), c.name
    return ratio


@pytest.mark.parametrize("c", [c for c in cc.CONV_CASES if "_subw_" not in c.name], ids=lambda c: c.name)
def test_conv_instance(c):
    assert not isinstance(cc.instance_of(c), cc.Refused)
    got, guards = _run_conv(c)
    ref, _ = cc.conv_ref_of(c)
    _check_conv(c, got, guards, ref)


@pytest.mark.parametrize("c", [c for c in cc.CONV_CASES if "_subw_" in c.name], ids=lambda c: c.name)
def test_conv_sub_batch_split(c, monkeypatch):
    """A launch of exactly two rounds of tiles: the first images as one round of the layer's own kernel, the rest as a launch of
    32-channel blocks (SUBW) on the wider kernel's weight packing.  Against the reference (fp64 on the device: the only large
    batches of this file) and bit-equal to the single launch."""
    assert cc.instance_of(c)[-1].SUBW and cc.split_plan(c) is not None
    monkeypatch.delenv("MMK_CONV_SPLIT", raising=False)
    got, guards = _run_conv(c)
    ref, _ = cc.conv_ref_of(c, device=DEV)
    _check_conv(c, got, guards, ref)
    monkeypatch.setenv("MMK_CONV_SPLIT", "0")
    one, guards1 = _run_conv(c)
    assert all(g.intact() for g in guards1)
    assert torch.equal(one.view(torch.int16), got.view(torch.int16))
    Bm = cc.split_plan(c)[0]                            # the dropout draws continue across the split
    assert int((got[:Bm] == 0).sum()) > 0 and int((got[Bm:] == 0).sum()) > 0


def test_pool_codes_of_the_cases_are_the_kernels():
    """The arg-max codes the pooled cases use are the reference's; mmk_maxpool2_fwd_arg gives the same bytes."""
    for c in cc.ALL_CASES:
        if c.pooled:
            C = c.cin if c.kind == "conv" else c.cout
            pre = cc.pre_pool(c, C)
            y, arg = uh.maxpool2_arg(pre.to(DEV))
            assert torch.equal(arg.cpu(), cc.shared(c)["arg"]), c.name
            assert torch.equal(y.cpu().to(F64), cr.pool_codes(pre)[0]), c.name
            seen = set(torch.unique(cr.unpack_codes(arg.cpu())).tolist())
            assert seen >= {0, 4, 5, 6, 7}, seen


# ------------------------------------------------------------------------------------------------ weight gradients
def _reduced(part, cout, cin):
    db = Guarded(shape=(cout,), dtype=torch.float32, out=True)
    dW = uh.wgrad_unpack_batch([(part.t, cout, cin, db.t)])[0]
    torch.cuda.synchronize()
    return dW.cpu(), db


@pytest.mark.parametrize("c", cc.WGRAD_CASES, ids=lambda c: c.name)
def test_wgrad_instance(c):
    o = cc.shared(c)
    c1 = c.cin if c.c1 is None else c.c1
    ns = uh.wgrad_slices(c.cout, c.cin, c1, c.B, c.H, c.W)
    assert ns > 0
    x1 = Guarded(o["x"][..., :c1])
    x2 = Guarded(o["x"][..., c1:]) if c1 < c.cin else None
    g = Guarded(o["g"])
    arg = Guarded(o["arg"]) if c.pooled else None
    part = Guarded(shape=(ns, 9 * c.cout * c.cin + c.cout), dtype=torch.float32, out=True)
    kw = dict(x2=None if x2 is None else x2.t, g_pool_arg=None if arg is None else arg.t, g_pool_scale=c.pool_scale)
    uh.conv3x3_wgrad_partial(x1.t, g.t, c.cout, part.t, **kw)
    dW, db = _reduced(part, c.cout, c.cin)
    rkw = dict(g_pool_arg=o["arg"], g_pool_scale=c.pool_scale, hw=(c.H, c.W)) if c.pooled else {}
    ref = cr.wgrad_ref(o["x"][..., :c1], o["x"][..., c1:] if c1 < c.cin else None, o["g"], **rkw)
    guards = [q for q in (x1, x2, g, arg, part, db) if q is not None]
    worst = 0.0
    for k in (1, 2):                                    # k = 2: a second application accumulated into the same slices
        assert all(q.intact() for q in guards), "guard band changed: " + c.name
        assert bool(torch.isfinite(part.t).all()) and bool(torch.isfinite(db.t).all())
        n = k * c.B * c.H * c.W + ns
        rW, oW = cr.worst(dW, k * ref.dW, k * ref.SW, n, fp32_out=True)
        rb, ob = cr.worst(db.t.cpu(), k * ref.db, k * ref.Sb, n, fp32_out=True)
        worst = max(worst, rW, rb)
        assert oW == 0 and ob == 0, (c.name, cc.instance_of(c), k, oW, rW, ob, rb)
        if k == 1:
            uh.conv3x3_wgrad_partial(x1.t, g.t, c.cout, part.t, accumulate=True, **kw)
            dW, db2 = _reduced(part, c.cout, c.cin)
            guards.append(db2)
            db = db2
    _report(c, worst)


# ------------------------------------------------------------------------------------------------ pooling / up-sampling adjoints
def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _src_with_zeros(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return cc._signed_zeros(torch.randn(*shape, generator=g).to(BF16), g)


@pytest.mark.parametrize("slope", [0.1, 0.0])
@pytest.mark.parametrize("C,H,W", [(8, 9, 13), (32, 7, 11), (32, 8, 10)])
def test_maxpool2_bwd_slope(C, H, W, slope):
    B, scale = 2, cc.INV95
    d = _src_with_zeros((B, H, W, C), 500 + C + H)                  # +0.0 / -0.0 maxima, ties among them
    d = torch.where(d.float().abs() > 1.2, torch.full_like(d, -0.0), d)
    gy = torch.randn(B, H // 2, W // 2, C, generator=torch.Generator().manual_seed(7)).to(BF16)
    gd, gg = Guarded(d), Guarded(gy)
    gz = Guarded(shape=(B, H, W, C), out=True)
    _lib.check(_lib.lib().mmk_maxpool2_bwd(_p(gd.t), _p(gg.t), B, H, W, C, float(scale), float(slope), _p(gz.t), _lib.stream_ptr(DEV)))
    torch.cuda.synchronize()
    ref, S = cr.maxpool2_bwd_ref(d, gy, scale, slope)
    assert gd.intact() and gg.intact() and gz.intact()
    ratio, outside = cr.worst(gz.t.cpu(), ref, S, 1)
    print("RATIO aux maxpool2_bwd_%d_%dx%d_slope%g %.4f" % (C, H, W, slope, ratio))
    assert outside == 0, (outside, ratio)


@pytest.mark.parametrize("slope", [0.1, 0.0])
@pytest.mark.parametrize("C,Hs,Ws,Ho,Wo", [(8, 9, 13, 19, 27), (32, 5, 7, 11, 15), (32, 3, 5, 7, 10)])
def test_upsample_bwd_slope(C, Hs, Ws, Ho, Wo, slope):
    B, scale = 2, cc.INV95
    gy = torch.randn(B, Ho, Wo, C, generator=torch.Generator().manual_seed(600 + C + Hs)).to(BF16)
    src = _src_with_zeros((B, Hs, Ws, C), 700 + C + Hs)
    gg, gs = Guarded(gy), Guarded(src)
    gx = Guarded(shape=(B, Hs, Ws, C), out=True)
    _lib.check(_lib.lib().mmk_upsample_bwd(_p(gg.t), B, Hs, Ws, C, Ho, Wo, _p(gs.t), float(scale), float(slope), _p(gx.t),
                                           _lib.stream_ptr(DEV)))
    torch.cuda.synchronize()
    ref, S, n = cr.upsample_bwd_ref(gy, Hs, Ws, src, scale, slope)
    assert gg.intact() and gs.intact() and gx.intact()
    ratio, outside = cr.worst(gx.t.cpu(), ref, S, n)
    print("RATIO aux upsample_bwd_%d_%dx%d_slope%g %.4f" % (C, Hs, Ws, slope, ratio))
    assert outside == 0, (outside, ratio)


# ------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("c", cc.REFUSED_CASES, ids=lambda c: c.name)
def test_refused_by_the_dispatch(c):
    """What no kernel stages is an error with the dispatch's own text, not another path."""
    inst = cc.instance_of(c)
    assert isinstance(inst, cc.Refused)
    o = cc.shared(c)
    with pytest.raises(_lib.MmkError, match=re.escape(inst.text)):
        if c.kind == "wgrad":
            ns = max(1, uh.wgrad_slices(c.cout, c.cin, c.cin, c.B, c.H, c.W))
            uh.conv3x3_wgrad_partial(o["x"].to(DEV), o["g"].to(DEV), c.cout, uh.partial_buffer(ns, c.cout, c.cin, DEV),
                                     g_pool_arg=o["arg"].to(DEV))
        else:
            wp = uh.pack_weights((o["wt"] if c.transposed else o["w"]).to(DEV), transposed=c.transposed)
            o1 = c.cout if c.o1 is None else c.o1
            src = o["src"].to(DEV)
            uh.conv3x3(o["x"].to(DEV), wp, c.cout, relu=c.relu, slope=c.slope, split=c.o1,
                       out=o["base"][..., :o1].contiguous().to(DEV) if c.acc[0] else None, accumulate=c.acc[0],
                       relu_src=src[..., :o1].contiguous() if c.src[0] else None,
                       relu_src2=src[..., o1:].contiguous() if c.src[1] else None,
                       x1_pool_arg=o["arg"].to(DEV) if c.pooled else None, hw=(c.H, c.W) if c.pooled else None)
    torch.cuda.synchronize()
