"""tests/conv_ref.py, its error bound and the case table of tests/conv_cases.py, checked without a GPU: the reference against
torch's own fp64 operators and autograd, the bound against an fp32 emulation of the kernels' arithmetic on every row of the GPU
case table (it must accept every element) and against one-line mutants of the reference (it must reject each), and the table
against the explicit list of kernel instances the dispatch can launch."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_cases as cc
import conv_ref as cr
import dropout_ref as dr

F64 = torch.float64
BF16 = torch.bfloat16


def _rand(shape, seed, scale=1.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).to(BF16)


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1)


# ------------------------------------------------------------------------------------------------ the reference
def test_conv_ref_is_conv2d_fp64():
    x1, x2 = _rand((2, 7, 9, 8), 1), _rand((2, 7, 9, 16), 2)
    w = torch.randn(32, 24, 3, 3, generator=torch.Generator().manual_seed(3))
    r = cr.conv_ref(x1, w, x2=x2)
    x = torch.cat([x1, x2], dim=3).to(F64)
    want = _nhwc(F.conv2d(_nchw(x), cr.bf16v(w), padding=1))
    assert torch.allclose(r.y, want, rtol=0, atol=1e-12)
    wantS = _nhwc(F.conv2d(_nchw(x.abs()), cr.bf16v(w).abs(), padding=1))
    assert torch.allclose(r.S, wantS, rtol=0, atol=1e-12)
    assert bool((r.S >= r.y.abs() - 1e-12).all())


def test_wgrad_ref_and_transposed_operator_are_autograd_fp64():
    x1, x2 = _rand((2, 6, 5, 8), 4), _rand((2, 6, 5, 8), 5)
    g = _rand((2, 6, 5, 24), 6)
    w = torch.randn(24, 16, 3, 3, generator=torch.Generator().manual_seed(7))
    x = torch.cat([x1, x2], dim=3).to(F64).requires_grad_(True)
    wq = cr.bf16v(w).requires_grad_(True)
    b = torch.zeros(24, dtype=F64, requires_grad=True)
    y = _nhwc(F.conv2d(_nchw(x), wq, b, padding=1))
    (y * g.to(F64)).sum().backward()
    r = cr.wgrad_ref(x1, x2, g)
    assert torch.allclose(r.dW, wq.grad, rtol=0, atol=1e-11)
    assert torch.allclose(r.db, b.grad, rtol=0, atol=1e-11)
    assert bool((r.SW >= r.dW.abs() - 1e-11).all()) and bool((r.Sb >= r.db.abs() - 1e-11).all())
    dx = cr.conv_ref(g, w, transposed=True)                      # the data gradient: the transposed-packed operator on g
    assert torch.allclose(dx.y, x.grad, rtol=0, atol=1e-11)


def _pre_pool(B, H, W, C, seed):
    pre = (torch.randn(B, H, W, C, generator=torch.Generator().manual_seed(seed)) * 1.5).round() * 0.5
    pre[..., 0::5] = pre[..., 0::5].clamp_max(0)
    pre[..., 3::7] = -pre[..., 3::7].abs() - 0.5
    return pre.to(BF16)


@pytest.mark.parametrize("H,W", [(6, 8), (7, 9)])
def test_pool_codes_are_max_pool2d_with_indices(H, W):
    """Ties (values on a grid of 0.5) and windows without a positive value: torch's CPU max_pool2d also takes the first maximum
    in scan order."""
    pre = _pre_pool(2, H, W, 16, 11)
    py, nib = cr.pool_codes(pre)
    ty, ti = F.max_pool2d(_nchw(pre.to(F64)), 2, 2, return_indices=True)
    assert torch.equal(py, _nhwc(ty))
    iy, ix = _nhwc(ti) // W, _nhwc(ti) % W
    assert torch.equal(nib & 3, (iy % 2) * 2 + (ix % 2))
    assert torch.equal((nib >> 2) == 1, py > 0)
    assert int((py <= 0).sum()) > 0 and int((py > 0).sum()) > 0
    win = pre.to(F64)[:, :2 * (H // 2), :2 * (W // 2)].reshape(2, H // 2, 2, W // 2, 2, 16)
    assert int(((win == py[:, :, None, :, None, :]).sum(dim=(2, 4)) > 1).sum()) > 0           # tied windows occur
    assert torch.equal(cr.unpack_codes(cr.pack_codes(nib)), nib)
    r = cr.conv_ref(pre, torch.zeros(16, 16, 3, 3), bias=pre.new_zeros(16).float(), pool=True)   # (conv of zero weights: y = 0)
    assert r.pool_y.shape == (2, H // 2, W // 2, 16) and torch.equal(r.pool_arg, torch.zeros_like(r.pool_arg))


@pytest.mark.parametrize("H,W", [(6, 8), (7, 9)])
def test_pooled_forms_are_adjoint_then_plain(H, W):
    C = 16
    pre = _pre_pool(2, H, W, C, 21)
    arg = cr.pack_codes(cr.pool_codes(pre)[1])
    gy = _rand((2, H // 2, W // 2, C), 22, 0.3)
    scale = 1.0 / 0.95
    adj = cr.pool_adjoint(gy, arg, H, W, scale)
    # the adjoint itself: autograd of max_pool2d on the pre-pool tensor, times (maximum > 0), times scale, rounded to bf16
    p = _nchw(pre.to(F64)).clone().requires_grad_(True)
    m = F.max_pool2d(p, 2, 2)
    gv = (gy.float() * torch.tensor(np.float32(scale))).to(BF16).to(F64)
    (m * _nchw(gv) * (m.detach() > 0)).sum().backward()
    assert torch.equal(adj, _nhwc(p.grad))
    w = torch.randn(C, C, 3, 3, generator=torch.Generator().manual_seed(23))
    src = _rand((2, H, W, C), 24)
    a = cr.conv_ref(gy, w, x1_pool_arg=arg, x1_pool_scale=scale, hw=(H, W), relu_src=(src, None), transposed=True)
    b = cr.conv_ref(adj, w, relu_src=(src, None), transposed=True)
    assert torch.equal(a.y, b.y) and torch.equal(a.S, b.S)
    x = _rand((2, H, W, 8), 25)
    wa = cr.wgrad_ref(x, None, gy, g_pool_arg=arg, g_pool_scale=scale, hw=(H, W))
    wb = cr.wgrad_ref(x, None, adj)
    assert torch.equal(wa.dW, wb.dW) and torch.equal(wa.db, wb.db)


def test_aux_references_are_autograd_fp64():
    """maxpool2_bwd_ref (slope = 0, positive maxima) is max_pool2d's autograd; upsample_bwd_ref is the adjoint of the matrix
    form of the up-sampling, whose weights are F.interpolate(align_corners=True)'s to fp32 accuracy."""
    d = _rand((2, 7, 9, 8), 31).abs() + 0.25
    gy = _rand((2, 3, 4, 8), 32)
    p = _nchw(d.to(F64)).clone().requires_grad_(True)
    (F.max_pool2d(p, 2, 2) * _nchw(gy.to(F64))).sum().backward()
    gz, _ = cr.maxpool2_bwd_ref(d, gy, 1.0)
    assert torch.equal(gz, _nhwc(p.grad))
    gz2, _ = cr.maxpool2_bwd_ref(-d, gy, 2.0, slope=0.1)                        # negative maxima: slope * scale
    assert int((gz2 != 0).sum()) == gy.numel() and torch.allclose(gz2.abs().sum(), (gy.to(F64).abs() * cr.f32(0.1) * 2.0).sum())
    Hs, Ws, Ho, Wo = 4, 5, 9, 11
    g = _rand((2, Ho, Wo, 8), 33)
    xs = torch.randn(2, 8, Hs, Ws, dtype=F64, generator=torch.Generator().manual_seed(34)).requires_grad_(True)
    (F.interpolate(xs, size=(Ho, Wo), mode="bilinear", align_corners=True) * _nchw(g.to(F64))).sum().backward()
    gx, S, n = cr.upsample_bwd_ref(g, Hs, Ws)
    assert torch.allclose(gx, _nhwc(xs.grad), rtol=0, atol=1e-5) and n >= 8
    src = torch.tensor([1.0, -1.0, 0.0, -0.0], dtype=BF16)
    assert cr.bwd_factor(src, 2.0, 0.0).tolist() == [2.0, 0.0, 0.0, 0.0]
    assert torch.allclose(cr.bwd_factor(src, 2.0, 0.5), torch.tensor([2.0, 1.0, 0.0, 1.0], dtype=F64))


# ------------------------------------------------------------------------------------------------ the bound accepts the arithmetic
_F32_CONV = {}


def _f32(v):
    return torch.tensor(np.float32(v))


def _emulate_conv(c):
    """The kernels' arithmetic on the CPU: fp32 convolution of the bf16 operands, the epilogue in fp32 in the kernels' order, one
    rounding to bf16."""
    o = cc.shared(c)
    key = (c.cin, c.cout, c.B, c.H, c.W, c.pooled, c.transposed, c.pool_scale if c.pooled else None)
    if key not in _F32_CONV:
        if len(_F32_CONV) > 4:
            _F32_CONV.clear()
        x = o["x"]
        if c.pooled:
            x = cr.pool_adjoint(x, o["arg"], c.H, c.W, c.pool_scale)
        w = cr.op_weights(o["wt"] if c.transposed else o["w"], c.transposed).float()
        _F32_CONV[key] = _nhwc(F.conv2d(_nchw(x.float()), w, padding=1)).contiguous()
    v = _F32_CONV[key].clone()
    if c.bias:
        v = v + o["bias"]
    if c.relu:
        if c.slope > 0:
            v = torch.maximum(v, v * _f32(c.slope))
            v = torch.where(v == 0, torch.full_like(v, -0.0), v)
        else:
            v = v.clamp_min(0)
    P = dr.params(c.drop_p)
    if P.thr != 0:
        keep = torch.from_numpy(dr.keep_mask(cc.SEED, tuple(v.shape), c.drop_p))
        v = torch.where(keep, v * _f32(P.inv_keep), torch.zeros_like(v))
    o1 = c.cout if c.o1 is None else c.o1
    parts = []
    for i, (lo, hi) in enumerate(((0, o1), (o1, c.cout))):
        if hi == lo:
            continue
        p = v[..., lo:hi]
        if c.src[i]:
            s = o["src"][..., lo:hi].float()
            sc = _f32(c.scale[i])
            if c.slope > 0:
                neg = (s < 0) | ((s == 0) & torch.signbit(s))
                f = torch.where(s > 0, sc, torch.where(neg, sc * _f32(c.slope), _f32(0)))
            else:
                f = torch.where(s > 0, sc, _f32(0))
            p = p * f
        if c.acc[i]:
            p = p + o["base"][..., lo:hi].float()
        parts.append(p)
    return torch.cat(parts, dim=3).to(BF16)


@pytest.mark.parametrize("c", cc.CONV_CASES, ids=lambda c: c.name)
def test_bound_accepts_emulated_arithmetic(c):
    ref, _ = cc.conv_ref_of(c)
    got = _emulate_conv(c)
    ratio, outside = cr.worst(got, ref.y, ref.S, 9 * c.cin)
    assert outside == 0, (outside, ratio)
    if ref.keep is not None and c.slope > 0:                                  # the sign convention of the LeakyReLU network
        assert torch.equal(got.view(torch.int16) == 0, ~ref.keep)


@pytest.mark.parametrize("c", cc.WGRAD_CASES, ids=lambda c: c.name)
def test_bound_accepts_emulated_weight_gradient(c):
    o = cc.shared(c)
    c1 = c.cin if c.c1 is None else c.c1
    x1, x2 = o["x"][..., :c1], (o["x"][..., c1:] if c1 < c.cin else None)
    kw = dict(g_pool_arg=o["arg"], g_pool_scale=c.pool_scale, hw=(c.H, c.W)) if c.pooled else {}
    ref = cr.wgrad_ref(x1, x2, o["g"], **kw)
    g = cr.pool_adjoint(o["g"], o["arg"], c.H, c.W, c.pool_scale) if c.pooled else o["g"]
    xp = F.pad(o["x"].float(), (0, 0, 1, 1, 1, 1))
    g2 = g.float().reshape(-1, c.cout)
    got = torch.stack([torch.stack([g2.t() @ xp[:, ky:ky + c.H, kx:kx + c.W].reshape(-1, c.cin) for kx in range(3)], dim=-1)
                       for ky in range(3)], dim=-2)
    n = c.B * c.H * c.W + 1
    assert cr.worst(got, ref.dW, ref.SW, n, fp32_out=True)[1] == 0
    assert cr.worst(g2.sum(0), ref.db, ref.Sb, n, fp32_out=True)[1] == 0


# ------------------------------------------------------------------------------------------------ the bound rejects mutants
_MK = dict(cin=64, cout=16, H=5, W=7, c1=32)
MUTANT_KINDS = {
    "fwd": cc._case(name="m_fwd", bias=True, relu=True, **_MK),
    "fwd_drop": cc._case(name="m_fwd_drop", bias=True, relu=True, drop_p=0.05, **_MK),
    "lk_fwd_drop": cc._case(name="m_lk_fwd_drop", bias=True, relu=True, slope=0.1, drop_p=0.05, **_MK),
    "bwd_plain": cc._case(name="m_bwd_plain", transposed=True, **_MK),
    "bwd_src": cc._case(name="m_bwd_src", src=(True, False), scale=(cc.INV95, 1.0), transposed=True, **_MK),
    "bwd_acc": cc._case(name="m_bwd_acc", acc=(True, False), transposed=True, **_MK),
    "bwd_src_acc": cc._case(name="m_bwd_src_acc", src=(True, False), acc=(True, False), scale=(0.75, 1.0), transposed=True, **_MK),
    "lk_bwd_src": cc._case(name="m_lk_bwd_src", src=(True, False), scale=(cc.INV95, 1.0), slope=0.1, transposed=True, **_MK),
}
MUTANTS = ["tap_dropped", "scale_eps", "keep_twice", "drop_index_shift", "ge_relu_src", "slope_scale_swap", "x_swap",
           "last_chunk", "row_leak"]


def _applies(mut, c):
    if mut in ("scale_eps", "ge_relu_src"):
        return any(c.src)
    if mut in ("keep_twice", "drop_index_shift"):
        return c.drop_p > 0
    if mut == "slope_scale_swap":
        return any(c.src) and c.slope > 0
    return True


def _mutant(mut, c):
    """The fp64 reference of the case with one thing wrong."""
    o = cc.shared(c)
    x = o["x"].to(F64)
    w = cr.op_weights(o["wt"] if c.transposed else o["w"], c.transposed)
    val, S = cc.conv_core_of(c)
    val = val.clone()
    if mut == "tap_dropped":            # image 1, pixel (0, 0): the tap (ky, kx) = (2, 2), the in-image neighbour (1, 1)
        val[1, 0, 0] -= w[:, :, 2, 2] @ x[1, 1, 1]
        return cc.conv_ref_of(c, core=(val, S))[0].y
    if mut == "row_leak":               # image 1 reads the last row of image 0 as its row -1 (taps ky = 0 of output row 0)
        prev = F.pad(x[0, c.H - 1], (0, 0, 1, 1))
        for kx in range(3):
            val[1, 0] += prev[kx:kx + c.W] @ w[:, :, 0, kx].t()
        return cc.conv_ref_of(c, core=(val, S))[0].y
    if mut == "x_swap":                 # concat(x2, x1)
        xs = torch.cat([x[..., c.c1:], x[..., :c.c1]], dim=3)
        return cc.conv_ref_of(c, core=cr.conv_core(xs, w))[0].y
    if mut == "last_chunk":             # the last 32 input channels never reach the sum
        xs = x.clone()
        xs[..., -32:] = 0
        return cc.conv_ref_of(c, core=cr.conv_core(xs, w))[0].y
    if mut == "scale_eps":
        return cc.conv_ref_of(c, scale=tuple(s * (1 + 2.0 ** -6) for s in c.scale))[0].y
    if mut == "drop_index_shift":
        return cc.conv_ref_of(c, base_index=1)[0].y
    if mut == "keep_twice":
        r = cc.conv_ref_of(c)[0]
        return torch.where(r.keep, r.y * float(dr.params(c.drop_p).inv_keep), r.y)
    src = o["src"][..., :c.cout].to(F64)
    if mut == "ge_relu_src":            # src >= 0 counts as positive: +0.0 (and, in the ReLU network, -0.0) gets the scale
        pos = (src == 0) & (~torch.signbit(src) if c.slope > 0 else torch.ones_like(src, dtype=torch.bool))
        assert int(pos.sum()) > 0
        return cc.conv_ref_of(c, relu_src=(torch.where(pos, torch.ones_like(src), src), None))[0].y
    if mut == "slope_scale_swap":       # positive sources get slope * scale, negative ones scale
        return cc.conv_ref_of(c, relu_src=(torch.where(src != 0, -src, src), None))[0].y
    raise AssertionError(mut)


@pytest.mark.parametrize("mut", MUTANTS)
@pytest.mark.parametrize("kind", list(MUTANT_KINDS))
def test_bound_rejects_mutant(kind, mut):
    c = MUTANT_KINDS[kind]
    if not _applies(mut, c):
        return                          # (the mutant touches nothing this epilogue has)
    ref, _ = cc.conv_ref_of(c)
    clean = ref.y.to(BF16)
    assert cr.worst(clean, ref.y, ref.S, 9 * c.cin)[1] == 0
    ratio, outside = cr.worst(_mutant(mut, c).to(BF16), ref.y, ref.S, 9 * c.cin)
    assert outside > 0 and ratio > 1, (kind, mut, ratio)


def test_wgrad_bound_rejects_a_dropped_pixel_and_a_shifted_tap():
    c = cc._case(kind="wgrad", name="m_wg", cin=16, cout=16, H=9, W=33)
    o = cc.shared(c)
    ref = cr.wgrad_ref(o["x"], None, o["g"])
    n = c.B * c.H * c.W + 8
    assert cr.worst(ref.dW.float(), ref.dW, ref.SW, n, fp32_out=True)[1] == 0
    g = o["g"].clone()
    g[1, c.H - 1, c.W - 1] = 0                                                   # the last pixel of the last image left out
    assert cr.worst(cr.wgrad_ref(o["x"], None, g).dW.float(), ref.dW, ref.SW, n, fp32_out=True)[1] > 0
    assert cr.worst(ref.dW.flip(3).float(), ref.dW, ref.SW, n, fp32_out=True)[1] > 0


# ------------------------------------------------------------------------------------------------ the table covers the dispatch
def test_case_table_covers_every_instance():
    seen = set()
    for c in cc.ALL_CASES:
        inst = cc.instance_of(c)
        assert not isinstance(inst, cc.Refused), (c.name, inst)
        seen.update(inst)
    for c in cc.REFUSED_CASES:
        assert isinstance(cc.instance_of(c), cc.Refused), c.name
    wanted = set(cc.DEEP_CLASSES) | set(cc.THIN_CLASSES) | set(cc.WGRAD_CLASSES)
    assert len(cc.DEEP_CLASSES) == 42 and len(cc.THIN_CLASSES) == 16 and len(cc.WGRAD_CLASSES) == 19
    assert not (wanted - seen), sorted(map(str, wanted - seen))
    assert not (seen - wanted), sorted(map(str, seen - wanted))                   # a class the lists do not know: the dispatch grew
    for d in cc.DEEP_CLASSES:                                                     # every deep class at both tile widths
        assert d._replace(NT=8 - d.NT) in seen


def test_every_deep_class_has_a_ragged_row_in_each_direction():
    ragged_w, ragged_h = set(), set()
    for c in cc.CONV_CASES:
        for d in cc.instance_of(c):
            if isinstance(d, cc.Deep):
                # (the tail of a split launch has its own block width, hence its own tile height)
                if c.W % (d.NT * 16) != 0:
                    ragged_w.add(d)
                if c.H % cc.deep_th(d.BM) != 0:
                    ragged_h.add(d)
    assert set(cc.DEEP_CLASSES) <= ragged_w and set(cc.DEEP_CLASSES) <= ragged_h


def test_instance_of_on_the_shapes_the_issue_names():
    by = {c.name: c for c in cc.CONV_CASES}
    # 192 -> 32: resident at W <= 48, streamed above
    n3 = cc.instance_of(by["192-32_7x48_edge_fwd_bias_drop"])
    n5 = cc.instance_of(by["192-32_1x49_edge_fwd_bias_drop"])
    assert n3 == (cc.Deep(32, 3, 1, True, False, False, False),) and n5 == (cc.Deep(32, 5, 1, False, False, False, False),)
    # the two split launches: 300 tiles = two rounds, a one-round head of 42 / 85 images, a one-round 32-channel tail
    a, b = by["64-64_50x17x81_subw_fwd_bias_drop"], by["128-128_100x9x33_subw_fwd_bias_drop"]
    assert cc.deep_rounds(a.B, a.H, a.W, 64, 64, False) == (2, 6) and cc.split_plan(a) == (42, 8)
    assert cc.deep_rounds(b.B, b.H, b.W, 128, 128, True) == (2, 3) and cc.split_plan(b) == (85, 15)
    assert cc.instance_of(a) == (cc.Deep(64, 5, 1, True, False, False, False), cc.Deep(32, 5, 1, False, False, False, True))
    assert cc.instance_of(b) == (cc.Deep(128, 3, 1, False, False, False, False), cc.Deep(32, 3, 1, False, False, False, True))
    assert cc.split_plan(a._replace(no_split=True)) is None
    # roles: ReLU source and accumulate on one half, and a bias without activation, are the generic role
    assert cc.instance_of(by["64-64_9x81_nt5_bwd_src_acc"])[0].ROLE == 0
    assert cc.instance_of(by["64-64_9x81_nt5_lin_bias"])[0].ROLE == 0
    assert cc.instance_of(by["64-64_9x81_nt5_bwd_split_acc_src"])[0].ROLE == 2
    assert cc.instance_of(by["128-16_9x81_nt5_fwd_bias"]) == (cc.Deep(16, 5, 0, False, False, False, False),)
    assert cc.instance_of(by["64-64_17x35_poolg_src"]) == (cc.Deep(64, 3, 2, True, False, True, False),)
    assert cc.instance_of(by["128-128_9x51_poolg_acc"]) == (cc.Deep(128, 5, 2, False, False, True, False),)
    assert len({c.name for c in cc.ALL_CASES + cc.REFUSED_CASES}) == len(cc.ALL_CASES + cc.REFUSED_CASES)
