"""The case table of tests/test_gpu_conv_instances.py, the operands of every case (CPU tensors, built from the case alone), and
instance_of(): a restatement of the dispatch of csrc/mmk_unet.hip that names the kernel instance(s) a case launches.  No import
of the package, no GPU: tests/test_conv_ref_cpu.py checks the table against the explicit class lists at the end of this file.

What instance_of restates (csrc/mmk_unet.hip):
  conv_ck / conv_is_deep / conv_cm (:88-94), cin_chunk / cout_group (:83-84), xcd_grid (:162-171), DeepCfg and DeepCfg::smem
  (:1022-1042), deep_weights_fit (:1555), with_deep_cfg and narrow = W <= 48 (:1560-1565, :1590), the sub-batch split of
  dispatch_conv_deep (:1587-1626), the role rule and the instance choice of dispatch_conv_deep_plain (:1628-1662),
  with_thin_shape and dispatch_conv with its ring rule and the refusal of a split inside a lane's channel run (:1673-1721),
  wgrad_is_deep (:2677), with_wgrad_shape and its G8 rule (:2695-2705), dispatch_wgrad (:2707-2720)."""
import collections
import functools

import torch

import conv_ref as cr
from dropout_ref import params

BF16 = torch.bfloat16

_FIELDS = dict(name="", kind="conv", cin=0, cout=0, B=2, H=0, W=0, c1=None, o1=None, bias=False, relu=False, slope=0.0,
               drop_p=0.0, src=(False, False), acc=(False, False), scale=(1.0, 1.0), pooled=False, pool_scale=1.0,
               transposed=False, no_split=False)
Case = collections.namedtuple("Case", list(_FIELDS))


def _case(**kw):
    c = dict(_FIELDS)
    c.update(kw)
    return Case(**c)


# ------------------------------------------------------------------------------------------------ the dispatch, restated
def conv_ck(cin):
    return 32 if cin >= 32 else cin


def conv_is_deep(cin, cout):
    return cin >= 64 or (cin == 32 and cout >= 64)


def conv_cm(cin, cout):
    if conv_is_deep(cin, cout):
        return 128 if cout >= 128 else (16 if cout <= 16 else cout)
    return 64 if cout >= 64 else (16 if cout <= 16 else cout)


def cin_chunk(cin):
    return 64 if cin >= 64 else cin


def cout_group(cout):
    return 64 if cout >= 64 else (16 if cout <= 16 else cout)


def wgrad_is_deep(cout, cin, c1):
    return cin % 64 == 0 and cout % 64 == 0 and c1 % 64 == 0


def deep_th(BM):
    return 4 if BM >= 128 else 8             # DeepCfg: WM = BM >= 128 ? 2 : 1, TH = WN = 8 / WM


def deep_smem(BM, NT, wchunks):
    ht, wt = deep_th(BM) + 2, NT * 16 + 2
    return ht * wt * 48 * 2 + wchunks * (9 * (BM // 16) * 64 * 8 * 2) + BM * 4


def deep_weights_fit(BM, NT, cin):
    return deep_smem(BM, NT, cin // 32) <= 160 * 1024


def xcd_grid(B, H, W, tile_h, tile_w, groups, per_cu):
    tiles = -(-W // tile_w) * -(-H // tile_h)
    total = tiles * B
    per_xcd = (total + 7) // 8
    nb = (32 * per_cu) // groups
    nb = 1 if nb < 1 else min(nb, per_xcd)
    return dict(tiles=tiles, total=total, per_xcd=per_xcd, nb=nb, rounds=-(-per_xcd // nb))


def deep_rounds(B, H, W, cout, BM, narrow):
    g = xcd_grid(B, H, W, deep_th(BM), 48 if narrow else 80, -(-cout // BM), 1)
    return g["rounds"], g["tiles"]


Deep = collections.namedtuple("Deep", "BM NT ROLE resident LK POOLG SUBW")
Thin = collections.namedtuple("Thin", "CK CM path")
Wgrad = collections.namedtuple("Wgrad", "K M G8 pooled")
WgradDeep = collections.namedtuple("WgradDeep", "pooled")
Refused = collections.namedtuple("Refused", "text")


def split_plan(c):
    """(images of the head launch, images of the 32-channel tail launch) of dispatch_conv_deep's sub-batch split, or None."""
    BM, narrow = conv_cm(c.cin, c.cout), c.W <= 48
    forward_role = c.relu and not any(c.src) and not any(c.acc)
    if c.no_split or not forward_role or c.slope != 0 or BM not in (64, 128) or c.cout % 32 != 0:
        return None
    rounds, tpi = deep_rounds(c.B, c.H, c.W, c.cout, BM, narrow)
    if rounds != 2:
        return None
    groups = -(-c.cout // BM)
    nb = max(1, 32 // groups)
    Bm = (8 * nb) // tpi
    Bt = c.B - Bm
    under_filled = c.B * tpi * groups * 10 < 256 * 2 * 7
    o1 = c.cout if c.o1 is None else c.o1
    if (Bm >= 1 and Bt >= 1 and under_filled and deep_rounds(Bm, c.H, c.W, c.cout, BM, narrow)[0] == 1
            and deep_rounds(Bt, c.H, c.W, c.cout, 32, narrow)[0] == 1 and o1 % 32 == 0 and (c.cout - o1) % 32 == 0):
        return Bm, Bt
    return None


def _deep_plain(c):
    BM, NT = conv_cm(c.cin, c.cout), 3 if c.W <= 48 else 5
    any_src, any_acc = any(c.src), any(c.acc)
    both = any(s and a for s, a in zip(c.src, c.acc))
    if c.relu and not any_src and not any_acc:
        role = 1
    elif not c.relu and not c.bias and params(c.drop_p).thr == 0 and not both:
        role = 2
    else:
        role = 0
    resident = BM <= 64 and deep_weights_fit(BM, NT, c.cin)
    if c.slope > 0:
        return Deep(BM, NT, 0, False, True, False, False)
    if c.pooled:
        if BM >= 64 and role == 2:
            if resident:
                return Deep(BM, NT, 2, True, False, True, False)
            if BM > 64:
                return Deep(BM, NT, 2, False, False, True, False)
        return Refused("mmk_conv3x3: x1_pool_arg is not supported for this layer (CIN=%d COUT=%d)" % (c.cin, c.cout))
    if BM >= 32 and role in (1, 2):
        return Deep(BM, NT, role, resident, False, False, False)
    return Deep(BM, NT, 0, False, False, False, False)


def instance_of(c):
    """The kernel instances the case launches, as a tuple (two for a split deep launch), or a Refused with the error text."""
    if c.kind == "wgrad":
        c1 = c.cin if c.c1 is None else c.c1
        if c.pooled:
            if wgrad_is_deep(c.cout, c.cin, c1):
                return (WgradDeep(True),)
            if c.cin == 32 and c.cout == 32:
                return (Wgrad(32, 32, False, True),)
            return Refused("mmk_conv3x3_wgrad_partial_pooled: unsupported channel counts CIN=%d COUT=%d" % (c.cin, c.cout))
        if wgrad_is_deep(c.cout, c.cin, c1):
            return (WgradDeep(False),)
        return (Wgrad(cin_chunk(c.cin), cout_group(c.cout), c.cout == 8, False),)
    assert c.kind == "conv"
    if c.pooled and (c.slope > 0 or c.c1 is not None or c.H < 2 or c.W < 2):
        return Refused("mmk_conv3x3: x1_pool_arg needs the ReLU network, a single input and H, W >= 2")
    if conv_is_deep(c.cin, c.cout):
        o1 = c.cout if c.o1 is None else c.o1
        if o1 < c.cout and conv_cm(c.cin, c.cout) >= 64 and o1 % 16 != 0:      # (a lane's run of 16 channels goes to ONE half)
            return Refused("mmk_conv3x3: output split %d+%d: layers of >= 64 output channels split at multiples of 16"
                           % (o1, c.cout - o1))
        plan = split_plan(c)
        if plan is not None:
            head = _deep_plain(c._replace(B=plan[0]))
            return (head, Deep(32, head.NT, 1, False, False, False, True))
        r = _deep_plain(c)
        return r if isinstance(r, Refused) else (r,)
    CK, CM = conv_ck(c.cin), conv_cm(c.cin, c.cout)
    epi = any(c.src) or any(c.acc)
    if c.pooled and not (c.cin == 32 and CM == 32 and epi):
        return Refused("mmk_conv3x3: x1_pool_arg is not supported for this layer (CIN=%d COUT=%d)" % (c.cin, c.cout))
    if c.slope > 0:
        return (Thin(CK, CM, "leaky"),)
    return (Thin(CK, CM, "ring" if CM <= 32 else "pipelined"),)     # (one chunk always: a thin layer has CIN = CK; 32 -> 64 is deep)


# ------------------------------------------------------------------------------------------------ the classes the dispatch can launch
def _deep_classes():
    out = []
    for NT in (3, 5):
        for BM in (16, 32, 64, 128):
            out.append(Deep(BM, NT, 0, False, True, False, False))                     # LeakyReLU: the generic role, never resident
            out.append(Deep(BM, NT, 0, False, False, False, False))                    # generic role
            if BM >= 32:
                for role in (1, 2):
                    out.append(Deep(BM, NT, role, False, False, False, False))
                    if BM <= 64:
                        out.append(Deep(BM, NT, role, True, False, False, False))      # (wider blocks leave no room)
        out.append(Deep(64, NT, 2, True, False, True, False))                          # pooled input: resident at 64 ...
        out.append(Deep(128, NT, 2, False, False, True, False))                        # ... streamed at 128
        out.append(Deep(32, NT, 1, False, False, False, True))                         # tail of the sub-batch split
    return out


DEEP_CLASSES = _deep_classes()
THIN_CLASSES = ([Thin(K, M, "leaky") for K in (8, 16, 32) for M in (16, 32, 64) if not (K == 32 and M == 64)] +
                [Thin(K, M, "ring") for K in (8, 16, 32) for M in (16, 32)] + [Thin(K, 64, "pipelined") for K in (8, 16)])
WGRAD_CLASSES = ([Wgrad(K, M, False, False) for K in (8, 16, 32, 64) for M in (16, 32, 64)] +
                 [Wgrad(K, 16, True, False) for K in (8, 16, 32, 64)] +
                 [Wgrad(32, 32, False, True), WgradDeep(False), WgradDeep(True)])


# ------------------------------------------------------------------------------------------------ the table
INV95 = 1.0 / 0.95


def _concat_of(cin):
    return {64: 32, 128: 64, 192: 64, 256: 128}.get(cin)      # parts that are multiples of the deep kernel's 32-channel chunk


def _split_of(cout):
    return {16: 8, 32: 16, 64: 32, 128: 64, 192: 64, 256: 128}.get(cout)   # both parts multiples of a lane's run of channels


def conv_variants(cin, cout, H, W, tag, concat=True):
    """Every epilogue form of one channel pair at one shape: forward with / without bias and dropout, forward without
    activation, the four backward forms, a split output with a different kind per half on a concatenated input, scale != 1,
    and the LeakyReLU forms."""
    k = dict(cin=cin, cout=cout, H=H, W=W)
    n = "%d-%d_%dx%d_%s" % (cin, cout, H, W, tag)
    c1 = _concat_of(cin) if concat else None
    o1 = _split_of(cout)
    v = [_case(name=n + "fwd_bias", bias=True, relu=True, **k),
         _case(name=n + "fwd_drop", relu=True, drop_p=0.05, **k),
         _case(name=n + "fwd_bias_drop_cat", bias=True, relu=True, drop_p=0.05, c1=c1, **k),
         _case(name=n + "lin_bias", bias=True, **k),
         _case(name=n + "bwd_plain", transposed=True, **k),
         _case(name=n + "bwd_src", src=(True, False), scale=(INV95, 1.0), transposed=True, **k),
         _case(name=n + "bwd_acc", acc=(True, False), transposed=True, c1=c1, **k),
         _case(name=n + "bwd_src_acc", src=(True, False), acc=(True, False), scale=(0.75, 1.0), transposed=True, **k),
         _case(name=n + "lk_fwd_bias_drop", bias=True, relu=True, slope=0.1, drop_p=0.05, **k),
         _case(name=n + "lk_bwd_src_acc", src=(True, False), acc=(True, False), scale=(INV95, 1.0), slope=0.1, transposed=True, **k)]
    if o1 is not None:
        v.append(_case(name=n + "bwd_split_acc_src", o1=o1, acc=(True, False), src=(False, True), scale=(1.0, 1.25),
                       transposed=True, c1=c1, **k))
        v.append(_case(name=n + "lk_bwd_split_src_src", o1=o1, src=(True, True), scale=(1.25, INV95), slope=0.1,
                       transposed=True, **k))
    return v


# channel pairs of the deep kernel -> what they reach: 64-wide blocks resident (64 -> 64, 32 -> 64) and streamed (256 -> 64);
# 32-wide resident (64 -> 32, 128 -> 32), streamed (256 -> 32) and 192 -> 32, which is resident at W <= 48 only; 128-wide with one
# group, a half-empty second group (64 -> 192) and two groups; 16-wide (128 -> 16) and 8 of 16 channels (64 -> 8)
DEEP_PAIRS = [(64, 64), (32, 64), (64, 32), (128, 32), (192, 32), (256, 32), (256, 64), (128, 128), (64, 192), (256, 256),
              (128, 16), (64, 8)]


def _deep_cases():
    out = []
    for cin, cout in DEEP_PAIRS:
        th = deep_th(conv_cm(cin, cout))
        out += conv_variants(cin, cout, th + 1, 47, "nt3_")          # ragged H and W: one tile row + 1 row, 47 of 48 pixels
        out += conv_variants(cin, cout, th + 1, 81, "nt5_")          # ... 80 + 1 pixels
    # 32-channel blocks: a lane's run is 8 channels, so an 8+24 split is served (REFUSED_CASES has the 64-channel counterpart)
    for W, tag in ((47, "nt3_"), (81, "nt5_")):
        out.append(_case(name="64-32_9x%d_%sbwd_split_8+24" % (W, tag), cin=64, cout=32, H=9, W=W, o1=8, acc=(True, False),
                         src=(False, True), scale=(1.0, 1.25), transposed=True))
    # the other edges of the tile grid, forward (role 1) and ReLU-source backward (role 2)
    for cin, cout in [(64, 64), (128, 128), (192, 32), (64, 8)]:
        th = deep_th(conv_cm(cin, cout))
        for H, W in [(1, 1), (th - 1, 48), (1, 49), (th - 1, 50), (th + 1, 95)]:
            k = dict(cin=cin, cout=cout, H=H, W=W)
            n = "%d-%d_%dx%d_edge_" % (cin, cout, H, W)
            out.append(_case(name=n + "fwd_bias_drop", bias=True, relu=True, drop_p=0.05, **k))
            out.append(_case(name=n + "bwd_src", src=(True, False), scale=(INV95, 1.0), transposed=True, **k))
    # pooled input (POOLG) at odd H and W: the last row and column have no window
    for C, shapes in [(64, [(17, 35), (9, 51)]), (128, [(17, 35), (9, 51)])]:
        for H, W in shapes:
            k = dict(cin=C, cout=C, H=H, W=W, pooled=True, transposed=True)
            n = "%d-%d_%dx%d_poolg_" % (C, C, H, W)
            out.append(_case(name=n + "src", src=(True, False), pool_scale=INV95, **k))
            out.append(_case(name=n + "acc", acc=(True, False), **k))
    # the sub-batch split (SUBW tail): exactly two rounds of tiles
    for cin, cout, B, H, W in [(64, 64, 50, 17, 81), (128, 128, 100, 9, 33)]:
        out.append(_case(name="%d-%d_%dx%dx%d_subw_fwd_bias_drop" % (cin, cout, B, H, W), cin=cin, cout=cout, B=B, H=H, W=W,
                         bias=True, relu=True, drop_p=0.05))
    return out


THIN_ROWS = [(8, 32), (8, 64), (16, 64), (32, 8), (8, 128), (8, 16), (16, 16), (16, 32), (32, 32)]   # (the last four: ring controls)
THIN_LEAKY_ROWS = [(8, 16), (8, 32), (8, 64), (16, 16), (16, 32), (16, 64), (32, 8), (32, 32)]      # every thin (CK, CM)


def _thin_cases():
    out = []
    for cin, cout in THIN_ROWS:
        for H, W in [(17, 33), (9, 31)]:
            k = dict(cin=cin, cout=cout, H=H, W=W)
            n = "%d-%d_%dx%d_thin_" % (cin, cout, H, W)
            out += [_case(name=n + "fwd_bias_drop", bias=True, relu=True, drop_p=0.05, **k),
                    _case(name=n + "fwd_plain", relu=True, **k),
                    _case(name=n + "bwd_src", src=(True, False), scale=(INV95, 1.0), transposed=True, **k),
                    _case(name=n + "bwd_src_acc", src=(True, False), acc=(True, False), scale=(0.75, 1.0), transposed=True, **k)]
    for cin, cout in THIN_LEAKY_ROWS:
        k = dict(cin=cin, cout=cout, H=17, W=33, slope=0.1)
        n = "%d-%d_17x33_thin_lk_" % (cin, cout)
        out += [_case(name=n + "fwd_bias_drop", bias=True, relu=True, drop_p=0.05, **k),
                _case(name=n + "bwd_src_acc", src=(True, False), acc=(True, False), scale=(INV95, 1.0), transposed=True, **k)]
    return out


def _wgrad_cases():
    out = []
    rows = [(8, 8), (8, 16), (8, 32), (8, 64), (16, 8), (16, 16), (16, 32), (16, 64), (32, 8), (32, 16), (32, 32), (32, 64),
            (64, 8), (64, 16), (128, 32)]
    for cin, cout in rows:
        out.append(_case(kind="wgrad", name="wg_%d-%d_9x33" % (cin, cout), cin=cin, cout=cout, H=9, W=33))
    out.append(_case(kind="wgrad", name="wg_32+32-64_9x33", cin=64, cout=64, c1=32, H=9, W=33))            # not deep: c1 % 64 != 0
    for W in (49, 81):
        out.append(_case(kind="wgrad", name="wg_64+64-64_5x%d" % W, cin=128, cout=64, c1=64, B=3, H=5, W=W))
        out.append(_case(kind="wgrad", name="wg_128-128_5x%d" % W, cin=128, cout=128, B=3, H=5, W=W))
    for C, H, W in [(32, 17, 35), (64, 17, 35), (128, 9, 51)]:
        out.append(_case(kind="wgrad", name="wg_%d-%d_%dx%d_pooled" % (C, C, H, W), cin=C, cout=C, H=H, W=W, pooled=True,
                         pool_scale=INV95))
    return out


CONV_CASES = _deep_cases() + _thin_cases()
WGRAD_CASES = _wgrad_cases()
# refusals (dispatch_conv, launch_conv_ring_epi, dispatch_conv_deep_plain, dispatch_wgrad): the text is instance_of's.  A split
# output of the deep kernel inside a lane's run of 16 channels used to be launched: the run went whole to the first half, over
# the next pixel's channels and 16 bytes past the end of the tensor
REFUSED_CASES = [
    _case(name="refuse_poolg_16-16", cin=16, cout=16, H=16, W=32, pooled=True, src=(True, False), transposed=True),
    _case(name="refuse_poolg_leaky", cin=64, cout=64, H=16, W=32, pooled=True, src=(True, False), slope=0.1, transposed=True),
    _case(name="refuse_poolg_forward_role", cin=64, cout=64, H=16, W=32, pooled=True, relu=True),
    _case(name="refuse_poolg_64-32", cin=64, cout=32, H=16, W=32, pooled=True, src=(True, False), transposed=True),
    _case(name="refuse_poolg_128-64_streamed", cin=128, cout=64, H=16, W=32, pooled=True, src=(True, False), transposed=True),
    _case(name="refuse_split_8+56_inside_a_lane_run", cin=64, cout=64, H=9, W=33, o1=8, src=(True, True), transposed=True),
    _case(name="refuse_split_72+56_inside_a_lane_run", cin=64, cout=128, H=5, W=49, o1=72, acc=(True, False), transposed=True),
    _case(kind="wgrad", name="refuse_wg_pooled_8-16", cin=8, cout=16, H=16, W=32, pooled=True),
]
ALL_CASES = CONV_CASES + WGRAD_CASES


# ------------------------------------------------------------------------------------------------ operands
def _gen(c, salt):
    key = ((((c.cin * 257 + c.cout) * 101 + c.B) * 211 + c.H) * 307 + c.W) * 2 + int(c.pooled)
    return torch.Generator().manual_seed(key * 16 + salt)


def _signed_zeros(t, gen):
    """Sprinkle +0.0 and -0.0 over a bf16 tensor (about a tenth each)."""
    r = torch.rand(t.shape, generator=gen)
    t = torch.where(r < 0.1, torch.zeros_like(t), t)
    return torch.where((r >= 0.1) & (r < 0.2), torch.full_like(t, -0.0), t)


def pre_pool(c, C):
    """The tensor whose pooling gives the arg-max codes of a pooled case: values on a coarse grid (ties), channels whose maxima
    are never positive and strictly negative ones (as tests/test_gpu_pool_adjoint_fused.py::_operands)."""
    pre = (torch.randn(c.B, c.H, c.W, C, generator=_gen(c, 7)) * 1.5).round() * 0.5
    pre[:, :, :, 0::5] = pre[:, :, :, 0::5].clamp_max(0)
    pre[:, :, :, 3::7] = -pre[:, :, :, 3::7].abs() - 0.5
    return pre.to(BF16)


@functools.lru_cache(maxsize=6)
def shared_operands(cin, cout, B, H, W, pooled, kind):
    """What every epilogue form of one (channel pair, shape) shares: the input, the master weights of both packings and the fp64
    sums of the plain and the transposed-packed operator -- computed once, never modified."""
    c = _case(cin=cin, cout=cout, B=B, H=H, W=W, pooled=pooled, kind=kind)
    g = _gen(c, 1)
    o = {}
    if kind == "wgrad":
        o["x"] = (torch.randn(B, H, W, cin, generator=g) * 0.7).clamp_min(0).to(BF16)
        if pooled:
            o["g"] = (torch.randn(B, H // 2, W // 2, cout, generator=g) * 0.3).to(BF16)
            o["arg"] = cr.pack_codes(cr.pool_codes(pre_pool(c, cout))[1])
        else:
            o["g"] = (torch.randn(B, H, W, cout, generator=g) * 0.5).to(BF16)
        return o
    if pooled:
        o["x"] = (torch.randn(B, H // 2, W // 2, cin, generator=g) * 0.5).to(BF16)
        o["arg"] = cr.pack_codes(cr.pool_codes(pre_pool(c, cin))[1])
    else:
        o["x"] = torch.randn(B, H, W, cin, generator=g).to(BF16)
    o["w"] = torch.randn(cout, cin, 3, 3, generator=g) / (9 * cin) ** 0.5           # forward packing: (COUT,CIN,3,3)
    o["wt"] = torch.randn(cin, cout, 3, 3, generator=g) / (9 * cin) ** 0.5          # transposed packing: master weights (CIN,COUT,3,3)
    o["bias"] = torch.randn(cout, generator=g)
    o["src"] = _signed_zeros(torch.randn(B, H, W, cout, generator=g).to(BF16), g)
    o["base"] = (torch.randn(B, H, W, cout, generator=g) * 0.5).to(BF16)
    o["core"] = {}
    return o


def shared(c):
    return shared_operands(c.cin, c.cout, c.B, c.H, c.W, c.pooled, c.kind)


def conv_core_of(c, device="cpu"):
    """conv_core of the case's operands (cached per (pair, shape, packing, pool scale); on `device`, result kept there)."""
    o = shared(c)
    key = (c.transposed, c.pool_scale if c.pooled else None, str(device))
    if key not in o["core"]:
        x = o["x"].to(device)
        if c.pooled:
            x = cr.pool_adjoint(x, o["arg"].to(device), c.H, c.W, c.pool_scale)
        w = cr.op_weights(o["wt"] if c.transposed else o["w"], c.transposed).to(device)
        o["core"][key] = cr.conv_core(x.to(torch.float64), w)
    return o["core"][key]


SEED = 0x5EED


def conv_ref_of(c, device="cpu", **override):
    """conv_ref of a case (the shared fp64 sums reused).  Returns (ConvRef, kwargs used)."""
    o = shared(c)
    o1 = c.cout if c.o1 is None else c.o1
    kw = dict(bias=o["bias"] if c.bias else None, relu=c.relu, slope=c.slope, drop_p=c.drop_p, seed=SEED, O1=o1,
              relu_src=tuple(o["src"][..., lo:hi].to(device) if s else None for s, (lo, hi) in zip(c.src, ((0, o1), (o1, c.cout)))),
              scale=c.scale,
              base=tuple(o["base"][..., lo:hi].to(device) if a else None for a, (lo, hi) in zip(c.acc, ((0, o1), (o1, c.cout)))),
              transposed=c.transposed)
    kw.update(override)
    core = kw.pop("core", None)
    if core is None:
        core = conv_core_of(c, device)
    x = o["x"].to(device)
    if c.pooled:
        kw.update(x1_pool_arg=o["arg"].to(device), x1_pool_scale=c.pool_scale, hw=(c.H, c.W))
    return cr.conv_ref(x, o["wt"] if c.transposed else o["w"], core=core, **kw), kw
