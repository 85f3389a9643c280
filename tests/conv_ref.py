"""fp64 restatement of the 3x3 convolution entry points (include/mmk.h: mmk_conv_desc, mmk_conv3x3_wgrad_partial[_pooled],
mmk_maxpool2_bwd, mmk_upsample_bwd) and the one error bound the GPU tests hold every kernel instance to.  torch only, any
device, no import of the package: operands are bf16-VALUED tensors (any float dtype), every product and sum is fp64.

Each reference returns, next to the value, the magnitude sum S = sum |x w| (+ |bias|, + |base|, times the same epilogue
factors) of every output element: the quantity a forward error bound of a floating-point sum is proportional to.

The bound (within): a bf16 output is ONE rounding of an fp32 value that was accumulated in fp32 in an order we do not know, so
    |got - ref| <= 2^-8 |ref| + (n_terms + C_EPI) 2^-24 S + 2^-133
  * 2^-8 |ref|: bf16 keeps 8 significant bits (7 stored), so its ulp is 2^-7 of the lower end of a binade and round-to-nearest
    is off by at most half of that: the unit roundoff of the format is 2^-8 (2^-9 would be a 9-bit significand: the fp32
    emulation of tests/test_conv_ref_cpu.py leaves it by up to 1.8x on thousands of elements of any case);
  * n_terms 2^-24 S: n_terms - 1 fp32 additions of exact products (bf16 x bf16 has 16 significant bits), any order, first order
    in the unit roundoff 2^-24 (Higham, Accuracy and Stability, eq. 4.4: gamma_n ~ n u); n_terms = 9 CIN;
  * C_EPI = 6: every fp32 rounding an epilogue can apply to one value, read off the generic epilogues (csrc/mmk_unet.hip,
    conv3x3_kernel and conv3x3_deep_kernel ROLE 0, which apply all of them when a descriptor asks for all):
      acc + bias, v * slope (act_leaky), v * keep factor, scale * slope (bwd_factor_leaky), v * factor, v + base.
    The specialised epilogues round less often: role 1 / the ring kernel fold the keep factor into the bias (bias * keep, then
    one fma: 2), role 2 has one of v * scale or v + base (1).  Each rounding is at most 2^-24 of an intermediate no larger
    than S;
  * 2^-133: the smallest bf16 subnormal (a result below it may be flushed).
fp32 sums (weight gradients): |got - ref| <= (B H W + slices) 2^-24 S: B H W products per element, summed per slice and then
over the slices.  No constant here comes from an error observed on a GPU."""
import collections

import numpy as np
import torch

import dropout_ref as dr

F64 = torch.float64
BF16 = torch.bfloat16
C_EPI = 6
U32 = 2.0 ** -24
U16 = 2.0 ** -8
TINY = 2.0 ** -133


def bf16v(t):
    """Round to bf16 values, held in fp64."""
    return t.to(BF16).to(F64)


def f32(v):
    return float(np.float32(v))


def op_weights(w, transposed=False):
    """The operator's weights (OUT,IN,3,3) in fp64, bf16-rounded, from fp32 master weights: as they are, or (transposed: the
    data-gradient operator of mmk_conv3x3_pack_weights) OUT/IN swapped with the taps flipped."""
    w = bf16v(w)
    return w.permute(1, 0, 2, 3).flip(2, 3).contiguous() if transposed else w


# ---------------------------------------------------------------------------------------------- pooling codes
def pool_codes(x):
    """2x2 / stride 2 max pooling of (B,H,W,C) (floor sizes): (pool_y, nibble codes (B,H/2,W/2,C) int64) with
    code = position 0..3 of the window's FIRST maximum in scan order | (maximum > 0) << 2 (mmk.h: pool_arg)."""
    B, H, W, C = x.shape
    Ho, Wo = H // 2, W // 2
    x = x.to(F64)
    win = torch.stack([x[:, 0:2 * Ho:2, 0:2 * Wo:2], x[:, 0:2 * Ho:2, 1:2 * Wo:2],
                       x[:, 1:2 * Ho:2, 0:2 * Wo:2], x[:, 1:2 * Ho:2, 1:2 * Wo:2]], dim=0)
    m = win[0].clone()
    a = torch.zeros_like(m, dtype=torch.int64)
    for k in range(1, 4):
        gt = win[k] > m
        m = torch.where(gt, win[k], m)
        a = torch.where(gt, torch.full_like(a, k), a)
    return m, a | ((m > 0).to(torch.int64) << 2)


def pack_codes(nib):
    """(B,h,w,C) nibbles -> (B,h,w,C/2) uint8: channel c in bits 4 (c & 1) of byte c / 2."""
    return (nib[..., 0::2] | (nib[..., 1::2] << 4)).to(torch.uint8)


def unpack_codes(arg):
    a = arg.to(torch.int64)
    return torch.stack([a & 15, a >> 4], dim=-1).reshape(*arg.shape[:-1], arg.shape[-1] * 2)


def pool_adjoint(gy, arg, H, W, scale):
    """What mmk_maxpool2_bwd_arg(arg, gy, B, H, W, C, scale) writes, bit for bit, as bf16 values in fp64: the pooled value times
    scale (ONE fp32 product, rounded to bf16: maxpool2_bwd_arg_kernel) at the coded position of windows whose maximum was
    positive, zero elsewhere and in the last row / column of odd sizes."""
    B, Ho, Wo, C = gy.shape
    nib = unpack_codes(arg)
    gv = (gy.to(torch.float32) * torch.tensor(np.float32(scale), device=gy.device)).to(BF16).to(F64)
    gv = torch.where((nib & 4) != 0, gv, torch.zeros_like(gv))
    out = torch.zeros(B, H, W, C, dtype=F64, device=gy.device)
    for k in range(4):
        out[:, (k >> 1):2 * Ho:2, (k & 1):2 * Wo:2] = torch.where((nib & 3) == k, gv, torch.zeros_like(gv))
    return out


# ---------------------------------------------------------------------------------------------- convolution
def conv_core(x, w):
    """(sum, sum of magnitudes) of the 3x3 / pad 1 correlation: x (B,H,W,CIN), w (COUT,CIN,3,3), both fp64 -> (B,H,W,COUT)."""
    B, H, W, _ = x.shape
    xp = torch.zeros(B, H + 2, W + 2, x.shape[3], dtype=F64, device=x.device)
    xp[:, 1:H + 1, 1:W + 1] = x
    xa, wa = xp.abs(), w.abs()
    val = torch.zeros(B, H, W, w.shape[0], dtype=F64, device=x.device)
    mag = torch.zeros_like(val)
    for ky in range(3):
        for kx in range(3):
            val += xp[:, ky:ky + H, kx:kx + W] @ w[:, :, ky, kx].t()
            mag += xa[:, ky:ky + H, kx:kx + W] @ wa[:, :, ky, kx].t()
    return val, mag


def bwd_factor(src, scale, slope):
    """The relu_src factor of mmk_conv_desc: slope = 0: src > 0 ? scale : 0; slope > 0: src > 0 ? scale : (src < 0 or src is
    -0.0) ? slope scale : 0."""
    src = src.to(F64)
    s = torch.full_like(src, f32(scale))
    z = torch.zeros_like(src)
    if slope > 0:
        return torch.where(src > 0, s, torch.where((src < 0) | ((src == 0) & torch.signbit(src)), s * f32(slope), z))
    return torch.where(src > 0, s, z)


ConvRef = collections.namedtuple("ConvRef", "y S keep pool_y pool_arg")


def conv_ref(x1, w, x2=None, bias=None, relu=False, slope=0.0, drop_p=0.0, seed=0, base_index=0, O1=None,
             relu_src=(None, None), scale=(1.0, 1.0), base=(None, None), x1_pool_arg=None, x1_pool_scale=1.0, hw=None,
             transposed=False, pool=False, core=None):
    """mmk_conv_desc in fp64.  x1 / x2 / relu_src / base: bf16-valued (B,H,W,C); w: fp32 master weights (see op_weights); bias:
    fp32 (COUT) or None; base[i] set = accumulate_i with that target; the output halves [0,O1) and [O1,COUT) come back as ONE
    (B,H,W,COUT) tensor (split it at O1).  x1_pool_arg (with hw): x1 is pooled and the input is pool_adjoint(...).  core: a
    precomputed conv_core() of the same operands.  Order of the epilogue, as in every kernel: bias, activation, dropout, ReLU
    source factor, accumulate.  keep: the dropout's keep mask (None without dropout)."""
    if x1_pool_arg is not None:
        x1 = pool_adjoint(x1, x1_pool_arg, hw[0], hw[1], x1_pool_scale)
    x = x1.to(F64) if x2 is None else torch.cat([x1.to(F64), x2.to(F64)], dim=3)
    wo = op_weights(w, transposed).to(x.device)
    y, S = conv_core(x, wo) if core is None else (core[0].clone(), core[1].clone())
    B, H, W, COUT = y.shape
    if bias is not None:
        b = bias.to(F64).to(y.device)
        y, S = y + b, S + b.abs()
    if relu:
        if slope > 0:
            y = torch.maximum(y, y * f32(slope))
            y = torch.where(y == 0, torch.full_like(y, -0.0), y)         # a kept zero is -0.0
        else:
            y = y.clamp_min(0.0)
    keep = None
    if dr.params(drop_p).thr != 0:
        keep = torch.from_numpy(dr.keep_mask(seed, (B, H, W, COUT), drop_p, base_index)).to(y.device)
        k = float(dr.params(drop_p).inv_keep)
        y = torch.where(keep, y * k, torch.zeros_like(y))                 # a dropped element is +0.0
        S = torch.where(keep, S * k, torch.zeros_like(S))
    O1 = COUT if O1 is None else O1
    parts_y, parts_S = [], []
    for i, (lo, hi) in enumerate(((0, O1), (O1, COUT))):
        if hi == lo:
            continue
        yi, Si = y[..., lo:hi], S[..., lo:hi]
        if relu_src[i] is not None:
            f = bwd_factor(relu_src[i].to(y.device), scale[i], slope)
            yi, Si = yi * f, Si * f.abs()
        if base[i] is not None:
            bs = base[i].to(F64).to(y.device)
            yi, Si = yi + bs, Si + bs.abs()
        parts_y.append(yi)
        parts_S.append(Si)
    y, S = torch.cat(parts_y, dim=3), torch.cat(parts_S, dim=3)
    py = pa = None
    if pool:
        py, pa = pool_codes(y[..., :O1])
    return ConvRef(y, S, keep, py, pa)


WgradRef = collections.namedtuple("WgradRef", "dW db SW Sb")


def wgrad_ref(x1, x2, g, g_pool_arg=None, g_pool_scale=1.0, hw=None):
    """dW[co][ci][ky][kx] = sum over (b, y, x) of g[b,y,x,co] * x_pad[b,y+ky,x+kx,ci] (autograd of the pad-1 correlation), db[co]
    = sum g, with their magnitude sums.  g_pool_arg (with hw): g is pooled and routed as pool_adjoint()."""
    if g_pool_arg is not None:
        g = pool_adjoint(g, g_pool_arg, hw[0], hw[1], g_pool_scale)
    x = x1.to(F64) if x2 is None else torch.cat([x1.to(F64), x2.to(F64)], dim=3)
    g = g.to(F64)
    B, H, W, CIN = x.shape
    COUT = g.shape[3]
    xp = torch.zeros(B, H + 2, W + 2, CIN, dtype=F64, device=x.device)
    xp[:, 1:H + 1, 1:W + 1] = x
    g2, ga = g.reshape(-1, COUT), g.abs().reshape(-1, COUT)
    dW = torch.zeros(COUT, CIN, 3, 3, dtype=F64, device=x.device)
    SW = torch.zeros_like(dW)
    for ky in range(3):
        for kx in range(3):
            xs = xp[:, ky:ky + H, kx:kx + W].reshape(-1, CIN)
            dW[:, :, ky, kx] = g2.t() @ xs
            SW[:, :, ky, kx] = ga.t() @ xs.abs()
    return WgradRef(dW, g2.sum(0), SW, ga.sum(0))


# ---------------------------------------------------------------------------------------------- pooling / up-sampling adjoints
def maxpool2_bwd_ref(d, gy, scale, slope=0.0):
    """mmk_maxpool2_bwd: the pooled gradient goes to the first maximal position of its window of d (scan order, strict >) times
    the bwd_factor of that maximum; everything else, and the last row / column of odd sizes, is zero.  -> (gz, S)."""
    B, H, W, C = d.shape
    Ho, Wo = H // 2, W // 2
    d = d.to(F64)
    win = [d[:, (k >> 1):2 * Ho:2, (k & 1):2 * Wo:2] for k in range(4)]
    m, a = win[0].clone(), torch.zeros(B, Ho, Wo, C, dtype=torch.int64, device=d.device)
    for k in range(1, 4):
        gt = win[k] > m
        m = torch.where(gt, win[k], m)
        a = torch.where(gt, torch.full_like(a, k), a)
    gv = gy.to(F64) * bwd_factor(m, scale, slope)
    gz = torch.zeros(B, H, W, C, dtype=F64, device=d.device)
    for k in range(4):
        gz[:, (k >> 1):2 * Ho:2, (k & 1):2 * Wo:2] = torch.where(a == k, gv, torch.zeros_like(gv))
    return gz, gz.abs()


def up_weights(n_src, n_out):
    """(n_src, n_out) fp64 matrix of the fp32 interpolation weights of align_corners=True up-sampling exactly as the kernels
    compute them (up_coord: f = r * o in fp32, i0 = trunc f, l1 = f - i0, l0 = 1 - l1; r = (n_src - 1) / (n_out - 1) in fp32)."""
    r = np.float32(n_src - 1) / np.float32(n_out - 1) if n_out > 1 else np.float32(0)
    M = np.zeros((n_src, n_out), dtype=np.float32)
    for o in range(n_out):
        f = np.float32(r * np.float32(o))
        i0 = int(f)
        i1 = i0 + (1 if i0 < n_src - 1 else 0)
        l1 = np.float32(f - np.float32(i0))
        l0 = np.float32(np.float32(1.0) - l1)
        M[i0, o] = np.float32(M[i0, o] + l0)
        M[i1, o] = np.float32(M[i1, o] + l1)
    return torch.from_numpy(M.astype(np.float64))


def upsample_bwd_ref(gy, Hs, Ws, relu_src=None, scale=1.0, slope=0.0):
    """mmk_upsample_bwd: the adjoint of the bilinear up-sampling (Hs,Ws) -> gy's (Ho,Wo), times the bwd_factor of relu_src.
    -> (gx, S, n_terms): n_terms = 2 (nx + 1) (ny + 1) for the most products any element sums (nx, ny = the most non-zero weights
    of a source column / row; two fma levels each), plus Hs + Ws for the weights themselves: f = r * o is one fp32 rounding of
    a number below n_src (or none, where the compiler contracts it into l1 = fma(r, o, -i0)), so a weight is known to 2^-24 n_src."""
    B, Ho, Wo, C = gy.shape
    Wy, Wx = up_weights(Hs, Ho).to(gy.device), up_weights(Ws, Wo).to(gy.device)
    g = gy.to(F64)
    gx = torch.einsum("sy,byxc,tx->bstc", Wy, g, Wx)
    S = torch.einsum("sy,byxc,tx->bstc", Wy, g.abs(), Wx)
    if relu_src is not None:
        f = bwd_factor(relu_src, scale, slope)
        gx, S = gx * f, S * f.abs()
    n_terms = 2 * (int((Wy != 0).sum(1).max()) + 1) * (int((Wx != 0).sum(1).max()) + 1) + Hs + Ws
    return gx, S, n_terms


# ---------------------------------------------------------------------------------------------- the bound
def bound(ref, S, n_terms, fp32_out=False):
    if fp32_out:
        return n_terms * U32 * S
    return U16 * ref.abs() + (n_terms + C_EPI) * U32 * S + TINY


def within(got, ref, S, n_terms, fp32_out=False):
    """|got - ref| / bound per element (fp64; <= 1 is inside; a non-finite got, or any error at a zero bound, is inf).
    bf16 outputs: n_terms = 9 CIN.  fp32 sums (fp32_out): n_terms = B H W + slices."""
    got = got.to(F64)
    err = (got - ref).abs()
    bnd = bound(ref, S, n_terms, fp32_out)
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bnd)
    return torch.where(torch.isfinite(got), ratio, torch.full_like(ratio, float("inf")))


def worst(got, ref, S, n_terms, fp32_out=False):
    """(largest ratio, number of elements outside the bound)."""
    r = within(got, ref, S, n_terms, fp32_out)
    return float(r.max()), int((r > 1).sum())
