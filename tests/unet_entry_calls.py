"""Seeded calls of the U-Net entries through the C ABI, shared by tests/test_gpu_unet_entry_paths.py and its child process.

``python tests/unet_entry_calls.py first-calls`` is that child: a fresh process whose FIRST uses of the weight-gradient, convolution
and fused-backward kernels are the pooled-gradient (and resident-weight) instantiations, each then compared with the plain
composite (mmk_maxpool2_bwd_arg + the plain entry) computed afterwards.  A kernel instantiation that needs more than 64 KB of
LDS has to raise its own limit before its first launch; an ordered suite hides a missing one behind an earlier plain call."""
import ctypes
import sys

import torch

from mm_masking_amd import _lib

DEV = torch.device("cuda:0")
NULL = ctypes.c_void_p(0)
BF16 = torch.bfloat16
ENC = [8, 16, 32, 64, 128, 256]
P = _lib.ptr


def conv_shapes(cin):
    """(cout, cin) of conv k = 0..22 (csrc/mmk_unet_driver.hip: make_plan)."""
    s = []
    for i in range(6):
        s += [(ENC[i], cin if i == 0 else ENC[i - 1]), (ENC[i], ENC[i])]
    for j in range(5):
        s += [(ENC[4 - j], 2 * ENC[4 - j]), (ENC[4 - j], ENC[4 - j])]
    return s + [(1, 8)]


class Net:
    """One seeded network input and parameter set, run through mmk_unet_forward and the three backward entries."""

    def __init__(self, B, cin, H, W, slope, drop, norm, seed=3):
        g = torch.Generator().manual_seed(seed)
        self.B, self.cin, self.H, self.W, self.slope, self.drop, self.norm = B, cin, H, W, slope, drop, norm
        self.x = torch.rand(B, cin, H, W, generator=g).to(DEV)
        self.gmask = torch.randn(B, H, W, generator=g).to(DEV)
        self.params = []
        for k, (co, ci) in enumerate(conv_shapes(cin)):
            ks = 1 if k == 22 else 3
            self.params += [(torch.randn(co, ci, ks, ks, generator=g) * (2.0 / (ks * ks * ci)) ** 0.5).to(DEV),
                            (torch.randn(co, generator=g) * 0.05).to(DEV)]
        L = _lib.lib()
        self.ws_bytes = int(L.mmk_unet_workspace_bytes(B, H, W, cin))
        self.scratch_bytes = int(L.mmk_unet_scratch_bytes(B, H, W, cin))
        assert self.ws_bytes > 0 and self.scratch_bytes > 0, L.mmk_last_error()
        self.mask = torch.empty(B, H, W, dtype=torch.float32, device=DEV)

    def desc(self, ws, ws_bytes=None):
        self._pp = (ctypes.c_void_p * 46)(*[t.data_ptr() for t in self.params])
        return _lib.UNetDesc(B=self.B, H=self.H, W=self.W, cin=self.cin, x=self.x.data_ptr(), pre=None, params=self._pp,
                             drop_p=self.drop, seed=11, leaky_slope=self.slope, norm=self.norm, workspace=ws.data_ptr(),
                             workspace_bytes=self.ws_bytes if ws_bytes is None else ws_bytes, mask=self.mask.data_ptr(), keep_full_res=0)

    def forward(self, ws):
        d = self.desc(ws)
        _lib.check(_lib.lib().mmk_unet_forward(ctypes.byref(d), _lib.stream_ptr(DEV)))
        torch.cuda.synchronize()
        return self.mask.clone()

    def backward(self, entry, ws, scratch, events=None):
        """-> (46 parameter gradients, grad_x or None); entry: "", "_buckets" or "_input" (normalisation mode none)."""
        L, d = _lib.lib(), self.desc(ws)
        grads = [torch.zeros_like(p) for p in self.params]
        gp = (ctypes.c_void_p * 46)(*[t.data_ptr() for t in grads])
        ep = None if events is None else (ctypes.c_void_p * len(events))(*[int(e.cuda_event) for e in events])
        st, gx = _lib.stream_ptr(DEV), None
        if entry == "_input":
            gx = torch.empty_like(self.x)
            _lib.check(L.mmk_unet_backward_input(ctypes.byref(d), P(self.gmask), gp, P(gx), 0, NULL, P(scratch), self.scratch_bytes, ep, st))
        elif entry == "_buckets":
            _lib.check(L.mmk_unet_backward_buckets(ctypes.byref(d), P(self.gmask), gp, P(scratch), self.scratch_bytes, ep, st))
        else:
            _lib.check(L.mmk_unet_backward(ctypes.byref(d), P(self.gmask), gp, P(scratch), self.scratch_bytes, st))
        torch.cuda.synchronize()
        return grads, gx


# ----------------------------------------------------------------------------- the child: pooled variants as a process's first calls
def _bf16(g, *shape, scale=1.0):
    return (torch.randn(*shape, generator=g) * scale).to(BF16).to(DEV)


def _codes(g, B, h, w, C):
    """Arg-max codes as a pooling writes them, one nibble per channel: 4 | position for a positive maximum, else 0
    (include/mmk.h: pool_arg)."""
    n = torch.randint(0, 5, (B, h, w, C // 2, 2), generator=g, dtype=torch.int32)
    n = torch.where(n > 0, n + 3, n)
    return (n[..., 0] | (n[..., 1] << 4)).to(torch.uint8).to(DEV)


def _ok(rc, what):
    if rc != 0:
        raise SystemExit("%s returned %d: %s" % (what, rc, _lib.lib().mmk_last_error().decode()))


def _slice_floats(cout, cin):
    return 9 * cout * cin + cout


def _tiles(B, H, W):
    return B * ((H + 7) // 8) * ((W + 31) // 32)        # the slice count of every weight-gradient kernel is at most this


S = 1.25        # the pooling adjoint's factor (dropout's 1 / keep)


def _unpooled(arg, gy, B, H, W, C):
    L, gz = _lib.lib(), torch.empty(B, H, W, C, dtype=BF16, device=DEV)
    _ok(L.mmk_maxpool2_bwd_arg(P(arg), P(gy), B, H, W, C, S, P(gz), _lib.stream_ptr(DEV)), "mmk_maxpool2_bwd_arg")
    return gz


def _pooled_operands(g, B, H, W, C):
    return _bf16(g, B, H // 2, W // 2, C), _codes(g, B, H // 2, W // 2, C)


# Each case makes its pooled call at once and returns (name, results, function that computes the plain composite later).
def _wgrad_case(g, C, B, H, W):
    L, st = _lib.lib(), _lib.stream_ptr(DEV)
    x, (gy, arg) = _bf16(g, B, H, W, C), _pooled_operands(g, B, H, W, C)
    part = torch.zeros(_tiles(B, H, W), _slice_floats(C, C), device=DEV)
    _ok(L.mmk_conv3x3_wgrad_partial_pooled(P(x), NULL, C, 0, P(gy), P(arg), S, C, B, H, W, P(part), 0, st),
        "mmk_conv3x3_wgrad_partial_pooled %d" % C)

    def plain():
        ref = torch.zeros_like(part)
        _ok(L.mmk_conv3x3_wgrad_partial(P(x), NULL, C, 0, P(_unpooled(arg, gy, B, H, W, C)), C, B, H, W, P(ref), 0, st),
            "mmk_conv3x3_wgrad_partial %d" % C)
        return [ref]
    return "wgrad_pooled_%d" % C, [part], plain


def _conv_case(g, C, B, H, W):
    L, st = _lib.lib(), _lib.stream_ptr(DEV)
    (gy, arg), src = _pooled_operands(g, B, H, W, C), _bf16(g, B, H, W, C)
    wpack = _bf16(g, int(L.mmk_conv3x3_packed_elems(C, C, 1)), scale=0.05)      # (any bit pattern is a packed weight set)

    def conv(x1, pooled_arg):       # the data gradient as the driver asks for it: ReLU source, no bias, no activation
        y = torch.empty(B, H, W, C, dtype=BF16, device=DEV)
        d = _lib.ConvDesc(x1=P(x1), C1=C, wpack=P(wpack), y1=P(y), relu_src1=P(src), O1=C, scale1=1.0, scale2=1.0, B=B, H=H, W=W,
                          x1_pool_arg=None if pooled_arg is None else P(pooled_arg), x1_pool_scale=1.0 if pooled_arg is None else S)
        _ok(L.mmk_conv3x3(ctypes.byref(d), st), "mmk_conv3x3 %d%s" % (C, "" if pooled_arg is None else " with x1_pool_arg"))
        return y
    return "conv_pooled_%d" % C, [conv(gy, arg)], lambda: [conv(_unpooled(arg, gy, B, H, W, C), None)]


def _fused_case(g, C, B, H, W):
    L, st = _lib.lib(), _lib.stream_ptr(DEV)
    x, (gy, arg) = _bf16(g, B, H, W, C), _pooled_operands(g, B, H, W, C)
    wpack = _bf16(g, int(L.mmk_conv3x3_packed_elems(C, C, 1)), scale=0.05)
    dx, part = torch.empty_like(x), torch.zeros(_tiles(B, H, W), _slice_floats(C, C), device=DEV)
    _ok(L.mmk_conv_bwd_fused_pooled(P(x), P(gy), P(arg), S, P(wpack), 1.0, B, H, W, C, P(dx), P(part), 0, st), "mmk_conv_bwd_fused_pooled")

    def plain():
        rdx, ref = torch.empty_like(x), torch.zeros_like(part)
        _ok(L.mmk_conv_bwd_fused(P(x), P(_unpooled(arg, gy, B, H, W, C)), P(wpack), 1.0, B, H, W, C, P(rdx), P(ref), 0, st),
            "mmk_conv_bwd_fused")
        return [rdx, ref]
    return "bwd_fused_pooled", [dx, part], plain


def first_calls():
    g = torch.Generator().manual_seed(29)
    cases = [_wgrad_case(g, 32, 2, 18, 70), _wgrad_case(g, 64, 2, 20, 44),
             _conv_case(g, 32, 2, 18, 70), _conv_case(g, 64, 2, 20, 44), _conv_case(g, 128, 1, 12, 40),
             _fused_case(g, 16, 2, 18, 70)]
    torch.cuda.synchronize()
    out = {}
    for name, got, plain in cases:
        want = plain()
        torch.cuda.synchronize()
        for i, (a, b) in enumerate(zip(got, want)):
            if a.shape != b.shape or not torch.equal(a, b):
                raise SystemExit("%s[%d]: the pooled entry and the plain composite differ" % (name, i))
            if not bool(a.float().abs().sum() > 0):
                raise SystemExit("%s[%d]: all zero" % (name, i))
            out["%s.%d" % (name, i)] = a
    return out, len(out)


if __name__ == "__main__":
    assert sys.argv[1:2] == ["first-calls"], sys.argv
    tensors, count = first_calls()
    if len(sys.argv) > 2:
        torch.save({k: v.cpu() for k, v in tensors.items()}, sys.argv[2])
    print("first-calls ok %d" % count)
