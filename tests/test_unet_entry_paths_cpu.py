"""CPU: return code and full error text of the U-Net entries whose host bodies share code (mmk_unet.hip's C ABI section,
mmk_unet_driver.hip), one failing argument per check, all refused on the host before any launch.  The expected strings are
the ones the entries reported before their bodies were shared: each carries the entry's own name, and the three backward
entries of the driver share the prefix of mmk_unet_backward for everything their common body checks.

mmk_unet_scratch_bytes asks the device how many blocks of a weight-gradient kernel a CU holds, so without a GPU it reports 0
and the backward entries stop at "unsupported network input": their short-workspace and short-scratch texts are pinned in
tests/test_gpu_unet_entry_paths.py instead."""
import ctypes

import pytest

from mm_masking_amd import _lib

NULL = ctypes.c_void_p(0)
FAKE = ctypes.c_void_p(4096)          # never dereferenced: every call below fails on the host before any launch
ARG = -1                              # MMK_ERR_ARG
B, H, W, CIN = 2, 64, 64, 1


@pytest.fixture(scope="module")
def L():
    _lib.build()
    return _lib.lib()


def refused(L, rc, text):
    assert rc == ARG
    assert L.mmk_last_error() == text


def test_weight_gradient_entries(L):
    for name, pooled in ((b"mmk_conv3x3_wgrad_partial", False), (b"mmk_conv3x3_wgrad_partial_pooled", True)):
        def call(x1=FAKE, x2=NULL, C1=8, C2=0, g=FAKE, arg=FAKE, cout=8, b=1, h=8, w=8, part=FAKE):
            if pooled:
                return L.mmk_conv3x3_wgrad_partial_pooled(x1, x2, C1, C2, g, arg, 1.0, cout, b, h, w, part, 0, NULL)
            return L.mmk_conv3x3_wgrad_partial(x1, x2, C1, C2, g, cout, b, h, w, part, 0, NULL)
        refused(L, call(x1=NULL), name + b": NULL pointer")
        refused(L, call(g=NULL), name + b": NULL pointer")
        refused(L, call(part=NULL), name + b": NULL pointer")
        refused(L, call(b=0), name + b": bad shape")
        refused(L, call(C1=4), name + b": bad input split 4+0")
        refused(L, call(C2=8), name + b": bad input split 8+8")             # a second half without x2
        refused(L, call(C1=24), name + b": unsupported channel counts 24 -> 8")
        refused(L, call(cout=40), name + b": unsupported channel counts 8 -> 40")
    # what the two ask differently: the codes, and a shape the pooling can halve (the plain entry takes H = 1: it gets to
    # the next check)
    refused(L, L.mmk_conv3x3_wgrad_partial_pooled(FAKE, NULL, 8, 0, FAKE, NULL, 1.0, 8, 1, 8, 8, FAKE, 0, NULL),
            b"mmk_conv3x3_wgrad_partial_pooled: NULL pointer")
    refused(L, L.mmk_conv3x3_wgrad_partial_pooled(FAKE, NULL, 8, 0, FAKE, FAKE, 1.0, 8, 1, 1, 8, FAKE, 0, NULL),
            b"mmk_conv3x3_wgrad_partial_pooled: bad shape")
    refused(L, L.mmk_conv3x3_wgrad_partial(FAKE, NULL, 4, 0, FAKE, 8, 1, 1, 8, FAKE, 0, NULL),
            b"mmk_conv3x3_wgrad_partial: bad input split 4+0")


def test_fused_backward_entries(L):
    big = (32768, 256, 256)           # B * H * W * C = 2^34 elements
    refused(L, L.mmk_conv_bwd_fused(FAKE, NULL, FAKE, 1.0, 1, 8, 8, 8, FAKE, FAKE, 0, NULL), b"mmk_conv_bwd_fused: NULL pointer")
    refused(L, L.mmk_conv_bwd_fused(FAKE, FAKE, FAKE, 1.0, 1, 8, 8, 32, FAKE, FAKE, 0, NULL),
            b"mmk_conv_bwd_fused: bad shape (8 or 16 channels)")
    refused(L, L.mmk_conv_bwd_fused(FAKE, FAKE, FAKE, 1.0, *big, 8, FAKE, FAKE, 0, NULL),
            b"mmk_conv_bwd_fused: tensor too large for 32-bit offsets")
    refused(L, L.mmk_conv_bwd_fused_pooled(FAKE, FAKE, NULL, 1.0, FAKE, 1.0, 1, 8, 8, 16, FAKE, FAKE, 0, NULL),
            b"mmk_conv_bwd_fused_pooled: NULL pointer")
    refused(L, L.mmk_conv_bwd_fused_pooled(FAKE, FAKE, FAKE, 1.0, FAKE, 1.0, 1, 8, 8, 8, FAKE, FAKE, 0, NULL),
            b"mmk_conv_bwd_fused_pooled: bad shape (16 channels)")
    refused(L, L.mmk_conv_bwd_fused_pooled(FAKE, FAKE, FAKE, 1.0, FAKE, 1.0, *big, 16, FAKE, FAKE, 0, NULL),
            b"mmk_conv_bwd_fused_pooled: tensor too large for 32-bit offsets")
    refused(L, L.mmk_conv8x16_bwd_fused(FAKE, FAKE, FAKE, 1.0, 1, 8, 8, NULL, FAKE, 0, NULL), b"mmk_conv8x16_bwd_fused: NULL pointer")
    refused(L, L.mmk_conv8x16_bwd_fused(FAKE, FAKE, FAKE, 1.0, 1, 1, 8, FAKE, FAKE, 0, NULL), b"mmk_conv8x16_bwd_fused: bad shape")
    refused(L, L.mmk_conv8x16_bwd_fused(FAKE, FAKE, FAKE, 1.0, *big, FAKE, FAKE, 0, NULL),
            b"mmk_conv8x16_bwd_fused: tensor too large for 32-bit offsets")
    refused(L, L.mmk_conv16x8_bwd_fused(FAKE, NULL, FAKE, FAKE, 1.0, 1, 8, 8, FAKE, NULL, NULL, 0, NULL),
            b"mmk_conv16x8_bwd_fused: NULL pointer")
    refused(L, L.mmk_conv16x8_bwd_fused(FAKE, FAKE, FAKE, FAKE, 1.0, 1, 8, 8, FAKE, NULL, FAKE, 0, NULL),
            b"mmk_conv16x8_bwd_fused: x2 and dx2 go together (both NULL: one 16-channel input / unmasked output)")
    refused(L, L.mmk_conv16x8_bwd_fused(FAKE, NULL, FAKE, FAKE, 1.0, 0, 8, 8, FAKE, NULL, FAKE, 0, NULL),
            b"mmk_conv16x8_bwd_fused: bad shape")
    refused(L, L.mmk_conv16x8_bwd_fused(FAKE, FAKE, FAKE, FAKE, 1.0, *big, FAKE, FAKE, FAKE, 0, NULL),
            b"mmk_conv16x8_bwd_fused: tensor too large for 32-bit offsets")


def test_max_pool_entries(L):
    refused(L, L.mmk_maxpool2_fwd(FAKE, 1, 8, 8, 12, FAKE, NULL), b"mmk_maxpool2_fwd: bad argument")
    refused(L, L.mmk_maxpool2_fwd_arg(FAKE, 1, 8, 8, 8, FAKE, NULL, NULL), b"mmk_maxpool2_fwd_arg: bad argument")
    refused(L, L.mmk_maxpool2_bwd_arg(FAKE, FAKE, 1, 1, 8, 8, 1.0, FAKE, NULL), b"mmk_maxpool2_bwd_arg: bad argument")
    refused(L, L.mmk_maxpool2_bwd(FAKE, FAKE, 0, 8, 8, 8, 1.0, 0.0, FAKE, NULL), b"mmk_maxpool2_bwd: bad argument")


def test_final_layer_backward_entries(L):
    refused(L, L.mmk_final_bwd(FAKE, FAKE, FAKE, FAKE, 0, 1.0, 0.0, FAKE, FAKE, FAKE, FAKE, NULL), b"mmk_final_bwd: bad argument")
    refused(L, L.mmk_final_bwd(FAKE, FAKE, FAKE, FAKE, 64, 1.0, 0.0, FAKE, FAKE, FAKE, NULL, NULL), b"mmk_final_bwd: bad argument")
    refused(L, L.mmk_final_bwd_normalized(FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, 1, 64, 1.0, 0.0, FAKE, FAKE, FAKE, FAKE, FAKE, NULL, NULL),
            b"mmk_final_bwd_normalized: NULL pointer")
    refused(L, L.mmk_final_bwd_normalized(FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, 0, 64, 1.0, 0.0, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, NULL),
            b"mmk_final_bwd_normalized: bad shape")
    refused(L, L.mmk_final_bwd_normalized(FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, 65536, 64, 1.0, 0.0, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, NULL),
            b"mmk_final_bwd_normalized: bad shape")


def unet_desc(L, params=None, **over):
    if params is None:
        params = (ctypes.c_void_p * 46)(*[4096] * 46)
    kw = dict(B=B, H=H, W=W, cin=CIN, x=4096, pre=None, params=params, drop_p=0.1, seed=1, leaky_slope=0.0, norm=1, workspace=4096,
              workspace_bytes=L.mmk_unet_workspace_bytes(B, H, W, CIN), mask=4096, keep_full_res=0)
    kw.update(over)
    return _lib.UNetDesc(**kw)


def test_unet_forward(L):
    need = L.mmk_unet_workspace_bytes(B, H, W, CIN)
    assert need > 0
    refused(L, L.mmk_unet_forward(None, NULL), b"mmk_unet_forward: NULL descriptor")
    refused(L, L.mmk_unet_forward(ctypes.byref(unet_desc(L, mask=None)), NULL), b"mmk_unet_forward: NULL pointer")
    refused(L, L.mmk_unet_forward(ctypes.byref(unet_desc(L, H=16)), NULL),
            b"mmk_unet_forward: unsupported network input (B=2, 16 x 64, 1 channels)")
    refused(L, L.mmk_unet_forward(ctypes.byref(unet_desc(L, workspace_bytes=need - 1)), NULL),
            b"mmk_unet_forward: workspace too small (%d < %d bytes)" % (need - 1, need))
    refused(L, L.mmk_unet_forward(ctypes.byref(unet_desc(L, drop_p=1.0)), NULL),
            b"mmk_unet_forward: dropout probability 1 out of range (it is quantised to thr / 65536, thr <= 65535)")
    holed = (ctypes.c_void_p * 46)(*[4096] * 46)
    holed[3] = None
    refused(L, L.mmk_unet_forward(ctypes.byref(unet_desc(L, params=holed)), NULL), b"mmk_unet_forward: NULL parameter 3")


def test_unet_backward_entries(L):
    d = unet_desc(L)
    grads = (ctypes.c_void_p * 46)(*[4096] * 46)
    events = (ctypes.c_void_p * 3)(4096, 4096, 4096)
    holed = (ctypes.c_void_p * 3)(4096, None, 4096)
    # the common body, under the name it has always reported
    refused(L, L.mmk_unet_backward(None, FAKE, grads, FAKE, 1 << 40, NULL), b"mmk_unet_backward: NULL descriptor")
    refused(L, L.mmk_unet_backward_buckets(None, FAKE, grads, FAKE, 1 << 40, events, NULL), b"mmk_unet_backward: NULL descriptor")
    refused(L, L.mmk_unet_backward(ctypes.byref(d), NULL, grads, FAKE, 1 << 40, NULL), b"mmk_unet_backward: NULL pointer")
    refused(L, L.mmk_unet_backward_buckets(ctypes.byref(d), NULL, grads, FAKE, 1 << 40, events, NULL), b"mmk_unet_backward: NULL pointer")
    refused(L, L.mmk_unet_backward_input(ctypes.byref(d), NULL, grads, FAKE, 0, NULL, FAKE, 1 << 40, None, NULL),
            b"mmk_unet_backward: NULL pointer")
    small = unet_desc(L, W=31)
    refused(L, L.mmk_unet_backward(ctypes.byref(small), FAKE, grads, FAKE, 1 << 40, NULL), b"mmk_unet_backward: unsupported network input")
    refused(L, L.mmk_unet_backward_input(ctypes.byref(small), FAKE, grads, FAKE, 0, NULL, FAKE, 1 << 40, events, NULL),
            b"mmk_unet_backward: unsupported network input")
    # each entry's own checks, under its own name
    refused(L, L.mmk_unet_backward_buckets(ctypes.byref(d), FAKE, grads, FAKE, 1 << 40, None, NULL),
            b"mmk_unet_backward_buckets: NULL event array")
    refused(L, L.mmk_unet_backward_buckets(ctypes.byref(d), FAKE, grads, FAKE, 1 << 40, holed, NULL),
            b"mmk_unet_backward_buckets: NULL event 1")
    refused(L, L.mmk_unet_backward_input(None, FAKE, grads, FAKE, 0, NULL, FAKE, 1 << 40, None, NULL),
            b"mmk_unet_backward_input: NULL descriptor")
    refused(L, L.mmk_unet_backward_input(ctypes.byref(d), FAKE, grads, NULL, 0, NULL, FAKE, 1 << 40, None, NULL),
            b"mmk_unet_backward_input: NULL pointer (grad_x)")
    refused(L, L.mmk_unet_backward_input(ctypes.byref(unet_desc(L, cin=5)), FAKE, grads, FAKE, 0, NULL, FAKE, 1 << 40, None, NULL),
            b"mmk_unet_backward_input: bad shape (cin must be 1..4)")
    refused(L, L.mmk_unet_backward_input(ctypes.byref(d), FAKE, grads, FAKE, 7, NULL, FAKE, 1 << 40, None, NULL),
            b"mmk_unet_backward_input: unknown normalisation mode 7")
    refused(L, L.mmk_unet_backward_input(ctypes.byref(d), FAKE, grads, FAKE, 1, FAKE, FAKE, 1 << 40, None, NULL),
            b"mmk_unet_backward_input: normalisation mode 1 needs d->pre (NULL pointer)")
    refused(L, L.mmk_unet_backward_input(ctypes.byref(unet_desc(L, pre=4096)), FAKE, grads, FAKE, 1, NULL, FAKE, 1 << 40, None, NULL),
            b"mmk_unet_backward_input: MMK_NORM_MINMAX needs minmax (NULL pointer)")
    refused(L, L.mmk_unet_backward_input(ctypes.byref(d), FAKE, grads, FAKE, 0, NULL, FAKE, 1 << 40, holed, NULL),
            b"mmk_unet_backward_input: NULL event 1")
