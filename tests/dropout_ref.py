"""Host restatement of the library's dropout mask (csrc/mmk_unet_shared.h: dropout_params, dropout_words, dropout_draws4),
written from the definitions there: numpy only, no GPU, no import of the package.  It is the definition the GPU tests pin
every kernel to (tests/test_gpu_dropout_masks.py) and the one copy of the hash arithmetic (scripts/dropout_hash_check.py
imports it).

  element index   e = ((b H + y) W + x) C + c + base   (mod 2^32; C = the LAYER's output channel count)
  group           i = e >> 2: the 4 consecutive channels e & ~3 .. e | 3 share two 32-bit hash words (h, g)
  draw            signed 16-bit: element e & 3 = 0..3 takes  low half of h, high half of h, low half of g, high half of g
  kept            draw >= thr - 32768, thr = round(p * 65536) in fp32; a kept value is scaled by 65536 / (65536 - thr)
"""
import collections

import numpy as np

M32 = np.uint64(0xffffffff)
M24 = np.uint64(0xffffff)

Params = collections.namedtuple("Params", "thr inv_keep thr_s")


def params(p):
    """dropout_params: thr = (unsigned)(p * 65536.0f + 0.5f), inv_keep = 65536.0f / (float)(65536 - thr) (1 for thr = 0) as
    np.float32, thr_s = thr - 32768."""
    thr = int(np.float32(np.float32(p) * np.float32(65536.0)) + np.float32(0.5))
    if thr == 0:
        inv = np.float32(1.0)
    elif thr >= 65536:
        inv = np.float32(np.inf)
    else:
        inv = np.float32(65536.0) / np.float32(65536 - thr)
    return Params(thr, np.float32(inv), thr - 32768)


def umul24(a, b):
    """__umul24: low 32 bits of (a & 0xffffff) * (b & 0xffffff); a is a uint64 array holding 32-bit values."""
    return ((a & M24) * (np.uint64(b) & M24)) & M32


def words(seed, group):
    """dropout_words: the two 32-bit hash words (h, g) of the group numbers `group`, as uint64 arrays of 32-bit values."""
    i = np.asarray(group, dtype=np.uint64) & M32
    s = np.uint64(int(seed) & 0xffffffff)
    h = (umul24(i, 0x9E3779) + ((s + (i & np.uint64(0xff000000))) & M32)) & M32
    h ^= h >> np.uint64(13)
    h = (umul24(h, 0x85EBCA) + h) & M32
    h ^= h >> np.uint64(11)
    h = (umul24(h, 0xC2B2AE) + h) & M32
    h ^= h >> np.uint64(15)
    g = h ^ np.uint64(0x85ebca6b)
    g ^= g >> np.uint64(12)
    g = (umul24(g, 0x7FEB34) + g) & M32
    g ^= g >> np.uint64(14)
    return h, g


def draws(seed, n_elems, base=0):
    """The signed 16-bit draws of the elements base .. base + n_elems - 1 (mod 2^32) as an int16 array."""
    base = int(base) & 0xffffffff
    g0 = base >> 2
    g1 = (base + int(n_elems) + 3) >> 2                      # one past the last group touched (before the wrap)
    grp = (np.arange(g0, g1, dtype=np.uint64)) & np.uint64(0x3fffffff)      # (e mod 2^32) >> 2
    h, g = words(seed, grp)
    d = np.empty((grp.size, 4), dtype=np.uint16)
    d[:, 0] = (h & np.uint64(0xffff)).astype(np.uint16)
    d[:, 1] = (h >> np.uint64(16)).astype(np.uint16)
    d[:, 2] = (g & np.uint64(0xffff)).astype(np.uint16)
    d[:, 3] = (g >> np.uint64(16)).astype(np.uint16)
    off = base & 3
    return d.reshape(-1)[off:off + int(n_elems)].view(np.int16)


def keep_mask(seed, shape_BHWC, p, base=0):
    """bool (B,H,W,C): True where the element of index ((b H + y) W + x) C + c + base (mod 2^32) is kept at probability p."""
    n = int(np.prod(shape_BHWC))
    return (draws(seed, n, base).astype(np.int32) >= params(p).thr_s).reshape(shape_BHWC)


def layer_seed(step_seed, k):
    """Seed of the k-th dropout launch of a forward pass, k = 1 .. 16 in launch order: encoder block 0's second convolution,
    the second convolutions of encoder blocks 1-5, then per decoder block the two applications of its second convolution
    (unet_hip._UNet.forward, mmk_unet_driver.hip: ctr = seed * 64, ++ctr per launch)."""
    return (int(step_seed) * 64 + int(k)) & 0xffffffff
