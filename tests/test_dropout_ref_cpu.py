"""Deterministic CPU checks of the host restatement of the dropout hash (tests/dropout_ref.py): the rates it must have at the
benchmarked probability, independence of the masks of consecutive layers and of consecutive steps, distinct seeds, and the
agreement of the two host-side statements of 1 / keep."""
import numpy as np
import pytest

import dropout_ref as dr

N = 1 << 22
THR = 3277                      # round(0.05 * 65536)
P = THR / 65536.0


def _dropped(seed):
    return dr.draws(seed, N).astype(np.int32) < THR - 32768


def _within(rate, q, n, what):
    """|rate - q| <= 5 binomial standard deviations of a rate over n independent draws of probability q."""
    bound = 5.0 * np.sqrt(q * (1.0 - q) / n)
    assert abs(rate - q) <= bound, (what, rate, q, bound)


def test_params_quantisation():
    assert dr.params(0.05) == dr.Params(THR, np.float32(65536.0) / np.float32(65536 - THR), THR - 32768)
    assert dr.params(0.0).thr == 0 and dr.params(0.0).inv_keep == np.float32(1.0)
    assert dr.params(1e-6).thr == 0 and dr.params(1.0 / 65536).thr == 1 and dr.params(0.5).thr == 32768
    assert dr.params(65535.0 / 65536).thr == 65535 and dr.params(65535.0 / 65536).inv_keep == np.float32(65536.0)
    assert dr.params(1.0 - 1e-6).thr == 65536


def test_draws_layout_and_base():
    """Element r of a group: low / high half of h, low / high half of g; `base` shifts the element index, also by a
    non-multiple of 4, and the index wraps at 2^32."""
    seed = 12345
    h, g = dr.words(seed, np.arange(8))
    want = np.stack([h & 0xffff, h >> 16, g & 0xffff, g >> 16], 1).astype(np.uint16).reshape(-1).view(np.int16)
    assert np.array_equal(dr.draws(seed, 32), want)
    assert np.array_equal(dr.draws(seed, 20, base=6), want[6:26])
    far = dr.draws(seed, 64, base=(1 << 32) - 32)
    assert np.array_equal(far[32:], want[:32])
    # the group-number term: group 2^24 + k is not group k (the 24-bit multiply alone would make them equal)
    a = dr.draws(seed, 4096, base=1 << 26)
    assert not np.array_equal(a, dr.draws(seed, 4096)) and not np.array_equal(a, dr.draws(seed, 4096, base=4))
    m = dr.keep_mask(seed, (2, 3, 5, 8), P, base=16)
    assert m.shape == (2, 3, 5, 8) and np.array_equal(m.reshape(-1), dr.draws(seed, 240, base=16).astype(np.int32) >= THR - 32768)


def test_rates_at_the_benchmarked_probability():
    s = 3
    d1 = _dropped(dr.layer_seed(s, 1))
    _within(1.0 - d1.mean(), 1.0 - P, N, "keep rate")
    d2 = _dropped(dr.layer_seed(s, 2))
    _within((d1 & d2).mean(), P * P, N, "joint drop, consecutive layers")
    d16 = _dropped(dr.layer_seed(s, 16))
    n1 = _dropped(dr.layer_seed(s + 1, 1))
    _within((d16 & n1).mean(), P * P, N, "joint drop, last layer of a step and first of the next")


def test_seeds_of_two_steps_are_distinct():
    for s in (0, 9, 12345, (1 << 26) - 1):
        seeds = [dr.layer_seed(s, k) for k in range(1, 17)] + [dr.layer_seed(s + 1, k) for k in range(1, 17)]
        assert len(set(seeds)) == 32
        assert all(0 <= v < (1 << 32) for v in seeds)


@pytest.mark.parametrize("p", [0.0, 1e-6, 1.0 / 65536, 0.05, 0.25, 0.5, 65535.0 / 65536])
def test_dropout_scale_agrees_with_params(p):
    from mm_masking_amd import unet_hip as uh
    assert np.float32(uh.dropout_scale(p)) == dr.params(p).inv_keep
