"""The U-Net entries that share one host path give the same bits, whichever entry reaches that path and whatever ran before.

Through the C ABI directly; B = 2 so that a stride error shows in the second item.  No tolerance anywhere: every comparison is
torch.equal, between entries that must run the same launches or between two runs of one entry.

  backward   mmk_unet_backward == mmk_unet_backward_buckets == mmk_unet_backward_input (mode none; with and without events):
             the same 46 parameter gradients; the three bucket events are complete after a synchronize; grad_x is the same with
             and without events.  ReLU network with the normalised mask, and the LeakyReLU network on a 3-channel input.
  sizes      forward + backward twice from a workspace and a scratch of exactly mmk_unet_workspace_bytes / _scratch_bytes (a
             guard page behind each stays untouched): the same bits both times.  One byte less is refused before any launch, by
             all three backward entries under the name of their common body (the texts tests/test_unet_entry_paths_cpu.py
             cannot reach: without a device the scratch size is unknown).
  first use  a fresh child process whose first kernel launches are the pooled-gradient variants (tests/unet_entry_calls.py).
What other tests already hold: tests/test_gpu_pool_adjoint_fused.py compares the pooled entries with the plain composite in suite
order (so after plain calls); test_gpu_unet_kernels.py::test_conv_deep_sub_batch_split_bit_identical the split that sizes itself
by the persistent grid (deep_rounds); test_gpu_unet_driver.py the native driver against the per-call schedule (the descriptor
builder, second_conv_bwd, fork, pack_all); test_gpu_unet_kernels.py's test_bwd*_fused_* the four fused-backward entries against
the two-kernel path, and its weight-gradient tests every shape of the table through both mmk_conv3x3_wgrad_slices and the launch.
"""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

from mm_masking_amd import _lib
from unet_entry_calls import DEV, NULL, Net, P

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 4096


def _guarded(nbytes):
    """A buffer of exactly nbytes and the guard bytes behind it (one allocation, the guard filled with 0xA5)."""
    whole = torch.full((nbytes + GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
    return whole[:nbytes], whole[nbytes:]


@pytest.fixture(scope="module", params=[(2, 1, 64, 64, 0.0, 0.1, 1), (2, 3, 64, 96, 0.1, 0.05, 0)], ids=["relu-norm", "leaky-3ch"])
def net_after_forward(request):
    net = Net(*request.param)
    ws = torch.empty(net.ws_bytes, dtype=torch.uint8, device=DEV)
    net.forward(ws)
    return net, ws, torch.empty(net.scratch_bytes, dtype=torch.uint8, device=DEV)


def test_the_three_backward_entries_give_the_same_gradients(net_after_forward):
    net, ws, scratch = net_after_forward
    events = [torch.cuda.Event() for _ in range(3)]
    for e in events:
        e.record()          # (creates the handle)
    want, _ = net.backward("", ws, scratch)
    assert all(bool(g.abs().sum() > 0) for g in want)
    got_b, _ = net.backward("_buckets", ws, scratch, events)
    assert all(e.query() for e in events)
    got_e, gx_e = net.backward("_input", ws, scratch, events)
    assert all(e.query() for e in events)
    got_i, gx_i = net.backward("_input", ws, scratch)
    for k in range(46):
        assert torch.equal(want[k], got_b[k]) and torch.equal(want[k], got_e[k]) and torch.equal(want[k], got_i[k]), k
    assert torch.equal(gx_e, gx_i) and bool(gx_i.abs().sum() > 0)


def test_exact_size_buffers_twice_give_the_same_bits():
    net = Net(2, 1, 64, 64, 0.0, 0.1, 1)
    (ws, ws_guard), (scratch, sc_guard) = _guarded(net.ws_bytes), _guarded(net.scratch_bytes)
    runs = []
    for _ in range(2):
        mask = net.forward(ws)
        grads, gx = net.backward("_input", ws, scratch)
        runs.append([mask, gx] + grads)
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    assert bool((ws_guard == 0xA5).all()) and bool((sc_guard == 0xA5).all())


def test_one_byte_short_is_refused_before_any_launch():
    L, net = _lib.lib(), Net(2, 1, 64, 64, 0.0, 0.1, 1)
    fake = torch.empty(16, dtype=torch.uint8, device=DEV)          # never dereferenced
    gp = (ctypes.c_void_p * 46)(*[fake.data_ptr()] * 46)
    calls = {"": lambda d, n: L.mmk_unet_backward(ctypes.byref(d), P(fake), gp, P(fake), n, NULL),
             "_buckets": lambda d, n: L.mmk_unet_backward_buckets(ctypes.byref(d), P(fake), gp, P(fake), n, gp, NULL),
             "_input": lambda d, n: L.mmk_unet_backward_input(ctypes.byref(d), P(fake), gp, P(fake), 0, NULL, P(fake), n, None, NULL)}
    for entry, call in calls.items():
        assert call(net.desc(fake, net.ws_bytes - 1), net.scratch_bytes) == -1
        assert L.mmk_last_error() == b"mmk_unet_backward: workspace too small", entry
        assert call(net.desc(fake), net.scratch_bytes - 1) == -1
        assert L.mmk_last_error() == b"mmk_unet_backward: scratch too small (%d < %d bytes)" % (net.scratch_bytes - 1, net.scratch_bytes), entry


def test_pooled_variants_as_the_first_calls_of_a_process():
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "unet_entry_calls.py"), "first-calls"], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "first-calls ok 7" in r.stdout         # 2 + 3 + 2 results, each equal to its plain composite
