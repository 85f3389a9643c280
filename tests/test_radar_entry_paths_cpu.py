"""CPU: what the shared launch paths of the radar entries report on the host (no launch) and no other CPU test pins: both
ordered-scatter samplers name a workspace one byte short alike, as an argument error with the two sizes in bytes.  (The other
return codes and texts of tests/test_gpu_radar_entry_paths.py's entries are in test_radar_grads_cpu.py, test_resample_grads_cpu.py,
test_mask_scan_cpu.py, test_cfar_params_cpu.py and test_polar_weights_cpu.py.)"""
import ctypes

import pytest

from mm_masking_amd import _lib

NULL = ctypes.c_void_p(0)
FAKE = ctypes.c_void_p(4096)          # never dereferenced: every call below fails on the host before any launch
B, N, COLS = 1, 4, 3


@pytest.fixture(scope="module")
def L():
    _lib.build()
    return _lib.lib()


def test_both_samplers_report_a_workspace_one_byte_short_alike(L):
    need = L.mmk_sample_weights_bwd_ws_bytes(B, N)
    assert need == L.mmk_sample_weights_polar_bwd_ws_bytes(B, N) == B * N * 4 * 4 * 4     # next | val | pix | res per (point, tap)
    assert L.mmk_sample_weights_bwd(FAKE, FAKE, B, N, COLS, 16, 16, 16, 0.5, FAKE, FAKE, need - 1, NULL) == -1
    assert L.mmk_last_error() == b"mmk_sample_weights_bwd: workspace too small (%d < %d bytes)" % (need - 1, need)
    assert L.mmk_sample_weights_polar_bwd(FAKE, FAKE, FAKE, B, N, COLS, 16, 96, 0.0596, 1, 1, FAKE, FAKE, need - 1, NULL) == -1
    assert L.mmk_last_error() == b"mmk_sample_weights_polar_bwd: workspace too small (%d < %d bytes)" % (need - 1, need)
