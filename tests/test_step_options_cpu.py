"""CPU-only: the C-ABI entry points of the non-default step options (pose terms against a ground-truth pose, the validation
metric, the fft-threshold mask loss, standardisation folded into the first layer) are declared, exported and bound, and
reject bad arguments on the host before anything is launched."""
import ctypes
import os
import re

import pytest

from mm_masking_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mmk_pose_loss_gt_fwd", "mmk_pose_loss_gt_bwd", "mmk_val_metric", "mmk_fft_threshold_ws_bytes", "mmk_fft_threshold_mask",
       "mmk_bce_fft_threshold_fwd", "mmk_bce_fft_threshold_bwd", "mmk_channel_meanstd"]
NULL = ctypes.c_void_p(0)


@pytest.fixture(scope="module")
def L():
    _lib.build()
    return _lib.lib()


def _p(addr):
    return ctypes.c_void_p(addr)


def test_new_symbols_declared_exported_and_bound(L):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mmk.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(mmk_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared, name
        assert hasattr(L, name), name
        assert name in _lib.EXPORTED, name


def test_pose_entry_points_reject_bad_arguments(L):
    a, b, o = _p(0x10000), _p(0x20000), _p(0x30000)
    assert L.mmk_pose_loss_gt_fwd(NULL, b, 4, o, NULL) == -1
    assert b"mmk_pose_loss_gt_fwd" in L.mmk_last_error()
    assert L.mmk_pose_loss_gt_fwd(a, NULL, 4, o, NULL) == -1          # T_gt is required (the identity form has its own entry)
    assert L.mmk_pose_loss_gt_fwd(a, b, 4, NULL, NULL) == -1
    assert L.mmk_pose_loss_gt_fwd(a, b, 0, o, NULL) == -1
    assert L.mmk_pose_loss_gt_bwd(a, NULL, 4, NULL, NULL, o, NULL) == -1
    assert L.mmk_pose_loss_gt_bwd(a, b, 4, NULL, NULL, NULL, NULL) == -1
    assert L.mmk_pose_loss_gt_bwd(a, b, -1, NULL, NULL, o, NULL) == -1
    assert b"mmk_pose_loss_gt_bwd" in L.mmk_last_error()
    assert L.mmk_val_metric(NULL, b, 4, o, NULL) == -1
    assert L.mmk_val_metric(a, b, 4, NULL, NULL) == -1
    assert L.mmk_val_metric(a, NULL, 0, o, NULL) == -1
    assert b"mmk_val_metric" in L.mmk_last_error()


def test_gt_eye_pose_and_bce_entry_points_reject_bad_arguments(L):
    a, o, g = _p(0x10000), _p(0x30000), _p(0x40000)
    assert L.mmk_pose_loss_fwd(NULL, 4, o, NULL) == -1
    assert L.mmk_pose_loss_fwd(a, 4, NULL, NULL) == -1
    assert L.mmk_pose_loss_fwd(a, 0, o, NULL) == -1
    assert b"mmk_pose_loss_fwd" in L.mmk_last_error()
    assert L.mmk_pose_loss_bwd(NULL, 4, NULL, NULL, g, NULL) == -1
    assert L.mmk_pose_loss_bwd(a, 4, NULL, NULL, NULL, NULL) == -1
    assert L.mmk_pose_loss_bwd(a, -1, o, o, g, NULL) == -1
    assert b"mmk_pose_loss_bwd" in L.mmk_last_error()
    n, ws_bytes = 4097, L.mmk_bce_ws_bytes()
    assert ws_bytes == 2048 * 8                              # one fp64 partial per block of the forward's grid
    x, t, ws = _p(0x50000), _p(0x60000), _p(0x70000)
    assert L.mmk_bce_mean_fwd(NULL, t, n, ws, ws_bytes, o, NULL) == -1
    assert L.mmk_bce_mean_fwd(x, NULL, n, ws, ws_bytes, o, NULL) == -1
    assert L.mmk_bce_mean_fwd(x, t, n, NULL, ws_bytes, o, NULL) == -1
    assert L.mmk_bce_mean_fwd(x, t, n, ws, ws_bytes, NULL, NULL) == -1
    assert L.mmk_bce_mean_fwd(x, t, 0, ws, ws_bytes, o, NULL) == -1
    assert b"mmk_bce_mean_fwd: bad argument" in L.mmk_last_error()
    assert L.mmk_bce_mean_fwd(x, t, n, ws, ws_bytes - 1, o, NULL) == -1
    assert b"workspace" in L.mmk_last_error()
    assert L.mmk_bce_mean_fwd(_p(0x50004), t, n, ws, ws_bytes - 1, o, NULL) == -1       # the workspace is examined first
    assert b"workspace" in L.mmk_last_error()
    assert L.mmk_bce_mean_fwd(_p(0x50004), t, n, ws, ws_bytes, o, NULL) == -1
    assert b"aligned" in L.mmk_last_error()
    L.mmk_bce_mean_fwd(x, t, 0, ws, ws_bytes, o, NULL)                                  # (a fresh message in between)
    assert L.mmk_bce_mean_fwd(x, _p(0x60008), n, ws, ws_bytes, o, NULL) == -1
    assert b"aligned" in L.mmk_last_error()
    assert L.mmk_bce_mean_bwd(NULL, t, n, o, g, NULL) == -1
    assert L.mmk_bce_mean_bwd(x, NULL, n, o, g, NULL) == -1
    assert L.mmk_bce_mean_bwd(x, t, n, NULL, g, NULL) == -1
    assert L.mmk_bce_mean_bwd(x, t, n, o, NULL, NULL) == -1
    assert L.mmk_bce_mean_bwd(x, t, 0, o, g, NULL) == -1
    assert b"mmk_bce_mean_bwd: bad argument" in L.mmk_last_error()
    for bad in ((_p(0x50004), t, g), (x, _p(0x60008), g), (x, t, _p(0x4000c))):
        L.mmk_bce_mean_bwd(x, t, 0, o, g, NULL)
        assert L.mmk_bce_mean_bwd(bad[0], bad[1], n, o, bad[2], NULL) == -1
        assert b"aligned" in L.mmk_last_error()


def test_fft_threshold_entry_points_reject_bad_arguments(L):
    B, hw = 3, 640 * 640
    ws_bytes = L.mmk_fft_threshold_ws_bytes(B)
    assert ws_bytes >= B * 4 + L.mmk_bce_ws_bytes()         # the thresholds and the BCE block partials fit
    assert L.mmk_fft_threshold_ws_bytes(64) > L.mmk_fft_threshold_ws_bytes(1)
    assert L.mmk_fft_threshold_ws_bytes(0) == 0
    f, ws, m, t, o = _p(0x10000), _p(0x20000), _p(0x30000), _p(0x40000), _p(0x50000)
    assert L.mmk_fft_threshold_mask(NULL, B, hw, ws, ws_bytes, m, NULL) == -1
    assert L.mmk_fft_threshold_mask(f, B, hw, NULL, ws_bytes, m, NULL) == -1
    assert L.mmk_fft_threshold_mask(f, 0, hw, ws, ws_bytes, m, NULL) == -1
    assert L.mmk_fft_threshold_mask(f, B, 3, ws, ws_bytes, m, NULL) == -1
    assert L.mmk_fft_threshold_mask(f, B, hw, ws, ws_bytes - 1, m, NULL) == -1
    assert b"workspace" in L.mmk_last_error()
    assert L.mmk_fft_threshold_mask(_p(0x10004), B, hw, ws, ws_bytes, m, NULL) == -1
    assert b"aligned" in L.mmk_last_error()
    assert L.mmk_fft_threshold_mask(f, B, hw, ws, ws_bytes, _p(0x30008), NULL) == -1
    x = _p(0x60000)
    assert L.mmk_bce_fft_threshold_fwd(NULL, f, B, hw, ws, ws_bytes, t, o, NULL) == -1
    assert L.mmk_bce_fft_threshold_fwd(x, f, B, hw, ws, ws_bytes, NULL, o, NULL) == -1
    assert L.mmk_bce_fft_threshold_fwd(x, f, 0, hw, ws, ws_bytes, t, o, NULL) == -1
    assert L.mmk_bce_fft_threshold_fwd(x, f, B, hw, ws, ws_bytes - 8, t, o, NULL) == -1
    assert b"workspace" in L.mmk_last_error()
    assert L.mmk_bce_fft_threshold_fwd(_p(0x60004), f, B, hw, ws, ws_bytes, t, o, NULL) == -1
    assert b"aligned" in L.mmk_last_error()
    g = _p(0x70000)
    assert L.mmk_bce_fft_threshold_bwd(x, f, B, hw, NULL, o, g, NULL) == -1
    assert L.mmk_bce_fft_threshold_bwd(x, f, B, hw, t, NULL, g, NULL) == -1
    assert L.mmk_bce_fft_threshold_bwd(x, f, 0, hw, t, o, g, NULL) == -1
    assert L.mmk_bce_fft_threshold_bwd(x, f, B, hw, t, o, _p(0x70002), NULL) == -1
    assert b"aligned" in L.mmk_last_error()


def test_channel_meanstd_rejects_bad_arguments(L):
    x, part, pre = _p(0x10000), _p(0x20000), _p(0x30000)
    assert L.mmk_channel_meanstd(NULL, 2, 1, 4096, part, pre, NULL) == -1
    assert L.mmk_channel_meanstd(x, 2, 1, 4096, NULL, pre, NULL) == -1
    assert L.mmk_channel_meanstd(x, 2, 1, 4096, part, NULL, NULL) == -1
    assert L.mmk_channel_meanstd(x, 0, 1, 4096, part, pre, NULL) == -1
    assert L.mmk_channel_meanstd(x, 2, 0, 4096, part, pre, NULL) == -1
    assert L.mmk_channel_meanstd(x, 2, 1, 0, part, pre, NULL) == -1
    assert b"mmk_channel_meanstd" in L.mmk_last_error()


def test_cpu_tensors_keep_the_pytorch_expressions():
    """On the host the loss terms stay the reference's PyTorch expressions (the mirror test_losses_cpu.py checks): the
    ground-truth pose terms, the validation metric and the fft target match a direct evaluation."""
    import torch
    from mm_masking_amd import train_icp_weights as trn
    g = torch.Generator().manual_seed(5)
    B = 3
    Tp = torch.eye(4).repeat(B, 1, 1) + 0.1 * torch.randn(B, 4, 4, generator=g)
    Tg = torch.eye(4).repeat(B, 1, 1) + 0.1 * torch.randn(B, 4, 4, generator=g)
    mask = torch.rand(B, 8, 8, generator=g) * 0.98 + 0.01
    fft = torch.rand(B, 8, 8, generator=g) ** 8
    lw = {"icp_rot": 1.0, "icp_trans": 1.0, "fft": 0.5, "mask_pts": 0.0, "cfar": 0.0, "num_pts": 0.0}
    loss, comp = trn.eval_training_loss(Tp, mask, None, Tg, {"fft_data": fft}, None, None, loss_weights=lw, gt_eye=False)
    xi = Tp @ torch.inverse(Tg) - torch.eye(4)
    torch.testing.assert_close(comp["rot"], xi[:, 1, 0].abs().mean())
    torch.testing.assert_close(comp["trans"], xi[:, 0:2, 3].norm(dim=1).mean())
    tgt = (fft > 3.0 * fft.mean(dim=(1, 2), keepdim=True)).float()
    assert 0 < int(tgt.sum()) < tgt.numel()
    torch.testing.assert_close(comp["fft"], 0.5 * torch.nn.BCELoss()(mask, tgt))
    v = trn.eval_validation_loss(Tp, Tg, gt_eye=False)
    xs = torch.stack((xi[:, 1, 0], xi[:, 0, 3], xi[:, 1, 3]), dim=1)
    torch.testing.assert_close(v, torch.stack((xs.norm(dim=1).mean(), xs[:, 0].abs().mean(), xs[:, 1:].norm(dim=1).mean())))
