"""Shared by test_input_grads_cpu.py and test_gpu_input_grads.py: the two configurations of tests/golden/input_grads.npz
(make_golden_input_grads.py) rebuilt on this package's policy module, and the fp64 definition of the first layer's
input gradient."""
import os

import numpy as np
import torch

from mm_masking_amd import train_icp_weights as trn
from mm_masking_amd.icp_weight_policy import LearnICPWeightPolicy

OVER = {"n1": {}, "n3": {"cfar_input": True, "range_input": True, "leaky": True, "log_transform": True}}


def load_golden(golden_dir):
    return np.load(os.path.join(golden_dir, "input_grads.npz"), allow_pickle=False)


def golden_model(g, tag, device, **extra):
    """The reference's seed-1234 network of configuration ``tag`` (normalisation off, dropout 0) on ``device``."""
    p = trn.default_params(device)
    p.update({"dropout": 0.0, "normalize": ["none"]})
    p.update(OVER[tag])
    p.update(extra)
    torch.manual_seed(1234)
    model = LearnICPWeightPolicy(p).to(device)
    model.train()
    np.testing.assert_allclose([v.double().sum().item() for v in model.state_dict().values()], g["psum_" + tag], atol=1e-6)
    if p["range_input"]:
        model.range_mask = torch.from_numpy(g["range_" + tag]).to(device)
    return model


def golden_input_grads(g, tag, model, device):
    """(mask, fft.grad, cfar.grad or None) of loss = sum(mask * gsel) with the golden leaves, fed as the generator feeds them."""
    fft = torch.from_numpy(g["x_" + tag]).to(device).requires_grad_(True)
    cfar = torch.from_numpy(g["cfar_" + tag]).to(device).requires_grad_(True)
    B = fft.shape[0]
    scan = {"fft_data": fft.clone(), "fft_cfar": cfar.clone(), "raw_pc": torch.zeros(B, 4, 3)}
    m = model(scan, {"pc": torch.zeros(B, 4, 6)}, None, mask_only=True)
    (m * torch.from_numpy(g["gsel_" + tag]).to(device)).sum().backward()
    return m.detach(), fft.grad, cfar.grad


def normalize_channels(x, mode):
    """LearnICPWeightPolicy._normalize_channels (the out-of-place restatement the existing goldens pin to the reference's
    forward) without a module: mode "minmax" | "standardize" | "none"."""
    stub = type("S", (), {"normalize_type": [mode], "global_minmax": False})()
    return LearnICPWeightPolicy._normalize_channels(stub, x)


def first_layer_input_grad_ref(gz, w, x=None, mode="none"):
    """fp64 CPU definition: d/dx of sum(conv2d(round-free normalise(x), w, padding=1) * gz); gz (B,H,W,8), w (8,cin,3,3),
    x (B,cin,H,W) (only its shape matters when mode is "none").  The bf16 rounding of the input is straight-through."""
    gz = gz.detach().double().cpu().permute(0, 3, 1, 2).contiguous()
    w = w.detach().double().cpu()
    B, _, H, W = gz.shape
    if mode == "none":
        return torch.nn.grad.conv2d_input((B, w.shape[1], H, W), w, gz, padding=1)
    xd = x.detach().double().cpu().requires_grad_(True)
    y = torch.nn.functional.conv2d(normalize_channels(xd, mode), w, padding=1)
    (y * gz).sum().backward()
    return xd.grad
