"""Diagnostic: relative error of every parameter gradient of test_unet_hip_backward_exact_on_pinned_activations' (3, 64, 160, 0.05) case
over several dropout seeds -- is one tensor's 4.5 % the noise of a near-cancelling 16-element sum, or a kernel's bug?
   python scripts/diag_pinned_bias.py [tensor name ...]      (default: encoder.1.2.bias)
For each named tensor and seed: the relative error, its component along the reference gradient (a wrong scale shows there), and for
weight tensors the relative error per tap (a wrong tap or halo shows there).  The last line is the same shape without dropout."""
import sys
import torch
sys.path.insert(0, "."); sys.path.insert(0, "tests")
from mm_masking_amd import unet_hip as uh
import test_gpu_unet_kernels as T
from support import DEV, policy
B, H, W = 3, 64, 160
watch = sys.argv[1:] or ["encoder.1.2.bias"]


def run(drop, seed):
    model = policy(DEV, 11, dropout=drop, amp_dtype=torch.float32, unet_backend="torch")
    model.train()
    g = torch.Generator().manual_seed(1)
    x = torch.rand(B, 1, H, W, generator=g).to(DEV)
    gsel = torch.randn(B, H, W, generator=g).to(DEV)
    uh.DEBUG = {}
    try:
        out = uh.unet_mask(model, x, training=True, seed=seed)
        (out * gsel).sum().backward()
        fwd = uh.DEBUG["fwd"]
    finally:
        uh.DEBUG = None
    got = [p.grad.clone() for p in uh.param_list(model)]
    model.zero_grad()
    ref = T._unet_on_hip_activations(model, x, fwd, drop)
    (ref * gsel).sum().backward()
    names = [n for n, _ in model.named_parameters()]
    pairs = {n: (a, p.grad) for n, a, p in zip(names, got, uh.param_list(model))}
    rels = {n: ((a - r).norm() / (r.norm() + 1e-12)).item() for n, (a, r) in pairs.items()}
    worst_w = max((v, n) for n, v in rels.items() if pairs[n][1].ndim == 4)
    worst_b = max((v, n) for n, v in rels.items() if pairs[n][1].ndim != 4)
    print("drop %.2f seed %d  out err %.1e  worst weight %s %.4f  worst bias %s %.4f" % (
        drop, seed, (out - ref).abs().max().item(), worst_w[1], worst_w[0], worst_b[1], worst_b[0]), flush=True)
    for n in watch:
        a, r = pairs[n]
        e = a - r
        line = "    %-20s rel %.4f  along the reference %+.4f  |grad| %.3e" % (n, rels[n], ((e * r).sum() / (r * r).sum()).item(), r.norm().item())
        if r.ndim == 4 and r.shape[2] == 3:
            line += "  per tap " + " ".join("%.3f" % (e[:, :, i, j].norm() / (r[:, :, i, j].norm() + 1e-12)).item()
                                          for i in range(3) for j in range(3))
        print(line, flush=True)


for seed in range(1, 9):
    run(0.05, seed)
run(0.0, 1)
