"""Per level of the encoder at the benchmark's shapes (B = 32, 640 x 640 input): the backward of the block's second convolution
with the pooling adjoint inside its consumers against the standalone mmk_maxpool2_bwd_arg launch followed by the plain
consumers -- one stream, HIP events around REPS alternating repetitions of either sequence, median per sequence.  The levels
whose pooled form is faster are the driver's POOL_ADJOINT_LEVELS (csrc/mmk_unet_driver.hip).
   python scripts/bench_pool_adjoint_levels.py [out.txt]"""
import os, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mm_masking_amd import unet_hip as uh

DEV = torch.device("cuda:0")
B, REPS, S = 32, 41, 1.0 / 0.95
lines = []
for lvl, (C, H) in enumerate([(16, 640), (32, 320), (64, 160), (128, 80), (256, 40)], start=1):
    g = torch.Generator().manual_seed(lvl)
    x = (torch.randn(B, H, H, C, generator=g) * 0.7).clamp_min(0).to(torch.bfloat16).to(DEV)
    pre = torch.randn(B, H, H, C, generator=g).clamp_min(0).to(torch.bfloat16).to(DEV)
    _, arg = uh.maxpool2_arg(pre)
    del pre
    gy = (torch.randn(B, H // 2, H // 2, C, generator=g) * 0.3).to(torch.bfloat16).to(DEV)
    w = (torch.randn(C, C, 3, 3, generator=g) / (3 * C ** 0.5)).to(DEV)
    wpt = uh.pack_weights(w, transposed=True)
    ns = uh.wgrad_slices(C, C, C, B, H, H)
    part, dx = uh.partial_buffer(ns, C, C, DEV), torch.empty_like(x)
    gz = torch.empty_like(x)

    def alone():
        uh._lib.check(uh._lib.lib().mmk_maxpool2_bwd_arg(uh._p(arg), uh._p(gy), B, H, H, C, S, uh._p(gz), uh._sp(DEV)))
        if C == 16:
            uh.conv_bwd_fused(x, gz, wpt, 1.0, dx, part)
        else:
            uh.conv3x3_wgrad_partial(x, gz, C, part)
            uh.conv3x3(gz, wpt, C, out=dx, relu_src=x, scale=1.0)

    def pooled():
        if C == 16:
            uh.conv_bwd_fused(x, gy, wpt, 1.0, dx, part, g_pool_arg=arg, g_pool_scale=S)
        else:
            uh.conv3x3_wgrad_partial(x, gy, C, part, g_pool_arg=arg, g_pool_scale=S)
            uh.conv3x3(gy, wpt, C, out=dx, relu_src=x, scale=1.0, x1_pool_arg=arg, x1_pool_scale=S, hw=(H, H))

    t = {"alone": [], "pooled": []}
    for r in range(REPS + 4):
        for name, fn in (("alone", alone), ("pooled", pooled)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record(); e1.synchronize()
            if r >= 4:
                t[name].append(e0.elapsed_time(e1) * 1e3)
    med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
    q = {k: (sorted(v)[len(v) // 4], sorted(v)[3 * len(v) // 4]) for k, v in t.items()}
    lines.append("enc%d  %3d ch @ %3d^2   standalone launch + consumers %7.1f us (quartiles %.1f-%.1f)   pooled consumers %7.1f us (%.1f-%.1f)   %+6.1f us  %s"
                 % (lvl, C, H, med["alone"], *q["alone"], med["pooled"], *q["pooled"], med["pooled"] - med["alone"],
                    "pooled wins" if med["pooled"] < med["alone"] else "standalone wins"))
    del x, gy, gz, dx, part
    torch.cuda.empty_cache()
head = "B = %d, median of %d alternating repetitions, HIP events, one stream, dropout factor 1/0.95" % (B, REPS)
print("\n".join([head] + lines))
if len(sys.argv) > 1:
    open(sys.argv[1], "w").write("\n".join([head] + lines) + "\n")
