"""Timing of the polar-aware sampler (mmk_sample_weights_polar_fwd / _bwd / _bwd_pc) next to the Cartesian one
(mmk_sample_weights_fwd / _bwd / _bwd_pc) at the bench shape (B = 32, N = 5 120 points, polar mask 400 x 3360, Cartesian mask
640 x 640; the Cartesian sampler is also timed on the polar mask, which is what a polar network runs without
params["polar_sampling"]), and of one training step of the polar network with the flag off and on.  The flag-off step cannot
form the map-point BCE term (its target is 640 x 640), so the two steps that are compared run with that term's weight at 0; the
flag-on step with the default weights (the term at 1, its target from polar_target_from_pts) is reported beside them.  Device
events around repeated calls after a warm-up; the variants alternate within one run and the median over the rounds is reported
with the spread.  There is no target: the Cartesian launches and the flag-off step are the yardsticks.  Development tool (GPU
box); prints one JSON line.

    python scripts/bench_polar_weights.py [--batch 32] [--points 5120] [--rounds 7] [--reps 20] [--step-batch 8] [--out FILE]
"""
import argparse
import json
import math
import sys

sys.path.insert(0, ".")
import torch  # noqa: E402

from mm_masking_amd import _lib, synthetic  # noqa: E402
from mm_masking_amd import train_icp_weights as trn  # noqa: E402
from mm_masking_amd.icp_weight_policy import LearnICPWeightPolicy  # noqa: E402
from scripts.bench_mask_scan import alternate  # noqa: E402

RES = 0.0596


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--points", type=int, default=5120)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--step-batch", type=int, default=8)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_polar_weights needs a HIP device: a CPU run cannot give a time")
    dev = torch.device("cuda:0")
    B, N, A, R, H = args.batch, args.points, 400, 3360, 640
    g = torch.Generator().manual_seed(1)
    polar, cart = torch.rand(B, A, R, generator=g).to(dev), torch.rand(B, H, H, generator=g).to(dev)
    # a scan cloud: ranges over the detector's 2 .. 80 m, any bearing, the last fifth of the rows zero padding
    rng = 2.0 + 78.0 * torch.rand(B, N, generator=g)
    ang = 2 * math.pi * torch.rand(B, N, generator=g)
    pc = torch.stack([rng * torch.cos(ang), rng * torch.sin(ang), torch.zeros(B, N)], dim=-1)
    pc[:, N - N // 5:] = 0.0
    pc = pc.to(dev).contiguous()
    gw = torch.randn(B, N, generator=g).to(dev)
    az = ((torch.arange(A, dtype=torch.float64) + 0.5 + 0.4 * (torch.rand(B, A, generator=g, dtype=torch.float64) - 0.5))
          * (2 * math.pi / A)).float().to(dev).contiguous()
    L, st, p = _lib.lib(), _lib.stream_ptr(dev), _lib.ptr
    w = torch.empty(B, N, device=dev)
    gpc = torch.empty_like(pc)
    g_polar, g_cart = torch.empty_like(polar), torch.empty_like(cart)
    nb = int(L.mmk_sample_weights_polar_bwd_ws_bytes(B, N))
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)

    def cartesian(mask, gmask):
        h, wd = mask.shape[1:]
        return {"fwd": lambda: _lib.check(L.mmk_sample_weights_fwd(p(mask), p(pc), B, N, 3, h, wd, 640, 0.2384, p(w), st)),
                "bwd_mask": lambda: _lib.check(L.mmk_sample_weights_bwd(p(gw), p(pc), B, N, 3, h, wd, 640, 0.2384, p(gmask), p(ws),
                                                                        nb, st)),
                "bwd_pc": lambda: _lib.check(L.mmk_sample_weights_bwd_pc(p(gw), p(mask), p(pc), B, N, 3, h, wd, 640, 0.2384, p(gpc),
                                                                         st))}

    polar_calls = {
        "fwd": lambda: _lib.check(L.mmk_sample_weights_polar_fwd(p(polar), p(pc), p(az), B, N, 3, A, R, RES, 1, 1, p(w), st)),
        "bwd_mask": lambda: _lib.check(L.mmk_sample_weights_polar_bwd(p(gw), p(pc), p(az), B, N, 3, A, R, RES, 1, 1, p(g_polar),
                                                                      p(ws), nb, st)),
        "bwd_pc": lambda: _lib.check(L.mmk_sample_weights_polar_bwd_pc(p(gw), p(polar), p(pc), p(az), B, N, 3, A, R, RES, 1, 1,
                                                                       p(gpc), st))}
    variants = {"polar_" + k: f for k, f in polar_calls.items()}
    variants.update({"cartesian_640_" + k: f for k, f in cartesian(cart, g_cart).items()})
    variants.update({"cartesian_on_polar_" + k: f for k, f in cartesian(polar, g_polar).items()})
    res = {"shape": {"B": B, "N": N, "A": A, "R": R, "H": H, "W": H},
           "note": "bwd_mask = zero fill of the gradient image + link + sum + store; ms per call: median, min, max",
           "launch_ms": alternate(variants, args.rounds, args.reps)}
    del polar, cart, g_polar, g_cart, ws
    torch.cuda.empty_cache()

    Bs = args.step_batch
    raw = synthetic.make_batch(list(range(Bs)), device=dev)
    steps = {}
    for name, flag, pts_weight in (("flag_off_no_map_pts_term", False, 0.0), ("flag_on_no_map_pts_term", True, 0.0),
                                   ("flag_on_default_loss", True, 1.0)):
        params = trn.default_params(dev)
        params.update({"network_input_type": "polar", "network_output_type": "polar", "loss_map_pts_mask_weight": pts_weight})
        if flag:
            params["polar_sampling"] = True
        batch = trn.prepare_batch(raw, params)
        torch.manual_seed(0)
        model = LearnICPWeightPolicy(params).to(dev)
        opt = trn.make_optimizer(model, params)
        model.train()
        steps[name] = (lambda model=model, batch=batch, opt=opt, params=params:
                       trn.train_step(model, batch, opt, trn.loss_weights_from(params), dev))
    res["train_step_ms"] = {"B": Bs, **alternate(steps, args.rounds, max(1, args.reps // 6))}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
