"""Timing of the dICP with the soft (tanh) trim gate (parameters.trim: tanh; mmk_icp_params.trim_steep > 0) next to the hard
gate, at the sizes of BASELINE.json configs[2] (B = 32 synthetic pairs, N = 5 120 padded scan points, the padded map, dim 2,
pt2pl Huber, 10 iterations): the forward + backward of one ICP call with weight and T_init requiring grad (mmk_icp_backward)
and with the clouds requiring grad as well (mmk_icp_backward_points), and one training step of the policy's scan mode
(params["mask_target"] = "scan") with params["icp_trim"] "hard" and "tanh".  Device events around repeated calls after a
warm-up; the variants alternate within one run and the median over the rounds is reported with the spread.  There is no
target: the hard gate is the yardstick.  bench.py measures the default step only.  Development tool (GPU box); prints one JSON
line.

    python scripts/bench_soft_trim.py [--batch 32] [--rounds 7] [--reps 10] [--step-batch 8] [--steepness 10] [--out FILE]
"""
import argparse
import json
import sys

sys.path.insert(0, ".")
import torch  # noqa: E402

from mm_masking_amd import synthetic  # noqa: E402
from mm_masking_amd import train_icp_weights as trn  # noqa: E402
from mm_masking_amd.dICP.ICP import ICP  # noqa: E402
from mm_masking_amd.icp_weight_policy import LearnICPWeightPolicy  # noqa: E402
from scripts.bench_mask_scan import alternate  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--step-batch", type=int, default=8)
    ap.add_argument("--steepness", type=float, default=10.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_soft_trim needs a HIP device: a CPU run cannot give a time")
    dev = torch.device("cuda:0")
    B = args.batch
    params = trn.default_params(dev)
    raw = synthetic.make_batch(list(range(B)), device=dev)
    batch = trn.prepare_batch(raw, params)
    src, tgt, T0 = batch["loc_data"]["filtered_pc"].contiguous(), raw["map_pc"].contiguous(), raw["T_init"].contiguous()
    g = torch.Generator().manual_seed(1)
    w = (0.2 + 0.8 * torch.rand(B, src.shape[1], generator=g)).to(dev)
    G = torch.randn(B, 4, 4, generator=g).to(dev)
    loss_fn = {"name": "huber", "metric": 1.0}

    def icp_call(trim, clouds):
        icp = ICP("pt2pl", differentiable=True, max_iterations=10, tolerance=1e-5)
        icp.trim, icp.tanh_steepness = trim, args.steepness
        s, t = src.clone().requires_grad_(clouds), tgt.clone().requires_grad_(clouds)
        wg, Tg = w.clone().requires_grad_(True), T0.clone().requires_grad_(True)

        def run():
            s.grad = t.grad = wg.grad = Tg.grad = None
            T = icp.icp(s, t, T_init=Tg, weight=wg, trim_dist=5.0, loss_fn=loss_fn, dim=2)["T"]
            (T * G).sum().backward()
        return run

    variants = {"%s_%s" % (trim, "points" if clouds else "weights"): icp_call(trim, clouds)
                for clouds in (False, True) for trim in ("hard", "tanh")}
    res = {"shape": {"B": B, "N": int(src.shape[1]), "M": int(tgt.shape[1]), "dim": 2, "icp_type": "pt2pl", "loss": "huber",
                     "iterations": 10, "trim_dist": 5.0, "steepness": args.steepness},
           "note": "ms per call: median, min, max; *_weights: mmk_icp_backward, *_points: mmk_icp_backward_points",
           "icp_forward_backward_ms": alternate(variants, args.rounds, args.reps)}
    del variants
    torch.cuda.empty_cache()

    Bs = args.step_batch
    raw = synthetic.make_batch(list(range(Bs)), device=dev)
    steps = {}
    for trim in ("hard", "tanh"):
        params = trn.default_params(dev)
        params.update({"mask_target": "scan", "icp_trim": trim, "icp_tanh_steepness": args.steepness})
        batch = trn.prepare_batch(raw, params)
        torch.manual_seed(0)
        model = LearnICPWeightPolicy(params).to(dev)
        opt = trn.make_optimizer(model, params)
        model.train()
        steps[trim] = (lambda model=model, batch=batch, opt=opt, params=params:
                       trn.train_step(model, batch, opt, trn.loss_weights_from(params), dev))
    res["scan_mode_train_step_ms"] = {"B": Bs, **alternate(steps, args.rounds, max(1, args.reps // 3))}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
