"""Timing of the dICP with its robust scale, trim distance and steepness as device tensors that require grad
(mmk_icp_forward_hp / mmk_icp_backward_hp, three more fp64 block reductions per point block and a final ordered sum) next to
the same calls with floats (mmk_icp_forward / mmk_icp_backward[_points]), at the sizes of BASELINE.json configs[2] (B = 32
synthetic pairs, N = 5 120 padded scan points, the padded map, dim 2, pt2pl Huber, 10 iterations, the tanh gate): the forward
+ backward of one ICP call with weight and T_init requiring grad and with the clouds requiring grad as well, shared () and
per-pair (B,) tensors, and one training step of the policy (the benchmark's step, params["icp_trim"] = "tanh") with and
without params["learn_icp"].  Device events around repeated calls after a warm-up; the variants alternate within one run and
the median over the rounds is reported with the spread.  There is no target: the float call is the yardstick.  bench.py
measures the default step only.  Development tool (GPU box); prints one JSON line.

    python scripts/bench_icp_hyper.py [--batch 32] [--rounds 7] [--reps 10] [--step-batch 8] [--out FILE]
"""
import argparse
import json
import sys

sys.path.insert(0, ".")
import torch  # noqa: E402

from mm_masking_amd import synthetic  # noqa: E402
from mm_masking_amd import train_icp_weights as trn  # noqa: E402
from mm_masking_amd.dICP.ICP import ICP, check_errors  # noqa: E402
from mm_masking_amd.icp_weight_policy import LearnICPWeightPolicy  # noqa: E402
from scripts.bench_mask_scan import alternate  # noqa: E402

LEARN = ("metric", "trim_dist", "tanh_steepness")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--step-batch", type=int, default=8)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_icp_hyper needs a HIP device: a CPU run cannot give a time")
    dev = torch.device("cuda:0")
    B = args.batch
    params = trn.default_params(dev)
    raw = synthetic.make_batch(list(range(B)), device=dev)
    batch = trn.prepare_batch(raw, params)
    src, tgt, T0 = batch["loc_data"]["filtered_pc"].contiguous(), raw["map_pc"].contiguous(), raw["T_init"].contiguous()
    g = torch.Generator().manual_seed(1)
    w = (0.2 + 0.8 * torch.rand(B, src.shape[1], generator=g)).to(dev)
    G = torch.randn(B, 4, 4, generator=g).to(dev)
    k, trim, steep = 1.0, 5.0, 10.0

    def icp_call(kind, clouds):
        icp = ICP("pt2pl", differentiable=True, max_iterations=10, tolerance=1e-5)
        icp.trim = "tanh"
        if kind == "float":
            h = [k, trim, steep]
        else:
            shape = () if kind == "shared" else (B,)
            h = [torch.full(shape, v, dtype=torch.float32, device=dev, requires_grad=True) for v in (k, trim, steep)]
        icp.tanh_steepness = h[2]
        s, t = src.clone().requires_grad_(clouds), tgt.clone().requires_grad_(clouds)
        wg, Tg = w.clone().requires_grad_(True), T0.clone().requires_grad_(True)

        def run():
            s.grad = t.grad = wg.grad = Tg.grad = None
            for v in h:
                if isinstance(v, torch.Tensor):
                    v.grad = None
            T = icp.icp(s, t, T_init=Tg, weight=wg, trim_dist=h[1], loss_fn={"name": "huber", "metric": h[0]}, dim=2)["T"]
            (T * G).sum().backward()
        return run

    variants = {"%s_%s" % (kind, "points" if clouds else "weights"): icp_call(kind, clouds)
                for clouds in (False, True) for kind in ("float", "shared", "per_pair")}
    res = {"shape": {"B": B, "N": int(src.shape[1]), "M": int(tgt.shape[1]), "dim": 2, "icp_type": "pt2pl", "loss": "huber",
                     "iterations": 10, "trim": "tanh", "metric": k, "trim_dist": trim, "steepness": steep},
           "note": "ms per call: median, min, max; float_*: the older entries, shared_* / per_pair_*: the _hp entries with the "
                   "three values as () / (B,) tensors requiring grad; *_weights: no cloud requires grad, *_points: both do",
           "icp_forward_backward_ms": alternate(variants, args.rounds, args.reps)}
    del variants
    torch.cuda.empty_cache()

    Bs = args.step_batch
    raw = synthetic.make_batch(list(range(Bs)), device=dev)
    steps = {}
    for name, learn in (("float", ()), ("learn_icp", LEARN)):
        params = trn.default_params(dev)
        params.update({"icp_trim": "tanh", "learn_icp": learn})
        batch = trn.prepare_batch(raw, params)
        torch.manual_seed(0)
        model = LearnICPWeightPolicy(params).to(dev)
        opt = trn.make_optimizer(model, params)
        model.train()
        steps[name] = (lambda model=model, batch=batch, opt=opt, params=params:
                       trn.train_step(model, batch, opt, trn.loss_weights_from(params), dev))
    res["train_step_ms"] = {"B": Bs, **alternate(steps, args.rounds, max(1, args.reps // 3))}
    check_errors(wait=True)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
