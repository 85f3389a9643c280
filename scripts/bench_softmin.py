"""Timing of the dICP with soft correspondences (parameters.correspondence: softmin; mmk_icp_forward_soft /
mmk_icp_backward_soft) next to nearest correspondences, at the sizes of BASELINE.json configs[2] (B = 32 synthetic pairs,
N = 5 120 padded scan points, the padded map, dim 2, pt2pl Huber, 10 iterations), for k = 4 and 8: the forward + backward of
one ICP call with weight and T_init requiring grad and with the clouds requiring grad as well, the k-NN launch of one
iteration (the library's own event pairs, mmk_nn_profile_begin / _end) next to the grid engine's single-neighbour launch, and
one default training step of the policy with params["icp_correspondence"] "nearest" and "softmin".  Device events around
repeated calls after a warm-up; the variants alternate within one run and the median over the rounds is reported with the
spread.  There is no target: the default step (nearest, the parent's arithmetic) in the same run is the yardstick.  bench.py
measures the default step only.  --temp-tensor adds, next to every soft-min variant, the same call with the temperature as a
device tensor that requires grad (mmk_icp_forward_soft_t / mmk_icp_backward_soft_t, names ending in _tau) and the training
step with params["learn_icp"] = ("softmin_temp",); without the flag the run is the one it always was.  Development tool
(GPU box); prints one JSON line.

    python scripts/bench_softmin.py [--batch 32] [--rounds 7] [--reps 10] [--step-batch 32] [--temp 0.25] [--temp-tensor]
                                    [--out FILE]
"""
import argparse
import ctypes
import json
import statistics
import sys

sys.path.insert(0, ".")
import torch  # noqa: E402

from mm_masking_amd import _lib, synthetic  # noqa: E402
from mm_masking_amd import train_icp_weights as trn  # noqa: E402
from mm_masking_amd.dICP.ICP import ICP  # noqa: E402
from mm_masking_amd.icp_weight_policy import LearnICPWeightPolicy  # noqa: E402
from scripts.bench_mask_scan import alternate  # noqa: E402

KS = (4, 8)


def nn_launch_ms(run, launches):
    """Median (and spread) of the search launches the library brackets during ``run()``, in ms."""
    L = _lib.lib()
    run()
    torch.cuda.synchronize()
    _lib.check(L.mmk_nn_profile_begin(launches))
    run()
    torch.cuda.synchronize()
    out = (ctypes.c_float * launches)()
    n = ctypes.c_int32(0)
    _lib.check(L.mmk_nn_profile_end(out, launches, ctypes.byref(n)))
    ms = sorted(out[i] for i in range(min(n.value, launches)))
    return {"launches": n.value, "median": statistics.median(ms), "min": ms[0], "max": ms[-1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--step-batch", type=int, default=32)
    ap.add_argument("--temp", type=float, default=0.25)
    ap.add_argument("--temp-tensor", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_softmin needs a HIP device: a CPU run cannot give a time")
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

    def icp_call(k, clouds, engine="brute", backward=True, tau=False):
        icp = ICP("pt2pl", differentiable=True, max_iterations=10, tolerance=1e-5)
        icp.nn_search = engine
        temp = torch.tensor(args.temp, device=dev, requires_grad=True) if tau else args.temp
        if k:
            icp.correspondence, icp.softmin_k, icp.softmin_temp = "softmin", k, temp
        s, t = src.clone().requires_grad_(clouds), tgt.clone().requires_grad_(clouds)
        wg, Tg = w.clone().requires_grad_(True), T0.clone().requires_grad_(True)

        def run():
            s.grad = t.grad = wg.grad = Tg.grad = None
            if tau:
                temp.grad = None
            T = icp.icp(s, t, T_init=Tg, weight=wg, trim_dist=5.0, loss_fn=loss_fn, dim=2)["T"]
            if backward:
                (T * G).sum().backward()
        return run

    def name(k, engine="brute"):
        return "softmin_k%d" % k if k else "nearest_" + engine

    variants = {}
    for clouds in (False, True):
        for k, engine in ((0, "brute"), (0, "grid")) + tuple((k, "grid") for k in KS):
            variants["%s_%s" % (name(k, engine), "points" if clouds else "weights")] = icp_call(k, clouds, engine)
            if k and args.temp_tensor:
                variants["%s_%s_tau" % (name(k, engine), "points" if clouds else "weights")] = icp_call(k, clouds, engine, tau=True)
    res = {"shape": {"B": B, "N": int(src.shape[1]), "M": int(tgt.shape[1]), "dim": 2, "icp_type": "pt2pl", "loss": "huber",
                     "iterations": 10, "trim_dist": 5.0, "temp": args.temp},
           "note": "ms: median, min, max; *_weights: no cloud gradients, *_points: source and target gradients as well; "
                   "*_tau: the temperature a device tensor that requires grad",
           "icp_forward_backward_ms": alternate(variants, args.rounds, args.reps)}
    del variants
    res["search_launch_ms"] = {name(k, "grid"): nn_launch_ms(icp_call(k, False, "grid", backward=False), 10) for k in (0,) + KS}
    torch.cuda.empty_cache()

    Bs = args.step_batch
    raw = synthetic.make_batch(list(range(Bs)), device=dev)
    steps = {}
    for k, learn in [(k, False) for k in (0,) + KS] + [(k, True) for k in KS if args.temp_tensor]:
        params = trn.default_params(dev)
        if k:
            params.update({"icp_correspondence": "softmin", "icp_softmin_k": k, "icp_softmin_temp": args.temp})
        if learn:
            params["learn_icp"] = ("softmin_temp",)
        batch = trn.prepare_batch(raw, params)
        torch.manual_seed(0)
        model = LearnICPWeightPolicy(params).to(dev)
        opt = trn.make_optimizer(model, params)
        model.train()
        steps[("softmin_k%d" % k if k else "nearest") + ("_tau" if learn else "")] = (lambda model=model, batch=batch, opt=opt, params=params:
                                                        trn.train_step(model, batch, opt, trn.loss_weights_from(params), dev))
    res["default_train_step_ms"] = {"B": Bs, **alternate(steps, args.rounds, max(1, args.reps // 3))}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
