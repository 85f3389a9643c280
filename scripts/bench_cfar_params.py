"""Timing of the CFAR backward with threshold gradients, mmk_cfar_mask_bwd_p (scan gradient + both threshold gradients, and
the thresholds alone: grad_raw = NULL), against the by-value mmk_cfar_mask_bwd at the bench shape (B = 32, 400 x 3360), and of
the two forwards.  The C entries are called directly; device events around repeated calls after a warm-up; the variants
alternate within one run and the median over the rounds is reported with the spread.  Development tool (GPU box); prints one
JSON line.

    python scripts/bench_cfar_params.py [--batch 32] [--rounds 7] [--reps 10] [--per-scan] [--out FILE]
"""
import argparse
import json
import sys

sys.path.insert(0, ".")
sys.path.insert(0, "scripts")
import torch  # noqa: E402

from bench_mask_scan import alternate  # noqa: E402
from mm_masking_amd import _lib  # noqa: E402
from mm_masking_amd import radar_utils as ru  # noqa: E402

RES = 0.0596


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--per-scan", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_cfar_params needs a HIP device: a CPU run cannot give a time")
    dev = torch.device("cuda:0")
    B, A, R = args.batch, 400, 3360
    g = torch.Generator().manual_seed(1)
    raw = 0.04 * torch.rand(B, A, R, generator=g)
    raw[:, :, 150:3000:37] += 0.1 + 0.3 * torch.rand(B, A, len(range(150, 3000, 37)), generator=g)
    raw, G = raw.to(dev), torch.randn(B, A, R, generator=g).to(dev)
    w2, mincol, maxcol = ru.cfar_cols(R, RES)
    guard, a_th, b_th, steep = 5, 1.0, 0.09, 10.0
    n = B if args.per_scan else 1
    a, b = torch.full((n,), a_th, device=dev), torch.full((n,), b_th, device=dev)
    ga, gb = torch.empty_like(a), torch.empty_like(b)
    gx, gx_p, mask, mask_p = (torch.empty_like(raw) for _ in range(4))
    L = _lib.lib()
    ws = torch.empty(int(L.mmk_cfar_mask_bwd_p_ws_bytes(B, A)), dtype=torch.uint8, device=dev)
    st, p = _lib.stream_ptr(dev), _lib.ptr

    def fwd_value():
        _lib.check(L.mmk_cfar_mask(p(raw), B, A, R, w2, guard, mincol, maxcol, a_th, b_th, 1, steep, p(mask), st))

    def fwd_pointer():
        _lib.check(L.mmk_cfar_mask_p(p(raw), B, A, R, w2, guard, mincol, maxcol, p(a), p(b), int(args.per_scan), 1, steep, p(mask_p), st))

    def bwd_value():
        _lib.check(L.mmk_cfar_mask_bwd(p(raw), p(G), B, A, R, w2, guard, mincol, maxcol, a_th, b_th, steep, p(gx), st))

    def bwd_pointer(out):
        def run():
            _lib.check(L.mmk_cfar_mask_bwd_p(p(raw), p(G), B, A, R, w2, guard, mincol, maxcol, p(a), p(b), int(args.per_scan), steep,
                                             p(out), p(ga), p(gb), p(ws), ws.numel(), st))
        return run

    fwd_value(), fwd_pointer(), bwd_value(), bwd_pointer(gx_p)()
    assert torch.equal(mask, mask_p) and torch.equal(gx, gx_p)
    full = (ga.clone(), gb.clone())
    bwd_pointer(None)()
    assert torch.equal(full[0], ga) and torch.equal(full[1], gb)

    res = {"shape": {"B": B, "A": A, "R": R, "per_scan": bool(args.per_scan)},
           "grad_a": full[0].flatten()[0].item(), "grad_b": full[1].flatten()[0].item(),
           "forward_ms": alternate({"by_value": fwd_value, "pointer": fwd_pointer}, args.rounds, args.reps),
           "backward_ms": alternate({"by_value": bwd_value, "pointer_all": bwd_pointer(gx_p), "pointer_thresholds_only": bwd_pointer(None)},
                                    args.rounds, args.reps)}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
