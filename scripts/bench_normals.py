"""Timing of the target-normal estimator (dICP.estimate_normals = mmk_knn_normals: grid build + knn_normals_kernel) at
the training batch (B = 32 synthetic.make_batch maps, M = 20 480 rows of which 20 000 valid, k = 16, dim 2 and dim 3) and
on one 100 000-point cloud, beside the same result formed on the same device from torch.cdist + topk + torch.linalg.eigh
(fp64 covariance of the gathered neighbours; query rows in chunks, since a (B,M,M) distance matrix does not fit).  Device
events around repeated calls after a warm-up; median over the rounds with the spread.  The two forms' normals are compared
up to sign before anything is timed.  Development tool (GPU box); prints one JSON line.

    python scripts/bench_normals.py [--batch 32] [--rounds 5] [--reps 3] [--composed-rounds 2] [--out FILE]
"""
import argparse
import json
import statistics
import sys

sys.path.insert(0, ".")
sys.path.insert(0, "scripts")
import torch  # noqa: E402

from bench_mask_scan import timed  # noqa: E402
from mm_masking_amd import dICP, synthetic  # noqa: E402

PAD = 1000.0


def composed(points, k, dim, pad_val, chunk_elems=1 << 26):
    """(B,M,3) normals from library calls alone: per pair and chunk of query rows, cdist -> topk -> gather -> fp64
    covariance -> eigh -> smallest eigenvector, turned to the origin; zero for padding rows."""
    B, M, _ = points.shape
    out = torch.zeros(B, M, 3, dtype=torch.float32, device=points.device)
    step = max(1, chunk_elems // M)
    for b in range(B):
        x = points[b, :, :dim]
        pad = (x.abs() >= pad_val).any(dim=1)
        for r0 in range(0, M, step):
            q = x[r0:r0 + step]
            d = torch.cdist(q, x)
            d[:, pad] = float("inf")
            idx = torch.topk(d, k, dim=1, largest=False).indices
            nb = x[idx].double()                                    # (rows, k, dim)
            c = nb - nb.mean(dim=1, keepdim=True)
            cov = c.transpose(1, 2) @ c / k
            vec = torch.linalg.eigh(cov).eigenvectors[:, :, 0]      # ascending eigenvalues
            flip = (vec * -q.double()).sum(dim=1) < 0
            vec = torch.where(flip[:, None], -vec, vec)
            vec[pad[r0:r0 + step]] = 0
            out[b, r0:r0 + step, :dim] = vec.float()
    return out


def measure(fn, rounds, reps):
    fn()
    torch.cuda.synchronize()
    t = [timed(fn, reps) for _ in range(rounds)]
    return (statistics.median(t), min(t), max(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--composed-rounds", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_normals needs a HIP device: a CPU run cannot give a time")
    dev = torch.device("cuda:0")
    res = {"k": 16, "cases": {}}
    cases = [("batch_dim2", dict(indices=range(args.batch), m_valid=20000, m_pad=20480, dim=2), 2),
             ("batch_dim3", dict(indices=range(args.batch), m_valid=20000, m_pad=20480, dim=3), 3),
             ("cloud_100k_dim3", dict(indices=[0], m_valid=100000, m_pad=100000, dim=3), 3)]
    for name, kw, dim in cases:
        pts = synthetic.make_batch(list(kw.pop("indices")), **kw)["map_pc"][:, :, :3].contiguous().to(dev)
        B, M, _ = pts.shape
        n_k = dICP.estimate_normals(pts, k=16, dim=dim, pad_val=PAD)
        n_c = composed(pts, 16, dim, PAD)
        # same line wherever the answer is well-posed (near-ties in distance or eigenvalue may differ: counted, not hidden)
        dots = (n_k * n_c).sum(dim=2).abs()
        valid = (pts[:, :, :dim].abs() < PAD).all(dim=2)
        agree = float((dots[valid] > 0.9999).float().mean())
        kern = measure(lambda: dICP.estimate_normals(pts, k=16, dim=dim, pad_val=PAD), args.rounds, args.reps)
        comp = measure(lambda: composed(pts, 16, dim, PAD), args.composed_rounds, 1)
        res["cases"][name] = {"B": B, "M": M, "dim": dim, "kernel_ms": kern, "composed_ms": comp,
                              "composed_over_kernel": comp[0] / kern[0], "rows_agreeing": agree,
                              "points_per_s_kernel": B * M / (kern[0] * 1e-3)}
        print(name, json.dumps(res["cases"][name]), flush=True)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
