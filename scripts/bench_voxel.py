"""Timing of the voxel filter (dICP.voxel_downsample = mmk_voxel_downsample: insert, leaders, accumulate, finalise) at
the training batch (B = 32 synthetic.make_batch maps, M = 20 480 rows of which 20 000 valid, xyz | normal) and on one map
of 2^20 rows, at voxels of 0.1, 0.3 and 1.0 m (dim 3, centroids, normals re-normalised), beside the same result formed
on the same device from torch calls: packed int64 keys, torch.unique(return_inverse=True), index_add_ in fp64, a division
and the re-normalisation (its rows come out in key order, not in the order of first appearance, and its sums depend on the
arrival order).  Device events around repeated calls after a warm-up; median over the rounds with the spread.  The two
forms' cell counts and centroids are compared before anything is timed.  Development tool (GPU box); prints one JSON line.

    python scripts/bench_voxel.py [--batch 32] [--rounds 5] [--reps 5] [--out FILE]
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
SPAN = (1 << 21) + 1


def keys_of(points, voxel, dim=3):
    """(valid (B,M) bool, packed cell keys (B,M) int64) with the kernel's cell rule: floor of the fp32 product."""
    inv = torch.tensor(1.0 / float(torch.tensor(voxel, dtype=torch.float32)), dtype=torch.float32, device=points.device)
    valid = torch.isfinite(points).all(dim=2) & (points[:, :, :dim].abs() < PAD).all(dim=2)
    cell = torch.floor(points[:, :, :dim] * inv).to(torch.int64) + (1 << 20)
    key = cell[:, :, 0]
    for c in range(1, dim):
        key = key + cell[:, :, c] * SPAN ** c
    return valid, key


def composed(points, voxel):
    """[(keys (V,), centroids (V,cols) fp32, members (V,))] per pair from library calls alone."""
    valid, key = keys_of(points, voxel)
    out = []
    for b in range(points.shape[0]):
        rows = points[b][valid[b]]
        uniq, inverse = torch.unique(key[b][valid[b]], return_inverse=True)
        sums = torch.zeros(uniq.shape[0], rows.shape[1], dtype=torch.float64, device=points.device)
        sums.index_add_(0, inverse, rows.double())
        n = torch.bincount(inverse, minlength=uniq.shape[0])
        mean = sums / n[:, None]
        length = mean[:, 3:6].norm(dim=1, keepdim=True)
        mean[:, 3:6] = torch.where(length > 0, mean[:, 3:6] / length.clamp_min(1e-300), torch.zeros_like(length))
        out.append((uniq, mean.float(), n))
    return out


def compare(points, voxel):
    """(cells per pair, largest |centroid difference| in metres over the xyz columns) between the two forms."""
    out, count, n, first, _ = dICP.voxel_downsample(points, voxel, dim=3, pad_val=PAD, normals=True, return_info=True)
    _, key = keys_of(points, voxel)
    worst, counts = 0.0, []
    for b, (uniq, mean, members) in enumerate(composed(points, voxel)):
        c = int(count[b])
        assert c == uniq.shape[0], (b, c, uniq.shape[0])
        at = torch.searchsorted(uniq, key[b][first[b, :c].long()])
        assert torch.equal(uniq[at], key[b][first[b, :c].long()]) and torch.equal(members[at].int(), n[b, :c])
        worst = max(worst, float((out[b, :c, :3] - mean[at, :3]).abs().max()))
        counts.append(c)
    return counts, worst


def measure(fn, rounds, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t = [timed(fn, reps) for _ in range(rounds)]
    return (statistics.median(t), min(t), max(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_voxel needs a HIP device: a CPU run cannot give a time")
    dev = torch.device("cuda:0")
    res = {"cases": {}}
    clouds = [("batch", dict(indices=range(args.batch), m_valid=20000, m_pad=20480, dim=3)),
              ("map_1m", dict(indices=[0], m_valid=(1 << 20) - 480, m_pad=1 << 20, dim=3))]
    for name, kw in clouds:
        pts = synthetic.make_batch(list(kw.pop("indices")), **kw)["map_pc"].contiguous().to(dev)
        B, M, _ = pts.shape
        for voxel in (0.1, 0.3, 1.0):
            counts, worst = compare(pts, voxel)
            kern = measure(lambda: dICP.voxel_downsample(pts, voxel, dim=3, pad_val=PAD, normals=True), args.rounds, args.reps)
            comp = measure(lambda: composed(pts, voxel), args.rounds, max(1, args.reps // 2))
            valid = int(((pts[:, :, :3].abs() < PAD).all(dim=2)).sum())
            case = {"B": B, "M": M, "voxel": voxel, "kernel_ms": kern, "composed_ms": comp, "composed_over_kernel": comp[0] / kern[0],
                    "rows_valid": valid, "rows_out": sum(counts), "reduction": valid / max(sum(counts), 1),
                    "max_abs_xyz_difference": worst, "rows_per_s_kernel": B * M / (kern[0] * 1e-3)}
            res["cases"]["%s_%g" % (name, voxel)] = case
            print(name, voxel, json.dumps(case), flush=True)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
