"""GPU: mmk_voxel_downsample / dICP.voxel_downsample against the numpy restatement (voxel_ref.py).

Tolerances (derived, not measured).  Integer outputs (count, n, first, voxel_of) equal the restatement's.  A centroid lies
within 2^-23 |mean| + 2^-30 max|value of the pair| of the fp64 mean: one fp32 rounding, plus the fixed-point resolution
max|value| 2^(ceil(log2 M) - 61) for any M < 2^31.  A normal component lies within 2^-22 of the fp64 unit vector.  FIRST
rows are bit copies.  Inputs are normal fp32 numbers or exact zeros (a flushed denormal product would move a cell)."""
import os

import numpy as np
import pytest
import torch

from mm_masking_amd import dICP, synthetic
from mm_masking_amd import icp_weight_dataset as ds
from mm_masking_amd.dICP.ICP import ICP
import dicp_kat as kat
from export_util import dataset_params, write_fixture_export
from voxel_ref import valid_rows, voxel_ref_batch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
PAD = 1000.0


def run(points, voxel, **kw):
    out, count, n, first, voxel_of = dICP.voxel_downsample(torch.from_numpy(np.ascontiguousarray(points)).to(DEV), voxel,
                                                           return_info=True, **kw)
    B, M, cols = points.shape
    max_out = kw.get("max_out") or M
    assert out.dtype == torch.float32 and all(t.dtype == torch.int32 for t in (count, n, first, voxel_of))
    assert all(t.device == DEV for t in (out, count, n, first, voxel_of)) and not out.requires_grad
    assert tuple(out.shape) == (B, max_out, cols) and tuple(count.shape) == (B,) and tuple(voxel_of.shape) == (B, M)
    assert tuple(n.shape) == tuple(first.shape) == (B, max_out)
    return {"out": out.cpu().numpy(), "count": count.cpu().numpy(), "n": n.cpu().numpy(), "first": first.cpu().numpy(),
            "voxel_of": voxel_of.cpu().numpy()}


def check(points, got, ref, mode, normals):
    """``got`` (kernel) against ``ref`` (restatement) under the module's tolerances."""
    for key in ("count", "n", "first", "voxel_of"):
        assert np.array_equal(got[key], ref[key]), key
    B, max_out, cols = got["out"].shape
    for b in range(B):
        kept = min(int(ref["count"][b]), max_out)
        o, want = got["out"][b], ref["out"][b]
        assert (o[kept:] == np.float32(PAD)).all()
        if mode == "first":
            assert np.array_equal(o[:kept].view(np.uint32), points[b][ref["first"][b, :kept]].view(np.uint32))
            continue
        tol = 2.0 ** -23 * np.abs(want[:kept]) + 2.0 ** -30 * ref["vmax"][b]
        err = np.abs(o[:kept].astype(np.float64) - want[:kept])
        mean_cols = [c for c in range(cols) if not (normals and 3 <= c < 6)]
        assert (err[:, mean_cols] <= tol[:, mean_cols]).all(), (b, err[:, mean_cols].max())
        if normals:
            assert (err[:, 3:6] <= 2.0 ** -22).all(), (b, err[:, 3:6].max())


def unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def mixed_batch(cols, voxel, seed=0, B=3, M=1000):
    """Clustered rows in +-60 m (so that cells hold 1 .. tens of rows), negatives included, rows exactly on cell faces,
    and per pair a different number of trailing and interleaved padding rows (pad_val rows, a NaN, an infinity, a row
    beyond pad_val in z alone)."""
    rng = np.random.default_rng(seed)
    pts = np.zeros((B, M, cols), np.float32)
    for b in range(B):
        centres = rng.uniform(-59.0, 59.0, (40, 3)) * np.array([1.0, 1.0, 0.05])
        p = centres[rng.integers(0, 40, M)] + rng.uniform(-0.4, 0.4, (M, 3)) * np.array([1.0, 1.0, 0.2])
        on_face = rng.choice(M, 80, replace=False)
        p[on_face] = np.float32(voxel) * np.round(p[on_face] / voxel)                  # multiples of the edge, both signs
        pts[b, :, :min(cols, 3)] = p[:, :min(cols, 3)]
        if cols >= 6:
            pts[b, :, 3:6] = unit(rng.normal(size=(M, 3)))
        if cols > 6:
            pts[b, :, 6:] = rng.uniform(-5.0, 5.0, (M, cols - 6))
        if 3 < cols < 6:
            pts[b, :, 3:] = rng.uniform(-5.0, 5.0, (M, cols - 3))
        pts[b, M - 17 * (b + 1):] = PAD                                                # trailing padding
        holes = rng.choice(M - 60, 11 + 7 * b, replace=False)
        pts[b, holes] = PAD                                                            # interleaved padding
        pts[b, holes[0], 0] = 3.0                                                      # padding in y (and z) only
        pts[b, holes[1], :] = p[holes[1], :cols] if cols <= 3 else pts[b, holes[1] + 1]
        pts[b, holes[1], cols - 1] = np.nan
        pts[b, holes[2], :] = pts[b, holes[2] + 1]
        pts[b, holes[2], 1] = -np.inf
        if cols >= 3:
            pts[b, holes[3], :] = pts[b, holes[3] + 1]
            pts[b, holes[3], 2] = PAD                                                  # a key column only when dim = 3
    tiny = (pts != 0) & (np.abs(pts) < 1e-30)
    assert not tiny.any()
    return pts


@pytest.mark.parametrize("voxel", [0.25, 0.3])
@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("cols", [3, 6])
def test_mixed_batch(cols, dim, voxel):
    pts = mixed_batch(cols, voxel)
    valid = np.stack([valid_rows(p, dim, PAD) for p in pts])
    assert len(set(valid.sum(axis=1))) == 3 and (~valid[:, :900]).any(axis=1).all()
    for mode in ("centroid", "first"):
        ref = voxel_ref_batch(pts, voxel, dim=dim, pad_val=PAD, mode=mode)
        assert (ref["count"] > 100).all() and ref["n"].max() >= 8 and (ref["n"] == 1).any()
        got = run(pts, voxel, dim=dim, pad_val=PAD, mode=mode)
        check(pts, got, ref, mode, normals=cols == 6)
        assert (got["voxel_of"][~valid] == -1).all() and (got["voxel_of"][valid] >= 0).all()


@pytest.mark.parametrize("cols", [2, 4, 5, 8])
def test_every_column_width(cols):
    """2, 4 and 8 lanes per row in the accumulation, with and without idle lanes; normals on request at 8 columns."""
    pts = mixed_batch(cols, 0.5, seed=cols, B=2, M=333)
    for mode in ("centroid", "first"):
        ref = voxel_ref_batch(pts, 0.5, dim=2, pad_val=PAD, mode=mode)
        check(pts, run(pts, 0.5, dim=2, pad_val=PAD, mode=mode), ref, mode, normals=False)
    if cols == 8:
        ref = voxel_ref_batch(pts, 0.5, dim=3, pad_val=PAD, normals=True)
        check(pts, run(pts, 0.5, dim=3, pad_val=PAD, normals=True), ref, "centroid", normals=True)


def test_many_cells_one_cell_and_none():
    # 5000 rows in 5000 distinct cells: the table (16 384 slots) is a third full and probes
    i = np.arange(5000)
    rng = np.random.default_rng(1)
    pts = np.stack([(i % 100) - 49.5, (i // 100) - 24.5, np.full(5000, 0.25)], axis=1).astype(np.float32)[None]
    pts = pts[:, rng.permutation(5000)]
    ref = voxel_ref_batch(pts, 1.0, dim=3, pad_val=PAD)
    assert ref["count"][0] == 5000
    got = run(pts, 1.0, dim=3, pad_val=PAD)
    check(pts, got, ref, "centroid", False)
    assert np.array_equal(got["voxel_of"][0], i) and np.array_equal(got["out"][0], pts[0])      # a mean of one row is the row
    # 4096 rows in one cell
    one = rng.uniform(0.001, 0.999, (1, 4096, 6)).astype(np.float32) + np.float32([7, -3, 1, 0, 0, 0])
    one[0, :, 3:] = unit(one[0, :, 3:])
    for mode in ("centroid", "first"):
        ref = voxel_ref_batch(one, 1.0, dim=3, pad_val=PAD, mode=mode)
        assert ref["count"][0] == 1 and ref["n"][0, 0] == 4096
        check(one, run(one, 1.0, dim=3, pad_val=PAD, mode=mode), ref, mode, normals=True)
    # every row padding
    none = np.full((2, 300, 3), PAD, np.float32)
    none[1, 5] = np.nan
    got = run(none, 1.0, dim=3, pad_val=PAD)
    assert not got["count"].any() and (got["out"] == np.float32(PAD)).all() and not got["n"].any()
    assert (got["first"] == -1).all() and (got["voxel_of"] == -1).all()


def test_truncation():
    pts = mixed_batch(6, 0.3, seed=5)
    full = voxel_ref_batch(pts, 0.3, dim=3, pad_val=PAD)
    max_out = 64
    assert (full["count"] > 2 * max_out).all()
    for mode in ("centroid", "first"):
        ref = voxel_ref_batch(pts, 0.3, dim=3, pad_val=PAD, max_out=max_out, mode=mode)
        got = run(pts, 0.3, dim=3, pad_val=PAD, max_out=max_out, mode=mode)
        check(pts, got, ref, mode, normals=True)
        assert np.array_equal(got["count"], full["count"]) and np.array_equal(got["voxel_of"], full["voxel_of"])
        assert (got["voxel_of"] >= max_out).any() and (got["n"] > 0).all()
        assert np.array_equal(got["first"], full["first"][:, :max_out])
    # the default entry points without the optional outputs give the same rows
    out, count = dICP.voxel_downsample(torch.from_numpy(pts).to(DEV), 0.3, max_out=max_out, mode="first")
    assert np.array_equal(out.cpu().numpy(), got["out"]) and np.array_equal(count.cpu().numpy(), got["count"])


@pytest.fixture(scope="module")
def walls():
    """(2, 20 480 + 37, 6): simple_cloud_pair's walls with normals, 37 padding rows; 81 blocks of rows per pair."""
    pts = np.stack([synthetic.simple_cloud_pair(21 + b, 10, 20480, dim=3, pad_m=37, pad_val=PAD)[1] for b in range(2)])
    return pts, voxel_ref_batch(pts, 0.5, dim=3, pad_val=PAD), run(pts, 0.5, dim=3, pad_val=PAD)


def test_multi_block_compaction(walls):
    pts, ref, got = walls
    assert pts.shape == (2, 20517, 6) and (ref["count"] > 1000).all() and (ref["count"] < 20480).all()
    check(pts, got, ref, "centroid", normals=True)
    for b in range(2):
        kept = int(ref["count"][b])
        assert (np.diff(got["first"][b, :kept]) > 0).all() and got["n"][b].sum() == 20480
        assert (got["voxel_of"][b, 20480:] == -1).all()
    ref = voxel_ref_batch(pts, 0.5, dim=3, pad_val=PAD, mode="first")
    check(pts, run(pts, 0.5, dim=3, pad_val=PAD, mode="first"), ref, "first", normals=True)


def test_normals(walls):
    pts, ref, got = walls
    for b in range(2):
        kept = int(ref["count"][b])
        length = np.linalg.norm(got["out"][b, :kept, 3:6].astype(np.float64), axis=1)
        assert np.abs(length - 1.0).max() <= 2.0 ** -22
    # opposite normals (and only those) give exactly 0; columns 3..5 are plain means with normals=False
    p = np.zeros((1, 6, 6), np.float32)
    p[0, :, 0] = [5.5, 5.25, 1.5, 1.25, 1.75, 9.5]
    p[0, :, 1:3] = 0.5
    n = unit(np.float64([0.3, -0.5, 0.81]))
    p[0, :, 3:] = [n, -n, [1, 0, 0], [0, 1, 0], [1, 0, 0], [0, 0, 1]]
    ref = voxel_ref_batch(p, 1.0, dim=3, pad_val=PAD)
    got = run(p, 1.0, dim=3, pad_val=PAD)
    check(p, got, ref, "centroid", normals=True)
    assert got["count"][0] == 3 and not got["out"][0, 0, 3:].any() and got["out"][0, 0, 0] == np.float32(5.375)
    assert np.array_equal(got["out"][0, 2, 3:], np.float32([0, 0, 1]))
    ref = voxel_ref_batch(p, 1.0, dim=3, pad_val=PAD, normals=False)
    got = run(p, 1.0, dim=3, pad_val=PAD, normals=False)
    check(p, got, ref, "centroid", normals=False)
    assert abs(float(got["out"][0, 1, 3]) - 2.0 / 3.0) <= 2.0 ** -23


def test_reproducible_permutable_and_independent_of_the_batch(walls):
    pts, _, first = walls
    t = torch.from_numpy(pts).to(DEV)
    for a, b in zip(dICP.voxel_downsample(t, 0.5, pad_val=PAD, return_info=True),
                    dICP.voxel_downsample(t, 0.5, pad_val=PAD, return_info=True)):
        assert torch.equal(a, b)
    # a permutation of the rows: the same (row, n) for every cell, bit for bit, in the permuted order of first appearance
    rng = np.random.default_rng(2)
    perm = np.stack([rng.permutation(pts.shape[1]) for _ in range(2)])
    shuffled = np.stack([pts[b, perm[b]] for b in range(2)])
    got = run(shuffled, 0.5, dim=3, pad_val=PAD)
    assert np.array_equal(got["count"], first["count"])
    for b in range(2):
        kept = int(first["count"][b])
        assert (np.diff(got["first"][b, :kept]) > 0).all()
        was = first["voxel_of"][b, perm[b, got["first"][b, :kept]]]                     # each cell's rank before the shuffle
        assert np.array_equal(np.sort(was), np.arange(kept))
        assert np.array_equal(got["out"][b, :kept].view(np.uint32), first["out"][b, was].view(np.uint32))
        assert np.array_equal(got["n"][b, :kept], first["n"][b, was])
        old = first["voxel_of"][b, perm[b]]                                            # every row's rank before the shuffle
        assert np.array_equal(got["voxel_of"][b], np.where(old >= 0, np.argsort(was)[np.maximum(old, 0)], -1))
    # a pair's outputs do not depend on the other pairs of the batch
    other = np.stack([pts[1], shuffled[0], pts[0] * np.float32(3.0)])
    got = run(other, 0.5, dim=3, pad_val=PAD)
    alone = run(pts[1:2], 0.5, dim=3, pad_val=PAD)
    for key in first:
        want = np.asarray(first[key][1]).view(np.uint32)
        assert np.array_equal(np.asarray(got[key][0]).view(np.uint32), want), key
        assert np.array_equal(np.asarray(alone[key][0]).view(np.uint32), want), key


def test_pipeline_voxel_normals_icp():
    """voxel_downsample -> with_normals -> ICP('pt2pl') on the walls of simple_cloud_pair (dim 2, voxel 0.1, no noise): the
    source is a sub-sample of the full target moved by T_true; centroids of rows of a wall lie on the wall, so the
    downsampled target still has T_true as its answer and the pose meets the repo's standing gate."""
    S, Tg, Tt = [], [], []
    for b in range(2):
        s, t, T = synthetic.simple_cloud_pair(40 + b, 1500, 6000, dim=2, noise=0.0, pad_n=20, pad_m=60, pad_val=PAD,
                                              with_normals=False, yaw=0.02 + 0.01 * b, trans=(0.6, -0.4 + 0.1 * b, 0.0))
        S.append(s), Tg.append(t), Tt.append(T)
    src, tgt = torch.from_numpy(np.stack(S)).to(DEV), torch.from_numpy(np.stack(Tg)).to(DEV)
    down, count = dICP.voxel_downsample(tgt, 0.1, dim=2, pad_val=PAD)
    count = count.cpu().numpy()
    print("voxel 0.1: %s rows of 6000 kept" % count.tolist())
    assert (count < 0.75 * 6000).all() and (count > 1000).all()
    down = down[:, :int(count.max())].contiguous()
    six = dICP.with_normals(down, k=8, dim=2, pad_val=PAD)
    w = torch.ones(2, 1520, device=DEV)
    w[:, 1500:] = 0
    icp = ICP("pt2pl", differentiable=False, max_iterations=50, tolerance=1e-9)
    T = icp.icp(src, six, weight=w, trim_dist=5.0, dim=2)["T"]
    errs = [kat.pose_errors(T[b].cpu().numpy(), Tt[b], 2) for b in range(2)]
    print("pose errors after %s iterations: %s" % (icp.last_iterations, errs))
    for dt, da in errs:
        assert dt <= 1e-3 and da <= 1e-4, errs


def test_dataset_writes_the_voxel_cache_once(golden_dir, tmp_path):
    g = np.load(os.path.join(golden_dir, "dataset_item.npz"), allow_pickle=False)
    root = str(tmp_path)
    pairs = write_fixture_export(root, g)
    mdir = os.path.join(root, "vtr_export", "radar_lidar", pairs[0][0], pairs[0][1], "map")
    stamps = sorted(set(int(s) for s in g["map_stamp"]))
    params = dataset_params(max_map_pts=0, map_voxel=0.5)
    plain = ds.ICPWeightDataset(pairs, dataset_params(max_map_pts=0), dataset_type="test", data_dir=root)
    d = ds.ICPWeightDataset(pairs, params, dataset_type="test", data_dir=root)
    mtimes, clouds = {}, {}
    sources = {s: ds.load_xyz_bin(os.path.join(mdir, "%d.bin" % s), 6) for s in stamps}
    rows = max(c.shape[0] for c in sources.values())          # the Dataset pads its batch to the longest map (V1: the scale depends on M)
    for s in stamps:
        path = os.path.join(mdir, "%d_vox0.5.bin" % s)
        src = np.full((1, rows, 6), d.target_pad_val, np.float32)
        src[0, :sources[s].shape[0]] = sources[s]
        out, count = dICP.voxel_downsample(torch.from_numpy(src).to(DEV), 0.5, dim=3, pad_val=d.target_pad_val, normals=True)
        clouds[s] = ds.load_xyz_bin(path, 6)
        assert 0 < int(count[0]) <= sources[s].shape[0] and np.array_equal(clouds[s], out[0, :int(count[0])].cpu().numpy())
        mtimes[s] = os.stat(path).st_mtime_ns
    assert not [f for f in os.listdir(mdir) if f.endswith(".tmp")]
    assert sorted(f for f in os.listdir(mdir) if "_vox" in f) == ["%d_vox0.5.bin" % s for s in stamps]
    assert 0 < d.max_map_pts <= plain.max_map_pts
    for i in range(len(d)):
        c = clouds[int(g["map_stamp"][i])]
        pts, nrm = d._to_sensor_frame(torch.from_numpy(c[:, :3].copy()), torch.from_numpy(c[:, 3:].copy()), d.T_map_sensor_robot[0])
        kept, kept_n = ds.filter_map(pts, nrm, d.T_loc_gt[i], "radar", "lidar", return_aligned=True)
        assert torch.equal(d[i]["map_data"]["pc"], ds.pad_map(kept, kept_n, d.max_map_pts, d.target_pad_val))
    # a second construction reads the cache
    ds.ICPWeightDataset(pairs, params, dataset_type="test", data_dir=root)
    for s in stamps:
        assert os.stat(os.path.join(mdir, "%d_vox0.5.bin" % s)).st_mtime_ns == mtimes[s]
    assert not [f for f in os.listdir(mdir) if f.endswith(".tmp")]
