"""GPU: mmk_knn_normals / dICP.estimate_normals against the numpy restatement (knn_normals_ref.py):
neighbour sets element for element, normals and curvature against fp64, known answers, reproducibility, the dICP
config key and the Dataset's normals cache.  Every reference is computed once per module."""
import os

import numpy as np
import pytest
import torch

from mm_masking_amd import dICP, synthetic
from mm_masking_amd import icp_weight_dataset as ds
from mm_masking_amd.dICP.ICP import ICP
import dicp_kat as kat
from export_util import assert_same, dataset_params, write_fixture_export
from knn_normals_ref import knn_normals_ref_batch, lattice_line, lattice_plane
from support import icp_yaml

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
PAD = 1000.0
ESTIMATE = dict(target_normals="estimate", normals_k=16)
WALL_SEED = 11            # simple_cloud_pair seeds WALL_SEED, WALL_SEED + 1: every k / k+1 gap > 1e-6 (asserted below)
KS = (5, 16, 32)


def wall_clouds(dim, m=700, pad_m=37, seed=WALL_SEED):
    """(2, m + pad_m, 3): simple_cloud_pair's walls, xyz only, padding rows at 1000.0."""
    return np.stack([synthetic.simple_cloud_pair(seed + b, 10, m, dim=dim, pad_m=pad_m, pad_val=PAD, with_normals=False)[1]
                     for b in range(2)])


def wide_cloud(dim, m=1500, seed=4):
    """Rows over +-150 m (the grid covers +-128 m: the border cells hold clamped rows) and one row at (400, -300), which no
    ring settles (the exhaustive path)."""
    rng = np.random.default_rng(seed)
    p = np.zeros((1, m, 3), np.float32)
    p[0, :, :2] = rng.uniform(-150.0, 150.0, (m, 2))
    if dim == 3:
        p[0, :, 2] = rng.uniform(-2.0, 2.0, m)
    p[0, 17, :2] = (400.0, -300.0)
    return p


def doubled_lattice(n=24):
    """n x n integer lattice, every point stored twice (rows j and j + n*n): fp32 distances are exact, ties everywhere."""
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    g = np.stack([i.ravel(), j.ravel(), np.zeros(n * n)], axis=1).astype(np.float32) - np.float32(n // 2)
    return np.concatenate([g, g])[None]


def run(points, k, dim, **kw):
    n, c, cnt, nbr = dICP.estimate_normals(torch.from_numpy(np.ascontiguousarray(points)).to(DEV), k=k, dim=dim, return_info=True, **kw)
    assert n.dtype == torch.float32 and c.dtype == torch.float32 and cnt.dtype == torch.int32 and nbr.dtype == torch.int32
    assert n.device == DEV and tuple(nbr.shape) == tuple(points.shape[:2]) + (k,)
    return {"normals": n.cpu().numpy(), "curvature": c.cpu().numpy(), "count": cnt.cpu().numpy(), "nbr_idx": nbr.cpu().numpy()}


@pytest.fixture(scope="module")
def walls():
    """{(dim, k): (points, reference, kernel output)} on the wall clouds, shared by the tests below."""
    out = {}
    for dim in (2, 3):
        pts = wall_clouds(dim)
        for k in KS:
            out[(dim, k)] = (pts, knn_normals_ref_batch(pts, k, dim, pad_val=PAD), run(pts, k, dim, pad_val=PAD))
    return out


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("k", KS)
def test_neighbour_sets(walls, dim, k):
    pts, ref, got = walls[(dim, k)]
    valid = np.abs(pts[:, :, :dim]).max(axis=2) < PAD
    assert valid.sum() == 2 * 700
    assert ref["knn_gap"][valid].min() > 1e-6                      # precondition: no k / k+1 near-tie anywhere
    assert np.array_equal(got["count"], ref["count"]) and (got["count"][valid] == k).all()
    assert np.array_equal(got["nbr_idx"], ref["nbr_idx"])


@pytest.mark.parametrize("dim", [2, 3])
def test_exact_ties(dim):
    """Every distance is an exact small integer and every point has a twin: the order is (d2, index) alone.  The
    operator's smallest k is 3, so the twin rule is read from the first two slots of k = 3."""
    pts = doubled_lattice()
    m = pts.shape[1] // 2
    got = run(pts, 3, dim)
    rows = np.arange(2 * m)
    assert np.array_equal(got["nbr_idx"][0, :, 0], rows % m) and np.array_equal(got["nbr_idx"][0, :, 1], rows % m + m)
    ref = knn_normals_ref_batch(pts, 6, dim)
    got = run(pts, 6, dim)
    assert np.array_equal(got["nbr_idx"], ref["nbr_idx"]) and (got["count"] == 6).all()


@pytest.mark.parametrize("dim", [2, 3])
def test_outside_the_grid(dim):
    pts = wide_cloud(dim)
    assert (np.abs(pts[0, :, :2]).max(axis=1) > 128.0).sum() > 100
    ref = knn_normals_ref_batch(pts, 16, dim)
    assert ref["knn_gap"].min() > 1e-6
    got = run(pts, 16, dim)
    assert np.array_equal(got["nbr_idx"], ref["nbr_idx"]) and np.array_equal(got["count"], ref["count"])
    assert got["nbr_idx"][0, 17, 0] == 17 and (got["count"] == 16).all()


@pytest.mark.parametrize("dim", [2, 3])
def test_radius_and_count(dim):
    pts = wall_clouds(dim)
    ref = knn_normals_ref_batch(pts, 16, dim, max_radius=0.5, pad_val=PAD)
    valid = np.abs(pts[:, :, :dim]).max(axis=2) < PAD
    few = valid & (ref["count"] < 3)
    assert few.sum() >= 20 and (ref["count"] >= 3).sum() >= 20 and (ref["count"][valid] >= 1).all()      # isolated rows and crowded ones
    got = run(pts, 16, dim, max_radius=0.5, pad_val=PAD)
    assert np.array_equal(got["count"], ref["count"]) and np.array_equal(got["nbr_idx"], ref["nbr_idx"])
    assert not got["normals"][few].any() and not got["curvature"][few].any()
    full = valid & (ref["count"] >= 3)
    assert np.allclose(np.linalg.norm(got["normals"][full], axis=1), 1.0, atol=1e-6)


@pytest.mark.parametrize("dim", [2, 3])
def test_padding_rows(walls, dim):
    pts, _, got = walls[(dim, 16)]
    pad = ~(np.abs(pts[:, :, :dim]).max(axis=2) < PAD)
    assert pad.sum() == 2 * 37
    assert not got["normals"][pad].any() and not got["curvature"][pad].any() and not got["count"][pad].any()
    assert (got["nbr_idx"][pad] == -1).all()
    assert (got["nbr_idx"][~pad] >= 0).all() and (got["nbr_idx"][~pad] < 700).all()        # rows 700.. are the padding
    # a padding row in z only (dim 3) is padding as well; in dim 2 its z is not looked at
    p = pts.copy()
    p[:, 5, 2] = PAD
    got = run(p, 16, dim, pad_val=PAD)
    assert (got["count"][:, 5] == 0).all() == (dim == 3)
    assert ((got["nbr_idx"] == 5).any()) == (dim == 2)


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("k", KS)
def test_normals_and_curvature_against_fp64(walls, dim, k):
    """Same neighbours on both sides (test_neighbour_sets), so they differ by the order of fp64 sums (~1e-15 relative)
    over an eigen-gap >= 1e-3, plus one fp32 rounding (6e-8): 1e-5 is wide by two orders.  Below that gap the eigenvector
    is ill-conditioned and only its line is compared."""
    pts, ref, got = walls[(dim, k)]
    valid = np.abs(pts[:, :, :dim]).max(axis=2) < PAD
    n, nr = got["normals"].astype(np.float64), ref["normals"]
    assert np.allclose(np.linalg.norm(n[valid], axis=1), 1.0, atol=1e-6)
    if dim == 2:
        assert not n[:, :, 2].any()
    assert np.abs(got["curvature"] - ref["curvature"])[valid].max() <= 1e-6
    assert got["curvature"].min() >= 0 and got["curvature"].max() <= 1.0 / dim + 1e-6
    well = valid & (ref["eig_gap"] >= 1e-3)
    ill = valid & ~well
    assert ill.sum() <= 0.05 * valid.sum()
    # the orientation is not compared where the viewpoint lies in the estimated plane
    p = pts[:, :, :3].astype(np.float64)
    if dim == 2:
        p[:, :, 2] = 0
    facing = np.abs((nr * -p).sum(axis=2)) >= 1e-6 * np.linalg.norm(p, axis=2)
    err = np.abs(n - nr).max(axis=2)
    err_line = np.minimum(err, np.abs(n + nr).max(axis=2))
    print("dim %d k %d: max |n - n_ref| %.3g on %d well-posed rows, %d ill-posed, max curvature error %.3g"
          % (dim, k, err[well & facing].max(), (well & facing).sum(), ill.sum(), np.abs(got["curvature"] - ref["curvature"])[valid].max()))
    assert err[well & facing].max() <= 1e-5
    assert err_line[well & ~facing].max(initial=0.0) <= 1e-5
    # rows below the gap, up to sign only: down to a gap of 1e-8 the same bound holds (1e-15 / 1e-8 plus the fp32 rounding);
    # below that the direction is not determined by the data and the row is skipped
    some = ill & (ref["eig_gap"] >= 1e-8)
    assert err_line[some].max(initial=0.0) <= 1e-5
    assert ((n[valid] * -p[valid]).sum(axis=1) >= -1e-6 * np.linalg.norm(p[valid], axis=1)).all()      # they face the origin


def test_known_answers():
    line = np.stack([lattice_line(12, 3.0), lattice_line(12, -2.0)])
    got = run(line, 5, 2)
    assert np.array_equal(got["normals"][0], np.tile(np.float32([-1, 0, 0]), (12, 1)))
    assert np.array_equal(got["normals"][1], np.tile(np.float32([1, 0, 0]), (12, 1)))
    assert not got["curvature"].any()
    got = run(line, 5, 2, viewpoint=torch.tensor([[10.0, 0.0, 0.0], [-10.0, 0.0, 0.0]]))
    assert np.array_equal(got["normals"][0], np.tile(np.float32([1, 0, 0]), (12, 1)))
    assert np.array_equal(got["normals"][1], np.tile(np.float32([-1, 0, 0]), (12, 1)))
    plane = np.stack([lattice_plane(8, 5.0), lattice_plane(8, -4.0)])
    got = run(plane, 9, 3)
    assert np.array_equal(got["normals"][0], np.tile(np.float32([0, 0, -1]), (64, 1)))
    assert np.array_equal(got["normals"][1], np.tile(np.float32([0, 0, 1]), (64, 1)))
    assert not got["curvature"].any()
    got = run(plane, 9, 3, viewpoint=[0.0, 0.0, 9.0])                 # above the first plane and above the second
    assert np.array_equal(got["normals"][0], np.tile(np.float32([0, 0, 1]), (64, 1)))
    assert np.array_equal(got["normals"][1], np.tile(np.float32([0, 0, 1]), (64, 1)))
    # the plane x = 3 (rows (3, i, j)): the other axis
    xplane = np.ascontiguousarray(lattice_plane(8, 3.0)[:, [2, 0, 1]])[None]
    got = run(xplane, 9, 3)
    assert np.array_equal(got["normals"][0], np.tile(np.float32([-1, 0, 0]), (64, 1))) and not got["curvature"].any()


def test_noisy_wall_angle_is_reported():
    """synthetic._lidar's walls (2 cm of noise) with the generator's own normals: the angle between them and the estimate
    is printed, not asserted (it is a property of the data, k and the noise, not of the kernel)."""
    rng = np.random.default_rng(3)
    m = 20000                                                         # the training maps' density (synthetic.make_pair)
    pc = synthetic._lidar(rng, synthetic._walls(rng), synthetic._poles(rng), m, m + 480, PAD)[None]
    got = run(np.ascontiguousarray(pc[:, :, :3]), 16, 2, pad_val=PAD)
    n, g = got["normals"][0, :m, :2].astype(np.float64), pc[0, :m, 3:5].astype(np.float64)
    ang = np.degrees(np.arccos(np.clip(np.abs((n * g).sum(axis=1)), 0.0, 1.0)))
    print("%d rows of noisy walls + poles, k = 16, dim 2: angle to the generator's normal: median %.2f deg, 90th percentile %.2f deg, "
          "same side of the surface %.1f %%" % (m, np.median(ang), np.percentile(ang, 90), 100.0 * ((n * g).sum(axis=1) > 0).mean()))
    assert np.isfinite(ang).all() and (got["count"][0, :m] == 16).all() and not got["normals"][0, m:].any()


@pytest.mark.parametrize("dim", [2, 3])
def test_reproducible_and_independent_of_the_batch(walls, dim):
    pts, _, first = walls[(dim, 16)]
    again = run(pts, 16, dim, pad_val=PAD)
    alone = run(pts[1:2], 16, dim, pad_val=PAD)
    for key in first:
        assert np.array_equal(first[key], again[key]), key
        assert np.array_equal(first[key][1:2], alone[key]), key
    t = torch.from_numpy(pts).to(DEV)
    assert torch.equal(dICP.estimate_normals(t, k=16, dim=dim, pad_val=PAD), dICP.estimate_normals(t, k=16, dim=dim, pad_val=PAD))


@pytest.mark.parametrize("dim", [2, 3])
def test_icp_estimates_the_normals_of_an_xyz_target(tmp_path, dim):
    """`target_normals: estimate` == with_normals() + the default instance, bit for bit, and the pose meets the project's
    gate against T_true.  The source is an exact (noise-free) sub-sample of the target, so T_true is the exact answer
    of the problem whatever the normals are, and any distance from it is the code's."""
    S, Tg, Tt = [], [], []
    for b in range(2):
        s, t, T = synthetic.simple_cloud_pair(40 + b, 300, 900, dim=dim, noise=0.0, pad_n=20, pad_m=60, pad_val=PAD,
                                              with_normals=False, yaw=0.02 + 0.01 * b, trans=(0.6, -0.4 + 0.1 * b, 0.0))
        S.append(s), Tg.append(t), Tt.append(T)
    src, tgt = torch.from_numpy(np.stack(S)).to(DEV), torch.from_numpy(np.stack(Tg)).to(DEV)
    w = torch.ones(2, 320, device=DEV)
    w[:, 300:] = 0
    est = ICP("pt2pl", config_path=icp_yaml(tmp_path, **ESTIMATE), differentiable=False, max_iterations=50, tolerance=1e-9)
    dfl = ICP("pt2pl", differentiable=False, max_iterations=50, tolerance=1e-9)
    assert est.target_normals == "estimate" and dfl.target_normals == "given" and dfl.target_pad_val == PAD
    with pytest.raises(ValueError, match="pt2pl needs target normals"):
        dfl.icp(src, tgt, weight=w, dim=dim)
    T_est = est.icp(src, tgt, weight=w, trim_dist=5.0, dim=dim)["T"]
    six = dICP.with_normals(tgt, k=16, dim=dim, pad_val=dfl.target_pad_val)
    assert tuple(six.shape) == (2, 960, 6) and torch.equal(six[:, :, :3], tgt)
    T_dfl = dfl.icp(src, six, weight=w, trim_dist=5.0, dim=dim)["T"]
    assert torch.equal(T_est, T_dfl)
    for b in range(2):
        dt, da = kat.pose_errors(T_est[b].cpu().numpy(), Tt[b], dim)
        print("dim %d pair %d: %.3g m, %.3g rad from T_true after %s iterations" % (dim, b, dt, da, est.last_iterations))
    for b in range(2):
        dt, da = kat.pose_errors(T_est[b].cpu().numpy(), Tt[b], dim)
        assert dt <= 1e-3 and da <= 1e-4, (dim, b, dt, da)
    # the target's gradient flows through xyz only
    if dim == 2:
        g_icp = ICP("pt2pl", config_path=icp_yaml(tmp_path, **ESTIMATE), differentiable=True, max_iterations=3, tolerance=1e-9)
        tg = tgt.clone().requires_grad_(True)
        g_icp.icp(src, tg, weight=w, trim_dist=5.0, dim=dim)["T"][:, :2, 3].sum().backward()
        assert tuple(tg.grad.shape) == (2, 960, 3) and torch.isfinite(tg.grad).all() and tg.grad.abs().sum() > 0


def test_dataset_writes_the_normals_cache_once(golden_dir, tmp_path):
    g = np.load(os.path.join(golden_dir, "dataset_item.npz"), allow_pickle=False)
    root_a, root_b = os.path.join(str(tmp_path), "a"), os.path.join(str(tmp_path), "b")
    os.makedirs(root_a), os.makedirs(root_b)
    pairs = write_fixture_export(root_a, g)
    mdir = os.path.join(root_a, "vtr_export", "radar_lidar", pairs[0][0], pairs[0][1], "map")
    stamps = sorted(set(int(s) for s in g["map_stamp"]))
    xyz = {}
    for s in stamps:                                       # the maps exist only as <stamp>_xyz.bin
        six = ds.load_xyz_bin(os.path.join(mdir, "%d.bin" % s), 6)
        xyz[s] = np.ascontiguousarray(six[:, :3])
        xyz[s].tofile(os.path.join(mdir, "%d_xyz.bin" % s))
        os.remove(os.path.join(mdir, "%d.bin" % s))
    params = dataset_params(map_normal_k=8)
    da = ds.ICPWeightDataset(pairs, params, dataset_type="train", data_dir=root_a)
    mtimes = {}
    for s in stamps:
        path = os.path.join(mdir, "%d.bin" % s)
        six = ds.load_xyz_bin(path, 6)
        assert np.array_equal(six[:, :3], xyz[s])
        want = dICP.estimate_normals(torch.from_numpy(xyz[s])[None].to(DEV), k=8, dim=3).cpu().numpy()[0]
        assert np.array_equal(six[:, 3:], want) and np.abs(np.linalg.norm(want, axis=1) - 1).max() < 1e-6
        mtimes[s] = os.stat(path).st_mtime_ns
    assert not [f for f in os.listdir(mdir) if f.endswith(".tmp")]
    # an export that holds the six-column files from the start gives the same items
    pairs_b = write_fixture_export(root_b, g)
    mdir_b = os.path.join(root_b, "vtr_export", "radar_lidar", pairs_b[0][0], pairs_b[0][1], "map")
    for s in stamps:
        ds.load_xyz_bin(os.path.join(mdir, "%d.bin" % s), 6).tofile(os.path.join(mdir_b, "%d.bin" % s))
    db = ds.ICPWeightDataset(pairs_b, params, dataset_type="train", data_dir=root_b)
    assert len(da) == len(db) == 2
    for i in range(2):
        assert_same(da[i], db[i])
    # a second construction reads the cache
    ds.ICPWeightDataset(pairs, params, dataset_type="train", data_dir=root_a)
    for s in stamps:
        assert os.stat(os.path.join(mdir, "%d.bin" % s)).st_mtime_ns == mtimes[s]
    # neither file: today's error
    os.remove(os.path.join(mdir, "%d.bin" % stamps[0]))
    os.remove(os.path.join(mdir, "%d_xyz.bin" % stamps[0]))
    with pytest.raises(FileNotFoundError):
        ds.ICPWeightDataset(pairs, dataset_params(max_map_pts=0), dataset_type="train", data_dir=root_a)
