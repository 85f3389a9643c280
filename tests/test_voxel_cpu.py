"""CPU: the C ABI of the voxel filter (mmk_voxel_downsample) -- declared, exported, bound, workspace size, host-side
refusals (no launch) -- the Python wrapper's checks, the known answers of the test-side restatement (voxel_ref.py) that the
GPU tests compare the kernels with, and the Dataset option params["map_voxel"] on a CPU (cache files read, never built)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from mm_masking_amd import _lib
from mm_masking_amd import dICP
from mm_masking_amd import icp_weight_dataset as ds
from export_util import assert_same, dataset_params, write_fixture_export
from voxel_ref import cell_inverse, voxel_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mmk_voxel_downsample_workspace_bytes", "mmk_voxel_downsample")
PAD = 1000.0


@pytest.fixture(scope="module")
def L():
    _lib.build()
    return _lib.lib()


def test_new_entries_declared_exported_and_bound(L):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mmk.h")).read(), flags=re.S)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(L, name) and name in _lib.EXPORTED, name
    assert _lib.CONSTANTS["MMK_VOXEL_CENTROID"] == 0 and _lib.CONSTANTS["MMK_VOXEL_FIRST"] == 1
    assert L.mmk_version() == 502
    assert callable(dICP.voxel_downsample)


def test_workspace_bytes(L):
    f = L.mmk_voxel_downsample_workspace_bytes
    by_m = [f(2, m, 6, 100) for m in (1, 700, 20480, 100000)]
    by_b = [f(b, 700, 6, 700) for b in (1, 2, 32)]
    by_out = [f(2, 700, 6, n) for n in (1, 100, 700, 5000)]
    for sizes in (by_m, by_b, by_out):
        assert sizes[0] > 0 and all(a < b for a, b in zip(sizes, sizes[1:])), sizes
    for B, M in ((1, 1), (2, 700), (32, 20480), (1, 1 << 20)):
        assert f(B, M, 3, M) >= B * 2 * M * 8                       # the key table: capacity >= 2 M 64-bit keys per pair
    for bad in ((0, 700, 6, 700), (2, 0, 6, 700), (2, 700, 1, 700), (2, 700, 9, 700), (2, 700, 6, 0), (-1, 700, 6, 700),
                (2, (1 << 28) + 1, 6, 700)):
        assert f(*bad) == 0, bad


NULL = ctypes.c_void_p(0)
FAKE = ctypes.c_void_p(4096)          # never dereferenced: every call below fails on the host before any launch


def _call(L, points=FAKE, out=FAKE, out_count=FAKE, ws=FAKE, nbytes=None, B=2, M=100, cols=6, dim=3, voxel=0.5, pad_val=PAD,
          mode=0, normals=1, max_out=100):
    if nbytes is None:
        nbytes = L.mmk_voxel_downsample_workspace_bytes(2, 100, 6, 100)
    return L.mmk_voxel_downsample(points, B, M, cols, dim, voxel, pad_val, mode, normals, max_out, out, out_count, NULL, NULL,
                                  NULL, ws, nbytes, NULL)


def test_abi_refusals_name_the_argument(L):
    for name in ("points", "out", "out_count"):
        assert _call(L, **{name: NULL}) == -1 and b"NULL" in L.mmk_last_error(), name
    inf, nan = float("inf"), float("nan")
    for bad, word in (({"voxel": 0.0}, b"voxel"), ({"voxel": -0.5}, b"voxel"), ({"voxel": inf}, b"voxel"), ({"voxel": nan}, b"voxel"),
                      ({"pad_val": 0.0}, b"pad_val"), ({"pad_val": -PAD}, b"pad_val"), ({"pad_val": inf}, b"pad_val"),
                      ({"pad_val": nan}, b"pad_val"),
                      ({"voxel": 0.0009}, b"2^20"), ({"pad_val": 600000.0, "voxel": 0.5}, b"2^20"),
                      ({"cols": 2, "dim": 3, "normals": 0}, b"cols"), ({"cols": 9, "normals": 0}, b"cols"),
                      ({"cols": 5}, b"normals"), ({"cols": 3}, b"normals"), ({"normals": 2}, b"normals"),
                      ({"max_out": 0}, b"max_out"), ({"max_out": -3}, b"max_out"),
                      ({"mode": 2}, b"mode"), ({"mode": -1}, b"mode"),
                      ({"dim": 1}, b"dim"), ({"dim": 4}, b"dim"), ({"B": 0}, b"B"), ({"M": 0}, b"M")):
        assert _call(L, **bad) == -1, bad
        assert word in L.mmk_last_error(), (bad, L.mmk_last_error())
    # exactly 2^20 cells is accepted by the check (the call then fails on the workspace, which comes last)
    assert _call(L, pad_val=1024.0, voxel=1.0 / 1024.0, nbytes=0) == -1 and b"workspace" in L.mmk_last_error()
    need = L.mmk_voxel_downsample_workspace_bytes(2, 100, 6, 100)
    assert _call(L, nbytes=need - 1) == -1 and b"workspace" in L.mmk_last_error()
    assert _call(L, ws=NULL) == -1 and b"workspace" in L.mmk_last_error()


def test_wrapper_argument_checks_raise_value_error():
    pts = torch.zeros(1, 10, 6)
    for bad in ({"voxel": 0.0}, {"voxel": -1.0}, {"voxel": float("nan")}, {"voxel": float("inf")}, {"voxel": "0.5"},
                {"voxel": 0.5, "pad_val": 0.0}, {"voxel": 0.5, "pad_val": float("inf")}, {"voxel": 0.0009},
                {"voxel": 0.5, "dim": 1}, {"voxel": 0.5, "dim": 4}, {"voxel": 0.5, "mode": "nearest"},
                {"voxel": 0.5, "max_out": 0}, {"voxel": 0.5, "max_out": 2.5}, {"voxel": 0.5, "normals": "yes"}):
        with pytest.raises(ValueError):
            dICP.voxel_downsample(pts, **bad)
    with pytest.raises(ValueError, match="columns"):
        dICP.voxel_downsample(torch.zeros(1, 10, 2), 0.5, dim=3)
    with pytest.raises(ValueError, match="columns"):
        dICP.voxel_downsample(torch.zeros(1, 10, 9), 0.5)
    with pytest.raises(ValueError, match="normals"):
        dICP.voxel_downsample(torch.zeros(1, 10, 3), 0.5, normals=True)
    with pytest.raises(ValueError):
        dICP.voxel_downsample(torch.zeros(10, 3), 0.5)
    with pytest.raises(ValueError):
        dICP.voxel_downsample(torch.zeros(1, 0, 3), 0.5)


def test_no_device_is_an_error_not_a_fallback():
    with pytest.raises(_lib.MmkError, match="needs an MI355X/HIP device"):
        dICP.voxel_downsample(torch.zeros(1, 10, 3), 0.5)
    with pytest.raises(_lib.MmkError, match="needs an MI355X/HIP device"):
        dICP.voxel_downsample(torch.zeros(2, 10, 6), 0.25, dim=2, mode="first", return_info=True)


# ------------------------------------------------------------------------------------------------ the restatement
def test_restatement_cells():
    assert cell_inverse(0.25) == np.float32(4.0) and cell_inverse(0.3) == np.float32(1.0 / float(np.float32(0.3)))
    pts = np.array([[-0.1, 0, 0], [0.1, 0, 0], [-1.0, 0, 0], [0.999, 0, 0], [1.0, 0, 0]], np.float32)
    r = voxel_ref(pts, 1.0)
    assert r["count"] == 3 and np.array_equal(r["voxel_of"], [0, 1, 0, 1, 2])            # floor, not truncation; faces belong upward
    assert np.array_equal(r["n"][:3], [2, 2, 1]) and np.array_equal(r["first"][:3], [0, 1, 4])
    assert (r["n"][3:] == 0).all() and (r["first"][3:] == -1).all() and (r["out"][3:] == PAD).all()
    # dim 2 ignores z for the key and still averages it
    pts = np.array([[0.5, 0.5, -3.0], [0.25, 0.75, 5.0]], np.float32)
    assert voxel_ref(pts, 1.0, dim=3)["count"] == 2
    r = voxel_ref(pts, 1.0, dim=2)
    assert r["count"] == 1 and np.array_equal(r["out"][0], [0.375, 0.625, 1.0])


def test_restatement_doubled_lattice():
    """An 8 x 8 x 2 integer lattice stored twice, voxel 2: dim 2 folds z, 16 cells of 16 rows; dim 3, 16 cells of 16 rows in
    the one layer of cells that z = 0, 1 fall in as well; every centroid is exact."""
    i, j, k = np.meshgrid(np.arange(8), np.arange(8), np.arange(2), indexing="ij")
    g = np.stack([i.ravel(), j.ravel(), k.ravel()], axis=1).astype(np.float32) - np.float32([4, 4, 0])
    pts = np.concatenate([g, g])
    for dim in (2, 3):
        r = voxel_ref(pts, 2.0, dim=dim)
        assert r["count"] == 16 and (r["n"][:16] == 16).all() and (r["n"][16:] == 0).all()
        cells = np.floor(g[r["first"][:16]] / 2.0)
        assert np.array_equal(r["out"][:16, :2], 2.0 * cells[:, :2] + 0.5) and (r["out"][:16, 2] == 0.5).all()
        assert np.array_equal(r["voxel_of"][:128], r["voxel_of"][128:])
    f = voxel_ref(pts, 2.0, dim=2, mode="first")
    assert np.array_equal(f["out"][:16], pts[f["first"][:16]]) and f["count"] == 16


def test_restatement_normals_padding_and_order():
    pts = np.zeros((6, 6), np.float32)
    pts[:, 0] = [5.5, 5.25, 1.5, 1.25, 1.75, 9.5]
    pts[:, 3:] = [[0, 1, 0], [0, -1, 0], [1, 0, 0], [0, 1, 0], [1, 0, 0], [0, 0, 1]]
    r = voxel_ref(pts, 1.0)
    assert r["count"] == 3 and np.array_equal(r["first"][:3], [0, 2, 5])                 # first appearance, not cell order
    assert np.array_equal(r["out"][0], [5.375, 0, 0, 0, 0, 0])                           # opposite normals: the zero normal
    assert np.allclose(r["out"][1, 3:], np.array([2, 1, 0]) / np.sqrt(5.0), atol=1e-15) and r["out"][1, 0] == 1.5
    assert np.array_equal(r["out"][2], [9.5, 0, 0, 0, 0, 1])
    plain = voxel_ref(pts, 1.0, normals=False)
    assert np.array_equal(plain["out"][1, 3:], [2.0 / 3.0, 1.0 / 3.0, 0.0])
    # padding rows, a NaN and an infinity in any column, |x| >= pad_val in a key column: dropped, voxel_of -1
    p = np.tile(np.float32([1.5, 2.5, 3.5, 0, 0, 1]), (7, 1))
    p[1, :] = PAD
    p[2, 4] = np.nan
    p[3, 5] = np.inf
    p[4, 0] = -PAD
    p[5, 2] = PAD                                                                       # a key column only when dim = 3
    r = voxel_ref(p, 0.5, dim=3)
    assert r["count"] == 1 and np.array_equal(r["voxel_of"], [0, -1, -1, -1, -1, -1, 0]) and r["n"][0] == 2
    r = voxel_ref(p, 0.5, dim=2)
    assert r["count"] == 1 and np.array_equal(r["voxel_of"], [0, -1, -1, -1, -1, 0, 0]) and r["vmax"] == PAD
    r = voxel_ref(np.full((4, 3), PAD, np.float32), 0.5)
    assert r["count"] == 0 and (r["out"] == PAD).all() and (r["voxel_of"] == -1).all() and r["vmax"] == 0.0
    # max_out below the count: the first cells are kept, voxel_of keeps every rank
    r = voxel_ref(pts, 1.0, max_out=2)
    assert r["count"] == 3 and r["out"].shape == (2, 6) and np.array_equal(r["first"], [0, 2]) and r["voxel_of"][5] == 2


# ------------------------------------------------------------------------------------------------ the Dataset option
def _fixture(golden_dir, root):
    g = np.load(os.path.join(golden_dir, "dataset_item.npz"), allow_pickle=False)
    pairs = write_fixture_export(root, g)
    mdir = os.path.join(root, "vtr_export", "radar_lidar", pairs[0][0], pairs[0][1], "map")
    return g, pairs, mdir


def test_dataset_without_map_voxel_is_unchanged(golden_dir, tmp_path):
    g, pairs, mdir = _fixture(golden_dir, str(tmp_path))
    before = sorted(os.listdir(mdir))
    plain = ds.ICPWeightDataset(pairs, dataset_params(max_map_pts=0), dataset_type="test", data_dir=str(tmp_path))
    for off in ({"map_voxel": None}, {"map_voxel": 0}, {"map_voxel": 0.0}):
        d = ds.ICPWeightDataset(pairs, dataset_params(max_map_pts=0, **off), dataset_type="test", data_dir=str(tmp_path))
        assert d.max_map_pts == plain.max_map_pts and len(d) == len(plain) == 2
        assert d._cloud_sources(0) == plain._cloud_sources(0)
        for i in range(2):
            assert_same(d[i], plain[i])
    assert sorted(os.listdir(mdir)) == before and not [f for f in before if "_vox" in f]
    for bad in (-0.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="map_voxel"):
            ds.ICPWeightDataset(pairs, dataset_params(map_voxel=bad), dataset_type="test", data_dir=str(tmp_path))


def test_dataset_reads_the_voxel_cache_on_a_cpu(golden_dir, tmp_path):
    g, pairs, mdir = _fixture(golden_dir, str(tmp_path))
    voxel = 2.0
    plain = ds.ICPWeightDataset(pairs, dataset_params(max_map_pts=0), dataset_type="test", data_dir=str(tmp_path))
    if not torch.cuda.is_available():                      # no cache file and no device: an error, not the full map
        with pytest.raises(_lib.MmkError, match="needs an MI355X/HIP device"):
            ds.ICPWeightDataset(pairs, dataset_params(map_voxel=voxel), dataset_type="test", data_dir=str(tmp_path))
        assert not [f for f in os.listdir(mdir) if "_vox" in f or f.endswith(".tmp")]
    # the cache files, written by the restatement
    clouds, want_max = {}, 0
    for s in sorted(set(int(s) for s in g["map_stamp"])):
        six = ds.load_xyz_bin(os.path.join(mdir, "%d.bin" % s), 6)
        r = voxel_ref(six, voxel, dim=3, pad_val=PAD, normals=True)
        assert 0 < r["count"] < six.shape[0]                # the fixture's maps do shrink at this voxel
        clouds[s] = r["out"][:r["count"]].astype(np.float32)
        clouds[s].tofile(os.path.join(mdir, "%d_vox%r.bin" % (s, voxel)))
    d = ds.ICPWeightDataset(pairs, dataset_params(max_map_pts=0, map_voxel=voxel), dataset_type="test", data_dir=str(tmp_path))
    assert d._cloud_sources(0)[2] == os.path.join(mdir, "%d_vox2.0.bin" % int(g["map_stamp"][0]))
    for i in range(2):
        s = int(g["map_stamp"][i])
        pts, nrm = d._to_sensor_frame(torch.from_numpy(clouds[s][:, :3]), torch.from_numpy(clouds[s][:, 3:]), d.T_map_sensor_robot[0])
        kept, kept_n = ds.filter_map(pts, nrm, d.T_loc_gt[i], "radar", "lidar", return_aligned=True)
        want_max = max(want_max, kept.shape[0])
    assert d.max_map_pts == want_max and 0 < d.max_map_pts < plain.max_map_pts
    for i in range(2):
        s = int(g["map_stamp"][i])
        pts, nrm = d._to_sensor_frame(torch.from_numpy(clouds[s][:, :3]), torch.from_numpy(clouds[s][:, 3:]), d.T_map_sensor_robot[0])
        kept, kept_n = ds.filter_map(pts, nrm, d.T_loc_gt[i], "radar", "lidar", return_aligned=True)
        item = d[i]
        assert torch.equal(item["map_data"]["pc"], ds.pad_map(kept, kept_n, d.max_map_pts, d.target_pad_val))
        assert_same(item["loc_data"], plain[i]["loc_data"])           # the scan side does not see the option
    # an integer value names the same file: the name carries repr(float(voxel))
    d2 = ds.ICPWeightDataset(pairs, dataset_params(max_map_pts=0, map_voxel=2), dataset_type="test", data_dir=str(tmp_path))
    assert d2._cloud_sources(1) == d._cloud_sources(1) and d2.max_map_pts == d.max_map_pts
