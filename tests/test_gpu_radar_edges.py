"""GPU: forward parity of the radar front end (csrc/mmk_radar.hip) at row ends, image borders and launch classes -- against the
reference's stored outputs (tests/golden/radar_edges.npz, written by tests/golden/make_golden_radar_edges.py) and, where a shape
has no golden value, against oracle/radar_ref.py on inputs conditioned as the fixture's are (tests/radar_edge_cases.py).

No comparison forgives a share of cells or leaves a case out: every band in which the device's last bit could decide (a cell at
its threshold or at the hardshrink gate, two window sums that almost tie, tanh near its saturation, a pixel index at an
integer) is a condition on the INPUTS, asserted on the CPU before the device runs.

  CFAR       hard mask equal on every cell, soft mask within 2e-5 on every cell (test_gpu_radar.py's bound): the eight column
             range cases of the fixture (mincol = w2 + guard + 1; maxcol = R, right windows cut by the row's end), six launch
             classes R = 600 | 3412 | 3413 | 4097 | 5461 | 13647 with windows that reach the row's end, and the persistent
             kernel's row walk over six scans with six different threshold pairs.  At R = 5461 and 13647 also the scan gradient
             against the fp64 restatement of radar_edge_cases.py, under CFAR_REL = 1.6e-5 of max |ref| (test_gpu_cfar_params.py).
  extractor  exact counts, coordinates within 3e-5 (hard) / 4e-5 (soft), times equal to the fp32 (t1 + t0) / 2, zero padding:
             blobs from cell 0, blobs that reach column R - 1, single cells, an alternating row, R = 2, odd R (misaligned rows),
             A = 300 and A = 600 (several rows per thread of the row scan), an odd marker count, truncation.
  resampler  within 2e-5 of the fixture in all three variants; exactly 0 where every tap is padding; the paired entry.
  sampler and rasteriser   weights within 2e-5, statistics within test_extract_weights_golden's bounds, the BEV equal.

Where the reference differs from what was expected of it (pinned in tests/test_radar_edges_cpu.py): a pixel is all padding from
range (R + 0.5) res on, not from (R - 1) res; with the wobble fix a pixel above the last azimuth is clamped to the last row, not
padded; a single marker gives an empty cloud instead of an error; pk0 has two points that pair markers of different rows.

Measured on an MI355X (the worst of the RATIO lines the tests print, bound in brackets):
    RATIO cf 0a .. 1b, launch class R=600 .. 13647, persistent walk     max |soft - ref| = 5.960e-08   [2e-5]; hard masks equal
    RATIO scan gradient R=5461 item 0 / 1                               err/scale = 2.154e-06 / 2.274e-06   [1.6e-5]
    RATIO scan gradient R=13647 item 0 / 1                              err/scale = 2.196e-06 / 2.323e-06   [1.6e-5]
    RATIO R=5461 a_thresh / b_thresh     |got - ref| / scale = 1.554e-07 2.666e-08 / 1.595e-07 1.770e-08   [1.6e-5]
    RATIO R=13647 a_thresh / b_thresh    |got - ref| / scale = 5.372e-08 1.592e-07 / 4.233e-08 1.597e-07   [1.6e-5]
    RATIO pk0 .. pk5 pc, pcT (worst: pk4 pcT) / pks                     max |pc - ref| = 1.907e-06 / 5.960e-08   [3e-5 / 4e-5]
    RATIO pc0 / pc1 / pc2, every table and variant                      max |cart - ref| = 1.788e-06 / 3.427e-06 / 2.384e-07   [2e-5]
    RATIO weights c / s                                                 max |w - ref| = 2.980e-08 / 5.960e-08   [2e-5]

Found by test_cfar_threshold_gradients_at_the_longest_rows[13647]: cfar_mask_bwd_kernel<NPRE, CfarThPtr> declared a second
static LDS array for its two threshold sums, 128 bytes beyond the 64 that cfar_args leaves beside the longest row, so
mmk_cfar_mask_bwd_p was refused with "invalid argument" for R = 13637 .. 13647, rows that the other three entries run.  The
sums now go through the scan's own eight doubles, in the same order (equal bits).
"""
import numpy as np
import pytest
import torch

from mm_masking_amd import radar_utils as ru
from oracle import radar_ref
from radar_cases import RES, threshold_grads_f64
from radar_edge_cases import (CF_RES, EW_MASKS, GRAD_R, LAUNCH_R, PC_CASES, PC_TABLES, PC_VARIANTS, PEAK_HARD, PEAK_SOFT, SOFT_STEEP,
                              WALK_SHAPE, assert_cfar_conditions, beyond_range, cf_sets, cfar_scan_grad_f64, ew_mask, launch_scan,
                              marker_counts, peak_case, point_times, walk_scan)
from support import DEV, close, dev, load_golden

pytestmark = pytest.mark.gpu
SOFT_ABS = 2e-5
CFAR_REL = 1.6e-5


@pytest.fixture(scope="module")
def gold(golden_dir):
    return load_golden(golden_dir, "radar_edges.npz")


# ----------------------------------------------------------------------------- CFAR
def _masks_equal_oracle(got_hard, got_soft, want_hard, want_soft, name):
    """Hard equality on every cell and the soft bound on every cell."""
    assert np.array_equal(got_hard, want_hard), (name, np.argwhere(got_hard != want_hard)[:8])
    err = np.abs(got_soft - want_soft).max()
    print("RATIO %-40s max |soft - ref| = %.3e" % (name, err))
    assert err <= SOFT_ABS, (name, err)


@pytest.mark.parametrize("tag,kw", cf_sets())
def test_cfar_column_range_ends(gold, tag, kw):
    raw = gold["cf_raw"]
    hard = ru.cfar_mask(dev(raw), CF_RES, diff=False, **kw).cpu().numpy()
    soft = ru.cfar_mask(dev(raw), CF_RES, diff=True, **kw).cpu().numpy()
    _masks_equal_oracle(hard, soft, gold["cf_hard" + tag].astype(np.float32), gold["cf_soft" + tag], "cf " + tag)


@pytest.mark.parametrize("R", LAUNCH_R)
def test_cfar_values_at_every_launch_class(R):
    raw, kw = launch_scan(R)
    th64, (w2, guard, mincol, maxcol) = assert_cfar_conditions(raw, RES, **kw)
    assert maxcol + w2 + guard + 1 >= R and R - maxcol < 60         # the last windows end at the row's end
    assert np.abs(radar_ref.cfar_threshold(raw, RES, **kw)[:, :, mincol:maxcol] - th64).max() < 4e-7
    want_hard, want_soft = radar_ref.cfar_mask(raw, RES, diff=False, **kw), radar_ref.cfar_mask(raw, RES, diff=True, **kw)
    x = dev(raw).requires_grad_(R in GRAD_R)
    hard = ru.cfar_mask(x.detach(), RES, diff=False, **kw).cpu().numpy()
    soft = ru.cfar_mask(x, RES, diff=True, **kw)
    _masks_equal_oracle(hard, soft.detach().cpu().numpy(), want_hard, want_soft, "launch class R=%d" % R)
    for m in (want_hard, want_soft):
        assert 0 < (m[:, :, mincol:maxcol] != 0).mean() < 1 and (m[:, :, R - 200:] != 0).any()
    if R in GRAD_R:
        G = np.random.default_rng(R).normal(size=raw.shape).astype(np.float32)
        soft.backward(dev(G))
        want = cfar_scan_grad_f64(raw, G, RES, **kw)
        assert np.abs(want[:, :, R - 200:]).max() > 0
        for item in range(raw.shape[0]):
            close(x.grad[item], want[item], "scan gradient R=%d item %d" % (R, item), CFAR_REL)


@pytest.mark.parametrize("R", GRAD_R)
def test_cfar_threshold_gradients_at_the_longest_rows(R):
    """The tensor-threshold entries at the rows that need the raised dynamic-LDS limit, up to the last row cfar_args admits
    for all four entries: the mask and the scan gradient are the number path's bits, the two threshold gradients meet
    test_gpu_cfar_params.py's bound against radar_cases.threshold_grads_f64, relative to the same sums with |G|."""
    raw, kw = launch_scan(R)
    B = raw.shape[0]
    G = np.random.default_rng(R).normal(size=raw.shape).astype(np.float32)
    av, bv = np.full(B, 1.0), np.full(B, np.float32(0.09), dtype=np.float64)
    a, b = dev(av.astype(np.float32)).requires_grad_(True), dev(bv.astype(np.float32)).requires_grad_(True)
    x, x2 = dev(raw).requires_grad_(True), dev(raw).requires_grad_(True)
    m = ru.cfar_mask(x, RES, a_thresh=a, b_thresh=b, diff=True, **kw)
    m.backward(dev(G))
    m2 = ru.cfar_mask(x2, RES, diff=True, **kw)
    m2.backward(dev(G))
    assert torch.equal(m, m2) and torch.equal(x.grad, x2.grad)
    for name, got, ref, scale in zip(("a_thresh", "b_thresh"), (a.grad, b.grad), threshold_grads_f64(raw, G, av, bv, res=RES, **kw),
                                     threshold_grads_f64(raw, np.abs(G), av, bv, res=RES, **kw)):
        r = np.abs(got.cpu().double().numpy() - ref) / np.abs(scale)
        print("RATIO %-40s |got - ref| / scale = %s" % ("R=%d %s" % (R, name), " ".join("%.3e" % v for v in r)))
        assert (np.abs(scale) > 0).all() and (r <= CFAR_REL).all(), (name, r)


def test_cfar_persistent_walk_with_per_scan_thresholds():
    """B A = 1200 rows on 4 x CUs blocks: a block steps from a row of one scan to a row of another, whose thresholds differ."""
    B, A, _ = WALK_SHAPE
    assert B * A > 4 * torch.cuda.get_device_properties(DEV).multi_processor_count
    raw, sets = walk_scan()
    for i, kw in enumerate(sets):
        assert_cfar_conditions(raw[i:i + 1], CF_RES, **kw)
    a = dev(np.array([kw["a_thresh"] for kw in sets], np.float32))
    b = dev(np.array([kw["b_thresh"] for kw in sets], np.float32))
    assert len({(kw["a_thresh"], kw["b_thresh"]) for kw in sets}) == B
    got = [ru.cfar_mask(dev(raw), CF_RES, minr=0.0, maxr=1e6, a_thresh=a, b_thresh=b, diff=d).cpu().numpy() for d in (False, True)]
    want = [np.concatenate([radar_ref.cfar_mask(raw[i:i + 1], CF_RES, diff=d, **kw) for i, kw in enumerate(sets)]) for d in (False, True)]
    _masks_equal_oracle(got[0], got[1], want[0], want[1], "persistent walk, per-scan thresholds")
    assert all(0 < want[0][i].mean() < 1 for i in range(B))


# ----------------------------------------------------------------------------- extractor
def _extract(c, max_pts, use_T=False, **over):
    a = dict(c, **over)
    pc, cnt, t = ru.extract_pc_padded(dev(a["mask"]), a["res"], dev(a["az"]), dev(a["tm"]), max_pts, T_ab=dev(a["T_ab"]) if use_T else None,
                                      diff=a["diff"], steep_fact=SOFT_STEEP, return_times=True)
    return pc.cpu().numpy(), cnt.cpu().numpy(), t.cpu().numpy()


@pytest.mark.parametrize("name", PEAK_HARD + PEAK_SOFT)
def test_extractor_edge_cases(gold, name):
    c = peak_case(gold, name)
    B, n = c["mask"].shape[0], c["n"]
    max_pts = int(n.max()) + 3
    times = point_times(c["mask"], c["res"], c["diff"], c["tm"])
    for key, use_T in (("pc", False), ("pcT", True)):
        pc, cnt, t = _extract(c, max_pts, use_T)
        assert cnt.tolist() == n.tolist() == (c["nmark"] // 2).tolist()
        for b in range(B):
            if n[b]:
                err = np.abs(pc[b, :n[b]] - c[key][b, :n[b]]).max()
                print("RATIO %-40s max |pc - ref| = %.3e" % ("%s %s item %d" % (name, key, b), err))
                assert err <= (4e-5 if c["diff"] else 3e-5), (name, key, b, err)
            assert np.array_equal(t[b, :n[b]], times[b])
            assert (pc[b, n[b]:] == 0).all() and (t[b, n[b]:] == 0).all()


def test_extractor_odd_marker_count(gold):
    """One marker more, behind all others (a further azimuth row whose only set cell is the last one: its blob opens and never
    closes): the count stays total // 2 and every point keeps its bits.  The reference raises on such a mask
    (make_golden_radar_grads.py); on the single-marker items of pk1 it returns empty clouds, as the count 0 here."""
    c = peak_case(gold, "pk0")
    last = np.zeros((1, 1, c["mask"].shape[2]), np.float32)
    last[0, 0, -1] = 1.0
    odd = dict(mask=np.concatenate([c["mask"], last], axis=1), az=np.concatenate([c["az"], c["az"][:, -1:] + np.float32(0.1)], axis=1),
               tm=np.concatenate([c["tm"], c["tm"][:, -1:] + np.float32(0.1)], axis=1))
    assert marker_counts(odd["mask"], c["res"])[0].tolist() == [int(c["nmark"][0]) + 1] and c["nmark"][0] % 2 == 0
    even_out, odd_out = _extract(c, 8), _extract(c, 8, **odd)
    assert odd_out[1].tolist() == [(int(c["nmark"][0]) + 1) // 2] == even_out[1].tolist()
    assert all(np.array_equal(p, q) for p, q in zip(even_out, odd_out)) and (even_out[0][0, :5] != 0).any()
    single = peak_case(gold, "pk1")
    pc, cnt, t = _extract(single, 4)
    assert (single["nmark"] == 1).all() and cnt.tolist() == [0, 0] and (pc == 0).all() and (t == 0).all()


def test_extractor_truncation(gold):
    c = peak_case(gold, "pk0")
    full, short = _extract(c, 8), _extract(c, 2)
    assert short[1].tolist() == [5] and short[0].shape == (1, 2, 3)
    assert np.array_equal(short[0], full[0][:, :2]) and np.array_equal(short[2], full[2][:, :2])
    assert np.abs(short[0][0] - c["pc"][0, :2]).max() <= 3e-5


def test_extractor_many_azimuth_rows():
    """A = 600: the row scan gives every thread up to three rows; one blob in every 7th row, one of them open at the row's end."""
    B, A, R = 2, 600, 40
    mask = np.zeros((B, A, R), np.float32)
    for b in range(B):
        for a in range(b, A, 7):
            lo = 3 + (5 * a + 11 * b) % 30
            mask[b, a, lo:lo + 1 + a % 4] = 1.0
    mask[0, 595, R - 2:] = 1.0                                       # rows 595 and 602 - 7: two open blobs keep the count even
    mask[0, 588, :] = 0.0
    mask[0, 588, R - 1] = 1.0
    rng = np.random.default_rng(31)
    az = np.sort(rng.uniform(0, 2 * np.pi, (B, A)), axis=1).astype(np.float32)
    tm = np.cumsum(rng.uniform(0, 1e-3, (B, A)), axis=1).astype(np.float32)
    nmark = marker_counts(mask, RES)[0]
    assert (nmark % 2 == 0).all() and (nmark > 150).all()
    want = radar_ref.extract_pc(mask, RES, az, tm, diff=False)
    c = dict(mask=mask, res=RES, az=az, tm=tm, T_ab=None, diff=False)
    pc, cnt, t = _extract(c, 128)
    times = point_times(mask, RES, False, tm)
    for b in range(B):
        n = want[b].shape[0]
        assert cnt[b] == n == nmark[b] // 2 and n <= 128
        np.testing.assert_allclose(pc[b, :n], want[b], atol=3e-5)
        assert np.array_equal(t[b, :n], times[b]) and (pc[b, n:] == 0).all() and (t[b, n:] == 0).all()


# ----------------------------------------------------------------------------- resampler
@pytest.mark.parametrize("kind", PC_TABLES)
@pytest.mark.parametrize("ci", range(len(PC_CASES)))
def test_resampler_borders_and_tables(gold, ci, kind):
    A, R, res, W = PC_CASES[ci]
    img, az = dev(gold["pc%d_img" % ci]), dev(gold["pc%d_az_%s" % (ci, kind)])
    zero, edge = beyond_range(W, R, res)
    if ci < 2:
        assert zero.sum() >= 20 and edge.any()
    for vi, kw in enumerate(PC_VARIANTS):
        want = gold["pc%d_cart_%s%d" % (ci, kind, vi)]
        got = ru.radar_polar_to_cartesian_diff(img, az, res, cart_pixel_width=W, **kw)
        err = np.abs(got.cpu().numpy() - want).max()
        print("RATIO %-40s max |cart - ref| = %.3e" % ("pc%d %s variant %d" % (ci, kind, vi), err))
        assert err <= 2e-5, (ci, kind, vi, err)
        assert (got.cpu().numpy()[:, zero] == 0).all()
        assert ci == 2 or (got.cpu().numpy()[:, edge] != 0).any()
        if not kw:                                                   # the paired entry runs the default variant
            other = torch.flip(img, dims=(2,)).contiguous()
            a, b = ru._polar_to_cart_pair(img, other, az, res, cart_pixel_width=W)
            assert torch.equal(a, got) and torch.equal(b, ru.radar_polar_to_cartesian_diff(other, az, res, cart_pixel_width=W))
            assert not torch.equal(a, b)


# ----------------------------------------------------------------------------- sampler and rasteriser
@pytest.mark.parametrize("tag", sorted(EW_MASKS))
def test_weights_at_the_image_border(gold, tag):
    pts, mask = gold["ew_pts"], ew_mask(tag)
    w, dmn, mn, mean_w, max_w, min_w = ru.extract_weights(dev(mask), dev(pts))
    err = np.abs(w.cpu().numpy() - gold["ew_w_" + tag]).max()
    print("RATIO %-40s max |w - ref| = %.3e" % ("weights " + tag, err))
    assert err <= 2e-5
    np.testing.assert_allclose([dmn.item(), mn.item(), mean_w.item(), max_w.item(), min_w.item()], gold["ew_stats_" + tag],
                               rtol=1e-5, atol=2e-5)
    on_cpu = ru.extract_weights(torch.from_numpy(mask), torch.from_numpy(pts))       # CPU in -> CPU out
    assert on_cpu[0].device.type == "cpu" and torch.equal(on_cpu[0], w.cpu())


def test_bev_at_the_image_border(gold):
    pts = gold["bev_pts"]
    want = np.zeros((2, 640, 640), np.float32)
    j = gold["bev_nz_idx"].astype(np.int64)
    want[j[0], j[1], j[2]] = 1.0
    bev = ru.extract_bev_from_pts(dev(pts))
    np.testing.assert_array_equal(bev.cpu().numpy(), want)
    on_cpu = ru.extract_bev_from_pts(torch.from_numpy(pts))
    assert on_cpu.device.type == "cpu" and torch.equal(on_cpu, bev.cpu())
