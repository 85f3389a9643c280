"""GPU: gradients of the radar front end with respect to the scan -- cfar_mask(diff=True) (mmk_cfar_mask_bwd) and
extract_pc / extract_pc_padded (mmk_extract_peaks_bwd) against the reference's own CPU autograd (tests/golden/radar_grads.npz,
written by tests/golden/make_golden_radar_grads.py), the chain scan -> CFAR -> peaks -> extract_weights -> dICP -> pose,
structural zeros, run-to-run bit equality, full-size scans and long rows, dtype / device of the gradients.

Tolerances: the only rounding difference between the kernels and the reference's autograd is the device tanhf /
sinf / cosf against the host's; every comparison is against each gradient's own scale, max |ref| (support.close), and every
bound is 4 x the worst ratio measured on an MI355X:

    test                                    worst measured    bound
    cfar, default parameters                3.9e-6            CFAR_REL  = 1.6e-5
    cfar, second parameter set              8.8e-7            CFAR_REL
    peaks (all four cases, both forms)      2.3e-7            PEAKS_REL = 1.0e-6
    chain (both NN engines)                 3.8e-6            CHAIN_REL = 1.6e-5  (ceiling: the dICP backward's 2e-3)
"""
import numpy as np
import pytest
import torch

from mm_masking_amd import synthetic
from mm_masking_amd import radar_utils as ru
from mm_masking_amd.dICP.ICP import ICP
from radar_cases import RES, cfar_kw
from support import DEV, close, dev, load_golden, nn_engine  # noqa: F401  (nn_engine: a fixture)

pytestmark = pytest.mark.gpu
CFAR_REL = 1.6e-5
PEAKS_REL = 1.0e-6
CHAIN_REL = 1.6e-5


@pytest.fixture(scope="module")
def gold(golden_dir):
    return load_golden(golden_dir, "radar_grads.npz")


# ----------------------------------------------------------------------------- 1. cfar_mask
@pytest.mark.parametrize("tag", [0, 1])
def test_cfar_gradient_matches_reference(gold, tag):
    """raw.grad of cfar_mask(diff=True) for the three fixture items (the third: an empty field with isolated returns,
    exact ties of the two window sums), each against its own scale."""
    kw = cfar_kw(gold, tag)
    raw = dev(gold["ca_raw"]).requires_grad_(True)
    m = ru.cfar_mask(raw, RES, diff=True, **kw)
    assert m.requires_grad and m.grad_fn is not None
    m.backward(dev(gold["ca_G"]))
    assert raw.grad is not None and raw.grad.shape == raw.shape and raw.grad.dtype == torch.float32 and raw.grad.is_cuda
    want = gold["ca_grad%d" % tag]
    for item in range(want.shape[0]):
        close(raw.grad[item], want[item], "cfar set %d item %d" % (tag, item), CFAR_REL)
    assert ((raw.grad.cpu().numpy() == 0) == (want == 0)).mean() > 0.999


def test_cfar_without_grad_is_todays_path(gold):
    raw = dev(gold["ca_raw"])
    plain = ru.cfar_mask(raw, RES, diff=True)
    assert not plain.requires_grad
    with_grad = ru.cfar_mask(raw.clone().requires_grad_(True), RES, diff=True)
    assert with_grad.requires_grad and torch.equal(with_grad.detach(), plain)
    hard = ru.cfar_mask(raw.clone().requires_grad_(True), RES, diff=False)
    assert not hard.requires_grad and torch.equal(hard, ru.cfar_mask(raw, RES, diff=False))
    with torch.no_grad():
        ng = ru.cfar_mask(raw.clone().requires_grad_(True), RES, diff=True)
    assert not ng.requires_grad and torch.equal(ng, plain)


# ----------------------------------------------------------------------------- 2. extract_pc
PEAK_CASES = [(True, False), (True, True), (False, False), (False, True)]


def _peaks_inputs(gold, use_T):
    az = dev(gold["pk_az"])
    return az, torch.zeros_like(az), (dev(gold["pk_T_ab"]) if use_T else None)


@pytest.mark.parametrize("diff,use_T", PEAK_CASES)
def test_peaks_gradient_matches_reference(gold, diff, use_T):
    tag = "%d%d" % (int(diff), int(use_T))
    az, tm, T_ab = _peaks_inputs(gold, use_T)
    n, G, want = gold["pk_n" + tag], gold["pk_G" + tag], gold["pk_grad" + tag]
    # padded form
    mask = dev(gold["pk_mask"]).requires_grad_(True)
    pc, cnt = ru.extract_pc_padded(mask, RES, az, tm, int(n.max()), T_ab=T_ab, diff=diff)
    assert pc.requires_grad and not cnt.requires_grad and cnt.dtype == torch.int32
    assert cnt.cpu().tolist() == n.tolist()
    np.testing.assert_allclose(pc.detach().cpu().numpy(), gold["pk_pc" + tag], atol=2e-5)
    pc.backward(dev(G))
    close(mask.grad, want, "peaks padded diff=%d T=%d" % (diff, use_T), PEAKS_REL)
    assert (mask.grad[:, 5] == 0).all()                                  # an all-zero row
    # ragged list form: a loss on the list elements reaches the mask
    mask2 = dev(gold["pk_mask"]).requires_grad_(True)
    pcs = ru.extract_pc(mask2, RES, az, tm, T_ab=T_ab, diff=diff)
    assert [p.shape[0] for p in pcs] == n.tolist() and all(p.requires_grad for p in pcs)
    sum((p * dev(G[b, :n[b]])).sum() for b, p in enumerate(pcs)).backward()
    close(mask2.grad, want, "peaks list diff=%d T=%d" % (diff, use_T), PEAKS_REL)
    # a loss on one element only: the other item's cells get exactly 0
    mask3 = dev(gold["pk_mask"]).requires_grad_(True)
    pcs = ru.extract_pc(mask3, RES, az, tm, T_ab=T_ab, diff=diff)
    (pcs[1] * dev(G[1, :n[1]])).sum().backward()
    assert (mask3.grad[0] == 0).all() and torch.equal(mask3.grad[1], mask2.grad[1])


def _marker_cells(mask, diff):
    arr = RES * torch.arange(mask.shape[2], dtype=torch.float32) * torch.from_numpy(mask)
    return ru.mean_peaks_parallel_fast(arr, diff, 10.0).numpy() != 0


@pytest.mark.parametrize("diff", [True, False])
def test_peaks_structural_zeros(gold, diff):
    """The unpaired last marker of an odd count (the reference raises there: no golden value), points at or beyond
    max_pts, and cells that feed no marker get exactly 0; everything else is unchanged, bit for bit."""
    tag = "%d0" % int(diff)
    az, tm, _ = _peaks_inputs(gold, False)
    n, G = gold["pk_n" + tag], gold["pk_G" + tag]
    base = gold["pk_mask"]
    B, A, R = base.shape

    def grad_of(mask_np, max_pts, Gp):
        m = dev(mask_np).requires_grad_(True)
        pc, cnt = ru.extract_pc_padded(m, RES, az, tm, max_pts, diff=diff)
        pc.backward(dev(Gp))
        return m.grad, cnt.cpu().numpy()

    full, _ = grad_of(base, int(n.max()), G)
    # odd count: a blob that reaches the last column of item 1's last row leaves one marker after all pairs
    odd = base.copy()
    odd[1, A - 1, R - 2:] = [0.9950, 0.9975]
    assert _marker_cells(odd, diff)[1].sum() == _marker_cells(base, diff)[1].sum() + 1
    g_odd, cnt = grad_of(odd, int(n.max()), G)
    assert cnt.tolist() == n.tolist()
    assert torch.equal(g_odd[0], full[0])
    assert (g_odd[1, A - 1, R - 40:] == 0).all()
    keep = torch.ones(A, R, dtype=torch.bool, device=DEV)
    keep[A - 1, R - 40:] = False
    assert torch.equal(g_odd[1][keep], full[1][keep])
    # truncation: with max_pts = P the markers from 2 P on feed no point (P: the largest cut that falls, in every item,
    # between two markers that share no cell: a marker at cell p touches the cells p and p + 1)
    flat_mk = [np.flatnonzero(_marker_cells(base, diff)[b]) for b in range(B)]
    P = next(p for p in range(int(n.min()) // 2, 0, -1) if all(f[2 * p] - f[2 * p - 1] >= 4 for f in flat_mk))
    g_cut, cnt = grad_of(base, P, G[:, :P])
    assert cnt.tolist() == n.tolist()                                   # the count is the reference's, not the truncated one
    flat = torch.arange(A * R, device=DEV).reshape(A, R)
    for b in range(B):
        inside, outside = flat <= int(flat_mk[b][2 * P - 1]) + 1, flat >= int(flat_mk[b][2 * P]) - 1
        assert not (inside & outside).any()
        assert torch.equal(g_cut[b][inside], full[b][inside]) and (g_cut[b][outside] == 0).all()
        assert full[b][outside].abs().max() > 0
    # cells that feed no marker
    feeds = torch.from_numpy(_marker_cells(base, diff)).to(DEV)
    near = feeds.clone()
    near[:, :, 1:] |= feeds[:, :, :-1]
    near[:, :, :-1] |= feeds[:, :, 1:]
    near[:, :, 2:] |= feeds[:, :, :-2]
    assert (full[~near] == 0).all() and full[near].abs().max() > 0


# ----------------------------------------------------------------------------- 3. the chain
def _chain(gold, raw):
    az = dev(gold["ch_az"])
    npad, K = int(gold["ch_npad"]), int(gold["ch_iters"])
    m = ru.cfar_mask(raw, RES, diff=True)
    cloud, cnt = ru.extract_pc_padded(m, RES, az, torch.zeros_like(az), npad, diff=True)
    wmask = dev(gold["ch_mu"])[:, :, None] * dev(gold["ch_mv"])[:, None, :]
    w = ru.extract_weights(wmask, cloud)[0]
    icp = ICP(icp_type="pt2pl", differentiable=True, max_iterations=K, tolerance=1e-9)
    T = icp.icp(cloud, dev(gold["ch_map"]), weight=w, trim_dist=5.0, loss_fn={"name": "huber", "metric": 1.0}, dim=2)["T"]
    return T, cloud, cnt, w


def test_chain_pose_to_scan(gold, nn_engine):
    """pose functional -> T -> source cloud and extract_weights' scan_pc -> peak markers -> CFAR mask -> polar scan, against
    the reference's front end composed with the CPU restatement of dICP."""
    raw = dev(gold["ch_raw"]).requires_grad_(True)
    T, cloud, cnt, w = _chain(gold, raw)
    assert cnt.cpu().tolist() == gold["ch_n"].tolist()
    np.testing.assert_allclose(cloud.detach().cpu().numpy(), gold["ch_cloud"], atol=2e-5)
    np.testing.assert_allclose(w.detach().cpu().numpy(), gold["ch_w"], atol=2e-6)
    print("RATIO chain T max abs diff = %.3e" % np.abs(T.detach().cpu().numpy() - gold["ch_T"]).max())
    (T * dev(gold["ch_G"])).sum().backward()
    np.testing.assert_allclose(T.detach().cpu().numpy(), gold["ch_T"], atol=2e-6)
    for b in range(raw.shape[0]):
        close(raw.grad[b], gold["ch_grad"][b], "chain %s item %d" % (nn_engine, b), CHAIN_REL)


# ----------------------------------------------------------------------------- 4. reproducibility
def test_gradients_are_bit_reproducible(gold):
    def cfar():
        raw = dev(gold["ca_raw"]).requires_grad_(True)
        ru.cfar_mask(raw, RES, diff=True).backward(dev(gold["ca_G"]))
        return raw.grad

    def peaks(diff):
        az, tm, T_ab = _peaks_inputs(gold, True)
        tag = "%d1" % int(diff)
        m = dev(gold["pk_mask"]).requires_grad_(True)
        ru.extract_pc_padded(m, RES, az, tm, int(gold["pk_n" + tag].max()), T_ab=T_ab, diff=diff)[0].backward(dev(gold["pk_G" + tag]))
        return m.grad

    def chain():
        raw = dev(gold["ch_raw"]).requires_grad_(True)
        (_chain(gold, raw)[0] * dev(gold["ch_G"])).sum().backward()
        return raw.grad

    for name, f in (("cfar", cfar), ("peaks diff", lambda: peaks(True)), ("peaks hard", lambda: peaks(False)), ("chain", chain)):
        a, b = f(), f()
        assert torch.equal(a, b), name


# ----------------------------------------------------------------------------- 5. full size, long rows
def _front_end_grad(fft, az, Gp):
    raw = fft.clone().requires_grad_(True)
    m = ru.cfar_mask(raw, RES, diff=True)
    pc, cnt = ru.extract_pc_padded(m, RES, az, torch.zeros_like(az), Gp.shape[1], diff=True)
    m.retain_grad()
    pc.backward(Gp)
    return raw.grad, m.grad, cnt


def test_full_size_batch_items_and_rows_are_independent():
    """B = 4 scans of 400 x 3360: the gradient of one item equals, bit for bit, the gradient of that item run alone, and
    the CFAR gradient of selected rows that of the same rows run as a small batch; finite and non-zero on every item."""
    batch = synthetic.make_batch([0, 1, 2, 3], device=DEV)
    fft, az = batch["fft_polar"], batch["azimuths"]
    Gp = torch.randn(4, 5120, 3, generator=torch.Generator().manual_seed(0)).to(DEV)
    g_raw, g_mask, cnt = _front_end_grad(fft, az, Gp)
    assert torch.isfinite(g_raw).all() and torch.isfinite(g_mask).all() and (cnt > 100).all()
    for b in range(4):
        assert g_raw[b].abs().max() > 0 and g_mask[b].abs().max() > 0, b
    one_raw, one_mask, _ = _front_end_grad(fft[2:3], az[2:3], Gp[2:3])
    assert torch.equal(one_mask[0], g_mask[2]) and torch.equal(one_raw[0], g_raw[2])
    rows = torch.tensor([0, 7, 133, 399], device=DEV)
    sub = fft[1, rows][None].clone().requires_grad_(True)
    ru.cfar_mask(sub, RES, diff=True).backward(g_mask[1, rows][None].contiguous())
    assert torch.equal(sub.grad[0], g_raw[1, rows])


@pytest.mark.parametrize("R", [4000, 4500])
def test_cfar_gradient_long_rows(R):
    """Rows beyond the persistent forward kernel's LDS budget (R = 4000, as test_gpu_radar.py) and beyond eight cells per
    thread (R = 4500: the backward's long-row instance).  No window of a cell in [mincol, maxcol) reaches column 3360, so
    the first 3360 columns' gradient is that of the scan cut to 3360 columns (to rounding: other kernel instances sum the
    prefixes of k in another partition)."""
    rng = np.random.default_rng(11)
    raw = rng.random((2, 5, R), dtype=np.float32) * 0.04
    for c in range(150, 1250, 37):
        raw[:, :, c:c + 3] += rng.uniform(0.1, 0.4, (2, 5, 3)).astype(np.float32)
    G = rng.normal(size=raw.shape).astype(np.float32)
    x = dev(raw).requires_grad_(True)
    m = ru.cfar_mask(x, RES, diff=True)
    m.backward(dev(G))
    assert torch.isfinite(x.grad).all() and x.grad.abs().max() > 0
    x2 = dev(raw[:, :, :3360]).requires_grad_(True)
    m2 = ru.cfar_mask(x2, RES, diff=True)
    m2.backward(dev(G[:, :, :3360]))
    assert (x.grad[:, :, 3360:] == 0).all()
    close(x.grad[:, :, :3360], x2.grad.cpu().numpy(), "cfar long rows R=%d vs 3360" % R, 1e-6)
    # and the peaks backward on a long row
    az = torch.linspace(0.1, 6.0, 5, device=DEV).repeat(2, 1)
    mm = m.detach().clone().requires_grad_(True)
    pc, cnt = ru.extract_pc_padded(mm, RES, az, torch.zeros_like(az), 512, diff=True)
    pc.backward(torch.ones_like(pc))
    assert (cnt > 10).all() and torch.isfinite(mm.grad).all() and mm.grad.abs().max() > 0


# ----------------------------------------------------------------------------- 6. dtype and device
def test_cpu_tensors_in_cpu_gradients_out(gold):
    raw = torch.from_numpy(gold["ca_raw"]).double().requires_grad_(True)
    m = ru.cfar_mask(raw, RES, diff=True)
    assert m.device.type == "cpu" and m.requires_grad
    m.backward(torch.from_numpy(gold["ca_G"]))
    assert raw.grad.device.type == "cpu" and raw.grad.dtype == torch.float64
    on_dev = dev(gold["ca_raw"]).requires_grad_(True)
    ru.cfar_mask(on_dev, RES, diff=True).backward(dev(gold["ca_G"]))
    assert torch.equal(raw.grad, on_dev.grad.cpu().double())

    az, tm, _ = _peaks_inputs(gold, False)
    mask = torch.from_numpy(gold["pk_mask"]).double().requires_grad_(True)
    pcs = ru.extract_pc(mask, RES, az.cpu(), tm.cpu(), diff=True)
    assert all(p.device.type == "cpu" for p in pcs)
    sum(p.sum() for p in pcs).backward()
    assert mask.grad.device.type == "cpu" and mask.grad.dtype == torch.float64 and mask.grad.abs().max() > 0
