"""GPU: the GO-CFAR thresholds as tensors -- radar_utils.cfar_mask with a_thresh / b_thresh on the device (mmk_cfar_mask_p)
and their gradients (mmk_cfar_mask_bwd_p) against the reference's own autograd through ``thres = a_thresh * stat + b_thresh``
(tests/golden/cfar_params.npz, written by tests/golden/make_golden_cfar_params.py), against the fp64 restatement of
tests/radar_cases.py where there is no golden value, and the policy switch params["learn_cfar"].

Bit equalities: the tensor path hands the same two floats to the same expression as the number path, so masks and scan
gradients are torch.equal; the threshold sums are fp64 in a fixed order, so they are equal from run to run, with and without the
scan's gradient, and per scan whatever the rest of the batch holds.

Tolerances.  A threshold gradient is a sum of the k_c the scan gradient is made of, so it is compared with the
fp64 reference relative to its scale (the same sum with |G|: every term has one sign) under the bound those k_c already meet
against the device-versus-host tanhf difference, CFAR_REL = 1.6e-5 of test_gpu_radar_grads.py; the chain keeps that file's
CHAIN_REL = 1.6e-5.  Measured on an MI355X, beside the reference's own fp32 rounding e32 stored in the fixture:

    case                               worst |got - ref| / scale       the fixture's e32 (worst)
    set 0, shared / per scan           6.3e-7 / 1.5e-6                 2.1e-7 / 1.9e-6
    set 1, shared / per scan           1.5e-7 / 1.1e-6                 1.4e-7 / 2.1e-6
    long rows R = 4000 / 4500          6.7e-7 / 3.5e-7                 (against the fp64 restatement)
    full size 2 x 400 x 3360, shared   1.0e-8                          (against the fp64 restatement)
    chain, both NN engines             2.4e-6                          (against the reference's fp32 chain)
"""

import numpy as np
import pytest
import torch

from mm_masking_amd import radar_utils as ru
from mm_masking_amd.dICP.ICP import ICP
from radar_cases import CASES, RES, geom_of, load_fixture, scene64, threshold_grads_f64  # noqa: F401  (scene64: a module fixture)
from support import DEV, dev, nn_engine, policy, policy_params  # noqa: F401  (nn_engine: a fixture)

pytestmark = pytest.mark.gpu
CFAR_REL = 1.6e-5
CHAIN_REL = 1.6e-5


@pytest.fixture(scope="module")
def gold(golden_dir):
    return load_fixture(golden_dir)


def _thresholds(gold, key, grad=True):
    """The case's thresholds as device tensors: 0-dim when shared; a as (B,) and b as (B,1,1) per scan."""
    if key[1] == "s":
        a, b = (torch.tensor(float(gold[k + key]), dtype=torch.float32, device=DEV) for k in ("cp_a", "cp_b"))
    else:
        a, b = dev(gold["cp_a" + key]), dev(gold["cp_b" + key]).reshape(-1, 1, 1)
    return a.requires_grad_(grad), b.requires_grad_(grad)


def _number_path(gold, key, raw, diff=True, G=None):
    """The mask (and with G the scan gradient) of the number path with the case's values: one call when they are shared,
    one call per scan stacked otherwise."""
    a, b = np.atleast_1d(gold["cp_a" + key]), np.atleast_1d(gold["cp_b" + key])
    groups = [slice(0, raw.shape[0])] if key[1] == "s" else [slice(i, i + 1) for i in range(raw.shape[0])]
    masks, grads = [], []
    for i, sl in enumerate(groups):
        x = raw[sl].clone().requires_grad_(G is not None)
        m = ru.cfar_mask(x, RES, a_thresh=float(a[i]), b_thresh=float(b[i]), diff=diff, **geom_of(gold, key))
        if G is not None:
            m.backward(G[sl].contiguous())
            grads.append(x.grad)
        masks.append(m.detach())
    return torch.cat(masks), (torch.cat(grads) if grads else None)


def _ratios(got, ref64, scale, name):
    r = np.abs(got.detach().cpu().double().numpy().reshape(-1) - ref64.reshape(-1)) / scale.reshape(-1)
    print("RATIO %-44s |got - ref| / scale = %s" % (name, " ".join("%.3e" % v for v in r)))
    return r


@pytest.fixture(scope="module")
def runs(gold):
    """One forward and backward per case with scan and thresholds requiring grad; shared by the tests below."""
    out = {}
    raw, G = dev(gold["cp_raw"]), dev(gold["cp_G"])
    for key in CASES:
        x = raw.clone().requires_grad_(True)
        a, b = _thresholds(gold, key)
        m = ru.cfar_mask(x, RES, a_thresh=a, b_thresh=b, diff=True, **geom_of(gold, key))
        m.backward(G)
        out[key] = {"mask": m.detach(), "a": a, "b": b, "x": x}
    return out


# ----------------------------------------------------------------------------- 1. forward bits
@pytest.mark.parametrize("key", CASES)
@pytest.mark.parametrize("diff", [True, False])
def test_forward_bits_equal_the_number_path(gold, key, diff):
    raw = dev(gold["cp_raw"])
    want, _ = _number_path(gold, key, raw, diff=diff)
    assert want.abs().max() > 0
    a, b = _thresholds(gold, key, grad=False)
    got = ru.cfar_mask(raw, RES, a_thresh=a, b_thresh=b, diff=diff, **geom_of(gold, key))
    assert torch.equal(got, want) and not got.requires_grad and got.grad_fn is None
    # other admitted forms of the same values: host tensors, (1,) / (B,) / (B,1,1), a number mixed with a tensor
    B = raw.shape[0]
    if key[1] == "s":
        forms = [(a.cpu().reshape(1), b.double()), (float(a), b.expand(B).contiguous()), (a.expand(B).reshape(B, 1, 1), float(b))]
    else:
        forms = [(a.cpu().reshape(B, 1, 1), b.reshape(B).double())]
    for fa, fb in forms:
        assert torch.equal(ru.cfar_mask(raw, RES, a_thresh=fa, b_thresh=fb, diff=diff, **geom_of(gold, key)), want)
    # diff=False never requires grad; diff=True does as soon as a threshold does
    a, b = _thresholds(gold, key)
    m = ru.cfar_mask(raw, RES, a_thresh=a, b_thresh=b, diff=diff, **geom_of(gold, key))
    assert m.requires_grad == diff and torch.equal(m.detach(), want)
    with torch.no_grad():
        assert not ru.cfar_mask(raw, RES, a_thresh=a, b_thresh=b, diff=True, **geom_of(gold, key)).requires_grad


# ----------------------------------------------------------------------------- 2. gradients against the reference
@pytest.mark.parametrize("key", CASES)
def test_threshold_gradients_match_reference(gold, runs, key):
    r = runs[key]
    a, b, x = r["a"], r["b"], r["x"]
    B = x.shape[0]
    assert a.grad.shape == a.shape == (() if key[1] == "s" else (B,)) and a.grad.dtype == torch.float32 and a.grad.is_cuda
    assert b.grad.shape == b.shape == (() if key[1] == "s" else (B, 1, 1)) and b.grad.dtype == torch.float32
    ra = _ratios(a.grad, gold["cp_ga64_" + key], gold["cp_sa_" + key], "case %s a_thresh" % key)
    rb = _ratios(b.grad, gold["cp_gb64_" + key], gold["cp_sb_" + key], "case %s b_thresh" % key)
    print("      the reference's own fp32 rounding e32: a %s  b %s" % (gold["cp_ea32_" + key], gold["cp_eb32_" + key]))
    assert (ra <= CFAR_REL).all() and (rb <= CFAR_REL).all(), (key, ra, rb)
    # the scan's gradient and the mask are the number path's, bit for bit
    want_mask, want_grad = _number_path(gold, key, dev(gold["cp_raw"]), G=dev(gold["cp_G"]))
    assert torch.equal(r["mask"], want_mask) and torch.equal(x.grad, want_grad) and x.grad.abs().max() > 0


def test_gradients_come_back_in_the_thresholds_form(gold, runs):
    """Host fp64 thresholds get host fp64 gradients; a single value used with per-scan values gets the sum over the scans."""
    raw, G = dev(gold["cp_raw"]), dev(gold["cp_G"])
    a = torch.from_numpy(gold["cp_a0p"]).double().requires_grad_(True)
    b = torch.tensor(float(gold["cp_b0s"]), device=DEV, requires_grad=True)
    ru.cfar_mask(raw, RES, a_thresh=a, b_thresh=b, diff=True).backward(G)
    assert a.grad.shape == (3,) and a.grad.dtype == torch.float64 and a.grad.device.type == "cpu"
    assert b.grad.shape == () and b.grad.is_cuda
    a2 = dev(gold["cp_a0p"]).requires_grad_(True)
    b2 = b.detach().expand(3).clone().requires_grad_(True)
    ru.cfar_mask(raw, RES, a_thresh=a2, b_thresh=b2, diff=True).backward(G)
    assert torch.equal(a.grad, a2.grad.cpu().double()) and torch.equal(b.grad, b2.grad.sum())


# ----------------------------------------------------------------------------- 3. thresholds only
@pytest.mark.parametrize("key", CASES)
def test_thresholds_only_skip_the_scan_gradient(gold, runs, key):
    raw = dev(gold["cp_raw"])
    a, b = _thresholds(gold, key)
    m = ru.cfar_mask(raw, RES, a_thresh=a, b_thresh=b, diff=True, **geom_of(gold, key))
    assert m.requires_grad and torch.equal(m.detach(), runs[key]["mask"])
    m.backward(dev(gold["cp_G"]))
    assert torch.equal(a.grad, runs[key]["a"].grad) and torch.equal(b.grad, runs[key]["b"].grad)
    assert a.grad.abs().min() > 0 and b.grad.abs().min() > 0
    # one threshold alone
    a1, _ = _thresholds(gold, key)
    ru.cfar_mask(raw, RES, a_thresh=a1, b_thresh=b.detach(), diff=True, **geom_of(gold, key)).backward(dev(gold["cp_G"]))
    assert torch.equal(a1.grad, a.grad)


# ----------------------------------------------------------------------------- 4. structure
@pytest.mark.parametrize("key", ["0p", "1p"])
def test_structure_zero_scan_batch_independence_and_reproducibility(gold, runs, key):
    raw, G = dev(gold["cp_raw"]), dev(gold["cp_G"])
    kw = geom_of(gold, key)

    def grads(x, sel, with_scan=True):
        x = x.clone().requires_grad_(with_scan)
        a = dev(np.atleast_1d(gold["cp_a" + key])[sel]).requires_grad_(True)
        b = dev(np.atleast_1d(gold["cp_b" + key])[sel]).requires_grad_(True)
        ru.cfar_mask(x, RES, a_thresh=a, b_thresh=b, diff=True, **kw).backward(G[sel].contiguous())
        return a.grad, b.grad, x.grad

    full = grads(raw, [0, 1, 2])
    assert torch.equal(full[0], runs[key]["a"].grad) and torch.equal(full[1], runs[key]["b"].grad.reshape(-1))
    # an all-zero scan in the batch: exactly 0 for it, the others unchanged
    zeroed = raw.clone()
    zeroed[1] = 0.0
    za, zb, _ = grads(zeroed, [0, 1, 2])
    assert za[1].item() == 0.0 and zb[1].item() == 0.0
    assert torch.equal(za[[0, 2]], full[0][[0, 2]]) and torch.equal(zb[[0, 2]], full[1][[0, 2]])
    # item i of the batch of three == item i alone
    for i in range(3):
        ia, ib, ix = grads(raw[i:i + 1], [i])
        assert torch.equal(ia[0], full[0][i]) and torch.equal(ib[0], full[1][i]) and torch.equal(ix[0], full[2][i])
    # run to run
    again = grads(raw, [0, 1, 2])
    assert all(torch.equal(p, q) for p, q in zip(full, again))


# ----------------------------------------------------------------------------- 5. long rows, the row reduction
def _conditioned_scan(seed, shape, last_return):
    """Noise with three-cell returns every 37 columns (test_gpu_radar_grads.test_cfar_gradient_long_rows), changed by the
    generator's nudge() until no cell lies within 1e-4 of the gate: the fp64 restatement then keeps the device's cells."""
    from make_golden_radar_grads import nudge
    rng = np.random.default_rng(seed)
    raw = rng.random(shape, dtype=np.float32) * 0.04
    for c in range(150, last_return, 37):
        raw[:, :, c:c + 3] += rng.uniform(0.1, 0.4, shape[:2] + (3,)).astype(np.float32)
    return nudge(raw, ({},)), rng.normal(size=shape).astype(np.float32)


def _against_restatement(raw, G, name, per_scan):
    B = raw.shape[0]
    av, bv = np.full(B, 1.0), np.full(B, np.float32(0.09), dtype=np.float64)
    a = dev(av.astype(np.float32) if per_scan else np.float32(1.0)).requires_grad_(True)
    b = dev(bv.astype(np.float32) if per_scan else np.float32(0.09)).requires_grad_(True)
    x = dev(raw).requires_grad_(True)
    ru.cfar_mask(x, RES, a_thresh=a, b_thresh=b, diff=True).backward(dev(G))
    ga, gb = threshold_grads_f64(raw, G, av, bv)
    sa, sb = threshold_grads_f64(raw, np.abs(G), av, bv)
    if not per_scan:
        ga, gb, sa, sb = (v.sum(keepdims=True) for v in (ga, gb, sa, sb))
    assert (np.abs(sa) > 0).all() and (np.abs(sb) > 0).all()
    ra = _ratios(a.grad, ga, np.abs(sa), name + " a_thresh")
    rb = _ratios(b.grad, gb, np.abs(sb), name + " b_thresh")
    assert (ra <= CFAR_REL).all() and (rb <= CFAR_REL).all(), (name, ra, rb)
    # the scan gradient is the number path's here too
    x2 = dev(raw).requires_grad_(True)
    ru.cfar_mask(x2, RES, diff=True).backward(dev(G))
    assert torch.equal(x.grad, x2.grad)


@pytest.mark.parametrize("R", [4000, 4500])
def test_long_rows_against_restatement(R):
    """R = 4000: beyond the persistent forward kernel's LDS budget (the one-row forward kernel); R = 4500: beyond eight cells
    per thread (the backward's long-row instance)."""
    raw, G = _conditioned_scan(11, (1, 4, R), 1250)
    _against_restatement(raw, G, "long rows R=%d" % R, per_scan=True)


def test_full_size_shared_thresholds_against_restatement():
    """B = 2 scans of 400 x 3360 with shared thresholds: the final kernel adds 800 row partials."""
    raw, G = _conditioned_scan(12, (2, 400, 3360), 1250)
    _against_restatement(raw, G, "full size 2 x 400 x 3360", per_scan=False)


# ----------------------------------------------------------------------------- 6. the chain
def test_chain_pose_to_thresholds(gold, nn_engine):
    az = dev(gold["ch_az"])
    npad, K = int(gold["ch_npad"]), int(gold["ch_iters"])
    a = dev(gold["cc_a"]).reshape(-1, 1, 1).requires_grad_(True)
    b = dev(gold["cc_b"]).reshape(-1, 1, 1).requires_grad_(True)
    m = ru.cfar_mask(dev(gold["cc_raw"]), RES, a_thresh=a, b_thresh=b, diff=True)
    cloud, cnt = ru.extract_pc_padded(m, RES, az, torch.zeros_like(az), npad, diff=True)
    wmask = dev(gold["ch_mu"])[:, :, None] * dev(gold["ch_mv"])[:, None, :]
    w = ru.extract_weights(wmask, cloud)[0]
    icp = ICP(icp_type="pt2pl", differentiable=True, max_iterations=K, tolerance=1e-9)
    T = icp.icp(cloud, dev(gold["ch_map"]), weight=w, trim_dist=5.0, loss_fn={"name": "huber", "metric": 1.0}, dim=2)["T"]
    assert cnt.cpu().tolist() == gold["cc_n"].tolist()
    np.testing.assert_allclose(cloud.detach().cpu().numpy(), gold["cc_cloud"], atol=2e-5)
    np.testing.assert_allclose(T.detach().cpu().numpy(), gold["cc_T"], atol=2e-6)
    (T * dev(gold["ch_G"])).sum().backward()
    ra = _ratios(a.grad, gold["cc_ga"].astype(np.float64), gold["cc_sa"], "chain %s a_thresh" % nn_engine)
    rb = _ratios(b.grad, gold["cc_gb"].astype(np.float64), gold["cc_sb"], "chain %s b_thresh" % nn_engine)
    assert a.grad.shape == a.shape and (ra <= CHAIN_REL).all() and (rb <= CHAIN_REL).all(), (nn_engine, ra, rb)


# ----------------------------------------------------------------------------- 7. the policy
def test_policy_learns_the_thresholds(scene64, tmp_path):
    from mm_masking_amd import train_icp_weights as trn
    scan, mp, T0, G = scene64
    model = policy(DEV, 3, dropout=0.0, mask_target="scan", learn_cfar=True)
    assert len(list(model.parameters())) == 48 and model.cfar_a.is_cuda
    model.train()
    T, mask, _ = model(scan, mp, T0)
    (T * G).sum().backward()
    ga, gb = model.cfar_a.grad.clone(), model.cfar_b.grad.clone()
    print("POLICY cfar_a.grad %.6e cfar_b.grad %.6e" % (ga.item(), gb.item()))
    assert ga.shape == () and torch.isfinite(ga) and torch.isfinite(gb) and ga.item() != 0.0 and gb.item() != 0.0
    # the same operators called by hand
    a = model.cfar_a.detach().clone().requires_grad_(True)
    b = model.cfar_b.detach().clone().requires_grad_(True)
    masked = ru.mask_polar_scan(scan["fft_polar"], mask.detach(), scan["azimuths"], model.res)
    m = ru.cfar_mask(masked, model.res, a_thresh=a, b_thresh=b, diff=True)
    az = scan["azimuths"].to(DEV)
    cloud, _ = ru.extract_pc_padded(m, model.res, az, torch.zeros_like(az), max_pts=scan["raw_pc"].shape[1], diff=True)
    T2 = model.icp(cloud, mp["pc"], T0, None)
    (T2 * G).sum().backward()
    assert torch.equal(T2.detach(), T.detach()) and torch.equal(a.grad, ga) and torch.equal(b.grad, gb)
    # the U-Net's 46 gradients and the pose are those of a policy with the same values as numbers
    plain = policy(DEV, 3, dropout=0.0, mask_target="scan")
    assert (np.float32(plain.a_thres), np.float32(plain.b_thres)) == (model.cfar_a.item(), model.cfar_b.item())
    plain.train()
    Tp = plain(scan, mp, T0)[0]
    (Tp * G).sum().backward()
    assert torch.equal(Tp.detach(), T.detach())
    mine, theirs = dict(model.named_parameters()), dict(plain.named_parameters())
    assert len(theirs) == 46 and set(mine) - set(theirs) == {"cfar_a", "cfar_b"}
    for k, q in theirs.items():
        assert torch.equal(mine[k].grad, q.grad), k
    assert any(q.grad.abs().max() > 0 for q in theirs.values())
    # one Adam step moves both; a checkpoint restores them
    params = policy_params(DEV, dropout=0.0, mask_target="scan", learn_cfar=True)
    opt = trn.make_optimizer(model, params)
    before = (model.cfar_a.item(), model.cfar_b.item())
    opt.step()
    assert model.cfar_a.item() != before[0] and model.cfar_b.item() != before[1]
    trn.save_checkpoint(str(tmp_path / "ck.pt"), model, opt, epoch=0, best_norm=1.0)
    other = policy(DEV, 5, dropout=0.0, mask_target="scan", learn_cfar=True)
    assert other.cfar_a.item() == before[0]
    trn.load_checkpoint(str(tmp_path / "ck.pt"), other, trn.make_optimizer(other, params))
    assert torch.equal(other.cfar_a, model.cfar_a) and torch.equal(other.cfar_b, model.cfar_b)
    assert all(torch.equal(p, q) for p, q in zip(model.state_dict().values(), other.state_dict().values()))
