"""GPU: the Cartesian mask applied to the polar scan in one kernel (radar_utils.mask_polar_scan: mmk_mask_polar_scan and
mmk_mask_polar_scan_bwd) and the policy mode built on it (LearnICPWeightPolicy, params["mask_target"] = "scan"), against the
reference's own CPU autograd (tests/golden/mask_scan.npz, written by tests/golden/make_golden_mask_scan.py) and against the
composition of the operators that existed before, `radar_cartesian_to_polar(mask.double(), ...).float() * scan`.

Tolerances.
  golden forward            2^-23 absolute: values are below 1, and the fixture may come from a host whose sin / cos differ in
                            the last fp64 bit, which can move the one fp32 rounding of the polar mask.
  golden gradients          2^-23 of max|ref| per item: one fp32 rounding of an fp64 value that differs from the reference's by
                            the fixed-point resolution (2^-54 of the largest product for ms_a) and the summation order only.
  fused against composed    none: torch.equal.  The sums are integers, so equality follows from the same products and the same
                            scale rule.
  chain (ms_ch_*)           cloud 2e-5 and T 2e-6 absolute, the existing chain's bounds for the same front end
                            (test_gpu_resample_grads.py); the gradient at the mask max |got - ref| / max |ref| per item, asserted
                            at CHAIN_MASK_REL.  Measured on an MI355X (T: 5.4e-7 from the golden pose, both engines):

                                engine   item 0      item 1
                                brute    2.591e-6    1.709e-6
                                grid     2.591e-6    1.709e-6

                            CHAIN_MASK_REL = 1.04e-5 = 4 x the worst ratio, the convention of test_gpu_resample_grads.py; the
                            project's ceiling for anything behind the dICP backward is 2e-3.
"""
import importlib

import numpy as np
import pytest
import torch

from mm_masking_amd import radar_utils as ru
from radar_cases import B64, H64, NP64, RES, chain_inputs, scene64, wobbly_azimuths  # noqa: F401  (scene64: a module fixture)
from support import DEV, dev, load_golden, nn_engine, policy  # noqa: F401  (nn_engine: a fixture)

pytestmark = pytest.mark.gpu
ULP = 2.0 ** -23
CHAIN_MASK_REL = 1.04e-5


@pytest.fixture(scope="module")
def gold(golden_dir):
    return load_golden(golden_dir, "mask_scan.npz")


@pytest.fixture(scope="module")
def chain_in(golden_dir):
    return chain_inputs(golden_dir)


def _case(gold, key):
    rres, cres = (float(v) for v in gold[key + "_res"])
    return dev(gold[key + "_scan"]), dev(gold[key + "_mask"]), torch.from_numpy(gold[key + "_az"]), dev(gold[key + "_G"]), rres, cres


def _full_size_case():
    g = torch.Generator().manual_seed(91)
    scan = torch.rand(2, 400, 3360, generator=g).to(DEV)
    mask = torch.rand(2, 640, 640, generator=g).to(DEV)
    G = torch.randn(2, 400, 3360, generator=g).to(DEV)
    az = torch.cat([wobbly_azimuths(5), wobbly_azimuths(6)])
    return scan, mask, az, G, RES, 0.2384


def _fused(scan, mask, az, G, rres, cres, grad_scan=True, grad_mask=True):
    s, m = scan.clone().requires_grad_(grad_scan), mask.clone().requires_grad_(grad_mask)
    y = ru.mask_polar_scan(s, m, az, rres, cart_resolution=cres)
    y.backward(G)
    return y.detach(), s.grad, m.grad


def _composed(scan, mask, az, G, rres, cres, grad_scan=True, grad_mask=True):
    s, m = scan.clone().requires_grad_(grad_scan), mask.clone().requires_grad_(grad_mask)
    y = ru.radar_cartesian_to_polar(m.double(), az, rres, cart_resolution=cres, polar_pixel_shape=tuple(scan.shape[1:])).float() * s
    y.backward(G)
    return y.detach(), s.grad, m.grad


@pytest.fixture(scope="module")
def full_size():
    """Inputs, the composition and two fused runs at 640 x 640 -> 400 x 3360, B = 2, non-uniform azimuths; computed once."""
    case = _full_size_case()
    return {"case": case, "composed": _composed(*case), "fused": _fused(*case), "again": _fused(*case)}


# ----------------------------------------------------------------------------- 1. against the golden vectors
@pytest.mark.parametrize("key", ["ms_a", "ms_b"])
def test_forward_and_gradients_match_reference(gold, key):
    scan, mask, az, G, rres, cres = _case(gold, key)
    y, gs, gm = _fused(scan, mask, az, G, rres, cres)
    assert y.dtype == gs.dtype == gm.dtype == torch.float32 and y.shape == scan.shape and gm.shape == mask.shape
    err = (y.cpu().double().numpy() - gold[key + "_y"]).__abs__().max()
    print("FORWARD %s max abs diff = %.3e" % (key, err))
    assert err <= ULP
    for name, got, want in (("grad_scan", gs, gold[key + "_grad_scan"]), ("grad_mask", gm, gold[key + "_grad_mask"])):
        for b in range(want.shape[0]):
            scale = np.abs(want[b]).max()
            r = np.abs(got[b].cpu().double().numpy() - want[b]).max() / scale
            print("RATIO %s %s item %d err/scale = %.3e (scale %.3e)" % (key, name, b, r, scale))
            assert scale > 0 and r <= ULP, (key, name, b, r)


# ----------------------------------------------------------------------------- 2. fused == composed, bit for bit
@pytest.mark.parametrize("key", ["ms_a", "ms_b"])
@pytest.mark.parametrize("which", ["both", "scan", "mask"])
def test_fused_equals_composed_bitwise(gold, key, which):
    case = _case(gold, key)
    kw = {"grad_scan": which != "mask", "grad_mask": which != "scan"}
    (y, gs, gm), (yc, gsc, gmc) = _fused(*case, **kw), _composed(*case, **kw)
    assert torch.equal(y, yc)
    assert (gs is None) == (which == "mask") and (gm is None) == (which == "scan")
    assert gs is None or torch.equal(gs, gsc)
    assert gm is None or torch.equal(gm, gmc)


def test_fused_equals_composed_bitwise_at_full_size(full_size):
    (y, gs, gm), (yc, gsc, gmc) = full_size["fused"], full_size["composed"]
    assert torch.equal(y, yc) and torch.equal(gs, gsc) and torch.equal(gm, gmc)
    assert y.abs().max() > 0 and gs.abs().max() > 0 and gm.abs().max() > 0


@pytest.mark.parametrize("which", ["scan", "mask"])
def test_one_sided_gradients_at_full_size(full_size, which):
    kw = {"grad_scan": which == "scan", "grad_mask": which == "mask"}
    y, gs, gm = _fused(*full_size["case"], **kw)
    assert torch.equal(y, full_size["fused"][0])
    if which == "scan":
        assert gm is None and torch.equal(gs, full_size["fused"][1])
    else:
        assert gs is None and torch.equal(gm, full_size["fused"][2])


# ----------------------------------------------------------------------------- 3. structural zeros
def test_structural_zeros(gold):
    for key in ("ms_a", "ms_b"):
        y, gs, gm = _fused(*_case(gold, key))
        notap = dev(gold[key + "_notap"])
        assert notap.float().mean() > 0.1
        assert (y[notap] == 0).all() and (gs[notap] == 0).all() and (y[~notap] != 0).float().mean() > 0.99
        untouched = dev(gold[key + "_grad_mask"] == 0)
        assert untouched.float().mean() > 0.4
        assert (gm[untouched] == 0).all() and (gm[~untouched] != 0).float().mean() > 0.99


# ----------------------------------------------------------------------------- 4. reproducibility
def test_full_size_backward_is_bit_reproducible(full_size):
    first, second = full_size["fused"], full_size["again"]
    for a, b in zip(first, second):
        assert torch.isfinite(a).all() and torch.equal(a, b)
    # the four pixels at the sensor collect the first samples of all 400 rays
    centre = first[2][:, 319:321, 319:321]
    assert torch.equal(centre, second[2][:, 319:321, 319:321]) and centre.abs().min() > 0


def test_non_finite_product_makes_its_item_nan(gold):
    scan, mask, az, G, rres, cres = _case(gold, "ms_a")
    G = G.clone()
    G[1, 3, 7] = float("inf")
    _, gs, gm = _fused(scan, mask, az, G, rres, cres)
    assert torch.isfinite(gm[0]).all() and torch.isnan(gm[1]).all()
    assert torch.equal(gm[0], _fused(*_case(gold, "ms_a"))[2][0])
    _, gsc, gmc = _composed(scan, mask, az, G, rres, cres)
    assert torch.equal(gs, gsc) and torch.isinf(gs[1, 3, 7])    # (the cell lies in the image: inf * fl32(P) = inf in both)
    assert torch.isnan(gmc[1]).all()


# ----------------------------------------------------------------------------- 5. dtype and device
def test_dtype_device_and_no_grad_paths(gold):
    scan, mask, az, G, rres, cres = _case(gold, "ms_a")
    s = torch.from_numpy(gold["ms_a_scan"]).double().requires_grad_(True)
    m = torch.from_numpy(gold["ms_a_mask"]).double().requires_grad_(True)
    y = ru.mask_polar_scan(s, m, az, rres, cart_resolution=cres)
    assert y.device.type == "cpu" and y.dtype == torch.float32 and y.requires_grad
    y.backward(torch.from_numpy(gold["ms_a_G"]))
    yd, gs, gm = _fused(scan, mask, az, G, rres, cres)
    assert torch.equal(y.detach(), yd.cpu())
    for got, on_dev in ((s.grad, gs), (m.grad, gm)):
        assert got.device.type == "cpu" and got.dtype == torch.float64 and torch.equal(got, on_dev.cpu().double())
    # requires_grad=False and no_grad(): a single launch, no graph
    assert ru.mask_polar_scan(scan, mask, az, rres, cart_resolution=cres).grad_fn is None
    with torch.no_grad():
        out = ru.mask_polar_scan(scan.clone().requires_grad_(True), mask, az, rres, cart_resolution=cres)
    assert out.grad_fn is None and not out.requires_grad and torch.equal(out, yd)
    with pytest.raises(ValueError, match="azimuths"):
        ru.mask_polar_scan(scan, mask, az[:, :-1], rres)


# ----------------------------------------------------------------------------- 6. + 9. the policy at 64 x 64
def _front_end(model, scan, mask):
    masked = ru.mask_polar_scan(scan["fft_polar"], mask, scan["azimuths"], model.res)
    m = ru.cfar_mask(masked, model.res, a_thresh=model.a_thres, b_thresh=model.b_thres, diff=True)
    az = scan["azimuths"].to(DEV)
    return ru.extract_pc_padded(m, model.res, az, torch.zeros_like(az), max_pts=scan["raw_pc"].shape[1], diff=True)


def test_policy_scan_mode_equals_manual_composition(scene64):
    scan, mp, T0, G = scene64
    model = policy(DEV, 3, dropout=0.0, mask_target="scan")
    model.train()
    T, mask, _ = model(scan, mp, T0)
    assert mask.shape == (B64, H64, H64) and T.requires_grad
    assert torch.is_tensor(model.mean_scan_pts) and model.mean_scan_pts.is_cuda
    (T * G).sum().backward()
    through = [q.grad.detach().clone() for q in model.parameters()]
    model.zero_grad(set_to_none=True)

    mask2 = model(scan, mp, T0, mask_only=True)
    assert torch.equal(mask2.detach(), mask.detach())
    cloud, cnt = _front_end(model, scan, mask2)
    print("POLICY 64 x 64: points per item %s" % cnt.cpu().tolist())
    assert cnt.min() >= 8 and cnt.max() <= NP64
    assert model.mean_scan_pts.item() == cnt.float().mean().item()
    T2 = model.icp(cloud, mp["pc"], T0, None)
    assert torch.equal(T2.detach(), T.detach())
    (T2 * G).sum().backward()
    manual = [q.grad.detach() for q in model.parameters()]
    assert len(through) == len(manual) and any(t.abs().max() > 0 for t in through)
    for t, f in zip(through, manual):
        assert torch.isfinite(t).all() and torch.equal(t, f)

    # evaluation: the inference ICP on the same cloud
    model.eval()
    with torch.no_grad():
        Te, mask_e, _ = model(scan, mp, T0)
        cloud_e, cnt_e = _front_end(model, scan, mask_e)
        assert torch.equal(cloud_e, cloud.detach()) and torch.equal(cnt_e, cnt)
        assert Te.grad_fn is None and torch.equal(Te, model.icp(cloud_e, mp["pc"], T0, None))
    # training without the ICP terms returns T_init, as the default mode does
    model.train()
    model.use_ICP_4_train = False
    assert model(scan, mp, T0)[0] is T0


def test_policy_scan_mode_needs_the_polar_scan(scene64):
    scan, mp, T0, _ = scene64
    model = policy(DEV, 3, dropout=0.0, mask_target="scan")
    for key in ("fft_polar", "azimuths"):
        with pytest.raises(KeyError, match=key):
            model({k: v for k, v in scan.items() if k != key}, mp, T0)


def test_default_mode_is_untouched(scene64):
    scan, mp, T0, G = scene64
    outs = []
    for kw in ({}, {"mask_target": "weights"}):
        model = policy(DEV, 3, dropout=0.0, **kw)
        model.train()
        T, mask, num = model(scan, mp, T0)
        ((T * G).sum() + num).backward()
        outs.append((T.detach(), mask.detach(), num.detach(), [q.grad.detach() for q in model.parameters()]))
    (T1, m1, n1, g1), (T2, m2, n2, g2) = outs
    assert torch.equal(T1, T2) and torch.equal(m1, m2) and torch.equal(n1, n2)
    assert any(g.abs().max() > 0 for g in g1) and all(torch.equal(a, b) for a, b in zip(g1, g2))


# ----------------------------------------------------------------------------- 7. the policy on the golden chain
def test_policy_override_mask_matches_reference_chain(gold, chain_in, nn_engine):
    K, npad = chain_in["iters"], chain_in["npad"]
    model = policy(DEV, 3, dropout=0.0, mask_target="scan", icp_type="pt2pl", icp_loss_fn={"name": "huber", "metric": 1.0},
                   max_iter=K, norm_weights=False)
    model.ICP_alg.tolerance = 1e-9                              # the chain's: all K iterations run
    model.train()
    B = chain_in["raw"].shape[0]
    c = (dev(chain_in["cu"])[:, :, None] * dev(chain_in["cv"])[:, None, :]).contiguous().requires_grad_(True)
    scan = {"fft_data": torch.zeros(B, 64, 64, device=DEV), "fft_cfar": torch.zeros(B, 64, 64, device=DEV),
            "raw_pc": torch.zeros(B, npad, 3, device=DEV), "fft_polar": dev(chain_in["raw"]), "azimuths": torch.from_numpy(chain_in["az"])}
    T, mask, _ = model(scan, {"pc": dev(chain_in["map"])}, torch.eye(4, device=DEV).repeat(B, 1, 1), override_mask=c)
    assert mask is c
    cloud, cnt = _front_end(model, scan, c.detach())
    assert cnt.cpu().tolist() == gold["ms_ch_n"].tolist()
    assert model.mean_scan_pts.item() == float(np.mean(gold["ms_ch_n"]))
    np.testing.assert_allclose(cloud.cpu().numpy(), gold["ms_ch_cloud"], atol=2e-5)
    print("RATIO policy chain %s T max abs diff = %.3e" % (nn_engine, np.abs(T.detach().cpu().numpy() - gold["ms_ch_T"]).max()))
    np.testing.assert_allclose(T.detach().cpu().numpy(), gold["ms_ch_T"], atol=2e-6)
    (T * dev(chain_in["G"])).sum().backward()
    assert c.grad.dtype == torch.float32
    for b in range(B):
        want = gold["ms_ch_grad_mask"][b].astype(np.float64)
        r = np.abs(c.grad[b].cpu().double().numpy() - want).max() / np.abs(want).max()
        print("RATIO policy chain %s grad mask item %d err/scale = %.3e (scale %.3e)" % (nn_engine, b, r, np.abs(want).max()))
        assert r <= CHAIN_MASK_REL, (nn_engine, b, r)


# ----------------------------------------------------------------------------- 8. a full-size step
def test_full_size_scan_mode_step_is_bit_reproducible():
    from mm_masking_amd import synthetic
    from mm_masking_amd import train_icp_weights as trn
    from mm_masking_amd.icp_weight_policy import LearnICPWeightPolicy
    params = trn.default_params(DEV)
    params.update({"mask_target": "scan"})
    raw = synthetic.make_batch([0, 1], device=DEV)
    batch = trn.prepare_batch(raw, params)
    assert {"fft_polar", "azimuths", "az_times"} <= set(batch["loc_data"])
    assert not {"fft_polar", "azimuths", "az_times"} & set(trn.prepare_batch(raw, trn.default_params(DEV))["loc_data"])
    runs = []
    for _ in range(2):
        torch.manual_seed(0)
        model = LearnICPWeightPolicy(params).to(DEV)
        opt = trn.make_optimizer(model, params)
        model.train()
        loss, _ = trn.train_step(model, batch, opt, trn.loss_weights_from(params), DEV)
        runs.append((loss, [q.grad.detach().clone() for q in model.parameters()], model.mean_scan_pts))
    (l1, g1, n1), (l2, g2, n2) = runs
    print("FULL SIZE scan-mode step: loss %.6f, mean points from the masked scan %.1f" % (l1.item(), n1.item()))
    assert torch.isfinite(l1).all() and torch.equal(l1, l2) and n1.item() > 0 and torch.equal(n1, n2)
    assert any(g.abs().max() > 0 for g in g1) and all(torch.equal(a, b) for a, b in zip(g1, g2))
    importlib.import_module("mm_masking_amd.dICP.ICP").check_errors(wait=True)
