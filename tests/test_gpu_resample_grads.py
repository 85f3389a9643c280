"""GPU: gradients of the two radar resamplers with respect to their image -- radar_polar_to_cartesian_diff
(mmk_polar_to_cart_bwd, fp32) and radar_cartesian_to_polar (mmk_cart_to_polar_bwd, fp64) against the reference's own CPU
autograd (tests/golden/resample_grads.npz, written by tests/golden/make_golden_resample_grads.py): golden gradients,
structural zeros, the adjoint identity at full size, run-to-run bit equality, the chain through both links into dICP,
the U-Net's parameters behind the Cartesian -> polar link, dtype / device of the gradients.

Tolerances.  Against the golden gradients every comparison is max |got - ref| over max |ref| (support.ratio), no cell excluded, and every bound is 4 x the worst ratio measured on an MI355X:

    test                                          worst measured    bound
    polar -> Cartesian, pc_a (three variants)     8.7e-6            PC_A_REL  = 1.6e-5  (the front end's ceiling; 4 x = 3.5e-5)
    polar -> Cartesian, pc_b (three variants)     1.24e-6           PC_B_REL  = 5.0e-6
    Cartesian -> polar, cp_a (fp64)               2.35e-16          CP_REL    = 9.4e-16 (no project ceiling: fp64)
    chain, gradient at c (both NN engines)        3.2e-6            CHAIN_C_REL = 1.3e-5  (ceiling: the dICP backward's 2e-3)
    chain, gradient at p (both NN engines)        1.41e-5           CHAIN_P_REL = 5.7e-5  (same ceiling)

pc_a's ratio is the last bit of its fp32 sampling coordinates, not the sums: the coordinates reach 95 there (one ulp is
7.6e-6 of a cell, and a tap weight is a difference of two of them), the reference's CPU operators and the kernel's IEEE
divisions round them differently, and a gradient cell of scale 5 is a sum of about seven such taps.  An adjoint built on
the host from the coordinates of oracle/radar_ref.py with fp64 sums is 2.6e-6 from the same golden gradients; pc_b's
coordinates stay below 24 and its ratio is six times smaller.  No libm call is involved, so the ratio does not move with
the ROCm version, and the bound stays at the ceiling instead of 4 x the measurement.

The kernels form every sum in 64-bit fixed point (exact integer additions), so the only differences from the reference's
sequential fp32 / fp64 sums are the reference's own rounding of its partial sums, and the fixed-point resolution:
max|g| * 2^(cnt_bits - 62) per tap, cnt_bits = ceil(log2(4 W^2)) for polar -> Cartesian (2^-47 of max|g| at W = 72, 2^-41 at
W = 640) and ceil(log2(A (ceil(2 sqrt 2 cart_res / radar_res) + 1))) for Cartesian -> polar (2^-54 for cp_a, 2^-49 at
400 x 3360 -> 640 x 640).

The adjoint identity at full size is checked against a bound derived from the formats, not measured: with u the unit
roundoff of the operator's format, |<G, F(X)> - <F^T G, X>| <= 6 u sum|G| F(|X|)  (the forward's four products and three
additions, shared tap weights, and one rounding of each gradient cell)  +  n_taps * max|G| * max|X| * 2^(cnt_bits - 63)
(every tap rounded to the nearest fixed-point step).  Measured: 5.7e-11 (fp32) and 2.0e-17 (fp64) of sum|G| F(|X|).
"""
import math

import numpy as np
import pytest
import torch

from mm_masking_amd import radar_utils as ru
from mm_masking_amd.dICP.ICP import ICP
from radar_cases import RES, wobbly_azimuths
from support import DEV, close, dev, load_golden, nn_engine, policy  # noqa: F401  (nn_engine: a fixture)

pytestmark = pytest.mark.gpu
PC_A_REL = 1.6e-5
PC_B_REL = 5.0e-6
CP_REL = 9.4e-16
CHAIN_C_REL = 1.3e-5
CHAIN_P_REL = 5.7e-5
PC_VARIANTS = ({}, {"fix_wobble": False}, {"interpolate_crossover": False})


@pytest.fixture(scope="module")
def gold(golden_dir):
    return load_golden(golden_dir, "resample_grads.npz")


@pytest.fixture(scope="module")
def base(golden_dir):
    return load_golden(golden_dir, "radar_grads.npz")


def _pc_args(gold, key):
    R, W = (int(v) for v in gold[key + "_shape"])
    return dev(gold[key + "_az"]), float(gold[key + "_res"]), W


# ----------------------------------------------------------------------------- 1. against the golden gradients
@pytest.mark.parametrize("key", ["pc_a", "pc_b"])
@pytest.mark.parametrize("tag", [0, 1, 2])
def test_polar_to_cart_gradient_matches_reference(gold, key, tag):
    az, res, W = _pc_args(gold, key)
    kw = PC_VARIANTS[tag]
    x = dev(gold[key + "_x"]).requires_grad_(True)
    y = ru.radar_polar_to_cartesian_diff(x, az, res, cart_pixel_width=W, **kw)
    assert y.requires_grad and y.grad_fn is not None
    plain = ru.radar_polar_to_cartesian_diff(x.detach(), az, res, cart_pixel_width=W, **kw)
    assert not plain.requires_grad and torch.equal(y.detach(), plain)
    y.backward(dev(gold[key + "_G"]))
    assert x.grad.shape == x.shape and x.grad.dtype == torch.float32 and x.grad.is_cuda
    want = gold["%s_grad%d" % (key, tag)]
    for item in range(want.shape[0]):
        close(x.grad[item], want[item], "%s variant %d item %d" % (key, tag, item), PC_A_REL if key == "pc_a" else PC_B_REL)


def test_cart_to_polar_gradient_matches_reference(gold):
    A, R = (int(v) for v in gold["cp_a_shape"])
    az = dev(gold["cp_a_az"])
    x = dev(gold["cp_a_x"]).requires_grad_(True)
    y = ru.radar_cartesian_to_polar(x, az, 0.1, cart_resolution=0.3, polar_pixel_shape=(A, R))
    assert y.requires_grad and y.grad_fn is not None and y.dtype == torch.float64
    plain = ru.radar_cartesian_to_polar(x.detach(), az, 0.1, cart_resolution=0.3, polar_pixel_shape=(A, R))
    assert not plain.requires_grad and torch.equal(y.detach(), plain)
    y.backward(dev(gold["cp_a_G"]))
    assert x.grad.shape == x.shape and x.grad.dtype == torch.float64 and x.grad.is_cuda
    for item in range(x.shape[0]):
        close(x.grad[item], gold["cp_a_grad"][item], "cp_a item %d" % item, CP_REL)


# ----------------------------------------------------------------------------- 2. structural zeros
def test_polar_cells_no_pixel_samples_get_exact_zero(gold):
    """pc_a: no pixel of an even-width image lies within half a range cell of the sensor, so column 0 receives nothing.
    pc_b: the image corner is 12.1 m from the sensor, so the columns from 13.75 m (index 28) on receive nothing."""
    for key, cols in (("pc_a", slice(0, 1)), ("pc_b", slice(28, None))):
        az, res, W = _pc_args(gold, key)
        for tag, kw in enumerate(PC_VARIANTS):
            x = dev(gold[key + "_x"]).requires_grad_(True)
            ru.radar_polar_to_cartesian_diff(x, az, res, cart_pixel_width=W, **kw).backward(dev(gold[key + "_G"]))
            assert (x.grad[:, :, cols] == 0).all(), (key, tag)
            assert (gold["%s_grad%d" % (key, tag)][:, :, cols] == 0).all()
            assert x.grad.abs().max() > 0


def test_rows_cut_off_without_crossover_get_exact_zero(gold):
    """Pixels whose angle lies beyond the last azimuth, uniform table (fix_wobble=False): their second tap row is row A of an
    A-row image without the crossover rows (cut off), and padded row A + 1 = row 0 with them."""
    az, res, W = _pc_args(gold, "pc_a")
    A = az.shape[1]
    ang = ru.form_cart_range_angle_grid(cart_pixel_width=W, dtype=torch.float32)[1].to(DEV)
    G = dev(gold["pc_a_G"]).clone()
    for b in range(G.shape[0]):
        G[b][~(ang > az[b, -1] + 0.02)] = 0.0
        assert (G[b] != 0).sum() > 20
    grads = {}
    for cross in (False, True):
        x = dev(gold["pc_a_x"]).requires_grad_(True)
        ru.radar_polar_to_cartesian_diff(x, az, res, cart_pixel_width=W, interpolate_crossover=cross,
                                         fix_wobble=False).backward(G)
        grads[cross] = x.grad
    assert (grads[False][:, :A - 1] == 0).all() and (grads[False][:, A - 1].abs().amax(dim=1) > 0).all()
    assert (grads[True][:, 1:A - 1] == 0).all() and (grads[True][:, 0].abs().amax(dim=1) > 0).all()
    assert (grads[True][:, A - 1].abs().amax(dim=1) > 0).all()


def test_cartesian_pixels_no_ray_touches_get_exact_zero(gold):
    A, R = (int(v) for v in gold["cp_a_shape"])
    x = dev(gold["cp_a_x"]).requires_grad_(True)
    ru.radar_cartesian_to_polar(x, dev(gold["cp_a_az"]), 0.1, cart_resolution=0.3, polar_pixel_shape=(A, R)).backward(dev(gold["cp_a_G"]))
    untouched = dev(gold["cp_a_grad"] == 0)
    assert untouched.float().mean() > 0.4
    assert (x.grad[untouched] == 0).all() and (x.grad[~untouched] != 0).float().mean() > 0.99


# ----------------------------------------------------------------------------- 3. + 4. full size
@pytest.fixture(scope="module")
def full_size():
    """Inputs and both adjoints at 400 x 3360 <-> 640 x 640, B = 1, default parameters; computed once."""
    g = torch.Generator().manual_seed(77)
    az = wobbly_azimuths(5)
    out = {"az": az}
    # polar -> Cartesian, fp32
    X = torch.randn(1, 400, 3360, generator=g).to(DEV)
    G = torch.randn(1, 640, 640, generator=g).to(DEV)

    def pc_adjoint():
        x = X.clone().requires_grad_(True)
        ru.radar_polar_to_cartesian_diff(x, az.float().to(DEV), RES).backward(G)
        return x.grad
    with torch.no_grad():
        FX = ru.radar_polar_to_cartesian_diff(X, az.float().to(DEV), RES)
        FabsX = ru.radar_polar_to_cartesian_diff(X.abs(), az.float().to(DEV), RES)
    out["pc"] = (X, G, FX, FabsX, pc_adjoint(), pc_adjoint())
    # Cartesian -> polar, fp64
    Xd = torch.randn(1, 640, 640, generator=g, dtype=torch.float64).to(DEV)
    Gd = torch.randn(1, 400, 3360, generator=g, dtype=torch.float64).to(DEV)

    def cp_adjoint():
        x = Xd.clone().requires_grad_(True)
        ru.radar_cartesian_to_polar(x, az, RES).backward(Gd)
        return x.grad
    with torch.no_grad():
        FXd = ru.radar_cartesian_to_polar(Xd, az, RES)
        FabsXd = ru.radar_cartesian_to_polar(Xd.abs(), az, RES)
    out["cp"] = (Xd, Gd, FXd, FabsXd, cp_adjoint(), cp_adjoint())
    return out


def _fsum(t):
    return math.fsum(t.detach().cpu().double().reshape(-1).tolist())


@pytest.mark.parametrize("op", ["pc", "cp"])
def test_adjoint_identity_at_full_size(full_size, op):
    X, G, FX, FabsX, grad, _ = full_size[op]
    lhs, rhs = _fsum(G.double() * FX.double()), _fsum(grad.double() * X.double())
    scale = _fsum(G.double().abs() * FabsX.double())
    if op == "pc":
        u, cnt_bits, n_taps = 2.0 ** -24, math.ceil(math.log2(4 * 640 * 640)), 4 * 640 * 640
    else:
        per_ray = math.ceil(2 * math.sqrt(2) * 0.2384 / RES) + 1
        u, cnt_bits, n_taps = 2.0 ** -53, math.ceil(math.log2(400 * per_ray)), 4 * 400 * 3360
    tol = 6 * u * scale + n_taps * G.abs().max().item() * X.abs().max().item() * 2.0 ** (cnt_bits - 63)
    print("ADJOINT %s full size: <G,FX> %.12e  <FtG,X> %.12e  |diff| %.3e  tol %.3e  (diff / scale %.3e)"
          % (op, lhs, rhs, abs(lhs - rhs), tol, abs(lhs - rhs) / scale))
    assert scale > 0 and abs(lhs) > 0
    assert abs(lhs - rhs) <= tol, (op, lhs, rhs, tol)


@pytest.mark.parametrize("op", ["pc", "cp"])
def test_full_size_adjoints_are_bit_reproducible(full_size, op):
    first, second = full_size[op][4], full_size[op][5]
    assert torch.isfinite(first).all() and first.abs().max() > 0
    if op == "cp":
        # the four pixels at the sensor collect the first samples of all 400 rays
        centre = first[0, 318:322, 318:322]
        assert torch.equal(centre, second[0, 318:322, 318:322])
        assert centre[1:3, 1:3].abs().min() > 0
    assert torch.equal(first, second), op


# ----------------------------------------------------------------------------- 5. the chain
def _chain(gold, base, c, p):
    az = dev(base["ch_az"])
    npad, K = int(base["ch_npad"]), int(base["ch_iters"])
    B, A, R = base["ch_raw"].shape
    raw = base["ch_raw"].copy()
    raw.reshape(-1)[gold["ch_fix_idx"]] = gold["ch_fix_val"]
    polar_mask = ru.radar_cartesian_to_polar(c.double(), az.double(), RES, polar_pixel_shape=(A, R)).float()
    m = ru.cfar_mask(polar_mask * dev(raw), RES, diff=True)
    cloud, cnt = ru.extract_pc_padded(m, RES, az, torch.zeros_like(az), npad, diff=True)
    wmask = ru.radar_polar_to_cartesian_diff(p, az, float(gold["ch_p_res"]), cart_pixel_width=640)
    w = ru.extract_weights(wmask, cloud)[0]
    icp = ICP(icp_type="pt2pl", differentiable=True, max_iterations=K, tolerance=1e-9)
    T = icp.icp(cloud, dev(base["ch_map"]), weight=w, trim_dist=5.0, loss_fn={"name": "huber", "metric": 1.0}, dim=2)["T"]
    return T, cloud, cnt, w


def _chain_leaves(gold):
    c = (dev(gold["ch_cu"])[:, :, None] * dev(gold["ch_cv"])[:, None, :]).contiguous().requires_grad_(True)
    p = dev(gold["ch_p"]).requires_grad_(True)
    return c, p


def test_chain_pose_to_both_images(gold, base, nn_engine):
    """pose functional -> dICP -> (source cloud -> peaks -> CFAR -> masked scan -> Cartesian mask c) and
    (extract_weights -> Cartesian weight mask -> polar weight image p), against the reference's front end composed with the
    CPU restatement of dICP."""
    c, p = _chain_leaves(gold)
    T, cloud, cnt, w = _chain(gold, base, c, p)
    assert cnt.cpu().tolist() == gold["ch_n"].tolist()
    np.testing.assert_allclose(cloud.detach().cpu().numpy(), gold["ch_cloud"], atol=2e-5)
    np.testing.assert_allclose(w.detach().cpu().numpy(), gold["ch_w"], atol=2e-6)
    print("RATIO chain T max abs diff = %.3e" % np.abs(T.detach().cpu().numpy() - gold["ch_T"]).max())
    (T * dev(base["ch_G"])).sum().backward()
    np.testing.assert_allclose(T.detach().cpu().numpy(), gold["ch_T"], atol=2e-6)
    assert c.grad.dtype == torch.float32 and p.grad.dtype == torch.float32
    for b in range(c.shape[0]):
        close(c.grad[b], gold["ch_grad_c"][b], "chain %s grad c item %d" % (nn_engine, b), CHAIN_C_REL)
        close(p.grad[b], gold["ch_grad_p"][b], "chain %s grad p item %d" % (nn_engine, b), CHAIN_P_REL)


def test_chain_is_bit_reproducible(gold, base):
    def run():
        c, p = _chain_leaves(gold)
        (_chain(gold, base, c, p)[0] * dev(base["ch_G"])).sum().backward()
        return c.grad, p.grad
    (c1, p1), (c2, p2) = run(), run()
    assert torch.equal(c1, c2) and torch.equal(p1, p2)


# ----------------------------------------------------------------------------- 6. into the network
def test_gradient_reaches_the_unet_parameters():
    """A 64 x 64 mask of the U-Net through radar_cartesian_to_polar: every parameter gradient equals, bit for bit, the one
    obtained by feeding the standalone adjoint's mask gradient into mask.backward()."""
    model = policy(DEV, 3, train=True, dropout=0.0)
    g = torch.Generator().manual_seed(4)
    B, H, A, R = 2, 64, 32, 200
    scan = {"fft_data": (torch.rand(B, H, H, generator=g) ** 4).to(DEV), "fft_cfar": torch.zeros(B, H, H, device=DEV),
            "raw_pc": torch.zeros(B, 4, 3, device=DEV)}
    az = torch.sort(torch.rand(B, A, generator=g, dtype=torch.float64) * 2 * math.pi, dim=1).values
    G = torch.randn(B, A, R, generator=g, dtype=torch.float64).to(DEV)

    def to_polar(mask64):
        return ru.radar_cartesian_to_polar(mask64, az, RES, polar_pixel_shape=(A, R))

    mask = model(scan, {"pc": torch.zeros(B, 4, 6, device=DEV)}, None, mask_only=True)
    assert mask.shape == (B, H, H) and mask.requires_grad
    (to_polar(mask.double()) * G).sum().backward()
    through = [q.grad.detach().clone() for q in model.parameters()]
    model.zero_grad(set_to_none=True)
    mask2 = model(scan, {"pc": torch.zeros(B, 4, 6, device=DEV)}, None, mask_only=True)
    assert torch.equal(mask2.detach(), mask.detach())
    leaf = mask2.detach().double().requires_grad_(True)
    (to_polar(leaf) * G).sum().backward()
    mask2.backward(leaf.grad.to(mask2.dtype))
    fed = [q.grad.detach() for q in model.parameters()]
    assert len(through) == len(fed) and any(t.abs().max() > 0 for t in through)
    for t, f in zip(through, fed):
        assert torch.equal(t, f)


# ----------------------------------------------------------------------------- 7. dtype and device
def test_dtype_device_and_no_grad_paths(gold):
    az, res, W = _pc_args(gold, "pc_a")
    # a CPU fp64 image in: CPU image out, CPU fp64 gradient out, equal to the device gradient
    x = torch.from_numpy(gold["pc_a_x"]).double().requires_grad_(True)
    y = ru.radar_polar_to_cartesian_diff(x, az.cpu(), res, cart_pixel_width=W)
    assert y.device.type == "cpu" and y.requires_grad
    y.backward(torch.from_numpy(gold["pc_a_G"]))
    assert x.grad.device.type == "cpu" and x.grad.dtype == torch.float64
    d = dev(gold["pc_a_x"]).requires_grad_(True)
    ru.radar_polar_to_cartesian_diff(d, az, res, cart_pixel_width=W).backward(dev(gold["pc_a_G"]))
    assert torch.equal(x.grad, d.grad.cpu().double())
    # requires_grad=False and no_grad(): today's path
    assert ru.radar_polar_to_cartesian_diff(d.detach(), az, res, cart_pixel_width=W).grad_fn is None
    with torch.no_grad():
        assert ru.radar_polar_to_cartesian_diff(d, az, res, cart_pixel_width=W).grad_fn is None

    A, R = (int(v) for v in gold["cp_a_shape"])
    kw = dict(cart_resolution=0.3, polar_pixel_shape=(A, R))
    azd = torch.from_numpy(gold["cp_a_az"])
    xc = torch.from_numpy(gold["cp_a_x"]).requires_grad_(True)
    yc = ru.radar_cartesian_to_polar(xc, azd, 0.1, **kw)
    assert yc.device.type == "cpu" and yc.requires_grad and yc.dtype == torch.float64
    yc.backward(torch.from_numpy(gold["cp_a_G"]))
    assert xc.grad.device.type == "cpu" and xc.grad.dtype == torch.float64 and xc.grad.abs().max() > 0
    assert ru.radar_cartesian_to_polar(xc.detach(), azd, 0.1, **kw).grad_fn is None
    with torch.no_grad():
        assert ru.radar_cartesian_to_polar(xc, azd, 0.1, **kw).grad_fn is None
    # fp32 is refused as upstream, with or without grad; .double() is the caller's cast and autograd undoes it
    for t in (xc.detach().float(), xc.detach().float().requires_grad_(True)):
        with pytest.raises(RuntimeError, match="expected scalar type Float but found Double"):
            ru.radar_cartesian_to_polar(t, azd, 0.1, **kw)
    x32 = xc.detach().float().requires_grad_(True)
    ru.radar_cartesian_to_polar(x32.double(), azd, 0.1, **kw).backward(torch.from_numpy(gold["cp_a_G"]))
    assert x32.grad.dtype == torch.float32 and x32.grad.device.type == "cpu"
