"""CPU: learnable GO-CFAR thresholds -- the C ABI of mmk_cfar_mask_p / mmk_cfar_mask_bwd_p (declared, exported, host-side
argument and workspace checks, no launch), the golden fixture tests/golden/cfar_params.npz (the conditions its generator
asserts, re-asserted on the stored arrays; its fp64 threshold gradients against an fp64 numpy restatement),
``radar_utils.cfar_mask``'s shape check, and the policy switch params["learn_cfar"].  Cases, fixture loader and restatement
(``threshold_grads_f64``) are in tests/radar_cases.py.
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from mm_masking_amd import _lib
from radar_cases import CASES, RES, geom_of, load_fixture, per_scan_values, threshold_grads_f64
from support import ROOT, policy_params
from make_golden_radar_grads import cfar_terms, cfar_violations  # (radar_cases puts tests/golden on the path)

CPU = torch.device("cpu")
POLICY = {"dropout": 0.0, "amp_dtype": torch.float32, "unet_backend": "torch"}
NEW = ("mmk_cfar_mask_p", "mmk_cfar_mask_bwd_p_ws_bytes", "mmk_cfar_mask_bwd_p")


@pytest.fixture(scope="module")
def L():
    _lib.build()
    return _lib.lib()


@pytest.fixture(scope="module")
def gold(golden_dir):
    return load_fixture(golden_dir)


# ----------------------------------------------------------------------------- the C ABI
def test_new_entries_declared_and_exported(L):
    raw_hdr = open(os.path.join(ROOT, "include", "mmk.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", raw_hdr, flags=re.S)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(L, name) and name in _lib.EXPORTED, name
    assert L.mmk_version() == 502 == int(re.search(r"#define\s+MMK_VERSION\s+(\d+)", raw_hdr).group(1))
    for name in ("mmk_cfar_mask_p", "mmk_cfar_mask_bwd_p"):
        doc = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*(?:size_t\s+\w+\([^)]*\);\s*)?int\s+%s\s*\(" % name, raw_hdr, flags=re.S)
        assert doc and "radar_utils.py:56" in doc.group(1), name


def test_argument_and_workspace_checks(L):
    null, fake = ctypes.c_void_p(0), ctypes.c_void_p(4096)     # never dereferenced: every call fails on the host before a launch
    B, A = 2, 3
    need = L.mmk_cfar_mask_bwd_p_ws_bytes(B, A)
    assert need >= B * A * 16 and L.mmk_cfar_mask_bwd_p_ws_bytes(0, A) == 0 and L.mmk_cfar_mask_bwd_p_ws_bytes(B, 0) == 0

    def fwd(raw=fake, a=fake, b=fake, out=fake, B=B, A=A, R=1400, w2=50, guard=5, mincol=89, maxcol=1287):
        return L.mmk_cfar_mask_p(raw, B, A, R, w2, guard, mincol, maxcol, a, b, 1, 1, 10.0, out, null)

    def bwd(raw=fake, g=fake, a=fake, b=fake, ga=fake, gb=fake, ws=fake, nbytes=need, B=B, A=A, R=1400, w2=50, guard=5, mincol=89,
            maxcol=1287):
        return L.mmk_cfar_mask_bwd_p(raw, g, B, A, R, w2, guard, mincol, maxcol, a, b, 1, 10.0, null, ga, gb, ws, nbytes, null)

    for call, nulls in ((fwd, ("raw", "out", "a", "b")), (bwd, ("raw", "g", "a", "b", "ga", "gb"))):
        for k in nulls:
            assert call(**{k: null}) == -1 and b"NULL" in L.mmk_last_error(), k
        assert call(B=0) == -1 and b"3D" in L.mmk_last_error()
        assert call(w2=0) == -1 and b"window" in L.mmk_last_error()
        assert call(mincol=54) == -1 and b"column range" in L.mmk_last_error()
        assert call(maxcol=1401) == -1 and b"column range" in L.mmk_last_error()
        assert call(R=14000) == -1 and b"LDS" in L.mmk_last_error()
    assert b"threshold" in (fwd(a=null), L.mmk_last_error())[1] and b"threshold" in (bwd(b=null), L.mmk_last_error())[1]
    assert bwd(nbytes=need - 1) == -3 and b"workspace" in L.mmk_last_error()
    assert bwd(ws=null) == -3 and b"workspace" in L.mmk_last_error()


# ----------------------------------------------------------------------------- the fixture
@pytest.mark.parametrize("key", CASES)
def test_fixture_conditions(gold, key):
    raw = gold["cp_raw"]
    a, b = per_scan_values(gold, key, raw.shape[0])
    geom = geom_of(gold, key)
    for i in range(raw.shape[0]):
        kw = dict(geom, a_thresh=float(a[i]), b_thresh=float(b[i]))
        near_gate, near_tie, kept = cfar_violations(raw[i:i + 1], **kw)
        assert not near_gate.any()                              # no cell within 1e-4 of the 0.99 gate
        assert not near_tie.any()                               # a kept cell's window sums: equal, or 1e-4 apart
        assert kept.any()
        if i == 2:
            _, left, right, _ = cfar_terms(raw[i:i + 1], **kw)
            assert (kept & (left == right)).any()               # exact ties on kept cells of the empty field
    assert (gold["cp_sa_" + key] > 0).all() and (gold["cp_sb_" + key] > 0).all()
    e = np.concatenate([gold["cp_ea32_" + key], gold["cp_eb32_" + key]])
    assert (e < 1e-5).all()                                     # the reference's own fp32 rounding stays far below CFAR_REL


def test_fixture_conditions_chain(gold):
    raw = gold["cc_raw"]
    for a, b in ((np.ones(2), np.full(2, 0.09)), (gold["cc_a"].astype(np.float64), gold["cc_b"].astype(np.float64))):
        for i in range(raw.shape[0]):
            near_gate, near_tie, kept = cfar_violations(raw[i:i + 1], a_thresh=float(a[i]), b_thresh=float(b[i]))
            assert not near_gate.any() and not near_tie.any() and kept.any()
            assert (10.0 * RES * np.nonzero(kept)[2] * 0.99 > 10).all()      # kept cells lie in tanh's saturated columns
    assert (gold["cc_sa"] > 0).all() and (gold["cc_sb"] > 0).all()
    assert (np.abs(gold["cc_ga"]) <= gold["cc_sa"]).all() and (np.abs(gold["cc_gb"]) <= gold["cc_sb"]).all()


@pytest.mark.parametrize("key", CASES)
def test_restatement_agrees_with_the_fixture_fp64(gold, key):
    raw, G = gold["cp_raw"], gold["cp_G"]
    a, b = per_scan_values(gold, key, raw.shape[0])
    geom = geom_of(gold, key)
    ga, gb = threshold_grads_f64(raw, G, a, b, **geom)
    sa, sb = threshold_grads_f64(raw, np.abs(G), a, b, **geom)
    if key[1] == "s":
        ga, gb, sa, sb = ga.sum(keepdims=True), gb.sum(keepdims=True), sa.sum(keepdims=True), sb.sum(keepdims=True)
    np.testing.assert_allclose(np.abs(sa), gold["cp_sa_" + key], rtol=1e-9)
    np.testing.assert_allclose(np.abs(sb), gold["cp_sb_" + key], rtol=1e-9)
    assert (np.abs(ga - gold["cp_ga64_" + key]) <= 1e-9 * gold["cp_sa_" + key]).all()
    assert (np.abs(gb - gold["cp_gb64_" + key]) <= 1e-9 * gold["cp_sb_" + key]).all()
    # and the stored scan gradient of the shared cases is radar_grads.npz's own when no cell had to be changed
    if key[1] == "s" and len(gold["cp_fix_idx"]) == 0:
        assert np.array_equal(gold["cp_grad_" + key], gold["ca_grad" + key[0]])


# ----------------------------------------------------------------------------- radar_utils.cfar_mask
def test_bad_threshold_shape_raises_before_any_device_use():
    from mm_masking_amd import radar_utils as ru
    raw = torch.zeros(3, 4, 1400)
    for bad in (torch.ones(4), torch.ones(3, 1), torch.ones(2, 1, 1)):
        with pytest.raises(ValueError, match="a_thresh"):
            ru.cfar_mask(raw, RES, a_thresh=bad)
        with pytest.raises(ValueError, match="b_thresh"):
            ru.cfar_mask(raw, RES, a_thresh=1.0, b_thresh=bad)


# ----------------------------------------------------------------------------- the policy
def test_policy_learn_cfar_switch(golden_dir, tmp_path):
    from mm_masking_amd import ddp
    from mm_masking_amd import train_icp_weights as trn
    from mm_masking_amd.icp_weight_policy import LearnICPWeightPolicy
    today = [str(n) for n in np.load(os.path.join(golden_dir, "unet.npz"), allow_pickle=False)["names_a"]]
    for kw in ({}, {"mask_target": "scan"}, {"mask_target": "scan", "learn_cfar": False}):
        plain = LearnICPWeightPolicy(policy_params(CPU, **POLICY, **kw))
        assert list(plain.state_dict().keys()) == today and len(list(plain.parameters())) == 46
        assert not hasattr(plain, "cfar_a") and not plain.learn_cfar
    model = LearnICPWeightPolicy(policy_params(CPU, **POLICY, mask_target="scan", learn_cfar=True, a_thresh=1.1, b_thresh=0.08))
    keys = list(model.state_dict().keys())
    assert sorted(set(keys) - set(today)) == ["cfar_a", "cfar_b"] and len(keys) == len(today) + 2
    assert [k for k in keys if k in today] == today
    assert len(list(model.parameters())) == 48
    for q, v in ((model.cfar_a, 1.1), (model.cfar_b, 0.08)):
        assert isinstance(q, torch.nn.Parameter) and q.shape == () and q.dtype == torch.float32 and q.requires_grad
        assert q.item() == np.float32(v)
    assert (model.a_thres, model.b_thres) == (1.1, 0.08)        # the fixed values of the CFAR input channel stay
    for kw in ({}, {"mask_target": "weights"}):
        with pytest.raises(ValueError, match="learn_cfar"):
            LearnICPWeightPolicy(policy_params(CPU, **POLICY, learn_cfar=True, **kw))
    # the gradient bucket: the 46-parameter layout has the U-Net's buckets, anything else is one
    assert len(ddp.FlatGradSync(plain).bucket_ranges()) > 1
    sync = ddp.FlatGradSync(model)
    assert len(sync.params) == 48 and sync.bucket_ranges() == [(0, sync.flat.numel())]
    assert sync.flat.numel() == sum(q.numel() for q in plain.parameters()) + 2
    # optimizer and checkpoint pick the two up
    p = policy_params(CPU, **POLICY, mask_target="scan", learn_cfar=True)
    opt = trn.make_optimizer(model, p)
    assert sum(len(g["params"]) for g in opt.param_groups) == 48
    for q in model.parameters():
        q.grad = torch.full_like(q, 1e-3)
    opt.step()
    assert model.cfar_a.item() != np.float32(1.1) and model.cfar_b.item() != np.float32(0.08)
    trn.save_checkpoint(str(tmp_path / "ck.pt"), model, opt, epoch=1, best_norm=0.5)
    other = LearnICPWeightPolicy(p)
    trn.load_checkpoint(str(tmp_path / "ck.pt"), other, trn.make_optimizer(other, p))
    assert torch.equal(other.cfar_a, model.cfar_a) and torch.equal(other.cfar_b, model.cfar_b)
