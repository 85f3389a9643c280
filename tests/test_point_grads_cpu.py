"""CPU: the C ABI of the point-cloud gradients (mmk_icp_backward_points, mmk_sample_weights_bwd_pc) -- declared, exported,
host-side argument checks (no launch) -- and finite-difference checks of the oracle's gradients with respect to the
clouds, which the GPU tests compare the kernels against."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from mm_masking_amd import _lib, synthetic
from oracle import dicp_ref
from support import ROOT, icp_params
NEW = ("mmk_icp_backward_points", "mmk_icp_backward_points_workspace_bytes", "mmk_sample_weights_bwd_pc")


@pytest.fixture(scope="module")
def L():
    _lib.build()
    return _lib.lib()


def test_new_entries_declared_and_exported(L):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mmk.h")).read(), flags=re.S)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(L, name) and name in _lib.EXPORTED, name
    assert L.mmk_version() == 502


def test_icp_backward_points_workspace_and_argument_checks(L):
    p = icp_params()
    base = L.mmk_icp_workspace_bytes(ctypes.byref(p))
    assert L.mmk_icp_backward_points_workspace_bytes(ctypes.byref(p), 0) == base
    need = L.mmk_icp_backward_points_workspace_bytes(ctypes.byref(p), 1)
    # per-iteration rows (K,B,N,2 dim) fp32 + (B,M,4) int64 sums
    assert need >= base + 10 * 2 * 100 * 4 * 4 + 2 * 300 * 4 * 8
    assert L.mmk_icp_backward_points_workspace_bytes(ctypes.byref(icp_params(tgt_cols=3)), 1) == 0
    assert b"normals" in L.mmk_last_error()

    null = ctypes.c_void_p(0)
    fake = ctypes.c_void_p(4096)          # never dereferenced: every call below fails on the host before any launch

    def call(p, src=fake, gw=fake, ws=fake, nbytes=need):
        args = [src] + [fake] * 8 + [gw, null, fake, fake]
        return L.mmk_icp_backward_points(ctypes.byref(p), *args, ws, nbytes, null)

    assert call(p, src=null) == -1 and b"NULL" in L.mmk_last_error()
    assert call(p, gw=null) == -1 and b"NULL" in L.mmk_last_error()
    assert call(icp_params(dim=4)) == -1 and b"dim" in L.mmk_last_error()
    assert call(icp_params(save_state=0)) == -1 and b"save_state" in L.mmk_last_error()
    assert call(p, nbytes=need - 1) == -1 and b"workspace" in L.mmk_last_error()
    assert call(p, ws=null) == -1 and b"workspace" in L.mmk_last_error()


def test_sample_weights_bwd_pc_argument_checks(L):
    null = ctypes.c_void_p(0)
    fake = ctypes.c_void_p(4096)
    assert L.mmk_sample_weights_bwd_pc(null, fake, fake, 1, 4, 3, 64, 64, 640, 0.2384, fake, null) == -1
    assert b"NULL" in L.mmk_last_error()
    assert L.mmk_sample_weights_bwd_pc(fake, fake, fake, 1, 4, 3, 64, 64, 640, 0.2384, null, null) == -1
    assert L.mmk_sample_weights_bwd_pc(fake, fake, fake, 1, 4, 1, 64, 64, 640, 0.2384, fake, null) == -1
    assert b"shape" in L.mmk_last_error()
    assert L.mmk_sample_weights_bwd_pc(fake, fake, fake, 1, 4, 3, 1, 64, 640, 0.2384, fake, null) == -1


@pytest.mark.parametrize("icp_type,dim", [("pt2pt", 2), ("pt2pl", 2), ("pt2pt", 3), ("pt2pl", 3)])
def test_oracle_cloud_gradients_finite_difference(icp_type, dim):
    """The oracle's autograd in source, target xyz and target normals (fp64, fixed correspondences) against central
    differences; entries outside the arithmetic are exactly 0."""
    n, m, K = 80, 200, 3
    src, tgt, _ = synthetic.simple_cloud_pair(40 + dim, n, m, dim=dim, yaw=0.03, trans=(0.5, -0.3, 0.1))
    src, tgt = torch.from_numpy(src)[None], torch.from_numpy(tgt)[None]
    w = torch.from_numpy(np.random.default_rng(3).uniform(0.2, 1.0, (1, n)))
    G = torch.from_numpy(np.random.default_rng(4).normal(size=(1, 4, 4)))
    loss_fn = {"name": "cauchy", "metric": 1.0}
    ref = dicp_ref.ICPRef(icp_type, differentiable=True, max_iterations=K, tolerance=1e-12)
    fixed = ref.icp(src, tgt, T_init=torch.eye(4)[None], weight=w.float(), trim_dist=5.0, loss_fn=loss_fn, dim=dim)["hist"]["idx"]

    def f(s, t):
        T = ref.icp(s, t, T_init=torch.eye(4, dtype=torch.float64)[None], weight=w, trim_dist=5.0, loss_fn=loss_fn, dim=dim,
                    dtype=torch.float64, fixed_idx=fixed)["T"]
        return (T * G).sum()

    s = src.double().requires_grad_(True)
    t = tgt.double().requires_grad_(True)
    f(s, t).backward()
    gs, gt = s.grad[0], t.grad[0]
    used = torch.unique(torch.cat([ix[0].long() for ix in fixed]))
    unused = torch.ones(t.shape[1], dtype=torch.bool)
    unused[used] = False
    assert unused.any() and (gt[unused] == 0).all()
    if dim == 2:
        assert (gs[:, 2] == 0).all()
    assert (gt[:, dim:3] == 0).all()
    assert (gt[:, 3 + (dim if icp_type == "pt2pl" else 0):] == 0).all()

    eps = 1e-6
    checks = [("s", i, c) for i, c in ((0, 0), (17, 1), (63, dim - 1))]
    for j in used[[0, len(used) // 2, -1]].tolist():
        checks += [("t", j, c) for c in range(dim)]
        if icp_type == "pt2pl":
            checks += [("t", j, 3 + c) for c in range(dim)]
    for which, i, c in checks:
        base = s if which == "s" else t
        plus, minus = base.detach().clone(), base.detach().clone()
        plus[0, i, c] += eps
        minus[0, i, c] -= eps
        if which == "s":
            fd = (f(plus, t.detach()) - f(minus, t.detach())).item() / (2 * eps)
        else:
            fd = (f(s.detach(), plus) - f(s.detach(), minus)).item() / (2 * eps)
        g = (gs if which == "s" else gt)[i, c].item()
        assert abs(fd - g) <= 1e-5 * max(1e-3, abs(fd)) + 1e-8, (which, i, c, fd, g)
