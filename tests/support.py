"""What test files of every kernel family share: the device, loaders, the RATIO comparison, the NN-engine fixture, policy and
``IcpParams`` builders, the header's arities, cloud pairs, layout and bf16 helpers -- a module of the tests, not a test.  Nothing
here touches a device at import; ``DEV`` only names it.  The radar and policy cases are in radar_cases.py, the dICP ones in
dicp_cases.py."""
import os
import re
import socket

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda:0")


def dev(a):
    """A numpy array as a contiguous device tensor."""
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def load_golden(golden_dir, name):
    return dict(np.load(os.path.join(golden_dir, name), allow_pickle=False))


# ----------------------------------------------------------------------------- comparisons
def ratio(g, ref, name):
    """max |g - ref| over max |ref|, printed."""
    g, ref = g.detach().cpu().double().numpy(), np.asarray(ref, dtype=np.float64)
    scale = np.abs(ref).max()
    assert scale > 0, name
    r = np.abs(g - ref).max() / scale
    print("RATIO %-40s err/scale = %.3e   (scale %.3e)" % (name, r, scale))
    return r


def close(g, ref, name, rel):
    r = ratio(g, ref, name)
    assert r <= rel, (name, r, rel)


def mask_close(raw, got, want, thres, band=1e-6):
    """CFAR masks may differ only where the cell sits within `band` of its threshold (window-sum rounding order,
    SURVEY.md §8a R2)."""
    bad = got != want
    if bad.any():
        assert np.all(np.abs(raw[bad] - thres[bad]) < band), "CFAR mask differs away from the threshold"
    assert bad.mean() < 1e-4


# ----------------------------------------------------------------------------- dICP
@pytest.fixture(params=["brute", "grid"])
def nn_engine(request):
    """Both nearest-neighbour engines: the exhaustive scan and the exact uniform-grid search."""
    from mm_masking_amd.dICP.ICP import ICP
    ICP.NN_SEARCH_OVERRIDE = request.param
    yield request.param
    ICP.NN_SEARCH_OVERRIDE = None


def icp_params(**kw):
    from mm_masking_amd import _lib
    d = dict(B=2, N=100, M=300, tgt_cols=6, dim=2, icp_type=1, loss=2, loss_k=1.0, trim_dist=5.0, tolerance=1e-5, max_iter=10,
             save_state=1, check_every=0, nn_method=0)
    d.update(kw)
    return _lib.IcpParams(**d)


def pair_batch(B, n, m, dim, pad_n=0, pad_m=0, seed=0, with_normals=True):
    """B pairs of synthetic.simple_cloud_pair with seeds seed + b -> (sources, targets, true poses)."""
    from mm_masking_amd import synthetic
    S, Tg, Tt = [], [], []
    for b in range(B):
        s, t, T = synthetic.simple_cloud_pair(seed + b, n, m, dim=dim, pad_n=pad_n, pad_m=pad_m, with_normals=with_normals,
                                              yaw=0.02 + 0.01 * b, trans=(0.6, -0.4 + 0.1 * b, 0.1))
        S.append(s), Tg.append(t), Tt.append(T)
    return np.stack(S), np.stack(Tg), np.stack(Tt)


def icp_yaml(tmp_path, text=None, **params):
    """A dICP config file: ``text`` as it is, or the parameters ``params`` under the default target_pad_val."""
    import yaml
    path = os.path.join(str(tmp_path), "dICP_config.yaml")
    with open(path, "w") as f:
        f.write(yaml.safe_dump({"dICP": {"target_pad_val": 1000.0, "parameters": params}}) if text is None else text)
    return path


# ----------------------------------------------------------------------------- the policy
def policy_params(device, **over):
    from mm_masking_amd import train_icp_weights as trn
    p = trn.default_params(device)
    p.update(over)
    return p


def policy(device, seed, train=False, **over):
    from mm_masking_amd.icp_weight_policy import LearnICPWeightPolicy
    p = policy_params(device, **over)
    torch.manual_seed(seed)
    model = LearnICPWeightPolicy(p).to(device)
    return model.train() if train else model


# ----------------------------------------------------------------------------- the C header
def header():
    """include/mmk.h without its comments."""
    return re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "mmk.h")).read(), flags=re.S)


def n_args(hdr, name):
    """Number of arguments of the entry point ``name`` as ``hdr`` declares it."""
    m = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, hdr, flags=re.S)
    assert m, name
    return len([a for a in m.group(1).split(",") if a.strip() and a.strip() != "void"])


# ----------------------------------------------------------------------------- the U-Net
def nchw(t):
    return t.float().permute(0, 3, 1, 2)


def nhwc(x_nchw):
    return x_nchw.permute(0, 2, 3, 1).contiguous().to(torch.bfloat16)


class _Q(torch.autograd.Function):
    """bf16 storage point: rounds the tensor in forward and its gradient in backward."""

    @staticmethod
    def forward(ctx, x):
        return x.to(torch.bfloat16).float()

    @staticmethod
    def backward(ctx, g):
        return g.to(torch.bfloat16).float()


class _QB(torch.autograd.Function):
    """bf16 storage point of a gradient tensor only: identity in forward, rounds the gradient in backward."""

    @staticmethod
    def forward(ctx, x):
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return g.to(torch.bfloat16).float()


# ----------------------------------------------------------------------------- processes
def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port
