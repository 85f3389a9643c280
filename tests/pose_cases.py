"""What the tests of the SE(3) pose terms (pose_loss="se3") share: the pose set, the batches made by cycling it, the fp64
reference (the PyTorch expression of train_icp_weights._se3_terms under autograd, computed once per batch and form) and the
closed-form gradient -- a module of the tests, not a test.  Nothing here touches a device.

The pose set, as (name, T_pred, T_gt) in fp32 built with synthetic.se3_exp; the gt_eye form reads T_pred alone:
    identity, a pure roll of 0.1, a pure yaw of 0.4, a rotation without translation, a translation without rotation, a rotation by
    pi - 1e-3 about a generic axis (s is small there and c close to -1), four generic 6-DoF poses (||rho|| <= 2, |z| <= 0.5,
    |roll|, |pitch| <= 0.1, |yaw| <= 0.6) against generic ground-truth poses, T_pred == T_gt, and a T_gt whose rotation block is
    off by 1e-3 per entry (a pose read from data is not orthonormal).
Batch sizes 1, 5, 64, 65 and 130: the kernels' lanes stride over the pairs by 64, so these are the smallest sizes at which the
stride (65, 130) or the tail (1, 5, 65, 130 against the full wave of 64) can go wrong.
"""
import functools
import math

import numpy as np
import torch

from mm_masking_amd import train_icp_weights as trn
from mm_masking_amd.synthetic import se3_exp

BATCH_SIZES = (1, 5, 64, 65, 130)
G_ROT, G_TRANS = 0.7, 1.3                        # the upstream gradients of the gradient comparisons

# xi = (x, y, z, roll, pitch, yaw)
GENERIC = ((1.2, -0.7, 0.4, 0.08, -0.05, 0.5), (-1.1, 1.3, -0.5, -0.1, 0.1, -0.6), (0.3, 0.2, 0.1, 0.02, 0.07, 0.1),
           (-0.9, -1.2, 0.25, -0.06, -0.09, 0.33))
GENERIC_GT = ((0.4, 0.3, -0.2, 0.03, 0.02, -0.2), (-0.6, 0.1, 0.3, -0.04, 0.05, 0.45), (0.05, -0.3, 0.15, 0.06, -0.02, 0.15),
              (1.0, 0.8, -0.1, -0.01, 0.08, -0.5))
_AXIS = np.array([0.36, -0.48, 0.8])             # a unit vector
_OFF = 1e-3 * np.array([[1.0, -1.0, 1.0], [-1.0, 1.0, 1.0], [1.0, 1.0, -1.0]])


def _T(xi):
    return se3_exp(xi).astype(np.float32)


def pose_set():
    """[(name, T_pred (4,4) fp32, T_gt (4,4) fp32)]."""
    eye = np.eye(4, dtype=np.float32)
    cases = [("identity", eye.copy(), eye.copy()),
             ("roll", _T([0, 0, 0, 0.1, 0, 0]), eye.copy()),
             ("yaw", _T([0, 0, 0, 0, 0, 0.4]), eye.copy()),
             ("rotation_only", _T([0, 0, 0, 0.07, -0.09, 0.5]), eye.copy()),
             ("translation_only", _T([1.1, -0.8, 0.3, 0, 0, 0]), eye.copy()),
             ("near_pi", _T(np.concatenate(([0.5, -0.2, 0.1], (math.pi - 1e-3) * _AXIS))), eye.copy())]
    for k, (a, b) in enumerate(zip(GENERIC, GENERIC_GT)):
        cases.append(("generic%d" % k, _T(a), _T(b)))
    cases.append(("equal", _T(GENERIC[1]), _T(GENERIC[1])))
    off = _T(GENERIC_GT[2])
    off[:3, :3] += _OFF.astype(np.float32)
    cases.append(("gt_not_orthonormal", _T(GENERIC[3]), off))
    return cases


NAMES = [c[0] for c in pose_set()]
GENERIC_ROWS = [i for i, n in enumerate(NAMES) if n.startswith("generic")]


def batch(B):
    """(T_pred, T_gt) as (B,4,4) fp32 CPU tensors: the pose set cycled."""
    cases = pose_set()
    pick = [cases[i % len(cases)] for i in range(B)]
    return (torch.from_numpy(np.stack([c[1] for c in pick])), torch.from_numpy(np.stack([c[2] for c in pick])))


def equal_batch(B):
    """T_pred == T_gt for every pair, the ground-truth poses of the set (the one that is not orthonormal included) cycled."""
    Tg = batch(max(B, len(NAMES)))[1][-B:].clone()
    return Tg.clone(), Tg


def xi_f64(T_pred, T_gt):
    """xi = T_pred T_gt^-1 - I in fp64 from the fp32 inputs (T_gt None: the gt_eye form), as (T_pred - T_gt) T_gt^-1: the same
    matrix, and exactly zero for T_pred == T_gt.  (Formed as T_pred T_gt^-1 - I it is rounding noise of 1e-17 there, whose
    theta and r are right to 1e-17 but whose autograd gradient is a unit vector of noise: no reference for the zero the terms'
    gradient has at xi = 0.)"""
    T = T_pred.double()
    if T_gt is None:
        return T - torch.eye(4, dtype=torch.float64)
    return (T - T_gt.double()) @ torch.inverse(T_gt.double())


def expression(T_pred, T_gt):
    """(rot, trans, metric 3-vector) of the PyTorch expression in fp64."""
    theta, r = trn._se3_terms(xi_f64(T_pred, T_gt))
    return theta.mean(), r.mean(), torch.stack((torch.sqrt(theta * theta + r * r).mean(), theta.mean(), r.mean()))


@functools.lru_cache(maxsize=None)
def reference(B, with_gt):
    """fp64 values and autograd gradients of the cycled batch of size B in one form, as numpy arrays (shared, read-only):
    out2, out3, grad (G_ROT rot + G_TRANS trans), grad_rot (rot alone), grad_trans (trans alone)."""
    Tp, Tg = batch(B)
    T = Tp.double().requires_grad_(True)
    rot, trans, out3 = expression(T, Tg if with_gt else None)
    g_rot, = torch.autograd.grad(rot, T, retain_graph=True)
    g_trans, = torch.autograd.grad(trans, T)
    ref = {"out2": np.array([rot.item(), trans.item()]), "out3": out3.detach().numpy(), "grad_rot": g_rot.numpy(),
           "grad_trans": g_trans.numpy(), "grad": (G_ROT * g_rot + G_TRANS * g_trans).numpy()}
    for a in ref.values():
        a.setflags(write=False)
    return ref


def closed_form_grad(T_pred, T_gt, g_rot, g_trans):
    """d(g_rot mean theta + g_trans mean r) / dT_pred in fp64 by the closed form the kernel evaluates (include/mmk.h):
    G = dL/dxi, grad_T = G (gt_eye) or G T_gt^-T."""
    xi = xi_f64(T_pred, T_gt).detach()
    B = xi.shape[0]
    v = 0.5 * torch.stack((xi[:, 2, 1] - xi[:, 1, 2], xi[:, 0, 2] - xi[:, 2, 0], xi[:, 1, 0] - xi[:, 0, 1]), dim=1)
    s = torch.sqrt((v * v).sum(dim=1))
    c = 1 + 0.5 * (xi[:, 0, 0] + xi[:, 1, 1] + xi[:, 2, 2])
    d = s * s + c * c
    one = torch.ones_like(s)
    gv = torch.where(s > 0, c / torch.where(s > 0, s * d, one), 0 * s)[:, None] * v * (g_rot / B)
    gc = torch.where(d > 0, -s / torch.where(d > 0, d, one), 0 * s) * (g_rot / B)
    t = xi[:, 0:3, 3]
    r = torch.sqrt((t * t).sum(dim=1))
    G = torch.zeros_like(xi)
    G[:, 0:3, 3] = torch.where(r > 0, 1 / torch.where(r > 0, r, one), 0 * r)[:, None] * t * (g_trans / B)
    G[:, 2, 1], G[:, 1, 2] = 0.5 * gv[:, 0], -0.5 * gv[:, 0]
    G[:, 0, 2], G[:, 2, 0] = 0.5 * gv[:, 1], -0.5 * gv[:, 1]
    G[:, 1, 0], G[:, 0, 1] = 0.5 * gv[:, 2], -0.5 * gv[:, 2]
    for i in range(3):
        G[:, i, i] = 0.5 * gc
    if T_gt is None:
        return G
    return G @ torch.inverse(T_gt.double()).transpose(1, 2)
