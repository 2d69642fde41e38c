"""Helpers of the D3PM baseline (lib/d3pm.py): categorical KL / likelihood on the last axis, batch means, the beta schedules.
All torch ops: the host path of cfg.device == "cpu" and the yardstick of the fused kernels (csrc/d3pm.hip)."""
import math

import numpy as np
import torch
import torch.nn.functional as F

LN2 = math.log(2.0)


def get_diffusion_betas(spec):
    """(T,) betas of `spec.type`: 'linear' (spec.start .. spec.stop), 'cosine' (Hoogeboom et al. 2021, capped at 0.999) or
    'jsd' (1/T, 1/(T-1), ..., 1: absorbing models)."""
    T = int(spec.num_timesteps)
    if spec.type == "linear":
        return torch.linspace(spec.start, spec.stop, T)
    if spec.type == "cosine":
        u = np.arange(T + 1, dtype=np.float64) / T
        abar = np.cos((u + 0.008) / 1.008 * np.pi / 2)
        return torch.from_numpy(np.minimum(1.0 - abar[1:] / abar[:-1], 0.999))
    if spec.type == "jsd":
        return 1.0 / torch.linspace(T, 1.0, T)
    raise NotImplementedError(spec.type)


def log_min_exp(a, b, epsilon=1e-6):
    """log(exp(a) - exp(b)) for b < a, with `epsilon` inside the log1p."""
    return a + torch.log1p(epsilon - torch.exp(b - a))


def categorical_kl_logits(logits1, logits2, eps=1e-6):
    """KL(Cat(logits1) || Cat(logits2)) over the last axis (the `eps` shift of both logits is kept for parity; softmax
    ignores it up to rounding)."""
    la, lb = F.log_softmax(logits1 + eps, dim=-1), F.log_softmax(logits2 + eps, dim=-1)
    return (F.softmax(logits1 + eps, dim=-1) * (la - lb)).sum(-1)


def categorical_kl_probs(probs1, probs2, eps=1e-6):
    """KL between probability vectors over the last axis, eps inside both logs."""
    return (probs1 * (torch.log(probs1 + eps) - torch.log(probs2 + eps))).sum(-1)


def categorical_log_likelihood(x, logits):
    """log_softmax(logits)[x] over the last axis."""
    lp = F.log_softmax(logits, dim=-1)
    return (lp * F.one_hot(x.to(torch.int64), logits.shape[-1])).sum(-1)


def meanflat(x):
    """Mean over every axis but the first."""
    return x.mean(dim=tuple(range(1, x.dim())))
