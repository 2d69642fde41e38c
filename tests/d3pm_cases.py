"""Shared pieces of the D3PM tests: the stand-in network of tools/gen_d3pm_golden.py, a diffusion factory, and the fp64
evaluation of the objective and of the ancestral step's logits (the formulas of include/ctdd_d3pm.h, written out here)."""
import math

import torch

from ctdd.config_dict import ConfigDict
from oracle.toy_model import toy_logits

# S, bands, transition type, B, D, T: FMA chains (S = 2, 3, 16), the smallest GEMM (one 128-row tile, not full), two row tiles
# with the second partial, and a GEMM case whose tables are not symmetric (absorbing: a swap of Qbar and its transpose shows).
# B = 3 everywhere: t = (0, 1, T - 1) in one batch, so a late table reaches every path.
GPU_CASES = (
    (2, None, "uniform", 3, 5, 6),
    (3, None, "absorbing", 3, 5, 6),
    (16, 2, "uniform", 3, 7, 12),
    (32, None, "gaussian", 3, 40, 12),
    (256, None, "gaussian", 3, 130, 12),
    (32, None, "absorbing", 3, 40, 12),
)
GPU_IDS = [f"S{c[0]}-{c[2]}" for c in GPU_CASES]
SCHEDULE = {"uniform": "cosine", "gaussian": "linear", "absorbing": "jsd"}


def spec(kind, bands, S, T, sched=None, loss_type="kl", device="cpu", **extra):
    m = ConfigDict()
    start, stop = (0.02, 1.0) if kind == "uniform" else (1e-4, 0.02)
    m.update(type=sched or SCHEDULE[kind], start=start, stop=stop, num_timesteps=T, model_prediction="x_start", model_output="logits",
             transition_mat_type=kind, transition_bands=bands, loss_type=loss_type, hybrid_coeff=0.01, num_pixel_vals=S,
             device=device, is_img=False, **extra)
    return m


class ToyNet(torch.nn.Module):
    """toy_logits at time t / T, output in the input's shape + (S,)."""

    def __init__(self, S, T):
        super().__init__()
        self.S, self.T = S, T
        self.dummy = torch.nn.Parameter(torch.zeros(1))

    def forward(self, x, t):
        return toy_logits(x.reshape(x.shape[0], -1), t.to(torch.float32) / self.T, self.S).reshape(tuple(x.shape) + (self.S,))


def model_logits_f64(dif, logits, x_t, t):
    """fp64: log(f1 + eps) + log(softmax(l) @ Qbar_{t-1} + eps), l itself at t = 0.  logits (B, D, S), x_t (B, D), t (B,)."""
    l = logits.double()
    q, q1T = dif.q_mats.double(), dif.transpose_q_onestep_mats.double()
    t1 = torch.clamp(t - 1, min=0)
    f1 = q1T[t.view(-1, 1), x_t.long()]
    f2 = torch.matmul(torch.softmax(l, -1), q[t1])
    model = torch.log(f1 + dif.eps) + torch.log(f2 + dif.eps)
    return torch.where(t.view(-1, 1, 1) == 0, l, model), f1


def loss_f64(dif, logits, x0, x_t, t, vb_scale, ce_scale):
    """fp64 (loss, vb, ce) per sample and d sum_b loss_b / d logits through autograd."""
    l = logits.double().clone().requires_grad_(True)
    model, f1 = model_logits_f64(dif, l, x_t, t)
    t1 = torch.clamp(t - 1, min=0)
    true = torch.log(f1 + dif.eps) + torch.log(dif.q_mats.double()[t1.view(-1, 1), x0.long()] + dif.eps)
    lt, lm = torch.log_softmax(true, -1), torch.log_softmax(model, -1)
    kl = (lt.exp() * (lt - lm)).sum(-1)
    ce = -torch.log_softmax(l, -1).gather(-1, x0.long().unsqueeze(-1)).squeeze(-1)
    vb = torch.where(t.view(-1, 1) == 0, ce, kl).mean(1) / math.log(2.0)
    ce = ce.mean(1) / math.log(2.0)
    loss = vb_scale * vb + ce_scale * ce
    grad, = torch.autograd.grad(loss.sum(), l)
    return loss.detach(), vb.detach(), ce.detach(), grad
