"""Shared pieces of the absorbing-state diffusion tests: the case list and its inputs, the fp64 (and fp32) evaluation of the
objective with its gradient through autograd, and the CPU replay of the noising and step draws (the formulas and Philox layouts of
include/ctdd_absorb.h, written out here)."""
import functools

import numpy as np
import torch

from oracle import philox as oph

# (S, mask_state, B, D): one case per row packing of csrc/absorb.hip -- 64 rows a wave (S = 2, 3), 16 (S = 5), 4 (S = 64, float4
# loads), 1 with 4 / 8 / 16 states a lane (S = 65, 257, 1024; 1024 with float4 loads) -- each with a partial last workgroup
# (B D is no multiple of the 256 / 64 / 16 / 4 rows of a workgroup), mask states first, last and inside.
CASES = (
    (2, 1, 3, 5),
    (3, 0, 3, 5),
    (5, 2, 2, 37),
    (64, 63, 3, 40),
    (65, 17, 2, 37),
    (257, 256, 3, 130),
    (1024, 500, 2, 9),
)
IDS = [f"S{c[0]}-m{c[1]}" for c in CASES]
MODES = ("mix", "all", "none")          # which rows of x_t are masked


@functools.lru_cache(maxsize=None)
def inputs(case):
    """logits (B, D, S) fp32 ~ N(0, 3^2), every third row with the mask state's logit 50 above the row's largest; x0 (B, D) int64 in
    the real states except two entries at the mask state (they carry no term); w (B,) fp32 in (0.5, 3); computed once per case."""
    S, m, B, D = case
    g = torch.Generator().manual_seed(1000 + S)
    logits = 3.0 * torch.randn(B, D, S, generator=g)
    flat = logits.view(B * D, S)
    flat[::3, m] = flat[::3].max(dim=1).values + 50.0
    x0 = torch.randint(0, S - 1, (B, D), generator=g)
    x0 = x0 + (x0 >= m).long()                                   # skips the mask state
    x0.view(-1)[[1, B * D - 2]] = m
    w = 0.5 + 2.5 * torch.rand(B, generator=g)
    return logits.contiguous(), x0, w.float()


def x_t_of(case, mode):
    S, m, B, D = case
    _, x0, _ = inputs(case)
    if mode == "all":
        return torch.full_like(x0, m)
    if mode == "none":
        return x0.clone()
    g = torch.Generator().manual_seed(2000 + S)
    return torch.where(torch.rand(B, D, generator=g) < 0.5, torch.full_like(x0, m), x0)


def nll_scale_of(case, mode):
    """The cross-entropy weight: on in the mixed mode only (with it off, unmasked rows carry no term and are not read)."""
    return 0.3 / (case[2] * case[3]) if mode == "mix" else 0.0


def loss_eval(logits, x0, x_t, w, nll_scale, m, dtype):
    """(value, d value / d logits) in `dtype`: the mask state's column is dropped, then log_softmax and a gather."""
    S = logits.shape[-1]
    l = logits.to(dtype).clone().requires_grad_(True)
    cols = torch.tensor([s for s in range(S) if s != m])
    lp = torch.log_softmax(l[..., cols], dim=-1)                 # (B, D, S - 1)
    has = x0 != m
    pos = torch.where(has, x0 - (x0 > m).long(), torch.zeros_like(x0))
    nlp = torch.where(has, -lp.gather(-1, pos.unsqueeze(-1)).squeeze(-1), torch.zeros((), dtype=dtype))
    value = (w.to(dtype) * torch.where(x_t == m, nlp, torch.zeros((), dtype=dtype)).sum(1)).sum() / x0.shape[0]
    value = value + torch.as_tensor(nll_scale, dtype=dtype) * nlp.sum()
    grad, = torch.autograd.grad(value, l, allow_unused=True)
    return value.detach(), (torch.zeros_like(l) if grad is None else grad).detach()


@functools.lru_cache(maxsize=None)
def loss_refs(case, mode):
    """((value, grad) fp64, (value, grad) fp32 on the CPU) of one case and masking mode."""
    S, m, B, D = case
    logits, x0, w = inputs(case)
    args = (logits, x0, x_t_of(case, mode), w, nll_scale_of(case, mode), m)
    return loss_eval(*args, torch.float64), loss_eval(*args, torch.float32)


def term_rows(case, mode):
    """(B, D) bool: the rows that carry a term."""
    S, m, B, D = case
    _, x0, _ = inputs(case)
    carries = (x_t_of(case, mode) == m) | (nll_scale_of(case, mode) != 0.0)
    return carries & (x0 != m)


def noise_replay(x0, alpha, m, seed, offset):
    """(x_t, near, u): entry e = b D + d reads component e & 3 of the block of row e >> 2; near: |u - alpha| < 1e-6."""
    B, D = x0.shape
    n = B * D
    u = oph.row_uniforms(np.arange((n + 3) // 4), offset, seed, 1).reshape(-1)[:n].reshape(B, D)
    a = np.asarray(alpha, dtype=np.float32).reshape(B, 1)
    x_t = np.where(u >= a, m, np.asarray(x0))
    return x_t, np.abs(u.astype(np.float64) - a.astype(np.float64)) < 1e-6, u


def step_replay(logits, x, m, p, seed, offset):
    """Replay of ctdd_absorb_step's draws: (unmask (rows,), u0 near p, pick, pick's margin) for all N D rows (masked or not)."""
    N, D, S = logits.shape
    U = oph.row_uniforms(np.arange(N * D), offset, seed, 1)
    u0, u1 = U[:, 0], U[:, 1]
    l = np.asarray(logits, dtype=np.float32).reshape(N * D, S).copy()
    l[:, m] = -np.inf
    wts = np.exp(l - l.max(axis=1, keepdims=True)).astype(np.float32)
    pick, margin = oph.categorical_icdf(wts, u1)
    return u0 < np.float32(p), np.abs(u0.astype(np.float64) - float(np.float32(p))) < 1e-6, pick, margin


def argmax_f64(logits, m):
    """(argmax over s != m with the lowest index on ties, the gap between the two largest) in fp64."""
    l = np.asarray(logits, dtype=np.float64).reshape(-1, logits.shape[-1]).copy()
    l[:, m] = -np.inf
    top = np.sort(l, axis=1)
    gap = top[:, -1] - top[:, -2] if l.shape[1] > 2 else np.full(l.shape[0], np.inf)
    return l.argmax(axis=1), gap


def closed_form_qt(S, m, alpha):
    """q_t of the absorbing process: q[i, i] = alpha, q[i, m] = 1 - alpha, q[m, m] = 1."""
    q = alpha * np.eye(S)
    q[:, m] = 1.0 - alpha
    q[m, :] = 0.0
    q[m, m] = 1.0
    return q
