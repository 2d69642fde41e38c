"""Shared pieces of the held-out likelihood tests (ctdd_absorb_nll, lib/likelihood.py): the fp64 and fp32 CPU evaluation of the row
terms on the cases of absorb_cases.py, the project's error bar, the models whose bounds have a closed form, and the closed forms."""
import functools
import math

import numpy as np
import torch

import absorb_cases as ac
from ctdd import process
from oracle.toy_model import toy_logits


def rows_eval(logits, x0, x_t, m, dtype):
    """(B, D) in `dtype`: -log softmax over s != m at x0 where x_t == m and x0 != m, 0 elsewhere (the mask column is dropped)."""
    S = logits.shape[-1]
    cols = torch.tensor([s for s in range(S) if s != m])
    lp = torch.log_softmax(logits.to(dtype)[..., cols], dim=-1)
    term = (x_t == m) & (x0 != m)
    pos = torch.where(term, x0 - (x0 > m).long(), torch.zeros_like(x0))
    return torch.where(term, -lp.gather(-1, pos.unsqueeze(-1)).squeeze(-1), torch.zeros((), dtype=dtype)), term


@functools.lru_cache(maxsize=None)
def nll_refs(case, mode, weighted):
    """{row64, row32 (B, D), out64, out32 (B,), term, hit (B, D) bool}: computed once per case, masking mode and weighting."""
    S, m, B, D = case
    logits, x0, w = ac.inputs(case)
    if not weighted:
        w = torch.ones_like(w)
    x_t = ac.x_t_of(case, mode)
    row64, term = rows_eval(logits, x0, x_t, m, torch.float64)
    row32, _ = rows_eval(logits, x0, x_t, m, torch.float32)
    best, _ = ac.argmax_f64(logits.numpy(), m)
    hit = term & (torch.from_numpy(best).view(B, D) == x0)
    return dict(row64=row64, row32=row32, out64=w.double() * row64.sum(1), out32=w * row32.sum(1), term=term, hit=hit)


def bar(ref64, ref32):
    """max(8 E32, 1e-6 max(1, |value|)) per entry, E32 the largest error of the fp32 CPU evaluation over the call."""
    e32 = float((ref32.double() - ref64).abs().max())
    return torch.clamp(1e-6 * torch.clamp(ref64.abs(), min=1.0), min=8 * e32), e32


def proc(S, m, device="cpu", **kw):
    p = dict(rate_const=1.0, t_func="loglinear", alpha_eps=1e-3, mask_state=m)
    p.update(kw)
    if p["t_func"] == "log":
        p.update(time_base=3.0, time_exp=100.0)
    return process.DeviceForwardProcess("absorbing", S, device, **p)


class DimOnlyModel:
    """Logits that depend on the dimension d only: N(0, 3^2), fixed by a seed."""

    def __init__(self, S, m, D, device):
        self.S, self.device, self.process = S, device, proc(S, m, device)
        self.base = (3.0 * torch.randn(D, S, generator=torch.Generator().manual_seed(4))).to(device)

    def __call__(self, x, t):
        return self.base.unsqueeze(0).expand(x.shape[0], -1, -1)

    def cross_entropies(self, x0_row):
        """c_d = -lp[d][x0_d] in fp64."""
        l = self.base.cpu().double().clone()
        l[:, self.process.mask_state] = -np.inf
        return -torch.log_softmax(l, -1)[torch.arange(l.shape[0]), x0_row.long()]


class TimeOnlyModel:
    """test_gpu_absorb.py's model: toy_logits at x = 0, logits that depend on the time and the dimension only."""

    def __init__(self, S, m, device):
        self.S, self.device, self.process = S, device, proc(S, m, device)

    def __call__(self, x, t):
        return toy_logits(torch.zeros_like(x), t, self.S, scale=3.0)


def data(S, m, N, D, same=True):
    """x0 (N, D) in the real states; `same`: every sample is the first one (the closed forms are per x0)."""
    x = torch.randint(0, S - 1, (1 if same else N, D), generator=torch.Generator().manual_seed(8))
    x = x + (x >= m).long()
    return x.expand(N, D).contiguous()


def grid_of(pr, num_steps, min_t, max_t, rule):
    """(t_i, p_i, surv_i, surv_K) of AbsorbingLeap's grid in fp64 numpy."""
    ts = np.concatenate((np.linspace(max_t, min_t, num_steps), [0.0]))
    t = torch.from_numpy(ts)
    p = torch.clamp(pr.unmask_prob(t[:-1], t[:-1] - t[1:], rule), 0.0, 1.0).numpy()
    surv = np.concatenate(([1.0], np.cumprod(1.0 - p)))
    return ts[:-1], p, surv[:-1], surv[-1]


def alpha_sigma(pr, c, K, min_t, max_t):
    """The exact per-sample standard deviation of the "alpha" estimate for a network that ignores x_t and t."""
    a_hi, a_lo = (float(v) for v in pr.alpha(torch.tensor([min_t, max_t], dtype=torch.float64)))
    R, lam_min, c2 = a_hi - a_lo, (1 - a_hi) / (1 - a_lo), float((c ** 2).sum())
    V = R ** 2 * c2 / (1 - a_lo) ** 2 * (-math.log(lam_min) / (1 - lam_min) - 1)
    return math.sqrt(V / K + lam_min * (1 - lam_min) * c2)


def time_only_ce(S, m, D, x0_row, times):
    """CE_i(x0)[d] in fp64 of the time-only model at the fp32 times the network sees: (len(times), D)."""
    out = []
    for t in times:
        l = toy_logits(torch.zeros(1, D), torch.tensor([t], dtype=torch.float64).float(), S, scale=3.0)[0].double()
        l[:, m] = -np.inf
        out.append(-torch.log_softmax(l, -1)[torch.arange(D), x0_row.long()].numpy())
    return np.stack(out)
