"""Shared pieces of the remasking tests: the held pattern of a case, the remask schedule in exact rationals, and the CPU replay of
ctdd_absorb_remask_step's remask decision (Philox component 3, sigma_row) and of ctdd_absorb_remask_norm, written out from
include/ctdd_absorb.h; the fp64 / fp32 probability of a written state for the confidence record."""
from fractions import Fraction

import numpy as np

from oracle import philox as oph


def step_seed(S):
    """The Philox key of the step tests of a case.  tests/test_absorb_remask_cpu.py checks that no remask coin of these keys lies
    within the GPU tests' nearness bands of its threshold."""
    return 0x5E1EC7ED0000 + S


SIGMA, SIGMA_CONF, P_VALUES = 0.25, 0.3, (0.0, 0.3, 1.0)                 # the step tests' remask probabilities and unmasking probabilities


def conf_pattern(case):
    """(B, D) fp32 in (0, 1]: the confidence record that the step tests hand in."""
    S, m, B, D = case
    return (1.0 - np.random.default_rng(4000 + S).random((B, D))).astype(np.float32)


def rows_per_workgroup(S):
    """256 / LPR rows of csrc/absorb.hip's row packing."""
    return 256 // (1 if S <= 4 else 4 if S <= 16 else 16 if S <= 64 else 64)


def held_pattern(case, seed=0):
    """(B, D) bool, about a third of the rows held, with the first and the last row of the (partial) last workgroup held."""
    S, m, B, D = case
    rng = np.random.default_rng(3000 + S + seed)
    held = rng.random(B * D) < 1.0 / 3.0
    rpb = rows_per_workgroup(S)
    held[((B * D - 1) // rpb) * rpb] = True
    held[B * D - 1] = True
    return held.reshape(B, D)


def exact_schedule(p, strategy, eta, active=None):
    """(sigma, p_prime, surv) of the remask schedule in rationals: p, eta as the exact values of their fp64s."""
    p = [Fraction(float(v)) for v in p]
    eta = Fraction(float(eta))
    active = [True] * len(p) if active is None else list(active)
    sigma, pp, surv = [], [], [Fraction(1)]
    for pk, on in zip(p, active):
        s, nxt = surv[-1], surv[-1] * (1 - pk)
        sk = Fraction(0)
        if on and s < 1:
            smax = min(Fraction(1), nxt / (1 - s))
            sk = eta * smax if strategy == "rescale" else min(eta, smax)
        sigma.append(sk)
        pp.append(pk + sk * (1 - s) / s if s > 0 else pk)
        surv.append(nxt)
    return sigma, pp, surv


def norm_replay(x, held, conf, m, temp, dtype=np.float64):
    """(U (N,) int, Z (N,) dtype): per sample the number of free unmasked rows and the sum of exp(-conf / temp) over them; the
    quotient and the exponential in `dtype`, the sum in `dtype` too."""
    x, conf = np.asarray(x), np.asarray(conf, dtype=np.float32)
    free = (x != m) if held is None else (x != m) & ~np.asarray(held, dtype=bool)
    w = np.exp(-(conf.astype(dtype) / dtype(np.float32(temp)))).astype(dtype)
    return free.sum(1), np.where(free, w, dtype(0)).sum(1, dtype=dtype)


def remask_replay(x, held, m, sigma, seed, offset, conf=None, norm=None, temp=1.0):
    """(remask, sigma_row, u3, free) over the flat N D rows: u3 is component 3 of the row's Philox block, free the rows that are
    neither held nor masked, remask = free & (u3 < sigma_row).  sigma_row is float32(sigma), or with norm (N, 2) fp32 the kernel's
    fp32 expression min(1, ((sigma U_n) exp(-conf / temp)) / Z_n), 0 where Z_n <= 0."""
    x = np.asarray(x)
    N, D = x.shape
    u3 = oph.row_uniforms(np.arange(N * D), offset, seed, 1)[:, 3]
    free = (x != m).reshape(-1)
    if held is not None:
        free &= ~np.asarray(held, dtype=bool).reshape(-1)
    sg = np.full(N * D, np.float32(sigma), dtype=np.float32)
    if norm is not None:
        norm = np.asarray(norm, dtype=np.float32)
        U, Z = np.repeat(norm[:, 0], D), np.repeat(norm[:, 1], D)
        w = np.exp(-(np.asarray(conf, dtype=np.float32).reshape(-1) / np.float32(temp))).astype(np.float32)
        with np.errstate(divide="ignore", invalid="ignore"):
            sg = np.where(Z > 0, np.minimum(np.float32(1), ((np.float32(sigma) * U) * w) / Z), np.float32(0)).astype(np.float32)
    return free & (u3 < sg), sg, u3, free


def state_probability(logits, m, rows, states, dtype):
    """exp(l[state] - mx) / z over s != m for the flat rows `rows` at `states`, in `dtype` arithmetic."""
    S = logits.shape[-1]
    l = np.asarray(logits, dtype=np.float32).reshape(-1, S)[rows].astype(dtype)
    l[:, m] = -np.inf
    mx = l.max(axis=1)
    z = np.exp(l - mx[:, None]).astype(dtype).sum(axis=1, dtype=dtype)
    return (np.exp(l[np.arange(rows.size), states] - mx).astype(dtype) / z).astype(dtype)
