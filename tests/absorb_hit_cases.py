"""Shared pieces of the first-hitting sampler's tests: the numpy replays of ctdd_absorb_hit_time (the level recursion, the count rule,
the evaluation time) and of ctdd_absorb_hit_step's selection (Philox keys, stable order), written out from include/ctdd_absorb.h; the
schedules the tests run on.  The states of the selected rows are absorb_cases.step_replay's picks (the plain step at p = 1)."""
import numpy as np
import torch

import absorb_cases as ac
from ctdd import process
from oracle import philox as oph

# (t_func, rate_const): the parameters tests/test_absorb_cpu.py runs the schedules with ("log": time_base 3, time_exp 100)
SCHEDULES = (("loglinear", 1.0), ("log_sqr", 2.0), ("sqrt_cos", 1.55), ("log", 0.5))
NEAR = 1e-9                             # an event whose level is this close to log_cmin may be judged either way by another fp64 log


def proc(t_func="loglinear", rate_const=1.0, S=5, m=None):
    p = dict(rate_const=rate_const, t_func=t_func, alpha_eps=1e-3, mask_state=S - 1 if m is None else m)
    if t_func == "log":
        p.update(time_base=3.0, time_exp=100.0)
    return process.DeviceForwardProcess("absorbing", S, "cpu", **p)


def log_level(pr, t):
    """log(1 - alpha(t)) in fp64, as the sampler computes its start and closing levels."""
    return torch.log(1 - pr.alpha(torch.as_tensor(t, dtype=torch.float64))).numpy()


def hit_time_replay(x, logc_in, m, kmax, log_cmin, pr, t_min, t_max, seed, offset, levels=False):
    """(counts (N,) int, logc_out (N,) fp64, t_eval (N,) fp64, near (N,) bool) of ctdd_absorb_hit_time; with levels=True also the
    list, per sample, of the accepted events' levels L_1, L_2, ..  Sample n reads the blocks of the Philox row N D + n."""
    x, logc_in = np.asarray(x), np.asarray(logc_in, dtype=np.float64)
    N, D = x.shape
    counts, out, t_eval, near, lv = np.zeros(N, dtype=np.int64), logc_in.copy(), np.full(N, float(t_min)), np.zeros(N, dtype=bool), []
    u = oph.row_uniforms(N * D + np.arange(N), offset, seed, (int(kmax) + 3) // 4)       # (N, 4 blocks): component i & 3 of block i >> 2
    for n in range(N):
        M = int((x[n] == m).sum())
        L, acc = float(logc_in[n]), []
        for i in range(min(int(kmax), M)):
            Ln = L + np.log(np.float64(u[n, i])) / np.float64(M - i)
            near[n] |= abs(Ln - log_cmin) < NEAR
            if not Ln >= log_cmin:
                L = float(log_cmin)
                break
            L = float(Ln)
            acc.append(L)
        counts[n], out[n] = len(acc), L
        if acc:
            t = float(pr.time_of_alpha(torch.tensor(1.0 - np.exp(acc[0]), dtype=torch.float64)))
            t_eval[n] = min(max(t, float(t_min)), float(t_max)) if t == t else float(t_min)
        lv.append(acc)
    return (counts, out, t_eval, near, lv) if levels else (counts, out, t_eval, near)


# the cases of the GPU test of ctdd_absorb_hit_time: D below, at and above a wave and a workgroup's 256 rows
TIME_SHAPES = ((3, 1), (2, 5), (3, 64), (2, 65), (3, 257), (2, 1500))
KMAX = (1, 3, 9)                        # 9 crosses a Philox block of 4 twice
T_MIN, T_MAX = 0.05, 0.85


def time_inputs(N, D, pr):
    """x with the masked shares 0 / 0.5 / 1 cycling over the samples (a share above 0 masks row 0 at least), a start level per sample."""
    m = pr.mask_state
    rng = np.random.default_rng(100 * N + D)
    x = np.zeros((N, D), dtype=np.int32)
    for n in range(N):
        share = (0.0, 0.5, 1.0)[n % 3]
        x[n] = np.where(rng.random(D) < share, m, 0)
        if share > 0:
            x[n, 0] = m
    return x, log_level(pr, [0.9, 0.6, 0.8][:N])


def time_seed(D, kmax):
    return 0xC0FFEE00 + 16 * D + kmax, kmax


def closing_levels(x, logc, m, kmax, pr, seed, offset):
    """(-inf, a level that stops the sample with the most masked rows inside the step: between its first two events, or above its
    only one) and that sample's index."""
    _, _, _, _, lv = hit_time_replay(x, logc, m, kmax, -np.inf, pr, T_MIN, T_MAX, seed, offset, levels=True)
    big = int(np.argmax((np.asarray(x) == m).sum(1)))
    e = lv[big]
    cut = 0.5 * (e[0] + e[1]) if len(e) > 1 else 0.5 * (float(logc[big]) + e[0])
    return (-np.inf, float(cut)), big, (1 if len(e) > 1 else 0)


def row_keys(rows, seed, offset):
    """The uint32 selection key of the flat rows: component 0 of the block (row, offset, draw = 1)."""
    rows = np.asarray(rows, dtype=np.uint64)
    lo, hi = (rows & oph.MASK32).astype(np.uint32), (rows >> np.uint64(32)).astype(np.uint32)
    return oph.philox4x32_10(lo, hi, np.uint32(offset), np.uint32(1), np.uint32(seed & 0xFFFFFFFF), np.uint32((seed >> 32) & 0xFFFFFFFF))[0]


def clamp_count(k, M):
    return min(int(M), max(0, int(k)))


def hit_select_replay(x, m, counts, seed, offset):
    """Per sample the selected rows d (ascending): the k_n masked rows first in a stable sort on (key descending, d ascending)."""
    x = np.asarray(x)
    N, D = x.shape
    sel = []
    for n in range(N):
        rows = np.nonzero(x[n] == m)[0]                                  # ascending d
        order = np.argsort(-row_keys(n * D + rows, seed, offset).astype(np.int64), kind="stable")
        sel.append(np.sort(rows[order[:clamp_count(counts[n], rows.size)]]))
    return sel


def count_options(M):
    return (0, 1, M - 1, M, M + 3, -2)


def picks(logits, m, seed, offset):
    """(pick, margin) of every row: the state ctdd_absorb_step draws at p = 1 (component 1 of the row's draw-0 block)."""
    _, _, pick, margin = ac.step_replay(logits, None, m, 1.0, seed, offset)
    return pick, margin
