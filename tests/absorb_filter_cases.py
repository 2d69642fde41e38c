"""Shared pieces of the tests of ctdd_absorb_filter (temperature, top-k and top-p truncation of the masked rows' logits): the case
list and its inputs, and the fp64 replay of the semantics stated in include/ctdd_absorb.h -- the fp32 quotient, the order
(v descending, s ascending), the top-k prefix, the top-p prefix on the fp64 softmax -- with, per row, whether a cumulative mass of
the ordered candidates lies so close to p that an fp32 sum may judge the boundary state the other way."""
import functools

import numpy as np
import torch

import absorb_cases as ac

B, D = 3, 683                           # 2049 rows: a partial last workgroup in every packing (256 / 64 / 16 / 4 rows a workgroup)
CASES = tuple((S, m) for S, m, _, _ in ac.CASES)
IDS = [f"S{S}-m{m}" for S, m in CASES]
MODES = ("mix", "all", "none")          # which rows of x are masked
ROW_INF, ROW_NAN = 10, 11               # the row without a finite real-state logit, the row with a NaN (both masked in every mode but "none")
NEAR = 1e-5                             # absolute, on the normalised cumulative mass: an fp32 sum of at most 1024 weights stays well inside
TEMPS, PS = (0.7, 1.0), (0.5, 0.9)


def real_states(S, m):
    return np.array([s for s in range(S) if s != m])


@functools.lru_cache(maxsize=None)
def inputs(case):
    """logits (B, D, S) fp32 ~ N(0, 3^2) as absorb_cases.inputs draws them: every third row with the mask state's logit 50 above the
    row's largest; every seventh row (S = 3: every 49th) with up to three real states set to another real state's value (every fourteenth: to the
    row's largest), so that ties at and inside the boundary occur; ROW_INF with -inf at every real state; ROW_NAN with one NaN."""
    S, m = case
    g = torch.Generator().manual_seed(3000 + S)
    flat = 3.0 * torch.randn(B * D, S, generator=g)
    flat[::3, m] = flat[::3].max(dim=1).values + 50.0
    real = real_states(S, m)
    real_t = torch.from_numpy(real)
    # (a tie of every real state puts a cumulative mass at exactly 1/2, 1/4, ..: fewer states tie where there are few, and with two
    # real states, where a tie is the whole row, only every 49th row ties, so that replay()'s `near` rows stay a small share)
    for r in range(0, B * D, 49 if real.size == 2 else 7):
        src = int(real[int(flat[r, real_t].argmax())]) if r % 14 == 0 else int(real[r % real.size])
        for t in range(min(3, max(1, (real.size - 1) // 2), real.size - 1)):
            flat[r, int(real[(r + 1 + 5 * t) % real.size])] = flat[r, src]
    flat[ROW_INF, real_t] = -np.inf
    flat[ROW_NAN, int(real[real.size // 2])] = np.nan
    return flat.view(B, D, S).contiguous()


def x_of(case, mode):
    """x (B, D) int32: the mask state at about half the rows ("mix", ROW_INF and ROW_NAN among them), all or none of them."""
    S, m = case
    g = torch.Generator().manual_seed(4000 + S)
    other = int(real_states(S, m)[0])
    masked = torch.rand(B * D, generator=g) < 0.5
    if mode == "all":
        masked[:] = True
    elif mode == "none":
        masked[:] = False
    else:
        masked[[ROW_INF, ROW_NAN]] = True
    return torch.where(masked, torch.tensor(m), torch.tensor(other)).to(torch.int32).view(B, D)


def k_options(S):
    return (1, 2, 5, max(S - 2, 0), S - 1, S + 3)


def replay(logits, m, T, k, p):
    """The filter on every row of logits (R, S), in numpy.  Returns a dict of
      v      (R, S) fp32: np.float32(l) / np.float32(T), NaN as -inf, -inf at the mask state;
      kept   (R, S) bool: the states that stay AND carry a finite v (a state at -inf reads -inf whether it stays or not);
      near   (R,)   bool: some cumulative mass of the ordered candidates lies within NEAR of p (never when p >= 1);
      edge   (R, 2) int : the last state that stays and the first that does not, in the order (-1: none) -- the one state a near row
                          may be judged differently at is one of the two;
      dead   (R,)   bool: no finite real-state logit (the row comes back as it was)."""
    l = np.asarray(logits, dtype=np.float32)
    R, S = l.shape
    real = real_states(S, m)
    with np.errstate(invalid="ignore", over="ignore"):
        v = (l / np.float32(T)).astype(np.float32)
    v[np.isnan(v)] = -np.inf
    v[:, m] = -np.inf
    vv = v[:, real]                                                       # (R, S - 1)
    order = np.argsort(-vv.astype(np.float64), axis=1, kind="stable")     # (v descending, s ascending)
    vs = np.take_along_axis(vv, order, axis=1).astype(np.float64)
    n = real.size
    kk = int(k) if 1 <= int(k) < S - 1 else n
    dead = ~(vs[:, 0] > -np.inf)
    with np.errstate(invalid="ignore"):
        w = np.exp(vs - np.where(dead, 0.0, vs[:, 0])[:, None])
    w[:, kk:] = 0.0
    w[dead] = 0.0
    tot = w.sum(axis=1, keepdims=True)
    c = np.cumsum(w, axis=1) / np.where(tot > 0, tot, 1.0)
    if p >= 1.0:
        n_keep = np.full(R, kk)
        near = np.zeros(R, dtype=bool)
    else:
        n_keep = np.minimum((c[:, :kk] < p).sum(axis=1) + 1, kk)          # the shortest prefix whose mass reaches p
        near = (np.abs(c[:, :kk] - p) <= NEAR).any(axis=1) & ~dead
    pos = np.empty_like(order)
    np.put_along_axis(pos, order, np.broadcast_to(np.arange(n), (R, n)), axis=1)
    kept = np.zeros((R, S), dtype=bool)
    kept[:, real] = (pos < n_keep[:, None]) & (vv > -np.inf)
    kept[dead] = False
    last = real[np.take_along_axis(order, (n_keep - 1)[:, None], axis=1)[:, 0]]
    first_out = np.where(n_keep < n, real[np.take_along_axis(order, np.minimum(n_keep, n - 1)[:, None], axis=1)[:, 0]], -1)
    return dict(v=v, kept=kept, near=near, edge=np.stack((last, first_out), axis=1), dead=dead)


def brute_force_row(row, m, T, k, p):
    """The states of one row that stay, written out state by state (Python floats for the softmax)."""
    S = len(row)
    v = {}
    for s in range(S):
        if s != m:
            q = np.float32(row[s]) / np.float32(T)
            v[s] = -np.inf if np.isnan(q) else float(q)
    order = sorted(v, key=lambda s: (-v[s], s))
    if 1 <= k < S - 1:
        order = order[:k]
    if not order or v[order[0]] == -np.inf:
        return None
    if p < 1.0:
        w = [np.exp(v[s] - v[order[0]]) for s in order]
        z, run, cut = sum(w), 0.0, len(order)
        for i, wi in enumerate(w):
            run += wi
            if run / z >= p:
                cut = i + 1
                break
        order = order[:cut]
    return sorted(s for s in order if v[s] > -np.inf)


def probs(row, m, T, k, p):
    """fp64 probabilities of the tempered, truncated, renormalised distribution of one row (S,)."""
    r = replay(np.asarray(row, dtype=np.float32)[None], m, T, k, p)
    v = np.where(r["kept"][0], r["v"][0].astype(np.float64), -np.inf)
    e = np.exp(v - v.max())
    return e / e.sum()
