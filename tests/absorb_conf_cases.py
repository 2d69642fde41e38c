"""Shared pieces of the confidence-ordered unmasking tests: the CPU replay of ctdd_absorb_commit (key mapping, count rule, selection)
and of ctdd_absorb_propose (the step's pick, the fp64 and fp32 scores), written out from include/ctdd_absorb.h."""
import math

import numpy as np

import absorb_cases as ac
from oracle import philox as oph


def score_keys(score):
    """The order-preserving uint32 key of fp32 scores: NaN 0, -0 as +0, b | 0x80000000 for sign-clear bits b, ~b for sign-set."""
    b = np.ascontiguousarray(score, dtype=np.float32).view(np.uint32).copy()
    nan = (b & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)
    b[b == np.uint32(0x80000000)] = 0
    neg = (b & np.uint32(0x80000000)) != 0
    key = np.where(neg, ~b, b | np.uint32(0x80000000)).astype(np.uint32)
    key[nan] = 0
    return key


def count_rule(p, M):
    """k = min(M, ceil(double(float32(p)) M)): the fp64 product of an fp32 and a small int is exact."""
    return min(int(M), int(math.ceil(float(np.float32(p)) * int(M))))


def commit_replay(x, cand, score, m, p=None, counts=None):
    """(out_x, changed) of ctdd_absorb_commit: per sample the k_n masked rows first in a stable sort on (-key, d) take cand.
    cand and score are read at the masked rows only."""
    assert (p is None) != (counts is None)
    x, cand, score = np.asarray(x), np.asarray(cand), np.asarray(score, dtype=np.float32)
    out, changed = x.copy(), 0
    for n in range(x.shape[0]):
        rows = np.nonzero(x[n] == m)[0]                                  # ascending d
        M = rows.size
        k = count_rule(p, M) if counts is None else min(M, max(0, int(counts[n])))
        order = np.argsort(-score_keys(score[n, rows]).astype(np.int64), kind="stable")
        take = rows[order[:k]]
        out[n, take] = cand[n, take]
        changed += k
    return out, changed


def propose_picks(logits, m, seed, offset):
    """(pick, margin, u2) for all N D rows: the pick of ctdd_absorb_step's replay (component 1) and the ranking uniform
    (component 2) of the row's Philox block."""
    N, D, _ = logits.shape
    _, _, pick, margin = ac.step_replay(logits, None, m, 1.0, seed, offset)
    return pick, margin, oph.row_uniforms(np.arange(N * D), offset, seed, 1)[:, 2]


def propose_scores(logits, m, rows, cand, noise, u2, dtype):
    """score of the flat rows `rows` at the candidates `cand` in `dtype` arithmetic: (l[cand] - mx) - log z over s != m, plus
    float32(noise) * -log(-log u2) when noise != 0 (u2: the exact fp32 uniforms of those rows)."""
    S = logits.shape[-1]
    l = np.asarray(logits, dtype=np.float32).reshape(-1, S)[rows].astype(dtype)
    l[:, m] = -np.inf
    mx = l.max(axis=1)
    z = np.exp(l - mx[:, None]).astype(dtype).sum(axis=1, dtype=dtype)
    s = (l[np.arange(rows.size), cand] - mx) - np.log(z).astype(dtype)
    if noise != 0:
        g = -np.log(-np.log(np.asarray(u2, dtype=np.float32).astype(dtype)).astype(dtype)).astype(dtype)
        s = s + dtype(np.float32(noise)) * g
    return s.astype(dtype)
