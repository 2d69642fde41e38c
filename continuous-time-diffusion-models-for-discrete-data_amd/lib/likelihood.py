"""Held-out likelihood bounds of the absorbing-state ("masked") models: `absorbing_nll_bound` (per sample, in nats) and
`eval_likelihood` (a data loader -> bits per dimension and perplexity).  Not in the reference, which has no likelihood evaluation.

Notation: a(t) = alpha(t), w(t) = elbo_weight(t) = -a'(t) / (1 - a(t)), m the mask state, lp the log-softmax over the states s != m.
The samplers start from the all-mask state at t_max, so an entry of x_t of THEIR generative model is masked with probability
lam(t) = (1 - a(t)) / (1 - a(t_max)), not 1 - a(t) (the survival AbsorbingLeap's ancestral rule telescopes to); the hazard w(t) is the
same for both.  With CE(x_t, t) = sum over the free entries d with x_t[d] == m of -lp_theta(x0[d] | x_t, t) (held entries are never
masked and carry no term):

spacing = "alpha": the continuous-time limit of the ancestral sampler, closed by a SAMPLED step at t_min,
    -log p(x0_F | x0_held) <= E_{lam(t_min)}[CE(x_tmin, t_min)] + integral_{t_min}^{t_max} w(t) E_{lam(t)}[CE(x_t, t)] dt.
  The integral is estimated in u = a(t), where w(t) dt = -du / (1 - u): with R = a(t_min) - a(t_max) and K = n_times strata, sample n
  draws u_{n,k} = a(t_max) + R (k + jitter_{n,k}) / K, t_{n,k} = a^-1(u_{n,k}), noises x0 at the rate (1 - u) / (1 - a(t_max)) and
  takes y_{n,k} = R / (1 - u_{n,k}) CE.  The estimate is terminal_n + mean_k y_{n,k}, terminal_n one draw at lam(t_min), t_min.  In
  these variables the integrand is flat for every schedule (for a network that ignores x_t and t, E[y | u] does not depend on u).

spacing = "grid": the bound of AbsorbingLeap exactly as configured (num_steps, rule, min_t), closed by a SAMPLED step.  With the
  sampler's grid t_i = linspace(t_max, t_min, num_steps) followed by 0, its p_i = clamp(unmask_prob(t_i, t_i - t_{i+1}, rule), 0, 1),
  surv_0 = 1 and surv_{i+1} = surv_i (1 - p_i):
    bound = sum_{i < num_steps} p_i E_{surv_i}[CE(x_{t_i}, t_i)] + E_{surv_K}[CE(x_tmin, t_min)],
  one mask draw per grid point: the forwards of one sampling run.  Under the ancestral rule p_{K-1} = 1 and surv_K = 0: the last term
  vanishes and takes no forward.

The samplers' own closing step is an argmax, which is mode-seeking: it is not a distribution over x0 with a finite bound.  Both
bounds here are those of the same chain closed by a draw from the softmax at t_min instead.

Per draw: ctdd_absorb_noise (key `seed`, offset = the draw's index), held entries restored, one forward under no_grad, one
ctdd_absorb_nll launch pair into the draw's row of an fp64 buffer (deterministic per-sample sums, csrc/absorb.hip); no host sync inside
the loop and one read-back after it.  fused = False or a CPU model: the same terms in fp64 torch ops."""
import dataclasses
import math
import warnings

import numpy as np
import torch

from ctdd import native
from ctdd.process import UNMASK_RULES
from lib.models.models import borrow_engine_output

SPACINGS = ("alpha", "grid")


@dataclasses.dataclass
class LikelihoodBound:
    """nll (N,) fp64, nats: the bound on -log p(x0_free | x0_held) per sample.  stderr (N,): for "alpha" std_k(y) / sqrt(K) over
    the K strata -- conservative for the integral (stratifying u only removes variance that this figure still counts), and without the
    single terminal draw's own variance; None for "grid" (one draw per term).  n_free (N,) int64; bits_per_dim = nll / (n_free ln 2)
    (0 where nothing is free); accuracy: the share of masked entries, over all draws, whose argmax over s != m is x0 (NaN if no
    entry was masked); terms: the per-draw contributions, (K + 1, N) for "alpha" (the strata, then the terminal draw), (num_steps, N)
    or (num_steps + 1, N) for "grid"; n_masked, n_hit: the two counts behind `accuracy`."""
    nll: torch.Tensor
    stderr: object
    n_free: torch.Tensor
    bits_per_dim: torch.Tensor
    accuracy: float
    terms: torch.Tensor
    n_masked: int = 0
    n_hit: int = 0


def alpha_inverse(pr, u, t_lo, t_hi):
    """t in [t_lo, t_hi] with alpha(t) = u, fp64: closed form for loglinear, else a bisection (alpha is monotone decreasing) down to
    neighbouring fp64 times, taking the end with the smaller residual."""
    u = torch.as_tensor(u, dtype=torch.float64)
    if pr.p["t_func"] == "loglinear":
        return torch.clamp((1.0 - u) / (1.0 - pr.p["alpha_eps"]), t_lo, t_hi)
    lo, hi = torch.full_like(u, float(t_lo)), torch.full_like(u, float(t_hi))
    for _ in range(128):
        mid = 0.5 * (lo + hi)
        above = pr.alpha(mid) > u                   # alpha still too large: the root lies later
        lo, hi = torch.where(above, mid, lo), torch.where(above, hi, mid)
    return torch.where((pr.alpha(lo) - u).abs() <= (pr.alpha(hi) - u).abs(), lo, hi)


def _schedule(pr, spacing, N, n_times, num_steps, rule, min_t, max_t, gen):
    """Host fp64: (times (n, N), rate lam (n, N), weight (n, N)) of the n draws, each sample's own in "alpha"."""
    one = lambda v: torch.as_tensor(v, dtype=torch.float64).reshape(-1, 1).expand(-1, N)
    if spacing == "alpha":
        K = int(n_times)
        if K < 2:
            raise ValueError(f"n_times must be at least 2, got {n_times!r}")
        a_hi, a_lo = (float(v) for v in pr.alpha(torch.tensor([min_t, max_t], dtype=torch.float64)))
        R = a_hi - a_lo
        jitter = torch.rand((K, N), dtype=torch.float64, generator=gen)
        u = a_lo + R * (torch.arange(K, dtype=torch.float64).view(K, 1) + jitter) / K
        t = alpha_inverse(pr, u, min_t, max_t)
        lam_min = (1.0 - a_hi) / (1.0 - a_lo)
        return (torch.cat((t, one([min_t]))), torch.cat(((1.0 - u) / (1.0 - a_lo), one([lam_min]))),
                torch.cat((R / (1.0 - u), one([1.0]))))
    K = int(num_steps)
    if K < 1:
        raise ValueError(f"num_steps must be at least 1, got {num_steps!r}")
    ts = torch.from_numpy(np.concatenate((np.linspace(max_t, min_t, K), np.array([0.0]))))      # AbsorbingLeap._loop's grid
    p = torch.clamp(pr.unmask_prob(ts[:-1], ts[:-1] - ts[1:], rule), 0.0, 1.0)
    surv = torch.cat((torch.ones(1, dtype=torch.float64), torch.cumprod(1.0 - p, 0)))
    t, lam, wt = ts[:-1], surv[:-1], p
    if float(surv[-1]) > 0.0:                       # a closing draw at min_t for what the grid leaves masked
        t, lam, wt = torch.cat((t, torch.tensor([float(min_t)], dtype=torch.float64))), surv, torch.cat((p, torch.ones(1, dtype=torch.float64)))
    return one(t), one(lam), one(wt)


def _terms_torch(logits, x0, xt, m, w):
    """The draw's terms in fp64 torch ops: (w * per-sample sum, rows with a term, those whose argmax over s != m is x0)."""
    real = torch.arange(logits.shape[-1], device=logits.device) != m
    l = logits.double().masked_fill(~real, float("-inf"))
    term = (xt == m) & (x0 != m)
    idx = torch.where(term, x0, torch.full_like(x0, (m + 1) % logits.shape[-1])).long()
    nlp = -torch.log_softmax(l, -1).gather(-1, idx.unsqueeze(-1)).squeeze(-1)
    rows = torch.where(term, nlp, torch.zeros_like(nlp))
    return w.double() * rows.sum(1), term.sum(1), (term & (l.argmax(-1) == idx)).sum(1)


def absorbing_nll_bound(model, x0, *, spacing="alpha", n_times=16, num_steps=None, rule="ancestral", min_t, max_t, held=None, seed=None,
                        fused=True):
    """The bound of the module docstring for every sample of x0 (N, D) integer states -> LikelihoodBound.  held: bool (D,) or (N, D),
    True = given (as in the samplers' inpaint): the bound is on the free entries given the held ones.  seed: the Philox key of the
    mask draws and the generator seed of the strata's jitter (None: drawn from torch's global generator)."""
    pr = getattr(model, "process", None)
    if getattr(pr, "kind", None) != "absorbing":
        raise ValueError("absorbing_nll_bound needs a model on the absorbing process (AbsorbingRate, e.g. AbsorbingBertEMA)")
    if spacing not in SPACINGS:
        raise ValueError(f"spacing must be one of {SPACINGS}, got {spacing!r}")
    if rule not in UNMASK_RULES:
        raise ValueError(f"rule must be one of {UNMASK_RULES}, got {rule!r}")
    if spacing == "grid" and num_steps is None:
        raise ValueError('spacing "grid" takes the sampler\'s num_steps')
    if not 0.0 < float(min_t) < float(max_t):
        raise ValueError(f"expected 0 < min_t < max_t, got min_t = {min_t!r}, max_t = {max_t!r}")
    x0 = torch.as_tensor(x0)
    if x0.dim() != 2 or x0.shape[0] < 1 or x0.dtype.is_floating_point or x0.dtype.is_complex or x0.dtype == torch.bool:
        raise ValueError(f"x0: expected integer states (N, D), got {x0.dtype} {tuple(x0.shape)}")
    N, D = (int(v) for v in x0.shape)
    m, S = pr.mask_state, pr.S
    if held is None:
        hm = torch.zeros((N, D), dtype=torch.bool)
    else:
        hm = torch.as_tensor(held).cpu()
        if hm.dtype != torch.bool:
            raise ValueError(f"held: expected a bool tensor, got {hm.dtype}")
        if tuple(hm.shape) == (D,):
            hm = hm.view(1, D).expand(N, D)
        elif tuple(hm.shape) != (N, D):
            raise ValueError(f"held: expected shape ({D},) or {(N, D)}, got {tuple(hm.shape)}")
    xh = x0.cpu()                                   # (with `seed` the call's host round trip before the loop)
    if int(xh.min()) < 0 or int(xh.max()) >= S:
        raise ValueError(f"x0: states must lie in [0, {S})")
    if bool((xh[hm] == m).any()):
        raise ValueError(f"x0: a held entry is the mask state {m}")
    if bool((xh == m).any()):
        raise ValueError(f"x0: an entry is the mask state {m}, which is no data state")
    if seed is None:
        seed = int(torch.randint(0, 2**62, (1,), dtype=torch.int64).item())
    gen = torch.Generator().manual_seed(int(seed) % 2**63)
    t64, lam, wt = _schedule(pr, spacing, N, n_times, num_steps, rule, float(min_t), float(max_t), gen)
    n = t64.shape[0]
    n_free = (~hm).sum(1)
    if bool(hm.all()):                              # nothing to bound: no launch
        zero = torch.zeros(N, dtype=torch.float64)
        return LikelihoodBound(zero, zero.clone() if spacing == "alpha" else None, n_free, zero.clone(), float("nan"),
                               torch.zeros((n, N), dtype=torch.float64))
    dev = torch.device(model.device)
    on_gpu = dev.type == "cuda"
    keep, w32, t32 = (1.0 - lam).float().to(dev), wt.float().to(dev), t64.float().to(dev)
    xd = x0.to(dev).to(torch.int32).contiguous()
    hd = hm.to(dev) if held is not None else None
    buf = torch.zeros((n + 2, N), dtype=torch.float64, device=dev)      # the draws' terms, then the two counters for the one read-back
    masked, hit = (torch.zeros(N, dtype=torch.int32, device=dev) for _ in range(2))
    int32_states = on_gpu and getattr(model, "_engine_int32_states", False)
    with torch.no_grad(), borrow_engine_output(model, bf16_logits=False, uniform_time=spacing == "grid"):
        for k in range(n):
            if on_gpu:
                xt = native.absorb_noise(xd, keep[k].contiguous(), m, seed=seed, offset=k)
            else:
                xt = torch.where(torch.rand((N, D), generator=gen) >= keep[k].view(N, 1), torch.full_like(xd, m), xd)
            if hd is not None:
                xt = torch.where(hd, xd, xt)
            logits = model(xt if int32_states else xt.long(), t32[k].contiguous()).float().contiguous()
            if on_gpu and fused:
                native.absorb_nll(logits, xd, xt, m, w=w32[k].contiguous(), out=buf[k], masked=masked, hit=hit)
            else:
                val, nm, nh = _terms_torch(logits, xd, xt, m, w32[k])
                buf[k] += val
                masked += nm.to(torch.int32)
                hit += nh.to(torch.int32)
        buf[n] = masked.double()
        buf[n + 1] = hit.double()
    out = buf.cpu()                                 # the one read-back
    terms = out[:n]
    if spacing == "alpha":
        y = terms[:n - 1]
        nll, stderr = terms[n - 1] + y.mean(0), y.std(0, unbiased=True) / math.sqrt(n - 1)
    else:
        nll, stderr = terms.sum(0), None
    n_masked, n_hit = int(out[n].sum()), int(out[n + 1].sum())
    bpd = torch.where(n_free > 0, nll / (n_free.clamp(min=1).double() * math.log(2.0)), torch.zeros_like(nll))
    return LikelihoodBound(nll, stderr, n_free, bpd, n_hit / n_masked if n_masked else float("nan"), terms, n_masked, n_hit)


def eval_likelihood(cfg, model, dataloader, max_batches=None):
    """The held-out bound over a data loader.  Reads cfg.eval.{spacing ("alpha"), n_times (16), seed (0)} where the section exists,
    cfg.sampler.{min_t, num_steps, rule ("ancestral")} and cfg.training.max_t; batch b draws with the key seed + b.  Returns
    {"bits_per_dim", "nats_per_dim", "perplexity" = exp(nats_per_dim), "stderr", "accuracy", "n"}: the bound summed over the samples
    over the number of their entries; stderr: the standard error of the mean across samples of the per-sample bits per dimension;
    accuracy: the share of masked entries predicted by the argmax, over all draws; n: the number of samples.
    The bound describes the unfiltered samplers: a cfg.sampler that sets temperature, top_k or top_p away from 1, 0 and 1 draws from a
    truncated distribution, under which held-out data has no finite bound; one RuntimeWarning says so and the computation is unchanged."""
    ev, s = getattr(cfg, "eval", None), cfg.sampler
    knobs = {k: getattr(s, k, d) for k, d in (("temperature", 1.0), ("top_k", 0), ("top_p", 1.0))}
    if any(v != d for v, d in zip(knobs.values(), (1.0, 0, 1.0))):
        warnings.warn(f"eval_likelihood: cfg.sampler sets {knobs}; the bound is that of the unfiltered sampler (a tempered, truncated "
                      "distribution has no finite held-out bound)", RuntimeWarning, stacklevel=2)
    spacing, n_times, seed = (getattr(ev, k, d) for k, d in (("spacing", "alpha"), ("n_times", 16), ("seed", 0)))
    kw = dict(spacing=spacing, n_times=n_times, num_steps=getattr(s, "num_steps", None), rule=getattr(s, "rule", "ancestral"),
              min_t=s.min_t, max_t=cfg.training.max_t, fused=getattr(cfg.loss, "fused", True))
    nll, free, n_masked, n_hit = [], [], 0, 0
    for b, minibatch in enumerate(dataloader):
        if max_batches is not None and b >= max_batches:
            break
        x = minibatch[0] if isinstance(minibatch, (tuple, list)) else minibatch
        x = torch.as_tensor(x).long()                 # (as the training loop takes a minibatch)
        res = absorbing_nll_bound(model, x.reshape(x.shape[0], -1), seed=int(seed) + b, **kw)
        nll.append(res.nll)
        free.append(res.n_free)
        n_masked, n_hit = n_masked + res.n_masked, n_hit + res.n_hit
    if not nll:
        raise ValueError("eval_likelihood: the data loader gave no batch")
    nll, free = torch.cat(nll), torch.cat(free).double()
    nats = float(nll.sum() / free.sum())
    bpd = nll / (free * math.log(2.0))
    return {"bits_per_dim": nats / math.log(2.0), "nats_per_dim": nats, "perplexity": math.exp(nats),
            "stderr": float(bpd.std(unbiased=True) / math.sqrt(len(bpd))) if len(bpd) > 1 else float("nan"),
            "accuracy": n_hit / n_masked if n_masked else float("nan"), "n": int(len(bpd))}
