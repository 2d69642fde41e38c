"""Training losses behind the reference's registry names (lib/losses/losses.py): CTElbo 12-287,
NLL 1504-1778, CTElboLambda 1783-2058, CondCTElbo 547-781, CatRM 786-890, CatRMNLL 1135-1242,
NLLOriginal 1049-1103, ScoreElbo 1246-1500; and the inpainting objectives that have no counterpart there: InpaintCTElbo,
InpaintCatRM, InpaintScoreElbo (the CT-ELBO, CatRM / CatRMNLL and ScoreElbo of a per-sample set of free entries, lib/losses/masks.py),
and AbsorbingElbo (the absorbing-state process's negative ELBO, on its own kernels: csrc/absorb.hip).

Every loss = forward noising x0 -> x_t (and, for the ELBO family, the one-jump neighbour x~) followed
by an objective on the network's logits.  Noising runs in the HIP kernels K1/K2/K3 (per-sample
q_{t|0} / R_t tables, exponential-race categorical draws, csrc/noising.hip) with a Philox key taken
from torch's generator; the objectives are written as batched gathers and (B,D,S)x(B,S,S) products on
the device so autograd reaches the network (no index-vector construction, SURVEY 6: 63 % of the
reference's CPU time there).  Both argument orders of the reference are accepted: the class-level
`calc_loss(state, minibatch, label=None)` and the stale `calc_loss(minibatch, state)`.

Every objective exists once, with the held rows optional: `free` (B, D) bool names the entries that are noised and carry the
objective (None: all of them).  On a GPU value and logit-gradient come from the HIP kernels of csrc/losses.hip through one autograd
wrapper, _HipValueGrad; the plain-torch restatements below them are the CPU / S > 256 / cfg.loss.fused = False path.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

import lib.losses.losses_utils as losses_utils
import lib.utils.utils as utils
from ctdd import native
from lib.models.model_utils import get_logprob_with_logits


def _seed():
    return int(torch.randint(0, 2**62, (1,), dtype=torch.int64).item())


def _unpack(a, b):
    """(state, minibatch) in either order."""
    return (a, b) if isinstance(a, dict) else (b, a)


def _flatten(minibatch):
    if minibatch.dim() == 4:
        B, C, H, W = minibatch.shape
        minibatch = minibatch.view(B, C * H * W)
    return minibatch


# Parity-test hook: {"ts": (B,), "x_t": (B,D), "x_tilde": (B,D)} replaces the random draws so that the
# objective can be compared with the oracle on identical noise (tests/test_gpu_losses.py).
_FIXED_NOISE = None


def _draw_ts(B, device, lo, hi):
    if _FIXED_NOISE is not None:
        return _FIXED_NOISE["ts"].to(device)
    return torch.rand((B,), device=device) * (hi - lo) + lo


def _noise(model, x0, ts, with_tilde, want_T=False, free=None):
    """x_t ~ q_{t|0}(.|x0) per dimension and optionally the one-jump neighbour x~ (losses.py:39-101).
    Returns (qt0, qt0^T, rate, x_t, x~): tables (B,S,S), the transpose None unless want_T; int64 states, x~ None unless with_tilde.
    Under a mask `free` the held entries of x_t and x~ are x0 bit for bit and x~ moves a free entry."""
    fixed = _FIXED_NOISE is not None
    if getattr(model.process, "kind", None) == "absorbing":
        # (the one-jump neighbour is undefined at the all-mask state; nothing here has been checked on a zero rate row)
        raise ValueError("this objective runs the general S x S path, which does not cover the absorbing process: use AbsorbingElbo")
    qt0, qT, rate, probs = model.process.tables(ts, want_qt0=True, want_qt0T=want_T, want_rate=True, want_noise_probs=not fixed)
    if fixed:
        def pin(k):
            x = _FIXED_NOISE[k].to(x0.device).long()
            return x if free is None else torch.where(free, x, x0)
        return qt0, qT, rate, pin("x_t"), pin("x_tilde") if with_tilde else None
    x0i = x0.to(torch.int32).contiguous()
    x_t = native.noise_categorical(probs, x0i, seed=_seed())
    if free is not None:
        x_t = torch.where(free, x_t, x0i)
    if not with_tilde:
        return qt0, qT, rate, x_t.long(), None
    if free is None:
        _, _, x_tilde = native.xtilde_sample(rate, x_t, seed=_seed())
    else:
        _, _, x_tilde = native.xtilde_sample_masked(rate, x_t, free, seed=_seed())
    return qt0, qT, rate, x_t.long(), x_tilde.long()


def _tables_with_transpose(model, ts):
    """(q_{t|0}, its transpose), each (B,S,S): the transpose straight out of K1 when the model carries a device process."""
    pr = getattr(model, "process", None)
    if pr is not None and hasattr(pr, "tables"):
        qt0, qT, _, _ = pr.tables(ts, want_qt0=True, want_qt0T=True)
        return qt0, qT
    qt0 = model.transition(ts).float().contiguous()
    return qt0, qt0.transpose(1, 2).contiguous()


# ---------------------------------------------------------------- the HIP path: one autograd wrapper, one reverse-logit chain
class _HipValueGrad(torch.autograd.Function):
    """A value and its logit-gradient computed together by HIP (csrc/losses.hip).  `f` maps the detached fp32 contiguous logits to
    (value, d value / d logits) and holds every other operand; the gradient is saved and scaled in backward."""

    @staticmethod
    def forward(ctx, logits, f):
        val, grad = f(logits.detach().float().contiguous())
        ctx.save_for_backward(grad)
        return val

    @staticmethod
    def backward(ctx, g):
        (grad,) = ctx.saved_tensors
        return grad * g, None


def _i32(t):
    return None if t is None else t.to(torch.int32).contiguous()


def _fused(cfg, logits):
    return logits.is_cuda and logits.shape[-1] <= 256 and getattr(cfg.loss, "fused", True)


def _reverse_chain(lg, x, qt0, qT, logit_type, inner, x0=None, nll_scale=0.0):
    """An objective on ll_all for logit_type reverse_prob / reverse_logscale in HIP: ctdd_logprob -> inner(ll_all) = (value,
    d value / d ll_all) -> ctdd_logprob_bwd (a zero d/d ll_all row comes out as a zero logit-gradient row).  x0 given: CatRMNLL's
    cross-entropy term nll_scale * sum -log_softmax(lg)[x0] on the raw logits rides in the last launch.  Returns (value, d/d lg)."""
    tidx = torch.arange(lg.shape[0], dtype=torch.int32, device=lg.device)
    ll_all, _ = native.logprob(lg, x, qt0, logit_type, tidx, qt0T=qT)
    val, dll = inner(ll_all)
    grad, ce = native.logprob_bwd(logit_type, lg, qt0, qT, dll, x0, nll_scale, ll_all=ll_all)
    return (val if x0 is None else val + ce), grad


# ---------------------------------------------------------------- the plain-torch restatements (free = None: every row)
def _masked_rows(tab, x):
    """tab (B,S,S), x (B,D) -> tab[b, x_bd, :] with entry x_bd zeroed: (B,D,S)."""
    rows = tab[torch.arange(tab.shape[0], device=tab.device).view(-1, 1), x]
    return rows.scatter(-1, x.unsqueeze(-1), 0.0)


def _sum_d(v, free):
    """(B, D) -> (B): the sum over the sample's free rows."""
    return v.sum(1) if free is None else torch.where(free, v, torch.zeros_like(v)).sum(1)


def _sum_ds(v, free):
    """(B, D, S) -> (B): the sum over states and the sample's free rows."""
    return torch.sum(v, dim=(1, 2)) if free is None else _sum_d(torch.sum(v, dim=2), free)


def _signal_term(inner, x0, x_tilde, qt0, rate, eps, free):
    """mean_b(-outer_b / norm_b) of the CT-ELBO (losses.py:190-278) for the log-ratio `inner` (B,D,S).  Under a mask the base sum
    inside Z, outer and norm run over the sample's free rows; a sample without a free row contributes zero."""
    B = x0.shape[0]
    n = torch.arange(B, device=x0.device).view(B, 1)
    outer_rate = _masked_rows(rate.transpose(1, 2), x_tilde)      # rate[b, s, x~], s != x~
    q_x0 = qt0[n, x0]                                             # qt0[b, x0, s]
    q_x0_xt = torch.gather(q_x0, -1, x_tilde.unsqueeze(-1)) + eps  # (B,D,1)
    outer = _sum_ds(outer_rate * (q_x0 / q_x0_xt) * inner, free)
    row_sums = -torch.diagonal(rate, dim1=1, dim2=2)              # (B,S)
    base_tmp = row_sums[n, x_tilde]                               # (B,D)
    Z = _sum_d(base_tmp, free).view(B, 1, 1) - base_tmp.unsqueeze(-1) + row_sums.unsqueeze(1)
    if free is not None:
        Z = torch.where(free.unsqueeze(-1), Z, torch.ones_like(Z))                # (a held row's Z is not a normaliser of anything)
    sig_norm = _sum_ds(outer_rate * q_x0 / (Z * q_x0_xt), free)
    if free is None:
        return torch.mean(-outer / sig_norm)
    some = free.any(dim=1)
    return torch.mean(torch.where(some, -outer / torch.where(some, sig_norm, torch.ones_like(sig_norm)), torch.zeros_like(outer)))


def _ct_elbo_terms(logits_reg, logits_sig, x0, reg_x, x_tilde, qt0, rate, eps, free=None):
    """Negative CT-ELBO of tauLDR (losses.py:106-278): mean(-sig/norm) + mean(reg).  `free` (B, D) bool: every sum over dimensions
    restricted to the sample's free rows -- per sample the negative CT-ELBO of its free rows alone.  Full-shape operands."""
    n = torch.arange(x0.shape[0], device=x0.device).view(-1, 1)
    qT, rT = qt0.transpose(1, 2), rate.transpose(1, 2)            # qT[b,x,s0] = qt0[b,s0,x]; rT[b,x,s] = rate[b,s,x]
    p_reg = F.softmax(logits_reg, dim=2)
    reg_tmp = _masked_rows(rT, reg_x) @ qT                        # sum_s (mask*rate[s,x]) qt0[s0,s]
    reg_term = _sum_ds((p_reg / (qT[n, reg_x] + eps)) * reg_tmp, free)
    p_sig = p_reg if logits_sig is logits_reg else F.softmax(logits_sig, dim=2)
    inner = torch.log((p_sig / (qT[n, x_tilde] + eps)) @ qt0 + eps)
    return _signal_term(inner, x0, x_tilde, qt0, rate, eps, free) + torch.mean(reg_term)


def _score_elbo_terms(cfg, model, logits, x0, reg_x, x_tilde, ts, qt0, rate, eps, nll_weight, free=None):
    """ScoreElbo (losses.py:1246-1500): the CT-ELBO with the ratios exp(ll_all - ll_xt) + nll_weight * sum(-ll_xt) / B; under a mask
    every sum over dimensions runs over the sample's free rows."""
    ll_all, ll_xt = get_logprob_with_logits(cfg, model, x_tilde, ts, logits)
    d = ll_all - ll_xt.unsqueeze(-1)
    reg_term = _sum_ds(torch.exp(d) * _masked_rows(rate.transpose(1, 2), reg_x), free)
    neg_elbo = _signal_term(d, x0, x_tilde, qt0, rate, eps, free) + torch.mean(reg_term)
    nll = torch.sum(-ll_xt) if free is None else _sum_d(-ll_xt, free).sum()
    return neg_elbo + nll_weight * (nll / x0.shape[0])


def _ce_term(logits, x0, nll_weight, nll_scale, free):
    """nll_weight * mean CE(logits, x0); under a mask nll_scale * (the sum of CE over the free rows)."""
    if free is None:
        return nll_weight * F.cross_entropy(logits.permute(0, 2, 1), x0)
    ce = F.cross_entropy(logits.permute(0, 2, 1), x0, reduction="none")
    return nll_scale * torch.where(free, ce, torch.zeros_like(ce)).sum()


def _free_rows(name, cfg, minibatch):
    """The inpainting objectives' minibatch and mask: (x0 (B, D) int64, free (B, D) bool on x0's device, n_free).  The mask is
    drawn (or taken from the _FIXED_NOISE hook) and counted on the host; shape and config errors are ValueErrors before any
    device work."""
    import lib.losses.masks as masks
    minibatch = _flatten(minibatch)
    D = cfg.model.concat_dim
    if minibatch.dim() != 2 or minibatch.shape[1] != D or minibatch.shape[0] < 1:
        raise ValueError(f"{name}: minibatch of shape {tuple(minibatch.shape)}, model.concat_dim = {D}")
    B = int(minibatch.shape[0])
    if _FIXED_NOISE is not None and "free" in _FIXED_NOISE:
        masks.check_mask_config(cfg, D)
        free_host = torch.as_tensor(_FIXED_NOISE["free"]).cpu()
        if free_host.dtype != torch.bool or tuple(free_host.shape) != (B, D):
            raise ValueError(f"{name}: pinned free mask {free_host.dtype} {tuple(free_host.shape)}, expected bool {(B, D)}")
    else:
        free_host = masks.sample_free(cfg, B, D)
    n_free = int(free_host.sum())                                  # on the host: the cross-entropy weight is a plain float
    x0 = minibatch.long()
    # the step's one upload of the mask: from pinned memory, asynchronous -- a pageable copy would make the host wait for the device
    free = free_host.pin_memory().to(x0.device, non_blocking=True) if x0.is_cuda else free_host
    return x0, free, n_free


# ---------------------------------------------------------------- the CT-ELBO family
class _CTElboBase:
    def __init__(self, cfg):
        self.cfg = cfg
        self.ratio_eps = cfg.loss.eps_ratio
        self.nll_weight = cfg.loss.nll_weight
        self.min_time = cfg.loss.min_time
        self.one_forward_pass = cfg.loss.one_forward_pass
        self.max_t = cfg.training.max_t
        self.cross_ent = nn.CrossEntropyLoss()

    def _total(self, state, minibatch, elbo_scale, nll_coef):
        """elbo_scale * neg_elbo + nll_coef * CE(logits, x0).  On a GPU the objective and its logit gradient run in K11
        (csrc/losses.hip): one launch chain with one forward pass, one per network output with two."""
        model = state["model"]
        x0 = _flatten(minibatch).long()
        B, D = x0.shape
        ts = _draw_ts(B, model.device, self.min_time, self.max_t)
        qt0, qT, rate, x_t, x_tilde = _noise(model, x0, ts, True, want_T=True)
        x_logits = model(x_t, ts)
        if _fused(self.cfg, x_logits):
            eps, w, nll_scale = float(self.ratio_eps), float(elbo_scale), float(nll_coef) / (B * D)

            def k11(logits, x, elbo_scale, nll_scale, reg_scale=None):
                x0i, xi, tabs = _i32(x0), _i32(x), (qt0.contiguous(), qT.contiguous(), rate.contiguous())
                return _HipValueGrad.apply(logits, lambda lg: native.ctelbo_loss(lg, x0i, xi, *tabs, eps, elbo_scale, nll_scale, reg_scale))
            if self.one_forward_pass:
                return k11(x_logits, x_tilde, w, nll_scale)
            # two forward passes (losses.py:150-158): the regulariser and the cross entropy see model(x_t) at reg_x = x_t,
            # the signal term sees model(x~) at x~  --  K11 once per network output with the other term's weight at zero
            logits_sig = model(x_tilde, ts)
            return k11(x_logits, x_t, 0.0, nll_scale, w) + k11(logits_sig, x_tilde, w, 0.0, 0.0)
        if self.one_forward_pass:
            logits_sig, reg_x = x_logits, x_tilde
        else:
            logits_sig, reg_x = model(x_tilde, ts), x_t
        neg_elbo = _ct_elbo_terms(x_logits, logits_sig, x0, reg_x, x_tilde, qt0, rate, self.ratio_eps)
        nll = self.cross_ent(x_logits.permute(0, 2, 1), x0)
        return elbo_scale * neg_elbo + nll_coef * nll


@losses_utils.register_loss
class CTElbo(_CTElboBase):
    def calc_loss(self, state, minibatch, label=None):
        state, minibatch = _unpack(state, minibatch)
        return self._total(state, minibatch, 1.0, self.nll_weight)


@losses_utils.register_loss
class NLL(_CTElboBase):
    """Same sampling path as CTElbo, returns only the cross entropy (losses.py:1504-1778)."""

    def calc_loss(self, state, minibatch, label=None):
        state, minibatch = _unpack(state, minibatch)
        return self._total(state, minibatch, 0.0, 1.0)


@losses_utils.register_loss
class CTElboLambda(_CTElboBase):
    """w * neg_elbo + (1 - w) * nll with w = n_iter / n_iters (losses.py:1783-2058)."""

    def __init__(self, cfg):
        super().__init__(cfg)
        self.max_iter = cfg.training.n_iters

    def calc_loss(self, state, minibatch, label=None):
        state, minibatch = _unpack(state, minibatch)
        w = state["n_iter"] / self.max_iter
        return self._total(state, minibatch, w, 1 - w)


class _HeldCTElbo:
    """The body CondCTElbo and InpaintCTElbo share: the CT-ELBO of the rows that are not held.  t ~ U(min_time, 1); the single
    forward of one_forward_pass is at x~; with two passes the regulariser sees model(x_t) at reg_x = x_t and the signal term and
    the cross entropy see model(x~).  A subclass's _held_rows(minibatch) describes the held rows as (prefix, x0, free, n_ce):
    `prefix` (B, k) the held entries in front of the noised ones (k = 0 under a mask), x0 (B, d) the entries that are noised, `free`
    (B, d) bool the ones among them that carry the objective (None: all), n_ce the number of rows in the cross-entropy mean.
    On a GPU K11 reads the network's full (B, k + d, S) logits in place -- a row window (ctdd_ctelbo_loss_window) for a prefix, the
    free rows (ctdd_ctelbo_loss_masked) for a mask -- and the gradient comes back full shape with zeros on the held rows."""

    def __init__(self, cfg):
        self.cfg = cfg
        self.ratio_eps = cfg.loss.eps_ratio
        self.nll_weight = cfg.loss.nll_weight
        self.min_time = cfg.loss.min_time
        self.one_forward_pass = cfg.loss.one_forward_pass

    def calc_loss(self, minibatch, state=None, label=None):
        state, minibatch = _unpack(minibatch, state)
        prefix, x0, free, n_ce = self._held_rows(minibatch)
        model = state["model"]
        B, k = x0.shape[0], prefix.shape[1]
        ts = _draw_ts(B, model.device, self.min_time, 1.0)
        qt0, qT, rate, x_t, x_tilde = _noise(model, x0, ts, True, want_T=True, free=free)   # only the rows that are not held are noised
        eps, nll_scale = float(self.ratio_eps), float(self.nll_weight) / n_ce
        net = lambda x: model(torch.cat((prefix, x), dim=1) if k else x, ts)               # (B, k + d, S): the network sees held values
        if self.one_forward_pass:
            logits_sig = logits_reg = net(x_tilde)
            reg_x = x_tilde
        else:
            logits_reg = net(x_t)
            logits_sig = net(x_tilde)
            reg_x = x_t
        if _fused(self.cfg, logits_sig):
            def k11(logits, x, sig_scale, reg_scale, nll_scale):
                x0i, xi, tabs = _i32(x0), _i32(x), (qt0.contiguous(), qT.contiguous(), rate.contiguous())
                if free is None:
                    return _HipValueGrad.apply(logits, lambda lg: native.ctelbo_loss_window(lg, x0i, xi, *tabs, eps, sig_scale, reg_scale,
                                                                                              nll_scale, k))
                return _HipValueGrad.apply(logits, lambda lg: native.ctelbo_loss_masked(lg, x0i, xi, free, *tabs, eps, sig_scale, reg_scale,
                                                                                          nll_scale))
            if self.one_forward_pass:
                return k11(logits_sig, x_tilde, 1.0, 1.0, nll_scale)
            return k11(logits_reg, x_t, 0.0, 1.0, 0.0) + k11(logits_sig, x_tilde, 1.0, 0.0, nll_scale)
        l_reg = logits_reg[:, k:, :] if k else logits_reg                                  # (S > 256, cfg.loss.fused = False)
        l_sig = l_reg if self.one_forward_pass else logits_sig[:, k:, :] if k else logits_sig
        neg_elbo = _ct_elbo_terms(l_reg, l_sig, x0, reg_x, x_tilde, qt0, rate, self.ratio_eps, free)
        return neg_elbo + _ce_term(l_sig, x0, self.nll_weight, nll_scale, free)


@losses_utils.register_loss
class CondCTElbo(_HeldCTElbo):
    """CT-ELBO of the free rows given a held prefix (losses.py:547-781): the first `condition_dim` entries of every sample are the
    conditioner, passed to the network unnoised; rows condition_dim .. D-1 are noised and carry the objective.  What the
    conditional samplers (ConditionalTauLeaping / ConditionalPCTauLeaping) assume the model was trained with.

    Unlike CTElbo, t ~ U(min_time, 1) (567, no max_t), the single forward of one_forward_pass is at x~ (615-620), and with two
    passes the cross entropy is on the second (x~) forward's logits (665, 777-779)."""

    def __init__(self, cfg):
        super().__init__(cfg)
        self.condition_dim = cfg.loss.condition_dim
        self.cross_ent = nn.CrossEntropyLoss()

    def _held_rows(self, minibatch):
        minibatch = _flatten(minibatch)
        D, k = self.cfg.model.concat_dim, self.condition_dim
        if not (isinstance(k, int) and 0 < k < D):
            raise ValueError(f"CondCTElbo: loss.condition_dim must be an integer in (0, {D}), got {k!r}")
        if minibatch.dim() != 2 or minibatch.shape[1] != D:
            raise ValueError(f"CondCTElbo: minibatch of shape {tuple(minibatch.shape)}, model.concat_dim = {D}")
        x0_full = minibatch.long()
        return x0_full[:, :k], x0_full[:, k:].contiguous(), None, x0_full.shape[0] * (D - k)


@losses_utils.register_loss
class InpaintCTElbo(_HeldCTElbo):
    """CT-ELBO of a per-sample set of free entries given the held ones: what a model must be trained with for the samplers'
    `inpaint(model, x_known, mask)` under masks that are not a prefix.  cfg.loss.mask names the mask distribution
    (lib/losses/masks.py: prefix / bernoulli / half / box / mixture); the other fields are CondCTElbo's, and so are its
    conventions: t ~ U(min_time, 1), the one forward pass is at x~, with two passes the cross entropy is on the x~ forward.

    With free set F_b (n_b entries) of sample b:  x_t = x0 on held entries, ~ q_{t|0} on free ones;  x~ moves one free entry, chosen
    with probability rs[x_t^d] / sum_{d' in F_b} rs[x_t^d'];  the network sees the full state (held values, not the mask);
      loss = (1/B) sum_b neg_elbo_b + nll_weight * (sum_b sum_{d in F_b} CE_bd) / (sum_b n_b)
    where neg_elbo_b is the negative CT-ELBO of sample b on its free rows alone.  With mask = "prefix" this is CondCTElbo."""

    def __init__(self, cfg):
        super().__init__(cfg)
        self.mask = cfg.loss.mask

    def _held_rows(self, minibatch):
        x0, free, n_free = _free_rows("InpaintCTElbo", self.cfg, minibatch)
        return x0[:, :0], x0, free, max(n_free, 1)


# ---------------------------------------------------------------- categorical ratio matching
def _crm_loss(cfg, model, xt, t, ll_all, ll_xt):
    """Categorical ratio matching objectives (losses.py:794-836): rm / mle / elbo, per (b,d)."""
    S = cfg.data.S
    lt = cfg.loss.loss_type
    if lt == "rm":
        return -ll_xt
    if lt == "mle":
        return -((S - 1) * ll_xt + torch.sum(utils.log1mexp(ll_all), dim=-1) - utils.log1mexp(ll_xt))
    if lt == "elbo":
        qt0 = model.transition(t)
        n = torch.arange(xt.shape[0], device=xt.device).view(-1, 1)
        d = ll_all - ll_xt.unsqueeze(-1)
        own = F.one_hot(xt, S).to(ll_all.dtype)
        first = torch.sum(torch.exp(d) * qt0.transpose(1, 2)[n, xt] * (1 - own), dim=-1)
        second = torch.sum(-d * qt0[n, xt] * (1 - own), dim=-1)
        return first - second
    raise ValueError("Unknown loss_type: %s" % lt)


def _crm_reverse(logits, xt, x0, free, qt0, qT, logit_type, loss_type, scale, nll_scale):
    """The CRM objectives for logit_type reverse_prob / reverse_logscale in HIP: ctdd_logprob -> K12 on ll_all -> ctdd_logprob_bwd.
    The cross-entropy term (x0 given) is on the raw logits: without a mask it rides in the last launch, under a mask `free` it
    is one more ctdd_crm_loss_masked pass (loss_type rm, scale 0)."""
    xti, x0i, q_elbo = _i32(xt), _i32(x0), qt0 if loss_type == "elbo" else None

    def f(lg):
        if free is None:
            return _reverse_chain(lg, xti, qt0, qT, logit_type, lambda ll_all: native.crm_loss_ll(ll_all, xti, q_elbo, loss_type, scale),
                                  x0i, nll_scale)
        val, grad = _reverse_chain(lg, xti, qt0, qT, logit_type,
                                   lambda ll_all: native.crm_loss_ll_masked(ll_all, xti, free, q_elbo, loss_type, scale))
        if x0i is not None:
            ce, grad_ce = native.crm_loss_masked(lg, xti, x0i, free, None, "rm", 0.0, nll_scale)
            val, grad = val + ce, grad.add_(grad_ce)
        return val, grad
    return _HipValueGrad.apply(logits, f)


def _crm_objective(cfg, model, logits, xt, ts, x0, nll_weight, free=None, n_free=None, tables=None):
    """sum(loss_bd) (1 - ce_coeff) / B [+ nll_weight * CE(logits, x0)]; direct logits on a GPU run in K12.  `free` (B, D) bool with
    its count n_free: the sums run over the free rows and the cross entropy is their mean; `tables` = (q_{t|0}, its transpose)
    where the caller holds them already."""
    B, D = xt.shape
    kind, lt = cfg.loss.logit_type, cfg.loss.loss_type
    scale = (1.0 - cfg.loss.ce_coeff) / B
    nll_scale = float(nll_weight) / (B * D if free is None else max(n_free, 1)) if nll_weight else 0.0
    x0_ce = x0 if nll_weight else None
    # (without a mask the direct kernel runs whatever cfg.loss.fused says, as it always has)
    if kind == "direct" and logits.is_cuda and (free is None or getattr(cfg.loss, "fused", True)):
        qt0 = None
        if lt == "elbo":
            qt0 = (model.transition(ts) if tables is None else tables[0]).float().contiguous()
        xti, x0i, mask = _i32(xt), _i32(x0_ce), () if free is None else (free,)
        k12 = native.crm_loss if free is None else native.crm_loss_masked
        return _HipValueGrad.apply(logits, lambda lg: k12(lg, xti, x0i, *mask, qt0, lt, scale, nll_scale))
    if kind in ("reverse_prob", "reverse_logscale") and _fused(cfg, logits):
        qt0, qT = _tables_with_transpose(model, ts) if tables is None else tables
        return _crm_reverse(logits, xt, x0_ce, free, qt0.contiguous(), qT, kind, lt, scale, nll_scale)
    ll_all, ll_xt = get_logprob_with_logits(cfg, model, xt, ts, logits)      # (cfg.device == "cpu", S > 256, cfg.loss.fused = False)
    per_row = _crm_loss(cfg, model, xt, ts, ll_all, ll_xt)
    out = (torch.sum(per_row) if free is None else torch.where(free, per_row, torch.zeros_like(per_row)).sum()) * scale
    if nll_weight:
        out = out + _ce_term(logits, x0, nll_weight, nll_scale, free)
    return out


# The masked restatements under the names and argument orders tests/test_inpaint_seq_loss_cpu.py holds to the oracle: nothing of their
# own, the functions above with `free` given (the cross-entropy weight arrives as nll_scale = nll_weight / n_free).
def _crm_terms_masked(cfg, model, logits, x_t, ts, x0, free, nll_scale):
    return _crm_objective(cfg, model, logits, x_t, ts, x0, nll_scale, free, n_free=1)


def _score_elbo_terms_masked(cfg, model, logits, x0, reg_x, x_tilde, ts, free, qt0, rate, eps, nll_weight):
    return _score_elbo_terms(cfg, model, logits, x0, reg_x, x_tilde, ts, qt0, rate, eps, nll_weight, free)


class _CRMBase:
    clamp_t = True
    t_hi = 1.0

    def __init__(self, cfg):
        self.cfg = cfg
        self.ratio_eps = cfg.loss.eps_ratio
        self.min_time = cfg.loss.min_time
        self.S = cfg.data.S
        self.D = cfg.model.concat_dim

    def _forward(self, state, minibatch):
        model = state["model"]
        x0 = _flatten(minibatch).long()
        B = x0.shape[0]
        ts = _draw_ts(B, model.device, self.min_time, self.t_hi)
        if self.clamp_t:
            ts = torch.clamp(ts, max=0.99999)
        xt = _noise(model, x0, ts, False)[3]
        return model, x0, ts, xt


@losses_utils.register_loss
class CatRM(_CRMBase):
    def calc_loss(self, state, minibatch, label=None):
        state, minibatch = _unpack(state, minibatch)
        model, x0, ts, xt = self._forward(state, minibatch)
        logits = model(xt, ts)
        return _crm_objective(self.cfg, model, logits, xt, ts, None, 0.0)


@losses_utils.register_loss
class CatRMNLL(_CRMBase):
    """CatRM + nll_weight * CE(logits, x0), t ~ U(min_time, max_t) without clamp (losses.py:1135-1242)."""
    clamp_t = False

    def __init__(self, cfg):
        super().__init__(cfg)
        self.t_hi = cfg.training.max_t
        self.nll_weight = cfg.loss.nll_weight
        self.cross_ent = nn.CrossEntropyLoss()

    def calc_loss(self, minibatch, state=None, label=None):
        state, minibatch = _unpack(minibatch, state)
        model, x0, ts, xt = self._forward(state, minibatch)
        logits = model(xt, ts)
        return _crm_objective(self.cfg, model, logits, xt, ts, x0, self.nll_weight)


@losses_utils.register_loss
class NLLOriginal(_CRMBase):
    """Plain denoising cross entropy, t ~ U(min_time, 1) unclamped (losses.py:1049-1103)."""
    clamp_t = False

    def __init__(self, cfg):
        super().__init__(cfg)
        self.cross_ent = nn.CrossEntropyLoss()

    def calc_loss(self, state, minibatch, label=None):
        state, minibatch = _unpack(state, minibatch)
        model, x0, ts, xt = self._forward(state, minibatch)
        logits = model(xt, ts) if label is None else model(xt, ts, label)
        return self.cross_ent(logits.permute(0, 2, 1), x0)


@losses_utils.register_loss
class InpaintCatRM:
    """Categorical ratio matching of a per-sample set of free entries given the held ones: what a hollow / masked transformer must
    be trained with for `inpaint(model, x_known, mask)` of the CRM samplers.  cfg.loss.mask names the mask distribution
    (lib/losses/masks.py); loss_type rm / mle / elbo, logit_type, ce_coeff are CatRM's, nll_weight (default 0) CatRMNLL's.

    With free set F_b of sample b and n_free = sum_b |F_b|:  x_t = x0 on held entries, ~ q_{t|0} on free ones;  the network sees
    the full state (held values, not the mask);  t ~ U(min_time, 1) clamped to 0.99999;
      loss = (1 - ce_coeff)/B * sum_b sum_{d in F_b} crm_bd + nll_weight * (sum_b sum_{d in F_b} CE(l_bd, x0_bd)) / n_free.
    With an all-free mask this is CatRM (nll_weight = 0) or CatRMNLL's objective."""

    def __init__(self, cfg):
        self.cfg = cfg
        self.min_time = cfg.loss.min_time
        self.nll_weight = getattr(cfg.loss, "nll_weight", 0.0) or 0.0
        self.mask = cfg.loss.mask

    def calc_loss(self, minibatch, state=None, label=None):
        state, minibatch = _unpack(minibatch, state)
        cfg = self.cfg
        if cfg.loss.loss_type not in ("rm", "mle", "elbo"):
            raise ValueError(f"InpaintCatRM: loss.loss_type must be rm, mle or elbo, got {cfg.loss.loss_type!r}")
        if cfg.loss.logit_type not in native.LOGIT_TYPES:
            raise ValueError(f"InpaintCatRM: unknown loss.logit_type {cfg.loss.logit_type!r}")
        x0, free, n_free = _free_rows("InpaintCatRM", cfg, minibatch)
        model = state["model"]
        ts = torch.clamp(_draw_ts(int(x0.shape[0]), model.device, self.min_time, 1.0), max=0.99999)
        qt0, qT, _, x_t, _ = _noise(model, x0, ts, False, want_T=True, free=free)
        logits = model(x_t, ts)
        return _crm_objective(cfg, model, logits, x_t, ts, x0, self.nll_weight, free, n_free, tables=(qt0, qT))


# ---------------------------------------------------------------- ScoreElbo
@losses_utils.register_loss
class ScoreElbo:
    """CT-ELBO evaluated with SDDM ratios exp(ll_all - ll_xt) + nll_weight * mean(-ll_xt)
    (losses.py:1246-1500)."""

    def __init__(self, cfg):
        self.cfg = cfg
        self.ratio_eps = cfg.loss.eps_ratio
        self.nll_weight = cfg.loss.nll_weight
        self.min_time = cfg.loss.min_time
        self.one_forward_pass = cfg.loss.one_forward_pass

    def _rows(self, minibatch):
        """(x0 (B, D) int64, the mask of its free entries or None)."""
        return _flatten(minibatch).long(), None

    def calc_loss(self, minibatch, state=None, label=None):
        state, minibatch = _unpack(minibatch, state)
        x0, free = self._rows(minibatch)
        cfg, model = self.cfg, state["model"]
        B, kind = x0.shape[0], cfg.loss.logit_type
        eps, nll_scale = float(self.ratio_eps), float(self.nll_weight) / B
        ts = torch.clamp(_draw_ts(B, model.device, self.min_time, 1.0), max=0.99999)
        qt0, qT, rate, x_t, x_tilde = _noise(model, x0, ts, True, want_T=free is not None, free=free)
        reg_x = x_tilde if self.one_forward_pass else x_t
        logits = model(reg_x, ts)
        if kind in native.LOGIT_TYPES and _fused(cfg, logits):
            if kind != "direct" and free is None:                  # (the unmasked noising asks for no transpose: only this chain reads it)
                qT = _tables_with_transpose(model, ts)[1]
            mask = () if free is None else (free,)

            def f(lg):
                ops = (_i32(x0), _i32(x_tilde), _i32(reg_x), *mask, qt0.contiguous(), rate.contiguous())
                if kind == "direct":
                    return (native.score_elbo_loss if free is None else native.score_elbo_loss_masked)(lg, *ops, eps, nll_scale)
                k = native.score_elbo_loss_ll if free is None else native.score_elbo_loss_ll_masked
                return _reverse_chain(lg, ops[1], ops[-2], qT, kind, lambda ll_all: k(ll_all, *ops, eps, nll_scale))
            return _HipValueGrad.apply(logits, f)
        return _score_elbo_terms(cfg, model, logits, x0, reg_x, x_tilde, ts, qt0, rate, self.ratio_eps, self.nll_weight, free)


@losses_utils.register_loss
class InpaintScoreElbo(ScoreElbo):
    """ScoreElbo of a per-sample set of free entries given the held ones (cfg.loss.mask: lib/losses/masks.py; the other fields
    are ScoreElbo's).  x_t = x0 on held entries, ~ q_{t|0} on free ones;  x~ moves one free entry of x_t, chosen with probability
    rs[x_t^d] / sum_{d' in F_b} rs[x_t^d'];  reg_x = x~ with one forward pass and x_t with two, logits = model(reg_x, ts);
      loss = (1/B) sum_b (-outer_b / norm_b + reg_b) + (nll_weight/B) sum_b sum_{d in F_b} -ll_xt_bd
    with reg, outer, norm and the base sum inside Z over F_b only; a sample without a free row contributes zero.  With an all-free
    mask this is ScoreElbo."""

    def __init__(self, cfg):
        super().__init__(cfg)
        self.mask = cfg.loss.mask

    def _rows(self, minibatch):
        if self.cfg.loss.logit_type not in native.LOGIT_TYPES:
            raise ValueError(f"InpaintScoreElbo: unknown loss.logit_type {self.cfg.loss.logit_type!r}")
        return _free_rows("InpaintScoreElbo", self.cfg, minibatch)[:2]


# ---------------------------------------------------------------- absorbing-state diffusion
def _absorbing_elbo_terms(logits, x0, x_t, w, nll_scale, mask_state):
    """(1/B) sum_b w_b sum_{d: x_t = m, x0 != m} -lp[x0] + nll_scale sum_{x0 != m} -lp[x0], lp the log-softmax over the states
    s != m: the plain-torch statement of ctdd_absorb_elbo_loss (include/ctdd_absorb.h), in the logits' dtype."""
    B, m = x0.shape[0], int(mask_state)
    real = torch.arange(logits.shape[-1], device=logits.device) != m
    lp = F.log_softmax(logits.masked_fill(~real, float("-inf")), dim=-1)
    has = x0 != m
    nlp = -torch.gather(lp, -1, torch.where(has, x0, torch.full_like(x0, (m + 1) % logits.shape[-1])).unsqueeze(-1)).squeeze(-1)
    nlp = torch.where(has, nlp, torch.zeros_like(nlp))
    masked = torch.where(x_t == m, nlp, torch.zeros_like(nlp))
    return (w.to(nlp.dtype) * masked.sum(1)).sum() / B + nll_scale * nlp.sum()


@losses_utils.register_loss
class AbsorbingElbo:
    """Negative ELBO of the absorbing-state ("masked") process (lib.models.forward_model.AbsorbingRate), a weighted masked cross
    entropy:  t ~ U(min_time, max_t);  every entry of x_t is the mask state with probability 1 - alpha_t, else x0;  one forward at
    x_t;  loss = (1/B) sum_b w(t_b) sum_{d masked} -log p_theta(x0_d | x_t) + nll_weight * mean CE(logits, x0), with
    w = beta alpha / (1 - alpha) and every softmax over the states other than the mask.  On a GPU noising, value and logit
    gradient are the kernels of csrc/absorb.hip (no table, no contraction); cfg.loss.fused = False or a CPU model: torch ops."""

    def __init__(self, cfg):
        self.cfg = cfg
        self.nll_weight = getattr(cfg.loss, "nll_weight", 0.0) or 0.0
        self.min_time = cfg.loss.min_time
        self.max_t = cfg.training.max_t

    def calc_loss(self, state, minibatch, label=None):
        state, minibatch = _unpack(state, minibatch)
        model = state["model"]
        pr = getattr(model, "process", None)
        if getattr(pr, "kind", None) != "absorbing":
            raise ValueError("AbsorbingElbo needs a model on the absorbing process (AbsorbingRate, e.g. AbsorbingBertEMA)")
        m = pr.mask_state
        x0 = _flatten(minibatch).long()
        B, D = x0.shape
        ts = _draw_ts(B, model.device, self.min_time, self.max_t)
        w = pr.elbo_weight(ts).float().contiguous()
        nll_scale = float(self.nll_weight) / (B * D)
        on_gpu = x0.is_cuda and getattr(self.cfg.loss, "fused", True)
        if _FIXED_NOISE is not None:
            x_t = _FIXED_NOISE["x_t"].to(x0.device).long()
        elif on_gpu:
            x_t = native.absorb_noise(_i32(x0), pr.alpha(ts).float().contiguous(), m, seed=_seed()).long()
        else:
            x_t = torch.where(torch.rand(x0.shape, device=x0.device) >= pr.alpha(ts).view(B, 1), torch.full_like(x0, m), x0)
        logits = model(x_t, ts)
        if on_gpu and logits.is_cuda and logits.shape[-1] <= native.ABSORB_MAX_S:
            x0i, xti = _i32(x0), _i32(x_t)
            return _HipValueGrad.apply(logits, lambda lg: native.absorb_elbo_loss(lg, x0i, xti, w, nll_scale, m))
        return _absorbing_elbo_terms(logits, x0, x_t, w, nll_scale, m)


class d3pm_loss:
    """D3PM baseline objective (reference losses.py:1107-1130): a plain class, not registered -- the scripts build it as
    `d3pm_loss(cfg, make_diffusion(cfg.model))`.  One uniform integer step per sample, then the mean of
    CategoricalDiffusion.training_losses (lib/d3pm.py: ctdd_d3pm_loss on a GPU, torch ops on the CPU)."""

    def __init__(self, cfg, diffusion):
        self.cfg = cfg
        self.diffusion = diffusion
        self.device = cfg.device
        self.num_timesteps = cfg.model.num_timesteps

    def calc_loss(self, minibatch, state):
        model = state["model"]
        t = torch.randint(low=0, high=self.num_timesteps, size=(minibatch.shape[0],)).to(minibatch.device)
        return self.diffusion.training_losses(model, minibatch, t).mean()
