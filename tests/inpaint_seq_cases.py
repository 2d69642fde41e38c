"""Shared by tests/test_inpaint_seq_loss_cpu.py and tests/test_gpu_inpaint_seq_loss.py: the reference of the masked sequence
objectives (InpaintCatRM, InpaintScoreElbo) as the per-sample composition of the oracle's unmasked objectives -- called with
B = 1 on the gathered free rows of each sample -- plus the ragged masks and states both files use.  Host tensors only."""
import torch
import torch.nn.functional as F

EPS = 1e-9
CE_COEFF = 0.25


class Rows:
    """The stub model the oracle sees: returns the gathered logits, carries transition / rate."""

    def __init__(self, logits, qt0, rate=None):
        self.logits, self.qt0, self.rate_ = logits, qt0, rate

    def __call__(self, x, t):
        return self.logits

    def transition(self, t):
        return self.qt0

    def rate(self, t):
        return self.rate_


def _per_sample(free):
    for b in range(free.shape[0]):
        idx = free[b].nonzero().view(-1)
        if idx.numel():
            yield b, idx, (lambda t, b=b, idx=idx: t[b:b + 1][:, idx])


def ref_crm(logits, x0, x_t, free, qt0, *, logit_type, loss_type, ce_coeff, nll_weight):
    """(1 - ce_coeff)/B sum_b sum_{d in F_b} crm_bd + nll_weight (sum_b sum_{d in F_b} CE(l_bd, x0_bd)) / n_free."""
    from oracle import losses as ol
    B, S = x0.shape[0], logits.shape[-1]
    total, ce = logits.new_zeros(()), logits.new_zeros(())
    for b, idx, g in _per_sample(free):
        total = total + ol.crm_family("CatRM", Rows(g(logits), qt0[b:b + 1]), g(x0), None, g(x_t), S=S, logit_type=logit_type,
                                      loss_type=loss_type, ce_coeff=ce_coeff)
        ce = ce + F.cross_entropy(logits[b, idx], x0[b, idx], reduction="sum")
    return total / B + nll_weight * ce / max(int(free.sum()), 1)


def ref_score_elbo(logits, x0, x_t, x_tilde, free, qt0, rate, *, logit_type, nll_weight, one_forward_pass, eps=EPS):
    """(1/B) sum_b [ScoreElbo of sample b alone on its free rows]; a sample without a free row adds zero."""
    from oracle import losses as ol
    total = logits.new_zeros(())
    for b, idx, g in _per_sample(free):
        total = total + ol.score_elbo(Rows(g(logits), qt0[b:b + 1], rate[b:b + 1]), g(x0), None, g(x_t), g(x_tilde),
                                      logit_type=logit_type, eps=eps, nll_weight=nll_weight, one_forward_pass=one_forward_pass)
    return total / x0.shape[0]


def ragged_mask(B, D, seed=0):
    """(B, D) bool, True = free.  Sample 0: a single free row, the last one (so row 0 and every 4-row workgroup before it are
    held); sample 1: the two ends the other way round and, where D allows, a whole held run of 8 rows (two 4-row workgroups
    whatever the alignment leaves at least one fully held) between live ones; sample 2 (B >= 3): nothing free."""
    free = torch.rand(B, D, generator=torch.Generator().manual_seed(seed)) < 0.6
    free[0] = False
    free[0, D - 1] = True
    free[1, 0], free[1, D - 1] = True, False
    if D >= 14:
        free[1, 3:11] = False
        free[1, 2], free[1, 11] = True, True
    if B >= 3:
        free[2] = False
    return free


def states(x0, x_rand, free, S):
    """Full-shape x_t / x~ as the losses build them: x0 on held entries; x~ = x_t with one free entry of every sample moved."""
    x_t = torch.where(free, x_rand, x0)
    x_tilde = x_t.clone()
    for b in range(free.shape[0]):
        idx = free[b].nonzero().view(-1)
        if idx.numel():
            d = idx[min(1, idx.numel() - 1)]
            x_tilde[b, d] = (x_tilde[b, d] + 1) % S
    return x_t, x_tilde
