"""CPU: the inpainting objectives of the sequence models, InpaintCatRM and InpaintScoreElbo.
1. their plain-torch restatements (_crm_terms_masked, _score_elbo_terms_masked: the CPU / S > 256 / fused = False path) in fp64
   against the per-sample composition of oracle.losses.crm_family / score_elbo on the gathered free rows, on ragged masks;
2. with an all-free mask the classes are CatRM / CatRMNLL / ScoreElbo;
3. shape and config errors are ValueErrors raised before the model is touched;
4. the two inpainting configs build and register; the four masked entry points are declared, bound and exported."""
import inspect
import os
import re

import pytest
import torch

from inpaint_seq_cases import CE_COEFF, EPS, ragged_mask, ref_crm, ref_score_elbo, states

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B_, D_ = 4, 20
NLLW = 0.3
LOGIT_TYPES = ["direct", "reverse_prob", "reverse_logscale"]


class Model:
    """(x, t) -> fixed logits, with transition / rate and the `process.tables` the losses read under pinned noise."""
    device = "cpu"

    def __init__(self, logits, qt0, rate):
        self.logits, self.qt0, self.rate_, self.process, self.calls = logits, qt0, rate, self, []

    def __call__(self, x, t):
        self.calls.append(x.clone())
        return self.logits

    def transition(self, t):
        return self.qt0

    def rate(self, t):
        return self.rate_

    def tables(self, ts, want_qt0=False, want_qt0T=False, want_rate=False, want_noise_probs=False):
        return self.qt0, self.qt0.transpose(1, 2).contiguous(), self.rate_, None


class NoDevice:
    """A model stand-in whose every use fails: the checks must raise before the loss touches it."""

    def __getattr__(self, k):
        raise AssertionError(f"model.{k} used before the arguments were checked")

    def __call__(self, *a, **k):
        raise AssertionError("model called before the arguments were checked")


def _cfg(name, S, D=D_, **loss):
    from config.synthetic_config.config_hollow_synthetic_inpaint import get_config
    c = get_config()
    c.device = "cpu"
    c.data.S, c.model.concat_dim = S, D
    c.loss.update(name=name, ce_coeff=CE_COEFF, nll_weight=NLLW, eps_ratio=EPS, mask="bernoulli", mask_rate=[0.1, 0.9])
    c.loss.update(**loss)
    return c


def _case(S, all_free=False):
    from oracle.forward_process import ForwardProcess
    gen = torch.Generator().manual_seed(S)
    proc = ForwardProcess("uniform", S, rate_const=1.7, t_func="sqrt_cos")
    ts = torch.rand(B_, generator=gen) * 0.9 + 0.05
    qt0, rate = proc.transition(ts).double(), proc.rate(ts).double()
    x0 = torch.randint(0, S, (B_, D_), generator=gen)
    free = torch.ones(B_, D_, dtype=torch.bool) if all_free else ragged_mask(B_, D_, seed=S)
    x_t, x_tilde = states(x0, torch.randint(0, S, (B_, D_), generator=gen), free, S)
    logits = torch.randn(B_, D_, S, generator=gen, dtype=torch.float64)
    return ts, qt0, rate, x0, x_t, x_tilde, free, logits


def test_the_ragged_mask_is_ragged():
    free = ragged_mask(B_, D_, seed=3)
    assert int(free[0].sum()) == 1 and free[0, D_ - 1] and free[1, 0] and not free[1, D_ - 1] and not free[2].any() and free[3].any()


@pytest.mark.parametrize("S", [3, 37])
@pytest.mark.parametrize("logit_type", LOGIT_TYPES)
@pytest.mark.parametrize("loss_type", ["rm", "mle", "elbo"])
def test_crm_terms_masked_against_the_oracle_composition(loss_type, logit_type, S):
    import lib.losses.losses as L
    ts, qt0, _, x0, x_t, _, free, logits = _case(S)
    cfg = _cfg("InpaintCatRM", S, loss_type=loss_type, logit_type=logit_type)
    n_free = int(free.sum())
    want = ref_crm(logits, x0, x_t, free, qt0, logit_type=logit_type, loss_type=loss_type, ce_coeff=CE_COEFF, nll_weight=NLLW)
    lg = logits.clone().requires_grad_()
    got = L._crm_terms_masked(cfg, Model(lg, qt0, None), lg, x_t, ts, x0, free, NLLW / n_free)
    assert got.dtype == torch.float64 and torch.isfinite(got)
    torch.testing.assert_close(got.detach(), want, rtol=1e-10, atol=0)
    grad, = torch.autograd.grad(got, lg)
    assert torch.isfinite(grad).all() and (grad[~free] == 0).all() and (grad[free] != 0).any()
    no_ce = L._crm_terms_masked(cfg, Model(lg, qt0, None), lg, x_t, ts, x0, free, 0.0)
    want0 = ref_crm(logits, x0, x_t, free, qt0, logit_type=logit_type, loss_type=loss_type, ce_coeff=CE_COEFF, nll_weight=0.0)
    torch.testing.assert_close(no_ce.detach(), want0, rtol=1e-10, atol=0)


@pytest.mark.parametrize("S", [3, 37])
@pytest.mark.parametrize("logit_type", LOGIT_TYPES)
@pytest.mark.parametrize("one_pass", [True, False])
def test_score_elbo_terms_masked_against_the_oracle_composition(one_pass, logit_type, S):
    import lib.losses.losses as L
    ts, qt0, rate, x0, x_t, x_tilde, free, logits = _case(S)
    cfg = _cfg("InpaintScoreElbo", S, logit_type=logit_type, one_forward_pass=one_pass)
    want = ref_score_elbo(logits, x0, x_t, x_tilde, free, qt0, rate, logit_type=logit_type, nll_weight=NLLW, one_forward_pass=one_pass)
    lg = logits.clone().requires_grad_()
    reg_x = x_tilde if one_pass else x_t
    got = L._score_elbo_terms_masked(cfg, Model(lg, qt0, rate), lg, x0, reg_x, x_tilde, ts, free, qt0, rate, EPS, NLLW)
    assert got.dtype == torch.float64 and torch.isfinite(got)
    torch.testing.assert_close(got.detach(), want, rtol=1e-10, atol=0)
    grad, = torch.autograd.grad(got, lg)
    assert torch.isfinite(grad).all() and (grad[~free] == 0).all() and (grad[2] == 0).all() and (grad[free] != 0).any()
    # the fully held sample contributes zero: dropping it from the batch changes only the 1 / B
    keep = torch.tensor([0, 1, 3])
    sub = ref_score_elbo(logits[keep], x0[keep], x_t[keep], x_tilde[keep], free[keep], qt0[keep], rate[keep], logit_type=logit_type,
                         nll_weight=NLLW, one_forward_pass=one_pass)
    torch.testing.assert_close(want * B_, sub * 3, rtol=1e-12, atol=0)


def _run(name, S, case, pinned_free, **loss):
    import lib.losses.losses as L
    import lib.losses.losses_utils as lu
    ts, qt0, rate, x0, x_t, x_tilde, _, logits = case
    model = Model(logits, qt0, rate)
    fixed = {"ts": ts, "x_t": x_t, "x_tilde": x_tilde}
    if pinned_free is not None:
        fixed["free"] = pinned_free
    L._FIXED_NOISE = fixed
    try:
        val = lu.get_loss(_cfg(name, S, **loss)).calc_loss(x0, {"model": model, "n_iter": 0})
    finally:
        L._FIXED_NOISE = None
    return val, model


@pytest.mark.parametrize("S", [3, 37])
@pytest.mark.parametrize("logit_type", LOGIT_TYPES)
def test_all_free_masks_give_the_unmasked_objectives(logit_type, S):
    case = _case(S, all_free=True)
    case = case[:-1] + (case[-1].clone().requires_grad_(),)            # (the torch restatements of the log-probabilities need a graph)
    free = torch.ones(B_, D_, dtype=torch.bool)
    for loss_type in ("rm", "mle", "elbo"):
        for plain, nllw in (("CatRM", 0.0), ("CatRMNLL", NLLW)):
            want, m0 = _run(plain, S, case, None, logit_type=logit_type, loss_type=loss_type, nll_weight=nllw)
            got, m1 = _run("InpaintCatRM", S, case, free, logit_type=logit_type, loss_type=loss_type, nll_weight=nllw)
            assert len(m0.calls) == len(m1.calls) == 1 and torch.equal(m0.calls[0], m1.calls[0])
            torch.testing.assert_close(got, want, rtol=1e-12, atol=0)
    for one_pass in (True, False):
        want, m0 = _run("ScoreElbo", S, case, None, logit_type=logit_type, one_forward_pass=one_pass)
        got, m1 = _run("InpaintScoreElbo", S, case, free, logit_type=logit_type, one_forward_pass=one_pass)
        assert len(m0.calls) == len(m1.calls) == 1 and torch.equal(m0.calls[0], m1.calls[0])
        torch.testing.assert_close(got, want, rtol=1e-12, atol=0)


@pytest.mark.parametrize("name", ["InpaintCatRM", "InpaintScoreElbo"])
def test_the_classes_on_a_pinned_ragged_mask(name):
    """The class plumbing on the CPU path: held entries reach the model as x0, the value is the oracle composition."""
    S = 5
    case = _case(S)
    ts, qt0, rate, x0, x_t, x_tilde, free, logits = case
    case = case[:-1] + (logits.clone().requires_grad_(),)
    got, model = _run(name, S, case, free, logit_type="reverse_prob", loss_type="mle", one_forward_pass=True)
    assert len(model.calls) == 1 and torch.equal(model.calls[0][~free], x0[~free])
    if name == "InpaintCatRM":
        want = ref_crm(logits, x0, x_t, free, qt0, logit_type="reverse_prob", loss_type="mle", ce_coeff=CE_COEFF, nll_weight=NLLW)
    else:
        want = ref_score_elbo(logits, x0, x_t, x_tilde, free, qt0, rate, logit_type="reverse_prob", nll_weight=NLLW, one_forward_pass=True)
    torch.testing.assert_close(got.detach(), want, rtol=1e-10, atol=0)


BAD = ["mask_name", "mask_missing", "mask_rate", "width", "width_4d", "empty", "free_dtype", "free_shape", "logit_type"]


@pytest.mark.parametrize("name,bad", [("InpaintCatRM", b) for b in BAD + ["loss_type"]] + [("InpaintScoreElbo", b) for b in BAD])
def test_value_errors_before_any_device_work(name, bad):
    import lib.losses.losses as L
    import lib.losses.losses_utils as lu
    S = 4
    over = {"mask_name": dict(mask="diagonal"), "mask_missing": dict(mask=None), "mask_rate": dict(mask_rate=[0.9, 0.1]),
            "logit_type": dict(logit_type="logits"), "loss_type": dict(loss_type="kl")}.get(bad, {})
    shape = {"width": (3, D_ - 1), "width_4d": (3, 1, 3, 7), "empty": (0, D_)}.get(bad, (3, D_))
    loss = lu.get_loss(_cfg(name, S, **over))
    mb, state = torch.zeros(shape, dtype=torch.int64), {"model": NoDevice()}
    if bad in ("free_dtype", "free_shape"):
        free = torch.ones(3, D_, dtype=torch.bool)
        L._FIXED_NOISE = {"ts": None, "x_t": None, "x_tilde": None, "free": free.int() if bad == "free_dtype" else free[:, :-1]}
    try:
        with pytest.raises(ValueError):
            loss.calc_loss(mb, state)
        with pytest.raises(ValueError):
            loss.calc_loss(state, mb)
    finally:
        L._FIXED_NOISE = None


def test_registry_and_entry_points():
    import lib.losses.losses as L
    import lib.losses.losses_utils as lu
    from ctdd import native
    a, b = lu.get_loss(_cfg("InpaintCatRM", 3)), lu.get_loss(_cfg("InpaintScoreElbo", 3))
    assert type(a) is L.InpaintCatRM and type(b) is L.InpaintScoreElbo
    assert a.mask == b.mask == "bernoulli" and a.nll_weight == b.nll_weight == NLLW and b.ratio_eps == EPS and b.one_forward_pass is True
    c = _cfg("InpaintCatRM", 3)
    del c.loss["nll_weight"]
    assert lu.get_loss(c).nll_weight == 0.0                                       # nll_weight defaults to 0
    hdr = open(os.path.join(ROOT, "include", "ctdd.h")).read()
    for name in ("crm_loss_masked", "crm_loss_ll_masked", "score_elbo_loss_masked", "score_elbo_loss_ll_masked"):
        assert re.search(r"^int\s+ctdd_" + name + r"\s*\(", hdr, flags=re.M), name
        assert "ctdd_" + name in native.EXPORTS and callable(getattr(native, name))
    # one autograd wrapper for every fused objective, and the inpainting losses reach it through the bodies they share
    fns = [v for v in vars(L).values() if isinstance(v, type) and issubclass(v, torch.autograd.Function)]
    assert fns == [L._HipValueGrad]
    assert L.InpaintScoreElbo.calc_loss is L.ScoreElbo.calc_loss and L.InpaintCTElbo.calc_loss is L.CondCTElbo.calc_loss
    for body in (L.ScoreElbo.calc_loss, L.CondCTElbo.calc_loss, L._crm_objective, L._crm_reverse):
        assert "_HipValueGrad.apply(" in inspect.getsource(body), body
    assert "_crm_objective(" in inspect.getsource(L.InpaintCatRM.calc_loss)


@pytest.mark.parametrize("which", ["maze", "synthetic"])
def test_inpaint_configs(which):
    import importlib
    import lib.losses.losses as L
    import lib.losses.losses_utils as lu
    import lib.sampling.sampling as ls
    import lib.sampling.sampling_utils as su
    from lib.losses.masks import check_mask_config, sample_free
    base_name = {"maze": "config.maze_config.config_hollow_maze", "synthetic": "config.synthetic_config.config_hollow_synthetic"}[which]
    c, b = importlib.import_module(base_name + "_inpaint").get_config(), importlib.import_module(base_name).get_config()
    D = int(c.model.concat_dim)
    if which == "maze":
        assert c.loss.name == "InpaintScoreElbo" and type(lu.get_loss(c)) is L.InpaintScoreElbo and c.loss.mask == "mixture"
        assert sorted(n for n, _ in c.loss.mask_mixture) == ["bernoulli", "box", "half"] and list(c.loss.mask_rate) == [0.1, 0.9]
        assert c.sampler.condition_dim == 105 == 7 * 15 and D == 225 and list(c.data.shape) == [1, 15, 15]
    else:
        assert c.loss.name == "InpaintCatRM" and type(lu.get_loss(c)) is L.InpaintCatRM and c.loss.mask == "bernoulli"
        assert c.loss.loss_type == "rm" and c.loss.logit_type == "reverse_prob" and 0 < c.sampler.condition_dim < D == 32
    assert c.sampler.name == "ConditionalLBJF" and type(su.get_sampler(c)) is ls.ConditionalLBJF
    assert check_mask_config(c, D) == c.loss.mask
    torch.manual_seed(0)
    free = sample_free(c, 16, D)
    assert free.shape == (16, D) and free.dtype == torch.bool and free.any(1).all() and not free.all()
    for sec in ("model", "data", "training", "optimizer"):             # the network and the data are the base config's
        assert c[sec].to_dict() == b[sec].to_dict(), sec
    for k in ("eps_ratio", "min_time", "one_forward_pass", "ce_coeff"):
        assert c.loss[k] == b.loss[k]
    assert b.loss.name == "ScoreElbo" and b.sampler.name == "CRMLBJF"   # the base config is untouched
