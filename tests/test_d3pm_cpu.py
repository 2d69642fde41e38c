"""CPU: the host path of lib/d3pm.py against the reference implementation's recorded outputs (tests/golden/d3pm.npz, written by
tools/gen_d3pm_golden.py).  Bounds: tables 2^-23 absolute (both sides round fp64-built one-step probabilities <= 1 to
fp32 and multiply those in fp32), logits atol 1e-4 (the project's fp32 logit bar), scalars rtol 1e-5,
integer draws equal (the same fp32 torch ops on the same inputs).

prior_bpd carries an absolute floor in place of its rtol in one situation only: where the value the reference recorded is itself
at the rounding level of the sum.  For the full uniform tables Qbar_{T-1} is the stationary distribution to the last bit or
two, the KL is zero, and the recorded values are the reference's own fp32 rounding (+-4e-8, negative for some samples) -- no
relative bound can hold against that.  The floor is the rounding of the sum: one fp32 ulp (2^-23) on every term's two
logarithms, sum_s q_s (|log q_s| + |log prior_s|), mean over dimensions, in bits; it applies only when every recorded value
is below it, and every other case keeps rtol 1e-5 alone."""
import numpy as np
import pytest
import torch

import d3pm_cases as dc
from conftest import load_golden

import lib.d3pm as d3pm
from lib.losses import losses

G = load_golden("d3pm")
CASES = [str(c) for c in G["cases"]]
KIND = {"uniform_full": "uniform", "uniform_band": "uniform", "gaussian_full": "gaussian", "gaussian_band": "gaussian",
        "absorbing_small": "absorbing", "absorbing": "absorbing"}
TAB = 2.0 ** -23


class Case:
    def __init__(self, name, loss_type="kl"):
        self.name = name
        self.g = {k.split(".", 1)[1]: v for k, v in G.items() if k.startswith(name + ".")}
        self.S, self.T, bands = int(self.g["S"]), int(self.g["T"]), int(self.g["bands"])
        self.kind = KIND[name]
        self.dif = d3pm.make_diffusion(dc.spec(self.kind, None if bands < 0 else bands, self.S, self.T, loss_type=loss_type))
        self.net = dc.ToyNet(self.S, self.T)

    def t(self, k):
        return torch.from_numpy(self.g[k])


def prior_floor(case, recorded):
    """0 unless every recorded value is below the fp32 rounding of the sum that produced it (module docstring)."""
    q = torch.from_numpy(case.g["q_mats"]).double()[-1][case.t("x_start")]
    prior = torch.full_like(q, 1.0 / case.S)
    floor = float(((q * (torch.log(q + 1e-6).abs() + torch.log(prior + 1e-6).abs())).sum(-1).mean(1) * TAB / np.log(2.0)).max())
    return floor if float(np.abs(recorded).max()) < floor else 0.0


@pytest.fixture(scope="module", params=CASES)
def case(request):
    return Case(request.param)


def test_cases_cover_the_schedules_and_tables():
    assert {KIND[c] for c in CASES} == {"uniform", "gaussian", "absorbing"}
    assert {int(G[c + ".S"]) for c in CASES} == {3, 16} and {int(G[c + ".T"]) for c in CASES} == {8, 20}
    assert {int(G[c + ".bands"]) for c in CASES} == {-1, 2}
    for c in CASES:
        assert {0, 1, int(G[c + ".T"]) - 1} <= set(G[c + ".t"].tolist())


def test_tables(case):
    d, g = case.dif, case.g
    for name in ("betas", "q_onestep_mats", "q_mats"):
        ours = getattr(d, name)
        assert ours.dtype == torch.float32
        assert np.abs(ours.numpy().astype(np.float64) - g[name].astype(np.float64)).max() <= TAB, name
    assert np.abs(d.q_mats.double().sum(-1).numpy() - 1.0).max() <= TAB * case.S
    assert torch.equal(d.q_mats_T, d.q_mats.transpose(1, 2)) and torch.equal(d.transpose_q_onestep_mats, d.q_onestep_mats.transpose(1, 2))


def test_q_sample_and_p_sample_draw_the_same_integers(case):
    d = case.dif
    np.testing.assert_allclose(d.q_probs(case.t("x_start"), case.t("t")).numpy(), case.g["q_probs"], atol=TAB, rtol=0)
    assert torch.equal(d.q_sample(case.t("x_start"), case.t("t"), case.t("noise_q")), case.t("x_t"))
    sample, probs = d.p_sample(case.net, x=case.t("x_t"), t=case.t("t"), noise=case.t("noise_p"))
    assert torch.equal(sample, case.t("p_sample"))
    np.testing.assert_allclose(probs.numpy(), case.g["p_sample_probs"], atol=1e-6, rtol=0)


def test_logits(case):
    d = case.dif
    x0, xt, t, pred = case.t("x_start"), case.t("x_t"), case.t("t"), case.t("pred")
    np.testing.assert_allclose(d.q_posterior_logits(x0, xt, t, x_start_logits=False).numpy(), case.g["post_int"], atol=1e-4, rtol=0)
    np.testing.assert_allclose(d.q_posterior_logits(pred, xt, t, x_start_logits=True).numpy(), case.g["post_logits"], atol=1e-4, rtol=0)
    model, p2 = d.p_logits(case.net, x=xt, t=t)
    np.testing.assert_allclose(model.numpy(), case.g["model_logits"], atol=1e-4, rtol=0)
    np.testing.assert_allclose(p2.numpy(), case.g["pred"], atol=1e-4, rtol=0)


def test_scalars(case):
    d = case.dif
    x0, xt, t = case.t("x_start"), case.t("x_t"), case.t("t")
    vb, pred = d.vb_terms_bpd(case.net, x_start=x0, x_t=xt, t=t)
    np.testing.assert_allclose(vb.numpy(), case.g["vb"], rtol=1e-5)
    np.testing.assert_allclose(d.cross_entropy_x_start(x0, pred).numpy(), case.g["ce"], rtol=1e-5)
    if "prior" in case.g:
        np.testing.assert_allclose(d.prior_bpd(x0).numpy(), case.g["prior"], rtol=1e-5, atol=prior_floor(case, case.g["prior"]))
    else:
        # absorbing: KL against the point mass on S // 2, eps inside both logs (the reference's branch raises; fp64 here)
        q = d.q_mats[-1].double()[x0]
        prior = torch.nn.functional.one_hot(torch.full(x0.shape, case.S // 2), case.S).double()
        ref = (q * (torch.log(q + 1e-6) - torch.log(prior + 1e-6))).sum(-1).mean(1) / np.log(2.0)
        np.testing.assert_allclose(d.prior_bpd(x0).numpy(), ref.numpy(), rtol=1e-5)


@pytest.mark.parametrize("name", CASES)
def test_training_losses(name, monkeypatch):
    x0, t = None, None
    vals = {}
    for lt in ("kl", "cross_entropy_x_start", "hybrid"):
        c = Case(name, lt)
        x0, t = c.t("x_start"), c.t("t")
        monkeypatch.setattr(d3pm, "_FIXED_NOISE", {"x_t": c.t("train_x_t")})
        vals[lt] = c.dif.training_losses(c.net, x0, t)
        if lt != "hybrid":
            np.testing.assert_allclose(vals[lt].numpy(), c.g["train_" + lt], rtol=1e-5)
    assert torch.equal(vals["hybrid"], vals["kl"] + 0.01 * vals["cross_entropy_x_start"])
    # the unhooked draw: the same torch.rand stream as the recorded run
    monkeypatch.setattr(d3pm, "_FIXED_NOISE", None)
    c = Case(name, "kl")
    torch.manual_seed(7 + CASES.index(name))
    np.testing.assert_allclose(c.dif.training_losses(c.net, x0, t).numpy(), c.g["train_kl"], rtol=1e-5)


def test_loops(case):
    d, idx = case.dif, CASES.index(case.name)
    if "bpd_total" in case.g:
        torch.manual_seed(11 + idx)
        out = d.calc_bpd_loop(case.net, case.t("x_start"))
        np.testing.assert_allclose(out["vbterms"].numpy(), case.g["bpd_vbterms"], rtol=1e-5)
        np.testing.assert_allclose(out["total"].numpy(), case.g["bpd_total"], rtol=1e-5)
        np.testing.assert_allclose(out["prior"].numpy(), case.g["bpd_prior"], rtol=1e-5, atol=prior_floor(case, case.g["bpd_prior"]))
    torch.manual_seed(13 + idx)
    x_init, x_end = d.p_sample_loop(case.net, tuple(case.g["loop_init"].shape), case.T, return_x_init=True)
    assert torch.equal(x_init.long(), case.t("loop_init").long()) and torch.equal(x_end.long(), case.t("loop_end").long())
    if case.kind == "absorbing":
        assert (x_init == case.S // 2).all()


def test_image_shape_gives_the_same_numbers(case):
    d = case.dif
    x0, xt, t = case.t("x_start"), case.t("x_t"), case.t("t")
    img = lambda v: v.reshape(v.shape[0], 1, 2, 3, *v.shape[2:])
    vb, pred = d.vb_terms_bpd(case.net, x_start=x0, x_t=xt, t=t)
    vbi, predi = d.vb_terms_bpd(case.net, x_start=img(x0), x_t=img(xt), t=t)
    assert predi.shape == (4, 1, 2, 3, case.S) and torch.equal(vb, vbi) and torch.equal(pred, predi.reshape(pred.shape))
    assert torch.equal(d.q_sample(img(x0), t, img(case.t("noise_q"))), img(xt))
    s, _ = d.p_sample(case.net, x=xt, t=t, noise=case.t("noise_p"))
    si, _ = d.p_sample(case.net, x=img(xt), t=t, noise=img(case.t("noise_p")))
    assert torch.equal(img(s), si)
    assert torch.equal(d.prior_bpd(x0), d.prior_bpd(img(x0)))
    flat_net = lambda x, tt: case.net(x, tt).reshape(x.shape[0], -1, case.S)       # a network that answers (B, D, S)
    assert torch.equal(d.p_logits(flat_net, x=img(xt), t=t)[0], d.p_logits(case.net, x=img(xt), t=t)[0])


def test_d3pm_loss_class(monkeypatch):
    c = Case(CASES[0], "hybrid")
    cfg = dc.ConfigDict()
    cfg.device = "cpu"
    cfg.model = dc.spec(c.kind, None, c.S, c.T, loss_type="hybrid")
    loss = losses.d3pm_loss(cfg, c.dif)
    monkeypatch.setattr(d3pm, "_FIXED_NOISE", {"x_t": c.t("train_x_t")})
    torch.manual_seed(3)
    val = loss.calc_loss(c.t("x_start"), {"model": c.net})
    torch.manual_seed(3)
    t = torch.randint(low=0, high=c.T, size=(4,))
    assert torch.equal(val, c.dif.training_losses(c.net, c.t("x_start"), t).mean())
    from lib.training import training
    assert training.call_calc_loss(loss, {"model": c.net}, c.t("x_start")).shape == ()


@pytest.mark.parametrize("which", ["mnist", "synthetic"])
def test_configs_construct_what_the_training_scripts_name(which):
    """make_diffusion, d3pm_loss, the model, optimizer and train step of the reference's train_*_d3pm.py, from the new configs."""
    import lib.models.model_utils as model_utils
    import lib.models.models  # noqa: F401
    import lib.optimizers.optimizers  # noqa: F401
    import lib.optimizers.optimizers_utils as optimizers_utils
    import lib.training.training  # noqa: F401
    import lib.training.training_utils as training_utils
    if which == "mnist":
        from config.mnist_config.config_mnist_d3pm import get_config
    else:
        from config.synthetic_config.config_synthetic_d3pm import get_config
    cfg = get_config()
    assert cfg.model.num_timesteps == (1000 if which == "mnist" else 500) and cfg.model.loss_type == "hybrid"
    assert cfg.model.name == ("GaussianTargetRateImageX0PredEMAPaul" if which == "mnist" else "UniBertD3PM")
    cfg.device = cfg.model.device = "cpu"
    cfg.model.num_timesteps = 6
    if which == "mnist":
        cfg.model.ch = 32
        cfg.model.time_embed_dim = 32
    model = model_utils.create_model(cfg, torch.device("cpu"))
    state = {"model": model, "optimizer": optimizers_utils.get_optimizer(model.parameters(), cfg), "n_iter": 0}
    dif = d3pm.make_diffusion(cfg.model)
    assert dif.fused == bool(cfg.model.d3pm_fused) and dif.num_timesteps == 6 and dif.q_mats.shape == (6, cfg.data.S, cfg.data.S)
    loss = losses.d3pm_loss(cfg, dif)
    step = training_utils.get_train_step(cfg)
    shape = (2, 1, 28, 28) if which == "mnist" else (2, 32)
    torch.manual_seed(0)
    x = torch.randint(0, cfg.data.S, shape)
    before = [p.detach().clone() for p in model.parameters()]
    val = step.step(state, x, loss)                       # the scripts' argument order
    assert torch.isfinite(val) and any(not torch.equal(a, b) for a, b in zip(before, model.parameters()))
    model.eval()
    out = dif.p_sample_loop(model, shape, 2)
    assert out.shape == shape and int(out.min()) >= 0 and int(out.max()) < cfg.data.S
