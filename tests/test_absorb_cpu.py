"""CPU: the absorbing-state ("masked") process and its objective and sampler without a GPU -- schedule identities, the closed-form
eigensystem against the closed-form q_t, the torch restatement of the objective against the fp64 case evaluation, registry names,
the shipped configs, the refusals of foreign combinations and of CPU tensors."""
import importlib
import types

import numpy as np
import pytest
import torch

import absorb_cases as ac
from ctdd import native, process

CONFIGS = ("synthetic_config.config_bert_synthetic_absorb", "maze_config.config_bert_maze_absorb")


def _proc(S=5, m=None, **kw):
    p = dict(rate_const=1.0, t_func="loglinear", alpha_eps=1e-3, mask_state=S - 1 if m is None else m)
    p.update(kw)
    if p["t_func"] == "log":
        p.update(time_base=3.0, time_exp=100.0)
    return process.DeviceForwardProcess("absorbing", S, "cpu", **p)


def _registries():
    import lib.models.models  # noqa: F401
    import lib.models.model_utils as mu
    import lib.losses.losses  # noqa: F401
    import lib.losses.losses_utils as lu
    import lib.sampling.sampling  # noqa: F401
    import lib.sampling.sampling_utils as su
    return mu, lu, su


def _shipped(mod):
    mu = _registries()[0]
    cfg = importlib.import_module("config." + mod).get_config()
    cfg.device = "cpu"
    cfg.model.update(num_layers=1, engine="torch")
    torch.manual_seed(0)
    return cfg, mu.create_model(cfg, torch.device("cpu"))


# ------------------------------------------------------------------------------------------------ schedules
@pytest.mark.parametrize("t_func,rate_const", [("loglinear", 1.0), ("log_sqr", 2.0), ("sqrt_cos", 1.55), ("log", 0.5)])
def test_schedule_identities(t_func, rate_const):
    pr = _proc(t_func=t_func, rate_const=rate_const)
    t = torch.tensor([0.05, 0.3, 0.7, 0.95], dtype=torch.float64)
    assert float(pr.alpha(torch.zeros(1, dtype=torch.float64))) == 1.0
    a = pr.alpha(t)
    assert bool((a[1:] < a[:-1]).all()) and bool((a > 0).all()) and bool((a < 1).all())
    # alpha = exp(-c), c' = rate_const beta: elbo_weight = -alpha' / (1 - alpha), against a central difference
    d = 1e-6
    num = -(pr.alpha(t + d) - pr.alpha(t - d)) / (2 * d) / (1 - a)
    np.testing.assert_allclose(pr.elbo_weight(t).numpy(), num.numpy(), rtol=1e-6)
    if t_func == "loglinear":
        np.testing.assert_allclose(pr.elbo_weight(t).numpy(), (1 / t).numpy(), rtol=1e-14)
        np.testing.assert_allclose(a.numpy(), (1 - (1 - 1e-3) * t).numpy(), rtol=1e-14)
    # ancestral: 1 at t - h = 0, and the survival of the mask telescopes over a grid
    assert float(pr.unmask_prob(t[2:3], float(t[2]), "ancestral")) == 1.0
    grid = torch.linspace(0.95, 0.05, 7, dtype=torch.float64)
    p = pr.unmask_prob(grid[:-1], grid[:-1] - grid[1:], "ancestral")
    assert bool((p > 0).all()) and bool((p < 1).all())
    surv = torch.cumprod(1 - p, 0)
    want = (1 - pr.alpha(grid[1:])) / (1 - pr.alpha(grid[0]))
    np.testing.assert_allclose(surv.numpy(), want.numpy(), rtol=1e-10)
    lam = 0.01 * pr.elbo_weight(t)
    np.testing.assert_allclose(pr.unmask_prob(t, 0.01, "euler").numpy(), torch.clamp(lam, max=1.0).numpy(), rtol=1e-14)
    np.testing.assert_allclose(pr.unmask_prob(t, 0.01, "tauleap").numpy(), (lam * torch.exp(-lam)).numpy(), rtol=1e-14)
    assert float(pr.unmask_prob(torch.tensor([0.001], dtype=torch.float64), 0.5, "euler")) == 1.0
    with pytest.raises(ValueError):
        pr.unmask_prob(t, 0.01, "midpoint")


def test_process_argument_errors():
    with pytest.raises(ValueError, match="rate_const"):
        _proc(rate_const=2.0)
    with pytest.raises(ValueError, match="mask_state"):
        _proc(S=4, m=4)
    with pytest.raises(ValueError, match="t_func"):
        _proc(t_func="linear")
    with pytest.raises(ValueError, match="absorbing"):
        process.DeviceForwardProcess("uniform", 4, "cpu", rate_const=1.0).alpha(torch.ones(1))


@pytest.mark.parametrize("S,m", [(5, 0), (5, 2), (7, 6)])
def test_closed_form_eigensystem_gives_closed_form_qt(S, m):
    rc = 1.7
    R = process.absorbing_rate_matrix(S, rc, m)
    lam, V, W = process.absorbing_eigensystem(S, rc, m)
    np.testing.assert_allclose(V @ W, np.eye(S), atol=0)
    np.testing.assert_allclose(V @ np.diag(lam) @ W, R, atol=1e-15)
    assert (R.sum(1) == 0).all() and (R[m] == 0).all()
    for c in (0.0, 0.3, 2.5):
        q = V @ np.diag(np.exp(c * lam)) @ W
        np.testing.assert_allclose(q, ac.closed_form_qt(S, m, np.exp(-rc * c)), atol=1e-15)
    pr = _proc(S=S, m=m, t_func="log_sqr", rate_const=rc)
    np.testing.assert_allclose(pr.base_rate.numpy(), R.astype(np.float32))
    np.testing.assert_allclose(pr.eigvecs.numpy() @ np.diag(pr.eigvals.numpy()) @ pr.right.numpy(), R.astype(np.float32), atol=1e-6)


# ------------------------------------------------------------------------------------------------ the objective's torch statement
@pytest.mark.parametrize("mode", ac.MODES)
@pytest.mark.parametrize("case", ac.CASES[:5], ids=ac.IDS[:5])
def test_torch_objective_against_fp64_cases(case, mode):
    from lib.losses.losses import _absorbing_elbo_terms
    S, m, B, D = case
    logits, x0, w = ac.inputs(case)
    x_t, nll_scale = ac.x_t_of(case, mode), ac.nll_scale_of(case, mode)
    (v64, g64), _ = ac.loss_refs(case, mode)
    l = logits.double().clone().requires_grad_(True)
    val = _absorbing_elbo_terms(l, x0, x_t, w, nll_scale, m)
    if val.requires_grad:
        val.backward()
    grad = torch.zeros_like(l) if l.grad is None else l.grad
    assert torch.isfinite(val) and bool(torch.isfinite(grad).all())
    np.testing.assert_allclose(float(val.detach()), float(v64), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(grad.numpy(), g64.numpy(), rtol=0, atol=1e-12)
    carries = ac.term_rows(case, mode)
    assert bool((grad[~carries] == 0).all()), "a row without a term has a non-zero gradient"
    assert bool((grad[..., m] == 0).all()), "the mask state's column has a non-zero gradient"
    if mode == "none":
        assert float(val.detach()) == 0.0
    # the same in fp32 (what the fallback runs in): finite where the mask logit leads the row by 50
    l32 = logits.clone().requires_grad_(True)
    v32 = _absorbing_elbo_terms(l32, x0, x_t, w, nll_scale, m)
    assert torch.isfinite(v32)
    np.testing.assert_allclose(float(v32.detach()), float(v64), rtol=1e-5, atol=1e-6)


# ------------------------------------------------------------------------------------------------ registries, configs, refusals
def test_registry_names_resolve():
    mu, lu, su = _registries()
    assert mu.get_model("AbsorbingBertEMA").__name__ == "AbsorbingBertEMA"
    assert lu._LOSSES["AbsorbingElbo"].__name__ == "AbsorbingElbo"
    assert su._SAMPLERS["AbsorbingLeap"].__name__ == "AbsorbingLeap"
    assert "absorbing" in process.DeviceForwardProcess.KINDS


@pytest.mark.parametrize("mod", CONFIGS)
def test_shipped_configs_build_and_take_a_loss_on_the_cpu(mod):
    mu, lu, su = _registries()
    cfg, model = _shipped(mod)
    S, D = cfg.data.S, cfg.model.concat_dim
    assert model.process.kind == "absorbing" and model.mask_state == model.process.mask_state == S - 1 == cfg.model.mask_state
    assert cfg.loss.name == "AbsorbingElbo" and cfg.sampler.name == "AbsorbingLeap" and cfg.model.name == "AbsorbingBertEMA"
    assert su.get_sampler(cfg).rule == "ancestral"
    loss = lu.get_loss(cfg)
    x = torch.randint(0, S - 1, (2, D))
    torch.manual_seed(1)
    val = loss.calc_loss({"model": model, "n_iter": 0}, x)
    torch.manual_seed(1)
    again = loss.calc_loss(x, {"model": model, "n_iter": 0})          # the stale argument order
    assert torch.isfinite(val) and float(val.detach()) > 0 and float(val.detach()) == float(again.detach())
    val.backward()
    assert any(p.grad is not None and float(p.grad.abs().max()) > 0 for p in model.parameters())
    # tables for users' own code: the process mixin's surface on the closed-form eigensystem
    assert model.eigvals.shape == (S,) and model.rate_matrix.shape == (S, S)
    np.testing.assert_allclose(model.rate_mat(torch.tensor([[0, S - 1]]), torch.tensor([0.5])).numpy()[0, 1], np.zeros(S))


def test_initial_samples_absorbing():
    from lib.sampling.sampling import get_initial_samples
    x = get_initial_samples(3, 4, "cpu", 5, "absorbing")
    assert x.dtype == torch.int64 and tuple(x.shape) == (3, 4) and bool((x == 4).all())
    assert bool((get_initial_samples(3, 4, "cpu", 5, "absorbing", mask_state=1) == 1).all())
    with pytest.raises(ValueError):
        get_initial_samples(3, 4, "cpu", 5, "absorbing", mask_state=5)
    with pytest.raises(NotImplementedError):
        get_initial_samples(3, 4, "cpu", 5, "masked")


@pytest.mark.parametrize("loss_name", ["CTElbo", "CatRM", "ScoreElbo", "NLLOriginal"])
def test_general_losses_refuse_an_absorbing_model(loss_name):
    mu, lu, su = _registries()
    cfg, model = _shipped(CONFIGS[0])
    cfg.loss.update(name=loss_name, eps_ratio=1e-9, one_forward_pass=True, nll_weight=0.0, logit_type="direct", loss_type="rm",
                    ce_coeff=0.0)
    x = torch.randint(0, cfg.data.S - 1, (2, cfg.model.concat_dim))
    with pytest.raises(ValueError, match="AbsorbingElbo"):
        lu.get_loss(cfg).calc_loss(x, {"model": model, "n_iter": 0})


@pytest.mark.parametrize("sampler_name", ["TauL", "LBJF", "ExactSampling"])
def test_general_samplers_refuse_an_absorbing_model(sampler_name):
    mu, lu, su = _registries()
    cfg, model = _shipped(CONFIGS[0])
    cfg.sampler.update(name=sampler_name, initial_dist="uniform")
    with pytest.raises(ValueError, match="AbsorbingLeap"):
        su.get_sampler(cfg).sample(model, 2)


def test_absorbing_objective_and_sampler_refuse_other_processes():
    mu, lu, su = _registries()
    cfg, _ = _shipped(CONFIGS[0])
    other = types.SimpleNamespace(process=process.DeviceForwardProcess("uniform", cfg.data.S, "cpu", rate_const=1.0), device="cpu")
    x = torch.randint(0, cfg.data.S - 1, (2, cfg.model.concat_dim))
    with pytest.raises(ValueError, match="absorbing"):
        lu.get_loss(cfg).calc_loss(x, {"model": other, "n_iter": 0})
    with pytest.raises(ValueError, match="absorbing"):
        su.get_sampler(cfg).sample(other, 2)
    with pytest.raises(ValueError, match="absorbing"):
        su.get_sampler(cfg).inpaint(other, x, torch.zeros(cfg.model.concat_dim, dtype=torch.bool))
    cfg.sampler.rule = "midpoint"
    with pytest.raises(ValueError, match="rule"):
        su.get_sampler(cfg)


def test_native_absorb_calls_refuse_cpu_tensors():
    logits, x, w = torch.zeros(2, 3, 4), torch.zeros(2, 3, dtype=torch.int32), torch.ones(2)
    with pytest.raises(native.CtddError):
        native.absorb_noise(x, torch.full((2,), 0.5), 3)
    with pytest.raises(native.CtddError):
        native.absorb_elbo_loss(logits, x, x, w, 0.0, 3)
    with pytest.raises(native.CtddError):
        native.absorb_step(logits, x, 3, 0.5)
