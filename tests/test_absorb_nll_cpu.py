"""CPU: the held-out likelihood bounds of lib/likelihood.py without a GPU -- the estimators on the torch path against their closed
forms, the inverse of alpha for the four schedules, the torch statement of the row terms against the fp64 case evaluation, held
entries, refusals and argument errors, and the binding's refusal of CPU tensors."""
import math
import types

import numpy as np
import pytest
import torch

import absorb_cases as ac
import absorb_nll_cases as nc
import lib.likelihood as lk
from ctdd import native, process


# ------------------------------------------------------------------------------------------------ the estimators
@pytest.mark.parametrize("spacing", ["alpha", "grid"])
def test_bounds_are_tight_for_a_network_that_ignores_x_t(spacing):
    """Logits that depend on d only: the exact expectation of either bound is sum_d c_d and the per-sample variance is exact too;
    the batch mean within 5 sigma / sqrt(N) (the per-sample spread is printed beside its exact value)."""
    S, m, D, N, K, steps, min_t, max_t = 6, 2, 30, 256, 16, 10, 0.01, 1.0
    model = nc.DimOnlyModel(S, m, D, "cpu")
    x0 = nc.data(S, m, N, D)
    c = model.cross_entropies(x0[0])
    res = lk.absorbing_nll_bound(model, x0, spacing=spacing, n_times=K, num_steps=steps, min_t=min_t, max_t=max_t, seed=1234)
    if spacing == "alpha":
        sigma = nc.alpha_sigma(model.process, c, K, min_t, max_t)
        assert tuple(res.terms.shape) == (K + 1, N) and tuple(res.stderr.shape) == (N,) and bool((res.stderr > 0).all())
        np.testing.assert_allclose(res.nll.numpy(), (res.terms[K] + res.terms[:K].mean(0)).numpy(), rtol=1e-14)
    else:
        _, p, surv, last = nc.grid_of(model.process, steps, min_t, max_t, "ancestral")
        sigma = math.sqrt(float((p ** 2 * surv * (1 - surv)).sum()) * float((c ** 2).sum()))
        assert last == 0.0 and tuple(res.terms.shape) == (steps, N) and res.stderr is None
        np.testing.assert_allclose(res.nll.numpy(), res.terms.sum(0).numpy(), rtol=1e-14)
    mean, want, spread = float(res.nll.mean()), float(c.sum()), float(res.nll.std())
    print(f"{spacing}: batch mean {mean:.4f}, exact {want:.4f}, sigma / sqrt(N) {sigma / math.sqrt(N):.4f}; per-sample std {spread:.3f}, "
          f"exact {sigma:.3f}")
    assert abs(mean - want) <= 5 * sigma / math.sqrt(N)
    assert res.nll.dtype == torch.float64 and bool((res.n_free == D).all())
    np.testing.assert_allclose(res.bits_per_dim.numpy(), res.nll.numpy() / (D * math.log(2.0)), rtol=1e-14)
    assert res.n_masked > 0 and res.accuracy == res.n_hit / res.n_masked


@pytest.mark.parametrize("rule", ["ancestral", "tauleap"])
def test_grid_bound_is_the_samplers_bound(rule):
    """Time-only logits: E[bound] = sum_i pi_i CE_i(x0) (+ surv_K CE(t_min) where the rule leaves a share masked), pi_i = surv_i p_i;
    under the ancestral rule at least the sampler's exact -sum_d log sum_i pi_i p_i(x0_d); the grid's p_i are unmask_prob on the
    sampler's grid."""
    S, m, N, D, K, min_t, max_t = 6, 2, 256, 30, 10, 0.01, 1.0
    model = nc.TimeOnlyModel(S, m, "cpu")
    pr = model.process
    x0 = nc.data(S, m, N, D)
    ts, p, surv, last = nc.grid_of(pr, K, min_t, max_t, rule)
    t64, lam, wt = lk._schedule(pr, "grid", N, None, K, rule, min_t, max_t, None)
    want_p = torch.clamp(pr.unmask_prob(torch.from_numpy(ts), torch.from_numpy(ts - np.concatenate((ts[1:], [0.0]))), rule), 0, 1).numpy()
    closing = rule != "ancestral"
    assert t64.shape[0] == K + closing and (last == 0.0) == (not closing)
    np.testing.assert_allclose(wt[:K, 0].numpy(), want_p, rtol=0, atol=0)
    np.testing.assert_allclose(t64[:K, 0].numpy(), ts, rtol=0, atol=0)
    np.testing.assert_allclose(lam[:K, 0].numpy(), surv, rtol=1e-14)
    times = np.concatenate((ts, [min_t])) if closing else ts
    wts, rates = (np.concatenate((p, [1.0])), np.concatenate((surv, [last]))) if closing else (p, surv)
    if closing:
        assert float(wt[K, 0]) == 1.0 and float(t64[K, 0]) == min_t and abs(float(lam[K, 0]) - last) < 1e-14
    else:
        a = pr.alpha(torch.from_numpy(np.concatenate((ts, [0.0])))).numpy()
        np.testing.assert_allclose(surv, (1 - a[:-1]) / (1 - a[0]), rtol=1e-12)                   # the survival telescopes
    pi = wts * rates
    ce = nc.time_only_ce(S, m, D, x0[0], times)
    want = float((pi[:, None] * ce).sum())
    sigma = math.sqrt(float(((wts ** 2 * rates * (1 - rates))[:, None] * ce ** 2).sum()))
    res = lk.absorbing_nll_bound(model, x0, spacing="grid", num_steps=K, rule=rule, min_t=min_t, max_t=max_t, seed=99)
    mean = float(res.nll.mean())
    print(f"grid {rule}: batch mean {mean:.4f}, E[bound] {want:.4f} (sigma / sqrt(N) {sigma / math.sqrt(N):.4f})")
    assert abs(float(pi.sum()) - 1.0) < 1e-12
    assert abs(mean - want) <= 5 * sigma / math.sqrt(N)
    if not closing:
        exact = float(-np.log((pi[:, None] * np.exp(-ce)).sum(0)).sum())
        print(f"  the sampler's exact -log p {exact:.4f}")
        assert want >= exact


@pytest.mark.parametrize("t_func,rate_const", [("loglinear", 1.0), ("log_sqr", 2.0), ("sqrt_cos", 1.55), ("log", 0.5)])
def test_alpha_inverse(t_func, rate_const):
    pr = nc.proc(5, 4, t_func=t_func, rate_const=rate_const)
    t_lo, t_hi = 0.007, 0.99
    a_lo, a_hi = (float(v) for v in pr.alpha(torch.tensor([t_hi, t_lo], dtype=torch.float64)))
    u = a_lo + (a_hi - a_lo) * torch.cat((torch.rand(500, dtype=torch.float64, generator=torch.Generator().manual_seed(2)),
                                          torch.tensor([0.0, 1.0], dtype=torch.float64)))
    t = lk.alpha_inverse(pr, u, t_lo, t_hi)
    err = float((pr.alpha(t) - u).abs().max())
    print(f"{t_func}: max |a(t(u)) - u| = {err:.2e}")
    assert t.dtype == torch.float64 and bool((t >= t_lo).all()) and bool((t <= t_hi).all())
    assert err <= 1e-12
    # the strata of "alpha": u ascending from a(t_max) means t descending from t_max, one time per stratum
    times, lam, wt = lk._schedule(pr, "alpha", 3, 8, None, "ancestral", t_lo, t_hi, torch.Generator().manual_seed(0))
    assert tuple(times.shape) == (9, 3) and bool((times[1:8] < times[:7]).all()) and bool((times[8] == t_lo).all())
    R = a_hi - a_lo
    np.testing.assert_allclose((lam[:8] * wt[:8]).numpy(), R / (1 - a_lo), rtol=1e-13)          # E[y | u] is flat in u
    assert bool((wt[8] == 1).all()) and abs(float(lam[8, 0]) - (1 - a_hi) / (1 - a_lo)) < 1e-15


# ------------------------------------------------------------------------------------------------ the torch statement of the terms
@pytest.mark.parametrize("mode", ac.MODES)
@pytest.mark.parametrize("case", ac.CASES[:5], ids=ac.IDS[:5])
def test_torch_terms_against_the_fp64_cases(case, mode):
    S, m, B, D = case
    logits, x0, w = ac.inputs(case)
    ref = nc.nll_refs(case, mode, True)
    val, masked, hit = lk._terms_torch(logits, x0, ac.x_t_of(case, mode), m, w)
    np.testing.assert_allclose(val.numpy(), ref["out64"].numpy(), rtol=1e-12, atol=1e-12)
    assert torch.equal(masked, ref["term"].sum(1)) and torch.equal(hit, ref["hit"].sum(1))
    if mode == "none":
        assert bool((val == 0).all())


# ------------------------------------------------------------------------------------------------ held entries, refusals
def test_held_entries():
    S, m, N, D = 6, 5, 8, 30
    model = nc.DimOnlyModel(S, m, D, "cpu")
    x0 = nc.data(S, m, N, D, same=False)
    kw = dict(spacing="alpha", n_times=4, min_t=0.01, max_t=1.0, seed=3)
    g = torch.Generator().manual_seed(3)
    one = torch.rand(D, generator=g) < 0.4
    res = lk.absorbing_nll_bound(model, x0, held=one, **kw)
    assert bool((res.n_free == int((~one).sum())).all()) and bool((res.nll > 0).all())
    each = torch.rand(N, D, generator=g) < 0.4
    each[0] = True
    res = lk.absorbing_nll_bound(model, x0, held=each, **kw)
    assert torch.equal(res.n_free, (~each).sum(1)) and float(res.nll[0]) == 0.0 and bool((res.nll[1:] > 0).all())
    # a term of a draw is a sum over free entries only: with every c_d known, no draw can exceed its weight times their sum
    c = torch.stack([model.cross_entropies(x0[n]) for n in range(N)])
    _, _, wt = lk._schedule(model.process, "alpha", N, 4, None, "ancestral", 0.01, 1.0, torch.Generator().manual_seed(3))
    assert bool((res.terms <= wt.float().double() * (c * ~each).sum(1) * (1 + 1e-12)).all())
    res = lk.absorbing_nll_bound(model, x0, held=torch.ones(D, dtype=torch.bool), **kw)
    assert bool((res.nll == 0).all()) and bool((res.n_free == 0).all()) and bool((res.bits_per_dim == 0).all())
    assert tuple(res.terms.shape) == (5, N) and math.isnan(res.accuracy)
    bad = x0.clone()
    bad[0, 0] = m
    with pytest.raises(ValueError, match="held entry is the mask state"):
        lk.absorbing_nll_bound(model, bad, held=torch.ones(D, dtype=torch.bool), **kw)


def test_refuses_other_processes():
    other = types.SimpleNamespace(process=process.DeviceForwardProcess("uniform", 4, "cpu", rate_const=1.0), device="cpu")
    with pytest.raises(ValueError, match="absorbing"):
        lk.absorbing_nll_bound(other, torch.zeros(2, 3, dtype=torch.long), min_t=0.01, max_t=1.0)
    with pytest.raises(ValueError, match="absorbing"):
        lk.absorbing_nll_bound(types.SimpleNamespace(device="cpu"), torch.zeros(2, 3, dtype=torch.long), min_t=0.01, max_t=1.0)


def test_argument_errors():
    S, m, D = 6, 5, 4
    model = nc.DimOnlyModel(S, m, D, "cpu")
    x0 = torch.zeros(2, D, dtype=torch.long)
    ok = dict(min_t=0.01, max_t=1.0)
    for kw, match in ((dict(ok, spacing="uniform"), "spacing"), (dict(ok, spacing="grid"), "num_steps"), (dict(ok, rule="midpoint"), "rule"),
                      (dict(ok, n_times=1), "n_times"), (dict(ok, spacing="grid", num_steps=0), "num_steps"),
                      (dict(min_t=0.5, max_t=0.5), "min_t"), (dict(min_t=0.0, max_t=1.0), "min_t"),
                      (dict(ok, held=torch.ones(D + 1, dtype=torch.bool)), "held"), (dict(ok, held=torch.ones(D)), "held")):
        with pytest.raises(ValueError, match=match):
            lk.absorbing_nll_bound(model, x0, **kw)
    for bad in (x0.float(), x0[0], x0 + S, x0 - 1, torch.full_like(x0, m)):
        with pytest.raises(ValueError, match="x0"):
            lk.absorbing_nll_bound(model, bad, **ok)
    with pytest.raises(TypeError):
        lk.absorbing_nll_bound(model, x0)                               # min_t and max_t have no default


def test_eval_likelihood_reads_the_config_and_sums_over_batches():
    from ctdd.config_dict import ConfigDict
    S, m, D = 6, 5, 12
    model = nc.DimOnlyModel(S, m, D, "cpu")
    cfg = ConfigDict()
    for sec in ("sampler", "training", "loss"):
        cfg[sec] = ConfigDict()
    cfg.training.max_t = 1.0
    cfg.sampler.update(name="AbsorbingLeap", rule="ancestral", num_steps=6, min_t=0.01)
    x = nc.data(S, m, 10, D, same=False)
    out = lk.eval_likelihood(cfg, model, [x[:6].view(6, 1, 3, 4), (x[6:], None), x[:6]], max_batches=2)
    assert set(out) == {"bits_per_dim", "nats_per_dim", "perplexity", "stderr", "accuracy", "n"} and out["n"] == 10
    parts = [lk.absorbing_nll_bound(model, x[:6], n_times=16, min_t=0.01, max_t=1.0, seed=0),
             lk.absorbing_nll_bound(model, x[6:], n_times=16, min_t=0.01, max_t=1.0, seed=1)]
    nats = float(sum(p.nll.sum() for p in parts)) / (10 * D)
    assert abs(out["nats_per_dim"] - nats) < 1e-12 and abs(out["bits_per_dim"] - nats / math.log(2.0)) < 1e-12
    assert abs(out["perplexity"] - math.exp(nats)) < 1e-9 and out["stderr"] > 0 and 0 <= out["accuracy"] <= 1
    cfg["eval"] = ConfigDict()
    cfg.eval.update(spacing="grid", seed=7)
    grid = lk.eval_likelihood(cfg, model, [x])
    want = lk.absorbing_nll_bound(model, x, spacing="grid", num_steps=6, min_t=0.01, max_t=1.0, seed=7)
    assert abs(grid["nats_per_dim"] - float(want.nll.sum()) / (10 * D)) < 1e-12
    with pytest.raises(ValueError, match="no batch"):
        lk.eval_likelihood(cfg, model, [])


def test_native_absorb_nll_refuses_cpu_tensors():
    logits, x = torch.zeros(2, 3, 4), torch.zeros(2, 3, dtype=torch.int32)
    before = native.LAUNCH_COUNTS.get("ctdd_absorb_nll", 0)
    with pytest.raises(native.CtddError):
        native.absorb_nll(logits, x, x, 3)
    with pytest.raises(native.CtddError):
        native.absorb_nll(logits, x, x, 3, w=torch.ones(2), out=torch.zeros(2, dtype=torch.float64))
    assert native.LAUNCH_COUNTS.get("ctdd_absorb_nll", 0) == before
    assert "ctdd_absorb_nll" in native.EXPORTS
