"""GPU: ctdd_absorb_nll (csrc/absorb.hip) against fp64 on the cases of absorb_cases.py -- bar: 8 times the error of an fp32 CPU
evaluation, floor 1e-6 relative -- its accumulation, determinism and refusals, and the held-out likelihood bounds of lib/likelihood.py
against their closed forms: models whose logits ignore x_t (exact mean and variance of both estimators), the sampler's own bound, the
fused path against the torch path, held entries, and one batch of config_bert_synthetic_absorb through eval_likelihood."""
import importlib
import math

import numpy as np
import pytest
import torch

import absorb_cases as ac
import absorb_nll_cases as nc
from ctdd import native
from oracle.toy_model import toy_logits

pytestmark = pytest.mark.gpu

DEV = "cuda"
COUNTERS = ("ctdd_absorb_nll", "ctdd_absorb_noise")


def _i32(t):
    return t.to(torch.int32).to(DEV).contiguous()


# ------------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("weighted", [True, False], ids=["w", "w-none"])
@pytest.mark.parametrize("mode", ac.MODES)
@pytest.mark.parametrize("case", ac.CASES, ids=ac.IDS)
def test_nll_against_fp64(case, mode, weighted):
    """Per-row and per-sample values within max(8 E32, 1e-6 max(1, |value|)) of fp64, E32 the largest error of the same formula in
    fp32 torch on the CPU over the call; counters exact; rows without a term exact zeros and unread (NaN poison).  Measured on an
    MI355X: see DESIGN.md section 4f."""
    S, m, B, D = case
    logits, x0, w = ac.inputs(case)
    ref = nc.nll_refs(case, mode, weighted)
    x0d, xtd, wd = _i32(x0), _i32(ac.x_t_of(case, mode)), w.to(DEV) if weighted else None
    masked, hit = (torch.zeros(B, dtype=torch.int32, device=DEV) for _ in range(2))
    before = native.LAUNCH_COUNTS.get("ctdd_absorb_nll", 0)
    row, out = native.absorb_nll(logits.to(DEV), x0d, xtd, m, w=wd, masked=masked, hit=hit)
    assert native.LAUNCH_COUNTS["ctdd_absorb_nll"] == before + 1
    assert row.dtype == torch.float32 and tuple(row.shape) == (B, D) and out.dtype == torch.float64 and tuple(out.shape) == (B,)
    row, out = row.cpu(), out.cpu()
    row_bar, row_e32 = nc.bar(ref["row64"], ref["row32"])
    out_bar, out_e32 = nc.bar(ref["out64"], ref["out32"])
    row_err, out_err = (row.double() - ref["row64"]).abs(), (out - ref["out64"]).abs()
    print(f"S={S} {mode} {'w' if weighted else 'w=None'}: row error kernel {float(row_err.max()):.2e} / fp32 {row_e32:.2e} "
          f"(worst error / bar {float((row_err / row_bar).max()):.3f}); sample error kernel {float(out_err.max()):.2e} / fp32 {out_e32:.2e} "
          f"(worst error / bar {float((out_err / out_bar).max()):.3f}); largest sample value {float(ref['out64'].abs().max()):.4e}")
    assert bool(torch.isfinite(row).all()) and bool(torch.isfinite(out).all())
    assert bool((row_err <= row_bar).all())
    assert bool((out_err <= out_bar).all())
    assert bool((row[~ref["term"]] == 0).all()) and not bool(torch.signbit(row[~ref["term"]]).any()), "a row without a term is not +0.0"
    assert torch.equal(masked.cpu().long(), ref["term"].sum(1)), "out_masked"
    assert torch.equal(hit.cpu().long(), ref["hit"].sum(1)), "out_hit differs from the fp64 argmax"
    if mode == "none":
        assert bool((out == 0).all())
    # rows without a term are not read: NaN in their logits changes nothing, bit for bit
    poison = logits.clone()
    poison[~ref["term"]] = float("nan")
    row_p, out_p = native.absorb_nll(poison.to(DEV), x0d, xtd, m, w=wd)
    assert native.LAUNCH_COUNTS["ctdd_absorb_nll"] == before + 2
    assert torch.equal(row_p.cpu(), row) and torch.equal(out_p.cpu(), out)


def test_accumulation_and_determinism():
    case = ac.CASES[5]
    S, m, B, D = case
    logits, x0, w = ac.inputs(case)
    lg, x0d, wd = logits.to(DEV), _i32(x0), w.to(DEV)
    mix, every = _i32(ac.x_t_of(case, "mix")), _i32(ac.x_t_of(case, "all"))
    _, a = native.absorb_nll(lg, x0d, mix, m, w=wd)
    _, b = native.absorb_nll(lg, x0d, every, m, w=wd)
    buf = torch.zeros((3, B), dtype=torch.float64, device=DEV)             # a row of a (K, N) buffer
    masked, hit = (torch.zeros(B, dtype=torch.int32, device=DEV) for _ in range(2))
    for xt in (mix, every):
        _, got = native.absorb_nll(lg, x0d, xt, m, w=wd, out=buf[1], masked=masked, hit=hit)
        assert got.data_ptr() == buf[1].data_ptr()
    assert torch.equal(buf[1], a + b) and bool((buf[0] == 0).all()) and bool((buf[2] == 0).all())
    want = nc.nll_refs(case, "mix", True)["term"].sum(1) + nc.nll_refs(case, "all", True)["term"].sum(1)
    assert torch.equal(masked.cpu().long(), want)
    for _ in range(10):
        row, again = native.absorb_nll(lg, x0d, mix, m, w=wd)
        assert torch.equal(again, a), "repeated calls differ"


def test_one_long_sample():
    """D = 70 001 at S = 3: 35 workgroups of the row pass with eight row groups each, 274 rows a thread in the sum."""
    S, m, D = 3, 1, 70001
    g = torch.Generator().manual_seed(31)
    logits = 3.0 * torch.randn(1, D, S, generator=g)
    x0 = 2 * torch.randint(0, 2, (1, D), generator=g)
    x_t = torch.where(torch.rand(1, D, generator=g) < 0.5, torch.full_like(x0, m), x0)
    row64, term = nc.rows_eval(logits, x0, x_t, m, torch.float64)
    row32, _ = nc.rows_eval(logits, x0, x_t, m, torch.float32)
    masked, hit = (torch.zeros(1, dtype=torch.int32, device=DEV) for _ in range(2))
    row, out = native.absorb_nll(logits.to(DEV), _i32(x0), _i32(x_t), m, masked=masked, hit=hit)
    row, out = row.cpu(), out.cpu()
    out_bar, out_e32 = nc.bar(row64.sum(1), row32.sum(1))
    row_bar, row_e32 = nc.bar(row64, row32)
    err = float((out - row64.sum(1)).abs())
    print(f"D={D}: value {float(row64.sum()):.6e}; sample error kernel {err:.2e} / fp32 {out_e32:.2e} (bar {float(out_bar):.2e}); "
          f"row error kernel {float((row.double() - row64).abs().max()):.2e} / fp32 {row_e32:.2e}")
    assert err <= float(out_bar)
    assert bool(((row.double() - row64).abs() <= row_bar).all())
    assert int(masked.cpu()) == int(term.sum())
    best, _ = ac.argmax_f64(logits.numpy(), m)
    assert int(hit.cpu()) == int((term.view(-1) & (torch.from_numpy(best) == x0.view(-1))).sum())


def test_misuse_raises():
    lg = torch.zeros(2, 3, 4, device=DEV)
    x = torch.zeros(2, 3, dtype=torch.int32, device=DEV)
    ok = dict(logits=lg, x0=x, xt=x, mask_state=3)
    native.absorb_nll(**ok)
    bad = [dict(ok, logits=lg.cpu()), dict(ok, x0=x.cpu()), dict(ok, xt=x[:, :2].contiguous()), dict(ok, x0=x.view(3, 2)),
           dict(ok, logits=lg[0]), dict(ok, x0=x.long()), dict(ok, w=torch.ones(3, device=DEV)), dict(ok, w=torch.ones(2, 1, device=DEV)),
           dict(ok, w=torch.ones(2, dtype=torch.float64, device=DEV)), dict(ok, out=torch.zeros(2, device=DEV)),
           dict(ok, out=torch.zeros(3, dtype=torch.float64, device=DEV)), dict(ok, masked=torch.zeros(2, dtype=torch.int64, device=DEV)),
           dict(ok, hit=torch.zeros(1, dtype=torch.int32, device=DEV)), dict(ok, mask_state=4), dict(ok, mask_state=-1)]
    for kw in bad:
        with pytest.raises(native.CtddError):
            native.absorb_nll(**kw)
    S = native.ABSORB_MAX_S + 1
    with pytest.raises(native.CtddError):
        native.absorb_nll(torch.zeros(1, 2, S, device=DEV), x[:1, :2].contiguous(), x[:1, :2].contiguous(), 0)


# ------------------------------------------------------------------------------------------------ the bounds
@pytest.mark.parametrize("spacing", ["alpha", "grid"])
def test_bounds_are_tight_for_a_network_that_ignores_x_t(spacing):
    """Logits that depend on d only: the exact expectation of either bound is sum_d c_d, and the per-sample variance is exact too
    (alpha: V / K + lam_min (1 - lam_min) sum c_d^2; grid: sum_i p_i^2 surv_i (1 - surv_i) sum c_d^2).  The batch mean within 5 sigma."""
    import lib.likelihood as lk
    S, m, D, N, K, steps, min_t, max_t = 6, 2, 30, 256, 16, 10, 0.01, 1.0
    model = nc.DimOnlyModel(S, m, D, DEV)
    x0 = nc.data(S, m, N, D)
    c = model.cross_entropies(x0[0])
    res = lk.absorbing_nll_bound(model, x0.to(DEV), spacing=spacing, n_times=K, num_steps=steps, min_t=min_t, max_t=max_t, seed=1234)
    if spacing == "alpha":
        sigma = nc.alpha_sigma(model.process, c, K, min_t, max_t)
        assert tuple(res.terms.shape) == (K + 1, N) and tuple(res.stderr.shape) == (N,)
    else:
        _, p, surv, last = nc.grid_of(model.process, steps, min_t, max_t, "ancestral")
        sigma = math.sqrt(float((p ** 2 * surv * (1 - surv)).sum()) * float((c ** 2).sum()))
        assert last == 0.0 and tuple(res.terms.shape) == (steps, N) and res.stderr is None
    mean, want = float(res.nll.mean()), float(c.sum())
    print(f"{spacing}: batch mean {mean:.4f}, exact {want:.4f}, sigma / sqrt(N) {sigma / math.sqrt(N):.4f}; per-sample std "
          f"{float(res.nll.std()):.3f}, exact {sigma:.3f}; accuracy {res.accuracy:.4f}")
    assert abs(mean - want) <= 5 * sigma / math.sqrt(N)
    assert bool((res.n_free == D).all())
    np.testing.assert_allclose(res.bits_per_dim.numpy(), res.nll.numpy() / (D * math.log(2.0)), rtol=1e-14)
    assert res.n_masked > 0 and res.accuracy == res.n_hit / res.n_masked and 0.0 <= res.accuracy <= 1.0


def test_grid_bound_is_the_samplers_bound():
    """Time-only logits, ancestral rule: E[bound] = sum_i pi_i CE_i(x0) with pi_i = surv_i p_i, at least the sampler's exact
    -sum_d log sum_i pi_i p_i(x0_d); the grid's p_i are unmask_prob on the sampler's grid."""
    import lib.likelihood as lk
    S, m, N, D, K, min_t, max_t = 6, 2, 256, 30, 10, 0.01, 1.0
    model = nc.TimeOnlyModel(S, m, DEV)
    pr = nc.proc(S, m)
    x0 = nc.data(S, m, N, D)
    ts, p, surv, last = nc.grid_of(pr, K, min_t, max_t, "ancestral")
    t64, lam, wt = lk._schedule(pr, "grid", N, None, K, "ancestral", min_t, max_t, None)
    a = pr.alpha(torch.from_numpy(np.concatenate((ts, [0.0])))).numpy()
    np.testing.assert_allclose(wt[:, 0].numpy(), p, rtol=0, atol=0)
    np.testing.assert_allclose(p, (a[1:] - a[:-1]) / (1 - a[:-1]), rtol=1e-12)
    np.testing.assert_allclose(lam[:, 0].numpy(), (1 - a[:-1]) / (1 - a[0]), rtol=1e-12)        # the survival telescopes
    np.testing.assert_allclose(t64[:, 0].numpy(), ts, rtol=0, atol=0)
    pi = surv * p
    ce = nc.time_only_ce(S, m, D, x0[0], ts)                                                     # (K, D)
    want = float((pi[:, None] * ce).sum())
    exact = float(-np.log((pi[:, None] * np.exp(-ce)).sum(0)).sum())
    sigma = math.sqrt(float(((p ** 2 * surv * (1 - surv))[:, None] * ce ** 2).sum()))
    res = lk.absorbing_nll_bound(model, x0.to(DEV), spacing="grid", num_steps=K, min_t=min_t, max_t=max_t, seed=99)
    mean = float(res.nll.mean())
    print(f"grid, time-only model: batch mean {mean:.4f}, E[bound] {want:.4f} (sigma / sqrt(N) {sigma / math.sqrt(N):.4f}), "
          f"the sampler's exact -log p {exact:.4f}")
    assert abs(float(pi.sum()) - 1.0) < 1e-12 and last == 0.0
    assert want >= exact
    assert abs(mean - want) <= 5 * sigma / math.sqrt(N)


class _ToyModel:
    """Logits that depend on x_t, t and d."""

    def __init__(self, S, m):
        self.S, self.device, self.process = S, DEV, nc.proc(S, m, DEV)

    def __call__(self, x, t):
        return toy_logits(x, t, self.S, scale=3.0)


@pytest.mark.parametrize("spacing", ["alpha", "grid"])
def test_fused_and_torch_paths_agree(spacing):
    """The same seed gives both paths the same x_t: per-sample bounds within 1e-6 max(1, |value|) (the floor of the kernel's bar:
    the torch path is the fp64 evaluation itself), equal counts."""
    import lib.likelihood as lk
    S, m, N, D = 6, 5, 64, 30
    model = _ToyModel(S, m)
    x0 = nc.data(S, m, N, D, same=False).to(DEV)
    kw = dict(spacing=spacing, n_times=8, num_steps=7, rule="tauleap", min_t=0.01, max_t=1.0, seed=5)
    before = {k: native.LAUNCH_COUNTS.get(k, 0) for k in COUNTERS}
    fused = lk.absorbing_nll_bound(model, x0, **kw)
    n = fused.terms.shape[0]
    assert n == (9 if spacing == "alpha" else 8)                       # tauleap's p stays below 1: the grid's closing draw runs
    assert all(native.LAUNCH_COUNTS[k] == before[k] + n for k in COUNTERS)
    plain = lk.absorbing_nll_bound(model, x0, fused=False, **kw)
    assert native.LAUNCH_COUNTS["ctdd_absorb_nll"] == before["ctdd_absorb_nll"] + n
    err = (fused.nll - plain.nll).abs()
    bar = 1e-6 * torch.clamp(plain.nll.abs(), min=1.0)
    print(f"{spacing}: fused against torch path: largest error {float(err.max()):.2e}, worst error / bar {float((err / bar).max()):.3f}; "
          f"bounds in [{float(plain.nll.min()):.2f}, {float(plain.nll.max()):.2f}]; accuracy {fused.accuracy:.4f}")
    assert bool((err <= bar).all())
    assert (fused.n_masked, fused.n_hit) == (plain.n_masked, plain.n_hit) and fused.accuracy == plain.accuracy
    again = lk.absorbing_nll_bound(model, x0, **kw)
    assert torch.equal(again.terms, fused.terms), "a fixed seed does not fix the bound"


def test_held_entries():
    import lib.likelihood as lk
    S, m, N, D = 6, 5, 16, 30
    model = _ToyModel(S, m)
    x0 = nc.data(S, m, N, D, same=False)
    kw = dict(spacing="grid", num_steps=5, min_t=0.01, max_t=1.0, seed=3)
    g = torch.Generator().manual_seed(3)
    one = torch.rand(D, generator=g) < 0.4
    full = lk.absorbing_nll_bound(model, x0.to(DEV), **kw)
    res = lk.absorbing_nll_bound(model, x0.to(DEV), held=one, **kw)
    assert bool((res.n_free == int((~one).sum())).all()) and bool((full.n_free == D).all())
    assert bool((res.nll > 0).all()) and res.n_masked < full.n_masked
    each = torch.rand(N, D, generator=g) < 0.4
    each[0] = True                                                     # one sample with nothing free
    res = lk.absorbing_nll_bound(model, x0.to(DEV), held=each, **kw)
    assert torch.equal(res.n_free, (~each).sum(1)) and float(res.nll[0]) == 0.0 and float(res.bits_per_dim[0]) == 0.0
    assert bool((res.nll[1:] > 0).all())
    before = {k: native.LAUNCH_COUNTS.get(k, 0) for k in COUNTERS}
    res = lk.absorbing_nll_bound(model, x0.to(DEV), held=torch.ones(D, dtype=torch.bool), **kw)
    assert bool((res.nll == 0).all()) and bool((res.n_free == 0).all()) and tuple(res.terms.shape) == (5, N)
    assert all(native.LAUNCH_COUNTS.get(k, 0) == v for k, v in before.items()), "everything is held, yet a kernel ran"
    bad = x0.clone()
    bad[0, 0] = m
    with pytest.raises(ValueError, match="mask state"):
        lk.absorbing_nll_bound(model, bad.to(DEV), held=torch.ones(D, dtype=torch.bool), **kw)


def test_eval_likelihood_on_a_real_model():
    import lib.likelihood as lk
    import lib.models.models  # noqa: F401
    import lib.models.model_utils as mu
    cfg = importlib.import_module("config.synthetic_config.config_bert_synthetic_absorb").get_config()
    cfg.device = "cuda"
    torch.manual_seed(0)
    model = mu.create_model(cfg, torch.device("cuda"))
    model.eval()
    x = torch.randint(0, cfg.data.S - 1, (8, int(cfg.model.concat_dim)), device="cuda")
    before = native.LAUNCH_COUNTS.get("ctdd_absorb_nll", 0)
    out = lk.eval_likelihood(cfg, model, [x])
    assert native.LAUNCH_COUNTS["ctdd_absorb_nll"] == before + 16 + 1
    print("eval_likelihood, random-init config_bert_synthetic_absorb:", out, "; ln(S - 1) =", math.log(cfg.data.S - 1))
    assert set(out) == {"bits_per_dim", "nats_per_dim", "perplexity", "stderr", "accuracy", "n"}
    assert out["n"] == 8 and all(math.isfinite(float(v)) for v in out.values())
    assert out["nats_per_dim"] > 0 and abs(out["perplexity"] - math.exp(out["nats_per_dim"])) < 1e-9
