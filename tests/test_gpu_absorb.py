"""GPU: absorbing-state ("masked") diffusion on the kernels of csrc/absorb.hip -- K1 tables of the absorbing kind against the
closed form, ctdd_absorb_noise and ctdd_absorb_step against the CPU replay of their Philox draws, ctdd_absorb_elbo_loss against
fp64 (bar: 8 times the error of an fp32 CPU evaluation, floor 1e-6), the AbsorbingLeap sampler's statistics and inpainting, and one
Standard.step of config_bert_synthetic_absorb on the HIP training kernels against the module."""
import importlib

import numpy as np
import pytest
import torch

import absorb_cases as ac
from ctdd import native, process
from oracle.toy_model import toy_logits

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _proc(S, m, **kw):
    p = dict(rate_const=1.0, t_func="loglinear", alpha_eps=1e-3, mask_state=m)
    p.update(kw)
    return process.DeviceForwardProcess("absorbing", S, DEV, **p)


# ------------------------------------------------------------------------------------------------ tables
@pytest.mark.parametrize("S,m,t_func,rc", [(3, 0, "loglinear", 1.0), (65, 17, "sqrt_cos", 1.55), (256, 255, "log_sqr", 2.0)])
def test_k1_tables_match_the_closed_form(S, m, t_func, rc):
    pr = _proc(S, m, t_func=t_func, rate_const=rc)
    t = torch.tensor([0.05, 0.5, 0.97])
    q = pr.transition(t).cpu().numpy()
    alpha = pr.alpha(t.double()).numpy()
    for i in range(3):
        want = ac.closed_form_qt(S, m, alpha[i])
        err = np.abs(q[i] - want).max()
        print(f"S={S} t={float(t[i])}: max |q - closed form| = {err:.2e}")
        assert err <= 1e-6
    rate = pr.rate(t).cpu().numpy()
    np.testing.assert_allclose(rate, pr.beta(t).numpy()[:, None, None] * process.absorbing_rate_matrix(S, rc, m)[None], rtol=1e-6)
    between = pr.transit_between(t[:1], t[1:2]).cpu().numpy()[0]
    np.testing.assert_allclose(between, ac.closed_form_qt(S, m, alpha[1] / alpha[0]), atol=1e-6)


# ------------------------------------------------------------------------------------------------ noising
def test_noise_matches_the_philox_replay():
    B, D, m, seed, offset = 5, 4099, 7, 0x1234567890AB, 3               # (B D is no multiple of 4: the last Philox block is partial)
    g = torch.Generator().manual_seed(5)
    x0 = torch.randint(0, 7, (B, D), generator=g, dtype=torch.int32)
    alpha = torch.tensor([0.05, 0.3, 0.5, 0.9, 0.999])
    x_t = native.absorb_noise(x0.to(DEV), alpha.to(DEV), m, seed=seed, offset=offset).cpu().numpy()
    want, near, _ = ac.noise_replay(x0.numpy(), alpha.numpy(), m, seed, offset)
    print(f"noise: {near.mean():.2e} of the entries within 1e-6 of alpha")
    assert near.mean() < 1e-3
    assert (x_t[~near] == want[~near]).all()
    masked = x_t == m
    assert (x_t[~masked] == x0.numpy()[~masked]).all()
    for b in range(B):
        a = float(alpha[b])
        share, sigma = masked[b].mean(), np.sqrt(a * (1 - a) / D)
        print(f"noise: sample {b} masked share {share:.4f}, expected {1 - a:.4f} (sigma {sigma:.4f})")
        assert abs(share - (1 - a)) <= 5 * sigma


# ------------------------------------------------------------------------------------------------ the objective
@pytest.mark.parametrize("mode", ac.MODES)
@pytest.mark.parametrize("case", ac.CASES, ids=ac.IDS)
def test_loss_and_gradient_against_fp64(case, mode):
    """Value and max-abs gradient error against fp64 within 8 times the error of the fp32 CPU evaluation (floor 1e-6 absolute).
    Measured on an MI355X: see DESIGN.md section 4."""
    S, m, B, D = case
    logits, x0, w = ac.inputs(case)
    x_t, nll_scale = ac.x_t_of(case, mode), ac.nll_scale_of(case, mode)
    (v64, g64), (v32, g32) = ac.loss_refs(case, mode)
    before = native.LAUNCH_COUNTS.get("ctdd_absorb_elbo_loss", 0)
    val, grad = native.absorb_elbo_loss(logits.to(DEV), x0.to(torch.int32).to(DEV), x_t.to(torch.int32).to(DEV), w.to(DEV), nll_scale, m)
    assert native.LAUNCH_COUNTS["ctdd_absorb_elbo_loss"] == before + 1
    val, grad = float(val.cpu()), grad.cpu()
    ev, eg = abs(val - float(v64)), float((grad.double() - g64).abs().max())
    rv, rg = abs(float(v32) - float(v64)), float((g32.double() - g64).abs().max())
    print(f"S={S} {mode}: value {float(v64):.6e}; error kernel {ev:.2e} / fp32 {rv:.2e}; gradient error kernel {eg:.2e} / fp32 {rg:.2e}")
    assert np.isfinite(val) and bool(torch.isfinite(grad).all())
    carries = ac.term_rows(case, mode)
    assert bool((grad[~carries] == 0).all()), "a row without a term has a non-zero gradient"
    assert bool((grad[..., m] == 0).all()), "the mask state's column has a non-zero gradient"
    assert ev <= max(8 * rv, 1e-6)
    assert eg <= max(8 * rg, 1e-6)
    val_only, none = native.absorb_elbo_loss(logits.to(DEV), x0.to(torch.int32).to(DEV), x_t.to(torch.int32).to(DEV), w.to(DEV), nll_scale, m,
                                             want_grad=False)
    assert none is None and float(val_only.cpu()) == val, "the value depends on whether the gradient is written"


# ------------------------------------------------------------------------------------------------ the step
@pytest.mark.parametrize("mode", ac.MODES)
@pytest.mark.parametrize("case", ac.CASES, ids=ac.IDS)
def test_step_matches_the_replay(case, mode):
    S, m, B, D = case
    logits, _, _ = ac.inputs(case)
    x = ac.x_t_of(case, mode).to(torch.int32)
    xf = x.numpy().reshape(-1)
    was_masked = xf == m
    lg, xd = logits.to(DEV), x.to(DEV)
    seed = 0xABCDEF12345 + S
    compared = left_out = 0
    for offset, p in enumerate((0.0, 0.3, 1.0)):
        changed = torch.zeros(1, dtype=torch.int32, device=DEV)
        out = native.absorb_step(lg, xd, m, p, 0, seed, offset, changed=changed).cpu().numpy().reshape(-1)
        unmask, near, pick, margin = ac.step_replay(logits.numpy(), xf, m, p, seed, offset)
        assert (out[~was_masked] == xf[~was_masked]).all(), "an unmasked row moved"
        left = was_masked & (out != m)
        assert int(changed.cpu()) == int(left.sum())
        sure = was_masked & ~near
        assert (left[sure] == unmask[sure]).all(), "unmask decision differs from the replay"
        if p == 0.0:
            assert not left.any()
        if p == 1.0:
            assert left[was_masked].all()
        assert ((out >= 0) & (out < S)).all()
        moved = left & unmask
        decided = moved & (margin >= 1e-5)
        compared += int(moved.sum())
        left_out += int((moved & ~decided).sum())
        assert (out[decided] == pick[decided]).all(), "picked state differs from categorical_icdf"
    print(f"S={S} {mode}: {left_out} of {compared} picks left out (margin < 1e-5); their share is test_step_share_left_out's")
    changed = torch.zeros(1, dtype=torch.int32, device=DEV)
    out = native.absorb_step(lg, xd, m, 0.0, native.ABSORB_ARGMAX, seed, 9, changed=changed).cpu().numpy().reshape(-1)
    best, gap = ac.argmax_f64(logits.numpy(), m)
    assert (out[~was_masked] == xf[~was_masked]).all()
    assert (out != m)[was_masked].all() and int(changed.cpu()) == int(was_masked.sum())
    clear = was_masked & (gap >= 1e-3)
    assert (out[clear] == best[clear]).all(), "argmax mode differs from the fp64 argmax"


@pytest.mark.parametrize("case", ac.CASES, ids=ac.IDS)
def test_step_share_left_out(case):
    """The share of picks whose margin is below 1e-5 (left out of the comparison): at most 2 % for S <= 257, 5 % for S = 1024.  A
    share needs a sample: every row masked, p = 1, as many launches (offsets = fresh draws on the case's logits) as give 1000 picks
    -- with the few dozen picks of one launch a single left-out pick is already above 2 %.  Every other pick is compared."""
    S, m, B, D = case
    logits, _, _ = ac.inputs(case)
    x = torch.full((B, D), m, dtype=torch.int32)
    lg, xd, seed = logits.to(DEV), x.to(DEV), 0x5EED0000 + S
    compared = left_out = 0
    for offset in range(-(-1000 // (B * D))):
        out = native.absorb_step(lg, xd, m, 1.0, 0, seed, offset).cpu().numpy().reshape(-1)
        _, _, pick, margin = ac.step_replay(logits.numpy(), x.numpy().reshape(-1), m, 1.0, seed, offset)
        decided = margin >= 1e-5
        assert (out != m).all() and (out[decided] == pick[decided]).all()
        compared += out.size
        left_out += int((~decided).sum())
    print(f"S={S}: {left_out} of {compared} picks left out (margin < 1e-5)")
    assert left_out / compared <= (0.05 if S == 1024 else 0.02)


def test_step_argument_errors():
    lg, x = torch.zeros(2, 3, 4, device=DEV), torch.zeros(2, 3, dtype=torch.int32, device=DEV)
    with pytest.raises(native.CtddError):
        native.absorb_step(lg, x, 4, 0.5)                                  # mask_state outside [0, S)
    with pytest.raises(native.CtddError):
        native.absorb_step(lg, x, 3, 0.5, flags=2)
    with pytest.raises(native.CtddError):
        native.absorb_step(lg, x[:, :2].contiguous(), 3, 0.5)
    with pytest.raises(native.CtddError):
        native.absorb_elbo_loss(lg, x, x, torch.ones(3, device=DEV), 0.0, 3)


# ------------------------------------------------------------------------------------------------ the sampler
class _TimeOnlyModel:
    """Logits that depend on the time (and the dimension) only: toy_logits at x = 0."""

    def __init__(self, S, m):
        self.S, self.device, self.process = S, DEV, _proc(S, m)

    def __call__(self, x, t):
        return toy_logits(torch.zeros_like(x), t, self.S, scale=3.0)


def _sampler_cfg(S, D, rule, num_steps=10):
    from ctdd.config_dict import ConfigDict
    cfg = ConfigDict()
    for sec in ("data", "model", "sampler", "training", "loss"):
        cfg[sec] = ConfigDict()
    cfg.data.S, cfg.model.concat_dim, cfg.training.max_t = S, D, 1.0
    cfg.sampler.update(name="AbsorbingLeap", rule=rule, num_steps=num_steps, min_t=0.01)
    return cfg


def test_ancestral_sampler_statistics():
    import lib.sampling.sampling  # noqa: F401
    import lib.sampling.sampling_utils as su
    S, m, N, D, K = 6, 2, 100, 30, 10
    model = _TimeOnlyModel(S, m)
    sampler = su.get_sampler(_sampler_cfg(S, D, "ancestral", K))
    sampler.seed = 20240607
    before = native.LAUNCH_COUNTS.get("ctdd_absorb_step", 0)
    x, changed = sampler.sample(model, N)
    assert native.LAUNCH_COUNTS["ctdd_absorb_step"] == before + K + 1
    assert x.shape == (N, D) and len(changed) == K and (x != m).all() and ((x >= 0) & (x < S)).all()
    ts = np.concatenate((np.linspace(1.0, 0.01, K), [0.0]))
    a = model.process.alpha(torch.from_numpy(ts)).numpy()
    share = 1.0 - np.cumsum(np.asarray(changed) * N) / (N * D)
    for k in (0, 4, 8):
        want = (1 - a[k + 1]) / (1 - a[0])
        sigma = np.sqrt(want * (1 - want) / (N * D))
        print(f"ancestral: masked share after step {k}: {share[k]:.4f}, expected {want:.4f} (sigma {sigma:.4f})")
        assert abs(share[k] - want) <= 5 * sigma
    assert abs(share[-1]) < 1e-12                                        # the last step ends at t = 0: everything is unmasked
    # a row unmasks at step k with probability pi_k and then draws from the softmax at t_k over s != m
    surv = np.concatenate(([1.0], (1 - a[1:]) / (1 - a[0])))
    pi = surv[:-1] - surv[1:]
    t32 = torch.from_numpy(ts[:-1]).float()
    probs = np.zeros((D, S))
    for k in range(K):
        l = toy_logits(torch.zeros(1, D), t32[k:k + 1], S, scale=3.0)[0].double()
        l[:, m] = -np.inf
        probs += pi[k] * torch.softmax(l, -1).numpy()
    want = probs.mean(0)
    freq = np.bincount(x.reshape(-1), minlength=S) / (N * D)
    for s in range(S):
        sigma = np.sqrt(max(want[s] * (1 - want[s]), 1e-12) / (N * D))
        print(f"ancestral: state {s} frequency {freq[s]:.4f}, expected {want[s]:.4f} (sigma {sigma:.4f})")
        assert abs(freq[s] - want[s]) <= 5 * sigma
    again, _ = sampler.sample(model, N)
    assert (again == x).all(), "a fixed seed does not fix the sample"


@pytest.mark.parametrize("rule", ["euler", "tauleap"])
def test_other_rules_finish_without_a_mask_state(rule):
    import lib.sampling.sampling  # noqa: F401
    import lib.sampling.sampling_utils as su
    S, m, N, D = 6, 5, 100, 30
    model = _TimeOnlyModel(S, m)
    sampler = su.get_sampler(_sampler_cfg(S, D, rule, 6))
    sampler.seed = 7
    x, changed = sampler.sample(model, N)
    assert x.shape == (N, D) and (x != m).all() and ((x >= 0) & (x < S)).all() and len(changed) == 6
    assert 0 < sum(changed) <= D


def test_inpaint_keeps_held_entries():
    import lib.sampling.sampling  # noqa: F401
    import lib.sampling.sampling_utils as su
    S, m, N, D = 6, 5, 16, 30
    model = _TimeOnlyModel(S, m)
    sampler = su.get_sampler(_sampler_cfg(S, D, "ancestral", 5))
    sampler.seed = 11
    g = torch.Generator().manual_seed(3)
    x_known = torch.randint(0, S - 1, (N, D), generator=g)
    mask = torch.rand(N, D, generator=g) < 0.4
    out = sampler.inpaint(model, x_known, mask)
    assert out.shape == (N, D) and (out[mask.numpy()] == x_known.numpy()[mask.numpy()]).all()
    assert (out != m).all() and ((out >= 0) & (out < S)).all()
    before = native.LAUNCH_COUNTS.get("ctdd_absorb_step", 0)
    same = sampler.inpaint(model, x_known, torch.ones(D, dtype=torch.bool))
    assert (same == x_known.numpy()).all() and native.LAUNCH_COUNTS.get("ctdd_absorb_step", 0) == before
    bad = x_known.clone()
    bad[0, 0] = m
    with pytest.raises(ValueError, match="mask state"):
        sampler.inpaint(model, bad, torch.ones(D, dtype=torch.bool))


# ------------------------------------------------------------------------------------------------ training
def test_standard_step_on_the_hip_training_kernels_matches_the_module():
    """One Standard.step of config_bert_synthetic_absorb, batch 8, dropout 0, fp32 training precision: loss value and every
    parameter gradient of engine_train = "hip-encoder" against "torch" under the same seeds, with the bars of
    tests/test_gpu_bert_train.py's CT-ELBO step (1e-4 of the value, 2e-3 of each gradient's range)."""
    from test_gpu_bert_train import _registries
    from test_gpu_hollow_train import _compare
    mu, lu, tu, ou = _registries()
    res = {}
    for engine_train in ("torch", "hip-encoder"):
        cfg = importlib.import_module("config.synthetic_config.config_bert_synthetic_absorb").get_config()
        cfg.device = "cuda"
        cfg.model.update(dropout_rate=0.0, attention_dropout_rate=0.0, engine_train=engine_train, engine_train_precision="fp32")
        torch.manual_seed(0)
        model = mu.create_model(cfg, torch.device("cuda"))
        state = {"model": model, "optimizer": ou.get_optimizer(model.parameters(), cfg), "n_iter": 0}
        loss_fn, step = lu.get_loss(cfg), tu.get_train_step(cfg)
        x = torch.randint(0, cfg.data.S - 1, (8, int(cfg.model.concat_dim)), device="cuda")
        counts = {k: native.LAUNCH_COUNTS.get(k, 0) for k in ("ctdd_absorb_noise", "ctdd_absorb_elbo_loss")}
        torch.manual_seed(11)
        l = step.step(state, loss_fn, x)
        assert all(native.LAUNCH_COUNTS.get(k, 0) == v + 1 for k, v in counts.items()), "the objective did not run on the HIP kernels"
        assert bool(torch.isfinite(l)) and float(l) != 1e9
        res[engine_train] = (float(l), {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None})
        assert (model._trainer is not None) == (engine_train == "hip-encoder")
    err = abs(res["hip-encoder"][0] - res["torch"][0])
    print(f"AbsorbingElbo loss: torch {res['torch'][0]:.6e}, hip-encoder {res['hip-encoder'][0]:.6e}")
    assert err < 1e-4 * max(1.0, abs(res["torch"][0]))
    print(f"AbsorbingElbo gradients: worst error {_compare(res['hip-encoder'][1], res['torch'][1], 2e-3):.3e} of the range (bar 2e-3)")
