"""CPU: the remasking sampler without a GPU -- the AbsorbingRemask registry name, its two shipped configs and option checks, the
refusal of CPU tensors by the two bindings, remask_schedule against exact rationals (recursion, sigma_max, the conservation identity,
the window), and the replay that the GPU tests compare the kernels with against a brute-force loop."""
import importlib
import math
from fractions import Fraction

import numpy as np
import pytest
import torch

import absorb_cases as ac
import absorb_remask_cases as rc
from ctdd import native
from oracle import philox as oph

CONFIGS = (("synthetic_config.config_bert_synthetic_absorb_remask", "synthetic_config.config_bert_synthetic_absorb", 32),
           ("maze_config.config_bert_maze_absorb_remask", "maze_config.config_bert_maze_absorb", 32))


def _registries():
    import lib.models.models  # noqa: F401
    import lib.models.model_utils as mu
    import lib.sampling.sampling  # noqa: F401
    import lib.sampling.sampling_utils as su
    return mu, su


# ------------------------------------------------------------------------------------------------ registry, configs, options
def test_registry_name_resolves():
    _, su = _registries()
    cls = su._SAMPLERS["AbsorbingRemask"]
    assert cls.__name__ == "AbsorbingRemask" and issubclass(cls, su._SAMPLERS["AbsorbingLeap"])
    assert "ctdd_absorb_remask_step" in native.EXPORTS and "ctdd_absorb_remask_norm" in native.EXPORTS


@pytest.mark.parametrize("mod,base,steps", CONFIGS)
def test_shipped_configs_load(mod, base, steps):
    mu, su = _registries()
    cfg = importlib.import_module("config." + mod).get_config()
    s = cfg.sampler
    assert (s.name, s.num_steps, s.remask, s.remask_eta, s.remask_temp) == ("AbsorbingRemask", steps, "cap", 0.02, 1.0)
    want = importlib.import_module("config." + base).get_config()
    assert cfg.to_dict().keys() == want.to_dict().keys()
    for sec in want.to_dict():                                           # everything but the sampler section is the base config's
        if sec != "sampler":
            a, b = cfg[sec], want[sec]
            assert (a.to_dict() if hasattr(a, "to_dict") else a) == (b.to_dict() if hasattr(b, "to_dict") else b), sec
    ours, theirs = s.to_dict(), want.sampler.to_dict()
    changed = {k for k in ours if k not in theirs or ours[k] != theirs[k]}
    assert changed <= {"name", "num_steps", "remask", "remask_eta", "remask_temp"} and set(theirs) <= set(ours)
    sampler = su.get_sampler(cfg)
    assert type(sampler).__name__ == "AbsorbingRemask" and sampler.num_steps == steps and sampler.rule == "ancestral"
    assert (sampler.remask, sampler.remask_eta, sampler.remask_temp) == ("cap", 0.02, 1.0)
    cfg.device = "cpu"
    cfg.model.update(num_layers=1, engine="torch")
    model = mu.create_model(cfg, torch.device("cpu"))
    assert model.process.kind == "absorbing" and model.process.mask_state == cfg.model.mask_state
    _, sigma, p = sampler.schedule(model.process)                        # the shipped schedule is a valid one
    assert len(sigma) == steps and sigma[0] == 0.0 and max(sigma) == 0.02 and all(0.0 <= v <= 1.0 for v in p)


def test_options_defaults_and_refusals():
    _, su = _registries()
    cfg = importlib.import_module("config." + CONFIGS[0][0]).get_config()
    for key in ("remask", "remask_eta", "remask_temp"):
        del cfg.sampler[key]
    sampler = su.get_sampler(cfg)
    assert (sampler.remask, sampler.remask_eta, sampler.remask_temp) == ("cap", 0.02, 1.0)
    assert sampler.remask_window == (float("inf"), float("-inf")) and sampler.remasked == []
    cfg.sampler.update(remask="conf", remask_eta=1.0, remask_temp=0.02, remask_window=(0.8, 0.1))
    sampler = su.get_sampler(cfg)
    assert (sampler.remask, sampler.remask_eta, sampler.remask_temp, sampler.remask_window) == ("conf", 1.0, 0.02, (0.8, 0.1))
    for key, bad, match in (("remask", "loop", "remask"), ("remask_eta", -0.01, "remask_eta"), ("remask_eta", 1.5, "remask_eta"),
                            ("remask_eta", float("nan"), "remask_eta"), ("remask_temp", 0.01, "remask_temp"),
                            ("remask_temp", float("nan"), "remask_temp"), ("remask_window", (0.1, 0.8), "remask_window"),
                            ("remask_window", (0.5,), "remask_window"), ("remask_window", 0.5, "remask_window")):
        c = importlib.import_module("config." + CONFIGS[0][0]).get_config()
        c.sampler[key] = bad
        with pytest.raises(ValueError, match=match):
            su.get_sampler(c)


def test_native_calls_refuse_cpu_tensors():
    logits, x, conf = torch.zeros(2, 3, 4), torch.zeros(2, 3, dtype=torch.int32), torch.ones(2, 3)
    with pytest.raises(native.CtddError):
        native.absorb_remask_step(logits, x, 3, 0.5, 0.1)
    with pytest.raises(native.CtddError):
        native.absorb_remask_step(logits, x, 3, 0.5, 0.1, held=torch.zeros(2, 3, dtype=torch.bool), conf=conf)
    with pytest.raises(native.CtddError):
        native.absorb_remask_norm(x, 3, conf)


# ------------------------------------------------------------------------------------------------ the schedule
def _ancestral(K, eps=1e-3):
    ts = np.concatenate((np.linspace(1.0, 0.01, K), [0.0]))
    a = 1 - (1 - eps) * ts
    return ((a[1:] - a[:-1]) / (1 - a[:-1])).clip(0.0, 1.0).tolist()


P_LISTS = {
    "ancestral10": _ancestral(10),
    "ancestral32": _ancestral(32),
    "euler": [0.0, 0.1, 0.3, 0.05, 0.7, 0.2, 0.9],
    "one_inside": [0.2, 0.5, 1.0, 0.3, 0.4],
    "one_at_the_end": [0.25, 0.125, 0.5, 1.0],
    "one_first": [1.0, 0.5],
    "zeros": [0.0, 0.0, 0.5, 0.0],
}


@pytest.mark.parametrize("strategy,eta", [("cap", 0.02), ("cap", 0.6), ("rescale", 0.5), ("rescale", 1.0), ("conf", 0.3)])
@pytest.mark.parametrize("name", P_LISTS)
def test_schedule_against_exact_rationals(name, strategy, eta):
    from lib.sampling.sampling import remask_schedule
    p = P_LISTS[name]
    sigma, pp = remask_schedule(p, strategy, eta)
    es, ep, surv = rc.exact_schedule(p, strategy, eta)
    assert len(sigma) == len(pp) == len(p) and sigma[0] == 0.0 and pp[0] == p[0]
    for k in range(len(p)):
        assert surv[k + 1] == surv[k] * (1 - Fraction(p[k]))            # the recursion
        if surv[k] < 1:
            smax = min(Fraction(1), surv[k + 1] / (1 - surv[k]))
            assert es[k] == (Fraction(eta) * smax if strategy == "rescale" else min(Fraction(eta), smax)) and es[k] <= smax
        else:
            assert es[k] == 0
        assert surv[k] * (1 - ep[k]) + (1 - surv[k]) * es[k] == surv[k + 1], "the identity does not hold in rationals"
        assert 0 <= ep[k] <= 1
        # the fp64 result: against the rationals, inside [0, 1], and the identity to 1e-14
        assert abs(Fraction(sigma[k]) - es[k]) <= Fraction(1, 10 ** 14) and abs(Fraction(pp[k]) - ep[k]) <= Fraction(1, 10 ** 14)
        assert 0.0 <= sigma[k] <= 1.0 and 0.0 <= pp[k] <= 1.0 and pp[k] >= p[k]
        s, nxt = float(surv[k]), float(surv[k + 1])
        assert abs(s * (1 - pp[k]) + (1 - s) * sigma[k] - nxt) <= 1e-14
    if name.startswith("ancestral") or name == "one_at_the_end":       # a grid that ends with p = 1: the last sigma is 0 by itself
        assert sigma[-1] == 0.0 and pp[-1] == 1.0


def test_schedule_eta_zero_window_and_refusals():
    from lib.sampling.sampling import remask_schedule
    for p in P_LISTS.values():
        for strategy in ("cap", "rescale", "conf"):
            sigma, pp = remask_schedule(p, strategy, 0.0)
            assert sigma == [0.0] * len(p)
            assert np.asarray(pp).tobytes() == np.asarray(p, dtype=np.float64).tobytes(), "eta = 0 does not return p bit for bit"
    p = P_LISTS["ancestral10"]
    active = [False, True, True, False, False, True, False, True, True, True]
    sigma, pp = remask_schedule(p, "cap", 0.05, active)
    full, _ = remask_schedule(p, "cap", 0.05)
    for k in range(10):
        assert sigma[k] == (full[k] if active[k] else 0.0)
        assert active[k] or pp[k] == p[k]
    assert sum(v > 0 for v in sigma) == 5                                # (the last step's sigma is 0 whether active or not)
    es, ep, surv = rc.exact_schedule(p, "cap", 0.05, active)
    assert all(surv[k] * (1 - ep[k]) + (1 - surv[k]) * es[k] == surv[k + 1] for k in range(10))
    for bad in (dict(strategy="loop", eta=0.1), dict(strategy="cap", eta=1.1), dict(strategy="cap", eta=-0.1)):
        with pytest.raises(ValueError):
            remask_schedule(p, bad["strategy"], bad["eta"])
    with pytest.raises(ValueError):
        remask_schedule(p, "cap", 0.1, active[:3])
    with pytest.raises(ValueError):
        remask_schedule([0.5, 1.5], "cap", 0.1)


def test_sampler_window_selects_the_steps():
    _, su = _registries()
    cfg = importlib.import_module("config." + CONFIGS[0][0]).get_config()
    cfg.sampler.update(num_steps=10, min_t=0.01, remask_eta=0.05, remask_window=(0.8, 0.3))
    cfg.training.max_t = 1.0

    class _Process:
        @staticmethod
        def unmask_prob(t, h, rule):
            return torch.as_tensor(_ancestral(10), dtype=torch.float64)
    t64, sigma, _ = su.get_sampler(cfg).schedule(_Process())
    ts = t64[:-1].tolist()
    assert [v > 0 for v in sigma] == [0.3 <= t <= 0.8 for t in ts] and 0 < sum(v > 0 for v in sigma) < 10


# ------------------------------------------------------------------------------------------------ the replay itself
@pytest.mark.parametrize("seed", range(4))
def test_remask_replay_against_brute_force(seed):
    rng = np.random.default_rng(seed)
    N, D, m, temp, sigma = 3, 11, 4, 0.5, 0.2
    x = np.where(rng.random((N, D)) < 0.4, m, rng.integers(0, 4, (N, D))).astype(np.int32)
    held = rng.random((N, D)) < 0.3
    x[1] = m                                                             # a sample with nothing unmasked
    conf = rng.random((N, D)).astype(np.float32)
    U, Z = rc.norm_replay(x, held, conf, m, temp)
    norm = np.stack((U.astype(np.float32), Z.astype(np.float32)), 1)
    for n in range(N):                                                   # the norm, entry by entry
        rows = [d for d in range(D) if x[n, d] != m and not held[n, d]]
        assert U[n] == len(rows)
        assert abs(Z[n] - sum(math.exp(-float(conf[n, d]) / temp) for d in rows)) <= 1e-12
    assert U[1] == 0 and Z[1] == 0.0
    key, offset = 0x1234ABCD + seed, 5
    flat, fixed = rc.remask_replay(x, held, m, sigma, key, offset), rc.remask_replay(x, None, m, sigma, key, offset)
    weighted = rc.remask_replay(x, held, m, sigma, key, offset, conf=conf, norm=norm, temp=temp)
    for r in range(N * D):
        n, d = divmod(r, D)
        u3 = oph.row_uniforms(np.array([r]), offset, key, 1)[0, 3]      # component 3 of the row's own block
        assert u3 == flat[2][r] == weighted[2][r]
        free = x[n, d] != m and not held[n, d]
        assert bool(flat[3][r]) == free and bool(fixed[3][r]) == (x[n, d] != m)
        assert bool(flat[0][r]) == (free and u3 < np.float32(sigma))
        assert bool(fixed[0][r]) == (x[n, d] != m and u3 < np.float32(sigma))
        want = min(1.0, sigma * U[n] * math.exp(-float(conf[n, d]) / temp) / Z[n]) if Z[n] > 0 else 0.0
        assert abs(float(weighted[1][r]) - want) <= 1e-6
        if abs(float(u3) - want) > 1e-5:
            assert bool(weighted[0][r]) == (free and u3 < want)
    # sigma 0 / 1: nobody / every free unmasked row
    assert not rc.remask_replay(x, held, m, 0.0, key, offset)[0].any()
    every = rc.remask_replay(x, held, m, 1.0, key, offset)
    assert (every[0] == every[3]).all()
    # the mean of sigma_row over a sample's free unmasked rows is sigma when nothing clamps
    sg = weighted[1].reshape(N, D)
    free = weighted[3].reshape(N, D)
    for n in (0, 2):
        assert U[n] > 0 and abs(float(sg[n][free[n]].astype(np.float64).mean()) - sigma) <= 1e-6


@pytest.mark.parametrize("mode", ac.MODES)
@pytest.mark.parametrize("case", ac.CASES, ids=ac.IDS)
def test_step_seeds_leave_no_coin_near_its_threshold(case, mode):
    """The keys and offsets of tests/test_gpu_absorb_remask.py: at most 1 % of a call's free unmasked rows (here: none) have their
    remask coin within 1e-6 of sigma, or within 1e-5 of the confidence-weighted sigma_row (with the norm restated in fp64 on the CPU;
    the kernel's differs from it by fp32 rounding, far below the band)."""
    S, m, B, D = case
    x = ac.x_t_of(case, mode).numpy()
    held, conf = rc.held_pattern(case), rc.conf_pattern(case)
    for offset in range(len(rc.P_VALUES)):
        _, sg, u3, free = rc.remask_replay(x, held, m, rc.SIGMA, rc.step_seed(S), offset)
        near = free & (np.abs(u3.astype(np.float64) - sg) < 1e-6)
        assert near.sum() <= 0.01 * free.sum()
    U, Z = rc.norm_replay(x, held, conf, m, 1.0)
    norm = np.stack((U.astype(np.float32), Z.astype(np.float32)), 1)
    for offset, sigma in enumerate((rc.SIGMA_CONF, 1.0)):
        _, sg, u3, free = rc.remask_replay(x, held, m, sigma, rc.step_seed(S), 10 + offset, conf=conf, norm=norm, temp=1.0)
        near = free & (np.abs(u3.astype(np.float64) - sg) < 1e-5)
        assert near.sum() <= 0.01 * free.sum()


def test_held_pattern_and_state_probability():
    for case in ac.CASES:
        S, m, B, D = case
        held = rc.held_pattern(case).reshape(-1)
        rpb = rc.rows_per_workgroup(S)
        tail = held[((B * D - 1) // rpb) * rpb:]
        assert tail[0] and tail[-1] and not held.all()
        if B * D >= 30:
            assert 0.15 < held.mean() < 0.55
    logits, _, _ = ac.inputs(ac.CASES[2])
    S, m = ac.CASES[2][:2]
    rows = np.arange(10)
    states = np.array([(m + 1 + r) % S if (m + 1 + r) % S != m else 0 for r in rows])
    p64 = rc.state_probability(logits.numpy(), m, rows, states, np.float64)
    l = logits.double().view(-1, S)[:10].clone()
    l[:, m] = -np.inf
    want = torch.softmax(l, -1).numpy()[rows, states]
    assert np.abs(p64 - want).max() <= 1e-14
