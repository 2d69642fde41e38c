"""CPU: the first-hitting sampler without a GPU -- DeviceForwardProcess.time_of_alpha against alpha, the level recursion of the replay
against the law it claims (every entry's masking level is uniform on (0, c0); bars from the binomial law), the selection replay
against a brute force over the keys, the two shipped configs, the registry name and the refusals."""
import importlib
import math

import numpy as np
import pytest
import torch

import absorb_hit_cases as hc
from ctdd import native


def _registries():
    import lib.models.models  # noqa: F401
    import lib.models.model_utils as mu
    import lib.sampling.sampling  # noqa: F401
    import lib.sampling.sampling_utils as su
    return mu, su


# ------------------------------------------------------------------------------------------------ time_of_alpha
@pytest.mark.parametrize("t_func,rate_const", hc.SCHEDULES)
def test_time_of_alpha_inverts_alpha(t_func, rate_const):
    pr = hc.proc(t_func, rate_const)
    t = torch.linspace(0.01, 0.99, 52, dtype=torch.float64)[1:-1]        # 50 points inside (0.01, 0.99)
    back = pr.time_of_alpha(pr.alpha(t))
    err = ((back - t).abs() / t).max().item()
    print(f"{t_func}: largest relative error of time_of_alpha(alpha(t)) over {t.numel()} points: {err:.2e}")
    assert t.numel() == 50 and back.dtype == torch.float64 and err <= 1e-12
    assert pr.time_of_alpha(pr.alpha(t.float())).dtype == torch.float32  # the dtype follows the input


def test_time_of_alpha_edges_and_refusal():
    from ctdd import process
    pr = hc.proc("sqrt_cos", 1.55)
    lo = pr.time_of_alpha(torch.tensor([math.exp(-1.55) * 0.5, 1.0], dtype=torch.float64))
    assert abs(lo[0].item() - 1.0) <= 1e-15 and lo[1].item() == 0.0      # below alpha(1): t = 1; alpha = 1: t = 0
    with pytest.raises(ValueError, match="absorbing"):
        process.DeviceForwardProcess("uniform", 5, "cpu", rate_const=1.0).time_of_alpha(torch.tensor([0.5]))


# ------------------------------------------------------------------------------------------------ the replay is exact in law
N_, M_, C0 = 64, 50, 0.8


def _run_replay(kmax, seed):
    """The time replay iterated until every entry has had its event, from the all-masked state at level C0 with no closing level;
    one masked entry per accepted event is unmasked in between (which one does not enter the recursion).  Returns every event's level."""
    pr = hc.proc()
    m = pr.mask_state
    x = np.full((N_, M_), m)
    logc = np.full(N_, math.log(C0))
    levels, steps = [[] for _ in range(N_)], -(-M_ // kmax)
    for it in range(steps):
        counts, logc_new, t_eval, near, lv = hc.hit_time_replay(x, logc, m, kmax, -np.inf, pr, 0.0, 1.0, seed, it, levels=True)
        for n in range(N_):
            left = M_ - len(levels[n])
            assert counts[n] == min(kmax, left) == len(lv[n]) and not near[n]
            assert logc_new[n] == lv[n][-1] and all(b < a for a, b in zip([logc[n]] + lv[n], lv[n]))   # the levels fall
            want_t = math.exp(lv[n][0]) / (1 - 1e-3)                      # loglinear: t = c / (1 - alpha_eps)
            assert abs(t_eval[n] - want_t) <= 1e-15                       # (alpha = 1 - c is rounded at 1: an absolute bound)
            x[n, len(levels[n]):len(levels[n]) + counts[n]] = 0
            levels[n] += lv[n]
        logc = logc_new
    assert (x != m).all() and all(len(v) == M_ for v in levels)
    return np.exp(np.asarray(levels))


@pytest.mark.parametrize("kmax", [1, 7])
def test_replay_levels_follow_the_uniform_law(kmax):
    """Given M entries masked at level c0 their masking levels are i.i.d. uniform on (0, c0): of the N M = 3200 events the share with a
    level above c* is Binomial(3200, q) / 3200 with q = 1 - c* / c0.  Bar: 4 standard deviations of that law.  kmax = 7 takes the
    events seven to a step (the last step one): the levels of a step are the same order statistics, so the same statistic and bar
    hold, and the level a step hands on is its last event's."""
    c = _run_replay(kmax, seed=20250117 + kmax)
    assert c.shape == (N_, M_) and (c < C0).all() and (c > 0).all()
    for frac in (0.25, 0.5, 0.75):
        q = 1 - frac
        share, bar = float((c > frac * C0).mean()), 4 * math.sqrt(q * (1 - q) / (N_ * M_))
        print(f"kmax={kmax}: share of events above {frac} c0: {share:.4f}, law {q:.4f}, bar {bar:.4f}")
        assert abs(share - q) <= bar


def test_replay_stops_at_the_closing_level():
    pr = hc.proc()
    m = pr.mask_state
    x = np.full((4, 6), m)
    x[3] = 0
    logc = np.log(np.array([0.5, 0.5, 1e-3, 0.5]))
    _, _, _, _, lv = hc.hit_time_replay(x, logc, m, 6, -np.inf, pr, 0.01, 0.9, 5, 0, levels=True)
    cut = 0.5 * (lv[0][2] + lv[0][3])                                    # between sample 0's third and fourth event
    counts, out, t_eval, near = hc.hit_time_replay(x, logc, m, 6, cut, pr, 0.01, 0.9, 5, 0)
    assert counts[0] == 3 and out[0] == cut and counts[2] == 0 and out[2] == cut and t_eval[2] == 0.01
    assert counts[3] == 0 and out[3] == logc[3] and t_eval[3] == 0.01 and not near.any()
    assert counts[1] == sum(v >= cut for v in lv[1])                      # (the levels fall: the accepted events come first)
    assert 0.01 <= t_eval[0] <= 0.9 and abs(t_eval[0] - min(max(math.exp(lv[0][0]) / (1 - 1e-3), 0.01), 0.9)) <= 1e-15


@pytest.mark.parametrize("t_func,rate_const", hc.SCHEDULES)
def test_time_seeds_leave_no_event_near_the_closing_level(t_func, rate_const):
    """The inputs, seeds and closing levels of tests/test_gpu_absorb_hit.py: no event lies within 1e-9 of the closing level, a sample
    without a masked row and one with are there, and the finite closing level stops its sample inside the step."""
    pr = hc.proc(t_func, rate_const)
    m = pr.mask_state
    for N, D in hc.TIME_SHAPES:
        x, logc = hc.time_inputs(N, D, pr)
        M = (x == m).sum(1)
        assert M[0] == 0 and M[1] > 0 and np.isfinite(logc).all() and (logc <= 0).all()
        for kmax in hc.KMAX:
            seed, offset = hc.time_seed(D, kmax)
            cuts, big, big_count = hc.closing_levels(x, logc, m, kmax, pr, seed, offset)
            assert cuts[0] == -np.inf and cuts[1] < logc[big]
            for log_cmin in cuts:
                counts, out, t_eval, near = hc.hit_time_replay(x, logc, m, kmax, log_cmin, pr, hc.T_MIN, hc.T_MAX, seed, offset)
                assert not near.any() and counts[0] == 0 and ((t_eval >= hc.T_MIN) & (t_eval <= hc.T_MAX)).all()
                if log_cmin > -np.inf:
                    assert counts[big] == big_count < min(kmax, M[big]) and out[big] == log_cmin
                else:
                    assert (counts == np.minimum(kmax, M)).all()


# ------------------------------------------------------------------------------------------------ the selection replay
@pytest.mark.parametrize("D", [1, 5, 65])
def test_selection_replay_against_brute_force(D):
    rng = np.random.default_rng(D)
    N, m, seed, offset = 4, 2, 0x5EED0000 + D, 3
    x = np.where(rng.random((N, D)) < 0.6, m, 0)
    x[0] = m                                                             # one sample fully masked
    for n in range(N):
        M = int((x[n] == m).sum())
        for k in hc.count_options(M):
            counts = np.zeros(N, dtype=np.int64)
            counts[n] = k
            sel = hc.hit_select_replay(x, m, counts, seed, offset)
            assert all(sel[o].size == 0 for o in range(N) if o != n)
            keys = {d: int(hc.row_keys([n * D + d], seed, offset)[0]) for d in range(D) if x[n, d] == m}
            want = [d for d in keys if sum(1 for e in keys if keys[e] > keys[d] or (keys[e] == keys[d] and e < d)) < hc.clamp_count(k, M)]
            assert sel[n].tolist() == sorted(want) and len(want) == hc.clamp_count(k, M)


# ------------------------------------------------------------------------------------------------ configs, registry, refusals
@pytest.mark.parametrize("mod,base", [("synthetic_config.config_bert_synthetic_absorb_hit", "synthetic_config.config_bert_synthetic_absorb"),
                                      ("maze_config.config_bert_maze_absorb_hit", "maze_config.config_bert_maze_absorb")])
def test_shipped_configs_load(mod, base):
    mu, su = _registries()
    cfg = importlib.import_module("config." + mod).get_config()
    want = importlib.import_module("config." + base).get_config()
    assert cfg.sampler.name == "AbsorbingFirstHit" and cfg.sampler.num_steps == cfg.model.concat_dim == want.model.concat_dim
    for sec in want.to_dict():                                           # everything but the sampler section is the base config's
        if sec != "sampler":
            a, b = cfg[sec], want[sec]
            assert (a.to_dict() if hasattr(a, "to_dict") else a) == (b.to_dict() if hasattr(b, "to_dict") else b), sec
    ours, theirs = cfg.sampler.to_dict(), want.sampler.to_dict()
    assert {k for k in ours if k not in theirs or ours[k] != theirs[k]} <= {"name", "num_steps", "candidate"} and set(theirs) <= set(ours)
    sampler = su.get_sampler(cfg)
    D = cfg.model.concat_dim
    assert type(sampler).__name__ == "AbsorbingFirstHit" and sampler.plan(D) == (1, D) and sampler.candidate == "sample"
    cfg.device = "cpu"
    cfg.model.update(num_layers=1, engine="torch")
    model = mu.create_model(cfg, torch.device("cpu"))
    assert model.process.kind == "absorbing" and model.process.p["t_func"] in native.ABSORB_T_FUNCS


def test_registry_plan_and_option_refusals():
    _, su = _registries()
    cls = su._SAMPLERS["AbsorbingFirstHit"]
    assert cls.__name__ == "AbsorbingFirstHit" and issubclass(cls, su._SAMPLERS["AbsorbingLeap"])
    assert "ctdd_absorb_hit_time" in native.EXPORTS and "ctdd_absorb_hit_step" in native.EXPORTS
    cfg = importlib.import_module("config.synthetic_config.config_bert_synthetic_absorb_hit").get_config()
    cfg.sampler.num_steps = 8
    sampler = su.get_sampler(cfg)
    assert sampler.plan(50) == (7, 8) and sampler.plan(32) == (4, 8) and sampler.plan(1) == (1, 1) and sampler.plan(9) == (2, 5)
    cfg.sampler.candidate = "argmax"
    assert su.get_sampler(cfg).candidate == "argmax"
    for key, bad in (("rule", "euler"), ("rule", "tauleap"), ("candidate", "best"), ("num_steps", 0)):
        c = importlib.import_module("config.synthetic_config.config_bert_synthetic_absorb_hit").get_config()
        c.sampler[key] = bad
        with pytest.raises(ValueError, match=key):
            su.get_sampler(c)


def test_native_calls_refuse_cpu_tensors():
    x, logc = torch.zeros(2, 3, dtype=torch.int32), torch.zeros(2, dtype=torch.float64)
    sched = dict(t_func="loglinear", rate_const=1.0, alpha_eps=1e-3)
    with pytest.raises(native.CtddError):
        native.absorb_hit_time(x, logc, 3, 1, -math.inf, sched, 0.01, 1.0)
    with pytest.raises(native.CtddError):
        native.absorb_hit_step(torch.zeros(2, 3, 4), x, torch.zeros(2, dtype=torch.int32), 3)
    with pytest.raises(native.CtddError):
        native.absorb_hit_time(x, logc, 3, 1, -math.inf, dict(t_func="linear"), 0.01, 1.0)
