"""CPU: confidence-ordered unmasking without a GPU -- the AbsorbingConfidence registry name and its two shipped configs, the refusal
of an unknown candidate rule and of CPU tensors, and the replay that the GPU tests compare the kernels with: commit_replay against
a brute-force selection that compares the floats themselves (ties, +-0, +-inf, NaN), the count rule against exact rationals."""
import importlib
import math
from fractions import Fraction

import numpy as np
import pytest
import torch

import absorb_conf_cases as cc
from ctdd import native

CONFIGS = (("synthetic_config.config_bert_synthetic_absorb_conf", "synthetic_config.config_bert_synthetic_absorb", 16),
           ("maze_config.config_bert_maze_absorb_conf", "maze_config.config_bert_maze_absorb", 32))


def _registries():
    import lib.models.models  # noqa: F401
    import lib.models.model_utils as mu
    import lib.sampling.sampling  # noqa: F401
    import lib.sampling.sampling_utils as su
    return mu, su


def test_registry_name_resolves():
    _, su = _registries()
    cls = su._SAMPLERS["AbsorbingConfidence"]
    assert cls.__name__ == "AbsorbingConfidence" and issubclass(cls, su._SAMPLERS["AbsorbingLeap"])
    assert "ctdd_absorb_propose" in native.EXPORTS and "ctdd_absorb_commit" in native.EXPORTS


@pytest.mark.parametrize("mod,base,steps", CONFIGS)
def test_shipped_configs_load(mod, base, steps):
    mu, su = _registries()
    cfg = importlib.import_module("config." + mod).get_config()
    s = cfg.sampler
    assert (s.name, s.num_steps, s.conf_temp, s.candidate) == ("AbsorbingConfidence", steps, 1.0, "sample")
    want = importlib.import_module("config." + base).get_config()
    for sec in ("data", "model", "loss", "training"):                    # everything but the sampler is the base config's
        assert cfg[sec].to_dict() == want[sec].to_dict(), sec
    assert s.rule == want.sampler.rule and s.min_t == want.sampler.min_t
    sampler = su.get_sampler(cfg)
    assert type(sampler).__name__ == "AbsorbingConfidence" and sampler.num_steps == steps
    assert sampler.conf_temp == 1.0 and sampler.candidate == "sample" and sampler.rule == "ancestral"
    cfg.device = "cpu"
    cfg.model.update(num_layers=1, engine="torch")
    model = mu.create_model(cfg, torch.device("cpu"))
    assert model.process.kind == "absorbing" and model.process.mask_state == cfg.model.mask_state


def test_candidate_rule_is_checked():
    _, su = _registries()
    cfg = importlib.import_module("config." + CONFIGS[0][0]).get_config()
    cfg.sampler.candidate = "argmax"
    assert su.get_sampler(cfg).candidate == "argmax"
    del cfg.sampler["conf_temp"], cfg.sampler["candidate"]
    sampler = su.get_sampler(cfg)
    assert sampler.conf_temp == 1.0 and sampler.candidate == "sample"    # the defaults
    cfg.sampler.candidate = "topk"
    with pytest.raises(ValueError, match="candidate"):
        su.get_sampler(cfg)


def test_native_calls_refuse_cpu_tensors():
    logits, x, score = torch.zeros(2, 3, 4), torch.zeros(2, 3, dtype=torch.int32), torch.zeros(2, 3)
    with pytest.raises(native.CtddError):
        native.absorb_propose(logits, x, 3)
    with pytest.raises(native.CtddError):
        native.absorb_commit(x, x, score, 3, p_unmask=0.5)


# ------------------------------------------------------------------------------------------------ the replay itself
def _better(a, b):
    """a ranks strictly above b, on the floats themselves: NaN below everything, -0 == +0, otherwise by value."""
    if math.isnan(a):
        return False
    return math.isnan(b) or a > b


def _brute_force(x, cand, score, m, k_of):
    out, changed = x.copy(), 0
    for n in range(x.shape[0]):
        left = [d for d in range(x.shape[1]) if x[n, d] == m]
        for _ in range(k_of(n, len(left))):
            best = left[0]
            for d in left[1:]:                                           # ascending d: a later row wins only if strictly better
                if _better(float(score[n, d]), float(score[n, best])):
                    best = d
            out[n, best] = cand[n, best]
            left.remove(best)
            changed += 1
    return out, changed


SPECIALS = np.array([-1.0, -0.0, 0.0, 2.0, np.inf, -np.inf, np.nan, 1e-45, -1e-45, 3.4e38, -3.4e38, 0.5], dtype=np.float32)


@pytest.mark.parametrize("seed", range(6))
def test_commit_replay_against_brute_force(seed):
    rng = np.random.default_rng(seed)
    N, D, m = 4, 23, 5
    x = np.where(rng.random((N, D)) < 0.7, m, rng.integers(0, 5, (N, D))).astype(np.int32)
    x[0] = 0                                                             # a sample with nothing masked
    cand = rng.integers(0, 5, (N, D)).astype(np.int32)
    score = SPECIALS[rng.integers(0, SPECIALS.size, (N, D))]
    if seed % 2:
        score = np.where(rng.random((N, D)) < 0.5, score, rng.standard_normal((N, D)).astype(np.float32))
    score[3, 1::2] = -score[3, 1::2]                                     # NaNs of either sign, more +-0 pairs
    for p in (0.0, 0.25, 0.3, 0.5, 1.0):
        got = cc.commit_replay(x, cand, score, m, p=p)
        want = _brute_force(x, cand, score, m, lambda n, M: min(M, math.ceil(Fraction(float(np.float32(p))) * M)))
        assert (got[0] == want[0]).all() and got[1] == want[1], p
    for counts in ([0, 1, 2, 3], [-2, 40, 5, 7], [3, 3, 3, 3]):
        got = cc.commit_replay(x, cand, score, m, counts=np.array(counts))
        want = _brute_force(x, cand, score, m, lambda n, M: min(M, max(0, counts[n])))
        assert (got[0] == want[0]).all() and got[1] == want[1], counts


def test_key_mapping_orders_like_the_floats():
    v = np.array([np.nan, -np.inf, -3.4e38, -1.0, -1e-45, -0.0, 0.0, 1e-45, 0.5, 2.0, 3.4e38, np.inf], dtype=np.float32)
    k = cc.score_keys(v).astype(np.int64)
    assert k[0] == 0 and k[1] == 0x007FFFFF and k[5] == k[6] == 0x80000000 and k[-1] == 0xFF800000
    assert (np.diff(k)[[0, 1, 2, 3, 4, 6, 7, 8, 9, 10]] > 0).all()
    assert cc.score_keys(np.array([-np.nan], dtype=np.float32))[0] == 0
    r = np.random.default_rng(0).standard_normal(1000).astype(np.float32)
    assert (np.argsort(cc.score_keys(r), kind="stable") == np.argsort(r, kind="stable")).all()


@pytest.mark.parametrize("p", [0.0, 0.25, 0.3, 0.5, 1.0])
def test_count_rule(p):
    for M in range(10):
        exact = math.ceil(Fraction(float(np.float32(p))) * M)           # the fp32 p as a rational: no rounding anywhere
        assert cc.count_rule(p, M) == min(M, exact)
        assert float(np.float32(p)) * M == Fraction(float(np.float32(p))) * M, "the fp64 product is not exact"
    known = {0.0: [0] * 10, 0.25: [0, 1, 1, 1, 1, 2, 2, 2, 2, 3], 0.3: [0, 1, 1, 1, 2, 2, 2, 3, 3, 3], 0.5: [0, 1, 1, 2, 2, 3, 3, 4, 4, 5],
             1.0: list(range(10))}
    assert [cc.count_rule(p, M) for M in range(10)] == known[p]
    # float32(0.3) lies above 0.3: at M = 10 the product is just above 3, so four rows are committed
    assert cc.count_rule(0.3, 10) == 4 and cc.count_rule(0.25, 8) == 2
