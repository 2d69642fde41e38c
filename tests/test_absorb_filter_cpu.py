"""CPU: the temperature / top-k / top-p filter of the absorbing samplers without a GPU -- the vectorised replay of
tests/absorb_filter_cases.py against a state-by-state evaluation, the share of rows the GPU test may leave out of its exact
comparison (the replay's own `near` rows), the three config keys of the four samplers with their refusals, the warning of
eval_likelihood, and the binding's refusal of CPU tensors."""
import importlib
import warnings

import numpy as np
import pytest
import torch

import absorb_filter_cases as fc
from ctdd import native

SAMPLER_CONFIGS = {"AbsorbingLeap": "config_bert_synthetic_absorb", "AbsorbingConfidence": "config_bert_synthetic_absorb_conf",
                   "AbsorbingRemask": "config_bert_synthetic_absorb_remask", "AbsorbingFirstHit": "config_bert_synthetic_absorb_hit"}


def _sampler(name, **kw):
    import lib.sampling.sampling  # noqa: F401
    import lib.sampling.sampling_utils as su
    cfg = importlib.import_module("config.synthetic_config." + SAMPLER_CONFIGS[name]).get_config()
    assert cfg.sampler.name == name
    for k, v in kw.items():
        cfg.sampler[k] = v
    return su.get_sampler(cfg)


# ------------------------------------------------------------------------------------------------ the replay
@pytest.mark.parametrize("case", [c for c in fc.CASES if c[0] <= 65], ids=[i for c, i in zip(fc.CASES, fc.IDS) if c[0] <= 65])
def test_replay_against_brute_force(case):
    S, m = case
    rows = fc.inputs(case).view(-1, S).numpy()[:120]                     # ties (rows 0, 7, ..), the mask column, ROW_INF, ROW_NAN
    checked = 0
    for T in fc.TEMPS:
        for k in (0,) + fc.k_options(S):
            for p in (1.0, 0.9, 0.5, 1e-6):
                rep = fc.replay(rows, m, T, k, p)
                for r in range(rows.shape[0]):
                    want = fc.brute_force_row(rows[r], m, T, k, p)
                    if want is None:
                        assert rep["dead"][r] and not rep["kept"][r].any()
                        continue
                    if rep["near"][r]:
                        continue                                         # two fp64 sums in different orders may differ there
                    assert np.nonzero(rep["kept"][r])[0].tolist() == want, (T, k, p, r)
                    last = rep["edge"][r, 0]                              # (at -inf it stays without counting as kept)
                    assert not rep["kept"][r, m] and (last in want or rep["v"][r, last] == -np.inf)
                    checked += 1
                assert rep["dead"][fc.ROW_INF] and not rep["kept"][fc.ROW_NAN, np.isnan(rows[fc.ROW_NAN])].any()
    assert checked > 1000


def test_replay_of_a_row_by_hand():
    row = np.log(np.array([0.4, 0.3, 99.0, 0.2, 0.1], dtype=np.float64)).astype(np.float32)      # state 2 is the mask
    assert np.nonzero(fc.replay(row[None], 2, 1.0, 0, 0.65)["kept"][0])[0].tolist() == [0, 1]   # 0.4 + 0.3 reaches 0.65
    assert np.nonzero(fc.replay(row[None], 2, 1.0, 0, 0.75)["kept"][0])[0].tolist() == [0, 1, 3]
    assert np.nonzero(fc.replay(row[None], 2, 1.0, 1, 0.75)["kept"][0])[0].tolist() == [0]
    assert np.nonzero(fc.replay(row[None], 2, 1.0, 3, 1.0)["kept"][0])[0].tolist() == [0, 1, 3]
    assert np.nonzero(fc.replay(row[None], 2, 1.0, 4, 1.0)["kept"][0])[0].tolist() == [0, 1, 3, 4]   # k = S - 1: off
    tie = np.array([1.0, 2.0, 2.0, 0.0, 2.0], dtype=np.float32)
    r = fc.replay(tie[None], 3, 1.0, 2, 1.0)
    assert np.nonzero(r["kept"][0])[0].tolist() == [1, 2] and r["edge"][0].tolist() == [2, 4]    # ties in ascending s
    assert np.allclose(fc.probs(row, 2, 0.5, 2, 1.0)[[0, 1]], np.array([0.16, 0.09]) / 0.25)


@pytest.mark.parametrize("case", fc.CASES, ids=fc.IDS)
def test_share_of_near_rows(case):
    """The share condition of the GPU test: the rows whose boundary an fp32 sum may judge the other way are below 3 % of a case's rows,
    at every temperature and p the GPU test runs (alone and under top_k = 5)."""
    S, m = case
    flat = fc.inputs(case).view(-1, S).numpy()
    for T in fc.TEMPS:
        for p in fc.PS:
            for k in (0, 5):
                share = float(fc.replay(flat, m, T, k, p)["near"].mean())
                print(f"S={S} T={T} p={p} k={k}: near share {share:.4%}")
                assert share < 0.03


# ------------------------------------------------------------------------------------------------ the samplers' keys
@pytest.mark.parametrize("name", list(SAMPLER_CONFIGS))
def test_sampler_keys_and_refusals(name):
    plain = _sampler(name)
    assert (plain.temperature, plain.top_k, plain.top_p, plain.filtered) == (1.0, 0, 1.0, False)
    neutral = _sampler(name, temperature=1, top_k=0, top_p=1)
    assert (neutral.temperature, neutral.top_k, neutral.top_p, neutral.filtered) == (1.0, 0, 1.0, False)
    s = _sampler(name, temperature=0.7, top_k=5, top_p=0.9)
    assert (s.temperature, s.top_k, s.top_p, s.filtered) == (0.7, 5, 0.9, True)
    for kw in (dict(temperature=0.5), dict(top_k=1), dict(top_p=0.99), dict(top_k=np.int64(3))):
        assert _sampler(name, **kw).filtered
    for key, bad in (("temperature", 0.0), ("temperature", -1.0), ("temperature", float("inf")), ("temperature", float("nan")),
                     ("temperature", "hot"), ("top_k", -1), ("top_k", 2.5), ("top_k", True), ("top_p", 0.0), ("top_p", 1.5),
                     ("top_p", -0.1), ("top_p", float("nan")), ("top_p", "most")):
        with pytest.raises(ValueError, match="sampler." + key):
            _sampler(name, **{key: bad})


def test_neutral_values():
    assert native.absorb_filter_is_neutral() and native.absorb_filter_is_neutral(1, 0, 1)
    assert not native.absorb_filter_is_neutral(0.99) and not native.absorb_filter_is_neutral(top_k=1)
    assert not native.absorb_filter_is_neutral(top_p=0.999)
    assert "ctdd_absorb_filter" in native.EXPORTS


def test_binding_refuses_cpu_tensors():
    with pytest.raises(native.CtddError):
        native.absorb_filter(torch.zeros(2, 3, 4), torch.zeros(2, 3, dtype=torch.int32), 3, 0.7, 2, 0.9)
    with pytest.raises(native.CtddError):
        native.absorb_filter(torch.zeros(2, 3, 4), torch.zeros(2, 2, dtype=torch.int32), 3)


# ------------------------------------------------------------------------------------------------ the likelihood's warning
def test_eval_likelihood_warns_once_under_a_filter():
    from lib import likelihood

    class Stop(Exception):
        pass

    def loader():
        raise Stop
        yield

    def cfg_with(**kw):
        cfg = importlib.import_module("config.synthetic_config.config_bert_synthetic_absorb").get_config()
        for k, v in kw.items():
            cfg.sampler[k] = v
        return cfg

    for kw in (dict(temperature=0.7), dict(top_k=3), dict(top_p=0.9)):
        with warnings.catch_warnings(record=True) as got:
            warnings.simplefilter("always")
            with pytest.raises(Stop):
                likelihood.eval_likelihood(cfg_with(**kw), None, loader())
        assert [w.category for w in got] == [RuntimeWarning] and "unfiltered" in str(got[0].message)
    for kw in ({}, dict(temperature=1.0, top_k=0, top_p=1.0)):
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            with pytest.raises(Stop):
                likelihood.eval_likelihood(cfg_with(**kw), None, loader())
