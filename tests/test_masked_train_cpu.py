"""CPU: what of the masked transformer's HIP training path (ctdd/masked_train.py) can be said without a GPU -- which models
`training_supported` takes, that the chunk walk covers the enumeration exactly once, and that cfg.model.engine_train =
"hip-masked" leaves a CPU forward on the module."""
import importlib
import warnings

import pytest
import torch

from test_bert_cpu import tiny_model


@pytest.mark.parametrize("tag,expected", [("mask_a", True), ("mask_c", True), ("mask_mlp", False), ("bert_a", False)])
def test_training_supported_on_golden_cases(golden, tag, expected):
    from ctdd.masked_train import training_supported
    assert training_supported(tiny_model(golden, tag)[1]) is expected


@pytest.mark.parametrize("mod,expected", [("synthetic_config.config_masked_synthetic", True), ("maze_config.config_bert_mazemasked", True),
                                          ("maze_config.config_bert_maze", False)])
def test_training_supported_on_shipped_configs(mod, expected):
    import lib.models.models  # noqa: F401
    import lib.models.model_utils as mu
    from ctdd.masked_train import training_supported
    cfg = importlib.import_module("config." + mod).get_config()
    cfg.device = "cpu"
    assert training_supported(mu.create_model(cfg, torch.device("cpu"))) is expected


def test_training_supported_respects_the_kernels_shape_limits(golden):
    from ctdd.masked_train import training_supported
    cfg, model, *_ = tiny_model(golden, "mask_a")
    assert training_supported(model)
    hd = cfg.model.embed_dim // cfg.model.num_heads
    assert hd in (4, 8, 16, 32)
    cfg.model.num_heads = cfg.model.embed_dim // 2       # head dimension 2: no training kernel takes it
    assert not training_supported(model)
    cfg.model.num_heads = cfg.model.embed_dim // hd
    assert training_supported(model)


@pytest.mark.parametrize("B,D,cond,chunk", [(3, 12, 0, 6), (3, 12, 0, 7), (3, 12, 0, 1), (3, 12, 0, 36), (3, 12, 0, 1000), (4, 17, 4, 13),
                                            (4, 17, 4, 7), (5, 17, 16, 2), (2, 225, 0, 290)])
def test_chunk_walk_covers_the_enumeration_exactly_once(B, D, cond, chunk):
    """Totals that the chunk divides and totals it does not, with and without a conditional prefix: the windows are contiguous,
    in order, none longer than the chunk, only the last one shorter, and together they are [0, B D')."""
    from ctdd.masked_train import chunk_walk
    total = B * (D - cond)
    walk = chunk_walk(total, chunk)
    seen = [g for r0, n in walk for g in range(r0, r0 + n)]
    assert seen == list(range(total))
    assert all(n == min(chunk, total) for _, n in walk[:-1]) and 1 <= walk[-1][1] <= chunk
    assert len(walk) == -(-total // min(chunk, total))


def test_chunk_walk_follows_enum_chunk_size(golden):
    from ctdd.masked_train import chunk_walk
    from lib.networks.hollow_networks import enum_chunk_size
    cfg, model, x, *_ = tiny_model(golden, "mask_c")
    total = x.shape[0] * (x.shape[1] - int(cfg.model.conditional_dim))
    assert len(chunk_walk(total, enum_chunk_size(cfg, total))) == 1          # the default: one chunk at this size
    cfg.model.enum_chunk = 7
    walk = chunk_walk(total, enum_chunk_size(cfg, total))
    assert [n for _, n in walk[:-1]] == [7] * (len(walk) - 1) and sum(n for _, n in walk) == total


def test_cpu_forward_under_hip_masked_runs_the_module_without_a_warning(golden):
    cfg, model, x, t, ref = tiny_model(golden, "mask_a")
    cfg.model.engine_train = "hip-masked"
    model.train()
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        out = model(x, t)
        out.square().mean().backward()
    assert not [w for w in rec if issubclass(w.category, RuntimeWarning)], [str(w.message) for w in rec]
    assert model._trainer is None and out.shape == ref.shape
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in model.parameters())
