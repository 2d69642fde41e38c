"""CPU: what of the x0-prediction transformer's HIP training path (ctdd/bert_train.py) can be said without a GPU -- which models
`training_supported` takes, and that cfg.model.engine_train = "hip-encoder" leaves a CPU forward on the module."""
import importlib
import warnings

import pytest
import torch

from test_bert_cpu import tiny_model


@pytest.mark.parametrize("tag,expected", [("bert_a", True), ("bert_b", True), ("mask_a", False), ("mask_c", False), ("mask_mlp", False)])
def test_training_supported_on_golden_cases(golden, tag, expected):
    from ctdd.bert_train import training_supported
    assert training_supported(tiny_model(golden, tag)[1]) is expected


@pytest.mark.parametrize("mod,expected", [("maze_config.config_bert_maze", True), ("synthetic_config.config_bert_synthetic", True),
                                          ("synthetic_config.config_masked_synthetic", False), ("maze_config.config_bert_mazemasked", False)])
def test_training_supported_on_shipped_configs(mod, expected):
    import lib.models.models  # noqa: F401
    import lib.models.model_utils as mu
    from ctdd.bert_train import training_supported
    cfg = importlib.import_module("config." + mod).get_config()
    cfg.device = "cpu"
    assert training_supported(mu.create_model(cfg, torch.device("cpu"))) is expected


def test_training_supported_respects_the_kernels_shape_limits(golden):
    from ctdd.bert_train import training_supported
    cfg, model, *_ = tiny_model(golden, "bert_b")
    assert training_supported(model)
    cfg.model.num_heads = 1                              # head dimension 64: inference kernels only
    assert not training_supported(model)


def test_cpu_forward_under_hip_encoder_runs_the_module_without_a_warning(golden):
    cfg, model, x, t, ref = tiny_model(golden, "bert_a")
    cfg.model.engine_train = "hip-encoder"
    model.train()
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        out = model(x, t)
        out.square().mean().backward()
    assert not [w for w in rec if issubclass(w.category, RuntimeWarning)], [str(w.message) for w in rec]
    assert model._trainer is None and out.shape == ref.shape
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in model.parameters())
