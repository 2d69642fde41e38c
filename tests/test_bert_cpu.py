"""CPU: the x0-prediction ("BERT") and masked transformer score models -- registry names, the four shipped configs' parameter
counts, reference checkpoints and logits (tests/golden/bert.npz, tools/gen_golden_bert.py), the refused settings, and the
chunked enumeration of the masked model against a plain loop over positions."""
import ast
import importlib

import numpy as np
import pytest
import torch

T = torch.from_numpy
NAMES = ("UniVarBertEMA", "UniformBertEMA", "UniVarMaskedEMA", "UniformMaskedEMA")
CONFIGS = {"maze_config.config_bert_maze": 7802627, "synthetic_config.config_bert_synthetic": 504834,
           "synthetic_config.config_masked_synthetic": 554754, "maze_config.config_bert_mazemasked": 554883}
CASES = ("bert_a", "bert_b", "mask_a", "mask_c", "mask_mlp")


def tiny_cfg(meta, device="cpu"):
    """A config for one golden case, from the shipped synthetic configs of its family."""
    masked = "Masked" in meta["name"]
    mod = "config.synthetic_config." + ("config_masked_synthetic" if masked else "config_bert_synthetic")
    cfg = importlib.import_module(mod).get_config()
    cfg.device = device
    cfg.data.S = meta["S"]
    cfg.model.update(name=meta["name"], concat_dim=meta["D"], embed_dim=meta["embed_dim"], num_layers=meta["num_layers"],
                     num_heads=meta["num_heads"], mlp_dim=meta["mlp_dim"], qkv_dim=meta["embed_dim"], readout_dim=meta["S"],
                     out_dim=meta["S"], num_output_ffresiduals=meta["num_output_ffresiduals"], readout=meta["readout"],
                     conditional_dim=meta["conditional_dim"], t_func=meta["t_func"], rate_const=meta["rate_const"],
                     time_scale_factor=meta["time_scale_factor"])
    return cfg


def tiny_model(golden, tag, device="cpu"):
    import lib.models.models  # noqa: F401
    import lib.models.model_utils as mu
    g = golden("bert")
    meta = ast.literal_eval(str(g[f"{tag}__cfg"]))
    cfg = tiny_cfg(meta, device)
    model = mu.create_model(cfg, torch.device(device))
    pre = f"{tag}__sd__"
    sd = {k[len(pre):]: T(v).to(device) for k, v in g.items() if k.startswith(pre)}
    sd.update(ema_decay=0.999, ema_num_updates=0, ema_shadow_params=[])
    model.load_state_dict(sd)                       # raises on any missing key, and on any unexpected one besides the EMA entries
    model.init_ema()
    model.eval()
    return cfg, model, T(g[f"{tag}__x"]).to(device), T(g[f"{tag}__t"]).to(device), g[f"{tag}__out"]


@pytest.mark.parametrize("name", NAMES)
def test_registry_names_resolve(name):
    import lib.models.models  # noqa: F401
    import lib.models.model_utils as mu
    assert mu.get_model(name).__name__ == name


@pytest.mark.parametrize("mod", sorted(CONFIGS))
def test_shipped_configs_build_with_reference_parameter_counts(mod):
    import lib.models.models  # noqa: F401
    import lib.models.model_utils as mu
    import lib.sampling.sampling  # noqa: F401
    import lib.sampling.sampling_utils as su
    import lib.losses.losses  # noqa: F401
    import lib.losses.losses_utils as lu
    cfg = importlib.import_module("config." + mod).get_config()
    cfg.device = "cpu"
    model = mu.create_model(cfg, torch.device("cpu"))
    assert sum(p.numel() for p in model.parameters()) == CONFIGS[mod]
    assert cfg.model.engine_train == "torch"
    su.get_sampler(cfg)                               # the sampler and loss names are registered ones
    lu.get_loss(cfg)


@pytest.mark.parametrize("tag", CASES)
def test_golden_checkpoint_loads_and_forward_matches_reference(golden, tag):
    cfg, model, x, t, ref = tiny_model(golden, tag)
    assert np.abs(ref).max() >= 1.0                   # an absolute bar needs O(1) logits
    assert len(set(t.tolist())) == 3
    with torch.no_grad():
        out = model(x, t).numpy()
    assert out.shape == ref.shape
    np.testing.assert_allclose(out, ref, rtol=0, atol=1e-4)
    c = int(cfg.model.conditional_dim)
    if tag == "mask_c":
        assert c == 4
    assert (out[:, :c] == 0).all() and (c == 0 or np.abs(out[:, c:]).min() > 0)


def test_refused_settings_raise_value_error(golden):
    import lib.models.models  # noqa: F401
    import lib.models.model_utils as mu
    g = golden("bert")
    for tag, field, value in (("bert_a", "readout", "mlp"), ("bert_a", "is_ebm", True), ("mask_a", "is_ebm", True),
                              ("mask_a", "readout", "nope")):
        cfg = tiny_cfg(ast.literal_eval(str(g[f"{tag}__cfg"])))
        cfg.model[field] = value
        with pytest.raises(ValueError):
            mu.create_model(cfg, torch.device("cpu"))


def _loop_forward(net, x, t):
    """The masked model written as the plain loop over positions: one encoder pass per masked position."""
    from lib.networks.hollow_networks import transformer_timestep_embedding
    temb = transformer_timestep_embedding(t * net.temb_scale, net.embed_dim)
    c = int(getattr(net.config.model, "conditional_dim", 0) or 0)
    cols = [torch.zeros(x.shape[0], net.S) for _ in range(c)]
    for pos in range(c, x.shape[1]):
        xm = x.clone()
        xm[:, pos] = net.S
        cols.append(net.transformer(xm, temb, pos).squeeze(1))
    return torch.stack(cols, dim=1)


@pytest.mark.parametrize("tag", ["mask_a", "mask_c", "mask_mlp"])
def test_enumerative_forward_equals_position_loop(golden, tag):
    cfg, model, x, t, _ = tiny_model(golden, tag)
    g = torch.Generator().manual_seed(3)
    x = torch.randint(0, cfg.data.S, (5, x.shape[1]), generator=g)
    t = torch.rand(5, generator=g)
    with torch.no_grad():
        out, ref = model(x, t), _loop_forward(model.net, x, t)
    np.testing.assert_allclose(out.numpy(), ref.numpy(), rtol=0, atol=1e-4)


@pytest.mark.parametrize("tag", ["mask_a", "mask_c"])
def test_enumerative_forward_independent_of_chunking(golden, tag):
    cfg, model, x, t, ref = tiny_model(golden, tag)
    total = x.shape[0] * (x.shape[1] - int(cfg.model.conditional_dim))
    outs = []
    for chunk in (None, 1, 7, total - 1, total, 10 * total):          # 7 and total - 1 leave a ragged last chunk
        cfg.model.enum_chunk = chunk
        with torch.no_grad():
            outs.append(model(x, t).numpy())
        np.testing.assert_allclose(outs[-1], ref, rtol=0, atol=1e-4)
        np.testing.assert_allclose(outs[-1], outs[0], rtol=0, atol=1e-4)
    assert total % 7 != 0


def test_train_mode_runs_the_module_and_backpropagates(golden):
    cfg, model, x, t, _ = tiny_model(golden, "mask_a")
    model.train()
    out = model(x, t)
    out.square().mean().backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in model.parameters())
