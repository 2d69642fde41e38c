"""GPU: the two D3PM configs end to end at reduced size -- one Standard.step through the engine's training path and
ctdd_d3pm_loss, then p_sample_loop in eval mode through the inference plan and ctdd_d3pm_step."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _build(which):
    import lib.d3pm as d3pm
    import lib.models.model_utils as model_utils
    import lib.models.models  # noqa: F401
    import lib.optimizers.optimizers  # noqa: F401
    import lib.optimizers.optimizers_utils as optimizers_utils
    import lib.training.training  # noqa: F401
    import lib.training.training_utils as training_utils
    from lib.losses import losses
    if which == "mnist":
        from config.mnist_config.config_mnist_d3pm import get_config
        cfg = get_config()
        cfg.model.update(ch=32, time_embed_dim=32)        # attn_resolutions stays [48]: attention in the mid block only
        cfg.data.batch_size = 4
        shape = (4, 1, 28, 28)
    else:
        from config.synthetic_config.config_synthetic_d3pm import get_config
        cfg = get_config()
        shape = (8, 32)
    cfg.model.num_timesteps = 12
    cfg.model.d3pm_fused = True            # the kernels at both configs, whatever each config's measured default is
    torch.manual_seed(0)
    model = model_utils.create_model(cfg, torch.device("cuda"))
    state = {"model": model, "optimizer": optimizers_utils.get_optimizer(model.parameters(), cfg), "n_iter": 0}
    dif = d3pm.make_diffusion(cfg.model)
    return cfg, model, state, dif, losses.d3pm_loss(cfg, dif), training_utils.get_train_step(cfg), shape


@pytest.mark.parametrize("which", ["mnist", "synthetic"])
def test_train_step_then_sampling(which):
    from ctdd import native
    cfg, model, state, dif, loss, step, shape = _build(which)
    S = cfg.data.S
    x = torch.randint(0, S, shape).cuda()
    before = [p.detach().clone() for p in model.parameters()]
    n0 = native.LAUNCH_COUNTS.get("ctdd_d3pm_loss", 0)
    val = step.step(state, x, loss)
    assert torch.isfinite(val)
    assert native.LAUNCH_COUNTS.get("ctdd_d3pm_loss", 0) == n0 + 1
    assert any(not torch.equal(a, b) for a, b in zip(before, model.parameters()))
    if which == "mnist":
        assert model._engine is not None and len(model._engine._train_plans) == 1        # the U-Net's HIP training plan ran
    model.eval()
    s0 = native.LAUNCH_COUNTS.get("ctdd_d3pm_step", 0)
    torch.manual_seed(9)
    out = dif.p_sample_loop(model, shape, 3)
    assert native.LAUNCH_COUNTS["ctdd_d3pm_step"] == s0 + 3
    assert out.shape == shape and int(out.min()) >= 0 and int(out.max()) < S
    torch.manual_seed(9)
    assert torch.equal(out, dif.p_sample_loop(model, shape, 3))
    model.train()


def test_mnist_loop_runs_the_inference_plan_and_decodes_the_network_at_t0():
    """One step (t = 0) of p_sample_loop at the reduced MNIST config is the argmax of the network's logits at t = 0: checked
    against a plain forward (own output buffer, own time path) on every pixel whose top-two gap is >= 1e-3; the loop's forward
    went through the engine's inference plan."""
    import lib.d3pm as d3pm
    cfg, model, state, dif, loss, step, shape = _build("mnist")
    with torch.no_grad():                       # (the output convolution starts at zero: every logit equal; move all weights off it)
        for p in model.parameters():
            p.add_(0.05 * torch.randn_like(p))
    model.init_ema()
    model.eval()
    torch.manual_seed(17)
    x_init, x = dif.p_sample_loop(model, shape, 1, return_x_init=True)
    assert model._engine is not None and len(model._engine._plans) >= 1
    assert getattr(model, "_engine_time_row", None) is None and not getattr(model, "_borrow_engine_output", False)
    with torch.no_grad():
        logits = model(x_init, torch.zeros(shape[0], device="cuda")).float().reshape(shape[0], -1, cfg.data.S)
    top = torch.topk(logits, 2, dim=-1)
    decided = (top.values[..., 0] - top.values[..., 1]) >= 1e-3
    print(f"t = 0 decode: {float(decided.float().mean()):.4f} of the pixels decided")
    assert bool(decided.any())
    assert torch.equal(x.reshape(shape[0], -1)[decided], top.indices[..., 0][decided])
    model.train()
