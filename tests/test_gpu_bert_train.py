"""GPU: the x0-prediction ("BERT") transformer's TRAINING path on HIP kernels (ctdd/bert_train.py): unmasked attention (mode 3)
of the four training attention kernels against fp64 and against each other, ctdd_bert_embed_bwd / ctdd_bert_gather_bwd through
the C ABI, BertTrainer against the reference's golden logits and autograd through the torch module at tiny and at maze size,
dropout-mask consistency, one CTElbo step, and the fallbacks of cfg.model.engine_train = "hip-encoder"."""
import ctypes as C
import importlib
import warnings

import numpy as np
import pytest
import torch

from test_bert_cpu import tiny_model
from test_gpu_hollow_train import _compare, _grads

pytestmark = pytest.mark.gpu

SHAPES_FP32 = [(33, 33), (226, 226), (18, 18), (129, 129), (64, 64), (5, 61), (40, 226)]      # (129: crosses one 128-query workgroup)
SHAPES_MFMA = [(226, 226), (33, 33), (129, 129), (40, 226)]


def _registries():
    import lib.models.models  # noqa: F401
    import lib.models.model_utils as mu
    import lib.losses.losses  # noqa: F401
    import lib.losses.losses_utils as lu
    import lib.training.training  # noqa: F401
    import lib.training.training_utils as tu
    import lib.optimizers.optimizers  # noqa: F401
    import lib.optimizers.optimizers_utils as ou
    return mu, lu, tu, ou


def _shipped(mod, **model_over):
    mu = _registries()[0]
    cfg = importlib.import_module("config." + mod).get_config()
    cfg.device = "cuda"
    cfg.model.update(**model_over)
    torch.manual_seed(0)
    return cfg, mu.create_model(cfg, torch.device("cuda"))


def _set_dropout(cfg, model, p_drop, p_att):
    """The rates the trainer reads (the config) and the ones the torch module holds."""
    cfg.model.update(dropout_rate=p_drop, attention_dropout_rate=p_att)
    for mod in model.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = p_drop
        elif isinstance(mod, torch.nn.MultiheadAttention):
            mod.dropout = p_att


def _attn_inputs(B, Tq, Tk, H, hd, seed):
    """Packed qkv rows (B*T, 3E) where Tq == Tk, separate q / k / v otherwise; plus the output weight."""
    E = H * hd
    g = torch.Generator(device="cuda").manual_seed(seed)
    if Tq == Tk:
        base = [torch.randn((B * Tq, 3 * E), device="cuda", generator=g)]
    else:
        base = [torch.randn((B * n, E), device="cuda", generator=g) for n in (Tq, Tk, Tk)]
    return base, torch.randn((B * Tq, E), device="cuda", generator=g)


def _run_attention(base, wgt, B, Tq, Tk, H, hd, p, rng, bf16):
    from ctdd.hollow_train import AttentionFn
    ins = [t.clone().requires_grad_(True) for t in base]
    q, k, v = (ins + [None, None])[:3]
    out = AttentionFn.apply(q, k, v, B, Tq, Tk, H, hd, 3, p, rng if p > 0 else None, 4, bf16)
    (out * wgt).sum().backward()
    return [out.detach()] + [t.grad for t in ins]


# ------------------------------------------------------------------------------------------------ mode 3 of the training attention kernels
@pytest.mark.parametrize("hd", [8, 16])
@pytest.mark.parametrize("Tq,Tk", SHAPES_FP32)
def test_unmasked_training_attention_fp32_against_fp64(hd, Tq, Tk):
    """ctdd_hollow_attention_train / _bwd in mode 3 on N(0, 1) inputs against torch fp64 softmax attention and its autograd under a
    random output weight: forward 2e-5 (the bar of the fp32 inference kernel's mode 3), every gradient within 1e-4 of the
    reference tensor's max-abs (the fp32 bar of the hollow training tests); every output element finite."""
    B, H = 3, 4
    E = H * hd
    base, wgt = _attn_inputs(B, Tq, Tk, H, hd, 100 + hd + 7 * Tq + Tk)
    got = _run_attention(base, wgt, B, Tq, Tk, H, hd, 0.0, None, False)
    ins = [t.double().requires_grad_(True) for t in base]
    if Tq == Tk:
        q, k, v = (ins[0].view(B, Tq, 3, H, hd)[:, :, c].transpose(1, 2) for c in range(3))
    else:
        q, k, v = (t.view(B, -1, H, hd).transpose(1, 2) for t in ins)
    ref_out = (torch.softmax((q @ k.transpose(-1, -2)) / hd ** 0.5, -1) @ v).transpose(1, 2).reshape(B * Tq, E)
    (ref_out * wgt.double()).sum().backward()
    ref = [ref_out.detach()] + [t.grad for t in ins]
    for t in got:
        assert torch.isfinite(t).all()
    err = float((got[0].double() - ref[0]).abs().max())
    print(f"mode 3 fp32 hd={hd} {Tq}x{Tk}: forward max err {err:.3e} (bar 2e-5)")
    assert err < 2e-5
    for name, g, r in zip(("dqkv",) if Tq == Tk else ("dq", "dk", "dv"), got[1:], ref[1:]):
        e = float((g.double() - r).abs().max()) / float(r.abs().max())
        print(f"mode 3 fp32 hd={hd} {Tq}x{Tk}: {name} max err {e:.3e} of the range (bar 1e-4)")
        assert e < 1e-4, name


@pytest.mark.parametrize("hd", [16, 32])
@pytest.mark.parametrize("p", [0.0, 0.2])
@pytest.mark.parametrize("Tq,Tk", SHAPES_MFMA)
def test_unmasked_training_attention_matrix_core_kernels_match_fp32_kernels(hd, p, Tq, Tk):
    """ctdd_hollow_attention_train_bf16 / _bwd_bf16 in mode 3 against the fp32 FMA kernels on the same inputs and the SAME Philox
    dropout masks, at the bars of the masked modes' test: 2e-2 of the range in max-abs, 6e-3 in relative L2."""
    B, H = 3, 4
    base, wgt = _attn_inputs(B, Tq, Tk, H, hd, 300 + hd + 7 * Tq + Tk)
    rng = torch.tensor([99, 5], dtype=torch.int64, device="cuda")
    ref = _run_attention(base, wgt, B, Tq, Tk, H, hd, p, rng, False)
    got = _run_attention(base, wgt, B, Tq, Tk, H, hd, p, rng, True)
    for r, g in zip(ref, got):
        assert torch.isfinite(g).all()
        scale = float(r.abs().max())
        e_max, e_l2 = float((g - r).abs().max()) / scale, float((g - r).norm() / r.norm())
        print(f"mode 3 mfma hd={hd} p={p} {Tq}x{Tk}: max {e_max:.3e} of the range (bar 2e-2), L2 {e_l2:.3e} (bar 6e-3)")
        assert e_max < 2e-2 and e_l2 < 6e-3


def test_unmasked_training_attention_dropout_rate():
    """q = k = 0 and V = 1 make every probability 1 / Tk, so out Tk (1 - p) counts the kept keys of a query."""
    from ctdd.hollow_train import AttentionFn
    B, T, H, hd, p = 3, 33, 4, 8, 0.25
    E = H * hd
    rng = torch.tensor([1234, 7], dtype=torch.int64, device="cuda")
    qkv = torch.zeros((B * T, 3 * E), device="cuda")
    qkv[:, 2 * E:] = 1.0
    out = AttentionFn.apply(qkv, None, None, B, T, T, H, hd, 3, p, rng, 3).view(B, T, H, hd)
    kept = out * T * (1 - p)
    assert float((kept - kept.round()).abs().max()) < 1e-3
    frac = float(kept[..., 0].sum() / (B * H * T * T))
    print(f"mode 3 dropout: kept fraction {frac:.4f} (1 - p = {1 - p})")
    assert abs(frac - (1 - p)) < 0.02


@pytest.mark.parametrize("mode", [-1, 4, 7])
def test_training_attention_refuses_unknown_modes_and_launches_nothing(mode):
    from ctdd import hollow_train as ht
    lib = ht.lib()
    B, T, H, hd = 2, 33, 4, 16
    E = H * hd
    st = torch.cuda.current_stream().cuda_stream
    qkv = torch.randn((B * T, 3 * E), device="cuda")
    dout = torch.randn((B * T, E), device="cuda")
    for fwd, bwd in ((lib.ctdd_hollow_attention_train, lib.ctdd_hollow_attention_bwd),
                     (lib.ctdd_hollow_attention_train_bf16, lib.ctdd_hollow_attention_bwd_bf16)):
        nan = lambda shape, dt=torch.float32: torch.full(shape, float("nan"), device="cuda", dtype=dt)
        out, stats, dqkv = nan((B * T, E)), nan((B, H, T, 4)), nan((B * T, 3 * E))
        out_hi, dqkv_hi = nan((B * T, E), torch.bfloat16), nan((B * T, 3 * E), torch.bfloat16)
        a = ht._attn_args(qkv, None, None, B, T, T, H, hd, mode, 0.0, None, 1)
        a.out, a.stats, a.out_bf16, a.d_out = out.data_ptr(), stats.data_ptr(), out_hi.data_ptr(), dout.data_ptr()
        a.dq, a.dk, a.dv = dqkv.data_ptr(), dqkv.data_ptr() + 4 * E, dqkv.data_ptr() + 8 * E
        a.dq_bf16, a.dk_bf16, a.dv_bf16 = dqkv_hi.data_ptr(), dqkv_hi.data_ptr() + 2 * E, dqkv_hi.data_ptr() + 4 * E
        a.dq_bs = a.dk_bs = a.dv_bs = T * 3 * E
        a.dq_rs = a.dk_rs = a.dv_rs = 3 * E
        assert fwd(C.byref(a), st) < 0
        assert bwd(C.byref(a), st) < 0
        torch.cuda.synchronize()
        for buf in (out, stats, dqkv, out_hi, dqkv_hi):
            assert torch.isnan(buf.float()).all()


# ------------------------------------------------------------------------------------------------ embed / gather backward through the C ABI
@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
def test_bert_embed_and_gather_backward_against_torch(dtype):
    from ctdd import bert_train as bt
    lib = bt.lib()
    B, D, E, S = 3, 17, 64, 5
    g_ = torch.Generator(device="cuda").manual_seed(11)
    x = torch.randint(0, S, (B, D), device="cuda", generator=g_).to(dtype)
    g = torch.randn((B, D + 1, E), device="cuda", generator=g_)
    st = torch.cuda.current_stream().cuda_stream
    dwb = torch.zeros((2, E), device="cuda")
    a = bt._BertEmbedBwdArgs()
    bt._state_ptrs(a, x)
    a.g, a.B, a.D, a.E, a.S, a.dw, a.db = g.data_ptr(), B, D, E, S, dwb[0].data_ptr(), dwb[1].data_ptr()
    assert lib.ctdd_bert_embed_bwd(C.byref(a), st) == 0
    xn = (x.double() / (S - 1)) * 2 - 1
    ref_dw = (g[:, 1:].double() * xn[:, :, None]).sum((0, 1))
    ref_db = g[:, 1:].double().sum((0, 1))
    for name, got, ref in (("dw", dwb[0], ref_dw), ("db", dwb[1], ref_db)):
        err, bar = float((got.double() - ref).abs().max()), 2e-5 * max(1.0, float(ref.abs().max()))
        print(f"bert embed bwd {dtype} {name}: max err {err:.3e} (bar {bar:.3e})")
        assert err < bar
    dxr = torch.randn((B * D, E), device="cuda", generator=g_)
    denc = torch.full((B, D + 1, E), float("nan"), device="cuda")
    assert lib.ctdd_bert_gather_bwd(dxr.data_ptr(), B, D, 0, E, denc.data_ptr(), st) == 0
    torch.cuda.synchronize()
    assert torch.equal(denc[:, 1:], dxr.view(B, D, E)) and bool((denc[:, 0] == 0).all())
    denc.fill_(float("nan"))
    assert lib.ctdd_bert_gather_bwd(dxr.data_ptr(), B, D, 2, E, denc.data_ptr(), st) < 0       # a conditional prefix is the masked model's
    torch.cuda.synchronize()
    assert torch.isnan(denc).all()


# ------------------------------------------------------------------------------------------------ the trainer
def _weighted(f, x, t, wgt):
    return (lambda o: ((o * wgt).sum().backward(), o.detach())[1])(f(x, t))


@pytest.mark.parametrize("tag", ["bert_a", "bert_b"])
def test_bert_train_matches_autograd_on_golden_nets(golden, tag):
    """bert_a (S 3, D 12, E 32, 2 layers, head dimension 8, one FiLM residual) and bert_b (S 5, D 17, E 64, 1 layer, head dimension
    16, no FiLM residual) in train mode with dropout 0: fp32 logits against the golden output and the module (1e-4), every
    parameter gradient against autograd through the module (1e-4 of its range); then through the wrapper with
    engine_train = "hip-encoder" and the default bf16 precision at the hollow test's bars for tiny nets."""
    from ctdd.bert_train import BertTrainer, training_supported
    cfg, model, x, t, ref = tiny_model(golden, tag, "cuda")
    _set_dropout(cfg, model, 0.0, 0.0)
    model.train()
    assert training_supported(model)
    torch.manual_seed(3)
    wgt = torch.randn(ref.shape, device="cuda")
    cfg.model.engine = "torch"
    out_ref, g_ref = _grads(model, lambda: _weighted(model, x, t, wgt))
    cfg.model.engine = "hip"
    tr = BertTrainer(model, precision="fp32")
    out, g_hip = _grads(model, lambda: _weighted(tr, x, t, wgt))
    print(f"{tag} fp32: logits max err {float((out - out_ref).abs().max()):.3e} (bar 1e-4)")
    np.testing.assert_allclose(out.cpu().numpy(), ref, rtol=0, atol=1e-4)
    np.testing.assert_allclose(out.cpu().numpy(), out_ref.cpu().numpy(), rtol=0, atol=1e-4)
    print(f"{tag} fp32: worst gradient error {_compare(g_hip, g_ref, 1e-4):.3e} of the range (bar 1e-4)")
    cfg.model.engine_train = "hip-encoder"
    assert model._trainer is None
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        out_w, g_w = _grads(model, lambda: _weighted(model, x, t, wgt))
    assert model._trainer is not None and model._trainer.precision == "bf16"
    assert not [w for w in rec if "no HIP training kernels" in str(w.message) or "coverage" in str(w.message)]
    assert float((out_w - out_ref).abs().max()) < 5e-2 * max(1.0, float(out_ref.abs().max()))
    print(f"{tag} bf16 through the wrapper: worst gradient L2 error {_compare(g_w, g_ref, 0.25, l2=True):.3e} (bar 0.25)")


def test_bert_train_matches_autograd_maze_size():
    """config_bert_maze (D = 225, S = 3, E = 128, 12 layers, head dimension 16), batch 4, dropout 0, at the bars of the hollow
    transformer's maze-size test (set against a float64 evaluation of a 16-block net; this one is 24 blocks deep)."""
    from config.maze_config.config_bert_maze import get_config
    from ctdd.bert_train import BertTrainer
    mu = _registries()[0]
    cfg = get_config()
    cfg.device = "cuda"
    cfg.model.update(dropout_rate=0.0, attention_dropout_rate=0.0)
    torch.manual_seed(0)
    model = mu.create_model(cfg, torch.device("cuda"))
    x = torch.randint(0, 3, (4, 225), device="cuda")
    t = torch.tensor([0.02, 0.3, 0.5, 0.99], device="cuda")
    wgt = torch.randn((4, 225, 3), device="cuda")
    cfg.model.engine = "torch"
    out_ref, g_ref = _grads(model, lambda: _weighted(model, x, t, wgt))
    cfg.model.engine = "hip"
    scale = max(1.0, float(out_ref.abs().max()))
    out, g_hip = _grads(model, lambda: _weighted(BertTrainer(model, precision="fp32"), x, t, wgt))
    print(f"maze fp32: logits {float((out - out_ref).abs().max()) / scale:.3e} of the scale (bar 2e-4)")
    assert float((out - out_ref).abs().max()) < 2e-4 * scale
    print(f"maze fp32: worst gradient L2 error {_compare(g_hip, g_ref, 1e-2, l2=True):.3e} (bar 1e-2)")
    out_b, g_b = _grads(model, lambda: _weighted(BertTrainer(model, precision="bf16"), x, t, wgt))
    print(f"maze bf16: logits {float((out_b - out_ref).abs().max()) / scale:.3e} of the scale (bar 5e-2)")
    assert float((out_b - out_ref).abs().max()) < 5e-2 * scale
    print(f"maze bf16: worst gradient L2 error {_compare(g_b, g_ref, 0.1, l2=True):.3e} (bar 0.1)")


def test_bert_train_dropout_masks_are_consistent(golden):
    """Dropout 0.2 on the residual, MLP and attention-probability sites of bert_a: the backward regenerates the forward's Philox
    masks (analytic directional derivative against a central finite difference with the SAME masks), another step draws other
    masks, eval mode equals the golden logits."""
    from ctdd.bert_train import BertTrainer
    cfg, model, x, t, ref = tiny_model(golden, "bert_a", "cuda")
    _set_dropout(cfg, model, 0.2, 0.2)
    model.train()
    tr = BertTrainer(model, precision="fp32")
    torch.manual_seed(5)
    wgt = torch.randn(ref.shape, device="cuda", dtype=torch.float64)
    params = list(model.parameters())
    dirs = [torch.randn_like(p) for p in params]

    def loss_at(step):
        tr.rng[1] = step                                  # the forward bumps it: masks of step + 1
        return (tr(x, t).double() * wgt).sum()

    for p in params:
        p.grad = None
    l0 = loss_at(10)
    l0.backward()
    analytic = sum(float((p.grad.double() * d.double()).sum()) for p, d in zip(params, dirs))
    eps = 2e-3
    with torch.no_grad():
        for p, d in zip(params, dirs):
            p.add_(eps * d)
        lp = float(loss_at(10))
        for p, d in zip(params, dirs):
            p.sub_(2 * eps * d)
        lm = float(loss_at(10))
        for p, d in zip(params, dirs):
            p.add_(eps * d)
        again = float(loss_at(10))
        other = float(loss_at(11))
    fd = (lp - lm) / (2 * eps)
    l0v = float(l0.detach())
    print(f"dropout consistency: analytic {analytic:.6e}, finite difference {fd:.6e}; loss {l0v:.6e}, again {again:.6e}, next step {other:.6e}")
    assert abs(again - l0v) < 1e-6 * max(1.0, abs(l0v))                      # same step -> same masks
    assert abs(other - l0v) > 1e-4 * max(1.0, abs(l0v))                      # next step -> different masks
    assert abs(fd - analytic) < 2e-2 * max(abs(analytic), 1.0), (fd, analytic)
    model.eval()
    with torch.enable_grad():
        out_eval = tr(x, t)
    np.testing.assert_allclose(out_eval.detach().cpu().numpy(), ref, rtol=0, atol=1e-4)
    model.train()


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_bert_train_two_forwards_before_backward_keep_their_masks(golden, precision):
    """A second training forward before the first one's backward (two-pass CT-ELBO, gradient accumulation) must not move the
    first forward's dropout masks: gradients of the interleaved run equal the sum of each forward run and backpropagated alone."""
    from ctdd.bert_train import BertTrainer
    cfg, model, x, t, ref = tiny_model(golden, "bert_a", "cuda")
    _set_dropout(cfg, model, 0.2, 0.2)
    model.train()
    tr = BertTrainer(model, precision=precision)
    torch.manual_seed(7)
    w1 = torch.randn(ref.shape, device="cuda")
    w2 = torch.randn(ref.shape, device="cuda")
    x2 = (x + 1) % cfg.data.S

    def alone(step, xx, ww):
        tr.rng[1] = step
        return _grads(model, lambda: (tr(xx, t) * ww).sum().backward())[1]

    g1 = alone(20, x, w1)                                  # masks of step 21
    g2 = alone(21, x2, w2)                                 # masks of step 22

    def both():
        tr.rng[1] = 20
        o1 = tr(x, t)                                      # step 21
        o2 = tr(x2, t)                                     # step 22, before the first backward
        ((o1 * w1).sum() + (o2 * w2).sum()).backward()

    gb = _grads(model, both)[1]
    tol = 1e-4 if precision == "fp32" else 2e-2
    for n, a in g1.items():
        if a is None:
            continue
        want = a + g2[n]
        scale = max(float(want.abs().max()), 1e-6)
        err = float((gb[n] - want).abs().max()) / scale
        assert err < tol, f"{n}: interleaved forwards changed the gradient by {err:.3e} of its range"


def test_bert_ctelbo_loss_matches_torch():
    """One CTElbo calc_loss (one forward pass) on config_bert_synthetic, batch 8, dropout 0, fp32 training precision: loss value
    and every parameter gradient of engine_train = "hip-encoder" against "torch" under the same seeds."""
    lu = _registries()[1]
    res = {}
    for engine_train in ("torch", "hip-encoder"):
        cfg, model = _shipped("synthetic_config.config_bert_synthetic", dropout_rate=0.0, attention_dropout_rate=0.0,
                              engine_train=engine_train, engine_train_precision="fp32")
        loss_fn = lu.get_loss(cfg)
        x = torch.randint(0, cfg.data.S, (8, int(cfg.model.concat_dim)), device="cuda")
        torch.manual_seed(11)
        l = loss_fn.calc_loss(x, {"model": model, "n_iter": 0})
        for p in model.parameters():
            p.grad = None
        l.backward()
        res[engine_train] = (float(l.detach()), {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None})
        assert (model._trainer is not None) == (engine_train == "hip-encoder")
    err = abs(res["hip-encoder"][0] - res["torch"][0])
    print(f"CTElbo loss: torch {res['torch'][0]:.6e}, hip-encoder {res['hip-encoder'][0]:.6e}")
    assert err < 1e-4 * max(1.0, abs(res["torch"][0]))
    print(f"CTElbo gradients: worst error {_compare(res['hip-encoder'][1], res['torch'][1], 2e-3):.3e} of the range (bar 2e-3)")


# ------------------------------------------------------------------------------------------------ fallbacks
@pytest.mark.parametrize("case", ["masked", "head64"])
def test_hip_encoder_falls_back_to_the_module_with_one_warning(case):
    """engine_train = "hip-encoder" on a masked model, and on an x0-prediction model whose head dimension (64) the training
    kernels do not take: one RuntimeWarning, the steps run on the module, no trainer is built."""
    _, lu, tu, ou = _registries()
    if case == "masked":
        cfg, model = _shipped("synthetic_config.config_masked_synthetic", engine_train="hip-encoder")
    else:
        cfg, model = _shipped("synthetic_config.config_bert_synthetic", engine_train="hip-encoder", num_heads=1)
        assert cfg.model.embed_dim // cfg.model.num_heads == 64
    from ctdd.bert_train import training_supported
    assert not training_supported(model)
    cfg.training.max_t = 0.99
    state = {"model": model, "optimizer": ou.get_optimizer(model.parameters(), cfg), "n_iter": 0}
    w0 = [p.detach().clone() for p in model.parameters()]
    mb = torch.randint(0, cfg.data.S, (6, int(cfg.model.concat_dim)), device="cuda")
    loss, step = lu.get_loss(cfg), tu.get_train_step(cfg)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        for _ in range(2):
            out = step.step(state, loss, mb)
            state["n_iter"] += 1
    assert out.dim() == 0 and torch.isfinite(out)
    assert sum(int(not torch.equal(a, b)) for a, b in zip(w0, model.parameters())) > 0.5 * len(w0)
    assert model._trainer is None
    hits = [w for w in rec if issubclass(w.category, RuntimeWarning) and "HIP encoder training kernels" in str(w.message)]
    assert len(hits) == 1, [str(w.message) for w in rec]


@pytest.mark.parametrize("engine_train", ["torch", "hip"])
def test_other_engine_train_values_build_no_trainer(engine_train):
    cfg, model = _shipped("synthetic_config.config_bert_synthetic", engine_train=engine_train)
    x = torch.randint(0, cfg.data.S, (4, int(cfg.model.concat_dim)), device="cuda")
    t = torch.rand(4, device="cuda")
    with warnings.catch_warnings(record=True):
        warnings.simplefilter("always")
        model(x, t).square().mean().backward()
    assert model._trainer is None
    assert all(p.grad is not None for p in model.parameters())
