"""GPU: the masked ("enumerative") transformer's TRAINING path on HIP kernels (ctdd/masked_train.py): ctdd_bert_embed_enum_bwd /
ctdd_bert_gather_enum_bwd through the C ABI against torch fp64, the short-sequence training attention against fp64 and against
the generic fp32 kernels (same Philox masks), MaskedTrainer against the reference's golden logits and autograd through the torch
module at tiny and at maze size and under two chunkings, dropout-stream consistency across chunks and forwards, one CatRMNLL
loss and step, and the fallbacks of cfg.model.engine_train = "hip-masked"."""
import ctypes as C
import warnings

import numpy as np
import pytest
import torch

from test_bert_cpu import tiny_model
from test_gpu_bert_train import _attn_inputs, _registries, _set_dropout, _shipped, _weighted
from test_gpu_hollow_train import _compare, _grads

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ enumerate-mode backward through the C ABI
def _windows(total, Dp):
    """The whole enumeration; a window from inside sample 0 to inside sample 2; one row."""
    return [(0, total), (Dp // 2, 2 * Dp + 3 - Dp // 2), (Dp + 1, 1)]


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("cond", [0, 4])
def test_embed_enum_backward_against_fp64(dtype, cond):
    from ctdd import bert_train as bt, masked_train as mt
    lib = mt.lib()
    B, D, E, S = 3, 17, 64, 5
    Dp = D - cond
    total = B * Dp
    g_ = torch.Generator(device="cuda").manual_seed(21 + cond)
    x = torch.randint(0, S, (B, D), device="cuda", generator=g_).to(dtype)
    st = torch.cuda.current_stream().cuda_stream
    for r0, n in _windows(total, Dp):
        assert 0 <= r0 and r0 + n <= total
        g = torch.randn((n, D + 1, E), device="cuda", generator=g_)
        seq = torch.arange(r0, r0 + n, device="cuda")
        b, p = seq // Dp, cond + seq % Dp
        xm = x[b].long().scatter(1, p[:, None], S)                              # (n, D): sample b with token p masked
        xn = (xm.double() / (S - 1)) * 2 - 1
        ref_dw = (g[:, 1:].double() * xn[:, :, None]).sum((0, 1))
        ref_db = g[:, 1:].double().sum((0, 1))
        dwb = torch.zeros((2, E), device="cuda")
        a = mt._BertEmbedEnumBwdArgs()
        bt._state_ptrs(a, x)
        a.g, a.B, a.D, a.E, a.S, a.cond, a.rows, a.r0 = g.data_ptr(), B, D, E, S, cond, n, r0
        a.dw, a.db = dwb[0].data_ptr(), dwb[1].data_ptr()
        for call in (1, 2):                                                      # the second call adds to the first
            assert lib.ctdd_bert_embed_enum_bwd(C.byref(a), st) == 0
            for name, got, ref in (("dw", dwb[0], call * ref_dw), ("db", dwb[1], call * ref_db)):
                err, bar = float((got.double() - ref).abs().max()), 2e-5 * max(1.0, float(ref.abs().max()))
                print(f"embed enum bwd {dtype} cond={cond} window=({r0}, {n}) call {call} {name}: max err {err:.3e} (bar {bar:.3e})")
                assert err < bar
    a.r0, a.rows = total - 1, 2                                                  # a window past the enumeration: refused, nothing written
    dwb.fill_(float("nan"))
    assert lib.ctdd_bert_embed_enum_bwd(C.byref(a), st) < 0
    torch.cuda.synchronize()
    assert torch.isnan(dwb).all()


@pytest.mark.parametrize("cond", [0, 4])
def test_gather_enum_backward_equals_the_scatter(cond):
    from ctdd import masked_train as mt
    lib = mt.lib()
    B, D, E = 3, 17, 64
    Dp = D - cond
    total = B * Dp
    g_ = torch.Generator(device="cuda").manual_seed(31 + cond)
    dxr = torch.randn((total, E), device="cuda", generator=g_)
    st = torch.cuda.current_stream().cuda_stream
    for r0, n in _windows(total, Dp):
        denc = torch.full((n, D + 1, E), float("nan"), device="cuda")
        poisoned = torch.full_like(dxr, float("nan"))                           # rows outside the window are never read
        poisoned[r0:r0 + n] = dxr[r0:r0 + n]
        assert lib.ctdd_bert_gather_enum_bwd(poisoned.data_ptr(), r0, n, B, D, cond, E, denc.data_ptr(), st) == 0
        seq = torch.arange(r0, r0 + n, device="cuda")
        ref = torch.zeros((n, D + 1, E), device="cuda")
        ref[torch.arange(n, device="cuda"), 1 + cond + seq % Dp] = dxr[r0:r0 + n]
        torch.cuda.synchronize()
        assert torch.equal(denc, ref), (r0, n)
    denc = torch.full((2, D + 1, E), float("nan"), device="cuda")
    assert lib.ctdd_bert_gather_enum_bwd(dxr.data_ptr(), total - 1, 2, B, D, cond, E, denc.data_ptr(), st) < 0
    torch.cuda.synchronize()
    assert torch.isnan(denc).all()


# ------------------------------------------------------------------------------------------------ short-sequence training attention
SHORT_T = [1, 5, 13, 33, 64]


def _run_short(base, wgt, B, T, H, hd, p, rng, short, layer=4):
    from ctdd.hollow_train import AttentionFn
    qkv = base[0].clone().requires_grad_(True)
    out = AttentionFn.apply(qkv, None, None, B, T, T, H, hd, 3, p, rng if p > 0 else None, layer, False, short)
    (out * wgt).sum().backward()
    return [out.detach(), qkv.grad]


@pytest.mark.parametrize("hd", [4, 8])
@pytest.mark.parametrize("T", SHORT_T)
def test_short_training_attention_against_fp64(hd, T):
    """ctdd_bert_attention_short_train / _bwd on N(0, 1) inputs against torch fp64 softmax attention and its autograd under a random
    output weight, at the project's bars for the fp32 kernels: forward 2e-5, every gradient within 1e-4 of the reference
    tensor's max-abs, all outputs finite.  B H = 9 pairs: not a multiple of the four pairs of a workgroup."""
    B, H = 3, 3
    E = H * hd
    base, wgt = _attn_inputs(B, T, T, H, hd, 500 + hd + 7 * T)
    got = _run_short(base, wgt, B, T, H, hd, 0.0, None, True)
    ins = base[0].double().requires_grad_(True)
    q, k, v = (ins.view(B, T, 3, H, hd)[:, :, c].transpose(1, 2) for c in range(3))
    ref_out = (torch.softmax((q @ k.transpose(-1, -2)) / hd ** 0.5, -1) @ v).transpose(1, 2).reshape(B * T, E)
    (ref_out * wgt.double()).sum().backward()
    for t in got:
        assert torch.isfinite(t).all()
    err = float((got[0].double() - ref_out.detach()).abs().max())
    print(f"short attention hd={hd} T={T}: forward max err {err:.3e} (bar 2e-5)")
    assert err < 2e-5
    floor = 1e-3 * float(ins.grad.abs().max())              # (T = 1: one key, dq and dk are zero in exact arithmetic)
    for c, name in enumerate(("dq", "dk", "dv")):
        g, r = got[1].view(B * T, 3, E)[:, c].double(), ins.grad.view(B * T, 3, E)[:, c]
        e = float((g - r).abs().max()) / max(float(r.abs().max()), floor)
        print(f"short attention hd={hd} T={T}: {name} max err {e:.3e} of the range (bar 1e-4)")
        assert e < 1e-4, name


@pytest.mark.parametrize("hd", [4, 8])
@pytest.mark.parametrize("T", SHORT_T)
def test_short_training_attention_matches_generic_kernels_under_dropout(hd, T):
    """Same inputs, the same rng / layer, p = 0.2: the short kernels draw the generic fp32 kernels' masks.  Each kernel is within
    the fp64 bars (2e-5, 1e-4 of the range), so two of them differ by at most twice that."""
    B, H = 3, 3
    base, wgt = _attn_inputs(B, T, T, H, hd, 700 + hd + 7 * T)
    rng = torch.tensor([99, 5], dtype=torch.int64, device="cuda")
    ref = _run_short(base, wgt, B, T, H, hd, 0.2, rng, False)
    got = _run_short(base, wgt, B, T, H, hd, 0.2, rng, True)
    for g in got:
        assert torch.isfinite(g).all()
    err = float((got[0] - ref[0]).abs().max())
    print(f"short vs generic hd={hd} T={T} p=0.2: forward max diff {err:.3e} (bar 4e-5)")
    assert err < 4e-5
    e = float((got[1] - ref[1]).abs().max()) / float(ref[1].abs().max())
    print(f"short vs generic hd={hd} T={T} p=0.2: dqkv max diff {e:.3e} of the range (bar 2e-4)")
    assert e < 2e-4


def test_short_training_attention_dropout_rate():
    """q = k = 0 and V = 1 make every probability 1 / T, so out T (1 - p) counts the kept keys of a query."""
    from ctdd.hollow_train import AttentionFn
    B, T, H, hd, p = 3, 33, 4, 8, 0.25
    E = H * hd
    rng = torch.tensor([1234, 7], dtype=torch.int64, device="cuda")
    qkv = torch.zeros((B * T, 3 * E), device="cuda")
    qkv[:, 2 * E:] = 1.0
    out = AttentionFn.apply(qkv, None, None, B, T, T, H, hd, 3, p, rng, 3, False, True).view(B, T, H, hd)
    kept = out * T * (1 - p)
    assert float((kept - kept.round()).abs().max()) < 1e-3
    frac = float(kept[..., 0].sum() / (B * H * T * T))
    print(f"short attention dropout: kept fraction {frac:.4f} (1 - p = {1 - p})")
    assert abs(frac - (1 - p)) < 0.02


@pytest.mark.parametrize("case", ["T65", "TqTk", "mode0", "hd16"])
def test_short_training_attention_refuses_what_is_outside_its_contract(case):
    from ctdd import hollow_train as ht
    lib = ht.lib()
    B, H = 2, 4
    Tq, Tk, hd, mode = {"T65": (65, 65, 8, 3), "TqTk": (33, 40, 8, 3), "mode0": (33, 33, 8, 0), "hd16": (33, 33, 16, 3)}[case]
    E = H * hd
    st = torch.cuda.current_stream().cuda_stream
    nan = lambda *shape: torch.full(shape, float("nan"), device="cuda")
    q, k, v = (torch.randn((B * n, E), device="cuda") for n in (Tq, Tk, Tk))
    dout = torch.randn((B * Tq, E), device="cuda")
    out, stats, dq, dk, dv = nan(B * Tq, E), nan(B, H, Tq, 4), nan(B * Tq, E), nan(B * Tk, E), nan(B * Tk, E)
    a = ht._attn_args(q, k, v, B, Tq, Tk, H, hd, mode, 0.0, None, 1)
    a.out, a.stats, a.d_out = out.data_ptr(), stats.data_ptr(), dout.data_ptr()
    a.dq, a.dk, a.dv = dq.data_ptr(), dk.data_ptr(), dv.data_ptr()
    a.dq_bs, a.dk_bs, a.dv_bs, a.dq_rs, a.dk_rs, a.dv_rs = Tq * E, Tk * E, Tk * E, E, E, E
    assert lib.ctdd_bert_attention_short_train(C.byref(a), st) < 0
    assert lib.ctdd_bert_attention_short_bwd(C.byref(a), st) < 0
    torch.cuda.synchronize()
    for buf in (out, stats, dq, dk, dv):
        assert torch.isnan(buf).all()


# ------------------------------------------------------------------------------------------------ the trainer
@pytest.mark.parametrize("tag", ["mask_a", "mask_c"])
def test_masked_train_matches_autograd_on_golden_nets(golden, tag):
    """mask_a and mask_c (E 16, head dimension 4; mask_c with a conditional prefix) in train mode with dropout 0: fp32 logits
    against the golden output and the module (1e-4), every parameter gradient against autograd through the module (1e-4 of its
    range), with the default chunk and with enum_chunk = 7 (at least three chunks, a ragged last one, a border inside a sample);
    the two chunkings agree to 1e-5; the conditional prefix is exactly zero; then through the wrapper with engine_train =
    "hip-masked" and the default bf16 precision at the BERT test's bars for tiny nets."""
    from ctdd.masked_train import MaskedTrainer, chunk_walk, training_supported
    from lib.networks.hollow_networks import enum_chunk_size
    cfg, model, x, t, ref = tiny_model(golden, tag, "cuda")
    _set_dropout(cfg, model, 0.0, 0.0)
    model.train()
    assert training_supported(model)
    c = int(cfg.model.conditional_dim)
    B, D = x.shape[0], x.shape[1]
    Dp = D - c
    torch.manual_seed(3)
    wgt = torch.randn(ref.shape, device="cuda")
    cfg.model.engine = "torch"
    out_ref, g_ref = _grads(model, lambda: _weighted(model, x, t, wgt))
    cfg.model.engine = "hip"
    tr = MaskedTrainer(model, precision="fp32")
    outs = []
    for chunk in (None, 7):
        cfg.model.enum_chunk = chunk
        walk = chunk_walk(B * Dp, enum_chunk_size(cfg, B * Dp))
        if chunk:
            assert len(walk) >= 3 and walk[-1][1] < 7 and Dp % 7 != 0
        out, g_hip = _grads(model, lambda: _weighted(tr, x, t, wgt))
        outs.append(out)
        print(f"{tag} fp32 chunk={chunk} ({len(walk)} chunks): logits max err {float((out - out_ref).abs().max()):.3e} (bar 1e-4)")
        np.testing.assert_allclose(out.cpu().numpy(), ref, rtol=0, atol=1e-4)
        np.testing.assert_allclose(out.cpu().numpy(), out_ref.cpu().numpy(), rtol=0, atol=1e-4)
        print(f"{tag} fp32 chunk={chunk}: worst gradient error {_compare(g_hip, g_ref, 1e-4):.3e} of the range (bar 1e-4)")
        if c:
            assert bool((out.view(B, D, -1)[:, :c] == 0).all())
    assert float((outs[0] - outs[1]).abs().max()) < 1e-5
    cfg.model.engine_train = "hip-masked"
    assert model._trainer is None
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        out_w, g_w = _grads(model, lambda: _weighted(model, x, t, wgt))
    assert isinstance(model._trainer, MaskedTrainer) and model._trainer.precision == "bf16"
    assert not [w for w in rec if "training kernels" in str(w.message) or "coverage" in str(w.message)], [str(w.message) for w in rec]
    assert float((out_w - out_ref).abs().max()) < 5e-2 * max(1.0, float(out_ref.abs().max()))
    print(f"{tag} bf16 through the wrapper: worst gradient L2 error {_compare(g_w, g_ref, 0.25, l2=True):.3e} (bar 0.25)")


def test_masked_train_dropout_streams_are_consistent(golden, monkeypatch):
    """Dropout 0.2 on the residual, MLP and attention-probability sites of mask_a, seven sequences per chunk: the backward
    regenerates the forward's Philox masks (analytic directional derivative against a central finite difference with the SAME step
    counter), the same step gives the same loss, the next step another, two chunks of one forward do not carry the same
    residual-dropout mask, and eval mode equals the golden logits."""
    from ctdd import hollow_train as ht, masked_train as mt
    cfg, model, x, t, ref = tiny_model(golden, "mask_a", "cuda")
    _set_dropout(cfg, model, 0.2, 0.2)
    cfg.model.enum_chunk = 7
    model.train()
    tr = mt.MaskedTrainer(model, precision="fp32")
    torch.manual_seed(5)
    wgt = torch.randn(ref.shape, device="cuda", dtype=torch.float64)
    params = list(model.parameters())
    dirs = [torch.randn_like(p) for p in params]
    first = []                                             # (input, output) of every chunk's first dropout (layer 1)

    class Recording:
        @staticmethod
        def apply(t_, p, rng, layer):
            out = mt_DropoutFn.apply(t_, p, rng, layer)
            if layer == 1:
                first.append((t_.detach(), out.detach()))
            return out

    mt_DropoutFn = ht.DropoutFn                           # (the trainers' dropout sites live in hollow_train.Forward)
    monkeypatch.setattr(ht, "DropoutFn", Recording)

    def loss_at(step):
        tr.rng[1] = step                                  # the forward bumps it: chunk i draws the masks of step + 1 + i
        return (tr(x, t).double() * wgt).sum()

    for p in params:
        p.grad = None
    l0 = loss_at(10)
    l0.backward()
    kept = [(o != 0)[i != 0] for i, o in first[:2]]       # chunks 0 and 1: seven sequences each
    assert first[0][0].shape == first[1][0].shape and first[0][0].shape[0] == 7
    for kk in kept:
        assert abs(float(kk.float().mean()) - 0.8) < 0.05
    assert not torch.equal(kept[0], kept[1]), "two chunks of one forward share a residual-dropout mask"
    assert len({int(s) for s in tr.chunk_rngs[:, 1]}) == tr.chunk_rngs.shape[0]
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
def test_masked_train_two_forwards_before_backward_keep_their_masks(golden, precision):
    """A second training forward before the first one's backward must not move the first forward's dropout masks: gradients of
    the interleaved run equal the sum of each forward run and backpropagated alone (1e-4 fp32, 2e-2 bf16)."""
    from ctdd.masked_train import MaskedTrainer
    cfg, model, x, t, ref = tiny_model(golden, "mask_a", "cuda")
    _set_dropout(cfg, model, 0.2, 0.2)
    cfg.model.enum_chunk = 7
    model.train()
    tr = MaskedTrainer(model, precision=precision)
    torch.manual_seed(7)
    w1 = torch.randn(ref.shape, device="cuda")
    w2 = torch.randn(ref.shape, device="cuda")
    x2 = (x + 1) % cfg.data.S

    def alone(step, xx, ww):
        tr.rng[1] = step
        return _grads(model, lambda: (tr(xx, t) * ww).sum().backward())[1]

    g1 = alone(20, x, w1)
    step2 = int(tr.rng[1])                                 # where the first forward left the trainer's step
    assert step2 > 20
    g2 = alone(step2, x2, w2)

    def both():
        tr.rng[1] = 20
        o1 = tr(x, t)
        assert int(tr.rng[1]) == step2
        o2 = tr(x2, t)                                     # before the first backward
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


def test_masked_train_matches_autograd_maze_size():
    """config_bert_mazemasked (D = 225, S = 3, E = 64, 4 layers, head dimension 8: T = 226, the generic attention kernels), batch 2
    = 450 sequences of 226 tokens, dropout 0, at the bars of test_bert_train_matches_autograd_maze_size (set for a deeper stack
    of the same blocks)."""
    from config.maze_config.config_bert_mazemasked import get_config
    from ctdd.masked_train import MaskedTrainer
    mu = _registries()[0]
    cfg = get_config()
    cfg.device = "cuda"
    cfg.model.update(dropout_rate=0.0, attention_dropout_rate=0.0)
    torch.manual_seed(0)
    model = mu.create_model(cfg, torch.device("cuda"))
    assert model.training
    x = torch.randint(0, 3, (2, 225), device="cuda")
    t = torch.tensor([0.3, 0.99], device="cuda")
    wgt = torch.randn((2, 225, 3), device="cuda")
    cfg.model.engine = "torch"
    out_ref, g_ref = _grads(model, lambda: _weighted(model, x, t, wgt))
    cfg.model.engine = "hip"
    scale = max(1.0, float(out_ref.abs().max()))
    out, g_hip = _grads(model, lambda: _weighted(MaskedTrainer(model, precision="fp32"), x, t, wgt))
    print(f"maze fp32: logits {float((out - out_ref).abs().max()) / scale:.3e} of the scale (bar 2e-4)")
    assert float((out - out_ref).abs().max()) < 2e-4 * scale
    print(f"maze fp32: worst gradient L2 error {_compare(g_hip, g_ref, 1e-2, l2=True):.3e} (bar 1e-2)")
    out_b, g_b = _grads(model, lambda: _weighted(MaskedTrainer(model, precision="bf16"), x, t, wgt))
    print(f"maze bf16: logits {float((out_b - out_ref).abs().max()) / scale:.3e} of the scale (bar 5e-2)")
    assert float((out_b - out_ref).abs().max()) < 5e-2 * scale
    print(f"maze bf16: worst gradient L2 error {_compare(g_b, g_ref, 0.1, l2=True):.3e} (bar 0.1)")


# ------------------------------------------------------------------------------------------------ loss, step, fallbacks
def test_masked_catrmnll_loss_matches_torch_and_steps_run():
    """One CatRMNLL calc_loss on config_masked_synthetic, batch 8, dropout 0, fp32 training precision: loss value and every
    parameter gradient of engine_train = "hip-masked" against "torch" under the same seeds (the bars of
    test_bert_ctelbo_loss_matches_torch); then two Standard.step calls at batch 6 with the config's own dropout."""
    _, lu, tu, ou = _registries()
    res = {}
    for engine_train in ("torch", "hip-masked"):
        cfg, model = _shipped("synthetic_config.config_masked_synthetic", dropout_rate=0.0, attention_dropout_rate=0.0,
                              engine_train=engine_train, engine_train_precision="fp32")
        loss_fn = lu.get_loss(cfg)
        x = torch.randint(0, cfg.data.S, (8, int(cfg.model.concat_dim)), device="cuda")
        torch.manual_seed(11)
        l = loss_fn.calc_loss(x, {"model": model, "n_iter": 0})
        for p in model.parameters():
            p.grad = None
        l.backward()
        res[engine_train] = (float(l.detach()), {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None})
        assert (model._trainer is not None) == (engine_train == "hip-masked")
    err = abs(res["hip-masked"][0] - res["torch"][0])
    print(f"CatRMNLL loss: torch {res['torch'][0]:.6e}, hip-masked {res['hip-masked'][0]:.6e}")
    assert err < 1e-4 * max(1.0, abs(res["torch"][0]))
    print(f"CatRMNLL gradients: worst error {_compare(res['hip-masked'][1], res['torch'][1], 2e-3):.3e} of the range (bar 2e-3)")
    from ctdd.masked_train import MaskedTrainer
    cfg, model = _shipped("synthetic_config.config_masked_synthetic", engine_train="hip-masked")
    assert cfg.model.dropout_rate > 0
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
    assert isinstance(model._trainer, MaskedTrainer)
    assert not [w for w in rec if issubclass(w.category, RuntimeWarning)], [str(w.message) for w in rec]


@pytest.mark.parametrize("case", ["mlp-readout", "x0-prediction"])
def test_hip_masked_falls_back_to_the_module_with_one_warning(golden, case):
    """engine_train = "hip-masked" on a masked model with the MLP readout and on an x0-prediction model: one RuntimeWarning, the
    steps run on the module, no trainer is built."""
    _, lu, tu, ou = _registries()
    if case == "mlp-readout":
        cfg, model, x, t, _ = tiny_model(golden, "mask_mlp", "cuda")
        cfg.model.engine_train = "hip-masked"
        model.train()
        D = x.shape[1]
    else:
        cfg, model = _shipped("synthetic_config.config_bert_synthetic", engine_train="hip-masked")
        D = int(cfg.model.concat_dim)
    from ctdd.masked_train import training_supported
    assert not training_supported(model)
    cfg.training.max_t = 0.99
    state = {"model": model, "optimizer": ou.get_optimizer(model.parameters(), cfg), "n_iter": 0}
    w0 = [p.detach().clone() for p in model.parameters()]
    mb = torch.randint(0, cfg.data.S, (6, D), device="cuda")
    loss, step = lu.get_loss(cfg), tu.get_train_step(cfg)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        for _ in range(2):
            out = step.step(state, loss, mb)
            state["n_iter"] += 1
    assert out.dim() == 0 and torch.isfinite(out)
    assert sum(int(not torch.equal(a, b)) for a, b in zip(w0, model.parameters())) > 0.5 * len(w0)
    assert model._trainer is None
    hits = [w for w in rec if issubclass(w.category, RuntimeWarning)]
    assert len(hits) == 1 and "HIP masked training kernels" in str(hits[0].message), [str(w.message) for w in rec]
