"""GPU: the x0-prediction ("BERT") and masked transformer score models on the HIP engine (ctdd/bert_engine.py): unmasked
attention (mode 3 of both attention kernels) and ctdd_bert_embed / ctdd_bert_gather through the C ABI, the engine against the
reference's golden logits (tests/golden/bert.npz) and against the fp32 module at the shipped sizes, weight updates, samplers,
training steps and the module fallback."""
import ctypes as C
import importlib
import warnings

import numpy as np
import pytest
import torch

from test_bert_cpu import tiny_model

pytestmark = pytest.mark.gpu


def _registries():
    import lib.models.models  # noqa: F401
    import lib.models.model_utils as mu
    import lib.sampling.sampling  # noqa: F401
    import lib.sampling.sampling_utils as su
    import lib.losses.losses  # noqa: F401
    import lib.losses.losses_utils as lu
    import lib.training.training  # noqa: F401
    import lib.training.training_utils as tu
    import lib.optimizers.optimizers  # noqa: F401
    import lib.optimizers.optimizers_utils as ou
    return mu, su, lu, tu, ou


def _shipped(mod, **model_over):
    mu = _registries()[0]
    cfg = importlib.import_module("config." + mod).get_config()
    cfg.device = "cuda"
    cfg.model.update(**model_over)
    torch.manual_seed(0)
    return cfg, mu.create_model(cfg, torch.device("cuda"))


# ------------------------------------------------------------------------------------------------ kernels through the C ABI
def _attn_args(q, k, v, B, Tq, Tk, H, hd, mode, split, out, out_hi, out_lo):
    from ctdd.hollow_engine import _AttnArgs
    E = H * hd
    a = _AttnArgs()
    a.split, a.out_lo = split, out_lo.data_ptr()
    a.q, a.k, a.v = q.data_ptr(), k.data_ptr(), v.data_ptr()
    a.q_bs, a.k_bs, a.v_bs, a.q_rs, a.k_rs, a.v_rs = Tq * E, Tk * E, Tk * E, E, E, E
    a.B, a.Tq, a.Tk, a.H, a.hd, a.mode, a.scale = B, Tq, Tk, H, hd, mode, 1.0 / hd ** 0.5
    a.out, a.out_rs, a.out_hi = out.data_ptr(), E, out_hi.data_ptr()
    return a


def _short():
    from ctdd.bert_engine import _lib
    return _lib().ctdd_bert_attention_short


@pytest.mark.parametrize("hd", [8, 16, 32, 64])
@pytest.mark.parametrize("Tq,Tk", [(197, 197), (33, 33), (226, 226), (40, 226), (64, 64), (5, 61)])
def test_unmasked_attention_against_fp64_softmax(hd, Tq, Tk):
    """Mode 3 of both attention kernels against an fp64 softmax over every key, N(0, 1) operands: fp32 FMA kernel 2e-5 (every head
    dimension), matrix-core kernel 2e-2 with bf16 operands and 5e-5 with hi / lo pairs (hd 16 / 32); hi + lo within 1e-4 of the fp32
    output.  Outputs start as NaN, so every element must be written."""
    from ctdd.hollow_engine import _lib
    lib = _lib()
    B, H = 3, 4
    E = H * hd
    g = torch.Generator(device="cuda").manual_seed(50 + hd + Tq)
    q = torch.randn(B, Tq, E, device="cuda", generator=g)
    k = torch.randn(B, Tk, E, device="cuda", generator=g)
    v = torch.randn(B, Tk, E, device="cuda", generator=g)
    qh, kh, vh = (z.view(B, -1, H, hd).transpose(1, 2).double() for z in (q, k, v))
    ref = (torch.softmax((qh @ kh.transpose(-1, -2)) / hd ** 0.5, -1) @ vh).transpose(1, 2).reshape(B, Tq, E).float()
    st = torch.cuda.current_stream().cuda_stream
    runs = [(lib.ctdd_hollow_attention, 2e-5, 0)]
    if hd in (16, 32):
        runs += [(lib.ctdd_hollow_attention_bf16, 2e-2, 0), (lib.ctdd_hollow_attention_bf16, 5e-5, 1)]
    if Tk <= 64 and hd <= 32:
        runs += [(_short(), 2e-5, 0)]                                     # the short-sequence kernel: fp32 arithmetic, fp32 bar
    for fn, tol, split in runs:
        out = torch.full((B, Tq, E), float("nan"), device="cuda")
        out_hi = torch.full((B, Tq, E), float("nan"), device="cuda", dtype=torch.bfloat16)
        out_lo = torch.full((B, Tq, E), float("nan"), device="cuda", dtype=torch.bfloat16)
        a = _attn_args(q, k, v, B, Tq, Tk, H, hd, 3, split, out, out_hi, out_lo)
        assert fn(C.byref(a), st) == 0
        torch.cuda.synchronize()
        err = (out - ref).abs().max().item()
        print(f"mode 3 {fn.__name__} split={split} hd={hd} {Tq}x{Tk}: max err {err:.3e} (bar {tol:g})")
        assert err < tol, fn                                              # (NaN fails the comparison)
        assert (out_hi.float() - ref).abs().max().item() < max(tol, 2e-2), fn
        assert (out_hi.float() + out_lo.float() - out).abs().max().item() < 1e-4


@pytest.mark.parametrize("mode", [-1, 4, 7])
def test_attention_refuses_unknown_modes_and_launches_nothing(mode):
    from ctdd.hollow_engine import _lib
    lib = _lib()
    B, H, hd, T = 2, 4, 16, 33
    E = H * hd
    q = torch.randn(B, T, E, device="cuda")
    for fn in (lib.ctdd_hollow_attention, lib.ctdd_hollow_attention_bf16):
        out = torch.full((B, T, E), float("nan"), device="cuda")
        hi = torch.full((B, T, E), float("nan"), device="cuda", dtype=torch.bfloat16)
        a = _attn_args(q, q, q, B, T, T, H, hd, mode, 0, out, hi, hi)
        assert fn(C.byref(a), torch.cuda.current_stream().cuda_stream) < 0
        torch.cuda.synchronize()
        assert torch.isnan(out).all() and torch.isnan(hi.float()).all()
    # the short-sequence entry point takes mode 3 up to 64 x 64 only
    for m_, tq, tk in ((mode, T, T), (3, T, 65), (3, 65, T), (0, T, T)):
        out = torch.full((B, tq, E), float("nan"), device="cuda")
        kk = torch.randn(B, tk, E, device="cuda")
        a = _attn_args(q if tq == T else kk, kk, kk, B, tq, tk, H, hd, m_, 0, out, hi, hi)
        assert _short()(C.byref(a), torch.cuda.current_stream().cuda_stream) < 0
        torch.cuda.synchronize()
        assert torch.isnan(out).all()
    # the masked modes still need their own shapes: causal attention with Tq != Tk is refused too
    out = torch.full((B, T, E), float("nan"), device="cuda")
    a = _attn_args(q, q, q, B, T, T - 1, H, hd, 0, 0, out, hi, hi)
    assert lib.ctdd_hollow_attention(C.byref(a), torch.cuda.current_stream().cuda_stream) < 0
    torch.cuda.synchronize()
    assert torch.isnan(out).all()


def _embed_reference(x, t, w, b, pe, S, scale, rows=None, r0=0, cond=0):
    """torch restatement of ctdd_bert_embed: (rows, D + 1, E); rows=None is the plain mode."""
    from lib.networks.hollow_networks import transformer_timestep_embedding
    B, D = x.shape
    temb = transformer_timestep_embedding(t * scale, w.numel())
    if rows is None:
        xb, tb = x, temb
    else:
        Dp = D - cond
        g = (r0 + torch.arange(rows, device=x.device)).clamp(max=B * Dp - 1)
        bi, p = g // Dp, cond + g % Dp
        xb, tb = x[bi].long().scatter(1, p[:, None], S), temb[bi]
    tok = ((xb.float() / (S - 1)) * 2 - 1)[:, :, None] * w[None, None, :] + b[None, None, :]
    return torch.cat([tb[:, None, :], tok], dim=1) + pe[None, : D + 1], temb


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
def test_bert_embed_plain_and_enumerate(dtype):
    """ctdd_bert_embed against a torch restatement at fp32 rounding: plain mode, and enumerate mode with a conditional prefix, a
    non-zero first sequence read from device memory and a chunk that runs past the last sequence."""
    from ctdd.bert_engine import _BertEmbedArgs, _lib
    from lib.networks.hollow_networks import PositionalEncoding
    lib = _lib()
    B, D, E, S, scale, cond = 5, 13, 32, 3, 1000.0, 3
    g = torch.Generator(device="cuda").manual_seed(9)
    x = torch.randint(0, S, (B, D), device="cuda", generator=g).to(dtype)
    t = torch.rand(B, device="cuda", generator=g)
    w, b = torch.randn(E, device="cuda", generator=g), torch.randn(E, device="cuda", generator=g)
    pe = PositionalEncoding("cuda", E, 0.0, D + 1).pe[0].contiguous()
    total = B * (D - cond)
    for rows, r0 in ((None, 0), (16, 0), (16, 37), (16, total - 9)):
        n = B if rows is None else rows
        out = torch.full((n, D + 1, E), float("nan"), device="cuda")
        temb = torch.full((B, E), float("nan"), device="cuda")
        r0_dev = torch.tensor([r0], dtype=torch.int32, device="cuda")
        a = _BertEmbedArgs()
        if dtype == torch.int64:
            a.x64 = x.data_ptr()
        else:
            a.x32 = x.data_ptr()
        a.t, a.w_in, a.b_in, a.pe = t.data_ptr(), w.data_ptr(), b.data_ptr(), pe.data_ptr()
        a.B, a.D, a.E, a.S, a.temb_scale, a.out, a.temb = B, D, E, S, scale, out.data_ptr(), temb.data_ptr()
        a.enumerate, a.cond, a.rows, a.r0 = int(rows is not None), 0 if rows is None else cond, n, r0_dev.data_ptr()
        assert lib.ctdd_bert_embed(C.byref(a), torch.cuda.current_stream().cuda_stream) == 0
        torch.cuda.synchronize()
        ref, temb_ref = _embed_reference(x, t, w, b, pe, S, scale, rows, r0, cond)
        # fp32 rounding: a few ulp of the O(1) token values; the time embedding's sin / cos arguments reach 1000, where one
        # ulp of the argument is 6e-5
        np.testing.assert_allclose(out[:, 1:].cpu().numpy(), ref[:, 1:].cpu().numpy(), rtol=0, atol=2e-6)
        np.testing.assert_allclose(out[:, 0].cpu().numpy(), ref[:, 0].cpu().numpy(), rtol=0, atol=5e-4)
        if rows is None:
            np.testing.assert_allclose(temb.cpu().numpy(), temb_ref.cpu().numpy(), rtol=0, atol=5e-4)
        else:                                             # temb rows of exactly the samples whose first free position is in the chunk
            gi = torch.arange(r0, min(r0 + rows, total))
            owners = set((gi[gi % (D - cond) == 0] // (D - cond)).tolist())
            if r0 + rows > total and (total - 1) % (D - cond) == 0:
                owners.add(B - 1)
            written = set(torch.nonzero(~torch.isnan(temb[:, 0])).view(-1).tolist())
            assert written == owners
            for bi in owners:
                np.testing.assert_allclose(temb[bi].cpu().numpy(), temb_ref[bi].cpu().numpy(), rtol=0, atol=5e-4)


def test_bert_gather_rows():
    from ctdd.bert_engine import _lib
    lib = _lib()
    B, D, E, cond, rows = 4, 9, 48, 2, 8
    Dp = D - cond
    total = B * Dp
    st = torch.cuda.current_stream().cuda_stream
    ptr = lambda z: None if z is None else z.data_ptr()
    # masked: chunk rows r0 .. r0 + rows - 1, the last chunk ragged
    out = torch.full((total, E), float("nan"), device="cuda")
    hi = torch.zeros((total, E), device="cuda", dtype=torch.bfloat16)
    lo = torch.zeros((total, E), device="cuda", dtype=torch.bfloat16)
    want = torch.empty((total, E), device="cuda")
    for r0 in range(0, total, rows):
        enc = torch.randn(rows, D + 1, E, device="cuda")
        r0_dev = torch.tensor([r0], dtype=torch.int32, device="cuda")
        assert lib.ctdd_bert_gather(ptr(enc), ptr(r0_dev), rows, 1, B, D, cond, E, ptr(out), ptr(hi), ptr(lo), st) == 0
        torch.cuda.synchronize()
        for r in range(min(rows, total - r0)):
            want[r0 + r] = enc[r, 1 + cond + (r0 + r) % Dp]
    assert total % rows != 0 and torch.equal(out, want)
    assert torch.equal(hi, want.to(torch.bfloat16)) and (hi.float() + lo.float() - want).abs().max().item() < 1e-4
    # plain: rows 1..D of every sequence
    enc = torch.randn(B, D + 1, E, device="cuda")
    out = torch.full((B * D, E), float("nan"), device="cuda")
    assert lib.ctdd_bert_gather(ptr(enc), None, B * D, 0, B, D, 0, E, ptr(out), None, None, st) == 0
    torch.cuda.synchronize()
    assert torch.equal(out.view(B, D, E), enc[:, 1:])


# ------------------------------------------------------------------------------------------------ engine
@pytest.mark.parametrize("tag", ["bert_a", "bert_b", "mask_a", "mask_c"])
def test_engine_matches_reference_golden(golden, tag):
    from ctdd.bert_engine import BertEngine, supports
    cfg, model, x, t, ref = tiny_model(golden, tag, "cuda")
    assert supports(model)
    if tag == "mask_a":
        cfg.model.enum_chunk = 7                                       # 36 sequences: six chunks, the last one ragged
    with torch.no_grad():
        for prec in ("fp32", "bf16x3"):
            eng = BertEngine(model, precision=prec)
            out = eng(x.long(), t).cpu().numpy()
            print(f"{tag} {prec}: max |engine - reference| = {np.abs(out - ref).max():.3e} (bar 1e-4), max |ref| = {np.abs(ref).max():.2f}")
            np.testing.assert_allclose(out, ref, rtol=0, atol=1e-4)
        via_model = model(x.long(), t).cpu().numpy()                    # eval / no_grad calls go to the default-precision engine
        np.testing.assert_array_equal(via_model, out)
        assert model._engine is not None and model._engine.precision == "bf16x3"
        # the captured plan on other inputs: against the module on the same weights (fp32 device ops)
        g = torch.Generator().manual_seed(8)
        x2 = torch.randint(0, cfg.data.S, tuple(x.shape), generator=g).cuda()
        t2 = torch.tensor([0.31, 0.77, 0.12], device="cuda")
        again = eng(x2, t2).cpu().numpy()
        cfg.model.engine = "torch"
        ref2 = model(x2, t2).cpu().numpy()
        cfg.model.engine = "hip"
        np.testing.assert_allclose(again, ref2, rtol=0, atol=1e-4)
        assert np.abs(ref2 - ref).max() > 1e-2
    if tag == "mask_c":
        assert (out[:, :4] == 0).all() and (again[:, :4] == 0).all()
    model.train()


@pytest.mark.parametrize("which", ["bert_maze", "bert_synthetic", "masked_synthetic"])
def test_engine_matches_module_at_shipped_sizes(which):
    """The three engine precisions against the fp32 module on torch device ops: fp32 and bf16x3 within 2e-4 max(1, max|ref|), bf16
    within 5e-2 max(1, max|ref|) (the hollow engine's bounds).  config_bert_maze at batch 5; config_masked_synthetic at batch 4
    (128 sequences) in chunks of 50: three chunks, the last one ragged."""
    from ctdd.bert_engine import BertEngine
    mod, B, over = {"bert_maze": ("maze_config.config_bert_maze", 5, {}), "bert_synthetic": ("synthetic_config.config_bert_synthetic", 6, {}),
                    "masked_synthetic": ("synthetic_config.config_masked_synthetic", 4, {"enum_chunk": 50})}[which]
    cfg, model = _shipped(mod, **over)
    model.eval()
    D, S = int(cfg.model.concat_dim), cfg.data.S
    x = torch.randint(0, S, (B, D), device="cuda")
    t = torch.linspace(0.02, 0.99, B, device="cuda")
    with torch.no_grad():
        cfg.model.engine = "torch"
        ref = model(x, t).cpu()
        cfg.model.engine = "hip"
        outs = {}
        for p in ("fp32", "bf16x3", "bf16"):
            eng = BertEngine(model, precision=p)
            outs[p] = eng(x, t).cpu()
            plan = eng._plans[(B, x.dtype)]
            if which == "masked_synthetic":
                assert plan.nchunks == 3
            # T = 33 runs the short-sequence attention kernel, T = 226 the generic mode-3 kernels
            assert any(s.label[0] == "ctdd_bert_attention_short" for s in plan.chunk_plan) == (D + 1 <= 64)
        if D + 1 <= 64:                                                 # the knob: the generic kernels on the same plan
            cfg.model.engine_attention_short = False
            eng = BertEngine(model, precision="bf16x3")
            outs["bf16x3 generic"] = eng(x, t).cpu()
            assert not any(s.label[0] == "ctdd_bert_attention_short" for s in eng._plans[(B, x.dtype)].chunk_plan)
            cfg.model.engine_attention_short = True
    scale = max(ref.abs().max().item(), 1.0)
    assert ref.shape == (B, D, S)
    for p, bar in (("fp32", 2e-4), ("bf16x3", 2e-4), ("bf16", 5e-2), ("bf16x3 generic", 2e-4)):
        if p not in outs:
            continue
        err = (outs[p] - ref).abs().max().item()
        print(f"{which} {p}: max |engine - module| = {err:.3e} (bar {bar * scale:.3e})")
        assert err < bar * scale, p
    model.train()


def test_engine_follows_weight_updates():
    """An optimizer step (raw-pointer writes) and the EMA swap of eval() / train() invalidate the cached plan."""
    mu, su, lu, tu, ou = _registries()
    from config.synthetic_config.config_bert_synthetic import get_config
    cfg = get_config()
    cfg.device = "cuda"
    cfg.optimizer.lr = 5e-2                                            # a visible step
    torch.manual_seed(0)
    model = mu.create_model(cfg, torch.device("cuda"))
    state = {"model": model, "optimizer": ou.get_optimizer(model.parameters(), cfg), "n_iter": 0}
    loss, step = lu.get_loss(cfg), tu.get_train_step(cfg)
    D, S = int(cfg.model.concat_dim), cfg.data.S
    x = torch.randint(0, S, (6, D), device="cuda")
    t = torch.rand(6, device="cuda") * 0.8 + 0.1

    def both():
        model.eval()
        with torch.no_grad():
            cfg.model.engine = "hip"
            eng = model(x, t).clone()
            cfg.model.engine = "torch"
            ref = model(x, t).clone()
            cfg.model.engine = "hip"
        model.train()
        return eng, ref

    e0, r0 = both()
    assert (e0 - r0).abs().max().item() < 2e-4 * max(r0.abs().max().item(), 1.0)
    mb = torch.randint(0, S, (16, D), device="cuda")
    for _ in range(3):
        step.step(state, loss, mb)
        state["n_iter"] += 1
    e1, r1 = both()
    assert (e1 - r1).abs().max().item() < 2e-4 * max(r1.abs().max().item(), 1.0)    # the engine sees the new (EMA) weights
    assert (r1 - r0).abs().max().item() > 1e-2 * max(r1.abs().max().item(), 1.0)    # ... which did change


# ------------------------------------------------------------------------------------------------ samplers, training, fallback
@pytest.mark.parametrize("case", ["bert_TauL", "bert_LBJF", "masked_LBJF"])
def test_samplers_run_and_reproduce(case):
    su = _registries()[1]
    family, name = case.split("_")
    cfg, model = _shipped("synthetic_config.config_" + ("bert_synthetic" if family == "bert" else "masked_synthetic"))
    cfg.sampler.name, cfg.sampler.num_steps = name, 6
    model.eval()
    N, D, S = 16, int(cfg.model.concat_dim), cfg.data.S
    outs = []
    for _ in range(2):
        smp = su.get_sampler(cfg)
        smp.seed = 123
        out = smp.sample(model, N)
        outs.append(np.asarray(out[0] if isinstance(out, tuple) else out))
    assert model._engine is not None and model._engine._plans          # the HIP engine ran the network
    assert outs[0].shape == (N, D) and outs[0].min() >= 0 and outs[0].max() < S
    assert np.array_equal(outs[0], outs[1])
    model.train()


def test_conditional_sampler_keeps_the_conditioner(golden):
    su = _registries()[1]
    cfg, model, x, _, _ = tiny_model(golden, "mask_c", "cuda")
    cfg.sampler.update(name="ConditionalTauLeaping", num_steps=6, condition_dim=int(cfg.model.conditional_dim))
    N, D, S = 8, x.shape[1], cfg.data.S
    cond = torch.randint(0, S, (N, 4), generator=torch.Generator().manual_seed(2))
    smp = su.get_sampler(cfg)
    smp.seed = 5
    out = smp.sample(model, N, cond)
    out = np.asarray(out[0] if isinstance(out, tuple) else out)
    assert out.shape == (N, D) and out.min() >= 0 and out.max() < S
    assert (out[:, :4] == cond.numpy()).all()
    assert model._engine is not None and model._engine._plans
    model.train()


@pytest.mark.parametrize("family", ["bert", "masked"])
def test_training_step_and_its_warning(family):
    """One Standard.step with the configured loss (CTElbo on the BERT model, CatRMNLL on the masked one) on the autograd module:
    finite loss, changed parameters; exactly one "bert-train" RuntimeWarning with engine_train = "hip", none with "torch"."""
    _, _, lu, tu, ou = _registries()
    mod = "synthetic_config.config_" + ("bert_synthetic" if family == "bert" else "masked_synthetic")
    for engine_train, expected in (("torch", 0), ("hip", 1)):
        cfg, model = _shipped(mod, engine_train=engine_train)
        assert cfg.loss.name == ("CTElbo" if family == "bert" else "CatRMNLL")
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
        hits = [w for w in rec if issubclass(w.category, RuntimeWarning) and "no HIP training kernels" in str(w.message)]
        assert len(hits) == expected, [str(w.message) for w in rec]


def test_mlp_readout_falls_back_to_the_module_with_one_warning(golden):
    from ctdd.bert_engine import supports
    cfg, model, x, t, ref = tiny_model(golden, "mask_mlp", "cuda")
    assert not supports(model)
    with warnings.catch_warnings(record=True) as rec, torch.no_grad():
        warnings.simplefilter("always")
        out = model(x, t).cpu().numpy()
        model(x, t)
    np.testing.assert_allclose(out, ref, rtol=0, atol=1e-4)
    assert model._engine is None
    hits = [w for w in rec if issubclass(w.category, RuntimeWarning) and "outside the HIP engine's coverage" in str(w.message)]
    assert len(hits) == 1
    model.train()
