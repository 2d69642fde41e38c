"""GPU: the sample-resident attention-block launch (csrc/unet_attn_kernels.hip, ctdd_unet_attention_block) against the three launches it
replaces (ctdd_unet_conv_patch into fp32 qkv -> ctdd_unet_attention -> ctdd_unet_conv_patch with the residual) and against torch fp64,
what it reads and writes outside its samples, its idempotence, its refusals, and the plans the engine builds with
cfg.model.attention_fused = 1 / 0.  The construction is that of tests/test_gpu_resblock_mid.py (helpers copied)."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

NEW, OLD = "ctdd_unet_attention_block", "ctdd_unet_attention"


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _block(B, H, Cn, heads, seed, qscale=1.0, tail=0):
    """Random bf16-valued inputs and parameters of one attention block at H x H behind its GroupNorm: `an` (the normalised input), `x`
    (the raw input: the residual), the [3 C][C] qkv and [C][C] proj matrices (proj non-zero: the module initialises it to zero), fp32
    biases.  tail: that many NaN samples behind the last one, in the same allocation as `an` and `x`."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    rn = lambda *s: torch.randn(s, device="cuda", generator=g)
    T = H * H
    d = {"B": B, "H": H, "T": T, "C": Cn, "heads": heads}
    for name in ("an", "x"):
        full = torch.full(((B + tail) * T, Cn), float("nan"), dtype=torch.bfloat16, device="cuda")
        full[:B * T] = rn(B * T, Cn).to(torch.bfloat16)
        d[name + "_full"], d[name] = full, full[:B * T]
    d["wq"] = (qscale * rn(3 * Cn, Cn) / Cn ** 0.5).to(torch.bfloat16)
    d["wp"] = (rn(Cn, Cn) / Cn ** 0.5).to(torch.bfloat16)
    d["bq"], d["bp"] = 0.1 * rn(3 * Cn), 0.1 * rn(Cn)
    return d


def _run_new(d, out, f32=0, T=None, Cn=None, heads=None):
    """One ctdd_unet_attention_block launch; T / Cn / heads override what the argument block says (the refusal cases: a refused call
    reads nothing)."""
    from ctdd import unet_engine as ue
    lib = ue._lib()
    d["wqp"], d["wpp"] = ue.pack_attention_weights(d["wq"]), ue.pack_attention_weights(d["wp"])      # (kept alive in d)
    a = ue._AttnBlockArgs()
    a.an_bf16, a.x_bf16, a.w_qkv, a.b_qkv = d["an"].data_ptr(), d["x"].data_ptr(), d["wqp"].data_ptr(), d["bq"].data_ptr()
    a.w_proj, a.b_proj, a.out_bf16 = d["wpp"].data_ptr(), d["bp"].data_ptr(), out.data_ptr()
    a.B, a.T, a.C, a.heads = d["B"], T or d["T"], Cn or d["C"], heads or d["heads"]
    return lib.ctdd_unet_attention_block(C.byref(a), f32, _stream())


def _run_unfused(d):
    """The three launches this block has without the kernel, each with the kernel and tiles _PlanBuilder.conv picks for it: the patch
    kernel where it takes the grid (>= 32 pixels per sample, or 16), 48-channel chunks and 96-column tiles for qkv once 128 x 96 tiles
    fill the chip, 64-channel chunks and 32-column tiles below that and for proj; the generic kernel (96-channel chunks, 32-column
    tiles) for the 5 x 5 grid, which the patch kernel does not take."""
    from ctdd import unet_engine as ue
    lib = ue._lib()
    B, H, T, Cn = d["B"], d["H"], d["T"], d["C"]
    M = B * T
    qkv = torch.empty((M, 3 * Cn), dtype=torch.float32, device="cuda")
    ao = torch.empty((M, Cn), dtype=torch.bfloat16, device="cuda")
    y = torch.empty((M, Cn), dtype=torch.bfloat16, device="cuda")

    def conv(src, w, bias, N, out_f32=None, out_hi=None, res=None):
        c = ue._ConvArgs()
        c.nseg = 1
        c.seg[0].hi, c.seg[0].C, c.seg[0].kind = src.data_ptr(), Cn, ue.SEG_1x1
        c.w_hi, c.B, c.H, c.W, c.Hin, c.Win, c.N, c.Ktot = w.data_ptr(), B, H, H, H, H, N, Cn
        c.bias = bias.data_ptr()
        if out_f32 is not None:
            c.out_f32 = out_f32.data_ptr()
        if out_hi is not None:
            c.out_hi = out_hi.data_ptr()
        if res is not None:
            c.res_bf16 = res.data_ptr()
        if T >= 32 or T == 16 or B == 1:
            small = -(-M // 128) * -(-N // 96) < 256
            bk, bnt = (64, 1) if small else (48, 3)
            assert lib.ctdd_unet_conv_patch(C.byref(c), bk, bnt, 32, _stream()) == 0, lib.ctdd_last_error()
        else:
            assert lib.ctdd_unet_conv(C.byref(c), 96, 1, 0, _stream()) == 0, lib.ctdd_last_error()

    conv(d["an"], d["wq"], d["bq"], 3 * Cn, out_f32=qkv)
    a = ue._AttnArgs()
    a.qkv, a.B, a.T, a.C, a.heads, a.out_hi = qkv.data_ptr(), B, T, Cn, d["heads"], ao.data_ptr()
    assert lib.ctdd_unet_attention(C.byref(a), _stream()) == 0, lib.ctdd_last_error()
    conv(ao, d["wp"], d["bp"], Cn, out_hi=y, res=d["x"])
    return y


def _fp64(d):
    """The block in torch fp64 from the same bf16-valued inputs, no intermediate rounding (unet.py:176-200: per-head channel order
    [q | k | v], q and k scaled by ch^-1/4, softmax over the keys)."""
    B, T, Cn, heads = d["B"], d["T"], d["C"], d["heads"]
    ch = Cn // heads
    qkv = d["an"].double() @ d["wq"].double().t() + d["bq"].double()
    h = qkv.view(B, T, heads, 3, ch).permute(0, 2, 3, 1, 4)
    q, k, v = h[:, :, 0], h[:, :, 1], h[:, :, 2]
    sc = ch ** -0.25
    w = torch.softmax(torch.einsum("bhtc,bhsc->bhts", q * sc, k * sc), dim=-1)
    ao = torch.einsum("bhts,bhsc->bhtc", w, v).permute(0, 2, 1, 3).reshape(B * T, Cn)
    return ao @ d["wp"].double().t() + d["bp"].double() + d["x"].double()


CASES = [  # (B, H, C, heads, scale of the qkv weights)
    (3, 7, 192, 8, 1.0),
    (130, 7, 192, 8, 1.0),        # more samples than one chain, a non-round batch
    (2, 8, 192, 8, 1.0),          # every tile full
    (2, 5, 192, 8, 1.0),          # pad tokens, T neither a multiple of 4 nor of 16
    (2, 6, 192, 8, 1.0),
    (3, 7, 192, 8, 4.0),          # peaked softmax: the max subtraction matters
]


@pytest.mark.parametrize("B,H,Cn,heads,qscale", CASES)
def test_attention_block_matches_replaced_launches_and_fp64(B, H, Cn, heads, qscale):
    """e_new = max|one launch - fp64| <= 1.5 e_old = max|three launches - fp64|: the same rounding points, so the two errors are draws
    from one distribution (the factor covers the fluctuation of a maximum); e_old itself under the project's bf16 bar."""
    from ctdd import unet_engine as ue
    d = _block(B, H, Cn, heads, seed=1000 * H + Cn + B + int(10 * qscale))
    ref = _fp64(d)
    old = _run_unfused(d).double()
    out = torch.full((B * H * H, Cn), float("nan"), dtype=torch.bfloat16, device="cuda")
    assert _run_new(d, out) == 0, ue._lib().ctdd_last_error()
    new = out.double()
    assert bool(torch.isfinite(new).all())
    e_old, e_new = float((old - ref).abs().max()), float((new - ref).abs().max())
    print(f"B={B} {H}x{H} C={Cn} heads={heads} qscale={qscale}: e_old={e_old:.4e} e_new={e_new:.4e} "
          f"max|new-old|={float((new - old).abs().max()):.4e} max|fp64|={float(ref.abs().max()):.3f}")
    assert e_old < 5e-2 * float(ref.abs().max())
    assert e_new <= 1.5 * e_old


@pytest.mark.parametrize("H", [7, 5])
def test_attention_block_stays_inside_its_samples(H):
    """NaN samples behind the last one in the allocations of `an` and `x`, one NaN sample behind the last output sample: the results
    are finite and equal to those without the tail, the extra output sample is untouched."""
    B, Cn = 5, 192
    T = H * H
    d = _block(B, H, Cn, 8, seed=77 + H, tail=2)
    assert bool(torch.isnan(d["an_full"][B * T:].float()).all()) and bool(torch.isnan(d["x_full"][B * T:].float()).all())
    out = torch.full(((B + 1) * T, Cn), float("nan"), dtype=torch.bfloat16, device="cuda")
    assert _run_new(d, out) == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out[:B * T].float()).all())
    assert bool(torch.isnan(out[B * T:].float()).all())
    ref = _fp64(d)
    assert float((out[:B * T].double() - ref).abs().max()) < 5e-2 * float(ref.abs().max())


def test_attention_block_idempotent_and_reproducible():
    B, H, Cn = 24, 7, 192
    d = _block(B, H, Cn, 8, seed=5)
    o1 = torch.full((B * H * H, Cn), 7.0, dtype=torch.bfloat16, device="cuda")
    o2 = torch.full((B * H * H, Cn), -3.0, dtype=torch.bfloat16, device="cuda")
    assert _run_new(d, o1) == 0
    first = o1.clone()
    assert _run_new(d, o1) == 0 and _run_new(d, o2) == 0
    torch.cuda.synchronize()
    assert torch.equal(first, o1) and torch.equal(o1, o2)
    assert bool(torch.isfinite(o1.float()).all())


def test_attention_block_refuses_what_it_cannot_hold():
    from ctdd import unet_engine as ue
    lib = ue._lib()
    d = _block(2, 7, 192, 8, seed=3)
    out = torch.full((2 * 81, 256), float("nan"), dtype=torch.bfloat16, device="cuda")
    assert _run_new(d, out, f32=1) != 0 and b"bf16" in lib.ctdd_last_error()
    assert _run_new(d, out, Cn=96) != 0 and b"C=96" in lib.ctdd_last_error()
    assert _run_new(d, out, heads=64) != 0 and b"multiple of 4" in lib.ctdd_last_error()      # head width 3
    assert _run_new(d, out, T=81) != 0 and b"T=81" in lib.ctdd_last_error()
    assert _run_new(d, out, Cn=256) != 0 and b"C=256" in lib.ctdd_last_error()                # (2, 4x4, 256, 8): CIFAR's mid block is not covered
    torch.cuda.synchronize()
    assert bool(torch.isnan(out.float()).all())
    cov = ue.attention_block_covers
    assert cov(49, 192, 8) and cov(64, 192, 8) and cov(25, 192, 8) and cov(1, 192, 8)
    assert not cov(81, 192, 8) and not cov(49, 96, 8) and not cov(49, 192, 64) and not cov(16, 256, 8) and not cov(49, 192, 4)


def _mnist(seed, **model_over):
    import lib.models.models  # noqa: F401
    import lib.models.model_utils as mu
    from config.mnist_config.config_tauUnet_mnist import get_config
    cfg = get_config()
    cfg.device = "cuda"
    cfg.model.update(model_over)
    torch.manual_seed(seed)
    model = mu.create_model(cfg, torch.device("cuda"))
    g = torch.Generator(device="cuda").manual_seed(seed + 1)
    with torch.no_grad():      # re-drawn (the stock initialisation zeroes proj_out and scales every conv2 and the output convolution by 1e-10)
        for name, p in model.named_parameters():
            if p.dim() > 1:
                p.copy_(torch.randn(p.shape, generator=g, device="cuda") / (p[0].numel() ** 0.5))
            elif name.endswith("bias"):
                p.copy_(0.1 * torch.randn(p.shape, generator=g, device="cuda"))
    model.init_ema()
    model.eval()
    return cfg, model


def _plan_fns(eng):
    steps = [s_ for v in eng._plans.values() for s_ in (v.plan if not isinstance(v, tuple) else v[1][0].plan)]
    return [s_.label for s_ in steps]


@pytest.mark.parametrize("B", [48, 256])
def test_plans_one_launch_vs_three(B):
    """attention_fused = 1: exactly one ctdd_unet_attention_block step in place of the qkv convolution, ctdd_unet_attention and the proj
    convolution (two steps fewer, its flops their sum, the GroupNorm launch before it kept, nothing else moved); 0: the plan of an
    engine that has no such launch to take, label for label.  Logits of both within the bf16 bar of the fp32 module and within 2e-2 of
    each other (batch 256: two 128-sample sub-batch plans, graph replay)."""
    from ctdd.unet_engine import UNetEngine
    cfg, model = _mnist(0)
    att = [m_ for m_ in model.net.modules() if hasattr(m_, "proj_out")]
    assert att and all(float(m_.proj_out.weight.detach().abs().max()) > 0 for m_ in att)     # the block contributes
    g = torch.Generator(device="cuda").manual_seed(11)
    x = torch.randint(0, 256, (B, 784), device="cuda", generator=g)
    t = torch.rand(B, device="cuda", generator=g) * 0.98 + 0.01
    with torch.no_grad():
        cfg.model.engine = "torch"
        want = torch.cat([model(x[i:i + 64], t[i:i + 64]) for i in range(0, B, 64)])
    assert getattr(cfg.model, "attention_fused", None) is None     # the default (on) is the engine's
    outs, labels, flops = {}, {}, {}
    for flag in (1, 0):
        cfg.model.attention_fused = flag
        eng = UNetEngine(model, precision="bf16")
        with torch.no_grad():
            outs[flag] = eng(x.view(B, 1, 28, 28), t).float().clone()
        labels[flag] = _plan_fns(eng)
        steps = [s_ for v in eng._plans.values() for s_ in (v.plan if not isinstance(v, tuple) else v[1][0].plan)]
        flops[flag] = [s_.flops for s_ in steps]
        assert (len(eng._plans) == 1 and isinstance(next(iter(eng._plans.values())), tuple)) == (B == 256)
    f1 = [lb[0] for lb in labels[1]]
    f0 = [lb[0] for lb in labels[0]]
    assert f1.count(NEW) == 1 and f1.count(OLD) == 0 and f0.count(NEW) == 0 and f0.count(OLD) == 1
    assert f0.count("ctdd_unet_conv_patch") == f1.count("ctdd_unet_conv_patch") + 2
    assert f0.count("ctdd_unet_gn_onepass") == f1.count("ctdd_unet_gn_onepass") >= 1
    assert len(f1) == len(f0) - 2
    i1, i0 = f1.index(NEW), f0.index(OLD)
    assert i0 == i1 + 1 and f0[i0 - 1] == f0[i0 + 1] == "ctdd_unet_conv_patch" and f1[i1 - 1] == f0[i0 - 2] == "ctdd_unet_gn_onepass"
    assert "7x7" in labels[1][i1][1]
    assert labels[1][:i1] + labels[1][i1 + 1:] == labels[0][:i0 - 1] + labels[0][i0 + 2:]          # nothing else moved
    assert flops[1][i1] == flops[0][i0 - 1] + flops[0][i0 + 1] > 0 and sum(flops[1]) == sum(flops[0])
    scale = float(want.abs().max())
    assert scale > 0.5
    e1, e0, e10 = (float((outs[1] - want).abs().max()), float((outs[0] - want).abs().max()), float((outs[1] - outs[0]).abs().max()))
    print(f"B={B}: scale={scale:.3f} one-launch-module={e1:.4e} three-launch-module={e0:.4e} one-three={e10:.4e}")
    assert e1 < 5e-2 * scale and e0 < 5e-2 * scale
    assert e10 < 2e-2 * scale
    assert bool(torch.isfinite(outs[1]).all())
    if B == 48:     # plans alone (nothing launched): the knob at 0 = an engine that has no such launch to take, label for label; the fp32
        #             engine and a training plan never take it
        from ctdd import unet_train
        del cfg.model.attention_fused
        eng = UNetEngine(model, precision="bf16")
        eng._fuses_attention = lambda *a_, **k_: False
        assert [s_.label for s_ in eng._build(B, torch.int64, None).plan] == labels[0]
        e32 = UNetEngine(model, precision="fp32")
        assert all(s_.label[0] != NEW for s_ in e32._build(4, torch.int64, None).plan)
        unet_train.lib()
        etr = UNetEngine(model, precision="bf16")
        st = etr._build(64, torch.int64, None, tc=unet_train.TrainCtx(etr, 64, True))
        assert all(s_.label[0] != NEW for s_ in st.plan) and any(s_.label[0] == OLD for s_ in st.plan)
