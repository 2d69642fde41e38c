"""GPU: the sample-resident fused ResBlock launch of the 14x14 level (csrc/unet_resblock_kernels.hip, ctdd_unet_resblock_mid)
against the four launches it replaces (ctdd_unet_gn_onepass -> ctdd_unet_conv_patch, twice) and against torch fp64, its
idempotence, its refusals, and the plans the engine builds with cfg.model.resblock_fused_mid = 1 / 0.  The construction is that of
tests/test_gpu_resblock_fused.py (helpers copied)."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

N = 192


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _block(B, H, C1, C2, tb_rows, affine, seed):
    """Random bf16-valued inputs and parameters of one ResBlock at H x H (NHWC sources, [N][K] weights, K = segment -> tap -> channel)."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    rn = lambda *s: torch.randn(s, device="cuda", generator=g)
    Ct, skip = C1 + C2, C2 > 0 or C1 != N
    d = {"B": B, "H": H, "C1": C1, "C2": C2, "skip": skip}
    d["x1"] = rn(B * H * H, C1).to(torch.bfloat16)
    d["x2"] = rn(B * H * H, C2).to(torch.bfloat16) if C2 else None
    d["g1"], d["be1"] = (1.0 + 0.3 * rn(Ct), 0.3 * rn(Ct)) if affine else (torch.ones(Ct, device="cuda"), torch.zeros(Ct, device="cuda"))
    d["g2"], d["be2"] = (1.0 + 0.3 * rn(N), 0.3 * rn(N)) if affine else (torch.ones(N, device="cuda"), torch.zeros(N, device="cuda"))
    d["w1"] = (rn(N, 9 * Ct) / (9 * Ct) ** 0.5).to(torch.bfloat16)
    K2 = 9 * N + (Ct if skip else 0)
    d["w2"] = (rn(N, K2) / K2 ** 0.5).to(torch.bfloat16)
    d["b1"], d["b2"] = 0.1 * rn(N), 0.1 * rn(N)
    d["tb"] = 0.5 * rn(tb_rows, N)                     # one row (stride 0) or a row per sample
    d["tb_stride"] = 0 if tb_rows == 1 else N
    return d


def _run_mid(d, out, f32=0, H=None, n=N, G1=32, C1=None, C2=None):
    """One ctdd_unet_resblock_mid launch; H / n / G1 / C1 / C2 override what the argument block says (the refusal cases: the weights
    are packed for the block's own shape, which a refused call never reads)."""
    from ctdd import unet_engine as ue
    lib = ue._lib()
    a = ue._ResblockArgs()
    a.s1_bf16, a.C1 = d["x1"].data_ptr(), d["C1"] if C1 is None else C1
    if d["x2"] is not None:
        a.s2_bf16, a.C2 = d["x2"].data_ptr(), d["C2"] if C2 is None else C2
    a.gamma1, a.beta1, a.gamma2, a.beta2 = d["g1"].data_ptr(), d["be1"].data_ptr(), d["g2"].data_ptr(), d["be2"].data_ptr()
    a.G1, a.G2, a.eps1, a.eps2 = G1, 32, 1e-5, 1e-5
    cs = [d["C1"]] + ([d["C2"]] if d["C2"] else [])
    d["w1p"], d["w2p"] = ue.pack_resblock_mid_weights(d["w1"], d["w2"], cs)      # (kept alive in d)
    a.w1, a.bias1, a.tbias, a.tb_stride = d["w1p"].data_ptr(), d["b1"].data_ptr(), d["tb"].data_ptr(), d["tb_stride"]
    a.w2, a.bias2, a.skip = d["w2p"].data_ptr(), d["b2"].data_ptr(), int(d["skip"])
    a.B, a.H, a.W, a.N, a.out_bf16 = d["B"], H or d["H"], H or d["H"], n, out.data_ptr()
    return lib.ctdd_unet_resblock_mid(C.byref(a), f32, _stream())


def _run_unfused(d):
    """The four launches this block has without the kernel: one-pass GroupNorm + Swish, patch convolution (the 14x14 level's
    48-channel chunks, 96-column tiles), twice."""
    from ctdd import unet_engine as ue
    lib = ue._lib()
    B, H, C1, C2 = d["B"], d["H"], d["C1"], d["C2"]
    Ct, M = C1 + C2, B * H * H
    a1 = torch.empty((M, Ct), dtype=torch.bfloat16, device="cuda")
    h = torch.empty((M, N), dtype=torch.bfloat16, device="cuda")
    a2 = torch.empty((M, N), dtype=torch.bfloat16, device="cuda")
    y = torch.empty((M, N), dtype=torch.bfloat16, device="cuda")

    def gn(s1, c1, s2, c2, gamma, beta, out):
        g = ue._GnArgs()
        g.s1_bf16, g.C1 = s1.data_ptr(), c1
        if s2 is not None:
            g.s2_bf16, g.C2 = s2.data_ptr(), c2
        g.gamma, g.beta, g.B, g.HW, g.G, g.eps, g.swish, g.out_hi = gamma.data_ptr(), beta.data_ptr(), B, H * H, 32, 1e-5, 1, out.data_ptr()
        assert lib.ctdd_unet_gn_onepass(C.byref(g), 0, 512, _stream()) == 0, lib.ctdd_last_error()

    def conv(segs, w, bias, out, tb=None, res=None):
        c = ue._ConvArgs()
        c.nseg = len(segs)
        for i, (src, cs, kind) in enumerate(segs):
            c.seg[i].hi, c.seg[i].C, c.seg[i].kind = src.data_ptr(), cs, kind
        c.w_hi, c.B, c.H, c.W, c.Hin, c.Win, c.N, c.Ktot = w.data_ptr(), B, H, H, H, H, N, w.shape[1]
        c.bias, c.out_hi = bias.data_ptr(), out.data_ptr()
        if tb is not None:
            c.tbias, c.tb_stride = tb.data_ptr(), d["tb_stride"]
        if res is not None:
            c.res_bf16 = res.data_ptr()
        assert lib.ctdd_unet_conv_patch(C.byref(c), 48, 3, 64, _stream()) == 0, lib.ctdd_last_error()

    gn(d["x1"], C1, d["x2"], C2, d["g1"], d["be1"], a1)
    conv([(a1, Ct, ue.SEG_3x3)], d["w1"], d["b1"], h, tb=d["tb"])
    gn(h, N, None, 0, d["g2"], d["be2"], a2)
    segs = [(a2, N, ue.SEG_3x3)]
    if d["skip"]:
        segs.append((d["x1"], C1, ue.SEG_1x1))
        if C2:
            segs.append((d["x2"], C2, ue.SEG_1x1))
    conv(segs, d["w2"], d["b2"], y, res=None if d["skip"] else d["x1"])
    return y


def _fp64(d):
    """The block in torch fp64 from the same bf16-valued inputs, no intermediate rounding."""
    import torch.nn.functional as F
    B, H, C1, C2 = d["B"], d["H"], d["C1"], d["C2"]
    Ct = C1 + C2
    x = d["x1"].double() if d["x2"] is None else torch.cat([d["x1"].double(), d["x2"].double()], 1)
    x = x.view(B, H, H, Ct).permute(0, 3, 1, 2)
    w4 = lambda w, c: w.double().view(N, 3, 3, c).permute(0, 3, 1, 2)
    a1 = F.silu(F.group_norm(x, 32, d["g1"].double(), d["be1"].double(), 1e-5))
    tb = d["tb"].double().expand(B, N) if d["tb"].shape[0] == 1 else d["tb"].double()
    h = F.conv2d(a1, w4(d["w1"], Ct), d["b1"].double(), padding=1) + tb[:, :, None, None]
    a2 = F.silu(F.group_norm(h, 32, d["g2"].double(), d["be2"].double(), 1e-5))
    y = F.conv2d(a2, w4(d["w2"][:, :9 * N], N), d["b2"].double(), padding=1)
    y = y + (F.conv2d(x, d["w2"][:, 9 * N:].double().view(N, Ct, 1, 1)) if d["skip"] else x)
    return y.permute(0, 2, 3, 1).reshape(B * H * H, N)


CASES = [  # (B, H, C1, C2, time-bias rows (1: stride 0), affine)
    (3, 14, 192, 0, 1, False),          # residual
    (3, 14, 192, 192, 3, True),         # two sources, skip
    (3, 14, 192, 96, 1, True),          # groups straddle the sources (288 / 32 = 9 channels), padded source
    (3, 14, 96, 0, 3, False),           # single padded source with skip
    (2, 13, 192, 192, 1, False),        # odd width, partial last tile
    (2, 12, 192, 0, 1, True),           # whole pixel tiles unused
    (130, 14, 192, 192, 130, False),    # more workgroups than half the chip, per-sample time bias
]


@pytest.mark.parametrize("B,H,C1,C2,tb_rows,affine", CASES)
def test_mid_block_matches_replaced_launches_and_fp64(B, H, C1, C2, tb_rows, affine):
    """e_new = max|fused - fp64| <= 1.5 e_old = max|four launches - fp64|: the same rounding points, so the two errors are draws
    from one distribution (the factor covers the fluctuation of a maximum); e_old itself under the project's bf16 bar."""
    d = _block(B, H, C1, C2, tb_rows, affine, seed=1000 * H + C1 + C2 + B + tb_rows)
    ref = _fp64(d)
    old = _run_unfused(d).double()
    out = torch.empty((B * H * H, N), dtype=torch.bfloat16, device="cuda")
    from ctdd import unet_engine as ue
    assert _run_mid(d, out) == 0, ue._lib().ctdd_last_error()
    new = out.double()
    e_old, e_new = float((old - ref).abs().max()), float((new - ref).abs().max())
    print(f"B={B} {H}x{H} C={C1}+{C2} tb_rows={tb_rows} affine={affine}: e_old={e_old:.4e} e_new={e_new:.4e} "
          f"max|fused-unfused|={float((new - old).abs().max()):.4e} max|fp64|={float(ref.abs().max()):.3f}")
    assert e_old < 5e-2 * float(ref.abs().max())
    assert e_new <= 1.5 * e_old


@pytest.mark.parametrize("C2", [0, 96])
def test_mid_block_idempotent_and_reproducible(C2):
    B = 24
    d = _block(B, 14, 192, C2, 1, True, seed=5 + C2)
    M = B * 196
    o1 = torch.full((M, N), 7.0, dtype=torch.bfloat16, device="cuda")
    o2 = torch.full((M, N), -3.0, dtype=torch.bfloat16, device="cuda")
    assert _run_mid(d, o1) == 0
    first = o1.clone()
    assert _run_mid(d, o1) == 0 and _run_mid(d, o2) == 0
    torch.cuda.synchronize()
    assert torch.equal(first, o1) and torch.equal(o1, o2)
    assert bool(torch.isfinite(o1.float()).all())


def test_mid_block_refuses_what_it_cannot_hold():
    from ctdd import unet_engine as ue
    lib = ue._lib()
    d = _block(1, 14, 192, 0, 1, False, seed=3)
    d2 = _block(1, 14, 192, 192, 1, False, seed=4)
    out = torch.full((4 * 196, N), 5.0, dtype=torch.bfloat16, device="cuda")
    assert _run_mid(d, out, H=28) != 0 and b"28x28" in lib.ctdd_last_error()
    assert _run_mid(d, out, H=15) != 0 and b"15x15" in lib.ctdd_last_error()            # 225 pixels > 208
    assert _run_mid(d, out, f32=1) != 0 and b"bf16" in lib.ctdd_last_error()
    assert _run_mid(d, out, n=96) != 0                                                   # N != 192
    assert _run_mid(d2, out, C2=48) != 0                                                 # a 48-channel source
    assert _run_mid(d2, out, C1=256) != 0                                                # a source over 192 channels
    assert _run_mid(d, out, G1=5) != 0 and b"groups" in lib.ctdd_last_error()            # 192 % 5 != 0
    torch.cuda.synchronize()
    assert bool((out == 5.0).all())
    cov = ue.resblock_mid_covers
    assert not cov(28, 28, [192], N, 32, 32) and not cov(15, 15, [192], N, 32, 32) and not cov(14, 14, [192], 96, 32, 32)
    assert not cov(14, 14, [192, 48], N, 32, 32) and not cov(14, 14, [256, 192], N, 32, 32) and not cov(14, 14, [192], N, 5, 32)
    assert cov(14, 14, [192], N, 32, 32) and cov(14, 14, [192, 96], N, 32, 32) and cov(14, 14, [96], N, 32, 32) and cov(13, 13, [192, 192], N, 32, 32)


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
    with torch.no_grad():      # re-drawn (the stock initialisation scales every conv2 and the output convolution by 1e-10)
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
def test_plans_mid_vs_four_launches(B):
    """resblock_fused_mid = 1: exactly 5 ctdd_unet_resblock_mid steps (the 14x14 level) and 15 fewer steps in all; 0: the plan of a
    configuration without the knob, label for label.  Logits of both within the bf16 bar of the fp32 module and within 2e-2 of each
    other (batch 256: two 128-sample sub-batch plans, graph replay)."""
    from ctdd.unet_engine import UNetEngine
    cfg, model = _mnist(0)
    g = torch.Generator(device="cuda").manual_seed(11)
    x = torch.randint(0, 256, (B, 784), device="cuda", generator=g)
    t = torch.rand(B, device="cuda", generator=g) * 0.98 + 0.01
    with torch.no_grad():
        cfg.model.engine = "torch"
        want = torch.cat([model(x[i:i + 64], t[i:i + 64]) for i in range(0, B, 64)])
    assert getattr(cfg.model, "resblock_fused_mid", None) is None     # the default (on) is the engine's
    outs, labels = {}, {}
    for flag in (1, 0):
        cfg.model.resblock_fused_mid = flag
        eng = UNetEngine(model, precision="bf16")
        with torch.no_grad():
            outs[flag] = eng(x.view(B, 1, 28, 28), t).float().clone()
        labels[flag] = _plan_fns(eng)
        assert (len(eng._plans) == 1 and isinstance(next(iter(eng._plans.values())), tuple)) == (B == 256)
    f1 = [lb[0] for lb in labels[1]]
    f0 = [lb[0] for lb in labels[0]]
    assert f1.count("ctdd_unet_resblock_mid") == 5 and f0.count("ctdd_unet_resblock_mid") == 0
    assert len(f1) == len(f0) - 15
    assert all("14x14" in lb[1] for lb in labels[1] if lb[0] == "ctdd_unet_resblock_mid")
    assert f0.count("ctdd_unet_gn_onepass") == f1.count("ctdd_unet_gn_onepass") + 10
    assert f0.count("ctdd_unet_resblock_small") == f1.count("ctdd_unet_resblock_small") == 7
    scale = float(want.abs().max())
    assert scale > 0.5
    e1, e0, e10 = (float((outs[1] - want).abs().max()), float((outs[0] - want).abs().max()), float((outs[1] - outs[0]).abs().max()))
    print(f"B={B}: scale={scale:.3f} mid-module={e1:.4e} four-launch-module={e0:.4e} mid-four-launch={e10:.4e}")
    assert e1 < 5e-2 * scale and e0 < 5e-2 * scale
    assert e10 < 2e-2 * scale
    assert bool(torch.isfinite(outs[1]).all())
    if B == 48:     # plans alone (nothing launched): the knob at 0 = an engine that has no such launch to take, label for label, and
        #             the fp32 engine never takes it
        del cfg.model.resblock_fused_mid
        eng = UNetEngine(model, precision="bf16")
        eng._fuses_resblock_mid = lambda *a_, **k_: False
        assert [s_.label for s_ in eng._build(B, torch.int64, None).plan] == labels[0]
        e32 = UNetEngine(model, precision="fp32")
        assert all(s_.label[0] != "ctdd_unet_resblock_mid" for s_ in e32._build(4, torch.int64, None).plan)
