"""GPU: GroupNorm + Swish + 3x3 convolution of the 28x28 level in one launch (csrc/unet_rows_kernels.hip, ctdd_unet_conv_rows) against
the pair it replaces (ctdd_unet_gn_apply -> ctdd_unet_conv_ring bnt 3, or ctdd_unet_conv_patch 48/3/64 with 1x1 segments) and against
torch fp64, its output statistics, its reproducibility, its refusals, and the plans the engine builds with cfg.model.conv_rows = 1 / 0.
The construction is that of tests/test_gpu_resblock_mid.py: bf16-valued random inputs; the input statistics are computed in torch
fp64 and handed to both paths."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

N = 96


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _case(B, H, W, cs, rcs, res, tb_rows, seed):
    """Random bf16-valued inputs and parameters of one GroupNorm + convolution pair (NHWC sources, [N][K] weights, K = the 3x3 segment
    as tap -> channel of the concatenation, then the 1x1 segments)."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    rn = lambda *s: torch.randn(s, device="cuda", generator=g)
    M, Ct, Rt = B * H * W, sum(cs), sum(rcs)
    d = {"B": B, "H": H, "W": W, "cs": cs, "rcs": rcs}
    d["x"] = [rn(M, c).to(torch.bfloat16) for c in cs]
    d["r"] = [rn(M, c).to(torch.bfloat16) for c in rcs]
    d["res"] = rn(M, N).to(torch.bfloat16) if res else None
    d["gamma"], d["beta"] = 1.0 + 0.3 * rn(Ct), 0.3 * rn(Ct)
    K = 9 * Ct + Rt
    d["w"] = (rn(N, K) / K ** 0.5).to(torch.bfloat16)
    d["bias"] = 0.1 * rn(N)
    d["tb"] = 0.5 * rn(tb_rows, N) if tb_rows else None               # one row (stride 0) or a row per sample
    d["tb_stride"] = 0 if tb_rows == 1 else N
    d["st"] = []
    for x in d["x"]:
        xd = x.double().view(B, H * W, -1)
        d["st"].append(torch.stack([xd.sum(1), (xd * xd).sum(1)], -1).contiguous())      # [B][C][2]
    return d


def _run_rows(d, out, stats=None, f32=0, **over):
    """One ctdd_unet_conv_rows launch; `over` overrides fields of the argument block (the refusal cases)."""
    from ctdd import unet_engine as ue
    lib = ue._lib()
    a = ue._ConvRowsArgs()
    for i, (x, st) in enumerate(zip(d["x"], d["st"])):
        setattr(a, f"s{i + 1}_bf16", x.data_ptr()); setattr(a, f"st{i + 1}", st.data_ptr()); setattr(a, f"C{i + 1}", x.shape[1])
    for i, r in enumerate(d["r"]):
        setattr(a, f"r{i + 1}_bf16", r.data_ptr()); setattr(a, f"RC{i + 1}", r.shape[1])
    a.gamma, a.beta, a.G, a.eps = d["gamma"].data_ptr(), d["beta"].data_ptr(), 32, 1e-5
    if "wp" not in d:
        d["wp"] = ue.pack_conv_rows_weights(d["w"], d["cs"], d["rcs"])           # (kept alive in d)
    a.w, a.bias = d["wp"].data_ptr(), d["bias"].data_ptr()
    if d["tb"] is not None:
        a.tbias, a.tb_stride = d["tb"].data_ptr(), d["tb_stride"]
    if d["res"] is not None:
        a.res_bf16 = d["res"].data_ptr()
    a.out_bf16 = out.data_ptr()
    if stats is not None:
        a.out_stats = stats.data_ptr()
    a.B, a.H, a.W, a.N = d["B"], d["H"], d["W"], N
    for k, v in over.items():
        setattr(a, k, v)
    return lib.ctdd_unet_conv_rows(C.byref(a), f32, _stream())


def _run_pair(d):
    """The two launches the kernel replaces: ctdd_unet_gn_apply from the same statistics, then the ring convolution (bnt 3), or the patch
    convolution (48-channel chunks, 96-column tiles, 64 rows per wave) when there are 1x1 segments."""
    from ctdd import unet_engine as ue
    lib = ue._lib()
    B, H, W, cs = d["B"], d["H"], d["W"], d["cs"]
    M, Ct = B * H * W, sum(cs)
    act = torch.empty((M, Ct), dtype=torch.bfloat16, device="cuda")
    y = torch.empty((M, N), dtype=torch.bfloat16, device="cuda")
    g = ue._GnArgs()
    g.s1_bf16, g.st1, g.C1 = d["x"][0].data_ptr(), d["st"][0].data_ptr(), cs[0]
    if len(cs) == 2:
        g.s2_bf16, g.st2, g.C2 = d["x"][1].data_ptr(), d["st"][1].data_ptr(), cs[1]
    g.gamma, g.beta, g.B, g.HW, g.G, g.eps, g.swish, g.out_hi = d["gamma"].data_ptr(), d["beta"].data_ptr(), B, H * W, 32, 1e-5, 1, act.data_ptr()
    assert lib.ctdd_unet_gn_apply(C.byref(g), _stream()) == 0, lib.ctdd_last_error()
    c = ue._ConvArgs()
    segs = [(act, Ct, ue.SEG_3x3)] + [(r, r.shape[1], ue.SEG_1x1) for r in d["r"]]
    c.nseg = len(segs)
    for i, (src, n_, kind) in enumerate(segs):
        c.seg[i].hi, c.seg[i].C, c.seg[i].kind = src.data_ptr(), n_, kind
    c.w_hi, c.B, c.H, c.W, c.Hin, c.Win, c.N, c.Ktot = d["w"].data_ptr(), B, H, W, H, W, N, d["w"].shape[1]
    c.bias, c.out_hi = d["bias"].data_ptr(), y.data_ptr()
    if d["tb"] is not None:
        c.tbias, c.tb_stride = d["tb"].data_ptr(), d["tb_stride"]
    if d["res"] is not None:
        c.res_bf16 = d["res"].data_ptr()
    if d["r"]:
        assert lib.ctdd_unet_conv_patch(C.byref(c), 48, 3, 64, _stream()) == 0, lib.ctdd_last_error()
    else:
        assert lib.ctdd_unet_conv_ring(C.byref(c), 3, _stream()) == 0, lib.ctdd_last_error()
    return y


def _fp64(d):
    """The pair in torch fp64 from the same bf16-valued inputs, no intermediate rounding."""
    import torch.nn.functional as F
    B, H, W, cs, rcs = d["B"], d["H"], d["W"], d["cs"], d["rcs"]
    Ct, Rt = sum(cs), sum(rcs)
    nchw = lambda ts: torch.cat([t_.double() for t_ in ts], 1).view(B, H, W, -1).permute(0, 3, 1, 2)
    a = F.silu(F.group_norm(nchw(d["x"]), 32, d["gamma"].double(), d["beta"].double(), 1e-5))
    y = F.conv2d(a, d["w"][:, :9 * Ct].double().view(N, 3, 3, Ct).permute(0, 3, 1, 2), d["bias"].double(), padding=1)
    if Rt:
        y = y + F.conv2d(nchw(d["r"]), d["w"][:, 9 * Ct:].double().view(N, Rt, 1, 1))
    if d["tb"] is not None:
        y = y + (d["tb"].double().expand(B, N) if d["tb"].shape[0] == 1 else d["tb"].double())[:, :, None, None]
    y = y.permute(0, 2, 3, 1).reshape(B * H * W, N)
    return y + d["res"].double() if d["res"] is not None else y


CASES = [  # (B, H, W, GroupNorm sources, raw 1x1 sources, residual, time-bias rows (0: none, 1: stride 0))
    (3, 28, 28, [96], [], True, 0),             # conv2 of a down block
    (3, 28, 28, [96], [], False, 3),            # conv1 of a down block, per-sample time bias
    (3, 28, 28, [192, 96], [], False, 1),       # groups of 9 straddle the sources, three pieces, stride-0 time bias
    (3, 28, 28, [96, 96], [], False, 1),
    (3, 28, 28, [96], [96, 96], False, 0),      # conv2 + skip of an up block
    (2, 28, 28, [96], [192, 96], False, 0),
    (2, 15, 17, [96], [], True, 1),             # a second band of one row, a second column half of two pixels
    (2, 27, 27, [96, 96], [], False, 2),
    (2, 14, 28, [96], [], False, 1),            # one band
    (130, 28, 28, [96], [], False, 130),        # more workgroups than CUs, per-sample time bias
]


@pytest.mark.parametrize("B,H,W,cs,rcs,res,tb_rows", CASES)
def test_rows_matches_replaced_pair_and_fp64(B, H, W, cs, rcs, res, tb_rows):
    """e_new = max|rows - fp64| <= 1.5 e_old = max|pair - fp64|: the same rounding points, so the two errors are draws from one
    distribution (the bars of tests/test_gpu_resblock_mid.py); e_old itself under the project's bf16 bar.  Output statistics: the sum
    per (sample, channel) within HW 2^-9 max|out| of the fp64 sum of the bf16 output, the sum of squares within HW 2^-8 max|out|^2 (the
    most per-element bf16 rounding can move them).  Sentinel rows after the output stay untouched."""
    from ctdd import unet_engine as ue
    d = _case(B, H, W, cs, rcs, res, tb_rows, seed=1000 * H + 10 * W + sum(cs) + sum(rcs) + B + tb_rows)
    M, HW = B * H * W, H * W
    ref = _fp64(d)
    old = _run_pair(d).double()
    buf = torch.full((M + 64, N), 9.0, dtype=torch.bfloat16, device="cuda")
    stats = torch.zeros((B, N, 2), dtype=torch.float64, device="cuda")
    assert _run_rows(d, buf, stats) == 0, ue._lib().ctdd_last_error()
    new = buf[:M].double()
    assert bool((buf[M:] == 9.0).all())
    e_old, e_new, top = float((old - ref).abs().max()), float((new - ref).abs().max()), float(ref.abs().max())
    print(f"B={B} {H}x{W} C={cs} raw={rcs} res={res} tb_rows={tb_rows}: e_old={e_old:.4e} e_new={e_new:.4e} "
          f"max|rows-pair|={float((new - old).abs().max()):.4e} max|fp64|={top:.3f}")
    assert e_old < 5e-2 * top
    assert e_new <= 1.5 * e_old
    nv = new.view(B, HW, N)
    omax = float(new.abs().max())
    ds, dq = float((stats[:, :, 0] - nv.sum(1)).abs().max()), float((stats[:, :, 1] - (nv * nv).sum(1)).abs().max())
    print(f"    statistics: |sum - fp64| = {ds:.4e} (bar {HW * 2.0 ** -9 * omax:.4e}), |sumsq - fp64| = {dq:.4e} (bar {HW * 2.0 ** -8 * omax ** 2:.4e})")
    assert ds <= HW * 2.0 ** -9 * omax and dq <= HW * 2.0 ** -8 * omax ** 2


@pytest.mark.parametrize("cs,rcs,res", [([96], [], True), ([192, 96], [], False), ([96], [96, 96], False)])
def test_rows_reproducible(cs, rcs, res):
    """A repeat launch and a launch into a buffer pre-filled with another value give bit-identical output, and (H <= 28: at most two
    bands, two commutative fp64 addends per address) bit-identical statistics from zeroed buffers."""
    B = 6
    d = _case(B, 28, 28, cs, rcs, res, 1, seed=7 + sum(cs))
    M = B * 784
    o1 = torch.full((M, N), 7.0, dtype=torch.bfloat16, device="cuda")
    o2 = torch.full((M, N), -3.0, dtype=torch.bfloat16, device="cuda")
    s1, s2, s3 = (torch.zeros((B, N, 2), dtype=torch.float64, device="cuda") for _ in range(3))
    assert _run_rows(d, o1, s1) == 0
    first = o1.clone()
    assert _run_rows(d, o1, s2) == 0 and _run_rows(d, o2, s3) == 0
    torch.cuda.synchronize()
    assert torch.equal(first, o1) and torch.equal(o1, o2)
    assert torch.equal(s1, s2) and torch.equal(s1, s3) and bool((s1[:, :, 1] > 0).all())
    assert bool(torch.isfinite(o1.float()).all())


def test_rows_refuses_what_it_does_not_take():
    from ctdd import unet_engine as ue
    lib = ue._lib()
    d = _case(1, 28, 28, [96], [], False, 1, seed=3)
    out = torch.full((2 * 784, N), 5.0, dtype=torch.bfloat16, device="cuda")
    assert _run_rows(d, out, W=29) != 0 and b"28x29" in lib.ctdd_last_error()
    assert _run_rows(d, out, N=192) != 0
    assert _run_rows(d, out, C1=48) != 0
    assert _run_rows(d, out, f32=1) != 0 and b"bf16" in lib.ctdd_last_error()
    assert _run_rows(d, out, s1_bf16=None) != 0 and b"null" in lib.ctdd_last_error()
    assert _run_rows(d, out, st1=None) != 0 and b"statistics" in lib.ctdd_last_error()
    assert _run_rows(d, out, G=5) != 0 and b"groups" in lib.ctdd_last_error()
    assert _run_rows(d, out, RC1=96, r1_bf16=d["x"][0].data_ptr(), res_bf16=d["x"][0].data_ptr()) != 0      # 1x1 segments and a residual
    torch.cuda.synchronize()
    assert bool((out == 5.0).all())


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


def test_plans_rows_vs_pairs():
    """Plans only (nothing launched), MNIST net, batch 128.  conv_rows = 0: the plan of an engine whose eligibility check says no, label
    for label.  conv_rows = 1 (the default): the ten GroupNorm + convolution pairs of the five 28x28 ResBlocks are ten
    ctdd_unet_conv_rows steps, everything else is unchanged and in order, the summed flops are equal; the output head keeps its
    ctdd_unet_gn_apply.  Training, fp32 and CIFAR plans hold no such step."""
    from ctdd import unet_train
    from ctdd.unet_engine import UNetEngine
    cfg, model = _mnist(0)
    assert getattr(cfg.model, "conv_rows", None) is None          # the default (on) is the engine's
    plans = {}
    for flag in (1, 0):
        cfg.model.conv_rows = flag
        plans[flag] = UNetEngine(model, precision="bf16")._build(128, torch.int64, None).plan
    del cfg.model.conv_rows
    eng = UNetEngine(model, precision="bf16")
    plans["default"] = eng._build(128, torch.int64, None).plan
    eng = UNetEngine(model, precision="bf16")
    eng._runs_conv_rows = lambda *a_, **k_: False
    plans["never"] = eng._build(128, torch.int64, None).plan
    lab = {k: [s_.label for s_ in v] for k, v in plans.items()}
    assert lab[0] == lab["never"] and lab[1] == lab["default"]
    f1, f0 = [lb[0] for lb in lab[1]], [lb[0] for lb in lab[0]]
    assert f1.count("ctdd_unet_conv_rows") == 10 and f0.count("ctdd_unet_conv_rows") == 0
    assert all("28x28" in lb[1] for lb in lab[1] if lb[0] == "ctdd_unet_conv_rows")
    assert f0.count("ctdd_unet_gn_apply") == f1.count("ctdd_unet_gn_apply") + 10 and f1.count("ctdd_unet_gn_apply") == 1
    assert f0.count("ctdd_unet_conv_ring") == f1.count("ctdd_unet_conv_ring") + 7
    assert f0.count("ctdd_unet_conv_patch") == f1.count("ctdd_unet_conv_patch") + 3
    assert len(f1) == len(f0) - 10
    # everything else unchanged and in order: each (gn_apply, N = 96 convolution) pair at 28x28 collapses to the rows step
    merged, i = [], 0
    while i < len(lab[0]):
        fn, lb = lab[0][i]
        nxt = lab[0][i + 1] if i + 1 < len(lab[0]) else ("", "")
        if fn == "ctdd_unet_gn_apply" and "28x28" in lb and nxt[0] in ("ctdd_unet_conv_ring", "ctdd_unet_conv_patch") and " N=96 " in nxt[1]:
            merged.append("ctdd_unet_conv_rows")
            i += 2
        else:
            merged.append((fn, lb))
            i += 1
    assert merged == [lb[0] if lb[0] == "ctdd_unet_conv_rows" else lb for lb in lab[1]]
    assert sum(s_.flops for s_ in plans[1]) == sum(s_.flops for s_ in plans[0])
    # no such step in a training plan, an fp32 plan, the CIFAR plan (W = 32), all at batch 128 and with the grid-size rule out of
    # the way (conv_rows_min_wgs = 1): what keeps the step out is the training / fp32 guard and the kernel's shape check
    cfg.model.conv_rows_min_wgs = 1
    unet_train.lib()
    te = UNetEngine(model, precision="bf16")
    shape = (128, 28, 28, [96], [], 96, 32, False)
    assert te._runs_conv_rows(*shape, False) and not te._runs_conv_rows(*shape, True)
    st = te._build(128, torch.int64, None, tc=unet_train.TrainCtx(te, 128, False))
    assert all(s_.label[0] != "ctdd_unet_conv_rows" for s_ in st.plan + st.bwd_plan)
    del st, te
    e32 = UNetEngine(model, precision="fp32")
    assert not e32._runs_conv_rows(*shape, False)
    assert all(s_.label[0] != "ctdd_unet_conv_rows" for s_ in e32._build(128, torch.int64, None).plan)
    del e32
    import lib.models.model_utils as mu
    from config.cifar10_config.config_tauUnet_cifar10 import get_config
    ccfg = get_config()
    ccfg.device = "cuda"
    ccfg.model.conv_rows_min_wgs = 1
    torch.manual_seed(0)
    cifar = mu.create_model(ccfg, torch.device("cuda"))
    assert all(s_.label[0] != "ctdd_unet_conv_rows" for s_ in UNetEngine(cifar, precision="bf16")._build(128, torch.int64, None, logits_bf16=True).plan)


def test_end_to_end_rows_vs_pairs():
    """MNIST net, batch 8: engine logits with conv_rows = 1 against conv_rows = 0 within 2e-2 of the logit scale, each within 5e-2 of
    the torch module (the bars of tests/test_gpu_unet.py)."""
    from ctdd.unet_engine import UNetEngine
    B = 8
    cfg, model = _mnist(0)
    g = torch.Generator(device="cuda").manual_seed(11)
    x = torch.randint(0, 256, (B, 784), device="cuda", generator=g)
    t = torch.rand(B, device="cuda", generator=g) * 0.98 + 0.01
    with torch.no_grad():
        cfg.model.engine = "torch"
        want = model(x, t)
    cfg.model.conv_rows_min_wgs = 1          # (batch 8 is 16 workgroups: the kernel runs whatever the default threshold)
    outs = {}
    for flag in (1, 0):
        cfg.model.conv_rows = flag
        eng = UNetEngine(model, precision="bf16")
        with torch.no_grad():
            outs[flag] = eng(x.view(B, 1, 28, 28), t).float().clone()
        fns = [s_.label[0] for v in eng._plans.values() for s_ in (v.plan if not isinstance(v, tuple) else v[1][0].plan)]
        assert fns.count("ctdd_unet_conv_rows") == (10 if flag else 0)
    scale = float(want.abs().max())
    assert scale > 0.5
    e1, e0, e10 = float((outs[1] - want).abs().max()), float((outs[0] - want).abs().max()), float((outs[1] - outs[0]).abs().max())
    print(f"scale={scale:.3f} rows-module={e1:.4e} pairs-module={e0:.4e} rows-pairs={e10:.4e}")
    assert e1 < 5e-2 * scale and e0 < 5e-2 * scale
    assert e10 < 2e-2 * scale
    assert bool(torch.isfinite(outs[1]).all())
