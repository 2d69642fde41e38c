"""GPU: the output head's GroupNorm + Swish + 3x3 convolution in one launch (csrc/unet_head_kernels.hip, ctdd_unet_conv_rows_head) against
the pair it replaces (ctdd_unet_gn_apply -> ctdd_unet_conv_ring bnt 2, bf16 output) and against torch fp64, against ctdd_unet_conv_rows
at N = 96, its reproducibility, its refusals, and the plans the engine builds with cfg.model.head_rows = 1 / 0.  The construction is
that of tests/test_gpu_conv_rows.py: bf16-valued random inputs; the input statistics are computed in torch fp64 and handed to both
paths."""
import ctypes as C
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

HEAD = "ctdd_unet_conv_rows_head"


def _stream():
    return torch.cuda.current_stream().cuda_stream


@functools.lru_cache(maxsize=None)
def _case(B, H, W, C1, N, seed):
    """Random bf16-valued input and parameters of one head (NHWC source, [N][9 C1] weights, K = tap -> channel), made once per shape
    and shared by the tests that use it (nothing writes into it but the packed weights cached beside it)."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    rn = lambda *s: torch.randn(s, device="cuda", generator=g)
    M, K = B * H * W, 9 * C1
    d = {"B": B, "H": H, "W": W, "C1": C1, "N": N}
    d["x"] = rn(M, C1).to(torch.bfloat16)
    d["gamma"], d["beta"] = 1.0 + 0.3 * rn(C1), 0.3 * rn(C1)
    d["w"] = (rn(N, K) / K ** 0.5).to(torch.bfloat16)
    d["bias"] = 0.1 * rn(N)
    xd = d["x"].double().view(B, H * W, -1)
    d["st"] = torch.stack([xd.sum(1), (xd * xd).sum(1)], -1).contiguous()      # [B][C][2]
    return d


def _args(d, out):
    from ctdd import unet_engine as ue
    a = ue._ConvRowsArgs()
    a.s1_bf16, a.st1, a.C1 = d["x"].data_ptr(), d["st"].data_ptr(), d["C1"]
    a.gamma, a.beta, a.G, a.eps = d["gamma"].data_ptr(), d["beta"].data_ptr(), 32, 1e-5
    a.bias, a.out_bf16 = d["bias"].data_ptr(), out if isinstance(out, int) else out.data_ptr()
    a.B, a.H, a.W, a.N = d["B"], d["H"], d["W"], d["N"]
    return a


def _run_head(d, out, f32=0, **over):
    """One ctdd_unet_conv_rows_head launch; `over` overrides fields of the argument block (the refusal cases)."""
    from ctdd import unet_engine as ue
    a = _args(d, out)
    if "wp_head" not in d:
        d["wp_head"] = ue.pack_conv_rows_head_weights(d["w"], d["C1"])           # (kept alive in d)
    a.w = d["wp_head"].data_ptr()
    for k, v in over.items():
        setattr(a, k, v)
    return ue._lib().ctdd_unet_conv_rows_head(C.byref(a), f32, _stream())


def _run_rows(d, out):
    """The same inputs through ctdd_unet_conv_rows (N = 96): no residual, no time bias, no output statistics."""
    from ctdd import unet_engine as ue
    a = _args(d, out)
    if "wp_rows" not in d:
        d["wp_rows"] = ue.pack_conv_rows_weights(d["w"], [d["C1"]], [])
    a.w = d["wp_rows"].data_ptr()
    return ue._lib().ctdd_unet_conv_rows(C.byref(a), 0, _stream())


def _run_pair(d):
    """The two launches the kernel replaces: ctdd_unet_gn_apply from the same statistics, then the ring convolution on 64-column
    tiles (bnt 2) with bf16 output.  The ring kernel takes a grid of fewer than 32 pixels (other than 16) for one sample only: such
    a case runs the convolution sample by sample."""
    from ctdd import unet_engine as ue
    lib = ue._lib()
    B, H, W, C1, N = d["B"], d["H"], d["W"], d["C1"], d["N"]
    M, HW = B * H * W, H * W
    act = torch.empty((M, C1), dtype=torch.bfloat16, device="cuda")
    y = torch.empty((M, N), dtype=torch.bfloat16, device="cuda")
    g = ue._GnArgs()
    g.s1_bf16, g.st1, g.C1 = d["x"].data_ptr(), d["st"].data_ptr(), C1
    g.gamma, g.beta, g.B, g.HW, g.G, g.eps, g.swish, g.out_hi = d["gamma"].data_ptr(), d["beta"].data_ptr(), B, HW, 32, 1e-5, 1, act.data_ptr()
    assert lib.ctdd_unet_gn_apply(C.byref(g), _stream()) == 0, lib.ctdd_last_error()
    whole = HW >= 32 or HW == 16
    for b0 in ([0] if whole else range(B)):
        c = ue._ConvArgs()
        c.nseg = 1
        c.seg[0].hi, c.seg[0].C, c.seg[0].kind = act.data_ptr() + b0 * HW * C1 * 2, C1, ue.SEG_3x3
        c.w_hi, c.B, c.H, c.W, c.Hin, c.Win, c.N, c.Ktot = d["w"].data_ptr(), (B if whole else 1), H, W, H, W, N, 9 * C1
        c.bias, c.out_hi = d["bias"].data_ptr(), y.data_ptr() + b0 * HW * N * 2
        assert lib.ctdd_unet_conv_ring(C.byref(c), 2, _stream()) == 0, lib.ctdd_last_error()
    return y


def _fp64(d):
    """The pair in torch fp64 from the same bf16-valued inputs, no intermediate rounding."""
    import torch.nn.functional as F
    B, H, W, C1, N = d["B"], d["H"], d["W"], d["C1"], d["N"]
    x = d["x"].double().view(B, H, W, C1).permute(0, 3, 1, 2)
    a = F.silu(F.group_norm(x, 32, d["gamma"].double(), d["beta"].double(), 1e-5))
    y = F.conv2d(a, d["w"].double().view(N, 3, 3, C1).permute(0, 3, 1, 2), d["bias"].double(), padding=1)
    return y.permute(0, 2, 3, 1).reshape(B * H * W, N)


def _seed(B, H, W, C1, N):
    return 1000 * H + 10 * W + C1 + N + B


CASES = [  # (B, H, W, C1, N)
    (2, 28, 28, 96, 256),        # the workload's launch
    (2, 15, 17, 96, 256),        # a second band of one row, a second column half of two pixels
    (2, 14, 28, 96, 160),        # one band, two passes, last pass 64 of 96 channels stored
    (3, 5, 3, 32, 96),           # one pass, one unit block, tiny grid
    (2, 9, 16, 64, 32),          # one pass of a third of a tile row
    (130, 28, 28, 96, 256),      # 260 workgroups, more than the CUs
]


@pytest.mark.parametrize("B,H,W,C1,N", CASES)
def test_head_matches_replaced_pair_and_fp64(B, H, W, C1, N):
    """e_new = max|head - fp64| <= 1.5 e_old = max|pair - fp64|: the same rounding points, so the two errors are draws from one
    distribution (the bars of tests/test_gpu_conv_rows.py); e_old itself under the project's bf16 bar.  The output buffer is
    pre-filled with a sentinel and followed by 64 sentinel rows: the rows stay untouched, and no sentinel is left among the M x N
    outputs, all of which the kernel writes.  N = 160, N = 32: every element of the [pixel][N] image is compared, so a store past
    channel N of a pixel -- which lands in channels [0, 96 passes - N) of the NEXT pixel, written a pass earlier -- shows up as an
    error of the order of the output itself in those channels; they are checked on their own as well."""
    from ctdd import unet_engine as ue
    d = _case(B, H, W, C1, N, _seed(B, H, W, C1, N))
    M = B * H * W
    ref = _fp64(d)
    old = _run_pair(d).double()
    buf = torch.full((M + 64, N), 9.0, dtype=torch.bfloat16, device="cuda")
    assert _run_head(d, buf) == 0, ue._lib().ctdd_last_error()
    new = buf[:M].double()
    assert bool((buf[M:] == 9.0).all())
    e_old, e_new, top = float((old - ref).abs().max()), float((new - ref).abs().max()), float(ref.abs().max())
    print(f"B={B} {H}x{W} C1={C1} N={N}: e_old={e_old:.4e} e_new={e_new:.4e} max|head-pair|={float((new - old).abs().max()):.4e} max|fp64|={top:.3f}")
    assert top < 8.0 and not bool((buf[:M] == 9.0).any())              # (the sentinel is no possible output)
    assert e_old < 5e-2 * top
    assert e_new <= 1.5 * e_old
    over = 96 * -(-N // 96) - N
    if over:
        lead = min(over, N)                                            # the channels of the next pixel a store past N would reach
        e_lead = float((new[:, :lead] - ref[:, :lead]).abs().max())
        print(f"    channels [0, {lead}): e_new={e_lead:.4e}")
        assert e_lead <= 1.5 * e_old


@pytest.mark.parametrize("B,H,W,C1", [(3, 5, 3, 32), (2, 28, 28, 96), (2, 15, 17, 64)])
def test_head_n96_is_conv_rows_bit_for_bit(B, H, W, C1):
    """N = 96 is one pass: the K loop, its order and the epilogue arithmetic (acc + bias, one rounding) of ctdd_unet_conv_rows without
    residual, time bias and output statistics."""
    d = _case(B, H, W, C1, 96, _seed(B, H, W, C1, 96))
    M = B * H * W
    o_head = torch.full((M, 96), 9.0, dtype=torch.bfloat16, device="cuda")
    o_rows = torch.full((M, 96), -9.0, dtype=torch.bfloat16, device="cuda")
    assert _run_head(d, o_head) == 0 and _run_rows(d, o_rows) == 0
    torch.cuda.synchronize()
    assert torch.equal(o_head, o_rows)


@pytest.mark.parametrize("N", [256, 160])
def test_head_reproducible(N):
    """A repeat launch and a launch into a buffer pre-filled with another value give bit-identical output."""
    B = 6
    d = _case(B, 28, 28, 96, N, 7 + N)
    M = B * 784
    o1 = torch.full((M, N), 7.0, dtype=torch.bfloat16, device="cuda")
    o2 = torch.full((M, N), -3.0, dtype=torch.bfloat16, device="cuda")
    assert _run_head(d, o1) == 0
    first = o1.clone()
    assert _run_head(d, o1) == 0 and _run_head(d, o2) == 0
    torch.cuda.synchronize()
    assert torch.equal(first, o1) and torch.equal(o1, o2)
    assert bool(torch.isfinite(o1.float()).all())


def test_head_refuses_what_it_does_not_take():
    from ctdd import unet_engine as ue
    lib = ue._lib()
    d = _case(1, 28, 28, 96, 256, 3)
    out = torch.full((2 * 784, 256), 5.0, dtype=torch.bfloat16, device="cuda")
    other = d["x"].data_ptr()
    assert _run_head(d, out, f32=1) != 0 and b"bf16" in lib.ctdd_last_error()
    assert _run_head(d, out, W=29) != 0 and b"28x29" in lib.ctdd_last_error()
    assert _run_head(d, out, C1=48) != 0 and b"channel counts" in lib.ctdd_last_error()
    assert _run_head(d, out, C1=128) != 0
    assert _run_head(d, out, C2=32, s2_bf16=other, st2=d["st"].data_ptr()) != 0
    assert _run_head(d, out, N=48) != 0
    assert _run_head(d, out, N=608) != 0
    assert _run_head(d, out, RC1=96, r1_bf16=other) != 0
    assert _run_head(d, out, res_bf16=other) != 0                                  # a residual
    assert _run_head(d, out, tbias=d["bias"].data_ptr()) != 0                      # a time bias
    assert _run_head(d, out, out_stats=d["st"].data_ptr()) != 0
    assert _run_head(d, out, s1_bf16=None) != 0 and b"null" in lib.ctdd_last_error()
    assert _run_head(d, out, st1=None) != 0 and b"statistics" in lib.ctdd_last_error()
    assert _run_head(d, out, w=None) != 0 and b"null" in lib.ctdd_last_error()
    assert _run_head(d, out.data_ptr() + 2) != 0 and b"aligned" in lib.ctdd_last_error()      # a misaligned output
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


def _labels(plan):
    return [s_.label for s_ in plan]


def test_plans_head_rows_vs_pair():
    """Plans only (nothing launched), MNIST net, batch 128, bf16 logits, the sampler loop's time row.  Default (head_rows = 1): one
    ctdd_unet_conv_rows_head step, last in the plan, no ctdd_unet_gn_apply at 28x28.  head_rows = 0: the plan of an engine whose
    eligibility check says no, label for label; the two label lists are equal after collapsing the head's (gn_apply, N = 256 ring)
    pair into the new step, and the summed flops are equal.  fp32 logits, conv_rows = 0, the fp32 engine, a training plan, the CIFAR
    plan (logistic head) and a batch-4 plan under the default threshold hold no such step."""
    from ctdd import unet_train
    from ctdd.unet_engine import HEAD_ROWS_MIN_WGS, UNetEngine
    cfg, model = _mnist(0)
    assert getattr(cfg.model, "head_rows", None) is None          # the default (on) is the engine's
    build = lambda eng, B=128, **kw: eng._build(B, torch.int32, None, **{"logits_bf16": True, "uniform_t": "row", **kw})
    plans = {"default": build(UNetEngine(model, precision="bf16")).plan}
    for flag in (1, 0):
        cfg.model.head_rows = flag
        plans[flag] = build(UNetEngine(model, precision="bf16")).plan
    del cfg.model.head_rows
    eng = UNetEngine(model, precision="bf16")
    eng._runs_head_rows = lambda *a_, **k_: False
    plans["never"] = build(eng).plan
    lab = {k: _labels(v) for k, v in plans.items()}
    assert lab[1] == lab["default"] and lab[0] == lab["never"]
    f1, f0 = [lb[0] for lb in lab[1]], [lb[0] for lb in lab[0]]
    assert f1.count(HEAD) == 1 and f0.count(HEAD) == 0
    assert lab[1][-1] == (HEAD, "28x28 K=864 N=256 gn+conv rows head C=[96]")
    assert not any(fn == "ctdd_unet_gn_apply" and "28x28" in lb for fn, lb in lab[1])
    assert lab[0][-2][0] == "ctdd_unet_gn_apply" and "28x28" in lab[0][-2][1]
    assert lab[0][-1][0] == "ctdd_unet_conv_ring" and " N=256 " in lab[0][-1][1] and "bnt=2" in lab[0][-1][1]
    assert lab[1][:-1] == lab[0][:-2]                              # the pair collapses into the new step, nothing else moves
    assert sum(s_.flops for s_ in plans[1]) == sum(s_.flops for s_ in plans[0])
    assert plans[1][-1].flops == 2 * 128 * 784 * 256 * 864
    # none of these holds the new step
    none = lambda plan: all(s_.label[0] != HEAD for s_ in plan)
    assert none(build(UNetEngine(model, precision="bf16"), logits_bf16=False).plan)            # fp32 logits
    cfg.model.conv_rows = 0
    assert none(build(UNetEngine(model, precision="bf16")).plan)
    del cfg.model.conv_rows
    assert 4 * 2 < HEAD_ROWS_MIN_WGS and none(build(UNetEngine(model, precision="bf16"), B=4).plan)   # under the default threshold
    shape = (128, 28, 28, 96, 256, 32)
    e32 = UNetEngine(model, precision="fp32")
    assert not e32._runs_head_rows(*shape, False) and none(e32._build(128, torch.int32, None).plan)
    del e32
    unet_train.lib()
    te = UNetEngine(model, precision="bf16")
    assert te._runs_head_rows(*shape, False) and not te._runs_head_rows(*shape, True)
    st = te._build(128, torch.int64, None, tc=unet_train.TrainCtx(te, 128, False))
    assert none(st.plan + st.bwd_plan)
    del st, te
    import lib.models.model_utils as mu
    from config.cifar10_config.config_tauUnet_cifar10 import get_config
    ccfg = get_config()
    ccfg.device = "cuda"
    ccfg.model.head_rows_min_wgs = 1
    torch.manual_seed(0)
    cifar = mu.create_model(ccfg, torch.device("cuda"))
    assert none(UNetEngine(cifar, precision="bf16")._build(128, torch.int64, None, logits_bf16=True).plan)


def test_end_to_end_head_rows_vs_pair():
    """MNIST net, batch 8, bf16 logits: head_rows = 1 against head_rows = 0 within 2e-2 of the logit scale, each within 5e-2 of the
    torch module (the bars of tests/test_gpu_unet.py), all finite."""
    from ctdd.unet_engine import UNetEngine
    B = 8
    cfg, model = _mnist(0)
    g = torch.Generator(device="cuda").manual_seed(11)
    x = torch.randint(0, 256, (B, 784), device="cuda", generator=g)
    t = torch.rand(B, device="cuda", generator=g) * 0.98 + 0.01
    with torch.no_grad():
        cfg.model.engine = "torch"
        want = model(x, t)
    cfg.model.head_rows_min_wgs = 1          # (batch 8 is 16 workgroups: the kernel runs whatever the default threshold)
    cfg.model.conv_rows_min_wgs = 1
    outs = {}
    for flag in (1, 0):
        cfg.model.head_rows = flag
        eng = UNetEngine(model, precision="bf16")
        with torch.no_grad():
            o = eng(x.view(B, 1, 28, 28), t, logits_bf16=True)
        assert o.dtype == torch.bfloat16
        outs[flag] = o.float().clone()
        fns = [s_.label[0] for v in eng._plans.values() for s_ in (v.plan if not isinstance(v, tuple) else v[1][0].plan)]
        assert fns.count(HEAD) == (1 if flag else 0)
    scale = float(want.abs().max())
    assert scale > 0.5
    e1, e0, e10 = float((outs[1] - want).abs().max()), float((outs[0] - want).abs().max()), float((outs[1] - outs[0]).abs().max())
    print(f"scale={scale:.3f} head-module={e1:.4e} pair-module={e0:.4e} head-pair={e10:.4e}")
    assert e1 < 5e-2 * scale and e0 < 5e-2 * scale
    assert e10 < 2e-2 * scale
    assert bool(torch.isfinite(outs[1]).all())
