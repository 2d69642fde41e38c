"""GPU: the Upsample convolution (3x3, pad 1, on the nearest-2x grid; reference lib/networks/unet.py:79-85) as four 2x2-tap phase
convolutions of the source in one launch (ctdd_unet_conv_up_phases, k_conv_ring_up), called directly.

Parent path: ctdd_unet_upsample2x into a materialised 2x grid, then the stride-1 3x3 ring launch (ctdd_unet_conv_ring) with the
original weights rounded to bf16 one by one.  New path: the weights summed in fp32 (ctdd.unet_engine.fold_upsample_weights),
rounded to bf16 once.

(a) Exact case.  Inputs integers in [-4, 4], weights and bias multiples of 1/4 in [-1, 1]: every product, folded weight
    (a multiple of 1/4 in [-4, 4]) and partial sum is exact in bf16 / fp32, the fp64 reference lies on quarter steps with
    |y| <= 4 * 9 * 64 + 1 = 2305, is exactly representable in fp32 and rounds to bf16 identically on every path.  Output bits
    of the new path == parent path == reference rounded to bf16.
    Statistics: every convolution epilogue of this library sums the fp32 values it is about to round to bf16 (the parent path
    too; tests/test_gpu_conv_stride2.py), so the reference sums are the fp64 sums of the outputs rounded to fp32 -- here the fp64
    reference itself -- and must be met to 1e-12 relative.  (Sums of the bf16-rounded outputs differ from what any of the
    epilogues accumulates by the rounding, ~2^-9 relative.)  The epilogue adds up to eight values and squares per lane in fp32
    before going to fp64: on quarter steps those partial sums are exact while 8 * 16 * max|y|^2 < 2^24, which the CPU check of
    the reference asserts for the shapes used together with the exactness claim above.
(b) Random case.  Gaussian inputs and weights against fp64 on the bf16-rounded input and the fp32 weights:
    max|new - ref| <= 2 max|parent - ref| (a folded weight's rounding error is at worst the sum of the roundings it replaces).
(c) Refusals: non-zero status, ctdd_last_error set, nothing launched.
(d) Engine plans with cfg.model.upsample_phases = 1 / 0 and the knob-1 logits against the fp32 torch module.
"""
import ctypes as C
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

SENT = 24576.0          # sentinel rows around the output (exact in bf16, far from any result)
PADROWS = 64
#          B   H  W   C    N
SHAPES = [(3, 5, 7, 16, 96),      # M = 105: one partial tile, H != W, one unit
          (12, 7, 7, 64, 192),    # M = 588: two tiles, the second partial; tiles straddle samples; four units (the ring wraps); two column tiles per phase
          (2, 8, 4, 32, 64)]      # H*W = 32, the entry's minimum; 64-column tiles
IDS = ["B3-5x7-C16-N96", "B12-7x7-C64-N192", "B2-8x4-C32-N64"]


def _stream():
    return torch.cuda.current_stream().cuda_stream


class _Case:
    """Operands of one Upsample convolution and its fp64 reference on the (B, 2H, 2W) grid, rows = output pixels."""

    def __init__(self, B, H, W, Cc, N, exact):
        g = torch.Generator().manual_seed(10000 * H + 100 * W + Cc + N + (1 if exact else 0))
        self.B, self.H, self.W, self.Cc, self.N = B, H, W, Cc, N
        self.M = B * H * W
        if exact:
            self.x = torch.randint(-4, 5, (B, H, W, Cc), generator=g).to(torch.bfloat16)
            self.w = torch.randint(-4, 5, (N, Cc, 3, 3), generator=g).float() / 4
            self.bias = torch.randint(-4, 5, (N,), generator=g).float() / 4
        else:
            self.x = torch.randn((B, H, W, Cc), generator=g).to(torch.bfloat16)
            self.w = torch.randn((N, Cc, 3, 3), generator=g) / (9 * Cc) ** 0.5
            self.bias = torch.randn(N, generator=g) * 0.5
        # (random, asymmetric in every tap: the four phases' folded weights all differ; tests/test_upsample_fold_cpu.py)
        up = self.x.double().permute(0, 3, 1, 2).repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)
        self.conv = F.conv2d(up, self.w.double(), padding=1).permute(0, 2, 3, 1).reshape(4 * self.M, N)

    def ref(self, bias):
        return self.conv + self.bias.double() if bias else self.conv

    def _finish(self, a, lib_call, want_stats, bias):
        from ctdd import unet_engine as ue
        lib = ue._lib()
        B, N, M4 = self.B, self.N, 4 * self.M
        keep = []
        if bias:
            bv = self.bias.cuda()
            keep.append(bv)
            a.bias = bv.data_ptr()
        out = torch.full((M4 + 2 * PADROWS, N), SENT, dtype=torch.bfloat16, device="cuda")
        a.out_hi = out[PADROWS:].data_ptr()
        stats = None
        if want_stats:
            stats = torch.zeros((B, N, 2), dtype=torch.float64, device="cuda")
            a.stats = stats.data_ptr()
        rc = lib_call(lib, a)
        assert rc == 0, lib.ctdd_last_error().decode()
        torch.cuda.synchronize()
        assert (out[:PADROWS] == SENT).all().item() and (out[PADROWS + M4:] == SENT).all().item(), "write outside the output"
        return out[PADROWS:PADROWS + M4].cpu(), None if stats is None else stats.cpu()

    def args_new(self):
        """(argument block, kept tensors) of the phase launch, output / bias / statistics not yet set."""
        from ctdd import unet_engine as ue
        B, H, W, Cc, N = self.B, self.H, self.W, self.Cc, self.N
        x = self.x.cuda()
        wf = ue.fold_upsample_weights(self.w).to(torch.bfloat16).reshape(4 * N, 4 * Cc).contiguous().cuda()   # fp32 sums, rounded once
        a = ue._ConvArgs()
        a.nseg = 1
        a.seg[0].hi, a.seg[0].C, a.seg[0].kind = x.data_ptr(), Cc, ue.SEG_3x3_UP
        a.w_hi = wf.data_ptr()
        a.B, a.H, a.W, a.Hin, a.Win, a.N, a.Ktot = B, 2 * H, 2 * W, H, W, N, 4 * Cc
        return a, [x, wf]

    def run_new(self, want_stats=False, bias=True):
        a, keep = self.args_new()
        return self._finish(a, lambda lib, a_: lib.ctdd_unet_conv_up_phases(C.byref(a_), 0, _stream()), want_stats, bias)

    def run_parent(self, want_stats=False, bias=True):
        from ctdd import unet_engine as ue
        lib = ue._lib()
        B, H, W, Cc, N = self.B, self.H, self.W, self.Cc, self.N
        x = self.x.cuda()
        up = torch.empty((B, 2 * H, 2 * W, Cc), dtype=torch.bfloat16, device="cuda")
        assert lib.ctdd_unet_upsample2x(x.data_ptr(), B, H, W, Cc, up.data_ptr(), _stream()) == 0, lib.ctdd_last_error().decode()
        wp = self.w.permute(0, 2, 3, 1).reshape(N, 9 * Cc).to(torch.bfloat16).contiguous().cuda()            # [n][tap][c], each rounded
        a = ue._ConvArgs()
        a.nseg = 1
        a.seg[0].hi, a.seg[0].C, a.seg[0].kind = up.data_ptr(), Cc, ue.SEG_3x3
        a.w_hi = wp.data_ptr()
        a.B, a.H, a.W, a.Hin, a.Win, a.N, a.Ktot = B, 2 * H, 2 * W, 2 * H, 2 * W, N, 9 * Cc
        bnt = 3 if N % 96 == 0 else 2
        return self._finish(a, lambda lib_, a_: lib_.ctdd_unet_conv_ring(C.byref(a_), bnt, _stream()), want_stats, bias)

    def sums(self, v):
        v = v.double().reshape(self.B, 4 * self.H * self.W, self.N)
        return torch.stack([v.sum(1), (v * v).sum(1)], -1)


@functools.lru_cache(maxsize=None)
def _case(shape, exact):
    return _Case(*shape, exact=exact)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_exact_reference_is_exact(shape):
    """CPU side of (a): the reference alone satisfies the exactness claim for these shapes."""
    case = _case(shape, True)
    for bias in (False, True):
        y = case.ref(bias)
        ymax = y.abs().max().item()
        assert torch.equal(y * 4, (y * 4).round()) and ymax <= 2305.0                  # quarter steps, bounded
        assert torch.equal(y.float().double(), y)                                      # exactly representable in fp32
        assert 8 * 16 * ymax * ymax < 2.0 ** 24                                        # fp32 sums of eight squares on 1/16 steps: exact
    from ctdd.unet_engine import fold_upsample_weights
    wf = fold_upsample_weights(case.w)
    assert torch.equal(wf.to(torch.bfloat16).float(), wf) and torch.equal(wf.double(), fold_upsample_weights(case.w.double()))
    assert torch.equal(case.w.to(torch.bfloat16).float(), case.w) and wf.abs().max().item() <= 4.0


@pytest.mark.parametrize("stats", [False, True], ids=["nostats", "stats"])
@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_exact_bits(shape, bias, stats):
    case = _case(shape, True)
    want = case.ref(bias)
    new, st_new = case.run_new(want_stats=stats, bias=bias)
    old, st_old = case.run_parent(want_stats=stats, bias=bias)
    want_bf16 = want.float().to(torch.bfloat16)                   # (fp64 -> fp32 is exact here: one rounding)
    n_new = int((new.view(torch.int16) != want_bf16.view(torch.int16)).sum())
    n_old = int((old.view(torch.int16) != want_bf16.view(torch.int16)).sum())
    print(f"{shape} bias={bias} stats={stats}: elements differing from the rounded fp64 reference: new {n_new}, parent {n_old}; "
          f"max |ref| {want.abs().max().item():.2f}")
    assert n_old == 0, "parent path is not exact: the construction of the case is wrong"
    assert n_new == 0
    assert torch.equal(new.view(torch.int16), old.view(torch.int16))
    if stats:
        want_st = case.sums(want)
        for name, st in (("new", st_new), ("parent", st_old)):
            dev = (st - want_st).abs()
            nz = want_st != 0                               # (a zero sum must be met exactly: the assertion below)
            rel = (dev[nz] / want_st[nz].abs()).max().item()
            print(f"  statistics ({name}): max relative deviation from the fp64 sums {rel:.3e}")
            assert bool((dev <= 1e-12 * want_st.abs()).all()), (name, rel)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_random_vs_fp64(shape):
    case = _case(shape, False)
    want = case.ref(True)
    new, _ = case.run_new()
    old, _ = case.run_parent()
    e_new = (new.double() - want).abs().max().item()
    e_old = (old.double() - want).abs().max().item()
    print(f"{shape}: max|new - ref| = {e_new:.4e}, max|parent - ref| = {e_old:.4e}, ratio {e_new / e_old:.3f}, max |ref| {want.abs().max().item():.3f}")
    assert e_new <= 2.0 * e_old, (e_new, e_old)


def test_random_statistics_match_output_sums():
    """Random values: the statistics of the four phases add into the same per-(sample, channel) sums -- the fp64 sums of the
    outputs to bf16 rounding (2^-9 relative per value; the means are shifted away from zero so that a relative bound holds)."""
    case = _case(SHAPES[1], False)
    bias0 = case.bias.clone()
    case.bias = bias0 + 4.0
    try:
        new, st = case.run_new(want_stats=True)
    finally:
        case.bias = bias0
    want = case.sums(new)
    rel = ((st - want).abs() / want.abs()).max().item()
    print(f"statistics vs sums of the bf16 output: max relative deviation {rel:.3e}")
    assert rel <= 2.0 ** -8


REFUSALS = {
    "fp32 mode": dict(f32=1),
    "two segments": dict(nseg=2),
    "C % 16 != 0": dict(C=24),
    "N = 32 (no 64- or 96-column tile)": dict(N=32),
    "N = 160 (no 64- or 96-column tile)": dict(N=160),
    "source H*W < 32": dict(Hs=4, Ws=4),
    "split-K": dict(ksplit=2),
}


@pytest.mark.parametrize("what", list(REFUSALS), ids=[k.split(" (")[0].replace(" ", "_") for k in REFUSALS])
def test_refusals(what):
    from ctdd import unet_engine as ue
    lib = ue._lib()
    over = REFUSALS[what]
    case = _case(SHAPES[0], True)
    B, Cc, N = case.B, over.get("C", case.Cc), over.get("N", case.N)
    Hs, Ws = over.get("Hs", case.H), over.get("Ws", case.W)
    x = torch.zeros((B, Hs, Ws, 32), dtype=torch.bfloat16, device="cuda")
    wf = torch.zeros((4 * 192, 4 * 32), dtype=torch.bfloat16, device="cuda")
    out = torch.full((4 * B * Hs * Ws, 192), SENT, dtype=torch.bfloat16, device="cuda")
    acc = torch.zeros((4 * B * Hs * Ws, 192), dtype=torch.float32, device="cuda")
    a = ue._ConvArgs()
    a.nseg = over.get("nseg", 1)
    for i in range(a.nseg):
        a.seg[i].hi, a.seg[i].C, a.seg[i].kind = x.data_ptr(), Cc, ue.SEG_3x3_UP
    a.w_hi, a.out_hi = wf.data_ptr(), out.data_ptr()
    a.B, a.H, a.W, a.Hin, a.Win, a.N, a.Ktot = B, 2 * Hs, 2 * Ws, Hs, Ws, N, 4 * Cc * a.nseg
    a.ksplit = over.get("ksplit", 0)
    if a.ksplit > 1:
        a.acc_buf = acc.data_ptr()
    rc =lib.ctdd_unet_conv_up_phases(C.byref(a), over.get("f32", 0), _stream())
    torch.cuda.synchronize()
    msg = lib.ctdd_last_error().decode()
    print(f"{what}: rc={rc} '{msg}'")
    assert rc != 0 and "upsample-phase" in msg
    assert bool((out == SENT).all()) and not bool(acc.any()), "a refused call launched something"


def test_refusal_base_block_is_accepted():
    """The argument block the refusal cases modify is itself accepted."""
    case = _case(SHAPES[0], True)
    new, _ = case.run_new()
    assert new.shape == (4 * case.M, case.N)


# ------------------------------------------------------------------ engine plans
def _model(config, seed=0):
    import lib.models.models  # noqa: F401
    import lib.models.model_utils as mu
    if config == "mnist":
        from config.mnist_config.config_tauUnet_mnist import get_config
    else:
        from config.cifar10_config.config_tauUnet_cifar10 import get_config
    cfg = get_config()
    cfg.model.ring_min_tiles = 1                    # the small batch reaches the ring
    torch.manual_seed(seed)
    model = mu.create_model(cfg, torch.device("cuda"))
    g = torch.Generator(device="cuda").manual_seed(seed + 1)
    with torch.no_grad():                           # (the reference zero-initialises the output conv: re-draw so logits vary)
        for name, p in model.named_parameters():
            if p.dim() > 1:
                p.copy_(torch.randn(p.shape, generator=g, device="cuda") / (p[0].numel() ** 0.5))
    model.init_ema()
    model.eval()
    return cfg, model


def _plans(cfg, model, B):
    """Launch labels of the bf16 inference plan with the knob at 1, at 0, and of an engine that cannot take the phase path."""
    from ctdd.unet_engine import UNetEngine
    labels = {}
    assert getattr(cfg.model, "upsample_phases", None) is None        # the default (on) is the engine's
    for flag in (1, 0):
        cfg.model.upsample_phases = flag
        labels[flag] = [s_.label for s_ in UNetEngine(model, precision="bf16")._build(B, torch.int64, None).plan]
    del cfg.model.upsample_phases
    import ctdd.unet_engine as ue
    saved = ue._PlanBuilder.upsample_in_phases
    ue._PlanBuilder.upsample_in_phases = lambda self, cur: False
    try:
        labels["parent"] = [s_.label for s_ in UNetEngine(model, precision="bf16")._build(B, torch.int64, None).plan]
    finally:
        ue._PlanBuilder.upsample_in_phases = saved
    return labels


def _check_plans(labels, n_phase, n_kept):
    f1, f0 = [lb[0] for lb in labels[1]], [lb[0] for lb in labels[0]]
    assert labels[0] == labels["parent"]                               # knob 0: the parent's launch list, label for label
    assert f0.count("ctdd_unet_conv_up_phases") == 0 and f0.count("ctdd_unet_upsample2x") == n_phase + n_kept
    assert f1.count("ctdd_unet_conv_up_phases") == n_phase and f1.count("ctdd_unet_upsample2x") == n_kept
    assert len(f1) == len(f0) - n_phase                                # each phase launch replaces two
    rest1 = [lb for lb in labels[1] if lb[0] != "ctdd_unet_conv_up_phases"]
    it = iter(labels[0])
    assert all(lb in it for lb in rest1)                               # everything else unchanged, in order


def test_engine_plans_and_logits_mnist():
    """MNIST network, batch 2, ring_min_tiles = 1: knob 1 has no ctdd_unet_upsample2x launch and two phase launches (7x7 -> 14x14,
    14x14 -> 28x28); knob 0 is the parent's plan; the knob-1 logits meet the bound tests/test_gpu_unet.py applies to the bf16
    engine against the fp32 torch module (5e-2 of the largest logit)."""
    from ctdd.unet_engine import UNetEngine
    cfg, model = _model("mnist")
    _check_plans(_plans(cfg, model, 2), n_phase=2, n_kept=0)
    B = 2
    g = torch.Generator(device="cuda").manual_seed(5)
    x = torch.randint(0, 256, (B, 784), device="cuda", generator=g)
    t = torch.tensor([0.07, 0.8], device="cuda")
    with torch.no_grad():
        cfg.model.engine = "torch"
        ref = model(x, t).float()
        outs = {}
        for flag in (1, 0):
            cfg.model.upsample_phases = flag
            eng = UNetEngine(model, precision="bf16")
            outs[flag] = eng(x.view(B, 1, 28, 28), t).float().clone()
            steps = [s_ for v in eng._plans.values() for s_ in (v.plan if not isinstance(v, tuple) else v[1][0].plan)]
            assert any(s_.label[0] == "ctdd_unet_conv_up_phases" for s_ in steps) == bool(flag)
    scale = ref.abs().max().item()
    e1, e0 = (outs[1] - ref).abs().max().item(), (outs[0] - ref).abs().max().item()
    print(f"scale {scale:.3f}: phases - module {e1:.4e}, two launches - module {e0:.4e}, phases - two launches {(outs[1] - outs[0]).abs().max().item():.4e}")
    assert scale > 0.5 and bool(torch.isfinite(outs[1]).all())
    assert e1 < 5e-2 * scale
    model.train()


def test_engine_plans_cifar():
    """CIFAR network, batch 2, ring_min_tiles = 1: the 8x8 -> 16x16 and 16x16 -> 32x32 Upsample convolutions become phase launches;
    the 4x4 -> 8x8 one keeps its two launches (a 16-pixel source: the entry refuses H*W < 32)."""
    cfg, model = _model("cifar10")
    _check_plans(_plans(cfg, model, 2), n_phase=2, n_kept=1)
    model.train()
