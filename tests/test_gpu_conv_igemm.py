"""GPU: k_conv_igemm, the generic gather convolution behind ctdd_unet_conv (the whole fp32 mode, every training data gradient,
whatever the specialised kernels refuse), directly against fp64: every segment kind, every compiled (bk, bnt) tile, both modes,
grids down to 2x2 pixels (a 32-row accumulator tile then spans up to eight samples) and non-square ones, ragged column tiles,
the logits layout and every epilogue term.  Cases, references and bounds: tests/conv_cases.py.

A bf16 call with one stride-2 segment would run on k_conv_ring_s2 (tests/test_gpu_conv_stride2.py); it carries a second, 1x1
segment of zeros here, which keeps it on k_conv_igemm and adds exact zeros.

Every small-grid case asks for the per-sample bias and the statistics: those are what a wrong sample index per row corrupts."""
import ctypes as C

import pytest
import torch

import conv_cases as cc

pytestmark = pytest.mark.gpu

TILES = [(96, 3), (96, 4), (96, 1), (64, 4), (64, 2), (64, 1), (32, 1), (32, 3), (32, 4), (16, 1)]     # the CASEs of ctdd_unet_conv
WORST = {}


def igemm_lds(bk, bnt, f32, HW):
    """Bytes of LDS launch_conv asks for: operand tiles, or the per-sample statistics of a 128-row tile if that is more."""
    esz = 4 if f32 else 2
    ldk = bk + 16 // esz
    samples = (128 + HW - 1) // HW + 1                        # tile_stats_samples(128, HW)
    return max((128 + 32 * bnt) * ldk * esz, samples * 32 * bnt * 16)


def _run(case, bk, bnt, what, **outs):
    from ctdd import unet_engine as ue
    lib = ue._lib()
    assert igemm_lds(bk, bnt, case.f32, case.H * case.W) <= 160 * 1024, "the case would ask for more LDS than a CU has"
    assert case.Ktot % bk == 0 and all(c % bk == 0 for c, _ in case.segs)
    out = case.run(lambda a: lib.ctdd_unet_conv(C.byref(a), bk, bnt, int(case.f32), cc.stream()), **outs)
    w = case.check(out, what)
    WORST[what] = w
    print(f"{what}: worst err/bound so far in this file {max(WORST.values()):.3f}")
    return out


def _outs(f32, stats=True):
    return dict(out_f32=True, out_hi=not f32, stats=stats)


def _off_ring(segs, f32, bk):
    """+ a zero 1x1 segment where the call would otherwise leave for the stride-2 ring kernel."""
    if not f32 and len(segs) == 1 and segs[0][1] == cc.KS2:
        return segs + [(bk, cc.K1, "zero")]
    return segs


KIND_GEOM = {                                                 # kind -> output grid and source grid (non-square, H*W = 35 or 24)
    cc.K3: dict(H=5, W=7), cc.K1: dict(H=5, W=7), cc.KS2: dict(H=5, W=7, Hin=10, Win=14),
    cc.KUP: dict(H=4, W=6, Hin=2, Win=3), cc.KS2T: dict(H=5, W=7, Hin=2, Win=3),
}


@pytest.mark.parametrize("f32", [False, True], ids=["bf16", "fp32"])
@pytest.mark.parametrize("bk,bnt", [(16, 1), (32, 3)])
@pytest.mark.parametrize("kind", [cc.K3, cc.K1, cc.KS2, cc.KUP, cc.KS2T])
def test_each_segment_kind_alone(kind, bk, bnt, f32):
    """N = 40: a ragged second column tile under bnt = 1, a partly filled one under bnt = 3."""
    case = cc.ConvCase(B=3, segs=_off_ring([(32, kind)], f32, bk), N=40, f32=f32, bias=True, bias_shift=4.0, tbias=True, res=True,
                       seed=10 + kind, **KIND_GEOM[kind])
    _run(case, bk, bnt, f"kind {kind} bk={bk} bnt={bnt} {'fp32' if f32 else 'bf16'}", **_outs(f32))


@pytest.mark.parametrize("f32", [False, True], ids=["bf16", "fp32"])
@pytest.mark.parametrize("segs,geom", [
    ([(32, cc.K3), (16, cc.K1)], dict(H=7, W=7)),                             # ResBlock conv2 with its folded skip
    ([(32, cc.K3), (16, cc.K3)], dict(H=7, W=7)),                             # the up path's concatenation
    ([(32, cc.KUP), (16, cc.K1)], dict(H=6, W=10, Hin=3, Win=5)),             # Upsample from Hin = H / 2, + a full-resolution 1x1 source
    ([(16, cc.K1), (16, cc.K3), (32, cc.K1)], dict(H=5, W=7)),                # three segments, 1x1 first
], ids=["conv2+skip", "concat", "up+1x1", "1x1-3x3-1x1"])
def test_segment_combinations(segs, geom, f32):
    case = cc.ConvCase(B=3, segs=segs, N=40, f32=f32, bias=True, bias_shift=4.0, tbias=True, res=True, seed=21, **geom)
    _run(case, 16, 1, f"segments {segs} {'fp32' if f32 else 'bf16'}", **_outs(f32))


@pytest.mark.parametrize("f32", [False, True], ids=["bf16", "fp32"])
@pytest.mark.parametrize("bk,bnt", TILES)
def test_every_instantiation(bk, bnt, f32):
    """B = 3 at 7x7: 147 rows, two workgroup tiles, 32-row tiles that straddle samples.  N = 40 under bnt = 1 (ragged second
    tile), else 32 bnt + 8 (a second tile of 8 columns)."""
    N = 40 if bnt == 1 else 32 * bnt + 8
    case = cc.ConvCase(B=3, H=7, W=7, segs=[(192 if bk in (96, 64) else 64, cc.K3)], N=N, f32=f32, bias=True, bias_shift=4.0,
                       tbias=True, res=True, seed=30 + bk + bnt)
    _run(case, bk, bnt, f"tile bk={bk} bnt={bnt} {'fp32' if f32 else 'bf16'}", **_outs(f32))


GRIDS = [(5, 2, 2), (4, 3, 3), (5, 4, 4), (3, 7, 7), (2, 5, 7), (3, 3, 12), (1, 3, 3)]


@pytest.mark.parametrize("f32", [False, True], ids=["bf16", "fp32"])
@pytest.mark.parametrize("B,H,W", GRIDS)
def test_grid_shapes(B, H, W, f32):
    """Per-sample bias, residual and statistics on every grid: each row's sample is row // (H*W), however many samples a 32-row
    tile spans ((5, 2, 2): eight; (4, 3, 3): four)."""
    case = cc.ConvCase(B=B, H=H, W=W, segs=[(32, cc.K3)], N=40, f32=f32, bias=True, bias_shift=4.0, tbias=True, res=True,
                       seed=100 * B + 10 * H + W)
    _run(case, 16, 1, f"grid ({B}, {H}, {W}) {'fp32' if f32 else 'bf16'}", **_outs(f32))


@pytest.mark.parametrize("f32", [False, True], ids=["bf16", "fp32"])
@pytest.mark.parametrize("B,H,W,bk,bnt", [(5, 2, 2, 16, 1), (4, 3, 3, 32, 3), (3, 7, 7, 16, 1), (2, 5, 7, 32, 3), (5, 4, 4, 32, 4)])
def test_small_grids_on_wide_tiles_and_stride2(B, H, W, bk, bnt, f32):
    """The Downsample convolution INTO the small grid (the deepest level of a three-level 8x8 / 12x12 network) and wide tiles."""
    case = cc.ConvCase(B=B, H=H, W=W, Hin=2 * H, Win=2 * W, segs=_off_ring([(32, cc.KS2)], f32, bk), N=96, f32=f32, bias=True,
                       bias_shift=4.0, tbias=True, seed=7 * B + H)
    _run(case, bk, bnt, f"stride 2 into ({B}, {H}, {W}) bk={bk} bnt={bnt} {'fp32' if f32 else 'bf16'}", **_outs(f32))


@pytest.mark.parametrize("f32", [False, True], ids=["bf16", "fp32"])
@pytest.mark.parametrize("B,H,W", [(5, 2, 2), (4, 3, 3), (3, 7, 7), (2, 5, 7)])
def test_logits_layout(B, H, W, f32):
    """N = 48 = 3 channels x 16 states straight in the (B, C*H*W, S) layout: fp32 in the fp32 mode, bf16 (alone) in the bf16 mode."""
    case = cc.ConvCase(B=B, H=H, W=W, segs=[(32, cc.K3)], N=48, f32=f32, bias=True, bias_shift=4.0, tbias=True, logits_C=3, seed=B + H)
    what = f"logits layout ({B}, {H}, {W}) {'fp32' if f32 else 'bf16'}"
    if f32:
        _run(case, 16, 1, what, out_f32=True, stats=True)
    else:
        _run(case, 16, 1, what, out_hi=True)
        _run(case, 32, 3, what + " both planes", out_f32=True, out_hi=True, stats=True)


@pytest.mark.parametrize("f32", [False, True], ids=["bf16", "fp32"])
@pytest.mark.parametrize("act", [1, 2])
@pytest.mark.parametrize("B,H,W", [(4, 3, 3), (2, 5, 7)])
def test_activations(B, H, W, act, f32):
    """ReLU / GELU(erf) on acc + bias + per-sample bias, before the residual."""
    case = cc.ConvCase(B=B, H=H, W=W, segs=[(32, cc.K3)], N=40, f32=f32, bias=True, tbias=True, res=True, act=act, seed=act)
    _run(case, 16, 1, f"act {act} ({B}, {H}, {W}) {'fp32' if f32 else 'bf16'}", out_f32=True, out_hi=not f32)


def test_plain_outputs_without_epilogue_terms():
    """No bias, no per-sample bias, no residual, no statistics: bf16 output alone, and fp32 output alone."""
    for f32 in (False, True):
        case = cc.ConvCase(B=4, H=3, W=3, segs=[(32, cc.K3)], N=40, f32=f32, seed=2)
        _run(case, 16, 1, f"plain {'fp32' if f32 else 'bf16'}", out_f32=f32, out_hi=not f32)


def test_statistics_accumulate_and_repeat():
    """Twice into the same pool: twice the sums; the outputs bit for bit the same."""
    from ctdd import unet_engine as ue
    lib = ue._lib()
    case = cc.ConvCase(B=4, H=3, W=3, segs=[(32, cc.K3)], N=40, bias=True, bias_shift=4.0, tbias=True, seed=3)
    call = lambda a: lib.ctdd_unet_conv(C.byref(a), 16, 1, 0, cc.stream())
    one = case.run(call, out_f32=True, stats=True)
    two = case.run(lambda a: call(a) or call(a), out_f32=True, stats=True)
    assert torch.equal(one["f32"], two["f32"])
    assert ((two["stats"] - 2 * one["stats"]).abs() <= 1e-12 * one["stats"].abs()).all().item()


def test_refusals():
    """Host-side checks only: nothing is launched."""
    from ctdd import unet_engine as ue
    lib = ue._lib()
    case = cc.ConvCase(B=2, H=5, W=7, segs=[(48, cc.K1)], N=40, seed=4)
    keep = []
    out = torch.full((case.M, case.N), cc.SENT, dtype=torch.bfloat16, device="cuda")

    def args():
        a = case.args(ue, keep)
        a.out_hi = out.data_ptr()
        return a
    a = args()
    assert "multiple of BK" in cc.refused(lib, lib.ctdd_unet_conv(C.byref(a), 32, 1, 0, cc.stream()))          # Ktot = 48
    assert "no conv instantiation" in cc.refused(lib, lib.ctdd_unet_conv(C.byref(a), 48, 1, 0, cc.stream()))   # no (48, 1)
    assert "no conv instantiation" in cc.refused(lib, lib.ctdd_unet_conv(C.byref(a), 16, 2, 0, cc.stream()))   # no (16, 2)
    assert "null source" in cc.refused(lib, lib.ctdd_unet_conv(C.byref(a), 16, 1, 1, cc.stream()))             # fp32 mode, bf16 operands
    a = args()
    a.seg[0].hi = None
    assert "null source" in cc.refused(lib, lib.ctdd_unet_conv(C.byref(a), 16, 1, 0, cc.stream()))
    a = args()
    a.w_hi = None
    assert "null weights" in cc.refused(lib, lib.ctdd_unet_conv(C.byref(a), 16, 1, 0, cc.stream()))
    a = args()
    a.nseg = 4
    assert "nseg" in cc.refused(lib, lib.ctdd_unet_conv(C.byref(a), 16, 1, 0, cc.stream()))
    torch.cuda.synchronize()
    assert (out == cc.SENT).all().item()


def test_statistics_that_do_not_fit_the_lds_are_refused():
    """H*W = 1: a 128-row tile holds 128 samples, whose statistics on a 96-column tile are 198 KB of LDS -- refused before the
    launch (the host-side size rule of this file, igemm_lds, is the launcher's)."""
    from ctdd import unet_engine as ue
    lib = ue._lib()
    case = cc.ConvCase(B=3, H=1, W=1, segs=[(32, cc.K1)], N=96, seed=5)
    assert igemm_lds(32, 3, False, 1) > 160 * 1024 >= igemm_lds(32, 1, False, 1)
    keep = []
    a = case.args(ue, keep)
    out = torch.full((case.M, case.N), cc.SENT, dtype=torch.bfloat16, device="cuda")
    a.out_hi = out.data_ptr()
    assert "LDS" in cc.refused(lib, lib.ctdd_unet_conv(C.byref(a), 32, 3, 0, cc.stream()))
    torch.cuda.synchronize()
    assert (out == cc.SENT).all().item()
    case1 = cc.ConvCase(B=3, H=1, W=1, segs=[(32, cc.K1)], N=40, bias=True, bias_shift=4.0, tbias=True, seed=5)
    _run(case1, 32, 1, "1x1 grid bk=32 bnt=1", out_f32=True, out_hi=True, stats=True)
