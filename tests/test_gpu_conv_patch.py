"""GPU: k_conv_patch (entry ctdd_unet_conv_patch), the bf16 slab convolution that the other kernels' tests take as their
baseline, directly against fp64: each compiled family (per-tap, ALLTAPS, DIRECT, EXT, split-K + k_conv_finish) on grids from one
3x3 sample to the widest row the entry accepts.  Cases, references and bounds: tests/conv_cases.py.

Which family a call reaches (ctdd_unet_conv_patch): act / out_lo -> EXT; else bf16 output alone without statistics on
(64|48, 1, 32) and (48, 3, 32|64) -> DIRECT; else (64|48, 1, 32) without split-K -> ALLTAPS; else the per-tap kernel."""
import ctypes as C

import pytest
import torch

import conv_cases as cc

pytestmark = pytest.mark.gpu

WORST = {}
FULL = dict(out_f32=True, out_hi=True, stats=True)           # fp32 + bf16 planes + statistics (keeps a call off DIRECT)
HI = dict(out_hi=True)                                        # what DIRECT takes


def _run(case, tile, what, **outs):
    from ctdd import unet_engine as ue
    lib = ue._lib()
    bk, bnt, wm = tile
    assert all(c % bk == 0 for c, _ in case.segs) and case.N % 8 == 0
    out = case.run(lambda a: lib.ctdd_unet_conv_patch(C.byref(a), bk, bnt, wm, cc.stream()), **outs)
    WORST[what] = case.check(out, what)
    print(f"{what}: worst err/bound so far in this file {max(WORST.values()):.3f}")
    return out


CASES = [
    # name, (B, H, W), segments, N, (bk, bnt, wm), outputs, extra case arguments
    ("per-tap 48x3 7x7", (3, 7, 7), [(96, cc.K3)], 104, (48, 3, 32), FULL, dict(res=True)),
    ("per-tap 48x3 wm64 14x14", (2, 14, 14), [(48, cc.K3)], 96, (48, 3, 64), FULL, dict(res="f32")),
    ("per-tap 64x2 wm64 5x9", (2, 5, 9), [(64, cc.K3)], 72, (64, 2, 64), FULL, {}),
    ("per-tap 64x4 14x14", (2, 14, 14), [(64, cc.K3)], 128, (64, 4, 32), FULL, {}),
    ("per-tap 32x1 4x4", (5, 4, 4), [(64, cc.K3)], 40, (32, 1, 32), FULL, dict(res=True)),
    ("per-tap 16x1 3x3 B=1", (1, 3, 3), [(16, cc.K3)], 40, (16, 1, 32), FULL, {}),
    ("per-tap 16x1 2x33", (1, 2, 33), [(32, cc.K3)], 32, (16, 1, 32), FULL, {}),
    ("alltaps 64x1 4x4", (5, 4, 4), [(64, cc.K3)], 40, (64, 1, 32), FULL, {}),
    ("alltaps 64x1 2x33", (1, 2, 33), [(128, cc.K3)], 64, (64, 1, 32), FULL, dict(res=True)),
    ("alltaps 48x1 5x9", (2, 5, 9), [(96, cc.K3)], 40, (48, 1, 32), FULL, {}),
    ("alltaps 48x1 7x7 1x1 first", (3, 7, 7), [(48, cc.K1), (96, cc.K3)], 64, (48, 1, 32), FULL, {}),
    ("direct 64x1 7x7", (3, 7, 7), [(128, cc.K3)], 40, (64, 1, 32), HI, dict(res=True)),
    ("direct 64x1 3x3 B=1", (1, 3, 3), [(64, cc.K3), (64, cc.K1)], 64, (64, 1, 32), HI, {}),
    ("direct 48x1 4x4", (5, 4, 4), [(48, cc.K3)], 40, (48, 1, 32), HI, {}),
    ("direct 48x3 wm64 14x14", (2, 14, 14), [(96, cc.K3)], 104, (48, 3, 64), HI, dict(res=True)),
    ("direct 48x3 wm32 5x9", (2, 5, 9), [(48, cc.K3)], 96, (48, 3, 32), HI, {}),
    ("direct 48x3 wm64 2x33", (1, 2, 33), [(48, cc.K1), (48, cc.K3)], 96, (48, 3, 64), HI, dict(res=True)),
    ("multi 1x1 first 64x2 14x14", (2, 14, 14), [(64, cc.K1), (128, cc.K3), (64, cc.K1)], 72, (64, 2, 32), FULL, dict(res=True)),
    ("logits 32x3 7x7", (3, 7, 7), [(32, cc.K3)], 48, (32, 3, 32), FULL, dict(logits_C=3)),
    ("logits 64x4 5x9", (2, 5, 9), [(64, cc.K3)], 128, (64, 4, 64), FULL, dict(logits_C=4)),
]


@pytest.mark.parametrize("name,grid,segs,N,tile,outs,extra", CASES, ids=[c[0].replace(" ", "-") for c in CASES])
def test_patch_vs_fp64(name, grid, segs, N, tile, outs, extra):
    B, H, W = grid
    case = cc.ConvCase(B=B, H=H, W=W, segs=segs, N=N, bias=True, bias_shift=4.0, tbias=True, seed=len(name) + 31 * H + W, **extra)
    _run(case, tile, name, **outs)


@pytest.mark.parametrize("act", [1, 2])
@pytest.mark.parametrize("grid,segs,N,tile", [
    ((3, 7, 7), [(64, cc.K3)], 72, (64, 2, 32)),
    ((5, 4, 4), [(48, cc.K3), (48, cc.K1)], 40, (48, 1, 32)),
    ((2, 5, 9), [(16, cc.K1)], 40, (16, 1, 32)),
], ids=["64x2-7x7", "48x1-4x4", "16x1-5x9"])
def test_patch_activation_and_split_output(grid, segs, N, tile, act):
    """EXT: ReLU / GELU(erf) before the residual, and out_lo = bf16(v - float(out_hi)) exactly (case.check)."""
    B, H, W = grid
    case = cc.ConvCase(B=B, H=H, W=W, segs=segs, N=N, bias=True, tbias=True, res=True, act=act, seed=50 + act)
    _run(case, tile, f"ext act={act} {tile} {grid}", out_f32=True, out_hi=True, out_lo=True)


@pytest.mark.parametrize("ksplit", [2, 3])
@pytest.mark.parametrize("grid,segs,N,tile,res", [
    ((3, 7, 7), [(192, cc.K3)], 72, (64, 1, 32), True),
    ((5, 4, 4), [(96, cc.K3), (48, cc.K1)], 104, (48, 3, 32), "f32"),
    ((2, 5, 9), [(64, cc.K1), (128, cc.K3)], 128, (64, 4, 64), "f32"),
    ((1, 3, 3), [(192, cc.K3)], 40, (64, 2, 32), True),
], ids=["64x1-7x7", "48x3-4x4", "64x4-5x9", "64x2-3x3"])
def test_patch_split_k(grid, segs, N, tile, res, ksplit):
    """grid.z slices add their partial sums into a zeroed acc_buf; k_conv_finish adds bias, per-sample bias and either residual
    type, writes both planes and the statistics."""
    B, H, W = grid
    case = cc.ConvCase(B=B, H=H, W=W, segs=segs, N=N, bias=True, bias_shift=4.0, tbias=True, res=res, seed=60 + ksplit)
    _run(case, tile, f"split-K {ksplit} {tile} {grid}", ksplit=ksplit, **FULL)


def test_patch_refusals():
    """Host-side checks only: nothing is launched."""
    from ctdd import unet_engine as ue
    lib = ue._lib()
    keep = []

    def refused_call(case, tile=(16, 1, 32), **fields):
        a = case.args(ue, keep)
        out = torch.full((case.M, case.N), cc.SENT, dtype=torch.bfloat16, device="cuda")
        keep.append(out)
        a.out_hi = out.data_ptr()
        for k, v in fields.items():
            setattr(a, k, v)
        msg = cc.refused(lib, lib.ctdd_unet_conv_patch(C.byref(a), *tile, cc.stream()))
        torch.cuda.synchronize()
        assert (out == cc.SENT).all().item()
        return msg
    assert "H*W=9" in refused_call(cc.ConvCase(B=2, H=3, W=3, segs=[(16, cc.K3)], N=40))           # a 32-row slice would span > 2 samples
    assert "H*W=4" in refused_call(cc.ConvCase(B=3, H=2, W=2, segs=[(16, cc.K3)], N=40))
    assert "W=34" in refused_call(cc.ConvCase(B=1, H=1, W=34, segs=[(16, cc.K3)], N=40))
    ok = cc.ConvCase(B=2, H=5, W=9, segs=[(16, cc.K3)], N=40)
    assert "N=36" in refused_call(cc.ConvCase(B=2, H=5, W=9, segs=[(16, cc.K3)], N=36))            # N % 8
    assert "BK=32" in refused_call(ok, tile=(32, 1, 32))                                          # C = 16
    assert "no patch-conv instantiation" in refused_call(ok, tile=(16, 2, 32))
    assert "stride 1" in refused_call(ok, Hin=10, Win=18)
    assert "acc_buf" in refused_call(ok, ksplit=2)
    assert "kind" in refused_call(cc.ConvCase(B=2, H=5, W=9, Hin=10, Win=18, segs=[(16, cc.KS2)], N=40), Hin=5, Win=9)
    assert "S % 8" in refused_call(cc.ConvCase(B=2, H=5, W=9, segs=[(16, cc.K3)], N=48, logits_C=4))   # S = 12
