"""CPU, fp64: the 3x3 convolution on the nearest-2x grid (reference lib/networks/unet.py:79-85) equals the interleave of four
2x2-tap convolutions of the source whose weights ctdd.unet_engine.fold_upsample_weights sums from the original ones -- borders
included: the zero pad of the 2x grid is the zero pad of the source grid.  Also the packed [4][N][4 C] layout the kernel streams
(include/ctdd_unet.h: ctdd_unet_conv_up_phases) against an explicit index formula."""
import pytest
import torch
import torch.nn.functional as F

from ctdd.unet_engine import fold_upsample_weights


def phase_convs(x, wf):
    """x [B][C][H][W], wf [4][N][4 C] folded weights -> [B][N][2H][2W]: phase (py, px), tap (i, j) reads source pixel
    (y + py + i - 1, x + px + j - 1), zero outside the source grid."""
    B, Cn, H, W = x.shape
    N = wf.shape[1]
    xp = F.pad(x, [1, 1, 1, 1])
    out = torch.zeros((B, N, 2 * H, 2 * W), dtype=x.dtype)
    for py in range(2):
        for px in range(2):
            w = wf[2 * py + px].reshape(N, 2, 2, Cn).permute(0, 3, 1, 2)          # [N][C][i][j]
            out[:, :, py::2, px::2] = F.conv2d(xp[:, :, py:py + H + 1, px:px + W + 1], w)
    return out


@pytest.mark.parametrize("H,W", [(1, 1), (3, 5), (7, 7)])
def test_fold_identity_fp64(H, W):
    g = torch.Generator().manual_seed(100 * H + W)
    x = torch.randn((2, 3, H, W), dtype=torch.float64, generator=g)
    w = torch.randn((2, 3, 3, 3), dtype=torch.float64, generator=g)
    up = x.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)                # nearest 2x
    assert torch.equal(up, F.interpolate(x, scale_factor=2, mode="nearest"))
    want = F.conv2d(up, w, padding=1)
    got = phase_convs(x, fold_upsample_weights(w))
    assert got.shape == want.shape == (2, 2, 2 * H, 2 * W)
    err = (got - want).abs().max().item()
    print(f"{H}x{W}: max |phases - conv3x3(up2)| = {err:.3e} (max |ref| {want.abs().max().item():.3f})")
    assert err <= 1e-12


def test_fold_layout():
    """Element [2 py + px][n][(2 i + j) C + c] is the sum of W[n][c][a][b] over the 3x3 rows a that phase py's tap i covers
    ({0}, {1, 2} for py = 0; {0, 1}, {2} for py = 1) and the columns b that px's tap j covers."""
    g = torch.Generator().manual_seed(7)
    N, Cn = 2, 3
    w = torch.randn((N, Cn, 3, 3), dtype=torch.float64, generator=g)
    wf = fold_upsample_weights(w)
    assert wf.shape == (4, N, 4 * Cn) and wf.dtype == torch.float64 and wf.is_contiguous()
    cover = {(0, 0): (0,), (0, 1): (1, 2), (1, 0): (0, 1), (1, 1): (2,)}           # (phase bit, tap bit) -> 3x3 indices
    for py in range(2):
        for px in range(2):
            for n in range(N):
                for i in range(2):
                    for j in range(2):
                        for c in range(Cn):
                            want = sum(w[n, c, a, b].item() for a in cover[(py, i)] for b in cover[(px, j)])
                            got = wf[2 * py + px, n, (2 * i + j) * Cn + c].item()
                            assert abs(got - want) <= 1e-15, (py, px, n, i, j, c)
    # no two phases share their weights for asymmetric W (the GPU test relies on this to tell phases apart)
    assert all(not torch.equal(wf[p], wf[q]) for p in range(4) for q in range(p))
    # fp32 in, fp32 out (the engine folds in fp32 and rounds to bf16 once, afterwards)
    assert fold_upsample_weights(w.float()).dtype == torch.float32
