"""CPU: the weight order ctdd_unet_conv_rows_head streams (ctdd/unet_engine.py: pack_conv_rows_head_weights) against an unpacker
written from the order documented in include/ctdd_unet.h alone: the [N][9 C1] matrix zero-padded to 96 passes rows, two streams of 48
output channels per pass, the streams one after the other."""
import pytest
import torch


def _unpack(wp, C1, passes):
    """The header's order, element by element: 2 passes streams (output channels [48 s, 48 s + 48)) one after the other, each a
    sequence of 1 KiB fragments (tile, 32 channels), element (n = 48 s + 16 tile + i, k = 8 q + e of the fragment's 32) at
    (16 q + i) * 8 + e; per stream: 32-channel block -> dx -> dy -> tile."""
    w3 = torch.zeros(96 * passes, 9, C1, dtype=wp.dtype)
    streams = wp.reshape(2 * passes, -1)
    for s in range(2 * passes):
        f = 0
        for blk in range(C1 // 32):
            for dx in range(3):
                for dy in range(3):
                    for tile in range(3):
                        frag = streams[s, f * 512:(f + 1) * 512].view(4, 16, 8).permute(1, 0, 2).reshape(16, 32)   # [q][i][e] -> [i][k]
                        n0 = 48 * s + 16 * tile
                        w3[n0:n0 + 16, dy * 3 + dx, 32 * blk:32 * blk + 32] = frag
                        f += 1
        assert f * 512 == streams.shape[1]
    return w3.reshape(96 * passes, 9 * C1)


@pytest.mark.parametrize("N", [96, 160, 256])
@pytest.mark.parametrize("C1", [32, 96])
def test_pack_head_weights_is_undone_by_the_documented_order(N, C1):
    from ctdd import unet_engine as ue          # (imports without a GPU: the library is loaded on first use)
    passes, K = -(-N // 96), 9 * C1
    w = torch.randn(N, K, generator=torch.Generator().manual_seed(N + C1)).to(torch.bfloat16)
    assert bool((w != 0).all())
    wp = ue.pack_conv_rows_head_weights(w, C1)
    assert wp.shape == (96 * passes, K) and wp.is_contiguous()
    back = _unpack(wp, C1, passes)
    assert torch.equal(back[:N], w)                                   # the pack inverts to the original matrix
    assert bool((back[N:] == 0).all())                                # the padding rows are zero
    assert int((wp != 0).sum()) == N * K                              # ... and nothing else is
    # the stream pair of pass p is contiguous: elements [p 96 K, (p + 1) 96 K) of the flat buffer hold rows [96 p, 96 p + 96) and
    # nothing else, in ctdd_unet_conv_rows' two-stream order
    flat = wp.reshape(-1)
    for p in range(passes):
        rows = torch.zeros(96, K, dtype=w.dtype)
        n = min(96, N - 96 * p)
        rows[:n] = w[96 * p:96 * p + n]
        assert torch.equal(flat[p * 96 * K:(p + 1) * 96 * K], ue.pack_conv_rows_weights(rows, [C1], []).reshape(-1))


def test_head_weights_of_one_pass_are_conv_rows_weights():
    from ctdd import unet_engine as ue
    w = torch.randn(96, 9 * 64, generator=torch.Generator().manual_seed(1)).to(torch.bfloat16)
    assert torch.equal(ue.pack_conv_rows_head_weights(w, 64), ue.pack_conv_rows_weights(w, [64], []))


def test_conv_rows_head_covers():
    from ctdd.unet_engine import conv_rows_head_covers as cov
    assert cov(28, 28, 96, 256, 32) and cov(15, 17, 96, 256, 32) and cov(5, 3, 32, 96, 32) and cov(9, 16, 64, 32, 32) and cov(100, 1, 96, 576, 32)
    assert not cov(28, 29, 96, 256, 32) and not cov(32, 32, 96, 256, 32)
    assert not cov(28, 28, 48, 256, 16) and not cov(28, 28, 128, 256, 32) and not cov(28, 28, 96, 256, 5)
    assert not cov(28, 28, 96, 48, 32) and not cov(28, 28, 96, 608, 32) and not cov(28, 28, 96, 16, 32)
