"""CPU: the weight order ctdd_unet_conv_rows streams (ctdd/unet_engine.py: pack_conv_rows_weights) against an unpacker written from the
order documented in include/ctdd_unet.h alone, and the LDS bank model (tools/lds_bank_model.py) on the kernel's fragment reads: the
address function stated in csrc/unet_rows_kernels.hip, with stride, pitch and guard position as literals."""
import importlib.util
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 96


def _unpack(wp, cs, rcs):
    """The header's order, element by element: two streams (output channels [48 s, 48 s + 48)) one after the other, each a sequence
    of 1 KiB fragments (tile, 32 channels), element (n = 48 s + 16 tile + i, k = 8 q + e of the fragment's 32) at (16 q + i) * 8 + e.
    3x3 segment: source -> 32-channel block -> dx -> dy -> tile; then the 1x1 segments: source -> block -> tile."""
    Ct, Rt = sum(cs), sum(rcs)
    w3 = torch.zeros(N, 9, Ct, dtype=wp.dtype)
    w1 = torch.zeros(N, Rt, dtype=wp.dtype)
    streams = wp.reshape(2, -1)

    def frag(s, f):
        return streams[s, f * 512:(f + 1) * 512].view(4, 16, 8).permute(1, 0, 2).reshape(16, 32)      # [q][i][e] -> [i][k]

    f, c0 = 0, 0
    for c in cs:
        for blk in range(c // 32):
            for dx in range(3):
                for dy in range(3):
                    for tile in range(3):
                        for s in range(2):
                            n0 = 48 * s + 16 * tile
                            w3[n0:n0 + 16, dy * 3 + dx, c0 + 32 * blk:c0 + 32 * blk + 32] = frag(s, f)
                        f += 1
        c0 += c
    c0 = 0
    for c in rcs:
        for blk in range(c // 32):
            for tile in range(3):
                for s in range(2):
                    n0 = 48 * s + 16 * tile
                    w1[n0:n0 + 16, c0 + 32 * blk:c0 + 32 * blk + 32] = frag(s, f)
                f += 1
        c0 += c
    assert f * 512 == streams.shape[1]
    return torch.cat([w3.reshape(N, 9 * Ct), w1], 1)


@pytest.mark.parametrize("cs", [[96], [96, 96], [192, 96]])
@pytest.mark.parametrize("raw", [False, True])
def test_pack_conv_rows_weights_is_undone_by_the_documented_order(cs, raw):
    from ctdd import unet_engine as ue          # (imports without a GPU: the library is loaded on first use)
    rcs = cs if raw else []
    K = 9 * sum(cs) + sum(rcs)
    g = torch.Generator().manual_seed(K)
    w = torch.randn(N, K, generator=g).to(torch.bfloat16)
    wp = ue.pack_conv_rows_weights(w, cs, rcs)
    assert wp.shape == w.shape and wp.is_contiguous()
    assert torch.equal(_unpack(wp, cs, rcs), w)


def test_pack_conv_rows_weights_raw_sources_of_their_own():
    """The 1x1 sources need not be the GroupNorm sources (conv2 of an up block: GroupNorm of h, 1x1 on the block's two inputs)."""
    from ctdd import unet_engine as ue
    w = torch.randn(N, 9 * 96 + 288, generator=torch.Generator().manual_seed(5)).to(torch.bfloat16)
    assert torch.equal(_unpack(ue.pack_conv_rows_weights(w, [96], [192, 96]), [96], [192, 96]), w)


def test_fragment_reads_of_the_rows_slab_are_conflict_free():
    """Lane j of column half h, padded row r, column shift dx: position 1 + 32 r + 16 h + j + dx - 1 of 224 bytes, + 16 bytes per k
    quarter, + 64 bytes per 32-channel block: 4 cycles each; 192- and 208-byte positions cost 8."""
    spec = importlib.util.spec_from_file_location("lds_bank_model", os.path.join(ROOT, "tools", "lds_bank_model.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    for r in range(16):
        for h in (0, 1):
            for dx in (-1, 0, 1):
                for blk in range(3):
                    assert m.b128_cycles(m.fragment_addr(lambda j: 1 + 32 * r + 16 * h + j + dx, 224, 64 * blk)) == 4, (r, h, dx, blk)
    assert m.b128_cycles(m.fragment_addr(lambda j: 1 + j, 192)) == 8 and m.b128_cycles(m.fragment_addr(lambda j: 1 + j, 208)) == 8


def test_conv_rows_covers():
    from ctdd.unet_engine import conv_rows_covers as cov
    assert cov(28, 28, [96], [], 96, 32) and cov(28, 28, [192, 96], [], 96, 32) and cov(28, 28, [96], [96, 96], 96, 32)
    assert cov(15, 17, [96], [], 96, 32, residual=True) and cov(100, 1, [32], [], 96, 32)
    assert not cov(28, 29, [96], [], 96, 32) and not cov(32, 32, [96], [], 96, 32)       # CIFAR rows
    assert not cov(28, 28, [96], [], 192, 32) and not cov(28, 28, [48], [], 96, 16)
    assert not cov(28, 28, [96], [], 96, 5) and not cov(28, 28, [96], [96], 96, 32, residual=True)
    assert not cov(28, 28, [192, 192, 96], [], 96, 32) and not cov(28, 28, [288, 192], [], 96, 32)
