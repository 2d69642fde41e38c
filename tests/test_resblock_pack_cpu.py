"""CPU: the weight order ctdd_unet_resblock_mid streams (ctdd/unet_engine.py: pack_resblock_mid_weights) against an unpacker written
from the order documented in include/ctdd_unet.h, and the LDS bank model (tools/lds_bank_model.py) on the fragment reads of both
fused ResBlock kernels: the address functions stated in the kernels' comments, with stride, pitch and first row as literals."""
import importlib.util
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 192


def _model():
    spec = importlib.util.spec_from_file_location("lds_bank_model", os.path.join(ROOT, "tools", "lds_bank_model.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _unpack(w1p, w2p, cs, skip):
    """The header's order, element by element: per wave the stream is a sequence of 1 KiB fragments (tile, 32 channels), element
    (n = 48 wave + 16 tile + i, k = 8 q + e of the fragment's 32) at (16 q + i) * 8 + e.  3x3 segment: source -> 32-channel block ->
    dx -> dy -> tile; skip: source -> block -> tile."""
    Ct = sum(cs)
    w1 = torch.zeros(N, 9, Ct, dtype=w1p.dtype)
    w2 = torch.zeros(N, 9 * N + (Ct if skip else 0), dtype=w2p.dtype)
    w2a = w2[:, :9 * N].view(N, 9, N)
    s1, s2 = w1p.reshape(4, -1), w2p.reshape(4, -1)

    def frag(stream, wave, f):
        return stream[wave, f * 512:(f + 1) * 512].view(4, 16, 8)       # [q][i][e]

    def seg3(stream, f0, dst, c0, c):
        f = f0
        for blk in range(c // 32):
            for dx in range(3):
                for dy in range(3):
                    for tile in range(3):
                        for wave in range(4):
                            n0 = 48 * wave + 16 * tile
                            dst[n0:n0 + 16, dy * 3 + dx, c0 + 32 * blk:c0 + 32 * blk + 32] = \
                                frag(stream, wave, f).permute(1, 0, 2).reshape(16, 32)
                        f += 1
        return f

    f, c0 = 0, 0
    for c in cs:
        f = seg3(s1, f, w1, c0, c)
        c0 += c
    assert f * 512 == s1.shape[1]
    f = seg3(s2, 0, w2a, 0, N)
    if skip:
        c0 = 0
        for c in cs:
            for blk in range(c // 32):
                for tile in range(3):
                    for wave in range(4):
                        n0 = 48 * wave + 16 * tile
                        w2[n0:n0 + 16, 9 * N + c0 + 32 * blk:9 * N + c0 + 32 * blk + 32] = frag(s2, wave, f).permute(1, 0, 2).reshape(16, 32)
                    f += 1
            c0 += c
    assert f * 512 == s2.shape[1]
    return w1.reshape(N, 9 * Ct), w2


# ([64, 32]: two sources of different sizes, each of its own number of blocks -- the source -> block order)
@pytest.mark.parametrize("cs", [[192], [192, 96], [96], [64, 32]])
@pytest.mark.parametrize("skip", [True, False])
def test_pack_mid_weights_is_undone_by_the_documented_order(cs, skip):
    from ctdd import unet_engine as ue          # (imports without a GPU: the library is loaded on first use)
    Ct = sum(cs)
    g = torch.Generator().manual_seed(Ct + skip)
    w1 = torch.randn(N, 9 * Ct, generator=g).to(torch.bfloat16)
    w2 = torch.randn(N, 9 * N + (Ct if skip else 0), generator=g).to(torch.bfloat16)
    w1p, w2p = ue.pack_resblock_mid_weights(w1, w2, cs)
    assert w1p.shape == w1.shape and w2p.shape == w2.shape and w1p.is_contiguous() and w2p.is_contiguous()
    u1, u2 = _unpack(w1p, w2p, cs, skip)
    assert torch.equal(u1, w1) and torch.equal(u2, w2)


def test_fragment_reads_are_conflict_free_in_both_kernels():
    m = _model()
    # k_resblock_mid: tile y, tap (dy, dx): lane j reads slab row 1 + 16 (y + 1 + dy) + j + dx (one guard row, pitch 16), stride 416
    for y in range(14):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                assert m.b128_cycles(m.fragment_addr(lambda j: 1 + 16 * (y + 1 + dy) + j + dx, 416)) == 4, (y, dy, dx)
    # k_resblock_small<4> at 7x7: tile pt, tap (dy, dx): lane j reads slab row 10 + 16 pt + j + 9 dy + dx, clamped to [10, 70];
    # strides 416 (192 channels) and 800 (384 channels)
    for rs in (416, 800):
        for pt in range(4):
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    assert m.b128_cycles(m.fragment_addr(lambda j: min(10 + 16 * pt + j, 70) + 9 * dy + dx, rs)) == 4, (rs, pt, dy, dx)
    # every k quarter offset (the second k half is + 64 bytes, the channel blocks + 64 / + 128): no change
    for koff in (64, 128, 320):
        assert m.b128_cycles(m.fragment_addr(lambda j: 17 + j, 416, koff)) == 4


def test_model_pins_the_layout_it_replaced():
    """400-byte rows and flattened 16-pixel tiles at 14x14: 12 cycles for each of the twelve full tiles, 148 for the thirteen."""
    m = _model()
    cyc = [m.b128_cycles(m.fragment_addr(m.flat_row(pt, 14, 14), 400)) for pt in range(13)]
    assert cyc[:12] == [12] * 12 and sum(cyc) == 148
    assert m.b128_cycles(lambda lane: lane * 16) == 4                   # 64 consecutive 16-byte reads
    assert m.b128_cycles(lambda lane: (lane & 15) * 256) == 64          # 16 rows on the same banks: 16-way in every group
