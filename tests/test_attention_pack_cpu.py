"""CPU: the weight order ctdd_unet_attention_block streams (ctdd/unet_engine.py: pack_attention_weights) against an unpacker written
from the order documented in include/ctdd_unet.h, and the coverage predicate of the launch."""
import pytest
import torch


def _unpack(wp, N, K):
    """The header's order, element by element: element (n, k), n = 16 (NT wave + tile) + i, k = 32 step + 8 q + e, at
    ((((wave * K / 32 + step) * NT + tile) * 4 + q) * 16 + i) * 8 + e, NT = N / 64."""
    NT, flat = N // 64, wp.reshape(-1)
    w = torch.zeros(N, K, dtype=wp.dtype)
    for wave in range(4):
        for step in range(K // 32):
            for tile in range(NT):
                f = flat[((wave * (K // 32) + step) * NT + tile) * 512:][:512].view(4, 16, 8)       # [q][i][e]
                n0 = 16 * (NT * wave + tile)
                w[n0:n0 + 16, 32 * step:32 * step + 32] = f.permute(1, 0, 2).reshape(16, 32)
    return w


@pytest.mark.parametrize("N,K", [(576, 192), (192, 192), (64, 32)])
def test_pack_attention_weights_is_undone_by_the_documented_order(N, K):
    from ctdd import unet_engine as ue          # (imports without a GPU: the library is loaded on first use)
    g = torch.Generator().manual_seed(N + K)
    w = torch.randn(N, K, generator=g).to(torch.bfloat16)
    wp = ue.pack_attention_weights(w)
    assert wp.shape == w.shape and wp.is_contiguous()
    assert torch.equal(_unpack(wp, N, K), w)


def test_attention_block_covers():
    from ctdd import unet_engine as ue
    cov = ue.attention_block_covers
    assert cov(49, 192, 8) and cov(64, 192, 8) and cov(25, 192, 8) and cov(36, 192, 8)
    assert not cov(65, 192, 8) and not cov(0, 192, 8) and not cov(49, 256, 8) and not cov(49, 192, 1) and not cov(49, 96, 8)
