"""GPU: the two work splits of the output head's GroupNorm + convolution row kernel (csrc/unet_head_kernels.hip):
ctdd_unet_conv_rows_head (eight waves per workgroup, a wave owns 7 rows of the band and stages them as 3 + 3 + 1) against
ctdd_unet_conv_rows_head_w4 (four waves, a wave owns the band's 14 rows).  The two are held to the same bits, the same refusals, and
the same plans apart from the entry's name.  What either computes is held to fp64 and to the replaced pair by
tests/test_gpu_conv_rows_head.py, whose helpers build the cases.  One further case holds the eight-wave ctdd_unet_conv_rows to its
4-wave entry with three samples of different statistics and groups that straddle two sources."""
import ctypes as C

import pytest
import torch

from test_gpu_conv_rows_head import _args, _case, _mnist, _stream

pytestmark = pytest.mark.gpu

H8, H4 = "ctdd_unet_conv_rows_head", "ctdd_unet_conv_rows_head_w4"
TAIL = 64                                                            # sentinel rows behind the output


def _launch(name, d, fill, f32=0, out=None, **over):
    """One launch of entry `name` into an output pre-filled with `fill` (TAIL sentinel rows behind it); `over` overrides fields of
    the argument block, `out` the output address (the refusal cases)."""
    from ctdd import unet_engine as ue
    lib = ue._lib()
    M = d["B"] * d["H"] * d["W"]
    buf = torch.full((M + TAIL, d["N"]), fill, dtype=torch.bfloat16, device="cuda")
    a = _args(d, buf if out is None else out(buf))
    if "wp_head" not in d:
        d["wp_head"] = ue.pack_conv_rows_head_weights(d["w"], d["C1"])           # (kept alive in d)
    a.w = d["wp_head"].data_ptr()
    for k, v in over.items():
        setattr(a, k, v)
    rc = getattr(lib, name)(C.byref(a), f32, _stream())
    err = lib.ctdd_last_error()
    torch.cuda.synchronize()
    return rc, err, buf


CASES = [  # (B, H, W, C1, N)
    (2, 28, 28, 96, 256),        # the workload's shape
    (2, 15, 17, 64, 160),        # band 2 has one row; last pass partial
    (1, 7, 5, 32, 32),           # the lower waves own nothing; N under one tile
    (1, 8, 16, 96, 576),         # the lower waves own one row; the second column half holds one pixel; the largest N
    (1, 21, 28, 96, 256),        # band 2 is exactly the upper half
    (1, 1, 1, 32, 96),
]


@pytest.mark.parametrize("B,H,W,C1,N", CASES)
def test_eight_waves_match_four_bit_for_bit(B, H, W, C1, N):
    """torch.equal on the whole output buffer, the sentinel rows behind the output included, which stay untouched."""
    d = _case(B, H, W, C1, N, 77 + 1000 * H + 10 * W + C1 + N)
    M = B * H * W
    rc8, err8, o8 = _launch(H8, d, 9.0)
    rc4, err4, o4 = _launch(H4, d, 9.0)
    assert rc8 == 0 and rc4 == 0, (err8, err4)
    assert bool((o8[M:] == 9.0).all()) and bool((o4[M:] == 9.0).all())
    assert bool(torch.isfinite(o8[:M].float()).all()) and not bool((o4[:M] == 9.0).any())
    print(f"B={B} {H}x{W} C1={C1} N={N}: {int((o8 != o4).sum())} of {M * N} outputs differ")
    assert torch.equal(o8, o4)


@pytest.mark.parametrize("B,H,W,C1,N", [(2, 28, 28, 96, 256), (2, 15, 17, 64, 160)])
def test_no_state_survives_a_launch(B, H, W, C1, N):
    """Two launches of the eight-wave entry into outputs pre-filled with different values give identical bits: nothing of the slab
    or of the waves' staging images is read before it is written."""
    d = _case(B, H, W, C1, N, 5 + H + C1 + N)
    M = B * H * W
    rc1, _, o1 = _launch(H8, d, 7.0)
    rc2, _, o2 = _launch(H8, d, -3.0)
    assert rc1 == 0 and rc2 == 0
    assert torch.equal(o1[:M], o2[:M])
    assert bool((o1[M:] == 7.0).all()) and bool((o2[M:] == -3.0).all())


def test_both_entries_refuse_alike():
    """The argument blocks of test_gpu_conv_rows_head.py::test_head_refuses_what_it_does_not_take: the same non-zero code and the
    same message from both entries, nothing written."""
    d = _case(1, 28, 28, 96, 256, 3)
    other, st, bias = d["x"].data_ptr(), d["st"].data_ptr(), d["bias"].data_ptr()
    blocks = [dict(f32=1), dict(W=29), dict(C1=48), dict(C1=128), dict(C2=32, s2_bf16=other, st2=st), dict(N=48), dict(N=608),
              dict(RC1=96, r1_bf16=other), dict(res_bf16=other), dict(tbias=bias), dict(out_stats=st), dict(s1_bf16=None),
              dict(st1=None), dict(w=None), dict(out=lambda buf: buf.data_ptr() + 2)]
    for over in blocks:
        rc8, err8, o8 = _launch(H8, d, 5.0, **over)
        rc4, err4, o4 = _launch(H4, d, 5.0, **over)
        assert rc8 != 0 and rc8 == rc4, (over, rc8, rc4)
        assert err8 == err4 and err8, over
        assert bool((o8 == 5.0).all()) and bool((o4 == 5.0).all())


def test_plans_and_logits_of_both_wave_counts():
    """MNIST net, batch 96 (192 workgroups: the default threshold of the head step): cfg.model.head_rows_waves = 8 (and unset) | 4
    give the same plan labels apart from the head step's entry name, and equal logits; any other value is refused."""
    from ctdd.unet_engine import HEAD_ROWS_MIN_WGS, UNetEngine
    B = 96
    assert 2 * B == HEAD_ROWS_MIN_WGS
    cfg, model = _mnist(0)
    assert getattr(cfg.model, "head_rows_waves", None) is None     # the default (8) is the engine's
    cfg.model.engine_streams = 1                                   # (one plan of 96 samples: two sub-batches of 48 are under the threshold)
    g = torch.Generator(device="cuda").manual_seed(13)
    x = torch.randint(0, 256, (B, 784), device="cuda", generator=g)
    t = torch.rand(B, device="cuda", generator=g) * 0.98 + 0.01
    labels, outs = {}, {}
    for waves in (None, 8, 4):
        if waves is not None:
            cfg.model.head_rows_waves = waves
        eng = UNetEngine(model, precision="bf16")
        with torch.no_grad():
            outs[waves] = eng(x.view(B, 1, 28, 28), t, logits_bf16=True).float().clone()
        (plan,) = [v.plan if not isinstance(v, tuple) else v[1][0].plan for v in eng._plans.values()]
        labels[waves] = [s_.label for s_ in plan]
    assert labels[None] == labels[8]
    assert [lb[0] for lb in labels[8]].count(H8) == 1 and [lb[0] for lb in labels[4]].count(H4) == 1
    assert [lb[0] for lb in labels[4]].count(H8) == 0 and labels[8][-1][0] == H8
    assert labels[8] == [(H8, lb[1]) if lb[0] == H4 else lb for lb in labels[4]]
    assert bool(torch.isfinite(outs[8]).all()) and float(outs[8].abs().max()) > 0.5
    assert torch.equal(outs[None], outs[8]) and torch.equal(outs[8], outs[4])
    cfg.model.head_rows_waves = 6
    with pytest.raises(ValueError):
        UNetEngine(model, precision="bf16")._build(B, torch.int64, None, logits_bf16=True)


def test_rows_eight_waves_match_four_three_samples_straddling_groups():
    """ctdd_unet_conv_rows against ctdd_unet_conv_rows_w4, output and out_stats bit for bit, with three samples in one launch (each
    with statistics of its own) and groups of 9 channels that straddle the two sources: the eight-wave epilogue adds the 16 lanes' fp32 sums of
    a column half from LDS in fp64, in the order of the 4-wave kernel's lane butterfly."""
    from test_gpu_conv_rows import _case as rows_case
    from test_gpu_conv_rows_waves import W4, W8, _launch as rows_launch
    d = rows_case(3, 28, 28, [192, 96], [], False, 3, seed=4242)
    M = 3 * 784
    rc8, err8, o8, s8 = rows_launch(W8, d, 9.0)
    rc4, err4, o4, s4 = rows_launch(W4, d, 9.0)
    assert rc8 == 0 and rc4 == 0, (err8, err4)
    assert bool((o8[M:] == 9.0).all()) and bool((s4[:, :, 1] > 0).all())
    assert not torch.equal(s4[0], s4[1]) and not torch.equal(s4[1], s4[2])
    assert torch.equal(o8, o4)
    assert torch.equal(s8, s4)
