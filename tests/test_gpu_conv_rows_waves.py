"""GPU: the two work splits of the 28x28 GroupNorm + convolution row kernel (csrc/unet_rows_kernels.hip): ctdd_unet_conv_rows (eight
waves per workgroup, a wave owns 7 rows of the band) against ctdd_unet_conv_rows_w4 (four waves, a wave owns the band's 14 rows).
The two are held to the same bits, output and output statistics, the same refusals, and the same plans apart from the entry's
name.  What either computes is held to fp64 and to the replaced pair by tests/test_gpu_conv_rows.py, whose helpers build the cases."""
import contextlib

import pytest
import torch

from test_gpu_conv_rows import N, _case, _mnist, _run_rows

pytestmark = pytest.mark.gpu

W8, W4 = "ctdd_unet_conv_rows", "ctdd_unet_conv_rows_w4"


@contextlib.contextmanager
def _entry(name):
    """_run_rows launches lib.ctdd_unet_conv_rows: hand it a library whose entry of that name is `name`."""
    from ctdd import unet_engine as ue
    real = ue._lib()

    class Lib:
        ctdd_unet_conv_rows = getattr(real, name)
        ctdd_last_error = real.ctdd_last_error

    saved = ue._lib
    ue._lib = lambda: Lib
    try:
        yield real
    finally:
        ue._lib = saved


def _launch(name, d, fill, **over):
    """One launch of entry `name` into an output pre-filled with `fill` (64 sentinel rows behind it) and zeroed statistics."""
    M = d["B"] * d["H"] * d["W"]
    buf = torch.full((M + 64, N), fill, dtype=torch.bfloat16, device="cuda")
    stats = torch.zeros((d["B"], N, 2), dtype=torch.float64, device="cuda")
    with _entry(name) as lib:
        rc = _run_rows(d, buf, stats, **over)
        err = lib.ctdd_last_error()
    torch.cuda.synchronize()
    return rc, err, buf, stats


CASES = [  # (B, H, W, GroupNorm sources, raw 1x1 sources, residual, time-bias rows)
    (2, 28, 28, [96], [], True, 0),
    (2, 28, 28, [192, 96], [], False, 1),       # three pieces, groups straddle the sources
    (2, 28, 28, [96], [96, 96], False, 0),
    (2, 28, 28, [96], [192, 96], False, 0),
    (2, 15, 17, [96], [], True, 2),             # band 2 has one row: its lower waves own nothing, its upper waves one row
    (1, 7, 5, [96], [], False, 0),              # the lower waves own nothing at all
    (1, 8, 16, [96], [], True, 0),              # the lower waves own one row; the second column half holds one pixel
    (1, 21, 28, [96, 96], [], False, 1),        # band 2 is exactly the upper half
    (1, 1, 1, [32], [], False, 0),
]


@pytest.mark.parametrize("B,H,W,cs,rcs,res,tb_rows", CASES)
def test_eight_waves_match_four_bit_for_bit(B, H, W, cs, rcs, res, tb_rows):
    """torch.equal on the output and on out_stats (from zeroed buffers); the sentinel rows behind the output are untouched."""
    d = _case(B, H, W, cs, rcs, res, tb_rows, seed=77 + 1000 * H + 10 * W + sum(cs) + sum(rcs) + tb_rows)
    M = B * H * W
    rc8, err8, o8, s8 = _launch(W8, d, 9.0)
    rc4, err4, o4, s4 = _launch(W4, d, 9.0)
    assert rc8 == 0 and rc4 == 0, (err8, err4)
    assert bool((o8[M:] == 9.0).all()) and bool((o4[M:] == 9.0).all())
    assert bool(torch.isfinite(o8[:M].float()).all()) and bool((s4[:, :, 1] > 0).all())
    nd = int((o8[:M] != o4[:M]).sum())
    print(f"B={B} {H}x{W} C={cs} raw={rcs} res={res} tb_rows={tb_rows}: {nd} of {M * N} outputs differ, "
          f"max|stats8 - stats4| = {float((s8 - s4).abs().max()):.3e}")
    assert torch.equal(o8, o4)
    assert torch.equal(s8, s4)


@pytest.mark.parametrize("H,W,cs,rcs,res", [(28, 28, [192, 96], [], False), (15, 17, [96], [], True), (28, 28, [96], [96, 96], False)])
def test_no_state_survives_a_launch(H, W, cs, rcs, res):
    """Two launches of the eight-wave entry into outputs pre-filled with different values give identical bits: nothing of the slab,
    of the partial sums behind the output image or of the statistics scratch is read before it is written."""
    d = _case(2, H, W, cs, rcs, res, 1, seed=5 + H + sum(cs))
    M = 2 * H * W
    rc1, _, o1, s1 = _launch(W8, d, 7.0)
    rc2, _, o2, s2 = _launch(W8, d, -3.0)
    assert rc1 == 0 and rc2 == 0
    assert torch.equal(o1[:M], o2[:M]) and torch.equal(s1, s2)
    assert bool((o1[M:] == 7.0).all()) and bool((o2[M:] == -3.0).all())


def test_both_entries_refuse_alike():
    """The argument blocks of test_gpu_conv_rows.py::test_rows_refuses_what_it_does_not_take: the same non-zero code from both
    entries, nothing written."""
    d = _case(1, 28, 28, [96], [], False, 1, seed=3)
    x0 = d["x"][0].data_ptr()
    blocks = [dict(W=29), dict(N=192), dict(C1=48), dict(f32=1), dict(s1_bf16=None), dict(st1=None), dict(G=5),
              dict(RC1=96, r1_bf16=x0, res_bf16=x0)]
    for over in blocks:
        rc8, err8, o8, s8 = _launch(W8, d, 5.0, **over)
        rc4, err4, o4, s4 = _launch(W4, d, 5.0, **over)
        assert rc8 != 0 and rc8 == rc4, (over, rc8, rc4)
        assert err8 == err4
        assert bool((o8 == 5.0).all()) and bool((o4 == 5.0).all()) and not bool(s8.any()) and not bool(s4.any())


def test_plans_and_logits_of_both_wave_counts():
    """MNIST net, batch 48 (96 workgroups: the default threshold): cfg.model.conv_rows_waves = 8 (and unset) | 4 give the same plan
    labels apart from the entry's name in the ten row launches, and equal logits."""
    from ctdd.unet_engine import UNetEngine
    B = 48
    cfg, model = _mnist(0)
    assert getattr(cfg.model, "conv_rows_waves", None) is None     # the default (8) is the engine's
    g = torch.Generator(device="cuda").manual_seed(13)
    x = torch.randint(0, 256, (B, 784), device="cuda", generator=g)
    t = torch.rand(B, device="cuda", generator=g) * 0.98 + 0.01
    labels, outs = {}, {}
    for waves in (None, 8, 4):
        if waves is not None:
            cfg.model.conv_rows_waves = waves
        eng = UNetEngine(model, precision="bf16")
        with torch.no_grad():
            outs[waves] = eng(x.view(B, 1, 28, 28), t).float().clone()
        (plan,) = [v.plan if not isinstance(v, tuple) else v[1][0].plan for v in eng._plans.values()]
        labels[waves] = [s_.label for s_ in plan]
    assert labels[None] == labels[8]
    assert [lb[0] for lb in labels[8]].count(W8) == 10 and [lb[0] for lb in labels[4]].count(W4) == 10
    assert [lb[0] for lb in labels[4]].count(W8) == 0
    assert labels[8] == [(W8, lb[1]) if lb[0] == W4 else lb for lb in labels[4]]
    assert bool(torch.isfinite(outs[8]).all()) and float(outs[8].abs().max()) > 0.5
    assert torch.equal(outs[None], outs[8]) and torch.equal(outs[8], outs[4])
    cfg.model.conv_rows_waves = 6
    with pytest.raises(ValueError):
        UNetEngine(model, precision="bf16")._build(B, torch.int64, None)
