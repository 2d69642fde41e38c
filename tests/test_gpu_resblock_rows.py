"""GPU: the fused ResBlock kernels on their row tiles (csrc/unet_resblock_kernels.hip): ctdd_unet_resblock_mid with one tile per
output row on a slab of 16 positions per padded row, ctdd_unet_resblock_small with tiles of 16 consecutive slab rows.  Non-square
and narrow grids, sources of 96 channels, lanes on border positions: accuracy against torch fp64 by the criterion of
tests/test_gpu_resblock_mid.py (e_new <= 1.5 e_old, e_old the four launches the kernel replaces, or, where those refuse the shape,
a torch restatement that rounds a1, h1, a2 and the output to bf16), rows around the output untouched, idempotence, and the
engine's cover function against the launcher."""
import ctypes as C
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

N = 192
SENTINEL = -1234.0


def _stream():
    return torch.cuda.current_stream().cuda_stream


@functools.lru_cache(maxsize=None)
def _block(B, H, W, cs, seed):
    """Random bf16-valued inputs and parameters of one ResBlock at H x W (NHWC sources, [N][K] weights, K = segment -> tap -> channel),
    affine GroupNorms, a time-bias row per sample, and its fp64 evaluation.  Shared between the tests; inputs and reference are never
    modified (the packed weights are added to it on first use)."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    rn = lambda *s: torch.randn(s, device="cuda", generator=g)
    C1, C2 = cs[0], (cs[1] if len(cs) > 1 else 0)
    Ct, skip = C1 + C2, C2 > 0 or C1 != N
    d = {"B": B, "H": H, "W": W, "C1": C1, "C2": C2, "skip": skip, "cs": list(cs)}
    d["x1"] = rn(B * H * W, C1).to(torch.bfloat16)
    d["x2"] = rn(B * H * W, C2).to(torch.bfloat16) if C2 else None
    d["g1"], d["be1"] = 1.0 + 0.3 * rn(Ct), 0.3 * rn(Ct)
    d["g2"], d["be2"] = 1.0 + 0.3 * rn(N), 0.3 * rn(N)
    d["w1"] = (rn(N, 9 * Ct) / (9 * Ct) ** 0.5).to(torch.bfloat16)
    K2 = 9 * N + (Ct if skip else 0)
    d["w2"] = (rn(N, K2) / K2 ** 0.5).to(torch.bfloat16)
    d["b1"], d["b2"] = 0.1 * rn(N), 0.1 * rn(N)
    d["tb"] = 0.5 * rn(B, N)
    d["ref"] = _torch_block(d, round_bf16=False)
    return d


def _torch_block(d, round_bf16):
    """The block in torch fp64 from the bf16-valued inputs; round_bf16: a1, h1, a2 and the output rounded to bf16 (the rounding points
    of the four launches)."""
    import torch.nn.functional as F
    B, H, W, C1, C2 = d["B"], d["H"], d["W"], d["C1"], d["C2"]
    Ct = C1 + C2
    rb = (lambda v: v.to(torch.bfloat16).double()) if round_bf16 else (lambda v: v)
    x = d["x1"].double() if d["x2"] is None else torch.cat([d["x1"].double(), d["x2"].double()], 1)
    x = x.view(B, H, W, Ct).permute(0, 3, 1, 2)
    w4 = lambda w, c: w.double().view(N, 3, 3, c).permute(0, 3, 1, 2)
    a1 = rb(F.silu(F.group_norm(x, 32, d["g1"].double(), d["be1"].double(), 1e-5)))
    h = rb(F.conv2d(a1, w4(d["w1"], Ct), d["b1"].double(), padding=1) + d["tb"].double()[:, :, None, None])
    a2 = rb(F.silu(F.group_norm(h, 32, d["g2"].double(), d["be2"].double(), 1e-5)))
    y = F.conv2d(a2, w4(d["w2"][:, :9 * N], N), d["b2"].double(), padding=1)
    y = rb(y + (F.conv2d(x, d["w2"][:, 9 * N:].double().view(N, Ct, 1, 1)) if d["skip"] else x))
    return y.permute(0, 2, 3, 1).reshape(B * H * W, N)


def _args(d, out, mid, H=None, W=None):
    from ctdd import unet_engine as ue
    a = ue._ResblockArgs()
    a.s1_bf16, a.C1 = d["x1"].data_ptr(), d["C1"]
    if d["x2"] is not None:
        a.s2_bf16, a.C2 = d["x2"].data_ptr(), d["C2"]
    a.gamma1, a.beta1, a.gamma2, a.beta2 = d["g1"].data_ptr(), d["be1"].data_ptr(), d["g2"].data_ptr(), d["be2"].data_ptr()
    a.G1, a.G2, a.eps1, a.eps2 = 32, 32, 1e-5, 1e-5
    key = "packed_mid" if mid else "packed_small"
    if key not in d:                                                             # (kept alive in d)
        d[key] = ue.pack_resblock_mid_weights(d["w1"], d["w2"], d["cs"]) if mid else (ue.pack_resblock_weights(d["w1"]),
                                                                                    ue.pack_resblock_weights(d["w2"]))
    w1p, w2p = d[key]
    a.w1, a.bias1, a.tbias, a.tb_stride = w1p.data_ptr(), d["b1"].data_ptr(), d["tb"].data_ptr(), N
    a.w2, a.bias2, a.skip = w2p.data_ptr(), d["b2"].data_ptr(), int(d["skip"])
    a.B, a.H, a.W, a.N, a.out_bf16 = d["B"], H or d["H"], W or d["W"], N, out.data_ptr()
    return a


def _run(d, out, mid, H=None, W=None):
    from ctdd import unet_engine as ue
    lib = ue._lib()
    a = _args(d, out, mid, H, W)
    return (lib.ctdd_unet_resblock_mid if mid else lib.ctdd_unet_resblock_small)(C.byref(a), 0, _stream())


def _four_launches(d, patch):
    """One-pass GroupNorm + Swish, patch convolution, twice; None when one of the launches refuses the shape (nothing further is
    launched then)."""
    from ctdd import unet_engine as ue
    lib = ue._lib()
    B, H, W, C1, C2 = d["B"], d["H"], d["W"], d["C1"], d["C2"]
    Ct, M = C1 + C2, B * H * W
    a1 = torch.empty((M, Ct), dtype=torch.bfloat16, device="cuda")
    h = torch.empty((M, N), dtype=torch.bfloat16, device="cuda")
    a2 = torch.empty((M, N), dtype=torch.bfloat16, device="cuda")
    y = torch.empty((M, N), dtype=torch.bfloat16, device="cuda")

    def gn(s1, c1, s2, c2, gamma, beta, out):
        g = ue._GnArgs()
        g.s1_bf16, g.C1 = s1.data_ptr(), c1
        if s2 is not None:
            g.s2_bf16, g.C2 = s2.data_ptr(), c2
        g.gamma, g.beta, g.B, g.HW, g.G, g.eps, g.swish, g.out_hi = gamma.data_ptr(), beta.data_ptr(), B, H * W, 32, 1e-5, 1, out.data_ptr()
        return lib.ctdd_unet_gn_onepass(C.byref(g), 0, 512, _stream()) == 0

    def conv(segs, w, bias, out, tb=None, res=None):
        c = ue._ConvArgs()
        c.nseg = len(segs)
        for i, (src, cs, kind) in enumerate(segs):
            c.seg[i].hi, c.seg[i].C, c.seg[i].kind = src.data_ptr(), cs, kind
        c.w_hi, c.B, c.H, c.W, c.Hin, c.Win, c.N, c.Ktot = w.data_ptr(), B, H, W, H, W, N, w.shape[1]
        c.bias, c.out_hi = bias.data_ptr(), out.data_ptr()
        if tb is not None:
            c.tbias, c.tb_stride = tb.data_ptr(), N
        if res is not None:
            c.res_bf16 = res.data_ptr()
        return lib.ctdd_unet_conv_patch(C.byref(c), *patch, _stream()) == 0

    segs = [(a2, N, ue.SEG_3x3)]
    if d["skip"]:
        segs.append((d["x1"], C1, ue.SEG_1x1))
        if C2:
            segs.append((d["x2"], C2, ue.SEG_1x1))
    ok = (gn(d["x1"], C1, d["x2"], C2, d["g1"], d["be1"], a1) and conv([(a1, Ct, ue.SEG_3x3)], d["w1"], d["b1"], h, tb=d["tb"])
          and gn(h, N, None, 0, d["g2"], d["be2"], a2) and conv(segs, d["w2"], d["b2"], y, res=None if d["skip"] else d["x1"]))
    return y if ok else None


def _check_accuracy(B, H, W, cs, mid):
    from ctdd import unet_engine as ue
    d = _block(B, H, W, tuple(cs), 7000 + 100 * H + 10 * W + sum(cs) + B)
    ref, M = d["ref"], B * H * W
    old = _four_launches(d, (48, 3, 64) if mid else (64, 1, 32))
    how = "four launches"
    if old is None:
        old, how = _torch_block(d, round_bf16=True), "torch restatement with bf16 rounding points"
    buf = torch.full((M + 2 * H * W, N), SENTINEL, dtype=torch.bfloat16, device="cuda")
    out = buf[H * W:H * W + M]
    assert _run(d, out, mid) == 0, ue._lib().ctdd_last_error()
    torch.cuda.synchronize()
    new = out.double()
    scale = float(ref.abs().max())
    e_old, e_new = float((old.double() - ref).abs().max()), float((new - ref).abs().max())
    print(f"{'mid' if mid else 'small'} B={B} {H}x{W} C={cs}: e_old={e_old:.4e} ({how}) e_new={e_new:.4e} max|fp64|={scale:.3f}")
    assert bool((buf[:H * W] == SENTINEL).all()) and bool((buf[H * W + M:] == SENTINEL).all())    # border lanes store nothing
    assert bool(torch.isfinite(new).all())
    assert e_old < 5e-2 * scale
    assert e_new <= 1.5 * e_old


MID_CASES = [  # (H, W, sources)
    (14, 14, [96]),             # a source of three 32-channel blocks: nothing padded
    (14, 14, [192, 96]),
    (5, 14, [192, 192]),        # H < 14: row tiles skipped
    (14, 3, [192]),             # a narrow grid: most lanes on positions that are not pixels
    (2, 2, [192, 96]),          # the smallest grid the small kernel leaves to this one by its channels
    (13, 11, [192]),            # odd pitch
]
SMALL_CASES = [(7, 7, [192]), (7, 7, [192, 192]), (5, 7, [192]), (3, 3, [192, 192])]


@pytest.mark.parametrize("H,W,cs", MID_CASES)
def test_mid_rows_match_fp64(H, W, cs):
    _check_accuracy(3 if H * W > 100 else 2, H, W, cs, mid=True)


@pytest.mark.parametrize("H,W,cs", SMALL_CASES)
def test_small_rows_match_fp64(H, W, cs):
    _check_accuracy(3, H, W, cs, mid=False)


@pytest.mark.parametrize("H,W,cs,mid", [(5, 14, [192, 192], True), (7, 7, [192, 192], False)])
def test_rows_idempotent(H, W, cs, mid):
    """Two launches into differently pre-filled outputs: bit-identical (no stale slab, border or guard-row state)."""
    d = _block(2 if mid else 3, H, W, tuple(cs), 7000 + 100 * H + 10 * W + sum(cs) + (2 if mid else 3))
    M = d["B"] * H * W
    o1 = torch.full((M, N), 7.0, dtype=torch.bfloat16, device="cuda")
    o2 = torch.full((M, N), -3.0, dtype=torch.bfloat16, device="cuda")
    assert _run(d, o1, mid) == 0
    first = o1.clone()
    assert _run(d, o1, mid) == 0 and _run(d, o2, mid) == 0
    torch.cuda.synchronize()
    assert torch.equal(first, o1) and torch.equal(o1, o2)
    assert bool(torch.isfinite(o1.float()).all())


def test_mid_cover_function_agrees_with_the_launcher():
    """resblock_mid_covers against the launcher's verdict; a refusal launches nothing, leaves the output untouched and sets
    ctdd_last_error.  Shapes the kernel holds are launched on data of their own shape; the others are only asked about."""
    from ctdd import unet_engine as ue
    lib = ue._lib()
    d14 = _block(3, 14, 14, (192, 96), 7000 + 1400 + 140 + 288 + 3)
    for (H, W) in [(14, 14), (13, 13), (8, 24), (15, 15), (14, 16)]:
        covers = ue.resblock_mid_covers(H, W, [192, 96], N, 32, 32)
        assert covers == (H <= 14 and W <= 14)
        out = torch.full((3 * H * W, N), 5.0, dtype=torch.bfloat16, device="cuda")
        if covers:
            d = d14 if (H, W) == (14, 14) else _block(3, H, W, (192, 96), 7000 + 100 * H + 10 * W + 288 + 3)
            assert _run(d, out, True) == 0, lib.ctdd_last_error()
            torch.cuda.synchronize()
            assert not bool((out == 5.0).all())
        else:
            assert _run(d14, out, True, H=H, W=W) != 0
            assert f"{H}x{W}".encode() in lib.ctdd_last_error()
            torch.cuda.synchronize()
            assert bool((out == 5.0).all())
