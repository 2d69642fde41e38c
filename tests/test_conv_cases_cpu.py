"""CPU: the case builder of the convolution kernel tests (tests/conv_cases.py) proves itself.  For every segment kind the product
of explicitly gathered patches -- index arithmetic in fp64, K ordered segment -> tap -> channel -- with the packed [N][Ktot]
weights must equal the conv2d reference to 1e-12: the tap order, the padding of each kind, the S2T transposition and the
non-square grids are settled here, without a GPU."""
import pytest
import torch

import conv_cases as cc


def _gather(case):
    """[M][Ktot] fp64: row (b, y, x) holds, per segment and tap (dy, dx), the C channels of the source pixel that tap reads
    (zeros where it reads padding)."""
    B, H, W = case.B, case.H, case.W
    cols = []
    for (Cs, kind), x in zip(case.segs, case.xs):
        x = x.double()
        hin, win = x.shape[1], x.shape[2]
        for tap in range(1 if kind == cc.K1 else 9):
            dy, dx = tap // 3, tap % 3
            blk = torch.zeros((B, H, W, Cs), dtype=torch.float64)
            for y in range(H):
                for xx in range(W):
                    if kind == cc.K1:
                        sy, sx = y, xx
                    elif kind == cc.K3:
                        sy, sx = y + dy - 1, xx + dx - 1
                    elif kind == cc.KS2:                       # padded right / bottom only: row hin is the zero row
                        sy, sx = 2 * y + dy, 2 * xx + dx
                    elif kind == cc.KUP:                       # 3x3 on the 2x grid, whose pixel (u, v) is source (u // 2, v // 2)
                        uy, ux = y + dy - 1, xx + dx - 1
                        if not (0 <= uy < H and 0 <= ux < W):
                            continue
                        sy, sx = uy // 2, ux // 2
                    else:                                      # S2T: dy pixel (sy, sx) read input (2 sy + dy, 2 sx + dx)
                        if (y - dy) % 2 or (xx - dx) % 2:
                            continue
                        sy, sx = (y - dy) // 2, (xx - dx) // 2
                    if 0 <= sy < hin and 0 <= sx < win:
                        blk[:, y, xx] = x[:, sy, sx]
            cols.append(blk.reshape(B * H * W, Cs))
    return torch.cat(cols, 1)


CASES = [
    dict(B=2, H=5, W=7, segs=[(3, cc.K3)], N=4),
    dict(B=2, H=3, W=12, segs=[(5, cc.K1)], N=3),
    dict(B=2, H=5, W=7, Hin=10, Win=14, segs=[(3, cc.KS2)], N=4),
    dict(B=2, H=3, W=2, Hin=7, Win=5, segs=[(3, cc.KS2)], N=4),              # odd source grids: the padding row is read
    dict(B=2, H=4, W=6, Hin=2, Win=3, segs=[(3, cc.KUP)], N=4),
    dict(B=2, H=5, W=7, Hin=2, Win=3, segs=[(4, cc.KS2T)], N=3),              # odd grid: the last row / column has no partner
    dict(B=2, H=4, W=6, Hin=2, Win=3, segs=[(4, cc.KS2T)], N=3),
    dict(B=3, H=3, W=3, segs=[(4, cc.K3), (2, cc.K1)], N=5),
    dict(B=2, H=2, W=5, segs=[(2, cc.K1), (4, cc.K3), (3, cc.K3)], N=5),
    dict(B=2, H=4, W=6, Hin=2, Win=3, segs=[(3, cc.KUP), (2, cc.K1)], N=4),
    dict(B=2, H=5, W=7, Hin=10, Win=14, segs=[(3, cc.KS2), (2, cc.K1, "zero")], N=4),
]


@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("kw", CASES, ids=lambda kw: "+".join(f"kind{s[1]}" for s in kw["segs"]) + f"-{kw['H']}x{kw['W']}")
def test_packed_product_of_gathered_patches_is_the_reference(kw, f32):
    case = cc.ConvCase(f32=f32, seed=3, **kw)
    A = _gather(case)
    assert A.shape == (case.M, case.Ktot) and case.w_packed.shape == (case.N, case.Ktot)
    got = A @ case.w_packed.double().T
    err = (got - case.conv).abs().max().item()
    assert case.conv.abs().max().item() > 0.1 and err <= 1e-12, err
    sc = A.abs() @ case.w_packed.double().abs().T
    assert (sc - case.scale).abs().max().item() <= 1e-12
    assert torch.equal(case.ref, case.conv) and (case.scale >= case.ref.abs() - 1e-12).all().item()
    for x in case.xs:                                           # operands are what the mode stores
        assert x.dtype == (torch.float32 if f32 else torch.bfloat16)


def test_epilogue_terms_layout_and_bounds():
    """bias + per-sample bias (row stride > N) -> activation -> residual, the logits layout's inverse, and the bounds' pieces."""
    kw = dict(B=3, H=2, W=3, segs=[(4, cc.K3)], N=6, seed=5)
    plain = cc.ConvCase(**kw)
    for act in (0, 1, 2):
        c = cc.ConvCase(bias=True, bias_shift=4.0, tbias=True, res=True, act=act, **kw)
        assert torch.equal(c.conv, plain.conv) and c.tb_stride > c.N and c.tbias.shape == (3, c.tb_stride)
        pre = c.conv + c.bias.double() + c.tbias[:, :6].double().repeat_interleave(6, dim=0)
        want = {0: pre, 1: pre.clamp(min=0), 2: torch.nn.functional.gelu(pre)}[act] + c.res.double()
        assert (c.ref - want).abs().max().item() <= 1e-12
        s_pre = plain.scale + c.bias.double().abs() + c.tbias[:, :6].double().abs().repeat_interleave(6, dim=0)
        assert (c.scale - (s_pre + c.res.double().abs())).abs().max().item() <= 1e-12
        lip = 1.13 if act == 2 else 1.0
        b32 = c.Ktot * 2.0 ** -23 * (lip * s_pre + c.res.double().abs()) + (2.0 ** -22 * (want - c.res.double()).abs() if act == 2 else 0.0)
        assert (c.bound_f32 - b32).abs().max().item() <= 1e-15
        assert (c.bound_bf16 - (b32 + 2.0 ** -8 * want.abs())).abs().max().item() <= 1e-15
    c = cc.ConvCase(logits_C=3, **kw)
    M, N, HW, S = c.M, c.N, 6, 2
    rows = torch.arange(M * N, dtype=torch.float64).reshape(M, N)          # element (p, n) of the row-major result ...
    flat = torch.empty(M * N, dtype=torch.float64)
    for p in range(M):
        for n in range(N):                                                  # ... sits at (b, c * HW + pixel, s) of (B, C*H*W, S)
            b, px, ch, s = p // HW, p % HW, n // S, n % S
            flat[((b * 3 + ch) * HW + px) * S + s] = rows[p, n]
    assert torch.equal(c.from_layout(flat), rows)
    st = c.sums(rows.float())
    assert st.shape == (3, 6, 2) and st[1, 2, 0].item() == rows[6:12, 2].sum().item()
