"""CPU: the references and case tables of the U-Net backward kernel tests (tests/unet_bwd_cases.py).  The fp64 formulas agree with
torch's float64 autograd on F.group_norm, the reference attention and F.conv2d, and the two plan queries of libctdd (host code:
the library loads without a GPU) send every row of the tables, and every GroupNorm shape of a batch-64 training step, to the
kernel the row names."""
import pytest
import torch
import torch.nn.functional as F

import unet_bwd_cases as uc

REL = 1e-12


def _built():
    import os
    from ctdd import native
    if not os.path.exists(native.lib_path()):
        import __graft_entry__ as ge
        ge.build()


def _close(got, ref, what):
    scale = float(ref.abs().max())
    err = float((got - ref).abs().max())
    assert err <= REL * scale, (what, err, scale)


# ---------------------------------------------------------------------------------------------------- references
@pytest.mark.parametrize("swish", [True, False])
@pytest.mark.parametrize("row,drop", [(9, False), (7, False), (7, True)])
def test_groupnorm_formulas_match_autograd(row, drop, swish):
    """the smallest row (3 pixels) and the two-source row, with and without a keep mask"""
    B, HW, C1, C2, G = uc.GN_CASES[row][:5]
    op = uc.gn_operands(row, False)
    xs = torch.cat([op["x1"].double()] + ([op["x2"].double()] if C2 else []), -1)
    da, gamma, beta = op["da"].double(), op["gamma"].double(), op["beta"].double()
    keep = (torch.rand(xs.shape, generator=torch.Generator().manual_seed(3)) >= uc.P_DROP) if drop else None
    p = uc.P_DROP if drop else 0.0
    ref = uc.gn_bwd_fp64(xs, da, gamma, beta, G, swish, keep, p)
    xr, gr, br = (t.clone().requires_grad_(True) for t in (xs, gamma, beta))
    uc.gn_forward_fp64(xr, gr, br, G, swish, keep, p).backward(da)
    _close(ref["dx"], xr.grad, "dX")
    _close(ref["s1"].sum(0), br.grad, "dbeta = sum over samples of sum_p dz")
    _close(ref["s2"].sum(0), gr.grad, "dgamma = sum over samples of sum_p dz xhat")
    assert bool((ref["a1"] >= ref["s1"].abs()).all()) and bool((ref["a2"] >= ref["s2"].abs()).all())


def test_attention_formulas_match_autograd():
    for row in (2, 3, 6):                                          # one token; head width 4; head width 6
        T, Cc, heads = uc.ATTN_CASES[row][:3]
        qkv, do = (t.double() for t in uc.attn_operands(row))
        qr = qkv.clone().requires_grad_(True)
        uc.attention_fp64(qr, heads).backward(do)
        _close(uc.attention_bwd_fp64(qkv, do, heads), qr.grad, ("d_qkv", T, Cc, heads))
        if T == 1:                                                 # a constant softmax: dq = dk = 0
            ch = Cc // heads
            g = qr.grad.reshape(uc.ATTN_B, T, heads, 3, ch)
            assert float(g[:, :, :, :2].abs().max()) == 0.0 and float(g[:, :, :, 2].abs().max()) > 0.0


def test_attention_matches_the_network_module():
    """the head split and the ch^-1/4 scale are those of lib/networks/unet.py's SelfAttention (fp32 softmax there: 1e-6)"""
    from lib.networks.unet import SelfAttention
    torch.manual_seed(0)
    T, Cc, heads = 9, 32, 4
    m = SelfAttention(Cc, n_head=heads)
    torch.nn.init.normal_(m.proj_out.weight, std=0.2)              # (zero-initialised in the network)
    x = torch.randn(2, Cc, T)
    with torch.no_grad():
        qkv = m.qkv(m.norm(x))                                     # [B, 3C, T]
        inner = uc.attention_fp64(qkv.permute(0, 2, 1).double(), heads).permute(0, 2, 1).float()
        torch.testing.assert_close(x + m.proj_out(inner), m(x), rtol=1e-5, atol=1e-5)


def test_first_conv_formulas_match_autograd():
    row = 3                                                        # (2, 2, 7, 5, 8): the smallest
    B, Cin, H, W, Cout = uc.FIRST_CASES[row]
    x, dy = uc.first_operands(row)
    dy = dy.double()
    gw, gb = uc.first_wgrad_fp64(x, dy)
    w = torch.zeros((Cout, Cin, 3, 3), dtype=torch.float64, requires_grad=True)
    b = torch.zeros((Cout,), dtype=torch.float64, requires_grad=True)
    xc = 2.0 * (x.double() - uc.FIRST_LO) / (uc.FIRST_HI - uc.FIRST_LO) - 1.0
    F.conv2d(xc, w, b, padding=1).backward(dy.reshape(B, H, W, Cout).permute(0, 3, 1, 2))
    _close(gw, w.grad, "dW")
    _close(gb, b.grad, "dbias")


def test_pack_expressions_round_trip():
    """the torch expressions of the packed layouts invert each other: unpacking the forward layout returns the parameter slice"""
    g = torch.Generator().manual_seed(1)
    for ent in uc.PACK_ENTRIES:
        N, Ct, c_off, Cc, ntap, Ktot, koff, flip, ldd = ent[:9]
        w = torch.randn((N, Ct, ntap), generator=g)
        fwd, dg = uc.packed_expect(w, ent, torch.float32)
        full = torch.zeros((N, Ktot))
        full[:, koff:koff + ntap * Cc] = fwd
        assert torch.equal(uc.unpacked_expect(full, ent), w[:, c_off:c_off + Cc])
        assert dg.shape == (Cc, ntap, ldd) and float(dg[:, :, N:].abs().sum()) == 0.0
        tp = ntap - 1 if flip else 0
        assert torch.equal(dg[:, tp, :N], w[:, c_off:c_off + Cc, 0].T)
    firsts = [0]
    for ent in uc.PACK_ENTRIES:
        firsts.append(firsts[-1] + ent[0] * ent[3] * ent[4])
    assert len(uc.PACK_ENTRIES) >= 5 and all(f % 256 for f in firsts[1:])


# ---------------------------------------------------------------------------------------------------- plan queries
@pytest.mark.parametrize("bf16", [True, False])
@pytest.mark.parametrize("row", range(len(uc.GN_CASES)))
def test_groupnorm_plan_of_every_row(row, bf16):
    _built()
    B, HW, C1, C2, G, variant, _ = uc.GN_CASES[row]
    rc, plan = uc.gn_plan(uc.gn_args(B, HW, C1, C2, G, bf16))
    assert rc == 0, uc.last_error()
    assert plan["variant"] == (variant if bf16 else 0), plan        # fp32 tensors always take the two launches
    Ct = C1 + C2
    assert Ct % plan["slab"] == 0 and plan["slab"] % (Ct // G) == 0 and plan["octets"] * 8 == plan["slab"]
    if plan["variant"]:
        assert plan["slices"] == 1 and plan["octets"] * plan["lanes"] <= 512
        passes = -(-HW // plan["lanes"])
        assert passes <= plan["variant"] and (plan["variant"] == 2 or passes > plan["variant"] // 2), (plan, passes)
    else:
        assert plan["slab"] == Ct and plan["lanes"] == 256 // (Ct // 8)
    for k, v in uc.GN_PLAN_DETAILS.get((row, bf16), {}).items():
        assert plan[k] == v, (k, plan)


def test_groupnorm_plan_of_the_training_shapes():
    """every GroupNorm of a batch-64 MNIST / CIFAR-10 step runs a kernel that a GPU row of the same precision reaches"""
    _built()
    reached = {r[5] for r in uc.GN_CASES}
    assert reached == {0, 2, 4, 8}
    for name, shapes in uc.GN_TRAINING_SHAPES.items():
        for (B, HW, Cc, G), variant in shapes:
            rc, plan = uc.gn_plan(uc.gn_args(B, HW, Cc, 0, G, True))
            assert rc == 0 and plan["variant"] == variant and variant in reached, (name, B, HW, Cc, G, plan)
            rc, plan = uc.gn_plan(uc.gn_args(B, HW, Cc, 0, G, False))
            assert rc == 0 and plan["variant"] == 0, (name, B, HW, Cc, G, plan)


def test_groupnorm_plan_makes_the_launchers_checks():
    _built()
    EINVAL = -22
    bad = uc.gn_args(2, 49, 96, 0, 24, True)
    bad.sums = None
    assert uc.gn_plan(bad)[0] == EINVAL
    assert uc.gn_plan(uc.gn_args(2, 49, 100, 0, 25, True))[0] == EINVAL          # C not a multiple of 8
    assert uc.gn_plan(uc.gn_args(2, 49, 96, 0, 36, True))[0] == EINVAL           # groups do not divide C
    assert uc.gn_plan(uc.gn_args(2, 49, 2056, 0, 8, True))[0] == EINVAL          # C > 2048
    two = uc.gn_args(2, 49, 64, 32, 8, True)
    two.dsum_n = 64
    assert uc.gn_plan(two)[0] == EINVAL                                          # per-sample sums of dX: single source only
    drop = uc.gn_args(2, 49, 96, 0, 24, True, drop_p=0.25)
    assert uc.gn_plan(drop)[0] == 0
    drop.rng = None
    assert uc.gn_plan(drop)[0] == EINVAL
    mixed = uc.gn_args(2, 49, 96, 0, 24, True)                                   # an fp32 output beside bf16 tensors: two launches
    mixed.d1_f32 = 64
    assert uc.gn_plan(mixed) == (0, dict(variant=0, slab=96, octets=12, lanes=21, slices=1))


@pytest.mark.parametrize("row", range(len(uc.ATTN_CASES)))
def test_attention_plan_of_every_row(row):
    _built()
    T, Cc, heads, kernel, _ = uc.ATTN_CASES[row]
    rc, t4, lds = uc.attn_plan(uc.attn_args(T, Cc, heads))
    if kernel is None:
        assert rc == uc.ERANGE
        return
    assert rc == 0 and t4 == kernel, (rc, t4, lds)
    ch, Tp = Cc // heads, (T + 3) & ~3
    want = 4 * (4 * ch * Tp + 3 * T * ch + 3 * T * Tp) if kernel else 4 * (4 * T * ch + 2 * T * T)
    assert lds == want and lds <= 160 * 1024
    if row in uc.ATTN_LDS:
        assert lds == uc.ATTN_LDS[row]
    if not kernel:                                                 # reached for the stated reason
        assert ch % 4 != 0 or 4 * (4 * ch * Tp + 3 * T * ch + 3 * T * Tp) > 160 * 1024


def test_attention_plan_of_the_training_shapes():
    """7x7 (MNIST) and 8x8 (CIFAR-10) mid blocks with the configurations' 8 heads take a kernel that a GPU row reaches"""
    _built()
    reached = {r[3] for r in uc.ATTN_CASES}
    for T, Cc, heads in ((49, 192, 8), (49, 384, 8), (64, 256, 8), (64, 512, 8)):
        rc, t4, lds = uc.attn_plan(uc.attn_args(T, Cc, heads, B=64))
        assert rc == 0 and t4 in reached, (T, Cc, heads, rc, t4, lds)
    assert uc.attn_plan(uc.attn_args(49, 64, 3))[0] == -22         # heads do not divide C
    nothing = uc.attn_args(49, 64, 4)
    nothing.d_qkv = None
    assert uc.attn_plan(nothing)[0] == -22                         # no output requested
