"""GPU: the hand-written U-Net backward kernels (csrc/unet_train_kernels.hip), one by one, against fp64 evaluations of the same
operations (tests/unet_bwd_cases.py) on every branch of their dispatch.  Each GroupNorm and attention test first asks the plan
query (ctdd_unet_gn_bwd_plan / ctdd_unet_attention_bwd_plan) which kernel its call runs and asserts that it is the one the row is
there for, so a change of the selection rule cannot silently move a row to another kernel.

Bars.  fp32 dX / d_qkv / first-conv gradients: 2e-5 of the reference tensor's largest magnitude (the project's bar for these
kernels).  bf16 dX: an ideal kernel returns bf16(ref), so per element 2^-8 |ref| (half a bf16 unit) + 2e-5 max |ref|.  fp32 sums of n
terms (`sums`, the per-sample sums of dX, the helpers): n 2^-24 sum |term|, any summation order; the GroupNorm sums add 1e-5 sum |term|
for the rounding of the terms themselves (fp32 mean / rstd, the fast sigmoid of the bf16 path).  A value that is added to counts
as one more term.  A bf16 destination of a sum adds the half unit of the result.  Copies, casts and layouts are exact (torch.equal;
bf16 = round to nearest even).

Measured on an MI355X (largest over the rows of a family; GroupNorm, first conv and helpers as a fraction of the bar; printed by every test):
  GroupNorm fp32 (two launches)      dX 0.015, sum dz 0.017, sum dz xhat 0.023, dsum_bn 0.059, dsum_n 0.018
  GroupNorm bf16, one launch         dX 0.980 (the half unit of the output itself), sum dz 0.014, sum dz xhat 0.024, dsum_bn 0.100, dsum_n 0.024
  GroupNorm bf16, two launches       dX 0.979, sums and dsum below 0.002
  attention, 4 x 4 tiles             dq / dk / dv 5.9e-7 of the tensor's range (bar 2e-5); thread per score 6.1e-7; T = 1: exact
  first conv weight / bias gradient  0.010
  colsum 0.26, sum_batch / sum_jobs 0.52, downsum2x 0.58 into fp32 and 0.996 into bf16 (its half unit); everything else exact

What this file found.  No kernel missed a bar.  The two-launch GroupNorm kernels asked for more than 64 KiB of dynamic LDS above
C = 1365 / 1536 without raising the kernels' ceiling first (the only such launches of the file); the launcher now does, and the
C = 2048 row runs them at 96 / 80 KiB."""
import pytest
import torch

import unet_bwd_cases as uc

pytestmark = pytest.mark.gpu

HALF, UNIT = uc.BF16_HALF_UNIT, uc.F32_UNIT
_refs = {}


def _rng():
    return torch.tensor([2024, 3], dtype=torch.int64, device="cuda")


def _ok(rc):
    assert rc == 0, uc.last_error()


def _worst(err, bar):
    """largest err / bar over a tensor (bar > 0 wherever err can be non-zero)"""
    return float((err / bar.clamp_min(1e-300)).max())


# ==================================================================================================== GroupNorm backward
def _gn_reference(res, row, bf16, swish, drop):
    """fp64 reference of a row on the (rounded) operands of the run; shared between the tests of the row, read-only"""
    key = (row, bf16, swish, drop)
    if _refs.get("gn_key") != key:
        B, HW, C1, C2, G = uc.GN_CASES[row][:5]
        op = res["op"]
        keep = uc.dropout_keep(B, HW, C1 + C2, _rng(), uc.DROP_LAYER) if drop else None
        if drop:
            frac = float(keep.float().mean())
            assert abs(frac - (1 - uc.P_DROP)) < 0.03, frac
        ref = uc.gn_bwd_fp64(res["xs"], op["da"].double(), op["gamma"].double(), op["beta"].double(), G, swish, keep,
                             uc.P_DROP if drop else 0.0)
        _refs["gn_key"], _refs["gn"] = key, ref
    return _refs["gn"]


def _check_gn(res, ref, row, bf16, acc, what):
    B, HW, C1, C2, G = uc.GN_CASES[row][:5]
    _ok(res["rc"])
    op = res["op"]
    figs = {}
    for name, lo, hi, got, old, ac in (("d1", 0, C1, res["d1"], op["old1"], acc[0]), ("d2", C1, C1 + C2, res["d2"], op["old2"], acc[1])):
        if hi == lo:
            continue
        want = ref["dx"][..., lo:hi] + (old.double() if ac else 0.0)
        top = float(want.abs().max())
        bar = (HALF * want.abs() if bf16 else 0.0) + torch.full_like(want, 2e-5 * top)
        figs[name] = _worst((got.double() - want).abs(), bar)
    n_bar = HW * UNIT + 1e-5
    sums = res["sums"].double()
    figs["sum dz"] = _worst((sums[..., 0] - ref["s1"]).abs(), n_bar * ref["a1"])
    figs["sum dz xhat"] = _worst((sums[..., 1] - ref["s2"]).abs(), n_bar * ref["a2"])
    if C2 == 0:
        dx = ref["dx"]
        figs["dsum_bn"] = _worst((res["dsum_bn"][:, :C1].double() - dx.sum(1)).abs(), n_bar * dx.abs().sum(1))
        assert torch.equal(res["dsum_bn"][:, C1:], res["bn0"][:, C1:]), "dsum_bn: columns beyond C1 were written"
        n0 = res["n0"].double()
        figs["dsum_n"] = _worst((res["dsum_n"].double() - (n0 + dx.sum((0, 1)))).abs(), n_bar * (dx.abs().sum((0, 1)) + n0.abs()))
    print(f"gn bwd {what} {uc.GN_CASES[row][:5]} {'bf16' if bf16 else 'fp32'} kernel {res['plan']['variant']}: "
          + ", ".join(f"{k} {v:.3f}" for k, v in figs.items()) + " of the bar")
    bad = {k: v for k, v in figs.items() if not v <= 1.0}
    assert not bad, (what, uc.GN_CASES[row], bad)


def _assert_gn_plan(res, row, bf16):
    assert res["plan_rc"] == 0, uc.last_error()
    want = uc.GN_CASES[row][5] if bf16 else 0
    assert res["plan"]["variant"] == want, (uc.GN_CASES[row], res["plan"])
    for k, v in uc.GN_PLAN_DETAILS.get((row, bf16), {}).items():
        assert res["plan"][k] == v, (k, res["plan"])


@pytest.mark.parametrize("swish", [True, False])
@pytest.mark.parametrize("bf16", [True, False])
@pytest.mark.parametrize("row", range(len(uc.GN_CASES)))
def test_groupnorm_backward(row, bf16, swish):
    """dX written over what is there (acc = 0), `sums`, and on a single source the per-sample sums of dX: dsum_bn stored into rows
    wider than C1 (the columns beyond stay), dsum_n added to what is there"""
    res = uc.run_gn_bwd(row, bf16, swish)
    _assert_gn_plan(res, row, bf16)
    _check_gn(res, _gn_reference(res, row, bf16, swish, False), row, bf16, (0, 0), "swish" if swish else "plain")


@pytest.mark.parametrize("bf16", [True, False])
@pytest.mark.parametrize("acc", [(0, 0), (1, 0), (0, 1), (1, 1)])
def test_groupnorm_backward_accumulates_per_source(acc, bf16):
    """two sources with existing non-zero gradients: each of d1 / d2 is added to or overwritten by its own flag"""
    row = uc.GN_TWO_SOURCE
    res = uc.run_gn_bwd(row, bf16, True, acc=acc)
    _assert_gn_plan(res, row, bf16)
    _check_gn(res, _gn_reference(res, row, bf16, True, False), row, bf16, acc, f"acc {acc}")


@pytest.mark.parametrize("bf16", [True, False])
@pytest.mark.parametrize("row", uc.GN_DROPOUT_ROWS)
def test_groupnorm_backward_dropout_swish_accumulate(row, bf16):
    """dropout p = 0.25 behind the Swish, added to existing gradients, on a row of each kernel; the reference applies the keep mask
    that ctdd_unet_dropout leaves on a tensor of ones with the same (rng, layer)"""
    C2 = uc.GN_CASES[row][3]
    acc = (1, 1 if C2 else 0)
    res = uc.run_gn_bwd(row, bf16, True, acc=acc, drop_p=uc.P_DROP, rng=_rng())
    _assert_gn_plan(res, row, bf16)
    _check_gn(res, _gn_reference(res, row, bf16, True, True), row, bf16, acc, "dropout")


# ==================================================================================================== attention backward
def _split(d, heads):
    B, T, C3 = d.shape
    x = d.reshape(B, T, heads, 3, C3 // 3 // heads)
    return [x[:, :, :, i] for i in range(3)]


@pytest.mark.parametrize("dout_bf16", [False, True])
@pytest.mark.parametrize("row", [i for i, c in enumerate(uc.ATTN_CASES) if c[3] is not None])
def test_attention_backward(row, dout_bf16):
    T, Cc, heads, kernel, _ = uc.ATTN_CASES[row]
    qkv, do = (t.cuda() for t in uc.attn_operands(row))
    if dout_bf16:
        do = do.to(torch.bfloat16)
    rc, plan, of, ob = uc.run_attn_bwd(qkv, do, heads, want_f32=True, want_bf16=True)
    assert plan[0] == 0 and plan[1] == kernel, plan
    if row in uc.ATTN_LDS:
        assert plan[2] == uc.ATTN_LDS[row]
    _ok(rc)
    qr = qkv.double().requires_grad_(True)
    uc.attention_fp64(qr, heads).backward(do.double())                       # (a bf16 d_out: its rounded values)
    refs = _split(qr.grad, heads)
    top = max(float(r.abs().max()) for r in refs)
    figs = []
    for name, got, ref in zip(("dq", "dk", "dv"), _split(of.double(), heads), refs):
        scale = float(ref.abs().max()) or top                                # (T = 1: dq = dk = 0 exactly; the largest of the three)
        figs.append((name, float((got - ref).abs().max()) / scale))
    print(f"attention bwd {uc.ATTN_CASES[row][:3]} kernel {'t4' if kernel else 'thread per score'} d_out {'bf16' if dout_bf16 else 'fp32'}: "
          + ", ".join(f"{n} {v:.2e}" for n, v in figs) + " of the tensor's range (bar 2e-5)")
    assert all(v <= 2e-5 for _, v in figs), figs
    assert torch.equal(ob.view(torch.int16), of.to(torch.bfloat16).view(torch.int16)), "the bf16 copy is not the rounded fp32 output"
    rc, plan2, none, only = uc.run_attn_bwd(qkv, do, heads, want_f32=False, want_bf16=True)
    _ok(rc)
    assert plan2 == plan and none is None and torch.equal(only.view(torch.int16), ob.view(torch.int16))


def test_attention_backward_refuses_what_fits_neither_kernel():
    row = [i for i, c in enumerate(uc.ATTN_CASES) if c[3] is None][0]
    T, Cc, heads = uc.ATTN_CASES[row][:3]
    qkv, do = (t.cuda() for t in uc.attn_operands(row))
    rc, plan, of, ob = uc.run_attn_bwd(qkv, do, heads, want_f32=True, want_bf16=True)
    assert plan[0] == uc.ERANGE and rc == uc.ERANGE
    assert bool(torch.isnan(of).all()) and bool(torch.isnan(ob.float()).all()), "a refused call wrote its outputs"
    assert float(torch.ones(4, device="cuda").sum()) == 4.0                  # (and the device took no launch error)


# ==================================================================================================== first convolution
@pytest.mark.parametrize("dy_bf16", [False, True])
@pytest.mark.parametrize("row", range(len(uc.FIRST_CASES)))
def test_first_conv_weight_gradient(row, dy_bf16):
    B, Cin, H, W, Cout = uc.FIRST_CASES[row]
    x, dy = (t.cuda() for t in uc.first_operands(row))
    if dy_bf16:
        dy = dy.to(torch.bfloat16)
    gw_ref, gb_ref = uc.first_wgrad_fp64(x, dy.double())
    worst = 0.0
    for xdt in (torch.int64, torch.int32):
        for with_bias in (True, False):
            rc, gw, gb = uc.run_first_wgrad(x.to(xdt), dy, Cout, with_bias)
            _ok(rc)
            ew = float((gw.double() - gw_ref).abs().max()) / (2e-5 * float(gw_ref.abs().max()) + 1e-6)
            eb = float((gb.double() - gb_ref).abs().max()) / (2e-5 * float(gb_ref.abs().max()) + 1e-6) if with_bias else 0.0
            worst = max(worst, ew, eb)
            assert ew <= 1.0 and eb <= 1.0, (uc.FIRST_CASES[row], xdt, with_bias, ew, eb)
    print(f"first conv wgrad {uc.FIRST_CASES[row]} dY {'bf16' if dy_bf16 else 'fp32'}: {worst:.3f} of the bar")


# ==================================================================================================== reductions / data movement
def _lib():
    from ctdd import unet_train as ut
    return ut.lib()


def _randn(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).cuda()


@pytest.mark.parametrize("bf16", [False, True])
def test_colsum(bf16):
    """N channels inside wider rows, per-sample and total sums added to what both outputs hold"""
    lib, B, worst = _lib(), 3, 0.0
    for HW in (5, 49, 784):
        for N in (8, 136):
            ld, stride = N + 8, N + 3
            g = _randn((B, HW, ld), 100 * HW + N)
            g = g.to(torch.bfloat16) if bf16 else g
            bn0, n0 = _randn((B, stride), 1), _randn((N,), 2)
            out_bn, out_n = bn0.clone(), n0.clone()
            _ok(lib.ctdd_unet_colsum(None if bf16 else g.data_ptr(), g.data_ptr() if bf16 else None, B, HW, N, ld, out_bn.data_ptr(), stride,
                                     out_n.data_ptr(), uc.stream()))
            torch.cuda.synchronize()
            gd = g.double()[..., :N]
            e1 = _worst((out_bn[:, :N].double() - (bn0[:, :N].double() + gd.sum(1))).abs(), (HW + 1) * UNIT * (gd.abs().sum(1) + bn0[:, :N].abs()))
            e2 = _worst((out_n.double() - (n0.double() + gd.sum((0, 1)))).abs(), (B * HW + 1) * UNIT * (gd.abs().sum((0, 1)) + n0.abs()))
            assert torch.equal(out_bn[:, N:], bn0[:, N:])
            assert e1 <= 1.0 and e2 <= 1.0, (HW, N, e1, e2)
            worst = max(worst, e1, e2)
            only = n0.clone()                                                      # one output alone
            _ok(lib.ctdd_unet_colsum(None if bf16 else g.data_ptr(), g.data_ptr() if bf16 else None, B, HW, N, ld, None, 0, only.data_ptr(),
                                     uc.stream()))
            torch.cuda.synchronize()
            assert _worst((only.double() - (n0.double() + gd.sum((0, 1)))).abs(), (B * HW + 1) * UNIT * (gd.abs().sum((0, 1)) + n0.abs())) <= 1.0
    print(f"colsum {'bf16' if bf16 else 'fp32'}: {worst:.3f} of the bar")


SUM_SHAPES = [(B, n, js, acc) for B in (1, 3, 6) for n in (1, 64, 65, 200) for js in (1, 2) for acc in (0, 1)]


def _sum_problem(B, n, js, seed):
    bstride = n * js + 5
    src = _randn((B * bstride,), seed)
    out0 = _randn((n + 3,), seed + 1)
    rows = src.reshape(B, bstride)[:, :n * js:js].double()
    return src, bstride, out0, rows.sum(0), rows.abs().sum(0)


def _check_sum(out, out0, n, acc, s, a, B, what):
    want = s + (out0[:n].double() if acc else 0.0)
    bar = (B + acc) * UNIT * (a + (out0[:n].double().abs() if acc else 0.0))
    fig = _worst((out[:n].double() - want).abs(), bar)
    assert fig <= 1.0, (what, fig)
    assert torch.equal(out[n:], out0[n:]), (what, "wrote beyond n")
    return fig


def test_sum_batch():
    lib, worst = _lib(), 0.0
    for i, (B, n, js, acc) in enumerate(SUM_SHAPES):
        src, bstride, out0, s, a = _sum_problem(B, n, js, 10 * i)
        out = out0.clone()
        _ok(lib.ctdd_unet_sum_batch(src.data_ptr(), B, bstride, js, n, out.data_ptr(), acc, uc.stream()))
        torch.cuda.synchronize()
        worst = max(worst, _check_sum(out, out0, n, acc, s, a, B, (B, n, js, acc)))
    print(f"sum_batch: {worst:.3f} of the bar")


def test_sum_jobs():
    """all 48 problems as ONE table: a problem of n outputs is ceil(n / 64) jobs (j0 = 0, 64, 128, 192: the last one ragged)"""
    from ctdd import unet_train as ut
    lib = _lib()
    probs, jobs = [], []
    for i, (B, n, js, acc) in enumerate(SUM_SHAPES):
        src, bstride, out0, s, a = _sum_problem(B, n, js, 10 * i)
        out = out0.clone()
        probs.append((out, out0, n, acc, s, a, B, src))
        for j0 in range(0, n, 64):
            q = ut._SumJob()
            q.inp, q.out, q.bstride, q.B, q.jstride, q.n, q.accumulate, q.j0 = src.data_ptr(), out.data_ptr(), bstride, B, js, n, acc, j0
            jobs.append(q)
    assert any(q.j0 > 64 for q in jobs) and any(q.j0 > 0 and q.n - q.j0 < 64 for q in jobs)      # blocks past 64; a ragged last block
    tab = (ut._SumJob * len(jobs))(*jobs)
    dev = torch.frombuffer(bytearray(bytes(tab)), dtype=torch.uint8).cuda()
    _ok(lib.ctdd_unet_sum_jobs(dev.data_ptr(), len(jobs), uc.stream()))
    torch.cuda.synchronize()
    worst = max(_check_sum(*p[:7], what=SUM_SHAPES[i]) for i, p in enumerate(probs))
    print(f"sum_jobs ({len(jobs)} jobs): {worst:.3f} of the bar")


@pytest.mark.parametrize("dst_bf16", [False, True])
@pytest.mark.parametrize("src_bf16", [False, True])
def test_accumulate_and_downsum2x(src_bf16, dst_bf16):
    lib = _lib()
    sdt, ddt = (torch.bfloat16 if b else torch.float32 for b in (src_bf16, dst_bf16))
    sp = lambda t: (None, t.data_ptr()) if t.dtype == torch.bfloat16 else (t.data_ptr(), None)
    worst = 0.0
    for acc in (0, 1):
        # dst (+)= src: one fp32 addition of the two values, rounded once into the destination format -- exact
        for n in (8, 8 * 333):
            src, dst0 = _randn((n,), 5 + n).to(sdt), _randn((n,), 6 + n).to(ddt)
            dst = dst0.clone()
            _ok(lib.ctdd_unet_accumulate(*sp(src), *sp(dst), n, acc, uc.stream()))
            torch.cuda.synchronize()
            want = (src.float() + dst0.float() if acc else src.float()).to(ddt)
            assert torch.equal(dst, want), ("accumulate", n, acc)
        # out[b, y, x] (+)= the 2 x 2 block of up: 4 (+ 1) terms
        for (B, H, W, Cc) in ((2, 3, 5, 8), (1, 7, 7, 24), (3, 1, 1, 16)):
            up = _randn((B, 2 * H, 2 * W, Cc), H * W).to(sdt)
            out0 = _randn((B, H, W, Cc), H * W + 1).to(ddt)
            out = out0.clone()
            _ok(lib.ctdd_unet_downsum2x(*sp(up), B, H, W, Cc, *sp(out), acc, uc.stream()))
            torch.cuda.synchronize()
            blocks = up.double().reshape(B, H, 2, W, 2, Cc)
            want, mag = blocks.sum((2, 4)), blocks.abs().sum((2, 4))
            if acc:
                want, mag = want + out0.double(), mag + out0.double().abs()
            bar = (4 + acc) * UNIT * mag + (HALF * want.abs() if dst_bf16 else 0.0)
            fig = _worst((out.double() - want).abs(), bar)
            assert fig <= 1.0, ("downsum2x", (B, H, W, Cc), acc, fig)
            worst = max(worst, fig)
    print(f"downsum2x {sdt} -> {ddt}: {worst:.3f} of the bar")


def test_upsample2x_f32():
    lib = _lib()
    for (B, H, W, Cc) in ((2, 3, 5, 4), (1, 7, 7, 24), (3, 1, 2, 8)):
        x = _randn((B, H, W, Cc), H + W)
        out = torch.full((B, 2 * H, 2 * W, Cc), float("nan"), device="cuda")
        _ok(lib.ctdd_unet_upsample2x_f32(x.data_ptr(), B, H, W, Cc, out.data_ptr(), uc.stream()))
        torch.cuda.synchronize()
        assert torch.equal(out, x.repeat_interleave(2, 1).repeat_interleave(2, 2))


@pytest.mark.parametrize("bf16", [False, True])
def test_cast_rows(bf16):
    lib = _lib()
    dt = torch.bfloat16 if bf16 else torch.float32
    for rows, n, ld_in, ld_out in ((7, 3, 3, 8), (5, 256, 256, 256), (33, 20, 27, 24), (2, 9, 16, 16)):
        src = _randn((rows, ld_in), n)
        out = torch.full((rows, ld_out), float("nan"), dtype=dt, device="cuda")
        _ok(lib.ctdd_unet_cast_rows(src.data_ptr(), rows, n, ld_in, ld_out, out.data_ptr() if bf16 else None, None if bf16 else out.data_ptr(),
                                    uc.stream()))
        torch.cuda.synchronize()
        want = torch.zeros((rows, ld_out), dtype=dt, device="cuda")
        want[:, :n] = src[:, :n].to(dt)
        assert torch.equal(out, want), (rows, n, ld_in, ld_out)


# ==================================================================================================== weight tables
@pytest.mark.parametrize("f32", [True, False])
def test_pack_weights(f32):
    lib = _lib()
    dt = torch.float32 if f32 else torch.bfloat16
    t = uc.pack_table(f32)
    rng = torch.tensor([99, 41], dtype=torch.int64, device="cuda")
    _ok(lib.ctdd_unet_pack_weights(t["tab"].data_ptr(), len(uc.PACK_ENTRIES), t["total"], int(f32), rng.data_ptr(), uc.stream()))
    torch.cuda.synchronize()
    assert rng.tolist() == [99, 42], "rng_bump: the step rises by exactly one, the seed stays"
    for ent, e in zip(uc.PACK_ENTRIES, t["ents"]):
        N, Ct, c_off, Cc, ntap, Ktot, koff = ent[:7]
        fwd, dg = uc.packed_expect(e["w"], ent, dt)
        assert torch.equal(e["dgrad"], dg), ("dgrad", ent)
        if e["fwd"] is not None:
            want = torch.zeros((N, Ktot), dtype=dt, device="cuda")
            want[:, koff:koff + ntap * Cc] = fwd
            assert torch.equal(e["fwd"], want), ("fwd", ent)
    _ok(lib.ctdd_unet_pack_weights(t["tab"].data_ptr(), len(uc.PACK_ENTRIES), t["total"], int(f32), None, uc.stream()))    # no counter to bump
    torch.cuda.synchronize()
    assert rng.tolist() == [99, 42]


def test_unpack_grads():
    lib = _lib()
    t = uc.pack_table(True)
    _ok(lib.ctdd_unet_unpack_grads(t["tab"].data_ptr(), len(uc.PACK_ENTRIES), t["total"], uc.stream()))
    torch.cuda.synchronize()
    for ent, e in zip(uc.PACK_ENTRIES, t["ents"]):
        N, Ct, c_off, Cc = ent[:4]
        want = torch.full_like(e["grad"], 7.0)                                     # what the table's gradients were filled with
        if e["gw"] is not None:
            want[:, c_off:c_off + Cc] = uc.unpacked_expect(e["gw"], ent)
        assert torch.equal(e["grad"], want), ("grad", ent)


def test_pack_then_unpack_returns_the_torch_layout():
    """a packed gradient laid out like the forward weights (the fp32 forward layout itself) un-packs to the parameter's slice"""
    lib = _lib()
    t = uc.pack_table(True)
    _ok(lib.ctdd_unet_pack_weights(t["tab"].data_ptr(), len(uc.PACK_ENTRIES), t["total"], 1, None, uc.stream()))
    tab = t["host"]
    for i, e in enumerate(t["ents"]):
        tab[i].gw = e["fwd"].data_ptr() if e["fwd"] is not None else None
    dev = torch.frombuffer(bytearray(bytes(tab)), dtype=torch.uint8).cuda()
    _ok(lib.ctdd_unet_unpack_grads(dev.data_ptr(), len(uc.PACK_ENTRIES), t["total"], uc.stream()))
    torch.cuda.synchronize()
    for ent, e in zip(uc.PACK_ENTRIES, t["ents"]):
        N, Ct, c_off, Cc = ent[:4]
        want = torch.full_like(e["grad"], 7.0)
        if e["fwd"] is not None:
            want[:, c_off:c_off + Cc] = e["w"][:, c_off:c_off + Cc]
        assert torch.equal(e["grad"], want), ent
