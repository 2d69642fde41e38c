"""GPU: the Downsample convolution (3x3, stride 2, input padded right/bottom by one; reference lib/networks/unet.py:88-97)
through the C entry ctdd_unet_conv, which runs bf16 calls with one CTDD_SEG_3x3_S2 segment on the stride-2 ring kernel
(k_conv_ring_s2) and everything else on the generic gather kernel (k_conv_igemm).

Reference: torch.nn.functional.conv2d in fp64 on the bf16-rounded inputs and weights, pad (0, 1, 0, 1), stride 2.
Bounds.  Both kernels round an fp32 sum of the same bf16 products to bf16; only the order of summation differs:
  per element      |new - ref| <= 2^-8 |ref| + K 2^-23 sum|x w|      (the second term in fp64, per element)
  over the tensor  max|new - ref| <= 1.5 max|old - ref|
`old` is k_conv_igemm on the same operands, reached in-process through a shape-equivalent call: a second, 1x1 segment of 16
all-zero channels with zero weights (two segments never dispatch to the ring kernel; the added products are exact zeros).

Statistics.  The epilogue sums the fp32 values it is about to round, so the fp64 sums are compared (rtol 1e-6) with fp64 sums
of the fp32 output written by the same call, and the bf16 output must be exactly that fp32 output rounded.  (Sums of the bf16
output itself differ from them by the rounding, ~2^-9 relative: not a 1e-6 comparison.)  The epilogue adds up to eight rows in
fp32 before it goes to fp64: at most 7 * 2^-24 = 4.2e-7 of sum|v|.  A purely relative bound on the sum needs sum|v| ~ |sum v|,
so the case has a bias of +4 on outputs of unit variance (per-channel means >= 2.5: no cancellation)."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

SENT = 24576.0          # sentinel rows around the output (exact in bf16, far from any result)
PADROWS = 64


def _stream():
    return torch.cuda.current_stream().cuda_stream


class _Case:
    """Operands of one convolution (bf16-rounded), its fp64 reference and the fp64 error scale sum|x w|."""

    def __init__(self, B, Hin, Cc, N, res=False, tbias=False, bias_shift=0.0, seed=0):
        g = torch.Generator().manual_seed(1000 * Hin + 10 * Cc + N + seed)
        self.B, self.Hin, self.Cc, self.N = B, Hin, Cc, N
        self.Ho = Ho = (Hin + 1 - 3) // 2 + 1
        self.M = B * Ho * Ho
        self.x = torch.randn((B, Hin, Hin, Cc), generator=g).to(torch.bfloat16)
        self.w = (torch.randn((N, Cc, 3, 3), generator=g) / (9 * Cc) ** 0.5).to(torch.bfloat16)
        self.bias = torch.randn(N, generator=g) * 0.5 + bias_shift
        self.tb_stride = N + 40
        self.tbias = torch.randn((B, self.tb_stride), generator=g) if tbias else None
        self.res = torch.randn((self.M, N), generator=g).to(torch.bfloat16) if res else None
        xin = self.x.double().permute(0, 3, 1, 2)
        ref = F.conv2d(F.pad(xin, [0, 1, 0, 1]), self.w.double(), stride=2)
        assert ref.shape[2:] == (Ho, Ho)
        ref = ref.permute(0, 2, 3, 1) + self.bias.double()
        if tbias:
            ref = ref + self.tbias[:, :N].double()[:, None, None, :]
        ref = ref.reshape(self.M, N)
        if res:
            ref = ref + self.res.double()
        self.ref = ref
        self.scale = F.conv2d(F.pad(xin.abs(), [0, 1, 0, 1]), self.w.double().abs(), stride=2).permute(0, 2, 3, 1).reshape(self.M, N)
        self.bound = 2.0 ** -8 * ref.abs() + 9 * Cc * 2.0 ** -23 * self.scale

    def run(self, old=False, want_f32=False, want_stats=False):
        """One call of ctdd_unet_conv.  Returns (bf16 output as fp32 on the CPU, fp32 output or None, statistics or None)."""
        from ctdd import unet_engine as ue
        lib = ue._lib()
        B, Hin, Ho, Cc, N, M = self.B, self.Hin, self.Ho, self.Cc, self.N, self.M
        x = self.x.cuda()
        wp = self.w.permute(0, 2, 3, 1).reshape(N, 9 * Cc)                     # [n][tap][c]
        a = ue._ConvArgs()
        keep = [x]
        if old:                                                               # + a 1x1 segment of zeros: k_conv_igemm, same sums
            wp = torch.cat([wp, torch.zeros((N, 16), dtype=torch.bfloat16)], 1)
            z = torch.zeros((B, Ho, Ho, 16), dtype=torch.bfloat16, device="cuda")
            keep.append(z)
            a.nseg = 2
            a.seg[1].hi, a.seg[1].C, a.seg[1].kind = z.data_ptr(), 16, ue.SEG_1x1
        else:
            a.nseg = 1
        wp = wp.contiguous().cuda()
        a.seg[0].hi, a.seg[0].C, a.seg[0].kind = x.data_ptr(), Cc, ue.SEG_3x3_S2
        a.w_hi = wp.data_ptr()
        a.B, a.H, a.W, a.Hin, a.Win, a.N, a.Ktot = B, Ho, Ho, Hin, Hin, N, wp.shape[1]
        bias = self.bias.cuda()
        a.bias = bias.data_ptr()
        if self.tbias is not None:
            tb = self.tbias.cuda()
            keep.append(tb)
            a.tbias, a.tb_stride = tb.data_ptr(), self.tb_stride
        if self.res is not None:
            res = self.res.cuda()
            keep.append(res)
            a.res_bf16 = res.data_ptr()
        out = torch.full((M + 2 * PADROWS, N), SENT, dtype=torch.bfloat16, device="cuda")
        a.out_hi = out[PADROWS:].data_ptr()
        out32 = stats = None
        if want_f32:
            out32 = torch.full((M + 2 * PADROWS, N), SENT, dtype=torch.float32, device="cuda")
            a.out_f32 = out32[PADROWS:].data_ptr()
        if want_stats:
            stats = torch.zeros((B, N, 2), dtype=torch.float64, device="cuda")
            a.stats = stats.data_ptr()
        rc = lib.ctdd_unet_conv(C.byref(a), 16, 1, 0, _stream())
        assert rc == 0, lib.ctdd_last_error().decode()
        torch.cuda.synchronize()
        for buf in (out, out32):                                              # no stray writes: rows < 0 and rows >= M untouched
            if buf is not None:
                assert (buf[:PADROWS] == SENT).all().item() and (buf[PADROWS + M:] == SENT).all().item(), "write outside [0, M)"
        return (out[PADROWS:PADROWS + M].float().cpu(), None if out32 is None else out32[PADROWS:PADROWS + M].cpu(),
                None if stats is None else stats.cpu())

    def check(self, got, what):
        err = (got.double() - self.ref).abs()
        excess = (err - self.bound).max().item()
        print(f"{what}: B={self.B} {self.Hin}x{self.Hin} C={self.Cc} N={self.N}: max err {err.max().item():.3e}, "
              f"max (err - bound) {excess:.3e}, max bound {self.bound.max().item():.3e}")
        assert excess <= 0.0, (what, excess)
        return err.max().item()


CASES = [
    dict(B=3, Hin=14, Cc=64, N=96),                           # four units: the three-buffer ring wraps; a tile spans three samples; partial 2nd tile
    dict(B=2, Hin=28, Cc=32, N=96),
    dict(B=2, Hin=28, Cc=32, N=64),                           # 64-column tiles
    dict(B=5, Hin=8, Cc=16, N=32),                            # H*W = 16, one unit, the column tile clamped at N
    dict(B=1, Hin=14, Cc=32, N=32),                           # first tile = last tile
    dict(B=3, Hin=14, Cc=64, N=96, res=True, tbias=True),     # residual + per-sample bias
]


@pytest.mark.parametrize("kw", CASES, ids=lambda kw: "-".join(f"{k}{v}" for k, v in kw.items()))
def test_stride2_ring_vs_fp64(kw):
    case = _Case(**kw)
    new, _, _ = case.run()
    old, _, _ = case.run(old=True)
    e_new = case.check(new, "ring")
    e_old = case.check(old, "igemm")
    print(f"max|new - ref| = {e_new:.4e}, max|old - ref| = {e_old:.4e}")
    assert e_new <= 1.5 * e_old, (e_new, e_old)


def _sums(out32, case):
    v = out32.double().reshape(case.B, case.Ho * case.Ho, case.N)
    return torch.stack([v.sum(1), (v * v).sum(1)], -1)


def test_stride2_ring_statistics():
    """GroupNorm statistics of the epilogue (the fp32-master and gn_onepass=0 plans request them), fp32 + bf16 outputs;
    twice into a zeroed pool: the same values."""
    case = _Case(B=3, Hin=14, Cc=64, N=96, bias_shift=4.0, seed=1)
    got, got32, st = case.run(want_f32=True, want_stats=True)
    got_b, got32_b, st_b = case.run(want_f32=True, want_stats=True)
    case.check(got, "ring bf16 out")
    case.check(got32, "ring fp32 out")
    assert torch.equal(got, got32.to(torch.bfloat16).float())
    want = _sums(got32, case)
    rel = ((st - want).abs() / want.abs()).max().item()
    print(f"statistics: max relative deviation from the fp64 sums of the fp32 output {rel:.3e}")
    assert (want.abs() > 0).all().item() and rel <= 1e-6, rel
    assert torch.equal(got32, got32_b) and torch.equal(got, got_b) and torch.equal(st, st_b)
    old, old32, st_old = case.run(old=True, want_f32=True, want_stats=True)
    e_new, e_old = case.check(got32, "ring fp32"), case.check(old32, "igemm fp32")
    assert (got.double() - case.ref).abs().max().item() <= 1.5 * (old.double() - case.ref).abs().max().item()
    want_old = _sums(old32, case)
    rel_old = ((st_old - want_old).abs() / want_old.abs()).max().item()
    print(f"fp32 outputs: max|new - ref| = {e_new:.4e}, max|old - ref| = {e_old:.4e}; igemm statistics deviation {rel_old:.3e}")


def test_stride2_fallback_small_grid():
    """7x7 -> 3x3 with B > 1 (H*W = 9: a 32-row slice would span four samples; odd input grid): the entry still returns
    CTDD_OK, on the generic kernel, and matches the reference."""
    case = _Case(B=4, Hin=7, Cc=32, N=64)
    got, _, _ = case.run()
    case.check(got, "fallback")
