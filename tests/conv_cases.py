"""Operands, fp64 reference and error scale of ONE call of the convolution entries (ctdd_unet_conv, ctdd_unet_conv_patch), built
from a description; shared by test_conv_cases_cpu.py (which proves the builder without a GPU) and the GPU tests of the two kernels.

A segment is (C, kind) or (C, kind, "zero") -- the latter a source of zeros with zero weights, which keeps a call off the
specialised kernels without changing any sum.  Kinds (csrc/unet_kernels.hip, SegKind):
  0  3x3, padding 1                        source grid = output grid
  1  1x1                                   source grid = output grid
  2  3x3 stride 2 on F.pad(x, [0,1,0,1])   source grid (Hin, Win), output ((Hin - 2) // 2 + 1, ...)
  3  3x3 padding 1 on the nearest-2x grid  source grid (Hin, Win) = (H / 2, W / 2)
  4  the data gradient of kind 2           source = dy on (Hin, Win), output = the stride-2 convolution's input grid (H, W)
The reference is torch.nn.functional.conv2d in fp64 on the operands as the kernel reads them (bf16-rounded in bf16 mode, plain
fp32 in fp32 mode); kind 4 is taken by autograd in fp64.  Every reference is linear in (x, w), so the same function on (|x|, |w|)
gives the error scale sum|x||w|.

Bounds (per output element; S_pre = sum|x||w| + |bias| + |tbias|, L = 1.13 >= max|gelu'| under act = 2, else 1):
  fp32 output   |got - ref| <= Ktot 2^-23 (L S_pre + |res|)  [+ 2^-22 |act(pre)| for erff under act = 2]
                -- recursive summation of Ktot products in fp32, in any order (split-K atomics included);
  bf16 output   the same + 2^-8 |ref|."""
import ctypes as C

import torch
import torch.nn.functional as F

K3, K1, KS2, KUP, KS2T = 0, 1, 2, 3, 4
SENT = 24576.0          # sentinel rows around every output (exact in bf16, far from any result)
PADROWS = 64
GELU_LIP = 1.13


def conv_ref(kind, x, w, H, W):
    """fp64 reference of one segment.  x: (B, C, Hin, Win) fp64, w: (N, C, k, k) fp64 (kind 4: the stride-2 convolution's own
    (C, N, 3, 3) weight, x = dy).  Returns (B, N, H, W)."""
    if kind == K3:
        out = F.conv2d(x, w, padding=1)
    elif kind == K1:
        out = F.conv2d(x, w)
    elif kind == KS2:
        out = F.conv2d(F.pad(x, [0, 1, 0, 1]), w, stride=2)
    elif kind == KUP:
        out = F.conv2d(x.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3), w, padding=1)
    elif kind == KS2T:
        xin = torch.zeros((x.shape[0], w.shape[1], H, W), dtype=torch.float64, requires_grad=True)
        y = F.conv2d(F.pad(xin, [0, 1, 0, 1]), w, stride=2)
        assert y.shape == x.shape, (y.shape, x.shape)
        y.backward(x)
        out = xin.grad
    else:
        raise ValueError(kind)
    assert out.shape[2:] == (H, W), (kind, out.shape, H, W)
    return out.detach()


def pack_weight(kind, w):
    """One segment's [N][ntap * C] block of the packed matrix: K runs tap, then channel.  Kind 4 ([c][tap][n] of the forward
    weight (C, N, 3, 3)): row = forward input channel, then tap, then dy channel."""
    if kind == KS2T:
        return w.permute(1, 2, 3, 0).reshape(w.shape[1], -1)
    return w.permute(0, 2, 3, 1).reshape(w.shape[0], -1)


def gelu64(v):
    return 0.5 * v * (1.0 + torch.erf(v * 0.70710678118654752))


class ConvCase:
    def __init__(self, B, H, W, segs, N, Hin=None, Win=None, f32=False, bias=False, bias_shift=0.0, tbias=False, res=False,
                 logits_C=0, act=0, seed=0):
        g = torch.Generator().manual_seed(seed)
        dt = torch.float32 if f32 else torch.bfloat16
        self.B, self.H, self.W, self.N, self.f32, self.logits_C, self.act = B, H, W, N, f32, logits_C, act
        self.Hin, self.Win = (H if Hin is None else Hin), (W if Win is None else Win)
        self.M = M = B * H * W
        self.segs = [(s[0], s[1]) for s in segs]
        self.xs, self.ws = [], []                                   # sources NHWC and conv-layout weights, as the kernel reads them
        conv = torch.zeros((B, N, H, W), dtype=torch.float64)
        scale = torch.zeros((B, N, H, W), dtype=torch.float64)
        packed = []
        Ktot_live = sum(c * (1 if k == K1 else 9) for c, k, *z in segs if not z)
        for s in segs:
            Cs, kind, zero = s[0], s[1], len(s) > 2
            hin, win = (H, W) if kind == K1 else (self.Hin, self.Win)
            k = 1 if kind == K1 else 3
            wshape = (Cs, N, 3, 3) if kind == KS2T else (N, Cs, k, k)
            if zero:
                x, w = torch.zeros((B, hin, win, Cs), dtype=dt), torch.zeros(wshape, dtype=dt)
            else:
                x = torch.randn((B, hin, win, Cs), generator=g).to(dt)
                w = (torch.randn(wshape, generator=g) / Ktot_live ** 0.5).to(dt)
            xd, wd = x.double().permute(0, 3, 1, 2), w.double()
            conv += conv_ref(kind, xd, wd, H, W)
            scale += conv_ref(kind, xd.abs(), wd.abs(), H, W)
            self.xs.append(x.contiguous())
            self.ws.append(w)
            packed.append(pack_weight(kind, w))
        self.w_packed = torch.cat(packed, 1).contiguous()            # [N][Ktot]
        self.Ktot = self.w_packed.shape[1]
        assert self.w_packed.shape[0] == N
        self.conv = conv.permute(0, 2, 3, 1).reshape(M, N)          # the bare convolution (what the packed product must equal)
        pre = self.conv.clone()
        spre = scale.permute(0, 2, 3, 1).reshape(M, N)
        self.bias = self.tbias = self.res = None
        self.tb_stride = N + 8                                       # > N (a multiple of 4: the direct epilogue's 16-byte reads)
        if bias:
            self.bias = torch.randn(N, generator=g) * 0.25 + bias_shift
            pre += self.bias.double()
            spre = spre + self.bias.double().abs()
        if tbias:
            self.tbias = torch.randn((B, self.tb_stride), generator=g) * 0.25      # (small next to bias_shift: no per-sample sum cancels)
            tb = self.tbias[:, :N].double().repeat_interleave(H * W, dim=0)
            pre += tb
            spre = spre + tb.abs()
        ref = torch.relu(pre) if act == 1 else gelu64(pre) if act == 2 else pre
        lip = GELU_LIP if act == 2 else 1.0
        extra = 2.0 ** -22 * ref.abs() if act == 2 else 0.0
        sres = 0.0
        if res:
            self.res = torch.randn((M, N), generator=g).to(torch.float32 if res == "f32" else dt)     # "f32": an fp32 residual in bf16 mode
            ref = ref + self.res.double()
            sres = self.res.double().abs()
        self.ref = ref                                               # [M][N], row-major whatever logits_C
        self.scale = spre + sres                                     # S of the module docstring
        self.bound_f32 = self.Ktot * 2.0 ** -23 * (lip * spre + sres) + extra
        self.bound_bf16 = self.bound_f32 + 2.0 ** -8 * ref.abs()

    # ------------------------------------------------------------------ layouts
    def from_layout(self, flat):
        """A kernel output ([M][N], or the (B, logits_C*H*W, S) logits layout) -> [M][N]."""
        if self.logits_C <= 0:
            return flat.reshape(self.M, self.N)
        HW, S = self.H * self.W, self.N // self.logits_C
        return flat.reshape(self.B, self.logits_C, HW, S).permute(0, 2, 1, 3).reshape(self.M, self.N)

    def sums(self, out32):
        """fp64 (sum, sum of squares) per (sample, channel) of an [M][N] fp32 output."""
        v = out32.double().reshape(self.B, self.H * self.W, self.N)
        return torch.stack([v.sum(1), (v * v).sum(1)], -1)

    # ------------------------------------------------------------------ one call on the GPU
    def args(self, ue, keep):
        """A filled _ConvArgs without outputs; device tensors are appended to `keep`."""
        a = ue._ConvArgs()
        a.nseg = len(self.segs)
        for i, ((Cs, kind), x) in enumerate(zip(self.segs, self.xs)):
            xd = x.cuda()
            keep.append(xd)
            a.seg[i].C, a.seg[i].kind = Cs, kind
            if self.f32:
                a.seg[i].f32 = xd.data_ptr()
            else:
                a.seg[i].hi = xd.data_ptr()
        wd = self.w_packed.cuda()
        keep.append(wd)
        if self.f32:
            a.w_f32 = wd.data_ptr()
        else:
            a.w_hi = wd.data_ptr()
        a.B, a.H, a.W, a.Hin, a.Win, a.N, a.Ktot = self.B, self.H, self.W, self.Hin, self.Win, self.N, self.Ktot
        a.logits_C, a.act = self.logits_C, self.act
        for name, t in (("bias", self.bias), ("tbias", self.tbias)):
            if t is not None:
                td = t.cuda()
                keep.append(td)
                setattr(a, name, td.data_ptr())
        a.tb_stride = self.tb_stride if self.tbias is not None else 0
        if self.res is not None:
            rd = self.res.cuda()
            keep.append(rd)
            if rd.dtype == torch.float32:
                a.res_f32 = rd.data_ptr()
            else:
                a.res_bf16 = rd.data_ptr()
        return a

    def run(self, call, out_f32=False, out_hi=False, out_lo=False, stats=False, ksplit=1):
        """call(args) -> return code of the entry.  Returns {"f32", "hi", "lo": [M][N] CPU tensors, "stats": (B, N, 2) fp64};
        every output buffer sits between sentinel rows, which must come back untouched."""
        from ctdd import unet_engine as ue
        lib = ue._lib()
        keep = []
        a = self.args(ue, keep)
        M, N = self.M, self.N
        bufs = {}
        for key, want, dt, field in (("f32", out_f32, torch.float32, "out_f32"), ("hi", out_hi, torch.bfloat16, "out_hi"),
                                     ("lo", out_lo, torch.bfloat16, "out_lo")):
            if want:
                bufs[key] = torch.full((M + 2 * PADROWS, N), SENT, dtype=dt, device="cuda")
                setattr(a, field, bufs[key][PADROWS:].data_ptr())
        st = None
        if stats:
            st = torch.zeros((self.B + 2, N, 2), dtype=torch.float64, device="cuda")     # a zero row on either side
            a.stats = st[1:].data_ptr()
        if ksplit > 1:
            acc = torch.zeros((M + 2 * PADROWS, N), dtype=torch.float32, device="cuda")
            bufs["acc"] = acc
            a.ksplit, a.acc_buf = ksplit, acc[PADROWS:].data_ptr()
        rc = call(a)
        assert rc == 0, lib.ctdd_last_error().decode()
        torch.cuda.synchronize()
        out = {}
        for key, buf in bufs.items():
            edge = 0.0 if key == "acc" else SENT
            assert (buf[:PADROWS] == edge).all().item() and (buf[PADROWS + M:] == edge).all().item(), f"{key}: write outside [0, M)"
            if key != "acc":
                out[key] = self.from_layout(buf[PADROWS:PADROWS + M].cpu())
        if st is not None:
            assert (st[0] == 0).all().item() and (st[-1] == 0).all().item(), "statistics outside [0, B)"
            out["stats"] = st[1:-1].cpu()
        return out

    def check(self, out, what):
        """Asserts the bounds of the module docstring on whatever `out` (of run) holds; returns the worst err / bound."""
        worst = 0.0
        if "f32" in out:
            err = (out["f32"].double() - self.ref).abs()
            ratio = (err / self.bound_f32).max().item()
            excess = (err - self.bound_f32).max().item()
            print(f"{what}: fp32 out max err {err.max().item():.3e}, worst err/bound {ratio:.3f}")
            assert excess <= 0.0, (what, "fp32", ratio, excess)
            worst = max(worst, ratio)
        if "hi" in out:
            err = (out["hi"].double() - self.ref).abs()
            ratio = (err / self.bound_bf16).max().item()
            excess = (err - self.bound_bf16).max().item()
            print(f"{what}: bf16 out max err {err.max().item():.3e}, worst err/bound {ratio:.3f}")
            assert excess <= 0.0, (what, "bf16", ratio, excess)
            worst = max(worst, ratio)
            if "f32" in out:
                assert torch.equal(out["hi"], out["f32"].to(torch.bfloat16)), (what, "out_hi != bf16(out_f32)")
        if "lo" in out:
            assert torch.equal(out["lo"], (out["f32"] - out["hi"].float()).to(torch.bfloat16)), (what, "out_lo != bf16(v - out_hi)")
        if "stats" in out:
            want = self.sums(out["f32"])
            assert (want.abs() > 0).all().item()
            rel = ((out["stats"] - want).abs() / want.abs()).max().item()
            print(f"{what}: statistics, worst relative deviation from the fp64 sums of the fp32 output {rel:.3e} (bar 1e-6)")
            assert rel <= 1e-6, (what, "statistics", rel)
        return worst


def stream():
    return torch.cuda.current_stream().cuda_stream


def refused(lib, rc):
    """An entry's refusal: a non-zero code and a message."""
    msg = lib.ctdd_last_error().decode()
    assert rc != 0 and msg, (rc, msg)
    return msg
