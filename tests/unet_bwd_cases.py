"""Shared cases of the U-Net backward kernel tests (test_unet_bwd_cases_cpu.py, test_gpu_unet_bwd_fp64.py): fp64 references of
what csrc/unet_train_kernels.hip computes, written out as formulas, the case tables with the kernel each row is meant to reach,
operands drawn on the CPU from seeded generators (the same on every machine), and thin drivers that fill the argument blocks of
ctdd/unet_train.py and launch.  Nothing here touches the GPU at import; the drivers import the package inside the functions.

Tensors are NHWC with the pixels flattened: [B, HW, C].  The references take and return float64 on the operands' device.

  GroupNorm (+Swish, +dropout) backward (reference network unet.py:103-133) over the channel concatenation of one or two sources:
      xhat = (x - mean_g) rstd_g,  z = gamma xhat + beta,  a = swish(z) keep / (1 - p)
      dz = dA keep / (1 - p) swish'(z),  swish'(z) = s (1 + z (1 - s)),  s = sigmoid(z)
      dX = rstd_g (gamma dz - mean_g(gamma dz) - xhat mean_g(gamma dz xhat))
      sums[b, c] = (sum_p dz, sum_p dz xhat);  dsum[b, c] = sum_p dX
  mid-block attention (unet.py:176-200): per head q, k, v of width ch, w = softmax((q s)(k s)^T), s = ch^-1/4, out = w v
      dV = w^T dO;  dW = dO V^T;  dS = w (dW - rowsum(dW w));  dQ = s^2 dS K;  dK = s^2 dS^T Q
  first convolution (unet.py:343) on the centred state xc = 2 (x - lo) / (hi - lo) - 1, 3x3, pad 1:
      dW[n, ci, ky, kx] = sum_{b, y, x} dY[b, y, x, n] xc[b, ci, y + ky - 1, x + kx - 1];  dbias[n] = sum dY[b, y, x, n]"""
import ctypes as C
import functools

import torch
import torch.nn.functional as F

BF16_HALF_UNIT = 2.0 ** -8          # |bf16(v) - v| <= 2^-8 |v|: eight significand bits, round to nearest
F32_UNIT = 2.0 ** -24               # unit round-off of fp32: a sum of n terms in any order is within n 2^-24 sum |term|
EPS = 1e-6


# ==================================================================================================== GroupNorm backward
# (B, HW, C1, C2, G, kernel the bf16 call is meant to reach: 0 two launches | 2 / 4 / 8 one launch, what the row is for)
GN_CASES = [
    (3, 49, 96, 0, 24, 2, "one octet per slab"),
    (2, 196, 24, 0, 2, 2, "two passes, ragged second pass, 12-channel groups over 3 octets"),
    (2, 600, 24, 0, 2, 4, "ragged fourth pass"),
    (2, 784, 24, 0, 2, 8, "5 passes"),
    (2, 1360, 24, 0, 2, 8, "exactly 8 full passes"),
    (2, 1361, 24, 0, 2, 0, "no slab fits: two launches, 3 pixel slices, atomics"),
    (64, 49, 64, 0, 16, 2, "slab widened to 16 while there are >= 256 workgroups"),
    (2, 50, 8, 16, 2, 2, "slab and first group straddle the source boundary"),
    (2, 20, 16, 0, 16, 2, "one channel per group"),
    (2, 3, 32, 0, 8, 2, "3 pixels"),
    (64, 196, 192, 0, 32, 4, "slab 48 (MNIST 14x14 at batch 64)"),
    (64, 196, 192, 192, 32, 8, "slab 96, 504 of 512 threads (MNIST 14x14 up path at batch 64)"),
    (1, 20, 2048, 0, 32, 2, "bf16: 8 octets; fp32: one pixel lane, both launches over 64 KiB of LDS"),
]
# further expectations of a row's plan: (row, bf16?) -> {field of gn_plan: value}
GN_PLAN_DETAILS = {
    (0, True): dict(slab=8, octets=1),
    (1, True): dict(slab=24, octets=3, lanes=170),
    (5, True): dict(slices=3),
    (5, False): dict(slices=3),
    (3, False): dict(slices=2),
    (6, True): dict(slab=16),
    (10, True): dict(slab=48),
    (11, True): dict(slab=96, octets=12, lanes=42),
    (12, True): dict(slab=64, octets=8),
    (12, False): dict(lanes=1, slices=3),
}
GN_TWO_SOURCE = 7                    # the row of the (acc1, acc2) combinations
GN_DROPOUT_ROWS = (1, 2, 3, 5, 7)    # dropout + Swish + accumulation: one row of each kernel (2, 4, 8, two launches) + two sources
# (B, HW, C, G) of every GroupNorm the training step runs at batch 64, and the one-launch kernel the bf16 step takes
GN_TRAINING_SHAPES = {
    "mnist": [((64, 784, 96, 24), 8), ((64, 784, 192, 32), 8), ((64, 196, 192, 32), 4), ((64, 196, 288, 32), 4), ((64, 196, 384, 32), 8),
              ((64, 49, 192, 32), 2), ((64, 49, 384, 32), 2)],
    "cifar10": [((64, 1024, 128, 32), 8), ((64, 256, 256, 32), 4), ((64, 256, 512, 32), 8)],
}
P_DROP, DROP_LAYER = 0.25, 5


def gn_bwd_fp64(xs, da, gamma, beta, G, swish, keep=None, p=0.0, eps=EPS):
    """xs, da [B, HW, C] (the sources concatenated), gamma, beta [C], keep [B, HW, C] or None: all float64.
    -> dict(dx [B, HW, C], s1, s2 [B, C] = sum_p dz, sum_p dz xhat, a1, a2 = the same sums of magnitudes)"""
    assert xs.dtype == da.dtype == gamma.dtype == beta.dtype == torch.float64
    B, HW, Cc = xs.shape
    cg = Cc // G
    grp = lambda t: t.reshape(B, HW, G, cg)
    mean = grp(xs).mean((1, 3), keepdim=True)
    var = (grp(xs) ** 2).mean((1, 3), keepdim=True) - mean ** 2
    rstd = 1.0 / torch.sqrt(var.clamp_min(0.0) + eps)
    xh = ((grp(xs) - mean) * rstd).reshape(B, HW, Cc)
    dz = da
    if keep is not None:
        dz = dz * keep.to(torch.float64) / (1.0 - p)
    if swish:
        z = gamma * xh + beta
        s = torch.sigmoid(z)
        dz = dz * s * (1.0 + z * (1.0 - s))
    gdz = gamma * dz
    m1 = grp(gdz).mean((1, 3), keepdim=True)
    m2 = grp(gdz * xh).mean((1, 3), keepdim=True)
    dx = (rstd * (grp(gdz) - m1 - grp(xh) * m2)).reshape(B, HW, Cc)
    return dict(dx=dx, s1=dz.sum(1), s2=(dz * xh).sum(1), a1=dz.abs().sum(1), a2=(dz * xh).abs().sum(1))


def gn_forward_fp64(xs, gamma, beta, G, swish, keep=None, p=0.0, eps=EPS):
    """the forward those formulas differentiate, on torch's own group_norm (test_unet_bwd_cases_cpu.py: autograd of this)"""
    y = F.group_norm(xs.permute(0, 2, 1), G, gamma, beta, eps=eps).permute(0, 2, 1)
    if swish:
        y = y * torch.sigmoid(y)
    if keep is not None:
        y = y * keep.to(y.dtype) / (1.0 - p)
    return y


@functools.lru_cache(maxsize=4)
def gn_operands(row, bf16):
    """CPU tensors of one row, rounded to the tensor format: x1, x2 (or None), dA, existing gradients old1, old2 (or None) in that
    format; gamma, beta fp32."""
    B, HW, C1, C2, G = GN_CASES[row][:5]
    g = torch.Generator().manual_seed(4000 + row)
    dt = torch.bfloat16 if bf16 else torch.float32
    rnd = lambda *shape: torch.randn(shape, generator=g)
    x1 = (rnd(B, HW, C1) * 1.5 + 0.3).to(dt)
    x2 = (rnd(B, HW, C2) * 0.7 - 0.2).to(dt) if C2 else None
    da = rnd(B, HW, C1 + C2).to(dt)
    gamma, beta = 1.0 + 0.5 * rnd(C1 + C2), 0.5 * rnd(C1 + C2)
    old1 = rnd(B, HW, C1).to(dt)
    old2 = rnd(B, HW, C2).to(dt) if C2 else None
    return dict(x1=x1, x2=x2, da=da, gamma=gamma, beta=beta, old1=old1, old2=old2)


def _ptr(t):
    return None if t is None else t.data_ptr()


def gn_args(B, HW, C1, C2, G, bf16, swish=True, drop_p=0.0):
    """A _GnBwdArgs of that shape whose tensor pointers are placeholders (never followed by the plan query)."""
    from ctdd import unet_train as ut
    a = ut._GnBwdArgs()
    one = 64
    if bf16:
        a.s1_bf16, a.da_bf16, a.d1_bf16 = one, one, one
        if C2:
            a.s2_bf16, a.d2_bf16 = one, one
    else:
        a.s1_f32, a.da_f32, a.d1_f32 = one, one, one
        if C2:
            a.s2_f32, a.d2_f32 = one, one
    a.st1, a.C1, a.st2, a.C2, a.gamma, a.beta, a.sums = one, C1, one if C2 else None, C2, one, one, one
    a.B, a.HW, a.G, a.eps, a.swish, a.drop_p = B, HW, G, EPS, int(swish), drop_p
    if drop_p:
        a.rng, a.layer = one, DROP_LAYER
    return a


def gn_plan(a):
    """ctdd_unet_gn_bwd_plan of a _GnBwdArgs -> (status, dict(variant, slab, octets, lanes, slices)); host code only"""
    from ctdd import unet_train as ut
    out = (C.c_int * 5)()
    rc = ut.lib().ctdd_unet_gn_bwd_plan(C.byref(a), out)
    return rc, dict(zip(("variant", "slab", "octets", "lanes", "slices"), list(out)))


def dropout_keep(B, HW, Cc, rng, layer, p=P_DROP):
    """the keep mask [B, HW, Cc] (bool, cuda) of (rng, layer): read from ctdd_unet_dropout on a tensor of ones -- both kernels draw
    the bit of the flat element index, so no Philox stream is restated"""
    from ctdd import unet_train as ut
    ones = torch.ones((B, HW, Cc), device="cuda")
    rc = ut.lib().ctdd_unet_dropout(ones.data_ptr(), None, ones.numel(), p, rng.data_ptr(), layer, stream())
    assert rc == 0, last_error()
    torch.cuda.synchronize()
    return ones != 0


def stream():
    return torch.cuda.current_stream().cuda_stream


def last_error():
    from ctdd import native
    return native.load().ctdd_last_error().decode(errors="replace")


DSUM_PAD = 5                         # dsum_bn rows are C1 + DSUM_PAD wide


def run_gn_bwd(row, bf16, swish, acc=(0, 0), drop_p=0.0, rng=None):
    """Launch ctdd_unet_gn_bwd on one row.  -> dict: plan, rc, d1, d2, sums, dsum_bn / dsum_n and what they were prefilled with
    (single source only), the operands on the GPU."""
    from ctdd import unet_train as ut
    B, HW, C1, C2, G = GN_CASES[row][:5]
    Ct = C1 + C2
    op = {k: (v.cuda() if v is not None else None) for k, v in gn_operands(row, bf16).items()}
    xs = torch.cat([op["x1"].double()] + ([op["x2"].double()] if C2 else []), -1)
    stats = torch.stack([xs.sum(1), (xs ** 2).sum(1)], -1)                       # [B][Ct][2] fp64 sums of the rounded operands
    st1, st2 = stats[:, :C1].contiguous(), stats[:, C1:].contiguous()
    sums = torch.zeros((B, Ct, 2), device="cuda")
    d1 = op["old1"].clone()                                                       # (acc = 0: must be overwritten)
    d2 = op["old2"].clone() if C2 else None
    a = ut._GnBwdArgs()
    sfx = "bf16" if bf16 else "f32"
    for name, t in (("s1", op["x1"]), ("s2", op["x2"]), ("da", op["da"]), ("d1", d1), ("d2", d2)):
        setattr(a, f"{name}_{sfx}", _ptr(t))
    a.st1, a.C1, a.st2, a.C2 = st1.data_ptr(), C1, st2.data_ptr() if C2 else None, C2
    a.gamma, a.beta, a.B, a.HW, a.G, a.eps, a.swish = op["gamma"].data_ptr(), op["beta"].data_ptr(), B, HW, G, EPS, int(swish)
    a.sums, a.acc1, a.acc2, a.drop_p = sums.data_ptr(), acc[0], acc[1], drop_p
    if drop_p:
        a.rng, a.layer = rng.data_ptr(), DROP_LAYER
    res = dict(op=op, xs=xs, d1=d1, d2=d2, sums=sums)
    if C2 == 0:
        g = torch.Generator().manual_seed(77 + row)
        res["bn0"] = torch.randn((B, C1 + DSUM_PAD), generator=g).cuda()
        res["n0"] = torch.randn((C1,), generator=g).cuda()
        res["dsum_bn"], res["dsum_n"] = res["bn0"].clone(), res["n0"].clone()
        a.dsum_bn, a.dsum_stride, a.dsum_n = res["dsum_bn"].data_ptr(), C1 + DSUM_PAD, res["dsum_n"].data_ptr()
    res["plan_rc"], res["plan"] = gn_plan(a)
    res["rc"] = ut.lib().ctdd_unet_gn_bwd(C.byref(a), stream())
    torch.cuda.synchronize()
    return res


# ==================================================================================================== attention backward
ATTN_B = 2
# (T, C, heads, kernel: 1 the 4 x 4 register tiles | 0 a thread per score | None refused, what the row is for)
ATTN_CASES = [
    (49, 64, 4, 1, "MNIST mid block"),
    (50, 48, 2, 1, "T off the tile by two"),
    (1, 16, 2, 1, "one token: dq = dk = 0"),
    (5, 8, 2, 1, "head width 4"),
    (64, 64, 1, 1, "exactly 160 KiB of tables"),
    (49, 48, 8, 0, "head width 6"),
    (7, 18, 3, 0, "head width 6, C not a multiple of 4"),
    (65, 64, 1, 0, "tables past 160 KiB"),
    (100, 64, 1, None, "neither kernel's tables fit"),
]
ATTN_LDS = {4: 160 * 1024}           # row -> dynamic LDS bytes the plan must report
ERANGE = -34                         # CTDD_ERANGE of include/ctdd.h


def attention_fp64(qkv, heads):
    """qkv [B, T, 3C] float64, head h in columns 3 h ch .. 3 (h + 1) ch - 1 as q | k | v -> out [B, T, C]; differentiable"""
    B, T, C3 = qkv.shape
    Cc, ch = C3 // 3, C3 // 3 // heads
    x = qkv.permute(0, 2, 1).reshape(B * heads, 3 * ch, T)
    q, k, v = torch.split(x, ch, dim=1)
    s = float(ch) ** -0.25
    w = torch.softmax(torch.einsum("bct,bcs->bts", q * s, k * s), dim=-1)
    return torch.einsum("bts,bcs->bct", w, v).reshape(B, Cc, T).permute(0, 2, 1)


def attention_bwd_fp64(qkv, d_out, heads):
    """the backward as formulas (module docstring): qkv [B, T, 3C], d_out [B, T, C] float64 -> d_qkv [B, T, 3C]"""
    B, T, C3 = qkv.shape
    ch = C3 // 3 // heads
    x = qkv.reshape(B, T, heads, 3, ch)
    q, k, v = (x[:, :, :, i].permute(0, 2, 1, 3) for i in range(3))               # [B, heads, T, ch]
    dO = d_out.reshape(B, T, heads, ch).permute(0, 2, 1, 3)
    s2 = float(ch) ** -0.5
    w = torch.softmax(s2 * q @ k.transpose(-1, -2), -1)
    dV = w.transpose(-1, -2) @ dO
    dW = dO @ v.transpose(-1, -2)
    dS = w * (dW - (dW * w).sum(-1, keepdim=True))
    dQ, dK = s2 * dS @ k, s2 * dS.transpose(-1, -2) @ q
    return torch.stack([dQ, dK, dV], 3).permute(0, 2, 1, 3, 4).reshape(B, T, C3)


def attn_operands(row):
    """N(0, 1) qkv [B, T, 3C] and d_out [B, T, C], fp32 values drawn on the CPU"""
    T, Cc = ATTN_CASES[row][:2]
    g = torch.Generator().manual_seed(5000 + row)
    return torch.randn((ATTN_B, T, 3 * Cc), generator=g), torch.randn((ATTN_B, T, Cc), generator=g)


def attn_args(T, Cc, heads, B=ATTN_B):
    """placeholder-pointer _AttnBwdArgs for the plan query"""
    from ctdd import unet_train as ut
    a = ut._AttnBwdArgs()
    a.qkv, a.d_out_f32, a.d_qkv, a.B, a.T, a.C, a.heads = 64, 64, 64, B, T, Cc, heads
    return a


def attn_plan(a):
    """ctdd_unet_attention_bwd_plan -> (status, kernel, LDS bytes); host code only"""
    from ctdd import unet_train as ut
    out = (C.c_int * 2)(-1, -1)
    rc = ut.lib().ctdd_unet_attention_bwd_plan(C.byref(a), out)
    return rc, out[0], out[1]


def run_attn_bwd(qkv, d_out, heads, want_f32=True, want_bf16=False):
    """qkv fp32, d_out fp32 or bf16 (cuda) -> (rc, plan, d_qkv fp32 or None, d_qkv bf16 or None); outputs prefilled with NaN"""
    from ctdd import unet_train as ut
    B, T, Cc = d_out.shape
    a = ut._AttnBwdArgs()
    a.qkv, a.B, a.T, a.C, a.heads = qkv.data_ptr(), B, T, Cc, heads
    if d_out.dtype == torch.bfloat16:
        a.d_out_bf16 = d_out.data_ptr()
    else:
        a.d_out_f32 = d_out.data_ptr()
    of = torch.full_like(qkv, float("nan")) if want_f32 else None
    ob = torch.full_like(qkv, float("nan"), dtype=torch.bfloat16) if want_bf16 else None
    a.d_qkv, a.d_qkv_bf16 = _ptr(of), _ptr(ob)
    plan = attn_plan(a)
    rc = ut.lib().ctdd_unet_attention_bwd(C.byref(a), stream())
    torch.cuda.synchronize()
    return rc, plan, of, ob


# ==================================================================================================== first convolution
# (B, C_in, H, W, C_out): 28 rows in 8 bands of 4 (the last empty); 17 rows in bands of 3 (two empty); C_out = 256: one pixel lane;
# one band, 8 output channels; C_out that does not divide 256
FIRST_CASES = [(3, 1, 28, 28, 96), (2, 3, 17, 17, 128), (2, 4, 8, 8, 256), (2, 2, 7, 5, 8), (1, 1, 16, 16, 40)]
FIRST_LO, FIRST_HI = 0.0, 255.0


def first_wgrad_fp64(x, dy, lo=FIRST_LO, hi=FIRST_HI):
    """x [B, C_in, H, W] integer states, dy [B, H W, C_out] float64 -> (dW [C_out, C_in, 3, 3], dbias [C_out]) float64"""
    B, Cin, H, W = x.shape
    xc = 2.0 * (x.double() - lo) / (hi - lo) - 1.0
    cols = F.unfold(xc, 3, padding=1)                                             # [B, C_in 9, H W], rows (ci, ky, kx)
    return torch.einsum("bkp,bpn->nk", cols, dy).reshape(-1, Cin, 3, 3), dy.sum((0, 1))


def first_operands(row):
    B, Cin, H, W, Cout = FIRST_CASES[row]
    g = torch.Generator().manual_seed(6000 + row)
    return torch.randint(0, 256, (B, Cin, H, W), generator=g), torch.randn((B, H * W, Cout), generator=g)


def run_first_wgrad(x, dy, Cout, with_bias):
    """x int64 / int32 [B, C_in, H, W], dy fp32 / bf16 [B, H W, C_out] (cuda) -> (rc, gw [C_out, C_in, 3, 3], gbias or None)"""
    from ctdd import unet_train as ut
    lib = ut.lib()
    B, Cin, H, W = x.shape
    a = ut._FirstWgradArgs()
    if x.dtype == torch.int64:
        a.x64 = x.data_ptr()
    else:
        a.x32 = x.data_ptr()
    if dy.dtype == torch.bfloat16:
        a.dy_bf16 = dy.data_ptr()
    else:
        a.dy_f32 = dy.data_ptr()
    a.lo, a.hi, a.B, a.Cin, a.H, a.W, a.Cout = FIRST_LO, FIRST_HI, B, Cin, H, W, Cout
    gw = torch.full((Cout, Cin, 3, 3), float("nan"), device="cuda")
    gb = torch.full((Cout,), float("nan"), device="cuda") if with_bias else None
    scratch = torch.full((lib.ctdd_unet_first_conv_wgrad_scratch(B, H, Cin, Cout),), float("nan"), device="cuda")
    a.gw, a.gbias, a.partial = gw.data_ptr(), _ptr(gb), scratch.data_ptr()
    rc = lib.ctdd_unet_first_conv_wgrad(C.byref(a), stream())
    torch.cuda.synchronize()
    return rc, gw, gb


# ==================================================================================================== weight tables
# (N, Cin_tot, c_off, C, ntap, Ktot, koff, flip, ldd, has fwd, has gw): 216, 960, 1152, 2304, 70, 576 items -- every entry but the
# first starts inside a 256-item block (216, 1176, 2328, 4632, 4702), and the last block (5278 items) is ragged
PACK_ENTRIES = [
    (8, 3, 0, 3, 9, 27, 0, 1, 8, True, True),
    (24, 40, 0, 40, 1, 56, 16, 0, 32, True, True),          # koff > 0 in a wider Ktot; 8 padding columns per tap
    (16, 24, 16, 8, 9, 80, 8, 1, 16, True, True),           # c_off > 0, flipped taps
    (16, 24, 0, 16, 9, 144, 0, 0, 24, False, True),         # no forward layout; padded, unflipped
    (10, 7, 0, 7, 1, 7, 0, 0, 16, True, False),             # no packed gradient: unpack skips it
    (8, 12, 4, 8, 9, 72, 0, 1, 8, True, True),
]


def pack_table(f32):
    """The entries on the GPU: dict(tab = device bytes of the _PackEntry array, total, ents = per entry dict(w, fwd, dgrad, gw, grad))"""
    from ctdd import unet_train as ut
    dt = torch.float32 if f32 else torch.bfloat16
    g = torch.Generator().manual_seed(7000)
    ents, first = [], 0
    tab = (ut._PackEntry * len(PACK_ENTRIES))()
    for i, (N, Ct, c_off, Cc, ntap, Ktot, koff, flip, ldd, has_fwd, has_gw) in enumerate(PACK_ENTRIES):
        e = dict(w=torch.randn((N, Ct, ntap), generator=g).cuda(),
                 fwd=torch.zeros((N, Ktot), dtype=dt, device="cuda") if has_fwd else None,
                 dgrad=torch.zeros((Cc, ntap, ldd), dtype=dt, device="cuda"),
                 gw=torch.randn((N, Ktot), generator=g).cuda() if has_gw else None,
                 grad=torch.full((N, Ct, ntap), 7.0, device="cuda"))
        t = tab[i]
        t.w, t.fwd, t.dgrad, t.gw, t.grad = e["w"].data_ptr(), _ptr(e["fwd"]), e["dgrad"].data_ptr(), _ptr(e["gw"]), e["grad"].data_ptr()
        t.N, t.Cin_tot, t.c_off, t.C, t.ntap, t.Ktot, t.koff, t.flip, t.ldd, t.first = N, Ct, c_off, Cc, ntap, Ktot, koff, flip, ldd, first
        first += N * Cc * ntap
        ents.append(e)
    dev = torch.frombuffer(bytearray(bytes(tab)), dtype=torch.uint8).cuda()
    return dict(tab=dev, host=tab, total=first, ents=ents)


def packed_expect(w, entry, dt):
    """torch expression of the two packed layouts of one entry: (fwd columns koff .. koff + ntap C [N, ntap C], dgrad [C, ntap, ldd])"""
    N, Ct, c_off, Cc, ntap, Ktot, koff, flip, ldd = entry[:9]
    ws = w[:, c_off:c_off + Cc, :]                                                # [N, C, ntap]
    fwd = ws.permute(0, 2, 1).reshape(N, ntap * Cc).to(dt)
    dg = torch.zeros((Cc, ntap, ldd), dtype=dt, device=w.device)
    dg[:, :, :N] = (ws.flip(2) if flip else ws).permute(1, 2, 0).to(dt)
    return fwd, dg


def unpacked_expect(gw, entry):
    """torch expression of the slice [:, c_off : c_off + C, :] of the torch-layout gradient that unpacking writes"""
    N, Ct, c_off, Cc, ntap, Ktot, koff = entry[:7]
    return gw[:, koff:koff + ntap * Cc].reshape(N, ntap, Cc).permute(0, 2, 1)
