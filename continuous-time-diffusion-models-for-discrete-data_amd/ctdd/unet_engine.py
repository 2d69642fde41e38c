"""Hand-written HIP inference engine for the tauLDR U-Net (lib/networks/unet.py; reference
TAUnSDDM/lib/networks/unet.py:303-459 + lib/models/models.py:225-292).

The engine walks the module tree of a built model once, packs every weight into the layouts the
kernels of csrc/unet_kernels.hip stream (implicit-GEMM [N][K] bf16 hi/lo, K = segment -> tap ->
channel), allocates all intermediate NHWC tensors for a given batch size, and records the forward
as a flat list of pre-bound launches.  The list is captured into a HIP graph (torch.cuda.CUDAGraph
is the capture API; every node is one of our kernels) and replayed per call, so a sampler step costs
one graph launch instead of ~150 Python-side launches.

precision = "bf16":  bf16 activations / weights on v_mfma_f32_32x32x16_bf16, fp32 accumulate (the
                     BASELINE config's dtype; throughput path)
precision = "fp32":  fp32 activations / weights on the exact-fp32 v_mfma_f32_32x32x2_f32 -- the path
                     the 1e-4 logit parity test runs.
"""
import contextlib
import ctypes as C

import torch

from . import native
from .plan_launch import bound_launch, graph_capture, ptr, unwrap as _unwrap

_P, _I, _F = C.c_void_p, C.c_int, C.c_float
SEG_3x3, SEG_1x1, SEG_3x3_S2, SEG_3x3_UP = 0, 1, 2, 3


class _Seg(C.Structure):
    _fields_ = [("hi", _P), ("f32", _P), ("C", _I), ("kind", _I)]


class _ConvArgs(C.Structure):
    _fields_ = [("seg", _Seg * 3), ("nseg", _I), ("w_hi", _P), ("w_f32", _P), ("B", _I), ("H", _I), ("W", _I),
                ("Hin", _I), ("Win", _I), ("N", _I), ("Ktot", _I), ("bias", _P), ("tbias", _P), ("tb_stride", _I),
                ("res_f32", _P), ("res_bf16", _P), ("out_f32", _P), ("out_hi", _P), ("stats", _P), ("logits_C", _I),
                ("ksplit", _I), ("acc_buf", _P), ("act", _I), ("out_lo", _P)]


class _FirstArgs(C.Structure):
    _fields_ = [("x64", _P), ("x32", _P), ("lo", _F), ("hi", _F), ("w", _P), ("bias", _P), ("B", _I), ("Cin", _I),
                ("H", _I), ("W", _I), ("Cout", _I), ("out_f32", _P), ("out_hi", _P), ("stats", _P), ("x0_f32", _P)]


class _GnArgs(C.Structure):
    _fields_ = [("s1_f32", _P), ("s1_bf16", _P), ("st1", _P), ("C1", _I), ("s2_f32", _P), ("s2_bf16", _P), ("st2", _P),
                ("C2", _I), ("gamma", _P), ("beta", _P), ("B", _I), ("HW", _I), ("G", _I), ("eps", _F), ("swish", _I),
                ("out_hi", _P), ("out_f32", _P)]


class _ResblockArgs(C.Structure):
    _fields_ = [("s1_bf16", _P), ("s2_bf16", _P), ("C1", _I), ("C2", _I), ("gamma1", _P), ("beta1", _P), ("gamma2", _P), ("beta2", _P),
                ("G1", _I), ("G2", _I), ("eps1", _F), ("eps2", _F), ("w1", _P), ("bias1", _P), ("tbias", _P), ("tb_stride", _I),
                ("w2", _P), ("bias2", _P), ("skip", _I), ("B", _I), ("H", _I), ("W", _I), ("N", _I), ("out_bf16", _P)]


class _ConvRowsArgs(C.Structure):
    _fields_ = [("s1_bf16", _P), ("st1", _P), ("C1", _I), ("s2_bf16", _P), ("st2", _P), ("C2", _I), ("gamma", _P), ("beta", _P), ("G", _I),
                ("eps", _F), ("w", _P), ("bias", _P), ("tbias", _P), ("tb_stride", _I), ("r1_bf16", _P), ("RC1", _I), ("r2_bf16", _P),
                ("RC2", _I), ("res_bf16", _P), ("out_bf16", _P), ("out_stats", _P), ("B", _I), ("H", _I), ("W", _I), ("N", _I)]


class _TimeArgs(C.Structure):
    _fields_ = [("t", _P), ("B", _I), ("ch", _I), ("tdim", _I), ("w1", _P), ("b1", _P), ("w2", _P), ("b2", _P),
                ("hid", _P), ("act", _P)]


class _AttnArgs(C.Structure):
    _fields_ = [("qkv", _P), ("B", _I), ("T", _I), ("C", _I), ("heads", _I), ("out_hi", _P), ("out_f32", _P)]


class _AttnBlockArgs(C.Structure):
    _fields_ = [("an_bf16", _P), ("x_bf16", _P), ("w_qkv", _P), ("b_qkv", _P), ("w_proj", _P), ("b_proj", _P), ("B", _I), ("T", _I),
                ("C", _I), ("heads", _I), ("out_bf16", _P)]


class _LogisticArgs(C.Structure):
    _fields_ = [("net", _P), ("x0", _P), ("B", _I), ("C", _I), ("HW", _I), ("S", _I), ("fix", _I), ("out", _P), ("fast", _I), ("out_bf16", _P)]


_sigs_done = False


def _lib():
    global _sigs_done
    lib = native.load()
    if not _sigs_done:
        for name, argt in (("ctdd_unet_conv", [_P, _I, _I, _I, _P]), ("ctdd_unet_conv_patch", [_P, _I, _I, _I, _P]), ("ctdd_unet_conv_res", [_P, _I, _P]), ("ctdd_unet_conv_ring", [_P, _I, _P]),
                           ("ctdd_unet_conv_up_phases", [_P, _I, _P]), ("ctdd_unet_upsample2x", [_P, _I, _I, _I, _I, _P, _P]), ("ctdd_unet_first_conv", [_P, _P]),
                           ("ctdd_unet_gn_apply", [_P, _P]), ("ctdd_unet_gn_onepass", [_P, _I, _I, _P]), ("ctdd_unet_channel_stats", [_P, _I, _I, _I, _P, _P]),
                           ("ctdd_unet_time", [_P, _P, _P, _I, _P, _P]), ("ctdd_unet_time_uniform", [_P, _P, _P, _I, _P, _P]),
                           ("ctdd_unet_attention", [_P, _P]), ("ctdd_unet_attention_block", [_P, _I, _P]),
                           ("ctdd_unet_resblock_small", [_P, _I, _P]),
                           ("ctdd_unet_resblock_mid", [_P, _I, _P]), ("ctdd_unet_conv_rows", [_P, _I, _P]), ("ctdd_unet_conv_rows_w4", [_P, _I, _P]),
                           ("ctdd_unet_conv_rows_head", [_P, _I, _P]), ("ctdd_unet_conv_rows_head_w4", [_P, _I, _P]),
                           ("ctdd_unet_logistic_head", [_P, _P])):
            fn = getattr(lib, name)
            fn.argtypes, fn.restype = argt, _I
        _sigs_done = True
    return lib


def supports(model):
    """The engine covers the reference's image U-Net wrapper without padding."""
    net = _unwrap(getattr(model, "net", None))
    return (net is not None and net.__class__.__name__ == "UNet" and not model.padding
            and model.cfg.model.model_output in ("logits", "logistic_pars"))


def training_supported(model):
    """Whether the hand-written training plan (forward that keeps what backward needs + HIP backward) covers this model:
    the same U-Nets as the inference engine with channel counts in multiples of 16."""
    if getattr(model.cfg.model, "engine_train", "hip") != "hip" or not supports(model):
        return False
    net = _unwrap(model.net)
    return net.channel % 16 == 0 and all((net.channel * int(m_)) % 16 == 0 for m_ in model.cfg.model.ch_mult)



def resblock_small_covers(H, W, cs, cout, G1, G2):
    """Shapes ctdd_unet_resblock_small holds (csrc/unet_resblock_kernels.hip): a sample of <= 64 pixels in rows of <= 8 whose interior
    spans at most 80 rows of the zero-bordered slab (five tiles of 16 consecutive rows; one tile of flattened pixels for <= 16
    pixels), 192 output channels, one or two sources in multiples of 64 channels (<= 384 in all), and its LDS image (row stride
    2 C + 32 bytes) within the CU's 160 KiB."""
    Ct = sum(cs)
    if H * W > 64 or W > 8 or cout != 192 or len(cs) > 2 or any(c % 64 for c in cs) or Ct > 384 or Ct % G1 or cout % G2:
        return False
    if H * W > 16 and (H - 1) * (W + 2) + W > 80:
        return False
    rs_a, rs_2, prows = Ct * 2 + 32, cout * 2 + 32, (H + 2) * (W + 2)
    return H * W * rs_a + prows * max(rs_a, rs_2) + 256 * 80 + 2 * 384 * 8 + 2 * 384 * 4 <= 160 * 1024


def pack_resblock_weights(w2d):
    """[192][K] (K % 64 == 0) -> the fragment order ctdd_unet_resblock_small streams (include/ctdd_unet.h): [wave][chunk][tile][k half]
    [q][i][8], so that every wave-instruction of the weight stream reads 1 KiB of consecutive bytes."""
    N, K = w2d.shape
    assert N == 192 and K % 64 == 0
    return w2d.reshape(4, 3, 16, K // 64, 2, 4, 8).permute(0, 3, 1, 4, 5, 2, 6).contiguous().reshape(N, K)


def attention_block_covers(T, Cn, heads):
    """Shapes ctdd_unet_attention_block holds (csrc/unet_attn_kernels.hip): a sample of <= 64 tokens, 192 channels in 8 heads (the
    heads' fp32 [q | k | v] regions of 64 tokens fill 152 KiB of the CU's 160 KiB of LDS)."""
    return bool(1 <= T <= 64 and Cn == 192 and heads == 8)


def pack_attention_weights(w2d):
    """[N][C] (N % 64 == 0, C % 32 == 0: the qkv or proj matrix of the attention block) -> the fragment order ctdd_unet_attention_block
    streams (include/ctdd_unet.h): [wave][k step][tile][q][i][8], wave w holding output channels [N / 4 w, N / 4 (w + 1)), so that every
    wave-instruction of the weight stream reads 1 KiB of consecutive bytes."""
    N, K = w2d.shape
    assert N % 64 == 0 and K % 32 == 0
    return w2d.reshape(4, N // 64, 16, K // 32, 4, 8).permute(0, 3, 1, 4, 2, 5).contiguous().reshape(N, K)


def resblock_mid_covers(H, W, cs, cout, G1, G2):
    """Shapes ctdd_unet_resblock_mid holds (csrc/unet_resblock_kernels.hip): a sample of <= 14 x 14 pixels (one row tile per output row
    on a slab of 16 positions per padded grid row), 192 output channels, one or two sources in multiples of 32 channels (<= 192
    each), and its LDS image (the 192-channel slab with its two guard rows + the reduction scratch) within the CU's 160 KiB."""
    Ct = sum(cs)
    if (H < 1 or W < 1 or H > 14 or W > 14 or cout != 192 or not 1 <= len(cs) <= 2
            or any(c <= 0 or c % 32 or c > 192 for c in cs) or G1 <= 0 or G2 <= 0 or Ct % G1 or cout % G2):
        return False
    return ((H + 2) * 16 + 2) * (cout * 2 + 32) + 256 * 80 + 2 * 384 * 8 + 2 * 384 * 4 <= 160 * 1024


def pack_row_tile_weights(w, cs, rcs, streams):
    """The [48 streams][9 sum(cs) + sum(rcs)] matrix of a convolution (K = the 3x3 segment as tap -> channel of the concatenation of `cs`,
    then the 1x1 segments on `rcs`) in the order the row-tile K loops stream it (include/ctdd_unet.h; csrc/row_tile.hpp): one stream
    per 48 output channels -- four waves of ctdd_unet_resblock_mid, two channel groups of ctdd_unet_conv_rows -- holding the 3x3 segment
    as source -> 32-channel block -> dx -> dy -> 16-channel tile, then the 1x1 segments as source -> 32-channel block -> tile, every
    (tile, 32 channels) fragment as [q][i][8] (1 KiB of consecutive bytes per wave-instruction).  Nothing is padded.  Returned as an
    [N][K] view of the flat streams ([streams][48 K])."""
    N, Ct, Rt = w.shape[0], sum(cs), sum(rcs)
    assert N == 48 * streams and w.shape[1] == 9 * Ct + Rt and all(c % 32 == 0 for c in [*cs, *rcs])
    w3, parts, c0 = w[:, :9 * Ct].reshape(N, 9, Ct), [], 0
    for c in cs:
        v = w3[:, :, c0:c0 + c].reshape(streams, 3, 16, 3, 3, c // 32, 4, 8)        # stream, tile, i, dy, dx, block, q, e
        parts.append(v.permute(0, 5, 4, 3, 1, 6, 2, 7).reshape(streams, -1))        # stream, block, dx, dy, tile, q, i, e
        c0 += c
    c0 = 9 * Ct
    for c in rcs:
        v = w[:, c0:c0 + c].reshape(streams, 3, 16, c // 32, 4, 8)                  # stream, tile, i, block, q, e
        parts.append(v.permute(0, 3, 1, 4, 2, 5).reshape(streams, -1))              # stream, block, tile, q, i, e
        c0 += c
    return torch.cat(parts, 1).contiguous().reshape(N, w.shape[1])


def pack_resblock_mid_weights(w1, w2, cs):
    """ctdd_unet_resblock_mid's [192][9 Ct] conv1 matrix and [192][9 * 192 (+ Ct)] conv2 matrix (3x3 on a2, then the 1x1 skip segments
    on the sources): pack_row_tile_weights, one stream per wave."""
    N = w1.shape[0]
    return pack_row_tile_weights(w1, cs, [], 4), pack_row_tile_weights(w2, [N], cs if w2.shape[1] > 9 * N else [], 4)


def pack_conv_rows_weights(w, cs, rcs):
    """ctdd_unet_conv_rows' [96][9 sum(cs) + sum(rcs)] matrix: pack_row_tile_weights, one stream per channel group."""
    return pack_row_tile_weights(w, cs, rcs, 2)


# default of cfg.model.conv_rows_min_wgs (UNetEngine._runs_conv_rows).  Graph replay of one MNIST plan, pairs | ctdd_unet_conv_rows:
# batch 16 (32 workgroups) 1157 | 1302 us, batch 32 (64) 1219 | 1305 us, batch 40 (80) 1264-1288 | 1303-1305 us, batch 48 (96)
# 1471-1485 | 1329-1331 us, batch 56 (112) 1519-1523 | 1344-1346 us, batch 64 (128) 1538 | 1381 us, batch 128 (256) 1710 | 1549 us
# (tools/conv_table.py): the smallest measured grid at which the one launch wins.  Taken with four waves per
# workgroup; with eight (cfg.model.conv_rows_waves, the default) 1247 | 1248 | 1251 | 1276 | 1306 | 1313 us at batch 16 | 32 | 40 | 48 | 56 | 64
# against the pairs' 1146 | 1206 | 1255 | 1476 | 1507 | 1529 us: 80 workgroups are a tie within the repeats, the threshold stays
CONV_ROWS_MIN_WGS = 96


def conv_rows_covers(H, W, cs, rcs, cout, G, residual=False):
    """Shapes ctdd_unet_conv_rows takes (csrc/unet_rows_kernels.hip): rows of <= 28 pixels (a slab of 32 positions per padded row, bands
    of 14 output rows), 96 output channels, one or two GroupNorm sources `cs` and up to two raw 1x1 sources `rcs` in multiples of 32
    channels (<= 384 per concatenation), groups dividing the GroupNorm channels, 1x1 segments or a residual but not both."""
    return bool(H >= 1 and 1 <= W <= 28 and cout == 96 and 1 <= len(cs) <= 2 and len(rcs) <= 2 and all(c > 0 and c % 32 == 0 for c in [*cs, *rcs])
                and sum(cs) <= 384 and sum(rcs) <= 384 and G > 0 and sum(cs) % G == 0 and not (rcs and residual))


def pack_conv_rows_head_weights(w, C1):
    """ctdd_unet_conv_rows_head's [N][9 C1] matrix: zero-padded to 96 ceil(N / 96) rows, then pack_row_tile_weights in two streams per
    96-channel pass (pass p reads streams 2 p and 2 p + 1, which lie one after the other).  Returned as [96 passes][9 C1]."""
    N, passes = w.shape[0], -(-w.shape[0] // 96)
    wp = torch.zeros((96 * passes, w.shape[1]), dtype=w.dtype, device=w.device)
    wp[:N] = w
    return pack_row_tile_weights(wp, [C1], [], 2 * passes)


# default of cfg.model.head_rows_min_wgs (UNetEngine._runs_head_rows): the grid of ctdd_unet_conv_rows_head (one workgroup per sample
# and band of 14 rows) from which the one launch replaces the head's ctdd_unet_gn_apply + ctdd_unet_conv_ring pair.  Graph replay of
# one MNIST plan, pair | one launch (tools/conv_table.py, twice per side from batch 64 on): batch 16 (32
# workgroups) 1154 | 1188 us, batch 32 (64) 1234 | 1265 us, batch 64 (128) 1360-1364 | 1362-1371 us, batch 96 (192) 1527-1528 |
# 1503-1508 us, batch 128 (256) 1558-1563 | 1519-1522 us: the smallest measured grid at which the one launch wins
HEAD_ROWS_MIN_WGS = 192


def conv_rows_head_covers(H, W, C1, N, G):
    """Shapes ctdd_unet_conv_rows_head takes (csrc/unet_head_kernels.hip): rows of <= 28 pixels, one GroupNorm source of 32, 64 or 96
    channels whose groups divide it, 32 .. 576 output channels in multiples of 32."""
    return bool(H >= 1 and 1 <= W <= 28 and C1 in (32, 64, 96) and G > 0 and C1 % G == 0 and 32 <= N <= 576 and N % 32 == 0)


def fold_upsample_weights(w):
    """The Upsample convolution's [N][C][3][3] weights -> [4][N][4 C] (include/ctdd_unet.h: ctdd_unet_conv_up_phases): the 3x3
    convolution on the nearest-2x grid as four 2x2-tap convolutions of the source.  Output pixel (2y + py, 2x + px) reads rows
    {y-1, y, y} (py = 0) or {y, y, y+1} (py = 1) of the source, columns alike, so phase 2 py + px has taps (i, j) on source pixel
    (y + py + i - 1, x + px + j - 1) with the weights of the 3x3 taps that land there summed: rows {W[0], W[1] + W[2]} for py = 0,
    {W[0] + W[1], W[2]} for py = 1.  K = tap 2 i + j -> channel.  Summed in the dtype of `w` (fp32 in the engine: rounded to bf16
    once, afterwards)."""
    N, Cn = w.shape[:2]
    assert tuple(w.shape[2:]) == (3, 3)
    sel = torch.tensor([[[1, 0, 0], [0, 1, 1]], [[1, 1, 0], [0, 0, 1]]], dtype=w.dtype, device=w.device)    # [phase][tap i][3x3 row]
    return torch.einsum("pia,qjb,ncab->pqnijc", sel, sel, w).reshape(4, N, 4 * Cn).contiguous()


def upsample_phases_covers(B, Hs, Ws, Cn, N):
    """Shapes ctdd_unet_conv_up_phases takes (source grid Hs x Ws)."""
    return bool(Cn >= 16 and Cn % 16 == 0 and (N % 96 == 0 or N % 64 == 0) and N > 0 and 1 <= Ws <= 33 and Hs * Ws >= 32
                and 4 * Cn * 64 < 2 ** 31 and 4 * B * Hs * Ws < 2 ** 31)


def _onepass_slab(B, HW, Cn, G, max_threads=1024):
    """Channels per workgroup ctdd_unet_gn_onepass will choose (csrc/unet_kernels.hip), 0 when no slab of whole groups fits."""
    if Cn % 8 or G <= 0 or Cn % G:
        return 0
    cg = Cn // G
    L = cg
    while L % 8:
        L += cg
    best = 0
    for sc in range(L, Cn + 1, L):
        if Cn % sc:
            continue
        noct = sc // 8
        if noct > max_threads:
            continue
        npl = min(max_threads // noct, HW)
        if -(-HW // npl) > 12:
            continue
        wgs = B * (Cn // sc)
        if best == 0 or wgs >= 256:
            best = sc
        if wgs < 256:
            break
    return best


class _Tensor:
    """NHWC activation [B*H*W][C] of the plan `pb` builds: bf16 (`hi`) in bf16 mode, fp32 (`f32`) in fp32 mode, plus the offset
    of its per-(b, channel) statistics in the plan's pool."""

    def __init__(self, pb, H, W, Cn, stats=True):
        eng, B = pb.eng, pb.B
        M = B * H * W
        self.B, self.H, self.W, self.C = B, H, W, Cn
        self.f32 = torch.empty((M, Cn), dtype=torch.float32, device=eng.dev) if eng.precise else None
        self.hi = None if eng.precise else torch.empty((M, Cn), dtype=torch.bfloat16, device=eng.dev)
        small = H * W <= pb.no_stats_hw      # a one-pass GroupNorm level: no statistics from the producers
        self.stats_by_gn = bool(stats and small and pb.gn_writes_stats)   # training: k_gn_onepass leaves them for backward
        self.stats = pb.alloc_stats(B * Cn * 2) if (stats and (not small or self.stats_by_gn)) else None
        pb.keep.append(self)             # raw pointers are baked into the plan: keep every buffer alive


class _PlanBuilder:
    """One build of one U-Net plan for batch B: launch list, kept-alive buffers, statistics-pool layout, split-K buffers.  `build`
    walks the network; the training context `tc` lays out its backward plan through the same methods (unet_train.TrainCtx.finish)."""

    def __init__(self, eng, B, tc, onepass_gn):
        self.eng, self.B, self.tc, self.onepass_gn = eng, B, tc, onepass_gn
        self.m, self.lib, self.net, self.dev, self.shape = eng.cfg.model, _lib(), eng.net, eng.dev, eng.cfg.data.shape
        # (levels up to gn_onepass_max_hw pixels per sample: above it the one-workgroup-per-(sample, slab) kernel loses to the many
        #  small workgroups of k_gn_apply, and those tensors keep their statistics epilogues.  MNIST net, batch 256, sampler loop:
        #  off 85.1 k sample-steps/s, 7x7 only 85.8 k, 7x7 + 14x14 87.9 k, all levels 85.1 k)
        self.no_stats_hw = eng._onepass_max_hw() if onepass_gn else 0
        self.gn_writes_stats = bool(onepass_gn and tc is not None)
        self.gn_threads = int(getattr(self.m, "gn_threads", 512))    # (measured in the two-chain sampler loop: 384-512 best, 1024 -1 %)
        self.bks = (32, 16) if eng.precise else (96, 64, 32, 16)      # fp32 tiles: K = 32 keeps 4 workgroups per CU
        self.plan, self.keep = [], []
        self.stats_off = 0
        self.stats_views = []          # (argument block, offset, field) resolved after the pool exists
        self.zero_views = []           # split-K partial-sum buffers: (conv args, elements)
        self._plan_to, self._zero_to = self.plan, self.zero_views     # where launch() and conv() append: see emitting_to
        self.st = type("Plan", (), {})()
        self.st.B = B

    def alloc_stats(self, n):
        off = self.stats_off
        self.stats_off += n
        return off

    @contextlib.contextmanager
    def emitting_to(self, plan, zero_views):
        """Within the block, launches go to `plan` and split-K buffers to `zero_views` (the backward plan, the forward prologue)."""
        saved = self._plan_to, self._zero_to
        self._plan_to, self._zero_to = plan, zero_views
        yield
        self._plan_to, self._zero_to = saved           # (an exception inside abandons the whole builder)

    def launch(self, fn, *args, label=None, flops=0):
        self._plan_to.append(bound_launch(fn, *args, label=label, flops=flops))

    def pick_bk(self, cs):
        for bk in self.bks:
            if all(c % bk == 0 for c in cs):
                return bk
        raise native.CtddError(f"no K tile divides channel counts {cs}")

    @staticmethod
    def pick_bnt(N, bk):
        if bk == 16:
            return 1
        if N % 96 == 0 and bk in (96, 32):
            return 3
        if N % 128 == 0:
            return 4
        if N % 64 == 0 and bk == 64:
            return 2
        return 1

    def pick_kernel(self, only3, M_, N, Hout, Wout):
        """cfg.model.conv_kernel, "auto" resolved to "ring" or "patch" for a bf16 convolution of M_ = B Hout Wout pixels (only3: every
        segment is a stride-1 3x3 one)."""
        m = self.m
        which = getattr(m, "conv_kernel", "auto")
        if which == "auto":
            # measured at batch 256 (MNIST net): the LDS-DMA ring wins where 512-pixel tiles give >= 160
            # workgroups and every unit has nine taps (28x28, 14x14); the patch kernel (128/256-pixel tiles, two
            # workgroups per CU) elsewhere.  Split-K lost everywhere it was tried (fp32 atomics + finish pass).
            ring_min = int(getattr(m, "ring_min_tiles", 80))
            which = "ring" if (only3 and -(-M_ // 512) * -(-N // 96) >= ring_min and N % 96 == 0) else "patch"
            # (CIFAR net, N = 256 at 16x16: 64-column ring tiles beat the 128-column patch tiles, 49 vs 54 / 69 vs 104 us at batch 128)
            if which == "patch" and only3 and N % 64 == 0 and N % 96 != 0 and Hout * Wout <= 256 and -(-M_ // 512) * (N // 64) >= ring_min:
                which = "ring"
            # (MNIST net's S = 256 output convolution, 28x28 K = 864: 64-column ring tiles 88 us, the 128-column patch tiles 105 us,
            #  128-column ring tiles 179 us at batch 128; +1.4 % on the sampler loop)
            if which == "patch" and only3 and N % 64 == 0 and N % 96 != 0 and N >= 256 and -(-M_ // 512) * (N // 64) >= ring_min:
                which = "ring"
        return which

    def conv(self, segs, wsrc, bias, N, Hout, Wout, Hin, Win, out, tb=None, res=None, logits_C=0, out_f32_tensor=None, bias_params=None,
             packed=None, back=True):
        """segs: list of (_Tensor, channels, kind); wsrc: per segment (weight parameter [N][Cin_tot][k][k], channel offset) --
        the [N][K] matrix the kernels stream is K = segment -> tap -> channel of those slices.  bias_params: the
        parameters whose sum `bias` is (training: each receives the bias gradient).  packed: (bf16 | None, fp32 | None)
        ready-made weights (the data-gradient convolutions of the training plan)."""
        eng, tc, m, lib, B = self.eng, self.tc, self.m, self.lib, self.B
        a = _ConvArgs()
        a.nseg = len(segs)
        for i, (src, cs, kind) in enumerate(segs):
            a.seg[i].hi, a.seg[i].f32, a.seg[i].C, a.seg[i].kind = ptr(src.hi), ptr(src.f32), cs, kind
        Ktot = sum(cs * (1 if kind == SEG_1x1 else 9) for _, cs, kind in segs)
        if packed is not None:
            whi, wf = packed
        elif tc is not None:
            whi, wf = tc.packed_forward(wsrc, segs, N, Ktot)     # persistent buffers, refreshed by ONE pack launch per step
        else:
            w2d = eng._w2d(wsrc, segs)
            assert w2d.shape[1] == Ktot
            whi, wf = eng._pack(w2d)
        self.keep.extend([whi, wf, bias])
        a.w_hi, a.w_f32 = ptr(whi), ptr(wf)
        a.B, a.H, a.W, a.Hin, a.Win, a.N, a.Ktot = B, Hout, Wout, Hin, Win, N, Ktot
        a.bias = ptr(bias)
        if tb is not None:
            a.tbias, a.tb_stride = tb
        if res is not None:
            if eng.precise:
                a.res_f32 = ptr(res.f32)
            else:
                a.res_bf16 = ptr(res.hi)
        if out_f32_tensor is not None:
            if out_f32_tensor.dtype == torch.bfloat16:      # (the bf16 logits of the sampler loops)
                a.out_hi = ptr(out_f32_tensor)
            else:
                a.out_f32 = ptr(out_f32_tensor)
        elif out is not None:
            a.out_f32, a.out_hi = ptr(out.f32), ptr(out.hi)
            if out.stats is not None and not out.stats_by_gn:
                self.stats_views.append((a, out.stats, "stats"))
        a.logits_C = logits_C
        self.keep.append(a)
        cs = [s[1] for s in segs]
        patchable = (not eng.precise) and all(s[2] in (SEG_3x3, SEG_1x1) for s in segs) and Wout <= 33
        hw_ = Hout * Wout
        patchable = patchable and N % 8 == 0 and (hw_ >= 32 or hw_ == 16 or B == 1) and (logits_C == 0 or (N // logits_C) % 8 == 0)
        M_ = B * Hout * Wout
        lab = f"{Hout}x{Wout} K={Ktot} N={N} segs={[(c_, k_) for _, c_, k_ in segs]}"
        if tc is not None and back:
            tc.record_conv(segs, wsrc, bias_params, N, Hout, Wout, Hin, Win, out, tb, res, logits_C, out_f32_tensor)
        only3 = all(s[2] == SEG_3x3 for s in segs)
        which = self.pick_kernel(only3, M_, N, Hout, Wout)
        resident = which == "res" and patchable and all(c % 32 == 0 for c in cs) and N % 32 == 0
        ring = which == "ring" and patchable and all(c % 16 == 0 for c in cs) and N % 32 == 0
        if resident or ring:
            # 512-pixel tiles, all nine taps' weights in LDS: register-staged 32-channel units (k_conv_res)
            # or an LDS-DMA ring of 16-channel units (k_conv_ring); csrc/unet_kernels.hip
            bnt = 3 if N % 96 == 0 else 4 if (N % 128 == 0 and resident) else 2
            ntiles = -(-M_ // 512) * -(-N // (32 * bnt))
            units = sum(c // (32 if resident else 16) for c in cs)
            if getattr(m, "conv_ksplit", 1) > 1 and units >= 2 and logits_C == 0:
                a.ksplit = min(units, int(m.conv_ksplit))
            if a.ksplit > 1:
                self._zero_to.append((a, M_ * N))
            fn = lib.ctdd_unet_conv_res if resident else lib.ctdd_unet_conv_ring
            # (ring_small_tiles: 256-pixel tiles, four waves, two workgroups per CU -- the variant two concurrent chains can share a CU with)
            sel = bnt + 10 if (ring and bnt in (2, 3) and getattr(m, "ring_small_tiles", 0)) else bnt
            self.launch(fn, C.byref(a), sel, label=lab + f" {which} bnt={sel} ks={a.ksplit}", flops=2 * M_ * N * Ktot)
        elif patchable:
            # throughput kernel: slab staged once per channel chunk (csrc/unet_kernels.hip: k_conv_patch)
            small = -(-M_ // 128) * -(-N // 96) < 256            # too few 128 x 96 tiles to fill the chip: 32-column tiles
            if small and all(c % 64 == 0 for c in cs) and N % 32 == 0:
                bk, bnt = 64, 1
            elif small and all(c % 48 == 0 for c in cs) and N % 32 == 0:
                bk, bnt = 48, 1
            elif all(c % 48 == 0 for c in cs) and (N % 96 == 0 or N % 128 == 0):
                bk, bnt = 48, (3 if N % 96 == 0 else 4)
            elif all(c % 64 == 0 for c in cs) and N % 64 == 0:
                bk, bnt = 64, (4 if N % 128 == 0 else 2)
            elif all(c % 32 == 0 for c in cs):
                bk, bnt = 32, (3 if N % 96 == 0 else 4 if N % 128 == 0 else 1)
            else:
                bk, bnt = 16, 1
            wm = 64 if (bnt >= 2 and bk in (48, 64) and M_ >= int(getattr(m, "patch_wm64_min_rows", 196 * 128)) and (bk, bnt) != (64, 4)) else 32
            units = sum(c // bk for c in cs)
            nwg = -(-M_ // (4 * wm)) * -(-N // (32 * bnt))
            if getattr(m, "conv_ksplit", 1) > 1 and units >= 2 and logits_C == 0 and out_f32_tensor is None:
                a.ksplit = min(units, int(m.conv_ksplit))
            elif nwg <= int(getattr(m, "ksplit_max_wgs", 96)) and units >= 4 and logits_C == 0 and out_f32_tensor is None:
                a.ksplit = max(1, min(units // 2, 256 // nwg))       # tiny grids (4x4 levels): split K to fill the chip
            if a.ksplit > 1:
                self._zero_to.append((a, M_ * N))
            self.launch(lib.ctdd_unet_conv_patch, C.byref(a), bk, bnt, wm, label=lab + f" patch bk={bk} bnt={bnt} wm={wm} ks={a.ksplit}",
                        flops=2 * M_ * N * Ktot)
        else:
            bk = self.pick_bk(cs)
            bnt = self.pick_bnt(N, bk)
            if (not eng.precise) and -(-M_ // 128) * -(-N // (32 * bnt)) < int(getattr(m, "igemm_small_wgs", 256)) and bk in (96, 64, 32):
                bnt = 1                                        # tiny grids: 32-column tiles, more workgroups
            self.launch(lib.ctdd_unet_conv, C.byref(a), bk, bnt, int(eng.precise), label=lab + f" igemm bk={bk} bnt={bnt}", flops=2 * M_ * N * Ktot)

    def gn_apply(self, srcs, norm, swish, eps, HW, drop_p=0.0):
        """srcs: one or two _Tensor; returns activated planes tensor (training: dropout applied in place after it)."""
        eng, tc, lib, B = self.eng, self.tc, self.lib, self.B
        Ct = sum(s.C for s in srcs)
        out = _Tensor(self, srcs[0].H, srcs[0].W, Ct, stats=False)
        a = _GnArgs()
        s1 = srcs[0]
        a.s1_f32, a.s1_bf16, a.C1 = (ptr(s1.f32), None, s1.C) if eng.precise else (None, ptr(s1.hi), s1.C)
        if s1.stats is not None:
            self.stats_views.append((a, s1.stats, "st1"))
        if len(srcs) == 2:
            s2 = srcs[1]
            a.s2_f32, a.s2_bf16, a.C2 = (ptr(s2.f32), None, s2.C) if eng.precise else (None, ptr(s2.hi), s2.C)
            if s2.stats is not None:
                self.stats_views.append((a, s2.stats, "st2"))
        g, b_ = norm.weight.detach().float().contiguous(), norm.bias.detach().float().contiguous()
        self.keep.extend([g, b_, a, out])
        a.gamma, a.beta = ptr(g), ptr(b_)
        a.B, a.HW, a.G, a.eps, a.swish = B, HW, norm.num_groups, eps, int(swish)
        a.out_hi, a.out_f32 = ptr(out.hi), ptr(out.f32)
        if self.onepass_gn and HW <= self.no_stats_hw:
            if _onepass_slab(B, HW, Ct, norm.num_groups, self.gn_threads) == 0:       # (UNetEngine._build checked every shape first)
                raise native.CtddError(f"one-pass GroupNorm does not cover HW={HW} C={Ct} G={norm.num_groups}")
            # inference, bf16: statistics + normalisation in one pass over the tensor (k_gn_onepass); the producers' epilogues
            # then carry no statistics at all (their tensors were created without statistics buffers)
            self.launch(lib.ctdd_unet_gn_onepass, C.byref(a), 0, self.gn_threads, label=f"gn1 {srcs[0].H}x{srcs[0].W} C={Ct} ({len(srcs)} src)")
        else:
            self.launch(lib.ctdd_unet_gn_apply, C.byref(a), label=f"gn {srcs[0].H}x{srcs[0].W} C={Ct} ({len(srcs)} src)")
        if tc is not None:
            tc.record_gn(self, srcs, norm, swish, eps, HW, out, drop_p)
        return out

    def conv_rows(self, srcs, norm, segs, wsrc, bias, out, tb=None, res=None, raws=()):
        """GroupNorm `norm` + Swish of the concatenation of `srcs`, the 3x3 convolution on it (+ the 1x1 segments on the raw tensors
        `raws` | + the residual `res`) as ONE ctdd_unet_conv_rows launch: the gn_apply + conv pair without the activated tensor.
        segs, wsrc: the weights as `conv` takes them (the 3x3 segment, then one 1x1 segment per raw tensor); bias: their summed bias."""
        eng, lib, B = self.eng, self.lib, self.B
        Hc, Wc, N = srcs[0].H, srcs[0].W, out.C
        cs, rcs = [s_.C for s_ in srcs], [s_.C for s_ in raws]
        a = _ConvRowsArgs()
        for i, s_ in enumerate(srcs):
            setattr(a, f"s{i + 1}_bf16", ptr(s_.hi))
            setattr(a, f"C{i + 1}", s_.C)
            self.stats_views.append((a, s_.stats, f"st{i + 1}"))
        for i, s_ in enumerate(raws):
            setattr(a, f"r{i + 1}_bf16", ptr(s_.hi))
            setattr(a, f"RC{i + 1}", s_.C)
        g, b_ = norm.weight.detach().float().contiguous(), norm.bias.detach().float().contiguous()
        a.gamma, a.beta, a.G, a.eps = ptr(g), ptr(b_), norm.num_groups, norm.eps
        w, _ = eng._pack(pack_conv_rows_weights(eng._w2d(wsrc, segs), cs, rcs))
        a.w, a.bias = ptr(w), ptr(bias)
        if tb is not None:
            a.tbias, a.tb_stride = tb
        if res is not None:
            a.res_bf16 = ptr(res.hi)
        a.out_bf16 = ptr(out.hi)
        if out.stats is not None and not out.stats_by_gn:
            self.stats_views.append((a, out.stats, "out_stats"))
        a.B, a.H, a.W, a.N = B, Hc, Wc, N
        self.keep.extend([g, b_, w, bias, a])
        Ktot = w.shape[1]
        # cfg.model.conv_rows_waves: 8 (default) waves per workgroup, or 4: the same bits from the kernel's 4-wave work split
        waves = int(getattr(eng.cfg.model, "conv_rows_waves", 8))
        if waves not in (4, 8):
            raise ValueError(f"cfg.model.conv_rows_waves = {waves}: 4 or 8")
        self.launch(lib.ctdd_unet_conv_rows if waves == 8 else lib.ctdd_unet_conv_rows_w4, C.byref(a), 0, label=f"{Hc}x{Wc} K={Ktot} N={N} gn+conv rows C={cs} raw={rcs}",
                    flops=2 * B * Hc * Wc * N * Ktot)

    def conv_rows_head(self, src, norm, oc, logits):
        """GroupNorm `norm` + Swish of `src` and the output convolution `oc` into the bf16 (B, H W, N) `logits` as ONE
        ctdd_unet_conv_rows_head launch: the head's gn_apply + conv pair without the activated tensor."""
        eng, B = self.eng, self.B
        N, C1 = oc.weight.shape[0], src.C
        a = _ConvRowsArgs()
        a.s1_bf16, a.C1 = ptr(src.hi), C1
        self.stats_views.append((a, src.stats, "st1"))
        g, b_ = norm.weight.detach().float().contiguous(), norm.bias.detach().float().contiguous()
        a.gamma, a.beta, a.G, a.eps = ptr(g), ptr(b_), norm.num_groups, norm.eps
        w, _ = eng._pack(pack_conv_rows_head_weights(eng._w2d([(oc.weight, 0)], [(None, C1, SEG_3x3)]), C1))
        bias = oc.bias.detach().float().contiguous()
        a.w, a.bias, a.out_bf16 = ptr(w), ptr(bias), ptr(logits)
        a.B, a.H, a.W, a.N = B, src.H, src.W, N
        self.keep.extend([g, b_, w, bias, a])
        # cfg.model.head_rows_waves: 8 (default) waves per workgroup, or 4: the same bits from the kernel's 4-wave work split
        waves = int(getattr(eng.cfg.model, "head_rows_waves", 8))
        if waves not in (4, 8):
            raise ValueError(f"cfg.model.head_rows_waves = {waves}: 4 or 8")
        # (flops: the unpadded N; the channels past N that the last pass computes are not the network's)
        self.launch(self.lib.ctdd_unet_conv_rows_head if waves == 8 else self.lib.ctdd_unet_conv_rows_head_w4, C.byref(a), 0, label=f"{src.H}x{src.W} K={9 * C1} N={N} gn+conv rows head C={[C1]}",
                    flops=2 * B * src.H * src.W * N * 9 * C1)

    def conv2_operands(self, rb, a2, srcs):
        """conv2 of a ResBlock as ONE K-segmented convolution: the 3x3 segment on the activated tensor `a2` (None where the kernel
        makes it itself) and, for a block with a linear skip, a 1x1 segment on each raw source.  Returns segs, wsrc, the bias
        parameters and their sum (training: the recorder's buffer, filled before the plan runs)."""
        tc = self.tc
        segs, wsrc, bias_params = [(a2, rb.conv2.weight.shape[0], SEG_3x3)], [(rb.conv2.weight, 0)], [rb.conv2.bias]
        bias = rb.conv2.bias.detach().float()
        if rb.skip is not None:
            c_ = 0
            for s_ in srcs:
                segs.append((s_, s_.C, SEG_1x1))
                wsrc.append((rb.skip.weight, c_))
                c_ += s_.C
            bias_params.append(rb.skip.bias)
            bias = tc.summed_bias(bias_params) if tc is not None else bias + rb.skip.bias.detach().float()
        return segs, wsrc, bias_params, bias.contiguous()

    def resblock_fused(self, rb, srcs, mid=False):
        """The block as ONE ctdd_unet_resblock_small launch (mid: ctdd_unet_resblock_mid, the 14x14 level): the same [N][K] matrices in
        the kernel's fragment order, the same summed conv2 + skip bias."""
        eng, lib, B = self.eng, self.lib, self.B
        Hc, Wc = srcs[0].H, srcs[0].W
        cs = [s.C for s in srcs]
        Ct, cout = sum(cs), rb.conv1.weight.shape[0]
        y = _Tensor(self, Hc, Wc, cout)
        a = _ResblockArgs()
        a.s1_bf16, a.C1 = ptr(srcs[0].hi), cs[0]
        if len(srcs) == 2:
            a.s2_bf16, a.C2 = ptr(srcs[1].hi), cs[1]
        par = [p_.detach().float().contiguous() for p_ in (rb.norm1.weight, rb.norm1.bias, rb.norm2.weight, rb.norm2.bias, rb.conv1.bias)]
        a.gamma1, a.beta1, a.gamma2, a.beta2, a.bias1 = (ptr(p_) for p_ in par)
        a.G1, a.G2, a.eps1, a.eps2 = rb.norm1.num_groups, rb.norm2.num_groups, rb.norm1.eps, rb.norm2.eps
        a.tbias, a.tb_stride = self.tproj.data_ptr() + 4 * self.toff[id(rb)], self.tb_stride
        w1 = eng._w2d([(rb.conv1.weight, 0)], [(None, Ct, SEG_3x3)])
        segs, wsrc, _, bias2 = self.conv2_operands(rb, None, srcs)
        w2 = eng._w2d(wsrc, segs)
        w1, w2 = pack_resblock_mid_weights(w1, w2, cs) if mid else (pack_resblock_weights(w1), pack_resblock_weights(w2))
        (w1, _), (w2, _) = eng._pack(w1), eng._pack(w2)
        a.w1, a.w2, a.bias2, a.skip = ptr(w1), ptr(w2), ptr(bias2), int(rb.skip is not None)
        a.B, a.H, a.W, a.N, a.out_bf16 = B, Hc, Wc, cout, ptr(y.hi)
        self.keep.extend(par + [w1, w2, bias2, a])
        K1, K2 = w1.shape[1], w2.shape[1]
        # (flops: the block's own products; the zero columns that pad a source of the mid kernel to whole chunks are not counted)
        self.launch(lib.ctdd_unet_resblock_mid if mid else lib.ctdd_unet_resblock_small, C.byref(a), 0,
                    label=f"{Hc}x{Wc} resblock C={cs} N={cout} K={K1}+{K2}", flops=2 * B * Hc * Wc * cout * (9 * Ct + 9 * cout + (Ct if rb.skip is not None else 0)))
        return y

    def resblock(self, rb, srcs):
        """srcs: list of 1-2 tensors forming the (virtual) channel concatenation."""
        eng, tc = self.eng, self.tc
        Hc, Wc = srcs[0].H, srcs[0].W
        cs = [s.C for s in srcs]
        cout = rb.conv1.weight.shape[0]
        # a small level's whole block in one launch (csrc/unet_resblock_kernels.hip: one workgroup per sample, both activated
        # tensors and h1 stay in LDS); cfg.model.resblock_fused = 0 keeps the four launches below
        if self.onepass_gn and eng._fuses_resblock(rb, Hc, Wc, cs, tc is not None) and all(s_.stats is None for s_ in srcs):
            return self.resblock_fused(rb, srcs)
        # the 14x14 level's: ctdd_unet_resblock_mid, one 192-channel slab, conv1 source by source; cfg.model.resblock_fused_mid = 0
        # keeps the four launches
        if self.onepass_gn and eng._fuses_resblock_mid(rb, Hc, Wc, cs, tc is not None) and all(s_.stats is None for s_ in srcs):
            return self.resblock_fused(rb, srcs, mid=True)
        # a level whose samples do not fit one workgroup (28x28): each GroupNorm + convolution pair as ONE ctdd_unet_conv_rows launch
        # (csrc/unet_rows_kernels.hip) when the producers left statistics; cfg.model.conv_rows = 0 keeps the pairs
        tbias = (self.tproj.data_ptr() + 4 * self.toff[id(rb)], self.tb_stride)
        h = _Tensor(self, Hc, Wc, cout)
        b1 = rb.conv1.bias.detach().float().contiguous()
        if eng._runs_conv_rows(self.B, Hc, Wc, cs, [], cout, rb.norm1.num_groups, False, tc is not None) and all(s_.stats is not None for s_ in srcs):
            self.conv_rows(srcs, rb.norm1, [(None, sum(cs), SEG_3x3)], [(rb.conv1.weight, 0)], b1, h, tb=tbias)
        else:
            a1 = self.gn_apply(srcs, rb.norm1, True, rb.norm1.eps, Hc * Wc)
            self.conv([(a1, a1.C, SEG_3x3)], [(rb.conv1.weight, 0)], b1, cout, Hc, Wc, Hc, Wc, h, tb=tbias, bias_params=[rb.conv1.bias])
        rcs, res = (cs, None) if rb.skip is not None else ([], srcs[0])    # linear skip as 1x1 K-segments on the raw input | residual
        if eng._runs_conv_rows(self.B, Hc, Wc, [cout], rcs, cout, rb.norm2.num_groups, rb.skip is None, tc is not None) and h.stats is not None:
            y = _Tensor(self, Hc, Wc, cout)
            segs, wsrc, _, bias2 = self.conv2_operands(rb, None, srcs)
            self.conv_rows([h], rb.norm2, segs, wsrc, bias2, y, res=res, raws=srcs if rb.skip is not None else ())
            return y
        drop = float(rb.dropout.p) if (tc is not None and tc.dropout) else 0.0
        a2 = self.gn_apply([h], rb.norm2, True, rb.norm2.eps, Hc * Wc, drop_p=drop)
        y = _Tensor(self, Hc, Wc, cout)
        segs, wsrc, bias_params, bias2 = self.conv2_operands(rb, a2, srcs)
        self.conv(segs, wsrc, bias2, cout, Hc, Wc, Hc, Wc, y, res=res, bias_params=bias_params)
        return y

    def block(self, layer, srcs):
        """One ResBlock (+ attention) module of net.down / net.mid / net.up."""
        cur = self.resblock(layer.resblocks, srcs)
        return cur if layer.attention is None else self.attention(layer.attention, cur)

    def attention(self, att, x):
        tc, lib, B = self.tc, self.lib, self.B
        T = x.H * x.W
        an = self.gn_apply([x], att.norm, False, att.norm.eps, T)
        Cx = x.C
        # bf16 inference behind a one-pass GroupNorm: qkv, softmax and proj as ONE ctdd_unet_attention_block launch
        # (csrc/unet_attn_kernels.hip: one workgroup per sample, qkv and the attention output stay in LDS);
        # cfg.model.attention_fused = 0 keeps the three launches below
        if self.onepass_gn and T <= self.no_stats_hw and self.eng._fuses_attention(att, T, Cx, tc is not None):
            return self.attention_fused(att, x, an)
        qkv = torch.empty((B * T, 3 * Cx), dtype=torch.float32, device=self.dev)
        self.keep.append(qkv)
        self.conv([(an, Cx, SEG_1x1)], [(att.qkv.weight, 0)],
                  att.qkv.bias.detach().float().contiguous(), 3 * Cx, x.H, x.W, x.H, x.W, None, out_f32_tensor=qkv,
                  bias_params=[att.qkv.bias])
        ao = _Tensor(self, x.H, x.W, Cx, stats=False)
        aa = _AttnArgs()
        aa.qkv, aa.B, aa.T, aa.C, aa.heads, aa.out_hi, aa.out_f32 = ptr(qkv), B, T, Cx, att.num_heads, ptr(ao.hi), ptr(ao.f32)
        self.keep.extend([aa, ao])
        self.launch(lib.ctdd_unet_attention, C.byref(aa))
        if tc is not None:
            tc.record_attention(att, qkv, ao, B, T, Cx)
        y = _Tensor(self, x.H, x.W, Cx)
        self.conv([(ao, Cx, SEG_1x1)], [(att.proj_out.weight, 0)],
                  att.proj_out.bias.detach().float().contiguous(), Cx, x.H, x.W, x.H, x.W, y, res=x, bias_params=[att.proj_out.bias])
        return y

    def attention_fused(self, att, x, an):
        """The block behind its GroupNorm as ONE ctdd_unet_attention_block launch: the two 1x1 matrices in the kernel's fragment order."""
        eng, B, T, Cx = self.eng, self.B, x.H * x.W, x.C
        y = _Tensor(self, x.H, x.W, Cx)
        (wq, _), (wp, _) = (eng._pack(pack_attention_weights(w.detach().float().reshape(w.shape[0], Cx))) for w in (att.qkv.weight, att.proj_out.weight))
        bq, bp = att.qkv.bias.detach().float().contiguous(), att.proj_out.bias.detach().float().contiguous()
        a = _AttnBlockArgs()
        a.an_bf16, a.x_bf16, a.w_qkv, a.b_qkv, a.w_proj, a.b_proj = ptr(an.hi), ptr(x.hi), ptr(wq), ptr(bq), ptr(wp), ptr(bp)
        a.B, a.T, a.C, a.heads, a.out_bf16 = B, T, Cx, att.num_heads, ptr(y.hi)
        self.keep.extend([wq, bq, wp, bp, a])
        # (flops: the two convolutions the launch replaces)
        self.launch(self.lib.ctdd_unet_attention_block, C.byref(a), 0, label=f"{x.H}x{x.W} attention block C={Cx} heads={att.num_heads}",
                    flops=2 * B * T * Cx * (3 * Cx + Cx))
        return y

    def time(self, uniform_t):
        """Time embedding + all ResBlock projections in two launches (st.tproj; `toff`: each block's column offset in it)."""
        tc, B, st, lib, dev, ch = self.tc, self.B, self.st, self.lib, self.dev, self.net.channel
        resblocks, pw, pb, tw = self.eng._time_weights()
        tdim, Ntot = ch * 4, pw.shape[1]
        st.tact = torch.empty((B, tdim), dtype=torch.float32, device=dev)
        time_row = uniform_t == "row" and tc is None
        uniform_t = bool(uniform_t) and tc is None
        # uniform_t: every sample at the same time (the samplers): ONE projection row from one fused launch, read by the
        # convolutions with a zero batch stride (csrc/unet_kernels.hip: k_time_uniform).  "row": that row comes from the caller
        # (a sampler's grid of times is known when it starts: time_table() computes every step's row at once) -- no time
        # launch in the plan at all
        st.time_row = time_row
        self.tproj = st.tproj = torch.empty((1 if uniform_t else B, Ntot), dtype=torch.float32, device=dev)
        self.tb_stride = 0 if uniform_t else Ntot
        ta = _TimeArgs()
        st.thid = torch.empty((B, tdim), dtype=torch.float32, device=dev)
        ta.t, ta.B, ta.ch, ta.tdim = ptr(st.t_in), B, ch, tdim
        ta.w1, ta.b1, ta.w2, ta.b2, ta.hid, ta.act = ptr(tw[0]), ptr(tw[1]), ptr(tw[2]), ptr(tw[3]), ptr(st.thid), ptr(st.tact)
        self.keep.extend(tw + [pw, pb, ta])
        if tc is None and not time_row:
            self.launch(lib.ctdd_unet_time_uniform if uniform_t else lib.ctdd_unet_time, C.byref(ta), ptr(pw), ptr(pb), Ntot, ptr(st.tproj))
        elif tc is None:
            st.tproj.zero_()
        else:
            tc.tproj, tc.resblocks = st.tproj, resblocks          # filled by the caller before the plan runs
        self.toff, o = {}, 0
        for rb in resblocks:
            self.toff[id(rb)] = o
            o += rb.time[1].weight.shape[0]

    def first_conv(self, c0):
        st, B, net, ch, (Cin, H0, W0) = self.st, self.B, self.net, self.net.channel, self.shape
        cur = _Tensor(self, H0, W0, ch)
        fa = _FirstArgs()
        if st.x_in.dtype == torch.int64:
            fa.x64 = ptr(st.x_in)
        else:
            fa.x32 = ptr(st.x_in)
        fa.lo, fa.hi = float(net.x_min_max[0]), float(net.x_min_max[1])
        w0, b0 = c0.weight.detach().float().contiguous(), c0.bias.detach().float().contiguous()
        fa.w, fa.bias, fa.B, fa.Cin, fa.H, fa.W, fa.Cout = ptr(w0), ptr(b0), B, Cin, H0, W0, ch
        fa.out_f32, fa.out_hi = ptr(cur.f32), ptr(cur.hi)
        if self.m.model_output == "logistic_pars":
            st.x0 = torch.empty((B, Cin, H0, W0), dtype=torch.float32, device=self.dev)
            fa.x0_f32 = ptr(st.x0)
        if cur.stats is not None:
            self.stats_views.append((fa, cur.stats, "stats"))
        self.keep.extend([w0, b0, fa])
        self.launch(self.lib.ctdd_unet_first_conv, C.byref(fa))
        if self.tc is not None:
            self.tc.record_first(c0, fa, cur)
        return cur

    def downsample(self, cv, cur):
        """Downsample: stride-2 conv, pad right/bottom by one."""
        Ho, Wo = (cur.H + 1 - 3) // 2 + 1, (cur.W + 1 - 3) // 2 + 1
        y = _Tensor(self, Ho, Wo, cur.C)
        self.conv([(cur, cur.C, SEG_3x3_S2)], [(cv.weight, 0)],
                  cv.bias.detach().float().contiguous(), cur.C, Ho, Wo, cur.H, cur.W, y, bias_params=[cv.bias])
        return y

    def upsample_in_phases(self, cur):
        """Whether the Upsample convolution on `cur` runs as ONE ctdd_unet_conv_up_phases launch: bf16 inference plans, where the
        stride-1 convolution on the materialised 2x grid would have gone to the plain 512-pixel ring (no split-K, not the
        four-wave variant) and the entry takes the shape; cfg.model.upsample_phases = 0 keeps the two launches."""
        eng, m, B, Cn = self.eng, self.m, self.B, cur.C
        if self.tc is not None or eng.precise or not int(getattr(m, "upsample_phases", 1)):
            return False
        Ho, Wo = cur.H * 2, cur.W * 2
        ring = self.pick_kernel(True, B * Ho * Wo, Cn, Ho, Wo) == "ring" and Wo <= 33 and Cn % 32 == 0
        if not ring or (getattr(m, "conv_ksplit", 1) > 1 and Cn // 16 >= 2) or getattr(m, "ring_small_tiles", 0):
            return False
        return upsample_phases_covers(B, cur.H, cur.W, Cn, Cn)

    def upsample_phases(self, cv, cur, y):
        """The four 2x2-tap phase convolutions of the source in one launch (csrc/unet_kernels.hip: k_conv_ring_up), weights folded
        per weights version (fold_upsample_weights)."""
        eng, B, Cn = self.eng, self.B, cur.C
        a = _ConvArgs()
        a.nseg = 1
        a.seg[0].hi, a.seg[0].C, a.seg[0].kind = ptr(cur.hi), Cn, SEG_3x3_UP
        whi, _ = eng._pack(fold_upsample_weights(cv.weight.detach().float()).reshape(4 * Cn, 4 * Cn))
        bias = cv.bias.detach().float().contiguous()
        a.w_hi, a.bias = ptr(whi), ptr(bias)
        a.B, a.H, a.W, a.Hin, a.Win, a.N, a.Ktot = B, y.H, y.W, cur.H, cur.W, Cn, 4 * Cn
        a.out_hi = ptr(y.hi)
        if y.stats is not None and not y.stats_by_gn:
            self.stats_views.append((a, y.stats, "stats"))
        self.keep.extend([whi, bias, a])
        # (flops: the products executed, four taps per output pixel)
        self.launch(self.lib.ctdd_unet_conv_up_phases, C.byref(a), 0, label=f"{y.H}x{y.W} K=4x{4 * Cn} N={Cn} up-phases of {cur.H}x{cur.W}",
                    flops=2 * B * y.H * y.W * Cn * 4 * Cn)

    def upsample(self, cv, cur):
        """Upsample: nearest x2 folded into the conv's addressing (fp32 inference), or materialised before a stride-1 convolution."""
        eng, tc, B, lib = self.eng, self.tc, self.B, self.lib
        y = _Tensor(self, cur.H * 2, cur.W * 2, cur.C)
        if self.upsample_in_phases(cur):
            self.upsample_phases(cv, cur, y)
        elif eng.precise and tc is None:
            self.conv([(cur, cur.C, SEG_3x3_UP)], [(cv.weight, 0)],
                      cv.bias.detach().float().contiguous(), cur.C, cur.H * 2, cur.W * 2, cur.H, cur.W, y)
        else:                                  # materialise the 2x grid (cheap), then a stride-1 convolution (training: both modes)
            up = _Tensor(self, cur.H * 2, cur.W * 2, cur.C, stats=False)
            if eng.precise:
                self.launch(lib.ctdd_unet_upsample2x_f32, ptr(cur.f32), B, cur.H, cur.W, cur.C, ptr(up.f32))
            else:
                self.launch(lib.ctdd_unet_upsample2x, ptr(cur.hi), B, cur.H, cur.W, cur.C, ptr(up.hi))
            if tc is not None:
                tc.record_upsample(cur, up)
            self.conv([(up, cur.C, SEG_3x3)], [(cv.weight, 0)],
                      cv.bias.detach().float().contiguous(), cur.C, up.H, up.W, up.H, up.W, y, bias_params=[cv.bias])
        return y

    def head(self, cur, logits_out, logits_bf16):
        """Output GroupNorm + convolution into st.logits (logistic_pars: into st.net_out, then the logistic head)."""
        eng, tc, B, st, m, net, dev, (Cin, H0, W0) = self.eng, self.tc, self.B, self.st, self.m, self.net, self.dev, self.shape
        S = net.S
        oc = net.out[2]
        n_out = oc.weight.shape[0]
        D = Cin * H0 * W0
        logistic = m.model_output == "logistic_pars"
        # (bf16 logits: the output convolution's epilogue; the logistic head writes them in the bf16 inference engine when S % 4 == 0)
        ldt = torch.bfloat16 if logits_bf16 and not (logistic and (tc is not None or eng.precise or S % 4)) else torch.float32
        st.logits = logits_out if logits_out is not None else torch.empty((B, D, S), dtype=ldt, device=dev)
        assert st.logits.dtype == ldt
        # the S-channel logits of a one-channel image are exactly [pixel][N]: GroupNorm + convolution as ONE ctdd_unet_conv_rows_head
        # launch (csrc/unet_head_kernels.hip); cfg.model.head_rows = 0 keeps the pair
        if (not logistic and Cin == 1 and ldt == torch.bfloat16 and cur.stats is not None
                and eng._runs_head_rows(B, cur.H, cur.W, cur.C, n_out, net.out[0].num_groups, tc is not None)):
            self.conv_rows_head(cur, net.out[0], oc, st.logits)
            return
        ao = self.gn_apply([cur], net.out[0], True, net.out[0].eps, cur.H * cur.W)
        if logistic:
            st.net_out = torch.empty((B * H0 * W0, n_out), dtype=torch.float32, device=dev)
            self.conv([(ao, ao.C, SEG_3x3)], [(oc.weight, 0)],
                      oc.bias.detach().float().contiguous(), n_out, H0, W0, H0, W0, None, out_f32_tensor=st.net_out, bias_params=[oc.bias])
            la = _LogisticArgs()
            la.net, la.x0, la.B, la.C, la.HW, la.S, la.fix = ptr(st.net_out), ptr(st.x0), B, Cin, H0 * W0, S, int(bool(m.fix_logistic))
            if ldt == torch.bfloat16:                  # (the sampler loops of the bf16 engine: the head writes what the bf16 step kernel reads)
                la.out_bf16 = ptr(st.logits)
            else:
                la.out = ptr(st.logits)
            la.fast = 0 if eng.precise else 1
            self.keep.append(la)
            if tc is None:                             # (training: the head runs as differentiable device ops on net_out)
                self.launch(self.lib.ctdd_unet_logistic_head, C.byref(la))
        else:
            self.conv([(ao, ao.C, SEG_3x3)], [(oc.weight, 0)],
                      oc.bias.detach().float().contiguous(), n_out, H0, W0, H0, W0, None, out_f32_tensor=st.logits,
                      logits_C=Cin, bias_params=[oc.bias])

    def build(self, x_dtype, logits_out, logits_bf16, uniform_t):
        st, B, net, dev = self.st, self.B, self.net, self.dev
        st.x_in = torch.zeros((B, *self.shape), dtype=x_dtype, device=dev)
        st.t_in = torch.zeros((B,), dtype=torch.float32, device=dev)
        self.time(uniform_t)
        cur = self.first_conv(net.down[0])
        feats = [cur]
        for layer in list(net.down)[1:]:
            cur = self.block(layer, [cur]) if hasattr(layer, "resblocks") else self.downsample(layer.downsample[0], cur)
            feats.append(cur)
        for layer in net.mid:
            cur = self.block(layer, [cur])
        for layer in net.up:
            cur = self.block(layer, [cur, feats.pop()]) if hasattr(layer, "resblocks") else self.upsample(layer[1], cur)
        self.head(cur, logits_out, logits_bf16)
        if self.tc is not None:                        # backward plan: built before the pools are laid out
            self.tc.finish(self)
        # ---- the per-(b, channel) statistics pool (one buffer, zeroed once per forward) and the split-K pool: the argument blocks
        # recorded against offsets get their addresses
        st.stats = torch.zeros((max(self.stats_off, 1),), dtype=torch.float64, device=dev)
        base = st.stats.data_ptr()
        for a_, off, field in self.stats_views:
            setattr(a_, field, base + 8 * off)
        nz = sum(n for _, n in self.zero_views)
        st.zpool = torch.zeros((max(nz, 1),), dtype=torch.float32, device=dev)
        zo = 0
        for a_, n in self.zero_views:
            a_.acc_buf = st.zpool.data_ptr() + 4 * zo
            zo += n
        st.plan, st.keep, st.graph = self.plan, self.keep, None
        return st


class UNetEngine:
    def __init__(self, model, precision=None):
        self.model = model
        self.net = _unwrap(model.net)
        self.cfg = model.cfg
        self.dev = next(self.net.parameters()).device
        if self.dev.type != "cuda":
            raise native.CtddError("UNetEngine needs the model on a GPU")
        self.precision = precision or getattr(self.cfg.model, "engine_precision", "bf16")
        if self.precision not in ("bf16", "fp32"):
            raise ValueError(f"unknown engine precision {self.precision}")
        self.precise = self.precision == "fp32"
        self._plans = {}
        self._wver = None
        self._time_w = None

    # ------------------------------------------------------------------ weights
    def _weights_version(self):
        return sum(p._version for p in self.net.parameters()) + 7919 * getattr(self.model, "_weights_version", 0)

    def _pack(self, w2d):
        """[N][K] weights in the mode's element type: (bf16 | None, fp32 | None)."""
        w = w2d.detach().float().contiguous()
        return (None, w) if self.precise else (w.to(torch.bfloat16).contiguous(), None)

    @staticmethod
    def _w2d(wsrc, segs):
        """The [N][K] matrix of a convolution, K = segment -> tap -> channel, from per-segment (parameter, channel offset)."""
        parts = []
        for (w, c_off), (_, cs, kind) in zip(wsrc, segs):
            w = w.detach().float()
            N = w.shape[0]
            if kind == SEG_1x1:
                parts.append(w.reshape(N, -1)[:, c_off:c_off + cs])
            else:
                parts.append(w[:, c_off:c_off + cs].permute(0, 2, 3, 1).reshape(N, 9 * cs))
        return torch.cat(parts, dim=1).contiguous()


    # ------------------------------------------------------------------ plan construction
    def _time_weights(self):
        """(resblocks, pw [tdim][Ntot], pb [Ntot], [w1, b1, w2, b2] as [in][out]): every ResBlock in plan order, their time
        projections concatenated, and the time-embedding MLP, as fp32 copies; rebuilt when the weights change."""
        ver = self._weights_version()
        if self._time_w is None or self._time_w[0] != ver:
            net = self.net
            resblocks = [mod.resblocks for mod in list(net.down) + list(net.mid) + list(net.up) if hasattr(mod, "resblocks")]
            pw = torch.cat([rb.time[1].weight.detach().float() for rb in resblocks], 0).t().contiguous()   # [tdim][Ntot]
            pb = torch.cat([rb.time[1].bias.detach().float() for rb in resblocks], 0).contiguous()
            tw = [net.time[1].weight.t(), net.time[1].bias, net.time[3].weight.t(), net.time[3].bias]      # weights as [in][out]
            tw = [w.detach().float().contiguous() for w in tw]
            self._time_w = (ver, resblocks, pw, pb, tw)
        return self._time_w[1:]

    def _onepass_max_hw(self):
        return int(getattr(self.cfg.model, "gn_onepass_max_hw", 256))

    def _fuses_resblock(self, rb, Hc, Wc, cs, training):
        """Whether a plan with one-pass GroupNorm runs this block as ONE ctdd_unet_resblock_small launch (bf16 inference only)."""
        return bool(not training and not self.precise and int(getattr(self.cfg.model, "resblock_fused", 1))
                    and Hc * Wc <= self._onepass_max_hw()
                    and resblock_small_covers(Hc, Wc, cs, rb.conv1.weight.shape[0], rb.norm1.num_groups, rb.norm2.num_groups))

    def _fuses_resblock_mid(self, rb, Hc, Wc, cs, training):
        """Whether such a plan runs this block as ONE ctdd_unet_resblock_mid launch: shapes the small kernel does not hold (whatever
        resblock_fused says: the two knobs are independent), bf16 inference only, cfg.model.resblock_fused_mid (default on)."""
        return bool(not training and not self.precise and int(getattr(self.cfg.model, "resblock_fused_mid", 1))
                    and Hc * Wc <= self._onepass_max_hw()
                    and not resblock_small_covers(Hc, Wc, cs, rb.conv1.weight.shape[0], rb.norm1.num_groups, rb.norm2.num_groups)
                    and resblock_mid_covers(Hc, Wc, cs, rb.conv1.weight.shape[0], rb.norm1.num_groups, rb.norm2.num_groups))

    def _fuses_attention(self, att, T, Cn, training):
        """Whether a plan with one-pass GroupNorm runs the attention block's qkv, softmax and proj as ONE ctdd_unet_attention_block
        launch: bf16 inference only (training records the fp32 qkv), cfg.model.attention_fused (default on), a shape the kernel holds."""
        return bool(not training and not self.precise and int(getattr(self.cfg.model, "attention_fused", 1))
                    and attention_block_covers(T, Cn, att.num_heads))

    def _runs_conv_rows(self, B, Hc, Wc, cs, rcs, cout, G, residual, training):
        """Whether a GroupNorm + convolution pair of the four-launch ResBlock runs as ONE ctdd_unet_conv_rows launch: bf16 inference
        only, cfg.model.conv_rows (default on), a shape the kernel takes, and at least cfg.model.conv_rows_min_wgs workgroups (one per
        sample and band of 14 rows: below that the pair's smaller tiles fill the chip better)."""
        m = self.cfg.model
        return bool(not training and not self.precise and int(getattr(m, "conv_rows", 1))
                    and conv_rows_covers(Hc, Wc, cs, rcs, cout, G, residual)
                    and B * -(-Hc // 14) >= int(getattr(m, "conv_rows_min_wgs", CONV_ROWS_MIN_WGS)))

    def _runs_head_rows(self, B, Hc, Wc, C1, N, G, training):
        """Whether the output head's GroupNorm + convolution pair runs as ONE ctdd_unet_conv_rows_head launch: bf16 inference only,
        cfg.model.conv_rows and cfg.model.head_rows (both default on), a shape the kernel takes, and at least
        cfg.model.head_rows_min_wgs workgroups (one per sample and band of 14 rows)."""
        m = self.cfg.model
        return bool(not training and not self.precise and int(getattr(m, "conv_rows", 1)) and int(getattr(m, "head_rows", 1))
                    and conv_rows_head_covers(Hc, Wc, C1, N, G)
                    and B * -(-Hc // 14) >= int(getattr(m, "head_rows_min_wgs", HEAD_ROWS_MIN_WGS)))

    def _onepass_gn_covers(self, B, training):
        """Whether ctdd_unet_gn_onepass has a slab for every GroupNorm launch a one-pass plan would hold at its small levels (the
        fused blocks carry theirs inside): _PlanBuilder.build's walk over shapes alone, so that nothing is built to find out."""
        net, (_, H, W) = self.net, self.cfg.data.shape
        max_hw, threads = self._onepass_max_hw(), int(getattr(self.cfg.model, "gn_threads", 512))
        norms, c = [], net.channel                     # (pixels, GroupNorm) of every launch; channels of the running tensor
        for layer in [*list(net.down)[1:], *net.mid, *net.up]:
            if hasattr(layer, "downsample"):
                H, W = (H + 1 - 3) // 2 + 1, (W + 1 - 3) // 2 + 1
            elif not hasattr(layer, "resblocks"):      # Upsample
                H, W = 2 * H, 2 * W
            else:
                rb, c1 = layer.resblocks, layer.resblocks.norm1.num_channels
                cs = [c] if c1 == c else [c, c1 - c]                                                   # (c1 > c: the skip concatenation)
                if not (self._fuses_resblock(rb, H, W, cs, training) or self._fuses_resblock_mid(rb, H, W, cs, training)):
                    norms += [(H * W, rb.norm1), (H * W, rb.norm2)]
                c = rb.norm2.num_channels
                if layer.attention is not None:
                    norms.append((H * W, layer.attention.norm))
        norms.append((H * W, net.out[0]))
        return all(hw > max_hw or _onepass_slab(B, hw, n.num_channels, n.num_groups, threads) > 0 for hw, n in norms)

    def _build(self, B, x_dtype, logits_out=None, tc=None, logits_bf16=False, uniform_t=False):
        # bf16 inference plans: GroupNorm as one pass per tensor with the statistics inside (k_gn_onepass), no statistics in
        # the convolution epilogues (cfg.model.gn_onepass, default on); a net with a GroupNorm the kernel does not cover is
        # built the old way (statistics by the producers, k_gn_apply)
        # (training plans too, cfg.model.gn_onepass_train: the kernel then also writes each source's per-channel sums into the
        #  tensors' statistics buffers, which the GroupNorm backward reads)
        m = self.cfg.model
        onepass_gn = bool((not self.precise) and int(getattr(m, "gn_onepass", 1)) and (tc is None or int(getattr(m, "gn_onepass_train", 1)))
                          and self._onepass_gn_covers(B, tc is not None))
        return _PlanBuilder(self, B, tc, onepass_gn).build(x_dtype, logits_out, logits_bf16, uniform_t)

    # ------------------------------------------------------------------ execution
    def _run_plan(self, st):
        st.stats.zero_()
        st.zpool.zero_()
        for step in st.plan:
            step()

    def _prepare(self, B, x_dtype, x, times, logits_out=None, logits_bf16=False, uniform_t=False, time_row=None):
        """Build, warm up and capture the plan for (B, dtype)."""
        st = self._build(B, x_dtype, logits_out, logits_bf16=logits_bf16, uniform_t=uniform_t)
        st.x_in.copy_(x.reshape(st.x_in.shape))
        self._set_time(st, times, time_row)
        self._run_plan(st)                    # eager warm-up (also sets the LDS attributes)
        torch.cuda.synchronize()
        (st.graph,) = self._capture([lambda: self._run_plan(st)], "", "the plan runs as eager launches")
        return st

    def _capture(self, runs, what, then):
        """One HIP graph per callable of `runs`, or None for each: cfg.model.engine_graph off, or stream capture refused (a warning)."""
        if getattr(self.cfg.model, "engine_graph", True):
            try:
                graphs = []
                for run in runs:
                    graphs.append(torch.cuda.CUDAGraph())
                    with graph_capture(graphs[-1]):
                        run()
                return graphs
            except native.CtddError:          # a kernel refused its arguments: never hide that
                raise
            except RuntimeError as e:         # stream capture refused (a HIP error, not a kernel-argument error): eager launches
                import warnings
                warnings.warn(f"[ctdd] UNetEngine: HIP-graph capture{what} failed ({e}); {then}", RuntimeWarning)
                torch.cuda.synchronize()
        return [None] * len(runs)

    @staticmethod
    def _set_time(st, times, time_row):
        if st.time_row:
            if time_row is None or time_row.numel() != st.tproj.numel():
                raise native.CtddError("UNetEngine: this plan takes a precomputed time-projection row (time_table()[i])")
            st.tproj.copy_(time_row.reshape(st.tproj.shape))
        else:
            st.t_in.copy_(times.float())

    @staticmethod
    def _replay(st, x, times, time_row=None):
        st.x_in.copy_(x.reshape(st.x_in.shape))
        UNetEngine._set_time(st, times, time_row)
        if st.graph is not None:
            st.graph.replay()
        else:                                 # (stats / split-K pools are zeroed inside _run_plan for the eager path)
            raise native.CtddError("eager replay goes through _run_plan")

    def time_table(self, times):
        """(T,) times -> (T, Ntot) fp32: the time embedding MLP and every ResBlock's time projection for T time values at once
        (`ctdd_unet_time`, the per-sample path with the T values as its rows).  A sampler computes it for its whole grid when it
        starts and hands row i to step i (`time_row=`): the plans then run without the two time launches at their head."""
        lib = _lib()
        dev, ch = self.dev, self.net.channel
        _, pw, pb, tw = self._time_weights()
        t = times.to(dev).float().contiguous().reshape(-1)
        T, tdim, Ntot = t.numel(), ch * 4, pw.shape[1]
        hid = torch.empty((T, tdim), dtype=torch.float32, device=dev)
        act = torch.empty((T, tdim), dtype=torch.float32, device=dev)
        out = torch.empty((T, Ntot), dtype=torch.float32, device=dev)
        ta = _TimeArgs()
        ta.t, ta.B, ta.ch, ta.tdim = t.data_ptr(), T, ch, tdim
        ta.w1, ta.b1, ta.w2, ta.b2, ta.hid, ta.act = tw[0].data_ptr(), tw[1].data_ptr(), tw[2].data_ptr(), tw[3].data_ptr(), hid.data_ptr(), act.data_ptr()
        bound_launch(lib.ctdd_unet_time, C.byref(ta), pw.data_ptr(), pb.data_ptr(), Ntot, out.data_ptr())()
        return out

    def __call__(self, x, times, logits_bf16=False, uniform_time=False, slot=None, time_row=None):
        """logits_bf16: write the (B, D, S) logits in bf16 (bf16 engine: the output convolution's epilogue, or the logistic head).
        uniform_time: the caller guarantees that every entry of `times` is the same value (the sampler loops): the time path
        runs once, as one launch, for times[0].
        slot: the caller drives several INDEPENDENT sub-batches itself, each on its own stream (TauL's pipelined loop): plan
        `slot` has buffers of its own and replays on the caller's current stream, with no sub-batch split in here."""
        B = x.shape[0]
        lb = bool(logits_bf16) and not self.precise and (self.cfg.model.model_output == "logits" or self.net.S % 4 == 0)
        ut = "row" if time_row is not None else bool(uniform_time)          # (time_row: the row of time_table() for this call's time)
        ver = self._weights_version()
        if ver != self._wver:                     # weights changed (optimizer step, EMA swap): re-pack
            self._plans.clear()
            self._wver = ver
        if x.dtype not in (torch.int64, torch.int32):
            raise native.CtddError(f"UNetEngine expects integer states, got {x.dtype}")
        # Sub-batches on parallel streams: samples are independent, and two half-size forwards in flight fill the
        # CUs that one forward leaves idle (half-empty last rounds of the 392-tile grids, 98-workgroup 7x7 levels).
        nsub = int(getattr(self.cfg.model, "engine_streams", 2)) if slot is None else 1
        if nsub > 1 and B % nsub == 0 and B // nsub >= 32 and getattr(self.cfg.model, "engine_graph", True):
            key = (B, x.dtype, nsub, ut, lb)
            grp = self._plans.get(key)
            Bs = B // nsub
            xs = x.reshape(B, -1)
            if grp is None:
                C_, H_, W_ = self.cfg.data.shape
                logits = torch.empty((B, C_ * H_ * W_, self.net.S), dtype=torch.bfloat16 if lb else torch.float32, device=self.dev)
                subs = [self._prepare(Bs, x.dtype, xs[i * Bs:(i + 1) * Bs], times[i * Bs:(i + 1) * Bs], logits[i * Bs:(i + 1) * Bs],
                                      logits_bf16=lb, uniform_t=ut, time_row=time_row) for i in range(nsub)]
                grp = self._plans[key] = (logits, subs, [torch.cuda.Stream(device=self.dev) for _ in range(nsub - 1)])
            logits, subs, streams = grp
            if all(s.graph is not None for s in subs):
                main = torch.cuda.current_stream()
                ready = torch.cuda.Event()
                ready.record(main)
                done = []
                for i in range(1, nsub):
                    with torch.cuda.stream(streams[i - 1]):
                        streams[i - 1].wait_event(ready)
                        self._replay(subs[i], xs[i * Bs:(i + 1) * Bs], times[i * Bs:(i + 1) * Bs], time_row)
                        ev = torch.cuda.Event()
                        ev.record(streams[i - 1])
                        done.append(ev)
                self._replay(subs[0], xs[:Bs], times[:Bs], time_row)
                for ev in done:
                    main.wait_event(ev)
                return logits
        key = (B, x.dtype, ut, lb) if slot is None else (B, x.dtype, "slot", int(slot), ut, lb)
        st = self._plans.get(key)
        if st is None:
            st = self._plans[key] = self._prepare(B, x.dtype, x, times, logits_bf16=lb, uniform_t=ut, time_row=time_row)
        st.x_in.copy_(x.reshape(st.x_in.shape))
        self._set_time(st, times, time_row)
        if st.graph is not None:
            st.graph.replay()
        else:
            self._run_plan(st)
        return st.logits

    # ------------------------------------------------------------------ training (ctdd/unet_train.py lays the plans out)
    def _time_projections(self, times, resblocks):
        """temb -> every ResBlock's time projection, (B, Ntot): the B x 4ch time MLP stays differentiable device ops."""
        net = self.net
        act = torch.nn.functional.silu(net.time(times.float()))
        w = torch.cat([rb.time[1].weight for rb in resblocks], 0)
        b = torch.cat([rb.time[1].bias for rb in resblocks], 0)
        return torch.nn.functional.linear(act, w, b)

    def train_forward(self, x, times):
        """model(x, t) with gradients: logits (B, D, S) attached to autograd through ONE Function whose backward is the
        hand-written backward plan."""
        from . import unet_train
        unet_train.lib()                                   # (binds the training entry points' signatures)
        B = x.shape[0]
        if x.dtype not in (torch.int64, torch.int32):
            raise native.CtddError(f"UNetEngine expects integer states, got {x.dtype}")
        dropout = bool(self.model.training) and any(float(getattr(mod, "p", 0.0)) > 0 for mod in self.net.modules()
                                                    if mod.__class__.__name__ == "Dropout")
        key = (B, x.dtype, dropout)
        pool = self.__dict__.setdefault("_train_plans", {}).setdefault(key, [])
        st = next((p for p in pool if not p.busy), None)
        if st is None:
            if len(pool) >= int(getattr(self.cfg.model, "engine_train_plans", 3)):
                st = min(pool, key=lambda p: p.gen)          # oldest forward never got its backward: reuse, its ctx is invalidated
            else:
                tc = unet_train.TrainCtx(self, B, dropout)
                st = self._build(B, x.dtype, tc=tc)
                st.gen, st.busy, st.fgraph, st.bgraph = 0, False, None, None
                tc.rng[0] = native.dropout_seed()
                self._train_warm_and_capture(st, x, times)
                pool.append(st)
        tc = st.tc
        Cin, H0, W0 = self.cfg.data.shape
        tproj = self._time_projections(times, tc.resblocks)
        out = unet_train.UNetTrainFn.apply(self, st, x, times, tproj, *tc.engine_params)
        if self.cfg.model.model_output == "logistic_pars":
            from lib.models.models import logistic_logits
            no = out.view(B, H0 * W0, 2 * Cin)
            loc, log_scale = no[..., :Cin].permute(0, 2, 1), no[..., Cin:].permute(0, 2, 1)          # (B, C, HW)
            mu = torch.tanh(loc + st.x0.view(B, Cin, H0 * W0))
            logits = logistic_logits(mu.unsqueeze(-1), log_scale.unsqueeze(-1), self.net.S, bool(self.cfg.model.fix_logistic))
            return logits.reshape(B, Cin * H0 * W0, self.net.S)
        return out

    def _run_bwd_plan(self, st):
        tc = st.tc
        tc.zbuf.zero_()
        tc.bzpool.zero_()
        tc.gflat.zero_()
        for step in st.bwd_plan:
            step()

    def _train_warm_and_capture(self, st, x, times):
        """Run both plans once eagerly (first launches set kernel attributes), then capture each as ONE HIP graph."""
        with torch.no_grad():
            st.x_in.copy_(x.reshape(st.x_in.shape))
            st.t_in.copy_(times.float())
            st.tc.tproj.copy_(self._time_projections(times, st.tc.resblocks))
            self._run_plan(st)
            self._run_bwd_plan(st)                  # (zero seed: only exercises the launches)
            torch.cuda.synchronize()
            st.fgraph, st.bgraph = self._capture([lambda: self._run_plan(st), lambda: self._run_bwd_plan(st)], " of the training plans",
                                                 "eager launches")

    def _train_run_forward(self, st, x, times, tproj):
        st.gen = self.__dict__["_train_gen"] = self.__dict__.get("_train_gen", 0) + 1
        st.busy = True
        st.x_in.copy_(x.reshape(st.x_in.shape))
        st.t_in.copy_(times.float())
        st.tc.tproj.copy_(tproj.detach())
        if st.fgraph is not None:
            st.fgraph.replay()
        else:
            self._run_plan(st)
        out = st.net_out if self.cfg.model.model_output == "logistic_pars" else st.logits
        return out.clone()

    def _train_run_backward(self, st, gen, dout):
        if gen != st.gen:
            raise native.CtddError("the training plan of this forward was reused by a later forward before its backward ran "
                                   "(more concurrent training forwards than cfg.model.engine_train_plans)")
        tc = st.tc
        # gradients handed out by the previous backward are views of the arena: a caller that kept them (no zero_grad) gets copies
        lo, hi = tc.gflat.data_ptr(), tc.gflat.data_ptr() + 4 * tc.gflat.numel()
        for p in tc.engine_params:
            if p.grad is not None and lo <= p.grad.data_ptr() < hi:
                p.grad = p.grad.clone()
        Cin, H0, W0 = self.cfg.data.shape
        d = dout.detach().float()
        if self.cfg.model.model_output != "logistic_pars" and Cin > 1:        # (B, C*HW, S) -> NHWC rows [b*HW + p][c*S + s]
            S = self.net.S
            d = d.view(-1, Cin, H0 * W0, S).permute(0, 2, 1, 3)
        tc.seed_in.copy_(d.reshape(tc.seed_in.shape))
        if st.bgraph is not None:
            st.bgraph.replay()
        else:
            self._run_bwd_plan(st)
        st.busy = False
        grads = [tc.gflat[o:o + n].view(shape) for o, n, shape in (tc.grad_view[id(p)] for p in tc.engine_params)]
        return tc.dtproj.clone(), grads
