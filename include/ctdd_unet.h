/* ctdd_unet.h -- C ABI of the U-Net inference kernels in libctdd.so (csrc/unet_kernels.hip).
 *
 * These entry points replace the forward pass of the reference's score network on the sampling
 * path: TAUnSDDM/lib/networks/unet.py:419-459 (UNet.forward) with its blocks (ResBlock 100-140,
 * Downsample/Upsample 79-97, SelfAttention/QKVAttention 152-200, TimeEmbedding 223-241) and the
 * logistic head of TAUnSDDM/lib/models/models.py:249-283.  Same conventions as ctdd.h: caller-
 * owned device pointers, hipStream_t as void*, 0 / negative status.  Argument blocks are plain C
 * structs passed by pointer (host memory); the Python host mirrors them with ctypes.Structure
 * (ctdd/unet_engine.py).  All activations are NHWC.
 */
#ifndef CTDD_UNET_H
#define CTDD_UNET_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* K-segment kinds of the implicit-GEMM convolution */
#define CTDD_SEG_3x3 0     /* 3x3, stride 1, pad 1                                   (unet.py:41-61)  */
#define CTDD_SEG_1x1 1     /* 1x1: ResBlock linear skip / attention qkv, proj        (119-138,165-167)*/
#define CTDD_SEG_3x3_S2 2  /* 3x3, stride 2, input padded (0,1,0,1)                  (88-97)          */
#define CTDD_SEG_3x3_UP 3  /* 3x3 pad 1 on the nearest-2x upsampled input            (79-85)          */
#define CTDD_SEG_3x3_S2T 4 /* transpose of CTDD_SEG_3x3_S2: data gradient of the Downsample conv (backward of 88-97); the
                              output grid (H, W) is the forward's input grid, (Hin, Win) the forward's output grid;
                              ctdd_unet_conv (generic kernel) only */

typedef struct { const void* hi; const float* f32; int C, kind; } ctdd_conv_seg;   /* [B][Hin][Win][C] bf16 | fp32 */
typedef struct {
  ctdd_conv_seg seg[3]; int nseg;
  const void* w_hi; const float* w_f32;        /* [N][Ktot] bf16 | fp32, K = segment -> tap -> channel */
  int B, H, W, Hin, Win, N, Ktot;
  const float* bias; const float* tbias; int tb_stride;
  const float* res_f32; const void* res_bf16;
  float* out_f32; void* out_hi; double* stats; int logits_C;   /* stats: [B][N][2] fp64 sum / sum of squares */
  int ksplit; float* acc_buf;                                  /* split-K: zeroed [M][N] fp32 partial-sum buffer */
  int act;                                                     /* 0 none, 1 ReLU, 2 GELU(erf) on acc + bias, before the residual (not in res / ring) */
  void* out_lo;                                                /* ctdd_unet_conv_patch: optional bf16(out - out_hi), the second term of a split operand */
} ctdd_conv_args;
/* out = conv(segments) + bias + tbias[b] + residual; bk in {96,64,32,16}, bnt = N-tile/32,
 * f32 = 0: bf16 MFMA, 1: exact-fp32 MFMA.
 * A bf16 call (f32 = 0) with exactly one CTDD_SEG_3x3_S2 segment (the Downsample convolution) runs on the stride-2
 * ring kernel whatever (bk, bnt) it names, when Hin = 2 H, Win = 2 W, W <= 16, C % 16 == 0, N % 32 == 0,
 * Ktot = 9 C, ksplit <= 1, H*W >= 32 or == 16 or B == 1, no logits layout / activation / out_lo, 16-byte aligned
 * tensors, 4*B*H*W < 2^31.  Every other call runs on the generic gather kernel as before; the results of the two
 * differ by the order of the fp32 sums only.  CTDD_CONV_S2_OLD=1 in the environment (read once per process) keeps
 * the generic kernel for those calls too.
 * The generic kernel takes any grid: with fewer than 32 pixels per sample (other than 16) and B > 1 each output row
 * looks up its own sample for tbias, the logits layout and the statistics.  CTDD_ERANGE where the statistics of one
 * 128-row tile (ceil(128 / (H*W)) + 1 samples x 32 bnt columns x 16 bytes) exceed the 160 KiB of LDS. */
int ctdd_unet_conv(const void* conv_args, int bk, int bnt, int f32, void* stream);
/* bf16 throughput kernel for stride-1 3x3 / 1x1 segments: the input slab of a pixel tile is staged in
 * LDS once per channel chunk and shared by the nine taps; bk in {48,64,32,16}, wm = rows per wave */
int ctdd_unet_conv_patch(const void* conv_args, int bk, int bnt, int wm, void* stream);
/* same contract, 512-pixel tiles with the weights of all nine taps of a 32-channel chunk resident in LDS
 * (no barrier between taps); segment channel counts must be multiples of 32; bnt in {2,3,4} */
int ctdd_unet_conv_res(const void* conv_args, int bnt, void* stream);
/* same contract, 16-channel units moved global -> LDS by LDS-DMA into a ring of unit buffers (no staging
 * registers, one barrier per unit); segment channel counts must be multiples of 16; bnt in {2,3,4}: 512-pixel
 * tiles, eight waves; bnt in {12,13}: N-tile 64/96 with 256-pixel tiles, four waves, two workgroups per CU */
int ctdd_unet_conv_ring(const void* conv_args, int bnt, void* stream);
/* The Upsample convolution (unet.py:79-85: 3x3, pad 1, on the nearest-2x grid) as four 2x2-tap phase convolutions of the
 * low-resolution tensor, one launch, the 2x grid never materialised; bf16 only (f32 must be 0).  One CTDD_SEG_3x3_UP segment
 * [B][Hin][Win][C]; (H, W) = (2 Hin, 2 Win) is the output grid; Ktot = 4 C and w_hi is [4][N][4 C]: phase 2 py + px of output
 * pixel (2y + py, 2x + px), K = tap 2 i + j -> channel, tap (i, j) on source pixel (y + py + i - 1, x + px + j - 1), its weight
 * the sum of the 3x3 weights that read that pixel: rows {W[0], W[1] + W[2]} for py = 0, {W[0] + W[1], W[2]} for py = 1, columns
 * alike with px (ctdd/unet_engine.py: fold_upsample_weights).  out_hi + bias (+ stats, summed over the four phases) only.
 * C % 16 == 0, N % 96 == 0 or N % 64 == 0, Win <= 33, Hin * Win >= 32, ksplit <= 1, 16-byte aligned tensors; anything else:
 * CTDD_EINVAL / CTDD_ERANGE, nothing launched. */
int ctdd_unet_conv_up_phases(const void* conv_args, int f32, void* stream);
int ctdd_unet_upsample2x(const void* x_bf16,int B, int H, int W, int C, void* out_bf16, void* stream);   /* unet.py:79-85 */

typedef struct {
  const int64_t* x64; const int32_t* x32; float lo, hi; const float* w; const float* bias;
  int B, Cin, H, W, Cout; float* out_f32; void* out_hi; double* stats; float* x0_f32;
} ctdd_first_conv_args;
/* center_data + first conv3x3 on the integer state (unet.py:428, network_utils.py:23-25) */
int ctdd_unet_first_conv(const void* first_conv_args, void* stream);

typedef struct {
  const float* s1_f32; const void* s1_bf16; const double* st1; int C1;
  const float* s2_f32; const void* s2_bf16; const double* st2; int C2;
  const float* gamma; const float* beta; int B, HW, G; float eps; int swish; void* out_hi; float* out_f32;
} ctdd_gn_args;
/* GroupNorm (+Swish) of the channel concatenation of one or two tensors (unet.py:103-133, 403-416) */
int ctdd_unet_gn_apply(const void* gn_args, void* stream);
/* The same normalisation of bf16 tensors in one pass over memory, statistics included (st1 / st2 are not read): a workgroup owns
 * (sample, slab of whole groups) and holds it in registers between the reduction and the write.  slab_channels: a multiple of
 * lcm(C / G, 8) dividing C, or 0 to let the library choose; max_threads: workgroup size limit (0: 1024); CTDD_ERANGE when no slab
 * fits (fall back to ctdd_unet_gn_apply). */
int ctdd_unet_gn_onepass(const void* gn_args, int slab_channels, int max_threads, void* stream);
int ctdd_unet_channel_stats(const float* x, int B, int HW, int C, double* stats, void* stream);

typedef struct {
  const void* s1_bf16; const void* s2_bf16; int C1, C2;   /* raw input [B][H][W][C1] (+ [B][H][W][C2]: their channel concatenation) */
  const float* gamma1; const float* beta1; const float* gamma2; const float* beta2; int G1, G2; float eps1, eps2;
  const void* w1; const float* bias1; const float* tbias; int tb_stride;   /* conv1: the [N][9 (C1 + C2)] bf16 matrix, K = tap -> channel, in fragment order (below) */
  const void* w2; const float* bias2;   /* conv2: [N][9 N (+ C1 + C2)], the 3x3 segment on a2, then the 1x1 skip segments on the raw input; fragment order */
  int skip;                             /* 1: 1x1 skip segments (their bias summed into bias2); 0: residual = the raw input (C1 == N, C2 == 0) */
  int B, H, W, N; void* out_bf16;       /* [B][H][W][N] bf16 */
} ctdd_resblock_args;
/* A whole ResBlock (unet.py:100-140, eval mode) of a small level in one launch, bf16: GroupNorm + Swish -> conv3x3 + bias + time bias
 * -> GroupNorm + Swish -> conv3x3 (+ 1x1 skip | + residual), one workgroup per sample, intermediates in LDS, the rounding points of
 * the four launches it replaces (ctdd_unet_gn_onepass, ctdd_unet_conv_patch, twice).  H * W <= 64, W <= 8, and for more than 16
 * pixels (H - 1)(W + 2) + W <= 80 (the pixel tiles are 16 consecutive rows of the zero-bordered LDS image, row stride 2 C + 32
 * bytes, five tiles at most); N = 192, C1 and C2 multiples of 64 with C1 + C2 <= 384; f32 must be 0.  Anything else: CTDD_ERANGE /
 * CTDD_EINVAL, nothing launched.
 * Weights in fragment order: element (n, k) of the [N][K] matrix, n = 48 wave + 16 tile + i, k = 64 chunk + 32 half + 8 q + e, is at
 * ((((wave * K / 64 + chunk) * 3 + tile) * 2 + half) * 64 + 16 q + i) * 8 + e (ctdd/unet_engine.py: pack_resblock_weights): each
 * wave-instruction of the kernel's weight stream reads 1 KiB of consecutive bytes. */
int ctdd_unet_resblock_small(const void* resblock_args, int f32, void* stream);
/* The same block, same argument struct, for a sample of up to 14 x 14 pixels (the 14x14 level): H <= 14, W <= 14, N = 192, C1 and C2
 * multiples of 32 with C1, C2 <= 192; f32 must be 0.  LDS holds one zero-bordered 192-channel slab (16 positions per padded grid
 * row whatever W, row stride 416 bytes, a guard row at either end) and no copy of the input: GroupNorm 1 reads the sources from
 * global memory and conv1 runs source by source.  A pixel tile is one output row; the K loop's unit is (32 channels, dx), whose row
 * fragments are read once and used by the three dy.  Anything else: CTDD_ERANGE / CTDD_EINVAL, nothing launched.
 * Weights (ctdd/unet_engine.py: pack_resblock_mid_weights = pack_row_tile_weights, four streams): a stream per wave (output channels [48 wave, 48 wave + 48)), the four
 * streams one after the other, each a sequence of 1 KiB fragments.  A fragment is (tile, 32 channels of K): element
 * (n = 48 wave + 16 tile + i, k = 8 q + e of the 32) at (16 q + i) * 8 + e.  conv1: for each source, for each 32-channel block of
 * it, for dx = -1, 0, 1, for dy = -1, 0, 1, for tile = 0, 1, 2: the fragment of tap (dy, dx) on that block (27 (C1 + C2) / 32
 * fragments per wave; nothing is padded).  conv2: the 3x3 segment on a2 in the same order (162 fragments), then for each source,
 * for each 32-channel block of it, for tile = 0, 1, 2: the fragment of the 1x1 skip segment (3 (C1 + C2) / 32 fragments). */
int ctdd_unet_resblock_mid(const void* resblock_args, int f32, void* stream);

typedef struct {
  const void* s1_bf16; const double* st1; int C1;   /* GroupNorm sources [B][H][W][C1] (+ [B][H][W][C2]) and their [B][C][2] fp64 sums */
  const void* s2_bf16; const double* st2; int C2;   /* (the statistics format of ctdd_conv_args.stats / ctdd_gn_args.st1) */
  const float* gamma; const float* beta; int G; float eps;   /* GroupNorm over the C1 + C2 channels of the concatenation */
  const void* w; const float* bias; const float* tbias; int tb_stride;   /* [N][9 (C1 + C2) + RC1 + RC2] bf16 in stream order (below) */
  const void* r1_bf16; int RC1; const void* r2_bf16; int RC2;   /* raw sources of the 1x1 segments (RC1 = 0: none) */
  const void* res_bf16;                             /* residual [B][H][W][N] or null */
  void* out_bf16; double* out_stats;                /* [B][H][W][N]; [B][N][2] fp64 sums of the output, added to (or null) */
  int B, H, W, N;
} ctdd_conv_rows_args;
/* GroupNorm + Swish + 3x3 convolution in one launch for a level whose samples do not fit one workgroup (csrc/unet_rows_kernels.hip):
 *   out = bf16(conv3x3(bf16(swish(GN(concat(s1[, s2]))))) [+ 1x1 on raw r1[, r2]] + bias [+ tbias[b]] [+ residual])
 * the ctdd_unet_gn_apply + ctdd_unet_conv_ring / ctdd_unet_conv_patch pair without the activated tensor in memory; scale / shift come
 * from st1 / st2 as in ctdd_unet_gn_apply, the output's sums (taken before the bf16 rounding) are added into out_stats
 * by one fp64 atomic per band (bit-reproducible from a zeroed buffer for H <= 28, two bands; beyond that up to the order of the adds).  One
 * workgroup of eight waves per (sample, band of 14 output rows): a wave owns 7 rows x 48 channels x a column half.  1 <= W <= 28, any H, N = 96, C1, C2, RC1, RC2 multiples of 32 (C2, RC1, RC2 may
 * be 0; RC2 > 0 needs RC1 > 0; <= 384 channels per concatenation), G divides C1 + C2, every GroupNorm source with statistics,
 * 1x1 segments or a residual but not both (a ResBlock has one of them), 16-byte aligned tensors, f32 must be 0.  Anything else: CTDD_ERANGE / CTDD_EINVAL, nothing launched.
 * Weights (ctdd/unet_engine.py: pack_conv_rows_weights = pack_row_tile_weights, the same order in two streams): two streams (output channels [48 s, 48 s + 48)), one after the other, each a
 * sequence of 1 KiB fragments.  A fragment is (tile, 32 channels of K): element (n = 48 s + 16 tile + i, k = 8 q + e of the 32) at
 * (16 q + i) * 8 + e.  Per stream: for each GroupNorm source, for each 32-channel block of it, for dx = -1, 0, 1, for dy = -1, 0, 1,
 * for tile = 0, 1, 2: the fragment of tap (dy, dx) on that block (27 (C1 + C2) / 32 fragments); then for each raw source, for each
 * 32-channel block of it, for tile = 0, 1, 2: the fragment of the 1x1 segment (3 (RC1 + RC2) / 32 fragments).  Nothing is padded. */
int ctdd_unet_conv_rows(const void* conv_rows_args, int f32, void* stream);
/* The same launch, same arguments, weights and refusals, on four waves per workgroup (a wave owns the band's 14 rows x 48 channels x
 * a column half): output and out_stats are bit-identical to ctdd_unet_conv_rows' (the sums keep one order: fp32 down a lane's
 * column in row order, then fp64), so either stands in for the other (cfg.model.conv_rows_waves = 4 | 8). */
int ctdd_unet_conv_rows_w4(const void* conv_rows_args, int f32, void* stream);
/* The output head of such a level on the same argument struct (csrc/unet_head_kernels.hip): GroupNorm + Swish + 3x3 convolution
 * into N output channels in one launch,
 *   out[b][y][x][0..N) = bf16(conv3x3(bf16(swish(GN(s1)))) + bias)
 * the ctdd_unet_gn_apply + ctdd_unet_conv_ring pair without the activated tensor in memory, the rounding points of the pair.  One
 * workgroup per (sample, band of 14 output rows) fills the slab of ctdd_unet_conv_rows once and runs ceil(N / 96) passes of 96
 * output channels over it; the output row pitch is N elements and a pass writes channels [96 p, min(96 p + 96, N)) of a pixel.
 * 1 <= W <= 28, any H, one GroupNorm source with statistics and C1 = 32, 64 or 96, G divides C1, N a multiple of 32 with
 * 32 <= N <= 576, C2 = RC1 = RC2 = 0, res_bf16, tbias and out_stats null, 16-byte aligned tensors, f32 must be 0.  Anything else:
 * CTDD_ERANGE / CTDD_EINVAL, nothing launched.
 * Weights (ctdd/unet_engine.py: pack_conv_rows_head_weights): the [N][9 C1] matrix zero-padded to 96 ceil(N / 96) rows, in
 * 2 ceil(N / 96) streams of ctdd_unet_conv_rows' order (stream s: output channels [48 s, 48 s + 48), 27 C1 / 32 fragments), one after
 * the other: pass p reads streams 2 p and 2 p + 1.  Channels >= N are computed and never stored.  The workgroup has eight waves: a
 * wave owns 7 rows x 48 channels x a column half of the current pass. */
int ctdd_unet_conv_rows_head(const void* conv_rows_args, int f32, void* stream);
/* The same launch, same arguments, weights and refusals, on four waves per workgroup (a wave owns the band's 14 rows x 48 channels x
 * a column half): the output is bit-identical to ctdd_unet_conv_rows_head's (per output pixel the order of the sums is the same),
 * so either stands in for the other (cfg.model.head_rows_waves = 4 | 8). */
int ctdd_unet_conv_rows_head_w4(const void* conv_rows_args, int f32, void* stream);

typedef struct {
  const float* t; int B, ch, tdim;
  const float* w1; const float* b1; const float* w2; const float* b2;   /* Linear weights transposed to [in][out] */
  float* hid; float* act;                                                /* [B][tdim] scratch, [B][tdim] = swish(temb) */
} ctdd_time_args;
/* sinusoid -> Linear -> Swish -> Linear -> Swish, then every ResBlock's time projection (unet.py:223-241,332-337,110);
 * proj_w = the concatenated projection weights transposed to [tdim][Ntot] */
int ctdd_unet_time(const void* time_args, const float* proj_w, const float* proj_b, int Ntot, float* proj_out, void* stream);
/* the same for ONE time shared by every sample (the samplers pass t * ones((N,)), sampling.py:119-121): t[0] only, one launch,
 * proj_out is a single row (Ntot) that the convolutions read with a zero batch stride */
int ctdd_unet_time_uniform(const void* time_args, const float* proj_w, const float* proj_b, int Ntot, float* proj_out, void* stream);

typedef struct { const float* qkv; int B, T, C, heads; void* out_hi; float* out_f32; } ctdd_attn_args;
int ctdd_unet_attention(const void* attn_args, void* stream);              /* unet.py:176-200 */

typedef struct {
  const void* an_bf16; const void* x_bf16;          /* [B][T][C] bf16: the block's GroupNorm output (ctdd_unet_gn_onepass) and its raw input (the residual) */
  const void* w_qkv; const float* b_qkv;            /* [3 C][C] bf16 in fragment order (below), [3 C] fp32; output channels in the reference's order, [q | k | v] per head */
  const void* w_proj; const float* b_proj;          /* [C][C] bf16 in fragment order, [C] fp32 */
  int B, T, C, heads; void* out_bf16;               /* [B][T][C] bf16 */
} ctdd_attn_block_args;
/* The mid-block self-attention behind its GroupNorm (unet.py:152-200) in one launch, bf16 (csrc/unet_attn_kernels.hip):
 *   qkv = an Wqkv^T + b_qkv (fp32) -> per head softmax((q s)(k s)^T) v, s = (C / heads)^-1/4 (fp32) -> ao (bf16)
 *   out = bf16(ao Wproj^T + b_proj + x)
 * one workgroup per sample, qkv and ao never leave the CU; the rounding points of the three launches it replaces (ctdd_unet_conv_patch
 * into fp32, ctdd_unet_attention, ctdd_unet_conv_patch with a residual), the fp32 sums in another order (accumulators start from the
 * bias) and the softmax's exponential as the hardware exp2 of (s - max) log2 e.  C = 192 in 8 heads, T <= 64,
 * 16-byte aligned tensors, f32 must be 0.  Anything else (fp32 mode, other channel or head counts, a head width that is not a multiple
 * of 4, T > 64: the LDS image would pass 160 KiB): CTDD_ERANGE / CTDD_EINVAL, nothing launched.
 * Weights (ctdd/unet_engine.py: pack_attention_weights): element (n, k) of an [N][C] matrix, N = 4 waves x NT tiles x 16 (NT = 9 for
 * qkv, 3 for proj), n = 16 (NT wave + tile) + i, k = 32 step + 8 q + e, is at ((((wave * C / 32 + step) * NT + tile) * 4 + q) * 16 + i) * 8 + e:
 * a stream per wave, each wave-instruction reading 1 KiB of consecutive bytes. */
int ctdd_unet_attention_block(const void* attn_block_args, int f32, void* stream);

typedef struct { const float* net; const float* x0; int B, C, HW, S, fix; float* out;
                 int fast;   /* 1: hardware exp2/log2 forms (bf16 engine mode) */
                 void* out_bf16;   /* or null; fast mode, S % 4 == 0: the (B, D, S) logits in bf16 instead of `out` (the sampler
                                    * loops of the bf16 engine: half the bytes of the head's write and the step's read) */ } ctdd_logistic_args;
int ctdd_unet_logistic_head(const void* logistic_args, void* stream);      /* models.py:249-283 */

#ifdef __cplusplus
}
#endif
#endif
