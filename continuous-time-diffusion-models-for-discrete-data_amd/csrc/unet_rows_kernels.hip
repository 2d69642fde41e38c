// unet_rows_kernels.hip -- GroupNorm + Swish + 3x3 convolution (+ 1x1 skip segments | + residual) of a level whose samples do
// NOT fit one workgroup (28x28, N = 96), as ONE launch on the row-tile K loop of k_resblock_mid (row_tile.hpp).
//
//   out = bf16( conv3x3( bf16(swish(GN(concat(s1[, s2])))) ) [+ 1x1 on raw r1[, r2]] + bias [+ tbias[b]] [+ residual] )
//
// replaces a k_gn_apply + k_conv_ring / k_conv_patch pair: the activated tensor is never written to memory.  At this level the
// producers leave fp64 per-(sample, channel) sums (ConvArgs.stats), so the GroupNorm needs no pass of its own and no workgroup
// waits for another: every workgroup folds the sums of its sample into scale / shift itself (the head of k_gn_apply) and
// normalises what it reads on the way into LDS.  The rounding points are those of the pair: the activated operand is rounded to
// bf16, accumulation is fp32 on the matrix cores, acc + bias + time bias + residual is rounded once; the output's own statistics
// are taken on the fp32 value before that rounding, as conv_epilogue_rows takes them.
//
// Work split: one workgroup per (sample, band of 14 output rows), of eight waves (ctdd_unet_conv_rows) or four
// (ctdd_unet_conv_rows_w4); wave ([rh,] cg, h) owns output channels [48 cg, 48 cg + 48) x column half h [x rows 7 rh .. 7 rh + 6 of
// the band]: lane j of half h is padded column 16 h + j (pixel x = 16 h + j - 1; lanes off the image compute values that are
// never stored).  A pixel tile is one output row of one column half: 14 (7) row tiles x 3 channel tiles of
// v_mfma_f32_16x16x32_bf16 (weights as the A operand: a lane's four results are four consecutive channels of one pixel), 168 (84)
// accumulator registers; four waves are the shape of k_resblock_mid, one wave per SIMD, eight put two on every SIMD.
//
// LDS: one zero-bordered slab of at most 96 channels: (14 + 2) padded rows x 32 positions, a guard position at either end, 224 bytes
// per position (192 + 32: sixteen consecutive positions at 224 bytes are conflict-free under the lane groups of ds_read_b128 for
// every base and every 32-channel offset, tools/lds_bank_model.py; 192 and 208 bytes cost 8 cycles instead of 4) = 115 136 bytes,
// then scale / shift of all source channels and the statistics scratch.  The sources enter in PIECES of <= 96 channels (a
// 192-channel source is two): normalise + Swish the band's rows and one halo row each side from global memory into the slab
// through registers, barrier, the piece's (32 channels, dx) units, barrier.  Unit: the 16 row fragments of that column shift are
// read ONCE, output row y takes nine matrix instructions (three dy x three weight tiles) on F[y], F[y + 1], F[y + 2]: 16
// ds_read_b128 per 126 matrix instructions.  The weights stream global -> registers through a ring of two units (ctdd_unet.h:
// pack_conv_rows_weights = pack_row_tile_weights' order in two streams; the two column halves of a channel group read the same stream).  Border positions, positions
// past W and rows outside the image are never written after the prologue's zero fill.
#include "row_tile.hpp"
#include "../../include/ctdd_unet.h"

namespace ctdd {
namespace {

constexpr int CR_N = 96, CR_BAND = 14, CR_PITCH = 32, CR_RS = 224, CR_MAXW = 28, CR_MAXC = 384, CR_PIECE = 96;
constexpr int CR_SLAB = ((CR_BAND + 2) * CR_PITCH + 2) * CR_RS;  // 115 136
constexpr int CR_SCALE = CR_SLAB;                                // float scale[CR_MAXC], shift[CR_MAXC]
constexpr int CR_RED = CR_SCALE + 2 * CR_MAXC * 4;               // double [column half][channel][moment] (four waves)
constexpr int CR_TOTAL = CR_RED + 2 * CR_N * 2 * 8;
constexpr int CR_FB = 12;                                        // pixels per thread in flight in the fill (half of them with eight waves)
constexpr int CR_CARRY = CR_BAND * CR_MAXW * CR_RS;               // eight waves: float4 [wave & 3][channel tile][s | q][lane] past the output image
static_assert(CR_CARRY + 4 * 3 * 2 * 64 * 16 <= CR_SLAB, "the output image and the upper waves' partial sums reuse the slab");

// bf16(swish(x * scale + shift)) of one piece (`pc` channels from `src`, the sample's first pixel at the piece's first channel,
// pixel stride `cs` channels; channels [coff, coff + pc) of the concatenation) into columns [0, pc) of the slab: padded rows
// rlo .. rhi of the band (image rows y0 - 1 + r), which are consecutive pixels in memory.  No barrier of its own.
template <int THREADS, int FB>
__device__ __attribute__((always_inline)) inline void cr_fill(unsigned char* sm, const unsigned short* __restrict__ src, int cs, int pc, int coff,
                                                             int y0, int H, int W) {
  const int t = threadIdx.x, noct = pc >> 3, npl = THREADS / noct;
  if (t >= noct * npl) return;
  const int oct = t % noct, pl = t / noct;
  const float* scale = (const float*)(sm + CR_SCALE) + coff + oct * 8;
  const float* shift = scale + CR_MAXC;
  const float4 sc0 = *(const float4*)scale, sc1 = *(const float4*)(scale + 4);
  const float4 sh0 = *(const float4*)shift, sh1 = *(const float4*)(shift + 4);
  const f32x2v scv[4] = {{sc0.x, sc0.y}, {sc0.z, sc0.w}, {sc1.x, sc1.y}, {sc1.z, sc1.w}};
  const f32x2v shv[4] = {{sh0.x, sh0.y}, {sh0.z, sh0.w}, {sh1.x, sh1.y}, {sh1.z, sh1.w}};
  const int rlo = y0 == 0 ? 1 : 0, rhi = H - y0 < CR_BAND + 1 ? H - y0 : CR_BAND + 1;
  const unsigned npix = (unsigned)((rhi - rlo + 1) * W), uW = (unsigned)W;
  const unsigned short* sp = src + (size_t)((y0 - 1 + rlo) * W) * cs + oct * 8;
  unsigned char* dst = sm + (1 + rlo * CR_PITCH + 1) * CR_RS + oct * 16;
  // FB pixels per thread in flight (a 96-channel piece of a 16-row band is 22 pixels per thread of 256 at 12 in flight, 11 per
  // thread of 512 at 6, where 12 spill: two round trips to memory, not six); the loads are unconditional on a clamped pixel, only
  // the LDS stores are predicated
  for (unsigned p0 = (unsigned)pl; p0 < npix; p0 += (unsigned)(FB * npl)) {
    u32x4 u[FB];
#pragma unroll
    for (int k = 0; k < FB; ++k) {
      const unsigned p = p0 + (unsigned)(k * npl);
      u[k] = *(const u32x4*)(sp + (size_t)(p < npix ? p : npix - 1) * cs);
    }
#pragma unroll
    for (int k = 0; k < FB; ++k) {
      const unsigned p = p0 + (unsigned)(k * npl);
      unsigned ow[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {                              // as k_gn_apply / rm_gn1_apply: packed fma, hardware exp2 / rcp
        const f32x2v x = {__uint_as_float(u[k][j] << 16), __uint_as_float(u[k][j] & 0xFFFF0000u)};
        f32x2v y = __builtin_elementwise_fma(x, scv[j], shv[j]);
        const f32x2v z = y * (f32x2v){-1.4426950408889634f, -1.4426950408889634f};
        const f32x2v d = (f32x2v){__builtin_amdgcn_exp2f(z.x), __builtin_amdgcn_exp2f(z.y)} + (f32x2v){1.0f, 1.0f};
        y = y * (f32x2v){__builtin_amdgcn_rcpf(d.x), __builtin_amdgcn_rcpf(d.y)};
        ow[j] = rt_pack2(y.x, y.y);
      }
      const unsigned rr = p / uW, x = p - rr * uW;
      if (p < npix) *(uint4*)(dst + (rr * CR_PITCH + x) * CR_RS) = make_uint4(ow[0], ow[1], ow[2], ow[3]);
    }
  }
}

// The 1x1 segments: nsk 32-channel units of the raw sources, B fragments straight from global memory (lane j of tile y: pixel
// (y0 + y, xc), y0 the wave's first row, rows and columns off the image clamped into it: computed, never stored), weight ring ws
// holding units 0 and 1.
template <int NPT>
__device__ __attribute__((always_inline)) inline void cr_gemm_skip(f32x4 (&acc)[3][NPT], u32x4 (&ws)[2][3], const unsigned short* __restrict__ wrow, int nsk,
                                                                  const unsigned short* __restrict__ r1, const unsigned short* __restrict__ r2,
                                                                  int C1, int C2, int xc, int lq, int y0, int H, int W) {
  const int nc1 = C1 >> 5;
  auto gload = [&](bf16x8 (&g)[NPT], int u) {
    const int ue = u < nsk ? u : nsk - 1;                       // past the last unit: the last unit again
    const bool two = ue >= nc1;
    const unsigned char* base = (const unsigned char*)(two ? r2 : r1);
    const int cs = two ? C2 : C1, cb = (ue - (two ? nc1 : 0)) * 32 + lq * 8;
#pragma unroll
    for (int y = 0; y < NPT; ++y) {
      const int ye = y0 + y < H ? y0 + y : H - 1;
      g[y] = *(const bf16x8*)(base + (unsigned)(((ye * W + xc) * cs + cb) * 2));
    }
  };
  auto step = [&](u32x4 (&slot)[3], bf16x8 (&gc)[NPT], bf16x8 (&gn)[NPT], int u, auto guard) {
    constexpr bool GUARD = decltype(guard)::value;
    if (GUARD && u >= nsk) return;
    gload(gn, u + 1);
#pragma unroll
    for (int y = 0; y < NPT; ++y)
#pragma unroll
      for (int t = 0; t < 3; ++t)
        acc[t][y] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, slot[t]), gc[y], acc[t][y], 0, 0, 0);
    if (!GUARD || u + 2 < nsk) rt_wload3(slot, wrow, u + 2);
    __builtin_amdgcn_sched_barrier(0);
  };
  bf16x8 G[2][NPT];
  gload(G[0], 0);
  __builtin_amdgcn_s_waitcnt(0x0F70);                           // vmcnt(0): unit 0's fragments are needed at once
  int u0 = 0;
  for (; u0 + 4 <= nsk; u0 += 2) {
    step(ws[0], G[0], G[1], u0, std::false_type{});
    step(ws[1], G[1], G[0], u0 + 1, std::false_type{});
  }
  for (; u0 < nsk; u0 += 2) {
    step(ws[0], G[0], G[1], u0, std::true_type{});
    step(ws[1], G[1], G[0], u0 + 1, std::true_type{});
  }
}

#ifdef CTDD_ROWS_STAMPS
// phase stamps (tools/build_conv_stamps.sh, tools/stamp_conv_rows.py): thread 0 of every workgroup leaves s_memtime at the phase
// boundaries in a [workgroups][8] buffer passed in place of out_stats (the statistics are off in this build)
#define CR_STAMP(i_)                                                                                      \
  do {                                                                                                    \
    unsigned long long t_;                                                                                \
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");                            \
    if (threadIdx.x == 0) ((unsigned long long*)a.out_stats)[(size_t)blockIdx.x * 8 + (i_)] = t_;         \
  } while (0)
#else
#define CR_STAMP(i_)
#endif

// SKIP: with 1x1 segments and no residual; otherwise a residual (or neither) and no 1x1 segments -- a ResBlock has one or the
// other, and one instantiation holding both loses its register allocation (189 spilled registers in the K loops)
//
// WAVES: 4 -- wave (cg, hh) owns the band's 14 rows; 8 -- wave (rh, cg, hh) owns rows [7 rh, 7 rh + 7) of the band, 84 accumulator
// registers, two waves per SIMD: waves wv and wv + 4 share a SIMD and a weight stream, and 512 threads carry the fill, the zero
// fill and the store.  Per output pixel the order of units, dy and tiles is the same, and the statistics keep the 4-wave chain
// (fp32 down a lane's column in row order, then fp64): the upper wave leaves its running fp32 sums in LDS and the lower wave
// continues from them, and the 16 lanes of a column half are added in fp64 from LDS in the order of the 4-wave kernel's lane
// butterfly, so both give the same bits.
template <bool SKIP, int WAVES>
__global__ __launch_bounds__(WAVES * 64, 1) void k_conv_rows(const ctdd_conv_rows_args a) {
  static_assert(WAVES == 4 || WAVES == 8, "one or two row halves");
  constexpr int CR_THREADS = WAVES * 64, NPT = CR_BAND * 4 / WAVES;   // rows of a wave
  extern __shared__ __attribute__((aligned(16))) unsigned char sm[];
  const int t = threadIdx.x;
  const int H = a.H, W = a.W, HW = H * W, C1 = a.C1, C2 = a.C2, C = C1 + C2;
  const int nbands = (H + CR_BAND - 1) / CR_BAND;
  const int b = blockIdx.x / nbands, y0 = (blockIdx.x - b * nbands) * CR_BAND;
  const int lane = t & 63, wv = t >> 6, lj = lane & 15, lq = lane >> 4, cg = WAVES == 8 ? (wv >> 1) & 1 : wv >> 1, hh = wv & 1;
  const int rh = WAVES == 8 ? __builtin_amdgcn_readfirstlane(wv >> 2) : 0, yw = y0 + NPT * rh;  // the wave's row half, its first image row
  const int nu3 = 3 * (C >> 5), nsk = SKIP ? (a.RC1 + a.RC2) >> 5 : 0;
  const unsigned short* wrow = (const unsigned short*)a.w + (size_t)cg * ((size_t)nu3 * RT_UNIT + (size_t)nsk * 1536) + lane * 8;
  u32x4 wr[2][3][3];                                          // the weight ring (rt_gemm_rows)
  CR_STAMP(0);

  // ---- prologue: the first piece's first two units, zero the slab (border positions stay zero to the end), scale / shift of all
  // source channels from the producers' sums (the head of k_gn_apply: fp64, a group may straddle the sources)
  rt_wload9(wr[0], wrow, 0);
  rt_wload9(wr[1], wrow, 1);
  for (int v = t; v < (CR_SLAB >> 4); v += CR_THREADS) *(uint4*)(sm + v * 16) = make_uint4(0, 0, 0, 0);
  {
    float* scale = (float*)(sm + CR_SCALE);
    float* shift = scale + CR_MAXC;
    const int cgp = C / a.G;
    for (int c = t; c < C; c += CR_THREADS) {
      const int g0 = (c / cgp) * cgp;
      double s = 0.0, q = 0.0;
      for (int j = g0; j < g0 + cgp; ++j) {
        const double* st = j < C1 ? a.st1 + ((size_t)b * C1 + j) * 2 : a.st2 + ((size_t)b * C2 + (j - C1)) * 2;
        s += st[0]; q += st[1];
      }
      const double n = (double)cgp * (double)HW;
      const double mean = s / n;
      const double var = fmax(q / n - mean * mean, 0.0);
      const float rstd = (float)(1.0 / sqrt(var + (double)a.eps));
      scale[c] = rstd * a.gamma[c];
      shift[c] = a.beta[c] - (float)mean * rstd * a.gamma[c];
    }
  }
  __syncthreads();
  CR_STAMP(1);

  // this lane's position of the wave's padded row 0 + its k quarter
  const int fb = (1 + 16 * hh + lj) * CR_RS + lq * 16 + rh * (NPT * CR_PITCH * CR_RS);
  f32x4 acc[3][NPT];
#pragma unroll
  for (int tt = 0; tt < 3; ++tt)
#pragma unroll
    for (int y = 0; y < NPT; ++y) acc[tt][y] = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};

  // ---- the 3x3 segment, piece by piece (the slab never holds more than 96 channels)
  int ub = 0;                                                 // the piece's first unit in the stream
  for (int s = 0; s < (C2 ? 2 : 1); ++s) {
    const int cs = s ? C2 : C1, coff = s ? C1 : 0;
    const unsigned short* src = (const unsigned short*)(s ? a.s2_bf16 : a.s1_bf16) + (size_t)b * HW * cs;
    for (int c0 = 0; c0 < cs; c0 += CR_PIECE) {
      const int pc = cs - c0 < CR_PIECE ? cs - c0 : CR_PIECE, nun = 3 * (pc >> 5);
      cr_fill<CR_THREADS, CR_FB * 4 / WAVES>(sm, src + c0, cs, pc, coff + c0, y0, H, W);
      __syncthreads();
      // (all the wave's row tiles whatever H: rows past the image read zeros and are never stored)
      if constexpr (WAVES == 8)                               // (a second fragment set does not fit 256 registers)
        rt_gemm_rows_1buf<CR_RS, CR_PITCH>(acc, wr, wrow + (size_t)ub * RT_UNIT, nun, sm, fb);
      else
        rt_gemm_rows<true, CR_RS, CR_PITCH>(acc, wr, wrow + (size_t)ub * RT_UNIT, nun, sm, fb, NPT);
      __syncthreads();                                        // every wave has read its last fragment of this piece
      ub += nun;
      if (ub < nu3) {                                         // the next piece's first two units travel behind its fill (a piece has >= 3)
        rt_wload9(wr[0], wrow + (size_t)ub * RT_UNIT, 0);
        rt_wload9(wr[1], wrow + (size_t)ub * RT_UNIT, 1);
      }
    }
  }
  CR_STAMP(2);

  // ---- the 1x1 segments on the raw sources
  if constexpr (SKIP) {
    const unsigned short* wsk = wrow + (size_t)nu3 * RT_UNIT;
    u32x4 ws[2][3];
    rt_wload3(ws[0], wsk, 0);
    if (nsk > 1) rt_wload3(ws[1], wsk, 1);
    const int cs_ = 16 * hh + rt_again(lj), xc = cs_ < 1 ? 0 : (cs_ > W ? W - 1 : cs_ - 1);
    cr_gemm_skip(acc, ws, wsk, nsk, (const unsigned short*)a.r1_bf16 + (size_t)b * HW * a.RC1,
                 (const unsigned short*)a.r2_bf16 + (size_t)b * HW * a.RC2, a.RC1, a.RC2, xc, lq, yw, H, W);
  }
  CR_STAMP(3);

  // ---- epilogue: acc + bias + time bias + residual in the accumulator layout, one rounding, into the [pixels][N] output image
  // (the slab is dead: every wave passed the barrier after the last piece); statistics on the fp32 value: fp32 over a lane's <= 14
  // rows, fp64 across the 16 lanes of a column half, the two halves meet in LDS.  Eight waves: the upper wave leaves its fp32
  // sums at CR_CARRY, the lower wave keeps its fp32 values (before the rounding) in acc and goes on from those sums after the barrier
  const int col = 16 * hh + rt_again(lj);
  const bool own = col >= 1 && col <= W;                       // this lane's column is a pixel
  const int x2 = own ? col - 1 : 0;
  const int nrows = H - y0 < CR_BAND ? H - y0 : CR_BAND;       // of the band
  const int nr = WAVES == 8 ? (nrows - NPT * rh < 0 ? 0 : (nrows - NPT * rh < NPT ? nrows - NPT * rh : NPT)) : nrows;   // of the wave
  double* red = (double*)(sm + CR_RED);
  float4* carry = (float4*)(sm + CR_CARRY) + (wv & 3) * (3 * 2 * 64) + lane;
  // the residual of all three channel tiles, requested at once (one round trip to memory, not three)
  uint2 rr[3][NPT] = {};
  const bool res = !SKIP && a.res_bf16;
  if (res) {
    const unsigned short* rp = (const unsigned short*)a.res_bf16 + (size_t)b * HW * CR_N + cg * 48 + lq * 4;
#pragma unroll
    for (int y = 0; y < NPT; ++y) {
      const unsigned short* rpy = rp + (size_t)(((y < nr ? yw + y : H - 1)) * W + x2) * CR_N;
#pragma unroll
      for (int tt = 0; tt < 3; ++tt) rr[tt][y] = *(const uint2*)(rpy + tt * 16);
    }
  }
#pragma unroll
  for (int tt = 0; tt < 3; ++tt) {
    const int n = cg * 48 + tt * 16 + lq * 4;
    const float4 bv = *(const float4*)(a.bias + n);
    const float4 tb = a.tbias ? *(const float4*)(a.tbias + (size_t)b * a.tb_stride + n) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const float add[4] = {bv.x + tb.x, bv.y + tb.y, bv.z + tb.z, bv.w + tb.w};
    const uint2 (&r)[NPT] = rr[tt];
    float s[4] = {0.0f, 0.0f, 0.0f, 0.0f}, q[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int y = 0; y < NPT; ++y) {
      if (y < nr && own) {
        const f32x4 v = acc[tt][y];
        float o[4] = {v[0] + add[0], v[1] + add[1], v[2] + add[2], v[3] + add[3]};
        if (res) {
          o[0] += __uint_as_float(r[y].x << 16); o[1] += __uint_as_float(r[y].x & 0xFFFF0000u);
          o[2] += __uint_as_float(r[y].y << 16); o[3] += __uint_as_float(r[y].y & 0xFFFF0000u);
        }
        if (WAVES == 8 && rh) {
          acc[tt][y] = (f32x4){o[0], o[1], o[2], o[3]};          // summed after the barrier, behind the upper wave's rows
        } else {
#pragma unroll
          for (int i = 0; i < 4; ++i) { s[i] += o[i]; q[i] = fmaf(o[i], o[i], q[i]); }
        }
        *(uint2*)(sm + ((NPT * rh + y) * W + x2) * CR_RS + n * 2) = make_uint2(rt_pack2(o[0], o[1]), rt_pack2(o[2], o[3]));
      }
    }
#ifndef CTDD_ROWS_STAMPS
    if (a.out_stats) {
      if constexpr (WAVES == 4) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          double ds = (double)s[i], dq = (double)q[i];
#pragma unroll
          for (int m = 1; m < 16; m <<= 1) { ds += __shfl_xor(ds, m, WAVE); dq += __shfl_xor(dq, m, WAVE); }
          if (lj == 0) { red[(hh * CR_N + n + i) * 2] = ds; red[(hh * CR_N + n + i) * 2 + 1] = dq; }
        }
      } else if (!rh) {
        carry[(tt * 2) * 64] = make_float4(s[0], s[1], s[2], s[3]);
        carry[(tt * 2 + 1) * 64] = make_float4(q[0], q[1], q[2], q[3]);
      }
    }
#endif
  }
  __syncthreads();
  CR_STAMP(4);
#ifndef CTDD_ROWS_STAMPS
  if (WAVES == 8 && rh && a.out_stats) {
#pragma unroll
    for (int tt = 0; tt < 3; ++tt) {
      const float4 cs_ = carry[(tt * 2) * 64], cq = carry[(tt * 2 + 1) * 64];
      float s[4] = {cs_.x, cs_.y, cs_.z, cs_.w}, q[4] = {cq.x, cq.y, cq.z, cq.w};
#pragma unroll
      for (int y = 0; y < NPT; ++y) {
        if (y < nr && own) {
#pragma unroll
          for (int i = 0; i < 4; ++i) { s[i] += acc[tt][y][i]; q[i] = fmaf(acc[tt][y][i], acc[tt][y][i], q[i]); }
        }
      }
      // the finished per-lane sums back into this wave's own slots (it is their only reader and has read them; the LDS
      // operations of one wave complete in order): the 16 lanes of a column half meet behind the next barrier
      carry[(tt * 2) * 64] = make_float4(s[0], s[1], s[2], s[3]);
      carry[(tt * 2 + 1) * 64] = make_float4(q[0], q[1], q[2], q[3]);
    }
  }
#endif
  {
    constexpr int npc = CR_N / 8;
    unsigned short* out = (unsigned short*)a.out_bf16 + ((size_t)b * HW + (size_t)y0 * W) * CR_N;   // the band's pixels are consecutive
    for (int v = t; v < nrows * W * npc; v += CR_THREADS) {
      const int p = v / npc, c0 = (v - p * npc) * 8;
      *(uint4*)(out + (size_t)p * CR_N + c0) = *(const uint4*)(sm + p * CR_RS + c0 * 2);
    }
#ifndef CTDD_ROWS_STAMPS
    // one fp64 atomic per (sample, channel, moment) and workgroup
    if constexpr (WAVES == 8) {
      // the lower waves' per-lane fp32 sums were written after the barrier above.  Thread (channel, moment) adds the 16 lanes of
      // either column half in fp64 in the tree of the 4-wave kernel's xor butterfly, ((v0 + v1) + (v2 + v3)) + ((v4 + v5) +
      // (v6 + v7)) and the same of v8 .. v15 on top, then half 0 + half 1: the same bits without its 96 fp64 shuffles per wave
      // (lanes whose column is no pixel hold 0.0 there as they did in the butterfly)
      __syncthreads();
      if (a.out_stats && t < 2 * CR_N) {
        const int n = t >> 1, ncg = n / 48, ntt = (n - ncg * 48) >> 4, nlq = (n >> 2) & 3;
        const float* tab = (const float*)(sm + CR_CARRY) + ((ncg * 2 * 3 + ntt) * 2 + (t & 1)) * 256 + nlq * 64 + (n & 3);
        double h[2];
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {
          double v[16];
#pragma unroll
          for (int j = 0; j < 16; ++j) v[j] = (double)tab[hf * (3 * 2 * 256) + j * 4];
#pragma unroll
          for (int m = 1; m < 16; m <<= 1)
#pragma unroll
            for (int j = 0; j < 16; j += 2 * m) v[j] += v[j + m];
          h[hf] = v[0];
        }
        atomicAdd(a.out_stats + (size_t)b * CR_N * 2 + t, h[0] + h[1]);
      }
    } else {
      if (a.out_stats && t < 2 * CR_N) atomicAdd(a.out_stats + (size_t)b * CR_N * 2 + t, red[t] + red[2 * CR_N + t]);
    }
#endif
  }
  CR_STAMP(5);
}

}  // namespace
}  // namespace ctdd

using namespace ctdd;

// Refuses (non-zero, ctdd_last_error set, nothing launched) what the kernel does not take: fp32 mode, W > 28 (the slab's pitch of
// 32 positions), N != 96, channel counts that are not multiples of 32 or exceed 384 in all, groups that do not divide the
// channels, a GroupNorm source without statistics, 1x1 segments together with a residual, tensors that are not 16-byte aligned.
template <int WAVES>
static int launch_conv_rows(const void* args_, int f32, void* stream) {
  CTDD_REQUIRE(args_, CTDD_EINVAL, "ctdd_unet_conv_rows: null arguments");
  const ctdd_conv_rows_args& a = *(const ctdd_conv_rows_args*)args_;
  CTDD_REQUIRE(f32 == 0, CTDD_ERANGE, "ctdd_unet_conv_rows: bf16 inference only (the fp32 mode keeps GroupNorm and convolution apart)");
  CTDD_REQUIRE(a.B > 0 && a.H > 0 && a.W >= 1 && a.W <= CR_MAXW, CTDD_ERANGE,
               "ctdd_unet_conv_rows: a grid of %dx%d pixels does not fit the row tiles (1 <= W <= 28)", a.H, a.W);
  const int nbands = (a.H + CR_BAND - 1) / CR_BAND;
  CTDD_REQUIRE((int64_t)a.B * nbands < ((int64_t)1 << 31) && (int64_t)a.H * a.W * CR_MAXC < ((int64_t)1 << 30), CTDD_ERANGE,
               "ctdd_unet_conv_rows: B=%d, %dx%d is over the 32-bit index range of the kernel", a.B, a.H, a.W);
  const int C = a.C1 + a.C2;
  CTDD_REQUIRE(a.N == CR_N && a.C1 > 0 && a.C1 % 32 == 0 && a.C2 >= 0 && a.C2 % 32 == 0 && C <= CR_MAXC && a.RC1 >= 0 && a.RC1 % 32 == 0 &&
                   a.RC2 >= 0 && a.RC2 % 32 == 0 && (a.RC2 == 0 || a.RC1 > 0) && a.RC1 + a.RC2 <= CR_MAXC, CTDD_ERANGE,
               "ctdd_unet_conv_rows: channel counts off the tile (N=%d, C1=%d, C2=%d, RC1=%d, RC2=%d; N = 96, sources in multiples of 32, <= 384 in all)",
               a.N, a.C1, a.C2, a.RC1, a.RC2);
  CTDD_REQUIRE(a.G > 0 && C % a.G == 0, CTDD_EINVAL, "ctdd_unet_conv_rows: %d groups do not divide %d channels", a.G, C);
  CTDD_REQUIRE(a.s1_bf16 && (a.C2 == 0 || a.s2_bf16) && (a.RC1 == 0 || a.r1_bf16) && (a.RC2 == 0 || a.r2_bf16) && a.gamma && a.beta && a.w &&
                   a.bias && a.out_bf16, CTDD_EINVAL, "ctdd_unet_conv_rows: null pointer");
  CTDD_REQUIRE(a.st1 && (a.C2 == 0 || a.st2), CTDD_EINVAL, "ctdd_unet_conv_rows: a GroupNorm source without statistics");
  auto al16 = [](const void* p) { return ((uintptr_t)p & 15) == 0; };
  CTDD_REQUIRE(al16(a.s1_bf16) && al16(a.s2_bf16) && al16(a.r1_bf16) && al16(a.r2_bf16) && al16(a.res_bf16) && al16(a.w) && al16(a.out_bf16) &&
                   al16(a.bias) && al16(a.tbias) && a.tb_stride % 4 == 0, CTDD_EINVAL, "ctdd_unet_conv_rows: tensors must be 16-byte aligned");
  CTDD_REQUIRE(!(a.RC1 > 0 && a.res_bf16), CTDD_EINVAL, "ctdd_unet_conv_rows: 1x1 segments and a residual in one call");
  static bool attr_done[2][16] = {};
  if (a.RC1 > 0) {
    ensure_lds_ceiling((const void*)k_conv_rows<true, WAVES>, attr_done[1]);
    hipLaunchKernelGGL((k_conv_rows<true, WAVES>), dim3(a.B * nbands), dim3(WAVES * 64), (size_t)CR_TOTAL, (hipStream_t)stream, a);
  } else {
    ensure_lds_ceiling((const void*)k_conv_rows<false, WAVES>, attr_done[0]);
    hipLaunchKernelGGL((k_conv_rows<false, WAVES>), dim3(a.B * nbands), dim3(WAVES * 64), (size_t)CR_TOTAL, (hipStream_t)stream, a);
  }
  return finish_launch("k_conv_rows");
}

// eight waves per workgroup
extern "C" int ctdd_unet_conv_rows(const void* args_, int f32, void* stream) { return launch_conv_rows<8>(args_, f32, stream); }
// the same launch on four waves, each owning the band's 14 rows: bit-identical results
extern "C" int ctdd_unet_conv_rows_w4(const void* args_, int f32, void* stream) { return launch_conv_rows<4>(args_, f32, stream); }
