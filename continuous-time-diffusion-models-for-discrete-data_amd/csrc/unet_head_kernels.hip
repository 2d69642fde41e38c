// unet_head_kernels.hip -- the output head of a level whose samples do not fit one workgroup (28x28, N = S = 256): GroupNorm + Swish
// + 3x3 convolution into N output channels as ONE launch on the row-tile K loop (row_tile.hpp), the slab of k_conv_rows
// (unet_rows_kernels.hip) filled ONCE and read by ceil(N / 96) output-channel passes.
//
//   out[b][y][x][0..N) = bf16( conv3x3( bf16(swish(GN(s1))) ) + bias )
//
// replaces a k_gn_apply + k_conv_ring pair: the activated tensor is never written to memory, and the slab a ring workgroup
// re-stages for each of its 64 output columns is staged once per (sample, band).  The rounding points are those of the pair: the
// activated operand is rounded to bf16, accumulation is fp32 on the matrix cores, acc + bias is rounded once.  No output
// statistics, time bias, residual or 1x1 segments: nothing follows the head.
//
// Work split, slab and fill are k_conv_rows': one workgroup per (sample, band of 14 output rows), of eight waves
// (ctdd_unet_conv_rows_head) or four (ctdd_unet_conv_rows_head_w4), wave ([rh,] cg, h) owns 48 channels x column half h [x rows
// 7 rh .. 7 rh + 6 of the band] of the current pass, 32 positions per padded row at 224 bytes (115 136 bytes), scale / shift from the
// producer's fp64 sums in the prologue.  Pass p computes output channels [96 p, 96 p + 96) from weight streams 2 p and 2 p + 1
// (ctdd_unet.h: the [N][9 C1] matrix zero-padded to 96 passes rows; channels >= N are computed and never stored).  After the
// fill's barrier no wave waits for another: the slab is only read, and the epilogue stages in wave-PRIVATE LDS beside the slab
// (seven output rows x 16 pixels x 48 channels, twice per pass; eight waves: three rows, as 3 + 3 + 1) so that the same wave writes its 96 bytes per pixel out in 16-byte
// buffer stores (the band's output as a buffer of its own: a lane with nothing to store carries an offset past it, no branches).  The next pass's first two weight units are requested before the epilogue and travel under it.
#include "row_tile.hpp"
#include "../../include/ctdd_unet.h"

namespace ctdd {
namespace {

constexpr int HD_TILE = 96, HD_BAND = 14, HD_PITCH = 32, HD_RS = 224, HD_MAXW = 28, HD_MAXC = 96, HD_MAXN = 576;
constexpr int HD_SLAB = ((HD_BAND + 2) * HD_PITCH + 2) * HD_RS;  // 115 136
constexpr int HD_SCALE = HD_SLAB;                                // float scale[HD_MAXC], shift[HD_MAXC]
constexpr int HD_STAGE = HD_SCALE + 2 * HD_MAXC * 4;             // per wave: [srows][16 pixels][48 channels] bf16
// rows of a wave's staging image: four waves stage their 14 rows as 7 + 7 (4 x 10 752 bytes), eight their 7 rows as 3 + 3 + 1
// (8 x 4 608 bytes: 5 992 per wave are left beside the slab)
constexpr int hd_srows(int waves) { return waves == 8 ? 3 : HD_BAND / 2; }
constexpr int hd_total(int waves) { return HD_STAGE + waves * hd_srows(waves) * 16 * 96; }   // 158 912 | 152 768
constexpr unsigned HD_OOB = 0x80000000u;                         // a byte offset no band reaches: the buffer store drops the lane
constexpr int HD_FB = 12;                                        // pixels per thread in flight in the fill (half of them with eight waves)
static_assert(hd_total(4) <= 160 * 1024 && hd_total(8) <= 160 * 1024 && HD_STAGE % 16 == 0 && HD_BAND % 2 == 0,
              "slab + scale / shift + staging within the CU's LDS");

// cr_fill of unet_rows_kernels.hip for the head's single source (row_tile.hpp: why it is a copy): bf16(swish(x * scale + shift))
// of `pc` channels from `src` (the sample's first pixel, pixel stride `cs` channels) into columns [0, pc) of the slab: padded rows
// rlo .. rhi of the band (image rows y0 - 1 + r), which are consecutive pixels in memory.  No barrier of its own.  What keeps the two
// copies from drifting apart: tests/test_gpu_conv_rows_head.py::test_head_n96_is_conv_rows_bit_for_bit (N = 96 against
// ctdd_unet_conv_rows, bit for bit) -- a change to either fill's arithmetic goes into both.
template <int THREADS, int FB>
__device__ __attribute__((always_inline)) inline void hd_fill(unsigned char* sm, const unsigned short* __restrict__ src, int cs, int pc, int coff,
                                                             int y0, int H, int W) {
  const int t = threadIdx.x, noct = pc >> 3, npl = THREADS / noct;
  if (t >= noct * npl) return;
  const int oct = t % noct, pl = t / noct;
  const float* scale = (const float*)(sm + HD_SCALE) + coff + oct * 8;
  const float* shift = scale + HD_MAXC;
  const float4 sc0 = *(const float4*)scale, sc1 = *(const float4*)(scale + 4);
  const float4 sh0 = *(const float4*)shift, sh1 = *(const float4*)(shift + 4);
  const f32x2v scv[4] = {{sc0.x, sc0.y}, {sc0.z, sc0.w}, {sc1.x, sc1.y}, {sc1.z, sc1.w}};
  const f32x2v shv[4] = {{sh0.x, sh0.y}, {sh0.z, sh0.w}, {sh1.x, sh1.y}, {sh1.z, sh1.w}};
  const int rlo = y0 == 0 ? 1 : 0, rhi = H - y0 < HD_BAND + 1 ? H - y0 : HD_BAND + 1;
  const unsigned npix = (unsigned)((rhi - rlo + 1) * W), uW = (unsigned)W;
  const unsigned short* sp = src + (size_t)((y0 - 1 + rlo) * W) * cs + oct * 8;
  unsigned char* dst = sm + (1 + rlo * HD_PITCH + 1) * HD_RS + oct * 16;
  // FB pixels per thread in flight; the loads are unconditional on a clamped pixel, only the LDS stores are predicated
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
      for (int j = 0; j < 4; ++j) {                              // as k_gn_apply / cr_fill: packed fma, hardware exp2 / rcp
        const f32x2v x = {__uint_as_float(u[k][j] << 16), __uint_as_float(u[k][j] & 0xFFFF0000u)};
        f32x2v y = __builtin_elementwise_fma(x, scv[j], shv[j]);
        const f32x2v z = y * (f32x2v){-1.4426950408889634f, -1.4426950408889634f};
        const f32x2v d = (f32x2v){__builtin_amdgcn_exp2f(z.x), __builtin_amdgcn_exp2f(z.y)} + (f32x2v){1.0f, 1.0f};
        y = y * (f32x2v){__builtin_amdgcn_rcpf(d.x), __builtin_amdgcn_rcpf(d.y)};
        ow[j] = rt_pack2(y.x, y.y);
      }
      const unsigned rr = p / uW, x = p - rr * uW;
      if (p < npix) *(uint4*)(dst + (rr * HD_PITCH + x) * HD_RS) = make_uint4(ow[0], ow[1], ow[2], ow[3]);
    }
  }
}

#ifdef CTDD_ROWS_STAMPS
// phase stamps (tools/build_conv_stamps.sh, tools/stamp_conv_rows.py): thread 0 of every workgroup leaves s_memtime at the phase
// boundaries in a [workgroups][16] buffer passed in place of out_stats: 0 entry, 1 prologue, 2 fill, then per pass its K loop and
// its epilogue / store
#define HD_STAMP(i_)                                                                                      \
  do {                                                                                                    \
    unsigned long long t_;                                                                                \
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");                            \
    if (threadIdx.x == 0) ((unsigned long long*)a.out_stats)[(size_t)blockIdx.x * 16 + (i_)] = t_;        \
  } while (0)
#else
#define HD_STAMP(i_)
#endif

// WAVES: 4 -- wave (cg, hh) owns the band's 14 rows, one wave per SIMD; 8 -- wave (rh, cg, hh) owns rows [7 rh, 7 rh + 7) of the band
// with 84 accumulator registers and one fragment set (rt_gemm_rows_1buf), two waves per SIMD: waves wv and wv + 4 share a SIMD and
// a weight stream, and 512 threads carry the zero fill and the fill.  Per output pixel the order of units, dy and tiles is the
// same, so both give the same bits (k_conv_rows has the same two splits).
template <int WAVES>
__global__ __launch_bounds__(WAVES * 64, 1) void k_conv_rows_head(const ctdd_conv_rows_args a) {
  static_assert(WAVES == 4 || WAVES == 8, "one or two row halves");
  constexpr int HD_THREADS = WAVES * 64, NPT = HD_BAND * 4 / WAVES;   // rows of a wave
  constexpr int HD_SROWS = hd_srows(WAVES), HD_WSTAGE = HD_SROWS * 16 * 96;
  extern __shared__ __attribute__((aligned(16))) unsigned char sm[];
  const int t = threadIdx.x;
  const int H = a.H, W = a.W, HW = H * W, C1 = a.C1, N = a.N;
  const int nbands = (H + HD_BAND - 1) / HD_BAND;
  const int b = blockIdx.x / nbands, y0 = (blockIdx.x - b * nbands) * HD_BAND;
  // (the wave's index as a scalar: what derives from it stays out of the vector registers, which the K loop fills)
  const int wv = __builtin_amdgcn_readfirstlane(t >> 6), cg = WAVES == 8 ? (wv >> 1) & 1 : wv >> 1, hh = wv & 1;
  const int rh = WAVES == 8 ? wv >> 2 : 0;                     // the wave's row half
  const int nu3 = 3 * (C1 >> 5), npass = (N + HD_TILE - 1) / HD_TILE;
  const size_t wstream = (size_t)nu3 * RT_UNIT;                // bf16 elements of one 48-channel stream
  const unsigned short* wcg = (const unsigned short*)a.w + (size_t)cg * wstream;
  const unsigned short* wrow = wcg + (t & 63) * 8;
  u32x4 wr[2][3][3];                                          // the weight ring (rt_gemm_rows)
  HD_STAMP(0);

  // ---- prologue: pass 0's first two units, zero the slab (border positions stay zero to the end), scale / shift from the
  // producer's sums (the head of k_gn_apply: fp64)
  rt_wload9(wr[0], wrow, 0);
  rt_wload9(wr[1], wrow, 1);
  for (int v = t; v < (HD_SLAB >> 4); v += HD_THREADS) *(uint4*)(sm + v * 16) = make_uint4(0, 0, 0, 0);
  {
    float* scale = (float*)(sm + HD_SCALE);
    float* shift = scale + HD_MAXC;
    const int cgp = C1 / a.G;
    for (int c = t; c < C1; c += HD_THREADS) {
      const int g0 = (c / cgp) * cgp;
      double s = 0.0, q = 0.0;
      for (int j = g0; j < g0 + cgp; ++j) {
        const double* st = a.st1 + ((size_t)b * C1 + j) * 2;
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
  HD_STAMP(1);

  // ---- the fill, once: every pass reads this slab, nothing writes it again
  hd_fill<HD_THREADS, HD_FB * 4 / WAVES>(sm, (const unsigned short*)a.s1_bf16 + (size_t)b * HW * C1, C1, C1, 0, y0, H, W);
  __syncthreads();
  HD_STAMP(2);

  const int nrows = H - y0 < HD_BAND ? H - y0 : HD_BAND;
  unsigned char* stg = sm + HD_STAGE + wv * HD_WSTAGE;         // this wave's staging rows
  // the band's pixels are consecutive: its nrows W N elements (at most 14 x 28 x 576) as a buffer of their own
  unsigned short* outb = (unsigned short*)a.out_bf16 + ((size_t)b * HW + (size_t)y0 * W) * N;
  const __amdgpu_buffer_rsrc_t orsrc = __builtin_amdgcn_make_buffer_rsrc((void*)outb, 0, nrows * W * N * 2, 0x00020000);

  // (every per-lane value of a pass is derived again from the thread index where it is used, rt_again: the K loop and the epilogue
  //  are one loop body, and what either keeps in registers across the other costs the K loop its allocation)
  for (int p = 0; p < npass; ++p) {
    const int lk = rt_again(t) & 63;
    // this lane's position of the wave's padded row 0 + its k quarter
    const int fb = (1 + 16 * hh + (lk & 15)) * HD_RS + (lk >> 4) * 16 + (WAVES == 8 ? rh * (NPT * HD_PITCH * HD_RS) : 0);
    const unsigned short* wrow = wcg + lk * 8;
    f32x4 acc[3][NPT];
#pragma unroll
    for (int tt = 0; tt < 3; ++tt)
#pragma unroll
      for (int y = 0; y < NPT; ++y) acc[tt][y] = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
    // (all the wave's row tiles whatever H: rows past the image read zeros and are never stored)
    if constexpr (WAVES == 8) {
      // (84 accumulators, the ring and one fragment set share the 256 registers of a wave with a partner on its SIMD: no pinning)
      rt_gemm_rows_1buf<HD_RS, HD_PITCH>(acc, wr, wrow + (size_t)(2 * p) * wstream, nu3, sm, fb);
    } else {
      // (the accumulators pinned to accumulation registers at either end of the K loop: with the epilogue's vector arithmetic on
      //  them in the same loop body the allocator otherwise keeps a part of them in vector registers and the unit loop carries
      //  268 register moves per two units: 27 k cycles per pass instead of 24 k)
#pragma unroll
      for (int tt = 0; tt < 3; ++tt)
#pragma unroll
        for (int y = 0; y < NPT; ++y) asm volatile("" : "+a"(acc[tt][y]));
      rt_gemm_rows<true, HD_RS, HD_PITCH>(acc, wr, wrow + (size_t)(2 * p) * wstream, nu3, sm, fb, NPT);
#pragma unroll
      for (int tt = 0; tt < 3; ++tt)
#pragma unroll
        for (int y = 0; y < NPT; ++y) asm volatile("" : "+a"(acc[tt][y]));
    }
    if (p + 1 < npass) {                                       // the next pass's first two units travel under this epilogue
      rt_wload9(wr[0], wrow + (size_t)(2 * p + 2) * wstream, 0);
      rt_wload9(wr[1], wrow + (size_t)(2 * p + 2) * wstream, 1);
    }
    HD_STAMP(3 + 2 * p);

    // ---- epilogue: acc + bias in the accumulator layout, one rounding, into this wave's [row][pixel][48 channels] staging
    // image, seven output rows at a time; the same wave then writes each pixel's 96 bytes out in 16-byte buffer stores (LDS
    // operations of one wave complete in order: no barrier, the wave_barrier only keeps the compiler from moving them)
    const int n0 = p * HD_TILE + cg * 48;                      // this wave's first output channel of the pass
    const int lane = rt_again(t) & 63, lj = lane & 15, lq = lane >> 4;
    // (the band's rows and width as per-pass vector values as well: as scalars their fourteen row tests and row offsets are
    //  hoisted out of the pass loop into scalar registers, which then spill to lanes)
    const int nre = rt_again(nrows), We = rt_again(W);
    float add[3][4];
#pragma unroll
    for (int tt = 0; tt < 3; ++tt) {
      const int n = n0 + tt * 16 + lq * 4;
      const float4 bv = n < N ? *(const float4*)(a.bias + n) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      add[tt][0] = bv.x; add[tt][1] = bv.y; add[tt][2] = bv.z; add[tt][3] = bv.w;
    }
    // (the wave's rows leave HD_SROWS at a time: 7 + 7 of four waves' 14, 3 + 3 + 1 of eight waves' 7)
#pragma unroll
    for (int half = 0; half < (NPT + HD_SROWS - 1) / HD_SROWS; ++half) {
      const int nsr = NPT - half * HD_SROWS < HD_SROWS ? NPT - half * HD_SROWS : HD_SROWS;   // (a constant once unrolled)
#pragma unroll
      for (int r = 0; r < HD_SROWS; ++r)
#pragma unroll
        for (int tt = 0; tt < 3; ++tt) {
          if (r < nsr) {
            const f32x4 v = acc[tt][half * HD_SROWS + r];
            *(uint2*)(stg + (r * 16 + lj) * 96 + tt * 32 + lq * 8) =
                make_uint2(rt_pack2(v[0] + add[tt][0], v[1] + add[tt][1]), rt_pack2(v[2] + add[tt][2], v[3] + add[tt][3]));
          }
        }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      // 16-byte piece v of the staging image: row v / 96, pixel (v / 6) % 16, channels [8 (v % 6), + 8) of the wave's 48; all
      // the wave's reads are requested before the first store waits for one
      constexpr int NKMAX = (HD_SROWS * 16 * 6 + 63) / 64;
      const int NV = nsr * 16 * 6, NK = (NV + 63) / 64;
      uint4 o[NKMAX];
#pragma unroll
      for (int k = 0; k < NKMAX; ++k)
        if (k < NK) o[k] = *(const uint4*)(stg + (lane + 64 * k < NV ? lane + 64 * k : NV - 1) * 16);
#pragma unroll
      for (int k = 0; k < NKMAX; ++k) {
        if (k >= NK) continue;
        const int v = lane + 64 * k, pi = v / 6, c8 = (v - pi * 6) * 8, y = NPT * rh + half * HD_SROWS + (pi >> 4), col = 16 * hh + (pi & 15);
        const bool ok = v < NV && y < nre && col >= 1 && col <= We && n0 + c8 < N;
        // (no branch per store: a lane with nothing to store carries an offset past the band, which the buffer store drops; eleven
        //  predicated stores cost 91 scalar registers spilled to lanes for their masks)
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, o[k]), orsrc, ok ? (unsigned)(((y * We + col - 1) * N + n0 + c8) * 2) : HD_OOB, 0, 0);
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      __builtin_amdgcn_wave_barrier();
    }
    HD_STAMP(4 + 2 * p);
  }
}

}  // namespace
}  // namespace ctdd

using namespace ctdd;

// Refuses (non-zero, ctdd_last_error set, nothing launched) what the kernel does not take: fp32 mode, W > 28 (the slab's pitch of
// 32 positions), a source that is not 32, 64 or 96 channels or comes without statistics, a second source, 1x1 segments, a
// residual, a time bias, output statistics, N off 32 .. 576 in multiples of 32, groups that do not divide the channels, tensors
// that are not 16-byte aligned.
template <int WAVES>
static int launch_conv_rows_head(const void* args_, int f32, void* stream) {
  CTDD_REQUIRE(args_, CTDD_EINVAL, "ctdd_unet_conv_rows_head: null arguments");
  const ctdd_conv_rows_args& a = *(const ctdd_conv_rows_args*)args_;
  CTDD_REQUIRE(f32 == 0, CTDD_ERANGE, "ctdd_unet_conv_rows_head: bf16 inference only (the fp32 mode keeps GroupNorm and convolution apart)");
  CTDD_REQUIRE(a.B > 0 && a.H > 0 && a.W >= 1 && a.W <= HD_MAXW, CTDD_ERANGE,
               "ctdd_unet_conv_rows_head: a grid of %dx%d pixels does not fit the row tiles (1 <= W <= 28)", a.H, a.W);
  const int nbands = (a.H + HD_BAND - 1) / HD_BAND;
  CTDD_REQUIRE((int64_t)a.B * nbands < ((int64_t)1 << 31) && (int64_t)a.H * a.W * HD_MAXN < ((int64_t)1 << 30), CTDD_ERANGE,
               "ctdd_unet_conv_rows_head: B=%d, %dx%d is over the 32-bit index range of the kernel", a.B, a.H, a.W);
  CTDD_REQUIRE((a.C1 == 32 || a.C1 == 64 || a.C1 == 96) && a.C2 == 0 && a.RC1 == 0 && a.RC2 == 0 && a.N >= 32 && a.N <= HD_MAXN && a.N % 32 == 0,
               CTDD_ERANGE,
               "ctdd_unet_conv_rows_head: channel counts off the tile (N=%d, C1=%d, C2=%d, RC1=%d, RC2=%d; one source of 32, 64 or 96 channels, "
               "N in multiples of 32 from 32 to 576)", a.N, a.C1, a.C2, a.RC1, a.RC2);
  CTDD_REQUIRE(a.G > 0 && a.C1 % a.G == 0, CTDD_EINVAL, "ctdd_unet_conv_rows_head: %d groups do not divide %d channels", a.G, a.C1);
  CTDD_REQUIRE(a.s1_bf16 && a.gamma && a.beta && a.w && a.bias && a.out_bf16, CTDD_EINVAL, "ctdd_unet_conv_rows_head: null pointer");
  CTDD_REQUIRE(a.st1, CTDD_EINVAL, "ctdd_unet_conv_rows_head: a GroupNorm source without statistics");
#ifdef CTDD_ROWS_STAMPS
  const bool no_stats = true;                                  // (out_stats carries the stamp buffer in this build)
#else
  const bool no_stats = !a.out_stats;
#endif
  CTDD_REQUIRE(!a.res_bf16 && !a.tbias && no_stats, CTDD_EINVAL,
               "ctdd_unet_conv_rows_head: the head takes no residual, time bias or output statistics");
  auto al16 = [](const void* p) { return ((uintptr_t)p & 15) == 0; };
  CTDD_REQUIRE(al16(a.s1_bf16) && al16(a.w) && al16(a.out_bf16) && al16(a.bias), CTDD_EINVAL,
               "ctdd_unet_conv_rows_head: tensors must be 16-byte aligned");
  static bool attr_done[16] = {};
  ensure_lds_ceiling((const void*)k_conv_rows_head<WAVES>, attr_done);
  hipLaunchKernelGGL((k_conv_rows_head<WAVES>), dim3(a.B * nbands), dim3(WAVES * 64), (size_t)hd_total(WAVES), (hipStream_t)stream, a);
  return finish_launch("k_conv_rows_head");
}

// eight waves per workgroup
extern "C" int ctdd_unet_conv_rows_head(const void* args_, int f32, void* stream) { return launch_conv_rows_head<8>(args_, f32, stream); }
// the same launch on four waves, each owning the band's 14 rows: bit-identical results
extern "C" int ctdd_unet_conv_rows_head_w4(const void* args_, int f32, void* stream) { return launch_conv_rows_head<4>(args_, f32, stream); }
