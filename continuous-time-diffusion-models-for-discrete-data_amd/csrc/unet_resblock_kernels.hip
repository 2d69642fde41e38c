// unet_resblock_kernels.hip -- a whole ResBlock of a small-resolution U-Net level in ONE launch (bf16 inference).
//
// At a fixed resolution a ResBlock (reference lib/networks/unet.py:100-140) is sample-local: the 3x3 convolutions never read
// across samples, GroupNorm statistics are per (sample, group), the time bias is per (sample, channel), the residual / 1x1
// skip is per pixel.  A workgroup that owns ONE whole sample (H*W <= 64 pixels) and ALL N = 192 output channels runs
//   GN1 + Swish -> conv1 + bias + time bias -> GN2 + Swish -> conv2 (+ 1x1 skip segments on the raw input | + residual)
// with nobody else involved: one launch instead of four, h1 and both activated tensors never leave LDS, every element is
// normalised once, the statistics are a reduction inside the workgroup.  The rounding points are those of the four launches
// it replaces (k_gn_onepass, k_conv_patch): a1, h1 (before GN2's statistics), a2 and the output are rounded to bf16, sums
// are fp32 per thread / fp64 across threads, accumulation is fp32 on the matrix cores.
//
// Matrix mapping (v_mfma_f32_16x16x32_bf16, weights as the A operand, pixels as the B operand, so that a lane's four result
// registers are four CONSECUTIVE channels of one pixel = one 8-byte bf16 store): wave w of four owns output channels
// [48 w, 48 w + 48) (three 16-row weight tiles) x all pixel tiles (NPT = 4 tiles of 16 consecutive slab rows, 5 for 8x8, one
// tile of flattened pixels for H*W <= 16: rb_tile_pixel).  No two waves
// read the same weight element, so the weights are streamed global -> registers by the wave that uses them, from a copy of
// the [N][K] matrix packed in fragment order (every wave-instruction reads 1 KiB of consecutive bytes), PD chunks ahead; there is no
// weight image in LDS, no ring and no barrier inside a K loop.  The pixel operand is read from a zero-bordered LDS slab in
// which the nine taps are row offsets: per 64-channel chunk and wave 2 NPT ds_read_b128 and 6 global_load_dwordx4 feed
// 6 NPT matrix instructions.
//
// LDS: raw input [HW][C] (kept for the skip segments / the residual), slab [(H+2)(W+2)][C] for a1, reused as the
// [(H+2)(W+2)][N] slab of h1 / a2 and as the output image; rows are padded by 32 bytes (row stride 2 C + 32 = 8 mod 16
// dwords).  A ds_read_b128 is served in four groups of 16 lanes that are NOT the four quarter waves ({0-3, 12-15, 20-27}, ...:
// two k quarters of eight rows each), so a row padding of 16 bytes, which this file had and called conflict-free, put the two
// k quarters of a group on the same banks, and the flattened 16-pixel tiles it used jump two slab rows where a grid row wraps:
// 12 LDS cycles per fragment read instead of 4 (tools/lds_bank_model.py; SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE 0.54 for
// this kernel, 0.63 for k_resblock_mid).  With 32 bytes and tiles of 16 consecutive slab rows every tap of every tile is 4
// cycles under that model (measured ratios 0.21 / 0.31, what is left being the GroupNorm passes and the epilogues' 8-byte stores).
// 7x7, C = 384: 38 + 63 + 29 (reduction scratch) = 130 KB.
#include "row_tile.hpp"
#include "../../include/ctdd_unet.h"

namespace ctdd {
namespace {

constexpr int RB_THREADS = 256, RB_N = 192, RB_PST = 20, RB_MAXC = 384;

struct RbLds {                       // byte offsets into the dynamic LDS block
  int raw, slab, part, red, scale, total;
  int rsA, rs2, prows;               // row strides (bytes) of the C- and N-channel images, rows of the padded grid
};
__host__ __device__ inline RbLds rb_layout(int H, int W, int C) {
  RbLds L;
  L.rsA = C * 2 + 32;
  L.rs2 = RB_N * 2 + 32;
  L.prows = (H + 2) * (W + 2);
  const int slabA = L.prows * L.rsA, slab2 = L.prows * L.rs2;
  L.raw = 0;
  L.slab = H * W * L.rsA;
  L.part = L.slab + (slabA > slab2 ? slabA : slab2);
  L.red = L.part + RB_THREADS * RB_PST * 4;
  L.scale = L.red + 2 * RB_MAXC * 8;
  L.total = L.scale + 2 * RB_MAXC * 4;
  return L;
}

// slab row of pixel p of an H x W sample on a zero-bordered grid of `pitch` positions per row (W + 2, or 16 in k_resblock_mid)
__device__ inline int rb_prow(int p, int W, int pitch) {
  const int y = p / W;
  return (y + 1) * pitch + (p - y * W) + 1;
}
// Pixel tiles of the K loops (NPT > 1): tile pt = the 16 CONSECUTIVE slab rows from Wp + 1 + 16 pt (Wp + 1: the first interior
// row), so that lane j reads row Wp + 1 + 16 pt + j + (dy Wp + dx) for tap (dy, dx): 16 consecutive rows at a stride of
// 2 C + 32 bytes (8 mod 16 dwords) whatever the tap, conflict-free under the lane groups of ds_read_b128
// (tools/lds_bank_model.py).  Lanes on border positions (and rows past the grid) compute a value that is never stored; their
// row is clamped to the interior range [Wp + 1, prows - Wp - 2], which keeps every tap of every lane inside the slab.
struct RbPix { int row, p; bool ok; };
__device__ inline RbPix rb_tile_pixel(int pt, int lj, int H, int W) {
  const int Wp = W + 2, r = Wp + 1 + pt * 16 + lj, last = H * Wp + W;
  const int yy = r / Wp, xx = r - yy * Wp;
  RbPix q;
  q.ok = r <= last && xx >= 1 && xx <= W;
  q.row = r < last ? r : last;
  q.p = q.ok ? (yy - 1) * W + xx - 1 : 0;
  return q;
}

// GroupNorm + Swish of an [HW][C] bf16 image in LDS (`src`, rows p or padded rows): statistics as k_gn_onepass takes them
// (fp32 per thread over its pixels, fp64 across threads and group members), then bf16(swish(x * scale + shift)) into the padded
// rows of `dst` (which may be `src` itself: every element is read and written by the same thread).  Ends with a barrier.
__device__ __attribute__((always_inline)) inline void rb_groupnorm(unsigned char* sm, const RbLds& L, int src, int src_rs, bool src_padded, int dst, int dst_rs,
                                                      int HW, int W, int pitch, int C, int G, const float* __restrict__ gamma,
                                                      const float* __restrict__ beta, float eps) {
  const int t = threadIdx.x, noct = C >> 3;
  const int npl = RB_THREADS / noct < HW ? RB_THREADS / noct : HW, T = noct * npl;
  const bool act = t < T;
  const int oct = act ? t % noct : 0, pl = act ? t / noct : 0;
  float* part = (float*)(sm + L.part);
  double* red = (double*)(sm + L.red);
  float* scale = (float*)(sm + L.scale);
  float* shift = scale + RB_MAXC;
  float sx[8], sq[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) { sx[j] = 0.0f; sq[j] = 0.0f; }
  if (act) {
    for (int p = pl; p < HW; p += npl) {
      const int row = src_padded ? rb_prow(p, W, pitch) : p;
      const uint4 u = *(const uint4*)(sm + src + row * src_rs + oct * 16);
      const unsigned w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float x0 = __uint_as_float(w[j] << 16), x1 = __uint_as_float(w[j] & 0xFFFF0000u);
        sx[2 * j] += x0; sq[2 * j] = fmaf(x0, x0, sq[2 * j]);
        sx[2 * j + 1] += x1; sq[2 * j + 1] = fmaf(x1, x1, sq[2 * j + 1]);
      }
    }
    float4* pt = (float4*)(part + t * RB_PST);
    pt[0] = make_float4(sx[0], sx[1], sx[2], sx[3]); pt[1] = make_float4(sx[4], sx[5], sx[6], sx[7]);
    pt[2] = make_float4(sq[0], sq[1], sq[2], sq[3]); pt[3] = make_float4(sq[4], sq[5], sq[6], sq[7]);
  }
  __syncthreads();
  for (int r = t; r < 2 * C; r += RB_THREADS) {                 // (moment m, channel c): over the pixel lanes, in fp64
    const int m = r >= C ? 1 : 0, c = r - m * C;
    const float* pp = part + (c >> 3) * RB_PST + m * 8 + (c & 7);
    double acc = 0.0;
    for (int q = 0; q < npl; ++q) acc += (double)pp[q * noct * RB_PST];
    red[r] = acc;
  }
  __syncthreads();
  const int cg = C / G;
  for (int c = t; c < C; c += RB_THREADS) {
    const int g0 = (c / cg) * cg;
    double s = 0.0, q = 0.0;
    for (int j = g0; j < g0 + cg; ++j) { s += red[j]; q += red[C + j]; }
    const double n = (double)cg * (double)HW;
    const double mean = s / n;
    const double var = fmax(q / n - mean * mean, 0.0);
    const float rstd = (float)(1.0 / sqrt(var + (double)eps));
    scale[c] = rstd * gamma[c];
    shift[c] = beta[c] - (float)mean * rstd * gamma[c];
  }
  __syncthreads();
  if (act) {
    const float4 sc0 = *(const float4*)(scale + oct * 8), sc1 = *(const float4*)(scale + oct * 8 + 4);
    const float4 sh0 = *(const float4*)(shift + oct * 8), sh1 = *(const float4*)(shift + oct * 8 + 4);
    const f32x2v scv[4] = {{sc0.x, sc0.y}, {sc0.z, sc0.w}, {sc1.x, sc1.y}, {sc1.z, sc1.w}};
    const f32x2v shv[4] = {{sh0.x, sh0.y}, {sh0.z, sh0.w}, {sh1.x, sh1.y}, {sh1.z, sh1.w}};
    for (int p = pl; p < HW; p += npl) {
      const int prow = rb_prow(p, W, pitch);
      const uint4 u = *(const uint4*)(sm + src + (src_padded ? prow : p) * src_rs + oct * 16);
      const unsigned w[4] = {u.x, u.y, u.z, u.w};
      unsigned ow[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {                              // as k_gn_onepass / k_gn_apply: packed fma, hardware exp2 / rcp
        const f32x2v x = {__uint_as_float(w[j] << 16), __uint_as_float(w[j] & 0xFFFF0000u)};
        f32x2v y = __builtin_elementwise_fma(x, scv[j], shv[j]);
        const f32x2v z = y * (f32x2v){-1.4426950408889634f, -1.4426950408889634f};
        const f32x2v d = (f32x2v){__builtin_amdgcn_exp2f(z.x), __builtin_amdgcn_exp2f(z.y)} + (f32x2v){1.0f, 1.0f};
        y = y * (f32x2v){__builtin_amdgcn_rcpf(d.x), __builtin_amdgcn_rcpf(d.y)};
        ow[j] = rt_pack2(y.x, y.y);
      }
      *(uint4*)(sm + dst + prow * dst_rs + oct * 16) = make_uint4(ow[0], ow[1], ow[2], ow[3]);
    }
  }
  __syncthreads();
}

// One K loop: acc[t][pt] += W[48 w + 16 t .. +16][k] * X[k][16 pt .. +16] over `n3` 64-channel chunks of a 3x3 segment on the
// padded image at b3 (row stride rs3, `cpt` chunks per tap) followed by nchunks - n3 chunks of 1x1 segments on the image at b1.
// wrow: this wave's weight stream + 8 lane elements.  The weights are packed in the order the fragments are consumed
// (ctdd_unet.h: [wave][chunk][tile][k half][lane][8]), so a wave-instruction reads 1 KiB of consecutive bytes and a wave's
// whole stream is sequential: with the plain [N][K] matrix the 16 lanes of a quarter wave sit in 16 different rows, every lane's
// 16 bytes are a request of their own at the L1, and the stream ran at 31 GB/s per CU (0.78 us per chunk against 0.29 us of
// matrix work).  The weights of chunk ci + PD are requested when chunk ci has been consumed; the compiler's counted vmcnt waits
// let PD - 1 chunks stay in flight.  wr: the ring, holding chunks 0 .. PD - 1 (rb_wprologue).
__device__ __attribute__((always_inline)) inline void rb_wload(u32x4 (&dst)[3][2], const unsigned short* __restrict__ wrow, int ci) {
#pragma unroll
  for (int t = 0; t < 3; ++t)
#pragma unroll
    for (int s = 0; s < 2; ++s) dst[t][s] = *(const u32x4*)(wrow + (size_t)ci * 3072 + (t * 2 + s) * 512);
}
// the first PD chunks of a weight stream (nchunks >= 9 > PD: a 3x3 segment of >= 64 channels): issued by the kernel BEFORE the
// GroupNorm phase that precedes the K loop, so that the stream's first latency hides behind it
template <int PD>
__device__ __attribute__((always_inline)) inline void rb_wprologue(u32x4 (&wr)[PD][3][2], const unsigned short* __restrict__ wrow) {
#pragma unroll
  for (int u = 0; u < PD; ++u) rb_wload(wr[u], wrow, u);
}

template <int NPT, int PD>
__device__ __attribute__((always_inline)) inline void rb_gemm(f32x4 (&acc)[3][NPT], u32x4 (&wr)[PD][3][2], const unsigned short* __restrict__ wrow, int nchunks, int n3,
                                                             int cpt, const unsigned char* sm, const int (&b3)[NPT], int rs3, int Wp,
                                                             const int (&b1)[NPT]) {
  auto wload = [&](u32x4 (&dst)[3][2], int ci) { rb_wload(dst, wrow, ci); };
  // the pixel fragments of chunk `cn` (requested in sequence, one chunk ahead of their use, so that the LDS latency hides behind
  // the previous chunk's matrix instructions; the request past the last chunk repeats a valid address)
  int tap = 0, cc = 0;
  auto xload = [&](bf16x8 (&xf)[NPT][2], int cn) {
    // (selects, not branches: a join inside the group would make the counted waits conservative)
    const int c = cn < nchunks ? cn : nchunks - 1;
    const bool three = c < n3;
    const int tp = tap < 8 ? tap : 8;
    const int dy = tp / 3 - 1, dx = tp - (tp / 3) * 3 - 1;
    const int koff = three ? (dy * Wp + dx) * rs3 + cc * 128 : (c - n3) * 128;
    const bool wrap = cc + 1 == cpt;
    cc = wrap ? 0 : cc + 1;
    tap += wrap ? 1 : 0;
#pragma unroll
    for (int pt = 0; pt < NPT; ++pt) {
      const int xb = (three ? b3[pt] : b1[pt]) + koff;
#pragma unroll
      for (int s = 0; s < 2; ++s) xf[pt][s] = *(const bf16x8*)(sm + xb + s * 64);
    }
  };
  // one chunk from ring slot `slot`; GUARD: the uniform tests of the last groups (the steady-state groups carry none, so that
  // the counted waits see one straight line of PD loads and PD uses)
  auto step = [&](u32x4 (&slot)[3][2], bf16x8 (&xf)[NPT][2], bf16x8 (&xnext)[NPT][2], int ci, auto guard) {
    constexpr bool GUARD = decltype(guard)::value;
    if (GUARD && ci >= nchunks) return;
    xload(xnext, ci + 1);
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int t = 0; t < 3; ++t)
#pragma unroll
        for (int pt = 0; pt < NPT; ++pt)
          acc[t][pt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, slot[t][s]), xf[pt][s], acc[t][pt], 0, 0, 0);
    if (!GUARD || ci + PD < nchunks) wload(slot, ci + PD);
  };
  static_assert(PD % 2 == 0, "the two pixel-fragment buffers alternate inside a group");
  bf16x8 xq[2][NPT][2];
  xload(xq[0], 0);
  int ci0 = 0;
  for (; ci0 + 2 * PD <= nchunks; ci0 += PD) {
#pragma unroll
    for (int u = 0; u < PD; ++u) step(wr[u], xq[u & 1], xq[(u + 1) & 1], ci0 + u, std::false_type{});
  }
  for (; ci0 < nchunks; ci0 += PD) {
#pragma unroll
    for (int u = 0; u < PD; ++u) step(wr[u], xq[u & 1], xq[(u + 1) & 1], ci0 + u, std::true_type{});
  }
}

template <int NPT>
__global__ __launch_bounds__(RB_THREADS, 1) void k_resblock_small(const ctdd_resblock_args a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char sm[];
  constexpr int PD = 6;
  const int t = threadIdx.x, b = blockIdx.x;
  const int H = a.H, W = a.W, HW = H * W, C = a.C1 + a.C2, Wp = W + 2;
  const RbLds L = rb_layout(H, W, C);
  const int lane = t & 63, wv = t >> 6, lj = lane & 15, lq = lane >> 4;

  const int K1 = 9 * C, K2 = 9 * RB_N + (a.skip ? C : 0);
  const unsigned short* w1p = (const unsigned short*)a.w1 + (size_t)wv * (K1 / 64) * 3072 + lane * 8;
  const unsigned short* w2p = (const unsigned short*)a.w2 + (size_t)wv * (K2 / 64) * 3072 + lane * 8;
  u32x4 wr[PD][3][2];                                         // the weight ring (rb_gemm)

  // ---- phase A: raw sample -> LDS, zero the slab, GroupNorm 1 + Swish into the slab
  {
    const int noct = C >> 3, nvec = HW * noct;
    const unsigned short* s1 = (const unsigned short*)a.s1_bf16 + (size_t)b * HW * a.C1;
    const unsigned short* s2 = (const unsigned short*)a.s2_bf16 + (size_t)b * HW * a.C2;
    constexpr int MAXV = 12;                                  // 64 pixels x 48 vectors over 256 threads; all requested before the first store
    u32x4 u[MAXV];
#pragma unroll
    for (int k = 0; k < MAXV; ++k) {
      const int v = t + k * RB_THREADS, p = v / noct, c0 = (v - p * noct) * 8;
      const unsigned short* src = c0 < a.C1 ? s1 + (size_t)p * a.C1 + c0 : s2 + (size_t)p * a.C2 + (c0 - a.C1);
      u[k] = v < nvec ? *(const u32x4*)src : (u32x4){0u, 0u, 0u, 0u};
    }
    rb_wprologue<PD>(wr, w1p);
#pragma unroll
    for (int k = 0; k < MAXV; ++k) {
      const int v = t + k * RB_THREADS, p = v / noct, c0 = (v - p * noct) * 8;
      if (v < nvec) *(u32x4*)(sm + L.raw + p * L.rsA + c0 * 2) = u[k];
    }
    const int nz = (L.part - L.slab) >> 4;
    for (int v = t; v < nz; v += RB_THREADS) *(uint4*)(sm + L.slab + v * 16) = make_uint4(0, 0, 0, 0);
    __syncthreads();
    rb_groupnorm(sm, L, L.raw, L.rsA, false, L.slab, L.rsA, HW, W, Wp, C, a.G1, a.gamma1, a.beta1, a.eps1);
  }

  // this lane's pixel of each pixel tile (rb_tile_pixel; one tile, H * W <= 16: the flattened pixels; pix < 0: computed, never stored)
  int pix[NPT], prow[NPT], b3[NPT], b1[NPT];
#pragma unroll
  for (int pt = 0; pt < NPT; ++pt) {
    if constexpr (NPT == 1) {
      const int pe = lj < HW ? lj : HW - 1;
      pix[pt] = lj < HW ? lj : -1;
      prow[pt] = rb_prow(pe, W, Wp);
      b1[pt] = L.raw + pe * L.rsA + lq * 16;
    } else {
      const RbPix q = rb_tile_pixel(pt, lj, H, W);
      pix[pt] = q.ok ? q.p : -1;
      prow[pt] = q.row;
      b1[pt] = L.raw + q.p * L.rsA + lq * 16;
    }
    b3[pt] = L.slab + prow[pt] * L.rsA + lq * 16;
  }
  const int n0 = wv * 48;                                     // this wave's first output channel
  f32x4 acc[3][NPT];
#pragma unroll
  for (int tt = 0; tt < 3; ++tt)
#pragma unroll
    for (int pt = 0; pt < NPT; ++pt) acc[tt][pt] = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};

  // ---- phase B: conv1 on the slab
  rb_gemm<NPT, PD>(acc, wr, w1p, K1 / 64, K1 / 64, C / 64, sm, b3, L.rsA, Wp, b1);
  __syncthreads();                                            // every wave has read its last a1 fragment: the slab becomes h1's
  rb_wprologue<PD>(wr, w2p);                                  // conv2's first chunks travel during the epilogue and GroupNorm 2
  {
    // borders of the N-channel image (its interior is written below by the lanes that own it)
    const int npc = L.rs2 >> 4, nv = L.prows * npc;
    for (int v = t; v < nv; v += RB_THREADS) {
      const int row = v / npc, y = row / Wp, x = row - y * Wp;
      if (y == 0 || y == H + 1 || x == 0 || x == W + 1) *(uint4*)(sm + L.slab + v * 16) = make_uint4(0, 0, 0, 0);
    }
#pragma unroll
    for (int tt = 0; tt < 3; ++tt) {
      const int n = n0 + tt * 16 + lq * 4;
      const float4 bv = *(const float4*)(a.bias1 + n);
      const float4 tb = a.tbias ? *(const float4*)(a.tbias + (size_t)b * a.tb_stride + n) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      const float add[4] = {bv.x + tb.x, bv.y + tb.y, bv.z + tb.z, bv.w + tb.w};
#pragma unroll
      for (int pt = 0; pt < NPT; ++pt) {
        if (pix[pt] >= 0) {
          const f32x4 v = acc[tt][pt];
          *(uint2*)(sm + L.slab + prow[pt] * L.rs2 + n * 2) =
              make_uint2(rt_pack2(v[0] + add[0], v[1] + add[1]), rt_pack2(v[2] + add[2], v[3] + add[3]));
        }
        acc[tt][pt] = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
      }
    }
  }
  __syncthreads();

  // ---- phase C: GroupNorm 2 + Swish of the bf16 h1, in place
  rb_groupnorm(sm, L, L.slab, L.rs2, true, L.slab, L.rs2, HW, W, Wp, RB_N, a.G2, a.gamma2, a.beta2, a.eps2);

  // ---- phase D: conv2 on a2, then the 1x1 skip segments on the raw input
#pragma unroll
  for (int pt = 0; pt < NPT; ++pt) b3[pt] = L.slab + prow[pt] * L.rs2 + lq * 16;
  rb_gemm<NPT, PD>(acc, wr, w2p, K2 / 64, 9 * RB_N / 64, RB_N / 64, sm, b3, L.rs2, Wp, b1);
  __syncthreads();                                            // a2 is dead: the slab becomes the [HW][N] output image
#pragma unroll
  for (int tt = 0; tt < 3; ++tt) {
    const int n = n0 + tt * 16 + lq * 4;
    const float4 bv = *(const float4*)(a.bias2 + n);
#pragma unroll
    for (int pt = 0; pt < NPT; ++pt) {
      if (pix[pt] >= 0) {
        const f32x4 v = acc[tt][pt];
        float o[4] = {v[0] + bv.x, v[1] + bv.y, v[2] + bv.z, v[3] + bv.w};
        if (!a.skip) {                                        // residual: the raw input (C1 == N)
          const uint2 r = *(const uint2*)(sm + L.raw + pix[pt] * L.rsA + n * 2);
          o[0] += __uint_as_float(r.x << 16); o[1] += __uint_as_float(r.x & 0xFFFF0000u);
          o[2] += __uint_as_float(r.y << 16); o[3] += __uint_as_float(r.y & 0xFFFF0000u);
        }
        *(uint2*)(sm + L.slab + pix[pt] * L.rs2 + n * 2) = make_uint2(rt_pack2(o[0], o[1]), rt_pack2(o[2], o[3]));
      }
    }
  }
  __syncthreads();
  {
    constexpr int npc = RB_N / 8;
    unsigned short* out = (unsigned short*)a.out_bf16 + (size_t)b * HW * RB_N;
    for (int v = t; v < HW * npc; v += RB_THREADS) {
      const int p = v / npc, c0 = (v - p * npc) * 8;
      *(uint4*)(out + (size_t)p * RB_N + c0) = *(const uint4*)(sm + L.slab + p * L.rs2 + c0 * 2);
    }
  }
}

// ---------------------------------------------------------------- k_resblock_mid: the same block for a sample of <= 14 x 14 pixels
//
// Ownership as above (one workgroup of four waves per sample, wave w owns channels [48 w, 48 w + 48)).  What changes is what LDS
// holds and what a pixel tile is.  LDS: ONE zero-bordered slab of 192 channels and the reduction scratch, no raw copy of the input.
// The slab has a FIXED PITCH of 16 positions per padded grid row whatever W <= 14 (position 0 and positions > W are zero), one
// guard row before and after: ((H + 2) 16 + 2) rows x 416 bytes = 105 KiB at H = 14.  Pixel tile y = output row y, lane j = padded
// column j (pixel x = j - 1; lanes 0 and > W compute a value that is never stored), RM_NPT = 14 tiles (168 accumulator registers), tiles
// y >= H skipped wave-uniformly.  The fragment that tap (dy, dx) needs for row y is then the fragment of padded row y + 1 + dy at
// column shift dx: lane j reads slab row 1 + 16 (y + 1 + dy) + j + dx, 16 consecutive rows at a stride of 416 bytes (104 dwords,
// 8 mod 16: conflict-free under the lane groups of ds_read_b128, tools/lds_bank_model.py; the shifts of lanes 0 and 15 of the
// first and last padded row land in the guard rows).  The K loop (rt_gemm_rows, row_tile.hpp) has the unit (32 channels, dx): the up-to-16 row fragments of that
// column shift are read ONCE, and output row y takes nine matrix instructions (three dy x three 16-channel weight tiles) on F[y],
// F[y+1], F[y+2] from registers: 16 ds_read_b128 per 126 matrix instructions (the flattened 16-pixel tiles this replaced took 39 per 117).  The weights are streamed in
// that order (unit -> dy -> tile, 9 KiB per wave and unit) through a ring of two units (72 registers).
// GroupNorm 1 takes its statistics straight from global memory (all sources first: a group may straddle two sources), then
// conv1 runs SOURCE BY SOURCE in 32-channel units (a 96-channel source is three of them: nothing is padded): normalise + Swish
// that source from global memory into the slab, barrier, its units, barrier.  The 1x1 skip segments read the raw sources as B
// fragments straight from global memory (a lane's 16 bytes = 8 consecutive channels of its pixel), before GroupNorm 2 so that
// conv2's first weights travel behind it.  The residual is added in the accumulator layout from global memory (one rounding of
// acc + bias + residual, as the launches it replaces).
constexpr int RM_NPT = 14, RM_PITCH = 16, RM_MAXH = 14, RM_MAXCS = 192;
constexpr int RM_RS = RB_N * 2 + 32;                           // bytes per slab position

__host__ __device__ inline RbLds rm_layout(int H, int W) {
  RbLds L;
  (void)W;                                                    // (the pitch is fixed)
  L.rsA = L.rs2 = RB_N * 2 + 32;
  L.prows = (H + 2) * RM_PITCH;
  L.raw = L.slab = L.rs2;                                     // padded position 0 (after the guard row)
  L.part = (L.prows + 2) * L.rs2;
  L.red = L.part + RB_THREADS * RB_PST * 4;
  L.scale = L.red + 2 * RB_MAXC * 8;
  L.total = L.scale + 2 * RB_MAXC * 4;
  return L;
}

// GroupNorm 1 statistics of the channel concatenation of the sample's sources (s1 / s2: the sample's first element), read from global
// memory in rb_groupnorm's order (fp32 per thread over its pixels, fp64 across threads and group members); leaves scale / shift of all
// C1 + C2 channels in LDS.  Ends with a barrier.
__device__ __attribute__((always_inline)) inline void rm_gn1_stats(unsigned char* sm, const RbLds& L, const unsigned short* __restrict__ s1,
                                                                  const unsigned short* __restrict__ s2, int C1, int C2, int HW, int G,
                                                                  const float* __restrict__ gamma, const float* __restrict__ beta, float eps) {
  const int t = threadIdx.x, C = C1 + C2, noct = C >> 3;
  const int npl = RB_THREADS / noct < HW ? RB_THREADS / noct : HW, T = noct * npl;
  const bool act = t < T;
  const int oct = act ? t % noct : 0, pl = act ? t / noct : 0, c0 = oct * 8;
  const bool first = c0 < C1;
  const unsigned short* src = first ? s1 + c0 : s2 + (c0 - C1);
  const int cs = first ? C1 : C2;
  float* part = (float*)(sm + L.part);
  double* red = (double*)(sm + L.red);
  float* scale = (float*)(sm + L.scale);
  float* shift = scale + RB_MAXC;
  float sx[8], sq[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) { sx[j] = 0.0f; sq[j] = 0.0f; }
  if (act) {
#pragma unroll 4
    for (int p = pl; p < HW; p += npl) {
      const u32x4 u = *(const u32x4*)(src + (size_t)p * cs);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float x0 = __uint_as_float(u[j] << 16), x1 = __uint_as_float(u[j] & 0xFFFF0000u);
        sx[2 * j] += x0; sq[2 * j] = fmaf(x0, x0, sq[2 * j]);
        sx[2 * j + 1] += x1; sq[2 * j + 1] = fmaf(x1, x1, sq[2 * j + 1]);
      }
    }
    float4* pt = (float4*)(part + t * RB_PST);
    pt[0] = make_float4(sx[0], sx[1], sx[2], sx[3]); pt[1] = make_float4(sx[4], sx[5], sx[6], sx[7]);
    pt[2] = make_float4(sq[0], sq[1], sq[2], sq[3]); pt[3] = make_float4(sq[4], sq[5], sq[6], sq[7]);
  }
  __syncthreads();
  for (int r = t; r < 2 * C; r += RB_THREADS) {
    const int m = r >= C ? 1 : 0, c = r - m * C;
    const float* pp = part + (c >> 3) * RB_PST + m * 8 + (c & 7);
    double acc = 0.0;
    for (int q = 0; q < npl; ++q) acc += (double)pp[q * noct * RB_PST];
    red[r] = acc;
  }
  __syncthreads();
  const int cg = C / G;
  for (int c = t; c < C; c += RB_THREADS) {
    const int g0 = (c / cg) * cg;
    double s = 0.0, q = 0.0;
    for (int j = g0; j < g0 + cg; ++j) { s += red[j]; q += red[C + j]; }
    const double n = (double)cg * (double)HW;
    const double mean = s / n;
    const double var = fmax(q / n - mean * mean, 0.0);
    const float rstd = (float)(1.0 / sqrt(var + (double)eps));
    scale[c] = rstd * gamma[c];
    shift[c] = beta[c] - (float)mean * rstd * gamma[c];
  }
  __syncthreads();
}

// bf16(swish(x * scale + shift)) of ONE source ([HW][cs] in global memory, channels [coff, coff + cs) of the concatenation) into
// columns [0, cs) of the slab's interior rows.  No barrier of its own.
__device__ __attribute__((always_inline)) inline void rm_gn1_apply(unsigned char* sm, const RbLds& L, const unsigned short* __restrict__ src, int cs,
                                                                  int coff, int HW, int W) {
  const int t = threadIdx.x, noct = cs >> 3, npl = RB_THREADS / noct;
  if (t >= noct * npl) return;
  const int oct = t % noct, pl = t / noct;
  const float* scale = (const float*)(sm + L.scale) + coff + oct * 8;
  const float* shift = scale + RB_MAXC;
  const float4 sc0 = *(const float4*)scale, sc1 = *(const float4*)(scale + 4);
  const float4 sh0 = *(const float4*)shift, sh1 = *(const float4*)(shift + 4);
  const f32x2v scv[4] = {{sc0.x, sc0.y}, {sc0.z, sc0.w}, {sc1.x, sc1.y}, {sc1.z, sc1.w}};
  const f32x2v shv[4] = {{sh0.x, sh0.y}, {sh0.z, sh0.w}, {sh1.x, sh1.y}, {sh1.z, sh1.w}};
  const unsigned short* sp = src + oct * 8;
#pragma unroll 4
  for (int p = pl; p < HW; p += npl) {
    const u32x4 u = *(const u32x4*)(sp + (size_t)p * cs);
    unsigned ow[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {                                // as rb_groupnorm: packed fma, hardware exp2 / rcp
      const f32x2v x = {__uint_as_float(u[j] << 16), __uint_as_float(u[j] & 0xFFFF0000u)};
      f32x2v y = __builtin_elementwise_fma(x, scv[j], shv[j]);
      const f32x2v z = y * (f32x2v){-1.4426950408889634f, -1.4426950408889634f};
      const f32x2v d = (f32x2v){__builtin_amdgcn_exp2f(z.x), __builtin_amdgcn_exp2f(z.y)} + (f32x2v){1.0f, 1.0f};
      y = y * (f32x2v){__builtin_amdgcn_rcpf(d.x), __builtin_amdgcn_rcpf(d.y)};
      ow[j] = rt_pack2(y.x, y.y);
    }
    *(uint4*)(sm + L.slab + rb_prow(p, W, RM_PITCH) * L.rs2 + oct * 16) = make_uint4(ow[0], ow[1], ow[2], ow[3]);
  }
}

// the first two units of a 3x3 weight stream (issued before the phase that precedes the K loop)
__device__ __attribute__((always_inline)) inline void rm_wprologue(u32x4 (&wr)[2][3][3], const unsigned short* __restrict__ wrow, int nunits) {
#pragma unroll
  for (int u = 0; u < 2; ++u)
    if (u < nunits) rt_wload9(wr[u], wrow, u);
}

// The 1x1 skip segments: nsk 32-channel units of the raw sources, B fragments straight from global memory (lane j of tile y: pixel
// (y, j - 1), columns off the sample clamped into it: computed, never stored), weight ring ws holding units 0 and 1.
template <bool FULL>
__device__ __attribute__((always_inline)) inline void rm_gemm_skip(f32x4 (&acc)[3][RM_NPT], u32x4 (&ws)[2][3], const unsigned short* __restrict__ wrow, int nsk,
                                                                  const unsigned short* __restrict__ s1, const unsigned short* __restrict__ s2,
                                                                  int C1, int C2, int xc, int lq, int H, int W) {
  const int nc1 = C1 >> 5;
  auto gload = [&](bf16x8 (&g)[RM_NPT], int u) {
    const int ue = u < nsk ? u : nsk - 1;                       // past the last unit: the last unit again
    const bool two = ue >= nc1;
    const unsigned char* base = (const unsigned char*)(two ? s2 : s1);
    const int cs = two ? C2 : C1, cb = (ue - (two ? nc1 : 0)) * 32 + lq * 8;
#pragma unroll
    for (int y = 0; y < RM_NPT; ++y) {
      const int ye = FULL || y < H ? y : H - 1;
      g[y] = *(const bf16x8*)(base + (unsigned)(((ye * W + xc) * cs + cb) * 2));
    }
  };
  auto step = [&](u32x4 (&slot)[3], bf16x8 (&gc)[RM_NPT], bf16x8 (&gn)[RM_NPT], int u, auto guard) {
    constexpr bool GUARD = decltype(guard)::value;
    if (GUARD && u >= nsk) return;
    gload(gn, u + 1);
#pragma unroll
    for (int y = 0; y < RM_NPT; ++y) {
      if (FULL || y < H) {
#pragma unroll
        for (int t = 0; t < 3; ++t)
          acc[t][y] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, slot[t]), gc[y], acc[t][y], 0, 0, 0);
      }
    }
    if (!GUARD || u + 2 < nsk) rt_wload3(slot, wrow, u + 2);
    __builtin_amdgcn_sched_barrier(0);
  };
  bf16x8 G[2][RM_NPT];
  gload(G[0], 0);
  __builtin_amdgcn_s_waitcnt(0x0F70);                           // vmcnt(0), as in rt_gemm_rows (unit 0's fragments are needed at once)
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

// FULL: H = 14, the K loops without their row tests (one straight line per unit)
template <bool FULL>
__global__ __launch_bounds__(RB_THREADS, 1) void k_resblock_mid(const ctdd_resblock_args a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char sm[];
  constexpr int NPT = RM_NPT;
  const int t = threadIdx.x, b = blockIdx.x;
  const int H = FULL ? RM_NPT : a.H, W = a.W, HW = H * W, C1 = a.C1, C2 = a.C2;
  const RbLds L = rm_layout(H, W);
  const int lane = t & 63, wv = t >> 6, lj = lane & 15, lq = lane >> 4;
  const int nu1a = 3 * (C1 >> 5), nu1b = 3 * (C2 >> 5), nsk = a.skip ? (C1 + C2) >> 5 : 0;
  const unsigned short* w1p = (const unsigned short*)a.w1 + (size_t)wv * (nu1a + nu1b) * RT_UNIT + lane * 8;
  const unsigned short* s1 = (const unsigned short*)a.s1_bf16 + (size_t)b * HW * C1;
  const unsigned short* s2 = (const unsigned short*)a.s2_bf16 + (size_t)b * HW * C2;
  u32x4 wr[2][3][3];                                          // the weight ring (rt_gemm_rows)

  // ---- phase A: zero the slab and its guard rows (border positions stay zero to the end), GroupNorm 1 statistics from global memory
  rm_wprologue(wr, w1p, nu1a);
  for (int v = t; v < (L.part >> 4); v += RB_THREADS) *(uint4*)(sm + v * 16) = make_uint4(0, 0, 0, 0);
  rm_gn1_stats(sm, L, s1, s2, C1, C2, HW, a.G1, a.gamma1, a.beta1, a.eps1);

  const int fb = L.slab + lj * RM_RS + lq * 16;               // this lane's position of padded row 0 + its k quarter
  const int n0 = wv * 48;                                     // this wave's first output channel
  f32x4 acc[3][NPT];
#pragma unroll
  for (int tt = 0; tt < 3; ++tt)
#pragma unroll
    for (int pt = 0; pt < NPT; ++pt) acc[tt][pt] = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};

  // ---- phase B: conv1, source by source (the slab never holds more than 192 channels)
  for (int s = 0; s < (C2 ? 2 : 1); ++s) {
    rm_gn1_apply(sm, L, s ? s2 : s1, s ? C2 : C1, s ? C1 : 0, HW, W);
    __syncthreads();
    rt_gemm_rows<FULL, RM_RS, RM_PITCH>(acc, wr, w1p + (size_t)(s ? nu1a : 0) * RT_UNIT, s ? nu1b : nu1a, sm, fb, H);
    __syncthreads();                                          // every wave has read its last fragment of this source
    if (s == 0 && C2) rm_wprologue(wr, w1p + (size_t)nu1a * RT_UNIT, nu1b);
  }
  // the next stream's first units travel during the epilogue: the skip segments' (after the 18 units of the 3x3 part) or conv2's
  const int tw = rt_again(t);
  const unsigned short* w2p = (const unsigned short*)a.w2 + (size_t)(tw >> 6) * (18 * RT_UNIT + nsk * 1536) + (tw & 63) * 8;
  u32x4 ws[2][3];
  if (nsk) {
    rt_wload3(ws[0], w2p + (size_t)18 * RT_UNIT, 0);
    if (nsk > 1) rt_wload3(ws[1], w2p + (size_t)18 * RT_UNIT, 1);
  } else {
    rm_wprologue(wr, w2p, 18);
  }
  const int lj1 = rt_again(lj);
  const bool own1 = lj1 >= 1 && lj1 <= W;                      // this lane's column is a pixel
#pragma unroll
  for (int tt = 0; tt < 3; ++tt) {
    const int n = n0 + tt * 16 + lq * 4;
    const float4 bv = *(const float4*)(a.bias1 + n);
    const float4 tb = a.tbias ? *(const float4*)(a.tbias + (size_t)b * a.tb_stride + n) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const float add[4] = {bv.x + tb.x, bv.y + tb.y, bv.z + tb.z, bv.w + tb.w};
#pragma unroll
    for (int y = 0; y < NPT; ++y) {
      if (y < H && own1) {
        const f32x4 v = acc[tt][y];
        *(uint2*)(sm + L.slab + ((y + 1) * RM_PITCH + lj1) * RM_RS + n * 2) =
            make_uint2(rt_pack2(v[0] + add[0], v[1] + add[1]), rt_pack2(v[2] + add[2], v[3] + add[3]));
      }
      acc[tt][y] = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
    }
  }
  __syncthreads();

  // ---- phase C: the 1x1 skip segments on the raw sources, B fragments straight from global memory (conv2's sums start with them)
  if (nsk) {
    const int ljs = rt_again(lj), xc = ljs < 1 ? 0 : (ljs > W ? W - 1 : ljs - 1);
    rm_gemm_skip<FULL>(acc, ws, w2p + (size_t)18 * RT_UNIT, nsk, s1, s2, C1, C2, xc, lq, H, W);
    rm_wprologue(wr, w2p, 18);                                // conv2's first units travel during GroupNorm 2
  }

  // ---- phase D: GroupNorm 2 + Swish of the bf16 h1, in place, then conv2 on a2
  rb_groupnorm(sm, L, L.slab, L.rs2, true, L.slab, L.rs2, HW, W, RM_PITCH, RB_N, a.G2, a.gamma2, a.beta2, a.eps2);
  rt_gemm_rows<FULL, RM_RS, RM_PITCH>(acc, wr, w2p, 18, sm, fb, H);
  __syncthreads();                                            // a2 is dead: the slab becomes the [HW][N] output image
  const int lj2 = rt_again(lj);
  const bool own2 = lj2 >= 1 && lj2 <= W;
  const int x2 = own2 ? lj2 - 1 : 0;
#pragma unroll
  for (int tt = 0; tt < 3; ++tt) {
    const int n = n0 + tt * 16 + lq * 4;
    const float4 bv = *(const float4*)(a.bias2 + n);
    uint2 r[NPT] = {};
    if (!a.skip) {                                            // residual: the raw input (C1 == N), in this lane's accumulator layout
#pragma unroll
      for (int y = 0; y < NPT; ++y) r[y] = *(const uint2*)(s1 + (size_t)((y < H ? y : H - 1) * W + x2) * RB_N + n);
    }
#pragma unroll
    for (int y = 0; y < NPT; ++y) {
      if (y < H && own2) {
        const f32x4 v = acc[tt][y];
        float o[4] = {v[0] + bv.x, v[1] + bv.y, v[2] + bv.z, v[3] + bv.w};
        if (!a.skip) {
          o[0] += __uint_as_float(r[y].x << 16); o[1] += __uint_as_float(r[y].x & 0xFFFF0000u);
          o[2] += __uint_as_float(r[y].y << 16); o[3] += __uint_as_float(r[y].y & 0xFFFF0000u);
        }
        *(uint2*)(sm + L.slab + (y * W + x2) * RM_RS + n * 2) = make_uint2(rt_pack2(o[0], o[1]), rt_pack2(o[2], o[3]));
      }
    }
  }
  __syncthreads();
  {
    constexpr int npc = RB_N / 8;
    unsigned short* out = (unsigned short*)a.out_bf16 + (size_t)b * HW * RB_N;
    for (int v = t; v < HW * npc; v += RB_THREADS) {
      const int p = v / npc, c0 = (v - p * npc) * 8;
      *(uint4*)(out + (size_t)p * RB_N + c0) = *(const uint4*)(sm + L.slab + p * RM_RS + c0 * 2);
    }
  }
}

}  // namespace
}  // namespace ctdd

using namespace ctdd;

// Refuses (non-zero, ctdd_last_error set, nothing launched) what the kernel cannot hold: fp32 mode, H*W > 64 or W > 8, more than
// 16 pixels whose interior spans more than 80 rows of the zero-bordered grid (five tiles of 16 consecutive rows), N != 192,
// source channel counts that are not multiples of 64 or exceed 384 in all, groups that do not divide the channels, an LDS
// image over the CU's 160 KiB.
extern "C" int ctdd_unet_resblock_small(const void* args_, int f32, void* stream) {
  CTDD_REQUIRE(args_, CTDD_EINVAL, "ctdd_unet_resblock_small: null arguments");
  const ctdd_resblock_args& a = *(const ctdd_resblock_args*)args_;
  CTDD_REQUIRE(f32 == 0, CTDD_ERANGE, "ctdd_unet_resblock_small: bf16 inference only (the fp32 mode keeps the four launches)");
  // the interior span of the zero-bordered grid, first to last interior row of the slab: what the tiles of 16 consecutive rows cover
  const int span = (a.H - 1) * (a.W + 2) + a.W;
  CTDD_REQUIRE(a.B > 0 && a.H > 0 && a.W > 0 && a.W <= 8 && a.H * a.W <= 64 && (a.H * a.W <= 16 || span <= 80), CTDD_ERANGE,
               "ctdd_unet_resblock_small: a sample of %dx%d pixels does not fit the workgroup tile (H*W <= 64, W <= 8, (H-1)(W+2)+W <= 80)", a.H, a.W);
  const int C = a.C1 + a.C2;
  CTDD_REQUIRE(a.N == RB_N && a.C1 > 0 && a.C1 % 64 == 0 && a.C2 >= 0 && a.C2 % 64 == 0 && C <= RB_MAXC, CTDD_ERANGE,
               "ctdd_unet_resblock_small: channel counts off the tile (N=%d, C1=%d, C2=%d; N = 192, sources in multiples of 64, <= 384)", a.N,
               a.C1, a.C2);
  CTDD_REQUIRE(a.G1 > 0 && C % a.G1 == 0 && a.G2 > 0 && RB_N % a.G2 == 0, CTDD_EINVAL, "ctdd_unet_resblock_small: groups do not divide the channels");
  CTDD_REQUIRE(a.skip || (a.C2 == 0 && a.C1 == RB_N), CTDD_EINVAL, "ctdd_unet_resblock_small: a residual block needs C1 == N and one source");
  CTDD_REQUIRE(a.s1_bf16 && (a.C2 == 0 || a.s2_bf16) && a.w1 && a.w2 && a.bias1 && a.bias2 && a.gamma1 && a.beta1 && a.gamma2 && a.beta2 &&
                   a.out_bf16, CTDD_EINVAL, "ctdd_unet_resblock_small: null pointer");
  const RbLds L = rb_layout(a.H, a.W, C);
  CTDD_REQUIRE(L.total <= 160 * 1024, CTDD_ERANGE, "ctdd_unet_resblock_small: LDS image of %d bytes over the 160 KiB budget", L.total);
  hipStream_t st = (hipStream_t)stream;
  static bool attr_done[3][16] = {};
  if (a.H * a.W <= 16) {
    ensure_lds_ceiling((const void*)k_resblock_small<1>, attr_done[0]);
    hipLaunchKernelGGL(k_resblock_small<1>, dim3(a.B), dim3(RB_THREADS), (size_t)L.total, st, a);
  } else if (span > 64) {                                     // 8x8: five tiles of slab rows
    ensure_lds_ceiling((const void*)k_resblock_small<5>, attr_done[2]);
    hipLaunchKernelGGL(k_resblock_small<5>, dim3(a.B), dim3(RB_THREADS), (size_t)L.total, st, a);
  } else {
    ensure_lds_ceiling((const void*)k_resblock_small<4>, attr_done[1]);
    hipLaunchKernelGGL(k_resblock_small<4>, dim3(a.B), dim3(RB_THREADS), (size_t)L.total, st, a);
  }
  return finish_launch("k_resblock_small");
}

// The same block for a sample of up to 14 x 14 pixels (the 14x14 level), k_resblock_mid.  Refuses (non-zero, ctdd_last_error set, nothing
// launched): fp32 mode, H > 14 or W > 14 (the slab's pitch of 16 positions), N != 192, a source that is not a multiple of 32
// channels or exceeds 192, groups that do not divide the channels, an LDS image over the CU's 160 KiB.
extern "C" int ctdd_unet_resblock_mid(const void* args_, int f32, void* stream) {
  CTDD_REQUIRE(args_, CTDD_EINVAL, "ctdd_unet_resblock_mid: null arguments");
  const ctdd_resblock_args& a = *(const ctdd_resblock_args*)args_;
  CTDD_REQUIRE(f32 == 0, CTDD_ERANGE, "ctdd_unet_resblock_mid: bf16 inference only (the fp32 mode keeps the four launches)");
  CTDD_REQUIRE(a.B > 0 && a.H > 0 && a.W > 0 && a.H <= RM_MAXH && a.W <= RM_PITCH - 2, CTDD_ERANGE,
               "ctdd_unet_resblock_mid: a sample of %dx%d pixels does not fit the workgroup tile (H <= 14, W <= 14)", a.H, a.W);
  const int C = a.C1 + a.C2;
  CTDD_REQUIRE(a.N == RB_N && a.C1 > 0 && a.C1 % 32 == 0 && a.C1 <= RM_MAXCS && a.C2 >= 0 && a.C2 % 32 == 0 && a.C2 <= RM_MAXCS, CTDD_ERANGE,
               "ctdd_unet_resblock_mid: channel counts off the tile (N=%d, C1=%d, C2=%d; N = 192, sources in multiples of 32, <= 192 each)", a.N,
               a.C1, a.C2);
  CTDD_REQUIRE(a.G1 > 0 && C % a.G1 == 0 && a.G2 > 0 && RB_N % a.G2 == 0, CTDD_EINVAL, "ctdd_unet_resblock_mid: groups do not divide the channels");
  CTDD_REQUIRE(a.skip || (a.C2 == 0 && a.C1 == RB_N), CTDD_EINVAL, "ctdd_unet_resblock_mid: a residual block needs C1 == N and one source");
  CTDD_REQUIRE(a.s1_bf16 && (a.C2 == 0 || a.s2_bf16) && a.w1 && a.w2 && a.bias1 && a.bias2 && a.gamma1 && a.beta1 && a.gamma2 && a.beta2 &&
                   a.out_bf16, CTDD_EINVAL, "ctdd_unet_resblock_mid: null pointer");
  const RbLds L = rm_layout(a.H, a.W);
  CTDD_REQUIRE(L.total <= 160 * 1024, CTDD_ERANGE, "ctdd_unet_resblock_mid: LDS image of %d bytes over the 160 KiB budget", L.total);
  static bool attr_done[2][16] = {};
  if (a.H == RM_NPT) {
    ensure_lds_ceiling((const void*)k_resblock_mid<true>, attr_done[1]);
    hipLaunchKernelGGL(k_resblock_mid<true>, dim3(a.B), dim3(RB_THREADS), (size_t)L.total, (hipStream_t)stream, a);
  } else {
    ensure_lds_ceiling((const void*)k_resblock_mid<false>, attr_done[0]);
    hipLaunchKernelGGL(k_resblock_mid<false>, dim3(a.B), dim3(RB_THREADS), (size_t)L.total, (hipStream_t)stream, a);
  }
  return finish_launch("k_resblock_mid");
}
