// unet_attn_kernels.hip -- the mid-block self-attention (reference lib/networks/unet.py:152-200) behind its GroupNorm in ONE launch
// (bf16 inference): qkv 1x1 convolution -> per-head softmax attention -> proj 1x1 convolution + residual.
//
// The block is sample-local like the ResBlocks of unet_resblock_kernels.hip: a workgroup of four waves owns ONE sample of T <= 64
// tokens and C = 192 channels in 8 heads of ch = 24.  It replaces ctdd_unet_conv_patch (fp32 qkv) -> ctdd_unet_attention ->
// ctdd_unet_conv_patch (+ residual) with the rounding points of those three: `an` (the GroupNorm output) is bf16, qkv = fp32
// accumulator + bias (never rounded, never in memory), scores / softmax (max subtracted) / value product in fp32, `ao` rounded to
// bf16 once, the output rounded once from (acc + bias) + x.  What differs is the order of the fp32 sums (both products' accumulators
// start from the bias instead of adding it last; the value product takes its keys in steps of {r, 4 + r, 8 + r, 12 + r}) and the
// softmax's exponential, the hardware exp2 of (s - max) log2 e where ctdd_unet_attention calls expf.
//
//   1. `an` [T][192] -> LDS (416-byte rows, rows T .. 63 zero).
//   2. qkv^T = Wqkv . an^T on v_mfma_f32_16x16x32_bf16, weights as the A operand and tokens as the B operand (k_resblock_small's
//      mapping): wave w owns output channels [144 w, 144 w + 144) = heads 2 w and 2 w + 1 whole (the reference's channel order is
//      [q | k | v] per head), nine weight tiles x four token tiles, 144 accumulator registers.  The weights come global ->
//      registers in fragment order (pack_attention_weights), all 54 KiB of a wave requested before `an` is stored to LDS.
//   3. barrier (`an` is dead); each wave writes its two heads as fp32 [64 tokens][q s | k s | v] rows of 76 floats (s = ch^-1/4)
//      into the head's LDS region, which only that wave reads.
//   4. per head, on the exact-fp32 v_mfma_f32_16x16x4_f32 (bit for bit an fmaf chain in k order, at the f32 vector rate, with the
//      operand traffic off the vector unit -- a 4 x 4 register-tile port of k_attn_small_t4 would have left a quarter of the lanes
//      idle at T = 49 and had a higher floor): S^T = (k s)(q s)^T with keys as rows, so that a lane holds 16 keys of ONE query
//      and the softmax needs two cross-lane steps; the sums of keys >= T start from -inf, so they never are the maximum and
//      get weight exactly 0.  A lane's
//      register r of key tile si is key 16 si + 4 (lane >> 4) + r of query (lane & 15): exactly the B operand of
//      O^T = v^T P^T when k step (si, r) of the value product takes keys {16 si + 4 g + r : g = 0 .. 3}.  So the weights go from
//      the score accumulators into the value product with no movement; pad tokens carry finite v (the bias) against zero weights.
//      O^T has 4 consecutive channels of one token per lane: bf16(O / sum) is stored as 8 bytes into the first 48 bytes of the
//      token's row of the head's region (q is dead by then).
//   5. barrier; out^T = Wproj . ao^T, wave w owns output channels [48 w, 48 w + 48); the B fragments (8 consecutive channels of
//      one head) come from the heads' regions.  Epilogue in the accumulator layout: + x read from global memory (requested before
//      the attention phase, like proj's weights and bias), 8-byte stores of tokens < T.
// LDS: 8 regions of 64 x 304 bytes = 152 KiB; the `an` image (26 KiB) lies under them.
#include "row_tile.hpp"
#include "../../include/ctdd_unet.h"

namespace ctdd {
namespace {

constexpr int AB_THREADS = 256, AB_C = 192, AB_HEADS = 8, AB_CH = AB_C / AB_HEADS, AB_TP = 64;
constexpr int AB_RS = AB_C * 2 + 32;                           // bytes per token of the bf16 `an` image
constexpr int AB_HROW = (3 * AB_CH + 4) * 4;                   // bytes per token of a head's fp32 [q | k | v] region (76 floats: 4 rows apart = 16 banks apart)
constexpr int AB_HREG = AB_TP * AB_HROW;
constexpr int AB_LDS = AB_HEADS * AB_HREG;
constexpr int AB_KS = AB_C / 32;                               // k steps of the two bf16 products
constexpr int AB_NQT = 3 * AB_C / 64;                          // weight tiles per wave of the qkv product
static_assert(AB_TP * AB_RS <= AB_LDS && AB_CH % 4 == 0 && AB_CH % 8 == 0 && AB_CH > 16 && AB_CH <= 32 && AB_NQT * 16 == 2 * 3 * AB_CH, "tile geometry");

__global__ __launch_bounds__(AB_THREADS, 1) void k_attn_block(const ctdd_attn_block_args a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char sm[];
  const int t = threadIdx.x, b = blockIdx.x, T = a.T;
  const int lane = t & 63, wv = t >> 6, lj = lane & 15, lq = lane >> 4;
  const unsigned short* wq = (const unsigned short*)a.w_qkv + (size_t)wv * (AB_KS * AB_NQT * 512) + lane * 8;
  const unsigned short* wp = (const unsigned short*)a.w_proj + (size_t)wv * (AB_KS * 3 * 512) + lane * 8;

  // ---- 1: the sample's `an` -> LDS, pad tokens zero.  Everything the qkv product reads from global memory is requested here, in one
  // straight line with no branch (a pad token's load repeats the last token's address and is zeroed by a select: a branch around a
  // load, or a load left inside the K loop, costs a full memory round trip where it is waited for): `an`, the bias -- the
  // accumulators start from it --, then all of this wave's 54 KiB of qkv weights (216 registers).
  constexpr int NV = AB_C / 8, MAXV = AB_TP * NV / AB_THREADS;
  const unsigned short* an = (const unsigned short*)a.an_bf16 + (size_t)b * T * AB_C;
  u32x4 u[MAXV];
#pragma unroll
  for (int k = 0; k < MAXV; ++k) {
    const int v = t + k * AB_THREADS, p = v / NV, c8 = v - p * NV, pc = p < T ? p : T - 1;
    u[k] = *(const u32x4*)(an + (size_t)pc * AB_C + c8 * 8);
  }
  asm volatile("" ::: "memory");                              // `an` first: its stores to LDS then wait for it alone, with the weights in flight
  f32x4 acc[AB_NQT][4];
#pragma unroll
  for (int tt = 0; tt < AB_NQT; ++tt) {
    const float4 bv = *(const float4*)(a.b_qkv + wv * (AB_NQT * 16) + 16 * tt + 4 * lq);
#pragma unroll
    for (int pt = 0; pt < 4; ++pt) acc[tt][pt] = (f32x4){bv.x, bv.y, bv.z, bv.w};
  }
  u32x4 wr[AB_KS][AB_NQT];
#pragma unroll
  for (int ks = 0; ks < AB_KS; ++ks)
#pragma unroll
    for (int tt = 0; tt < AB_NQT; ++tt) wr[ks][tt] = *(const u32x4*)(wq + (ks * AB_NQT + tt) * 512);
#pragma unroll
  for (int k = 0; k < MAXV; ++k) {
    const int v = t + k * AB_THREADS, p = v / NV, c8 = v - p * NV;
    *(u32x4*)(sm + p * AB_RS + c8 * 16) = p < T ? u[k] : (u32x4){0u, 0u, 0u, 0u};
  }
  __syncthreads();

  // ---- 2: qkv^T + bias, this wave's 144 channels x 64 tokens
#pragma unroll
  for (int ks = 0; ks < AB_KS; ++ks) {
    bf16x8 xf[4];
#pragma unroll
    for (int pt = 0; pt < 4; ++pt) xf[pt] = *(const bf16x8*)(sm + (16 * pt + lj) * AB_RS + ks * 64 + lq * 16);
#pragma unroll
    for (int tt = 0; tt < AB_NQT; ++tt)
#pragma unroll
      for (int pt = 0; pt < 4; ++pt)
        acc[tt][pt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, wr[ks][tt]), xf[pt], acc[tt][pt], 0, 0, 0);
  }
  __syncthreads();                                            // every wave has read its last `an` fragment: LDS becomes the heads' regions

  // proj's weights and bias (its accumulators start from it) and the residual travel during the attention phase
  u32x4 wpj[AB_KS][3];
#pragma unroll
  for (int ks = 0; ks < AB_KS; ++ks)
#pragma unroll
    for (int tt = 0; tt < 3; ++tt) wpj[ks][tt] = *(const u32x4*)(wp + (ks * 3 + tt) * 512);
  const unsigned short* xs = (const unsigned short*)a.x_bf16 + (size_t)b * T * AB_C;
  uint2 xr[3][4];
  f32x4 pa[3][4];
#pragma unroll
  for (int tt = 0; tt < 3; ++tt) {
    const float4 bv = *(const float4*)(a.b_proj + wv * 48 + tt * 16 + lq * 4);
#pragma unroll
    for (int pt = 0; pt < 4; ++pt) {
      const int p = 16 * pt + lj, pc = p < T ? p : T - 1;
      xr[tt][pt] = *(const uint2*)(xs + (size_t)pc * AB_C + wv * 48 + tt * 16 + lq * 4);
      pa[tt][pt] = (f32x4){bv.x, bv.y, bv.z, bv.w};
    }
  }

  // ---- 3: qkv -> the two heads' regions, q and k scaled
  {
    const float sc = 1.0f / sqrtf(sqrtf((float)AB_CH));
#pragma unroll
    for (int tt = 0; tt < AB_NQT; ++tt) {
      const int cw = 16 * tt + 4 * lq, hh = cw >= 3 * AB_CH ? 1 : 0, cc = cw - hh * 3 * AB_CH;
      const float mul = cc < 2 * AB_CH ? sc : 1.0f;
      unsigned char* dst = sm + (2 * wv + hh) * AB_HREG + cc * 4;
#pragma unroll
      for (int pt = 0; pt < 4; ++pt) {
        const f32x4 v = acc[tt][pt];
        *(float4*)(dst + (16 * pt + lj) * AB_HROW) = make_float4(v[0] * mul, v[1] * mul, v[2] * mul, v[3] * mul);
      }
    }
  }
  __syncthreads();                                            // (a region is read by the wave that wrote it, but by other lanes: ordered here)

  // ---- 4: the wave's two heads
#pragma unroll 1
  for (int hh = 0; hh < 2; ++hh) {
    unsigned char* R = sm + (2 * wv + hh) * AB_HREG;
    float kf[AB_CH / 4][4], qf[AB_CH / 4][4];
#pragma unroll
    for (int st = 0; st < AB_CH / 4; ++st)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        qf[st][i] = *(const float*)(R + (16 * i + lj) * AB_HROW + (4 * st + lq) * 4);
        kf[st][i] = *(const float*)(R + (16 * i + lj) * AB_HROW + (AB_CH + 4 * st + lq) * 4);
      }
    // the value product's A operands, requested here in one block: its k steps below are skipped wave-uniformly, and a read inside a
    // skipped-or-not step would be waited for in every step
    float vf[4][4][2];
#pragma unroll
    for (int si = 0; si < 4; ++si)
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int ci = 0; ci < 2; ++ci) {
          const int c = 16 * ci + lj < AB_CH ? 16 * ci + lj : AB_CH - 1;      // rows >= ch of the second tile: computed, never stored
          vf[si][r][ci] = *(const float*)(R + (16 * si + 4 * lq + r) * AB_HROW + (2 * AB_CH + c) * 4);
        }
    // [key tile][query tile]: row = key, column (lane & 15) = query.  The sum of a key >= T starts from -inf and stays there (finite
    // products): such a key never is the maximum and its weight is exp2(-inf) = 0 exactly, with no select per score
    f32x4 S[4][4];
#pragma unroll
    for (int si = 0; si < 4; ++si) {
      f32x4 s0;
#pragma unroll
      for (int r = 0; r < 4; ++r) s0[r] = 16 * si + 4 * lq + r < T ? 0.0f : -INFINITY;
#pragma unroll
      for (int ti = 0; ti < 4; ++ti) S[si][ti] = s0;
    }
#pragma unroll
    for (int st = 0; st < AB_CH / 4; ++st)
#pragma unroll
      for (int si = 0; si < 4; ++si)
#pragma unroll
        for (int ti = 0; ti < 4; ++ti) S[si][ti] = __builtin_amdgcn_mfma_f32_16x16x4f32(kf[st][si], qf[st][ti], S[si][ti], 0, 0, 0);

    float rz[4];
#pragma unroll
    for (int ti = 0; ti < 4; ++ti) {
      float m = -INFINITY;
#pragma unroll
      for (int si = 0; si < 4; ++si)
#pragma unroll
        for (int r = 0; r < 4; ++r) m = fmaxf(m, S[si][ti][r]);
      m = fmaxf(m, __shfl_xor(m, 16, WAVE));
      m = fmaxf(m, __shfl_xor(m, 32, WAVE));                   // (key 0 is always valid: finite)
      float z = 0.0f;
#pragma unroll
      for (int si = 0; si < 4; ++si)
#pragma unroll
        for (int r = 0; r < 4; ++r) {                           // hardware exp2, as the GroupNorm kernels' Swish: one wave per SIMD pays every vector instruction in full
          const float e = __builtin_amdgcn_exp2f((S[si][ti][r] - m) * 1.4426950408889634f);
          S[si][ti][r] = e;
          z += e;
        }
      z += __shfl_xor(z, 16, WAVE);
      z += __shfl_xor(z, 32, WAVE);
      rz[ti] = 1.0f / z;
    }

    f32x4 O[2][4];                                             // [channel tile][query tile]: row = channel, column = query
#pragma unroll
    for (int ci = 0; ci < 2; ++ci)
#pragma unroll
      for (int ti = 0; ti < 4; ++ti) O[ci][ti] = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int si = 0; si < 4; ++si)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if (16 * si + r >= T) continue;                        // (wave-uniform) the step's four keys 16 si + 4 g + r are all pad tokens: zero weights
#pragma unroll
        for (int ci = 0; ci < 2; ++ci)
#pragma unroll
          for (int ti = 0; ti < 4; ++ti) O[ci][ti] = __builtin_amdgcn_mfma_f32_16x16x4f32(vf[si][r][ci], S[si][ti][r], O[ci][ti], 0, 0, 0);
      }
#pragma unroll
    for (int ci = 0; ci < 2; ++ci) {
      const int c0 = 16 * ci + 4 * lq;
      if (c0 < AB_CH) {
#pragma unroll
        for (int ti = 0; ti < 4; ++ti) {
          const f32x4 o = O[ci][ti];
          const float r_ = rz[ti];
          *(uint2*)(R + (16 * ti + lj) * AB_HROW + c0 * 2) = make_uint2(rt_pack2(o[0] * r_, o[1] * r_), rt_pack2(o[2] * r_, o[3] * r_));
        }
      }
    }
  }
  __syncthreads();

  // ---- 5: proj (+ bias) + residual, this wave's 48 output channels
#pragma unroll
  for (int ks = 0; ks < AB_KS; ++ks) {
    constexpr int PER = AB_CH / 8;                             // 8-channel pieces per head
    const int cb = 4 * ks + lq, hd = cb / PER, off = (cb - hd * PER) * 16;
    bf16x8 xf[4];
#pragma unroll
    for (int pt = 0; pt < 4; ++pt) xf[pt] = *(const bf16x8*)(sm + hd * AB_HREG + (16 * pt + lj) * AB_HROW + off);
#pragma unroll
    for (int tt = 0; tt < 3; ++tt)
#pragma unroll
      for (int pt = 0; pt < 4; ++pt)
        pa[tt][pt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, wpj[ks][tt]), xf[pt], pa[tt][pt], 0, 0, 0);
  }
  unsigned short* out = (unsigned short*)a.out_bf16 + (size_t)b * T * AB_C;
#pragma unroll
  for (int tt = 0; tt < 3; ++tt) {
    const int n = wv * 48 + tt * 16 + lq * 4;
#pragma unroll
    for (int pt = 0; pt < 4; ++pt) {
      const int p = 16 * pt + lj;
      if (p < T) {
        const f32x4 v = pa[tt][pt];
        const uint2 r = xr[tt][pt];
        const float o0 = v[0] + __uint_as_float(r.x << 16), o1 = v[1] + __uint_as_float(r.x & 0xFFFF0000u);
        const float o2 = v[2] + __uint_as_float(r.y << 16), o3 = v[3] + __uint_as_float(r.y & 0xFFFF0000u);
        *(uint2*)(out + (size_t)p * AB_C + n) = make_uint2(rt_pack2(o0, o1), rt_pack2(o2, o3));
      }
    }
  }
}

}  // namespace
}  // namespace ctdd

using namespace ctdd;

// The attention block behind its GroupNorm as one launch (ctdd_unet.h).  Refuses (non-zero, ctdd_last_error set, nothing launched): fp32
// mode, C != 192 or heads != 8, a head width that is not a multiple of 4, T > 64, misaligned or null pointers.
extern "C" int ctdd_unet_attention_block(const void* args_, int f32, void* stream) {
  CTDD_REQUIRE(args_, CTDD_EINVAL, "ctdd_unet_attention_block: null arguments");
  const ctdd_attn_block_args& a = *(const ctdd_attn_block_args*)args_;
  CTDD_REQUIRE(f32 == 0, CTDD_ERANGE, "ctdd_unet_attention_block: bf16 inference only (the fp32 mode keeps the three launches)");
  CTDD_REQUIRE(a.B > 0 && a.T > 0 && a.C > 0 && a.heads > 0 && a.C % a.heads == 0, CTDD_EINVAL,
               "ctdd_unet_attention_block: bad shape (B=%d, T=%d, C=%d, heads=%d)", a.B, a.T, a.C, a.heads);
  CTDD_REQUIRE((a.C / a.heads) % 4 == 0, CTDD_ERANGE, "ctdd_unet_attention_block: head width %d is not a multiple of 4", a.C / a.heads);
  CTDD_REQUIRE(a.C == AB_C && a.heads == AB_HEADS, CTDD_ERANGE, "ctdd_unet_attention_block: C=%d in %d heads is off the tile (C = 192, 8 heads)", a.C,
               a.heads);
  CTDD_REQUIRE(a.T <= AB_TP, CTDD_ERANGE, "ctdd_unet_attention_block: T=%d tokens do not fit the workgroup tile (T <= 64: an LDS image within 160 KiB)",
               a.T);
  CTDD_REQUIRE(a.an_bf16 && a.x_bf16 && a.w_qkv && a.b_qkv && a.w_proj && a.b_proj && a.out_bf16, CTDD_EINVAL,
               "ctdd_unet_attention_block: null pointer");
  const uintptr_t al = (uintptr_t)a.an_bf16 | (uintptr_t)a.x_bf16 | (uintptr_t)a.w_qkv | (uintptr_t)a.b_qkv | (uintptr_t)a.w_proj |
                       (uintptr_t)a.b_proj | (uintptr_t)a.out_bf16;
  CTDD_REQUIRE((al & 15) == 0, CTDD_EINVAL, "ctdd_unet_attention_block: tensors must be 16-byte aligned");
  static_assert(AB_LDS <= 160 * 1024, "LDS image over the CU's 160 KiB");
  static bool attr_done[16] = {};
  ensure_lds_ceiling((const void*)k_attn_block, attr_done);
  hipLaunchKernelGGL(k_attn_block, dim3(a.B), dim3(AB_THREADS), (size_t)AB_LDS, (hipStream_t)stream, a);
  return finish_launch("k_attn_block");
}
