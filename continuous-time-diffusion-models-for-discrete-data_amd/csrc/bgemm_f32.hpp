// bgemm_f32.hpp -- the exact-fp32 matrix-core batched GEMM shared by the objectives (losses.hip: K11, the reverse_prob
// log-probabilities) and the D3PM kernels (d3pm.hip).
#pragma once
#include "common.hpp"

namespace ctdd {

// ---- C_b = A_b W_b^T on the exact-fp32 matrix instruction (v_mfma_f32_32x32x2_f32): A (B, M, K), W (B, N, K), C (B, M, N)
// with K = N = 32 NT (S = 256: NT = 8).  Workgroup = 128 rows x all N of one sample, a wave = 32 rows x N (NT accumulator
// tiles); K in chunks of 16 through LDS (rows padded to 20 floats: the 16-byte fragment reads of 16 lanes cover all 64
// banks), next chunk's global loads in registers behind the current chunk's 16 NT matrix instructions per wave.  A lane half
// g contracts k = 8 g .. 8 g + 7 of the chunk: each 16-byte read feeds four instructions.
constexpr int GK = 16, GLD = GK + 4;
template <int NT>
__global__ __launch_bounds__(256) void k_bgemm_f32(const float* __restrict__ A, const float* __restrict__ W, float* __restrict__ Cm, int M, size_t sA, size_t sC,
                                                   const uint8_t* __restrict__ live) {
  constexpr int N = 32 * NT, K = N, WV = (NT + 1) / 2;              // WV: float4 of W per thread and chunk (N * 16 / 4 / 256, rounded up)
  __shared__ __attribute__((aligned(16))) float As[2][128 * GLD];
  __shared__ __attribute__((aligned(16))) float Ws[2][N * GLD];
  using f32x16l = __attribute__((ext_vector_type(16))) float;
  // live: (B, M) or null -- the masked objective's free rows.  A tile of 128 rows none of which is live has no reader for its result
  // and leaves (the whole workgroup, before any barrier).  The grid is then (samples, tiles), sample fastest: workgroups are handed
  // out in that order and a CU holds two of them, so with the tile fastest the surviving tiles of a sample started as neighbours
  // on the same CUs next to idle ones (78 us against 44 for the same tiles of a window; a prefix mask of half the rows, B = 64).
  const int b = live ? blockIdx.x : blockIdx.y, m0 = (live ? blockIdx.y : blockIdx.x) * 128;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, li = lane & 31, g = lane >> 5;
  if (live) {
    const int r = m0 + (t & 127);
    if (!__syncthreads_or(t < 128 && r < M && live[(size_t)b * M + r] != 0)) return;
  }
  const float* Ab = A + (size_t)b * sA;          // sA / sC: batch strides of A / C in floats (M K / M N when dense; a window of rows of a
                                                 // taller tensor has the taller one's).  Rows >= M are never read (zero operand) nor written.
  const float* Wb = W + (size_t)b * N * K;
  float4 pa[2], pw[WV];
  auto fetch = [&](int k0) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int idx = t + 256 * u, row = idx >> 2, c4 = (idx & 3) * 4;
      pa[u] = m0 + row < M ? *(const float4*)(Ab + (size_t)(m0 + row) * K + k0 + c4) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int u = 0; u < WV; ++u) {
      const int idx = t + 256 * u, n = idx >> 2, c4 = (idx & 3) * 4;
      pw[u] = n < N ? *(const float4*)(Wb + (size_t)n * K + k0 + c4) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  };
  auto stash = [&](int buf) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int idx = t + 256 * u, row = idx >> 2, c4 = (idx & 3) * 4;
      *(float4*)(&As[buf][row * GLD + c4]) = pa[u];
    }
#pragma unroll
    for (int u = 0; u < WV; ++u) {
      const int idx = t + 256 * u, n = idx >> 2, c4 = (idx & 3) * 4;
      if (n < N) *(float4*)(&Ws[buf][n * GLD + c4]) = pw[u];
    }
  };
  f32x16l acc[NT];
#pragma unroll
  for (int i = 0; i < NT; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[i][r] = 0.0f;
  fetch(0);
  stash(0);
  __syncthreads();
  for (int c = 0; c < K / GK; ++c) {
    const int buf = c & 1;
    if (c + 1 < K / GK) fetch((c + 1) * GK);
    const float* Aw = &As[buf][(wave * 32 + li) * GLD + 8 * g];
    const float* Ww = &Ws[buf][li * GLD + 8 * g];
#pragma unroll
    for (int s4 = 0; s4 < 2; ++s4) {
      const float4 av = *(const float4*)(Aw + 4 * s4);
#pragma unroll
      for (int i = 0; i < NT; ++i) {
        const float4 bv = *(const float4*)(Ww + (size_t)i * 32 * GLD + 4 * s4);
        acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, bv.x, acc[i], 0, 0, 0);
        acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, bv.y, acc[i], 0, 0, 0);
        acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, bv.z, acc[i], 0, 0, 0);
        acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, bv.w, acc[i], 0, 0, 0);
      }
    }
    if (c + 1 < K / GK) stash(buf ^ 1);          // (the other buffer: its readers passed the barrier of the previous chunk)
    __syncthreads();
  }
  // accumulator tile i: column 32 i + li, rows (r & 3) + 8 (r >> 2) + 4 g of the wave's 32
  float* Cb = Cm + (size_t)b * sC;
#pragma unroll
  for (int i = 0; i < NT; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = m0 + wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * g;
      if (row < M) Cb[(size_t)row * N + 32 * i + li] = acc[i][r];
    }
}

// dense operands: batch entry b = blockIdx.y of the grid (ceil(M / 128), B); S = N = K, a multiple of 32 up to 256
template <typename F>
static int launch_bgemm(int S, dim3 gg, hipStream_t st, const float* Am, const float* Wm, float* Cm, int M) {
  switch (S / 32) {
    case 1: hipLaunchKernelGGL(k_bgemm_f32<1>, gg, dim3(256), 0, st, Am, Wm, Cm, M, (size_t)M * S, (size_t)M * S, (const uint8_t*)nullptr); break;
    case 2: hipLaunchKernelGGL(k_bgemm_f32<2>, gg, dim3(256), 0, st, Am, Wm, Cm, M, (size_t)M * S, (size_t)M * S, (const uint8_t*)nullptr); break;
    case 3: hipLaunchKernelGGL(k_bgemm_f32<3>, gg, dim3(256), 0, st, Am, Wm, Cm, M, (size_t)M * S, (size_t)M * S, (const uint8_t*)nullptr); break;
    case 4: hipLaunchKernelGGL(k_bgemm_f32<4>, gg, dim3(256), 0, st, Am, Wm, Cm, M, (size_t)M * S, (size_t)M * S, (const uint8_t*)nullptr); break;
    case 5: hipLaunchKernelGGL(k_bgemm_f32<5>, gg, dim3(256), 0, st, Am, Wm, Cm, M, (size_t)M * S, (size_t)M * S, (const uint8_t*)nullptr); break;
    case 6: hipLaunchKernelGGL(k_bgemm_f32<6>, gg, dim3(256), 0, st, Am, Wm, Cm, M, (size_t)M * S, (size_t)M * S, (const uint8_t*)nullptr); break;
    case 7: hipLaunchKernelGGL(k_bgemm_f32<7>, gg, dim3(256), 0, st, Am, Wm, Cm, M, (size_t)M * S, (size_t)M * S, (const uint8_t*)nullptr); break;
    default: hipLaunchKernelGGL(k_bgemm_f32<8>, gg, dim3(256), 0, st, Am, Wm, Cm, M, (size_t)M * S, (size_t)M * S, (const uint8_t*)nullptr); break;
  }
  return finish_launch("k_bgemm_f32");
}

}  // namespace ctdd
