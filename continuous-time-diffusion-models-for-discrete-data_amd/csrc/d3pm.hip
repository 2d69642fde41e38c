// d3pm.hip -- the D3PM baseline (Austin et al. 2021; lib/d3pm.py): the variational-bound objective with its logit gradient
// (ctdd_d3pm_loss) and one ancestral sampling step (ctdd_d3pm_step).  include/ctdd_d3pm.h states the formulas.
//
// Row passes: one wave per row (b, d), four rows per workgroup; lane i owns the PER = ceil(S / 64) consecutive states
// PER i .. PER i + PER - 1, every reduction stays inside the wave.
//   S % 32 == 0   loss:  k_d3pm_softmax -> k_bgemm_f32 (f2 = P Qbar) -> k_d3pm_terms -> k_bgemm_f32 (dp = G Qbar^T) -> k_d3pm_grad
//                 step:  k_d3pm_softmax -> k_bgemm_f32 (all N D rows one batch entry) -> k_d3pm_draw
//   other S       loss:  k_d3pm_loss_fma     step:  k_d3pm_draw<., true>
//                 the two contractions as fp32 FMA chains, the table streamed through LDS once per workgroup (its four rows
//                 share the sample's table), 16 table rows a tile.
// Row values go to an fp64 buffer (rows, 2); k_d3pm_sums adds them per sample.
#include "common.hpp"
#include "bgemm_f32.hpp"
#include "../../include/ctdd_d3pm.h"

#include <float.h>

namespace ctdd {

constexpr int DRW = 4;        // rows (waves) per workgroup
constexpr int DKC = 16;       // table rows per LDS tile of the FMA chains

template <int PER>
__device__ inline void row_load(const float* __restrict__ src, int S, int lane, float fill, float (&v)[PER]) {
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    const int s = lane * PER + j;
    v[j] = s < S ? src[s] : fill;
  }
}
template <int PER>
__device__ inline void row_store(float* __restrict__ dst, int S, int lane, const float (&v)[PER]) {
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    const int s = lane * PER + j;
    if (s < S) dst[s] = v[j];
  }
}
// v (-inf on the lanes past S) -> e = exp(v - max), returns max; z = sum e
template <int PER>
__device__ inline float row_exp(const float (&v)[PER], float (&e)[PER], float& z) {
  float m = -INFINITY;
#pragma unroll
  for (int j = 0; j < PER; ++j) m = fmaxf(m, v[j]);
  m = wave_max(m);
  float acc = 0.0f;
#pragma unroll
  for (int j = 0; j < PER; ++j) { e[j] = expf(v[j] - m); acc += e[j]; }
  z = wave_sum(acc);
  return m;
}
__device__ inline int clampi(int v, int S) { return min(max(v, 0), S - 1); }

// acc[s] = sum_k p[k] tab[k][s], tab (S, S) in global memory, the same table for every wave of the workgroup.  tile: DKC S
// floats, pw: this wave's S floats.  Every thread of the workgroup calls it (barriers inside).
template <int PER>
__device__ inline void fma_contract(const float* __restrict__ tab, int S, const float (&p)[PER], float (&acc)[PER], float* tile, float* pw) {
  const int t = threadIdx.x, lane = t & 63;
  row_store<PER>(pw, S, lane, p);
#pragma unroll
  for (int j = 0; j < PER; ++j) acc[j] = 0.0f;
  for (int k0 = 0; k0 < S; k0 += DKC) {
    const int kc = min(DKC, S - k0);
    __syncthreads();                                  // the previous tile's readers are through (and pw is visible to the wave)
    for (int i = t; i < kc * S; i += 64 * DRW) tile[i] = tab[(size_t)k0 * S + i];
    __syncthreads();
    for (int k = 0; k < kc; ++k) {
      const float pk = pw[k0 + k];
#pragma unroll
      for (int j = 0; j < PER; ++j) {
        const int s = lane * PER + j;
        if (s < S) acc[j] = fmaf(pk, tile[k * S + s], acc[j]);
      }
    }
  }
}

struct D3pmArgs {
  const float* logits;
  const int32_t *x0, *xt, *t;
  const float *qprev, *qprevT, *q1T;      // (B, S, S) each
  int B, D, S;
  float eps, vbw, cew;                    // vbw = vb_scale / (D ln 2), cew = ce_scale / (D ln 2)
  float *P, *F2;                          // matrix-core path: P = softmax, later dp;  F2 = f2, later G
  double* rows;                           // (B D, 2): vb, ce of the row
  float* grad;
};

// the row's two values and G = (softmax(model) - softmax(true)) / (f2 + eps); l, f2 on the lanes' states (l = -inf past S)
template <int PER>
__device__ inline void loss_terms(const D3pmArgs& a, int b, size_t row, int lane, const float (&l)[PER], float lse, const float (&f2)[PER],
                                  float (&G)[PER]) {
  const int S = a.S, x0 = clampi(a.x0[row], S), xt = clampi(a.xt[row], S);
  const float ce = lse - a.logits[row * S + x0];
  float vb = ce;
#pragma unroll
  for (int j = 0; j < PER; ++j) G[j] = 0.0f;
  if (a.t[b] != 0) {
    float f1[PER], q0[PER], mod[PER], tru[PER], em[PER], et[PER], zm, zt;
    row_load<PER>(a.q1T + ((size_t)b * S + xt) * S, S, lane, 0.0f, f1);
    row_load<PER>(a.qprev + ((size_t)b * S + x0) * S, S, lane, 0.0f, q0);
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      const bool on = lane * PER + j < S;
      const float lf1 = logf(f1[j] + a.eps);
      mod[j] = on ? lf1 + logf(f2[j] + a.eps) : -INFINITY;
      tru[j] = on ? lf1 + logf(q0[j] + a.eps) : -INFINITY;
    }
    const float mm = row_exp<PER>(mod, em, zm), mt = row_exp<PER>(tru, et, zt);
    const float lzm = logf(zm), lzt = logf(zt);
    float kl = 0.0f;
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      if (lane * PER + j < S) {
        const float pt = et[j] / zt;
        kl += pt * (((tru[j] - mt) - lzt) - ((mod[j] - mm) - lzm));      // (x - max) first: exact for the leading states
        G[j] = (em[j] / zm - pt) / (f2[j] + a.eps);
      }
    }
    vb = wave_sum(kl);
  }
  if (lane == 0) {
    a.rows[row * 2] = (double)vb;
    a.rows[row * 2 + 1] = (double)ce;
  }
}

// d loss_b / d l of the row: vbw p (dp - <p, dp>) [t > 0] + (cew + [t == 0] vbw) (p - onehot(x0))
template <int PER>
__device__ inline void loss_grad(const D3pmArgs& a, int b, size_t row, int lane, const float (&p)[PER], const float (&dp)[PER]) {
  const int S = a.S, x0 = clampi(a.x0[row], S);
  const bool t0 = a.t[b] == 0;
  float dot = 0.0f;
#pragma unroll
  for (int j = 0; j < PER; ++j) dot += p[j] * dp[j];
  dot = wave_sum(dot);
  const float w1 = a.cew + (t0 ? a.vbw : 0.0f);
  float g[PER];
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    const int s = lane * PER + j;
    g[j] = (t0 ? 0.0f : a.vbw * (p[j] * (dp[j] - dot))) + w1 * (p[j] - (s == x0 ? 1.0f : 0.0f));
  }
  row_store<PER>(a.grad + row * S, S, lane, g);
}

// P = softmax(logits) row by row
template <int PER>
__global__ __launch_bounds__(64 * DRW) void k_d3pm_softmax(const float* __restrict__ logits, int64_t rows, int S, float* __restrict__ P) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * DRW + (threadIdx.x >> 6);
  if (row >= rows) return;
  float l[PER], e[PER], z;
  row_load<PER>(logits + (size_t)row * S, S, lane, -INFINITY, l);
  row_exp<PER>(l, e, z);
#pragma unroll
  for (int j = 0; j < PER; ++j) e[j] = e[j] / z;
  row_store<PER>(P + (size_t)row * S, S, lane, e);
}

// after f2 = P Qbar: the row values, and G over f2 (the left operand of the backward GEMM) when a gradient is wanted
template <int PER>
__global__ __launch_bounds__(64 * DRW) void k_d3pm_terms(const D3pmArgs a) {
  const int lane = threadIdx.x & 63, S = a.S;
  const int64_t row = (int64_t)blockIdx.x * DRW + (threadIdx.x >> 6);
  if (row >= (int64_t)a.B * a.D) return;
  const int b = (int)(row / a.D);
  float l[PER], e[PER], f2[PER], G[PER], z;
  row_load<PER>(a.logits + (size_t)row * S, S, lane, -INFINITY, l);
  const float m = row_exp<PER>(l, e, z);
  row_load<PER>(a.F2 + (size_t)row * S, S, lane, 0.0f, f2);
  loss_terms<PER>(a, b, (size_t)row, lane, l, m + logf(z), f2, G);
  if (a.grad) row_store<PER>(a.F2 + (size_t)row * S, S, lane, G);
}

// after dp = G Qbar^T (in a.P): the logit gradient
template <int PER>
__global__ __launch_bounds__(64 * DRW) void k_d3pm_grad(const D3pmArgs a) {
  const int lane = threadIdx.x & 63, S = a.S;
  const int64_t row = (int64_t)blockIdx.x * DRW + (threadIdx.x >> 6);
  if (row >= (int64_t)a.B * a.D) return;
  float l[PER], p[PER], dp[PER], z;
  row_load<PER>(a.logits + (size_t)row * S, S, lane, -INFINITY, l);
  row_exp<PER>(l, p, z);
#pragma unroll
  for (int j = 0; j < PER; ++j) p[j] = p[j] / z;
  row_load<PER>(a.P + (size_t)row * S, S, lane, 0.0f, dp);
  loss_grad<PER>(a, (int)(row / a.D), (size_t)row, lane, p, dp);
}

// any S <= 256 in one launch.  grid (ceil(D / DRW), B): the rows of a workgroup share sample b and its tables.
template <int PER>
__global__ __launch_bounds__(64 * DRW) void k_d3pm_loss_fma(const D3pmArgs a) {
  __shared__ float tile[DKC * 256];
  __shared__ float pws[DRW][256];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, S = a.S, b = blockIdx.y;
  const int d = blockIdx.x * DRW + wave;
  const bool valid = d < a.D;                                   // a wave past D works on the last row and writes nothing
  const size_t row = (size_t)b * a.D + (valid ? d : a.D - 1);
  const bool t0 = a.t[b] == 0;                                  // uniform over the workgroup
  float l[PER], p[PER], f2[PER], G[PER], dp[PER], z;
  row_load<PER>(a.logits + row * S, S, lane, -INFINITY, l);
  const float m = row_exp<PER>(l, p, z);
#pragma unroll
  for (int j = 0; j < PER; ++j) { p[j] = p[j] / z; f2[j] = 0.0f; dp[j] = 0.0f; }
  if (!t0) fma_contract<PER>(a.qprev + (size_t)b * S * S, S, p, f2, tile, pws[wave]);
  if (valid) loss_terms<PER>(a, b, row, lane, l, m + logf(z), f2, G);
  if (!a.grad) return;
  if (!t0) {
    if (!valid) {
#pragma unroll
      for (int j = 0; j < PER; ++j) G[j] = 0.0f;
    }
    fma_contract<PER>(a.qprevT + (size_t)b * S * S, S, G, dp, tile, pws[wave]);
  }
  if (valid) loss_grad<PER>(a, b, row, lane, p, dp);
}

// per-sample sums of the row values: one workgroup per sample
__global__ __launch_bounds__(256) void k_d3pm_sums(const double* __restrict__ rows, int D, float vb_scale, float ce_scale,
                                                   float* __restrict__ out_loss, float* __restrict__ out_vb, float* __restrict__ out_ce) {
  __shared__ double red[2][256];
  const int b = blockIdx.x, t = threadIdx.x;
  double s0 = 0.0, s1 = 0.0;
  for (int d = t; d < D; d += 256) {
    const double* r = rows + ((size_t)b * D + d) * 2;
    s0 += r[0]; s1 += r[1];
  }
  red[0][t] = s0; red[1][t] = s1;
  __syncthreads();
  for (int o = 128; o >= 1; o >>= 1) {
    if (t < o) { red[0][t] += red[0][t + o]; red[1][t] += red[1][t + o]; }
    __syncthreads();
  }
  if (t == 0) {
    const double k = 1.0 / ((double)D * 0.6931471805599453), vb = red[0][0] * k, ce = red[1][0] * k;
    out_vb[b] = (float)vb;
    out_ce[b] = (float)ce;
    out_loss[b] = (float)((double)vb_scale * vb + (double)ce_scale * ce);
  }
}

struct D3pmStepArgs {
  const float* logits;
  const int32_t* x;
  const float *qprev, *q1T;               // (S, S) each
  int t;
  int64_t rows;
  int S;
  float eps;
  const float* noise;
  uint64_t seed, offset;
  const float* F2;                        // matrix-core path: f2 of every row
  int32_t* out_x;
  float* out_logits;
};

// model logits of the row and the Gumbel-max draw.  FMA: softmax and the contraction here (any S); otherwise f2 is read.
template <int PER, bool FMA>
__global__ __launch_bounds__(64 * DRW) void k_d3pm_draw(const D3pmStepArgs a) {
  __shared__ float tile[FMA ? DKC * 256 : 1];
  __shared__ float pws[FMA ? DRW : 1][FMA ? 256 : 1];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, S = a.S;
  const int64_t r0 = (int64_t)blockIdx.x * DRW + wave;
  const bool valid = r0 < a.rows;
  if (!FMA && !valid) return;
  const size_t row = (size_t)(valid ? r0 : a.rows - 1);
  float v[PER], f2[PER];
  row_load<PER>(a.logits + row * S, S, lane, -INFINITY, v);
  if (a.t != 0) {
    if (FMA) {
      float p[PER], z;
      row_exp<PER>(v, p, z);
#pragma unroll
      for (int j = 0; j < PER; ++j) p[j] = p[j] / z;
      fma_contract<PER>(a.qprev, S, p, f2, tile, pws[wave]);
    } else {
      row_load<PER>(a.F2 + row * S, S, lane, 0.0f, f2);
    }
    float f1[PER];
    row_load<PER>(a.q1T + (size_t)clampi(a.x[row], S) * S, S, lane, 0.0f, f1);
#pragma unroll
    for (int j = 0; j < PER; ++j) v[j] = lane * PER + j < S ? logf(f1[j] + a.eps) + logf(f2[j] + a.eps) : -INFINITY;
  }
  if (!valid) return;
  if (a.out_logits) row_store<PER>(a.out_logits + row * S, S, lane, v);
  float best = -INFINITY;
  int bi = S;
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    const int s = lane * PER + j;
    if (s >= S) continue;
    float w = v[j];
    if (a.t != 0) {
      float u;
      if (a.noise) {
        u = fminf(fmaxf(a.noise[row * S + s], FLT_MIN), 1.0f);
      } else {
        const u4 r = philox_row(a.seed, a.offset, (uint64_t)row, (uint32_t)(s >> 2));
        const int c = s & 3;
        u = u01(c == 0 ? r.x : c == 1 ? r.y : c == 2 ? r.z : r.w);
      }
      w = w - logf(-logf(u));
    }
    if (w > best || bi == S) { best = w; bi = s; }
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {                            // first index on ties
    const float ov = __shfl_xor(best, o, WAVE);
    const int oi = __shfl_xor(bi, o, WAVE);
    if (oi < S && (bi >= S || ov > best || (ov == best && oi < bi))) { best = ov; bi = oi; }
  }
  if (lane == 0) a.out_x[row] = bi < S ? bi : 0;
}

#define D3PM_PER(S, CALL)            \
  switch (((S) + 63) / 64) {         \
    case 1: { constexpr int PER = 1; CALL; } break; \
    case 2: { constexpr int PER = 2; CALL; } break; \
    case 3: { constexpr int PER = 3; CALL; } break; \
    default: { constexpr int PER = 4; CALL; } break; \
  }

}  // namespace ctdd

using namespace ctdd;

static inline size_t d3pm_align(size_t n) { return (n + 255) & ~(size_t)255; }

extern "C" int64_t ctdd_d3pm_scratch_bytes(int B, int D, int S) {
  if (B <= 0 || D <= 0 || S <= 0) return 0;
  const size_t n = (size_t)B * D * S;
  return (int64_t)(2 * d3pm_align(n * sizeof(float)) + d3pm_align((size_t)B * D * 2 * sizeof(double)));
}

extern "C" int ctdd_d3pm_loss(const float* logits, const int32_t* x0, const int32_t* xt, const int32_t* t, const float* qprev,
                              const float* qprevT, const float* q1T, int B, int D, int S, float eps, float vb_scale, float ce_scale,
                              void* scratch, float* grad_logits, float* out_loss, float* out_vb, float* out_ce, void* stream) {
  CTDD_REQUIRE(logits && x0 && xt && t && qprev && qprevT && q1T && scratch && out_loss && out_vb && out_ce, CTDD_EINVAL, "d3pm loss: null buffer");
  CTDD_REQUIRE(B > 0 && B <= 65535 && D > 0 && S >= 2 && S <= 256, CTDD_ERANGE, "d3pm loss: B=%d D=%d S=%d (B <= 65535, 2 <= S <= 256)", B, D, S);
  hipStream_t st = (hipStream_t)stream;
  const size_t n = (size_t)B * D * S;
  char* base = (char*)scratch;
  D3pmArgs a = {logits, x0, xt, t, qprev, qprevT, q1T, B, D, S, eps,
                (float)((double)vb_scale / ((double)D * 0.6931471805599453)), (float)((double)ce_scale / ((double)D * 0.6931471805599453)),
                (float*)base, (float*)(base + d3pm_align(n * sizeof(float))), (double*)(base + 2 * d3pm_align(n * sizeof(float))), grad_logits};
  const int64_t rows = (int64_t)B * D;
  const unsigned rb = (unsigned)((rows + DRW - 1) / DRW);
  if (S % 32 == 0) {
    const dim3 gg((D + 127) / 128, B);
    D3PM_PER(S, hipLaunchKernelGGL(k_d3pm_softmax<PER>, dim3(rb), dim3(64 * DRW), 0, st, logits, rows, S, a.P));
    if (int rc = finish_launch("k_d3pm_softmax")) return rc;
    if (int rc = launch_bgemm<void>(S, gg, st, a.P, qprevT, a.F2, D)) return rc;            // f2[row][s] = sum_k P[row][k] qprevT[s][k]
    D3PM_PER(S, hipLaunchKernelGGL(k_d3pm_terms<PER>, dim3(rb), dim3(64 * DRW), 0, st, a));
    if (int rc = finish_launch("k_d3pm_terms")) return rc;
    if (grad_logits) {
      if (int rc = launch_bgemm<void>(S, gg, st, a.F2, qprev, a.P, D)) return rc;           // dp[row][k] = sum_s G[row][s] qprev[k][s]
      D3PM_PER(S, hipLaunchKernelGGL(k_d3pm_grad<PER>, dim3(rb), dim3(64 * DRW), 0, st, a));
      if (int rc = finish_launch("k_d3pm_grad")) return rc;
    }
  } else {
    D3PM_PER(S, hipLaunchKernelGGL(k_d3pm_loss_fma<PER>, dim3((D + DRW - 1) / DRW, B), dim3(64 * DRW), 0, st, a));
    if (int rc = finish_launch("k_d3pm_loss_fma")) return rc;
  }
  hipLaunchKernelGGL(k_d3pm_sums, dim3(B), dim3(256), 0, st, (const double*)a.rows, D, vb_scale, ce_scale, out_loss, out_vb, out_ce);
  return finish_launch("k_d3pm_sums");
}

extern "C" int ctdd_d3pm_step(const float* logits, const int32_t* x, const float* qprev, const float* qprevT, const float* q1T, int t,
                              int N, int D, int S, float eps, const float* noise, uint64_t seed, uint64_t offset, float* scratch,
                              int32_t* out_x, float* out_logits, void* stream) {
  CTDD_REQUIRE(logits && x && qprev && qprevT && q1T && out_x, CTDD_EINVAL, "d3pm step: null buffer");
  CTDD_REQUIRE(N > 0 && D > 0 && S >= 2 && S <= 256 && t >= 0, CTDD_ERANGE, "d3pm step: N=%d D=%d S=%d t=%d (2 <= S <= 256)", N, D, S, t);
  const int64_t rows = (int64_t)N * D;
  CTDD_REQUIRE(rows <= INT32_MAX, CTDD_ERANGE, "d3pm step: N D = %lld rows", (long long)rows);
  hipStream_t st = (hipStream_t)stream;
  const unsigned rb = (unsigned)((rows + DRW - 1) / DRW);
  D3pmStepArgs a = {logits, x, qprev, q1T, t, rows, S, eps, noise, seed, offset, nullptr, out_x, out_logits};
  if (S % 32 == 0) {
    if (t != 0) {
      CTDD_REQUIRE(scratch, CTDD_EINVAL, "d3pm step: the matrix-core path needs scratch");
      float* P = scratch;
      float* F2 = scratch + (size_t)rows * S;
      D3PM_PER(S, hipLaunchKernelGGL(k_d3pm_softmax<PER>, dim3(rb), dim3(64 * DRW), 0, st, logits, rows, S, P));
      if (int rc = finish_launch("k_d3pm_softmax")) return rc;
      if (int rc = launch_bgemm<void>(S, dim3((unsigned)((rows + 127) / 128), 1), st, P, qprevT, F2, (int)rows)) return rc;
      a.F2 = F2;
    }
    D3PM_PER(S, hipLaunchKernelGGL(HIP_KERNEL_NAME(k_d3pm_draw<PER, false>), dim3(rb), dim3(64 * DRW), 0, st, a));
  } else {
    D3PM_PER(S, hipLaunchKernelGGL(HIP_KERNEL_NAME(k_d3pm_draw<PER, true>), dim3(rb), dim3(64 * DRW), 0, st, a));
  }
  return finish_launch("k_d3pm_draw");
}
