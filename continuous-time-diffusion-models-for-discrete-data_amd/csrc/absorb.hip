// absorb.hip -- absorbing-state ("masked") diffusion: forward noising (ctdd_absorb_noise), the negative ELBO with its logit
// gradient (ctdd_absorb_elbo_loss), one reverse step (ctdd_absorb_step) and the two halves of a confidence-ordered step: a candidate
// and a score per masked row (ctdd_absorb_propose, the step's layout and pick), then a per-sample top-k of the scores by radix select
// (ctdd_absorb_commit); and the terms of the held-out likelihood bounds, a row pass and a deterministic per-sample fp64 sum
// (ctdd_absorb_nll); and the step with remasking (ctdd_absorb_remask_step: the step's layout and pick, held rows, a remask coin for
// committed rows, the confidence a row committed at) with its per-sample normaliser (ctdd_absorb_remask_norm); and the two halves of
// a first-hitting step, which simulates the reverse chain event by event instead of on a time grid: with M entries masked at level
// c = 1 - alpha_t their masking levels are i.i.d. uniform on (0, c), so the next entry to unmask is uniform among them and unmasks
// at level c u^(1/M).  ctdd_absorb_hit_time counts a sample's masked rows and walks that recursion in fp64 logs (up to kmax events,
// none below the closing level) to a per-sample event count and network time; ctdd_absorb_hit_step selects that many masked rows
// uniformly (the commit's radix select, on Philox keys) and gives each the state the plain step would draw for it; and
// ctdd_absorb_filter, which tempers and truncates (top-k, top-p) the logits of the masked rows in place ahead of any of these steps.
// include/ctdd_absorb.h states the formulas, the Philox counter layouts, the key that orders the scores and the order of the sums.
//
// Loss and step are row softmaxes over a row that fits in registers.  A row is owned by a group of LPR lanes of one wave, lane j of
// the group holding the PER consecutive states PER j .. PER j + PER - 1 (float4 loads when S % 4 == 0); 64 / LPR rows per wave,
// four waves per workgroup:
//   S <= 4: LPR 1 (64 rows a wave)   S <= 16: LPR 4 (16)   S <= 64: LPR 16 (4)   S <= 256 / 512 / 1024: LPR 64, PER 4 / 8 / 16 (1)
// Every reduction and the inverse-CDF scan are shuffles inside the group.  A row is read once (maximum, sum, scan and gradient
// come from the registers) and not at all where nothing depends on it: rows without a term in the loss, rows that are not masked or
// do not unmask in the step.  The loss sum and the step's counter take one atomic per workgroup.
#include "common.hpp"
#include "../../include/ctdd_absorb.h"

namespace ctdd {

constexpr int AWV = 4;        // waves per workgroup

template <int LPR>
__device__ inline float grp_max(float v) {
#pragma unroll
  for (int m = LPR / 2; m >= 1; m >>= 1) v = fmaxf(v, __shfl_xor(v, m, WAVE));
  return v;
}
template <int LPR>
__device__ inline float grp_sum(float v) {
#pragma unroll
  for (int m = LPR / 2; m >= 1; m >>= 1) v += __shfl_xor(v, m, WAVE);
  return v;
}
template <int LPR>
__device__ inline int grp_sum_i(int v) {
#pragma unroll
  for (int m = LPR / 2; m >= 1; m >>= 1) v += __shfl_xor(v, m, WAVE);
  return v;
}

// the lane's PER states of one row, -inf past S and at the mask state; nothing is read unless `need`
template <int PER>
__device__ inline void absorb_load(const float* __restrict__ src, int S, int s0, int mask_state, bool vec, bool need, float (&v)[PER]) {
#pragma unroll
  for (int k = 0; k < PER; ++k) v[k] = -INFINITY;
  if (!need) return;
  if (vec) {                                                    // S % 4 == 0 and a 16-byte aligned base: a float4 is inside the row or past it
#pragma unroll
    for (int q = 0; q < PER / 4; ++q) {
      const int s = s0 + 4 * q;
      if (s < S) {
        const float4 t = *reinterpret_cast<const float4*>(src + s);
        v[4 * q] = t.x; v[4 * q + 1] = t.y; v[4 * q + 2] = t.z; v[4 * q + 3] = t.w;
      }
    }
  } else {
#pragma unroll
    for (int k = 0; k < PER; ++k)
      if (s0 + k < S) v[k] = src[s0 + k];
  }
#pragma unroll
  for (int k = 0; k < PER; ++k)
    if (s0 + k == mask_state) v[k] = -INFINITY;
}

template <int PER>
__device__ inline void absorb_store(float* __restrict__ dst, int S, int s0, bool vec, const float (&g)[PER]) {
  if (vec) {
#pragma unroll
    for (int q = 0; q < PER / 4; ++q) {
      const int s = s0 + 4 * q;
      if (s < S) *reinterpret_cast<float4*>(dst + s) = make_float4(g[4 * q], g[4 * q + 1], g[4 * q + 2], g[4 * q + 3]);
    }
  } else {
#pragma unroll
    for (int k = 0; k < PER; ++k)
      if (s0 + k < S) dst[s0 + k] = g[k];
  }
}

// ---------------------------------------------------------------- noising: thread i owns the entries 4 i .. 4 i + 3 (one Philox block)
__global__ __launch_bounds__(256) void k_absorb_noise(const int32_t* __restrict__ x0, const float* __restrict__ alpha, int64_t n, int D,
                                                      int mask_state, uint64_t seed, uint64_t offset, int32_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t e0 = i * 4;
  if (e0 >= n) return;
  const u4 r = philox_row(seed, offset, (uint64_t)i, 0u);
  const uint32_t w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int64_t e = e0 + c;
    if (e < n) out[e] = u01(w[c]) >= alpha[e / D] ? mask_state : x0[e];
  }
}

// ---------------------------------------------------------------- negative ELBO + logit gradient
struct AbsorbLossArgs {
  const float* logits;
  const int32_t *x0, *xt;
  const float* w;
  float nll_scale, inv_B;
  int64_t rows;
  int D, S, mask_state;
  int vec;
  double* acc;                // scratch: the fp64 sum of the call ...
  unsigned int* done;         // ... and the number of workgroups that have added to it
  float* out_loss;
  float* grad;
};

template <int LPR, int PER>
__global__ __launch_bounds__(64 * AWV) void k_absorb_loss(const AbsorbLossArgs a) {
  __shared__ double red[AWV];
  constexpr int RPW = WAVE / LPR;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, j = lane % LPR, s0 = j * PER, S = a.S, m = a.mask_state;
  const int64_t row = ((int64_t)blockIdx.x * AWV + wave) * RPW + lane / LPR;
  const bool in = row < a.rows;
  float wt = 0.0f;
  int x0 = -1;
  if (in) {
    x0 = a.x0[row];
    if (x0 != m && x0 >= 0 && x0 < S) {
      wt = a.nll_scale;
      if (a.xt[row] == m) wt += a.w[row / a.D] * a.inv_B;
    }
  }
  const bool need = wt != 0.0f;                                 // uniform over the row's group
  float v[PER], e[PER];
  absorb_load<PER>(a.logits + (size_t)(in ? row : 0) * S, S, s0, m, a.vec, need, v);
  float mx = -INFINITY;
#pragma unroll
  for (int k = 0; k < PER; ++k) mx = fmaxf(mx, v[k]);
  mx = grp_max<LPR>(mx);
  if (!(mx > -INFINITY)) mx = 0.0f;                             // rows that were not read
  float z = 0.0f, lx = 0.0f;
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    e[k] = expf(v[k] - mx);                                     // exp(-inf) = 0: the mask state and the states past S
    z += e[k];
    if (s0 + k == x0) lx = v[k] - mx;
  }
  z = grp_sum<LPR>(z);
  lx = grp_sum<LPR>(lx);
  if (in && a.grad) {
    float g[PER];
#pragma unroll
    for (int k = 0; k < PER; ++k) g[k] = need ? wt * (e[k] / z - (s0 + k == x0 ? 1.0f : 0.0f)) : 0.0f;
    absorb_store<PER>(a.grad + (size_t)row * S, S, s0, a.vec, g);
  }
  double t = (need && j == 0) ? (double)wt * (double)(logf(z) - lx) : 0.0;
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) t += __shfl_xor(t, o, WAVE);
  if (lane == 0) red[wave] = t;
  __syncthreads();
  if (threadIdx.x == 0) {
    double tot = 0.0;
#pragma unroll
    for (int i = 0; i < AWV; ++i) tot += red[i];
    atomicAdd(a.acc, tot);                                      // (device scope: performed where every XCD sees it)
    __threadfence();
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");            // the sum's add has completed before the ticket is drawn
    if (atomicAdd(a.done, 1u) == gridDim.x - 1) {               // the last workgroup: round once, leave the scratch zeroed
      __threadfence();
      const double sum = atomicAdd(a.acc, 0.0);
      a.out_loss[0] += (float)sum;
      atomicExch((unsigned long long*)a.acc, 0ull);
      atomicExch(a.done, 0u);
    }
  }
}

// ---------------------------------------------------------------- one reverse step
struct AbsorbStepArgs {
  const float* logits;
  const int32_t* x;
  int64_t rows;
  int S, mask_state;
  int vec;
  float p;
  uint32_t flags;
  uint64_t seed, offset;
  int32_t* out_x;
  int32_t* changed;
};

// The new state of a row from the registers of its group (lane j holds v, the states PER j ..): argmax_{s != m} with the lowest
// index on ties if `greedy`, else the first s whose running sum of e[s] = exp(l[s] - mx) exceeds u1 z.  The step and the proposal
// share it, so the two take the same state from the same u1.  mx: the row maximum; z: the sum of the weights (draw mode only).
template <int LPR, int PER>
__device__ inline int absorb_pick(const float (&v)[PER], int S, int m, int j, bool greedy, float u1, float& mx_out, float& z_out) {
  const int s0 = j * PER;
  float mx = -INFINITY;
  int bi = S;                                                   // the lane's first index of its maximum
#pragma unroll
  for (int k = 0; k < PER; ++k)
    if (s0 + k < S && s0 + k != m && (bi == S || v[k] > mx)) { mx = v[k]; bi = s0 + k; }
  int pick;
  if (greedy) {
#pragma unroll
    for (int o = LPR / 2; o >= 1; o >>= 1) {                    // lowest index on ties
      const float ov = __shfl_xor(mx, o, WAVE);
      const int oi = __shfl_xor(bi, o, WAVE);
      if (oi < S && (bi >= S || ov > mx || (ov == mx && oi < bi))) { mx = ov; bi = oi; }
    }
    pick = bi;
    z_out = 0.0f;
  } else {
    mx = grp_max<LPR>(mx);
    if (!(mx > -INFINITY)) mx = 0.0f;
    float c[PER], run = 0.0f;                                   // inclusive running sums of the lane's weights
#pragma unroll
    for (int k = 0; k < PER; ++k) { run += expf(v[k] - mx); c[k] = run; }
    float inc = run;                                            // inclusive scan of the lanes' totals over the group
#pragma unroll
    for (int o = 1; o < LPR; o <<= 1) {
      const float up = __shfl_up(inc, o, LPR);
      if (j >= o) inc += up;
    }
    const float before = inc - run;
    const float total = __shfl(inc, LPR - 1, LPR);
    const float target = u1 * total;
    int cnt = 0;                                                // states whose running sum is <= target: the pick is their number
#pragma unroll
    for (int k = 0; k < PER; ++k)
      if (s0 + k < S && before + c[k] <= target) ++cnt;
    pick = grp_sum_i<LPR>(cnt);
    z_out = total;
  }
  mx_out = mx;
  if (pick >= S || pick == m || pick < 0) pick = (m == S - 1) ? S - 2 : S - 1;   // target == total after rounding: the last real state
  return pick;
}

template <int LPR, int PER>
__global__ __launch_bounds__(64 * AWV) void k_absorb_step(const AbsorbStepArgs a) {
  __shared__ int red[AWV];
  constexpr int RPW = WAVE / LPR;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, j = lane % LPR, s0 = j * PER, S = a.S, m = a.mask_state;
  const int64_t row = ((int64_t)blockIdx.x * AWV + wave) * RPW + lane / LPR;
  const bool in = row < a.rows, greedy = (a.flags & CTDD_ABSORB_ARGMAX) != 0;
  const int xo = in ? a.x[row] : 0;
  bool need = in && xo == m;
  float u1 = 0.0f;
  if (need && !greedy) {
    const u4 r = philox_row(a.seed, a.offset, (uint64_t)row, 0u);
    need = u01(r.x) < a.p;
    u1 = u01(r.y);
  }
  float v[PER];
  absorb_load<PER>(a.logits + (size_t)(in ? row : 0) * S, S, s0, m, a.vec, need, v);
  float mx, z;
  const int pick = absorb_pick<LPR, PER>(v, S, m, j, greedy, u1, mx, z);
  const bool left = need;
  if (in && j == 0) a.out_x[row] = left ? pick : xo;
  if (a.changed) {
    int n = (left && j == 0) ? 1 : 0;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) n += __shfl_xor(n, o, WAVE);
    if (lane == 0) red[wave] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
      int tot = 0;
#pragma unroll
      for (int i = 0; i < AWV; ++i) tot += red[i];
      if (tot) atomicAdd(a.changed, tot);
    }
  }
}

// ---------------------------------------------------------------- confidence-ordered unmasking: candidate + score of every masked row
struct AbsorbProposeArgs {
  const float* logits;
  const int32_t* x;
  int64_t rows;
  int S, mask_state;
  int vec;
  float noise;
  uint32_t flags;
  uint64_t seed, offset;
  int32_t* out_cand;
  float* out_score;
};

template <int LPR, int PER>
__global__ __launch_bounds__(64 * AWV) void k_absorb_propose(const AbsorbProposeArgs a) {
  constexpr int RPW = WAVE / LPR;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, j = lane % LPR, s0 = j * PER, S = a.S, m = a.mask_state;
  const int64_t row = ((int64_t)blockIdx.x * AWV + wave) * RPW + lane / LPR;
  const bool in = row < a.rows, greedy = (a.flags & CTDD_ABSORB_ARGMAX) != 0;
  const bool need = in && a.x[in ? row : 0] == m;
  float u1 = 0.0f, u2 = 0.5f;
  if (need && (!greedy || a.noise != 0.0f)) {
    const u4 r = philox_row(a.seed, a.offset, (uint64_t)row, 0u);  // (r.x is the step's unmasking coin: unused here)
    u1 = u01(r.y);
    u2 = u01(r.z);
  }
  float v[PER];
  absorb_load<PER>(a.logits + (size_t)(in ? row : 0) * S, S, s0, m, a.vec, need, v);
  float mx, z;
  const int pick = absorb_pick<LPR, PER>(v, S, m, j, greedy, u1, mx, z);
  if (greedy) {                                                 // the draw's scan has summed the weights already
    z = 0.0f;
#pragma unroll
    for (int k = 0; k < PER; ++k) z += expf(v[k] - mx);
    z = grp_sum<LPR>(z);
  }
  float lc = 0.0f;                                              // l[cand] - mx: one lane of the group holds it
#pragma unroll
  for (int k = 0; k < PER; ++k)
    if (s0 + k == pick) lc = v[k] - mx;
  lc = grp_sum<LPR>(lc);
  float score = lc - logf(z);
  if (a.noise != 0.0f) score += a.noise * (-logf(-logf(u2)));
  if (need && j == 0) {
    a.out_cand[row] = pick;
    a.out_score[row] = score;
  }
}

// ---------------------------------------------------------------- confidence-ordered unmasking: per-sample top-k of the scores
// order-preserving key of a score (include/ctdd_absorb.h): NaN 0, -0 as +0, b | 0x80000000 for b >= 0, ~b for b < 0
__device__ inline uint32_t score_key(float s) {
  uint32_t b = __float_as_uint(s);
  if ((b & 0x7FFFFFFFu) > 0x7F800000u) return 0u;
  if (b == 0x80000000u) b = 0u;
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

struct AbsorbCommitArgs {
  const int32_t *x, *cand;
  const float* score;
  int D, mask_state;
  float p;
  const int32_t* counts;
  int32_t* out_x;
  int32_t* changed;
};

// Radix select over the 32-bit keys of one sample's masked rows, by a workgroup of 256 threads, most significant digit first: a pass
// histograms the digit of the masked rows whose key agrees with the digits found so far; wave 0 scans the 256 bins from the top
// (lane L owns the bins 255 - 4 L .. 252 - 4 L) for the bin that holds the need-th largest key.  After four passes `prefix` is that
// key and `need` the number of rows at it that are still wanted.  key_of(d): the key of the masked row d (recomputed in every pass);
// want_of(M): k_n from the number of masked rows, which is the first pass's total.  k_n == 0 ends after that pass, with `prefix`
// above every key.  hist: 256 bins; sel: digit, rows still wanted inside it, k_n.  Shared by k_absorb_commit and k_absorb_hit_step.
template <class KeyOf, class WantOf>
__device__ inline void radix_select(const int32_t* __restrict__ x, int D, int m, KeyOf key_of, WantOf want_of, int* hist, int* sel,
                                    uint32_t& prefix, int& need, int& kn) {
  static_assert(AWV == 4, "256 threads: one per histogram bin");
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  prefix = 0u;
  need = 0;
  kn = 0;
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 24 - 8 * pass;
    hist[tid] = 0;
    __syncthreads();
    for (int d = tid; d < D; d += 64 * AWV)
      if (x[d] == m) {
        const uint32_t key = key_of(d);
        if (pass == 0 || (key >> (shift + 8)) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1);
      }
    __syncthreads();
    if (wave == 0) {
      int h[4], s4 = 0;
#pragma unroll
      for (int c = 0; c < 4; ++c) { h[c] = hist[255 - 4 * lane - c]; s4 += h[c]; }
      int incl = s4;                                            // inclusive scan from the top bin down
#pragma unroll
      for (int o = 1; o < WAVE; o <<= 1) {
        const int up = __shfl_up(incl, o, WAVE);
        if (lane >= o) incl += up;
      }
      if (pass == 0) {                                          // the histogram's total is M_n
        need = want_of(__shfl(incl, WAVE - 1, WAVE));
        if (lane == 0) sel[2] = need;
      }
      int cum = incl - s4, digit = -1, rest = 0;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        if (digit < 0 && cum < need && need <= cum + h[c]) { digit = 255 - 4 * lane - c; rest = need - cum; }
        cum += h[c];
      }
      if (digit >= 0) { sel[0] = digit; sel[1] = rest; }         // one lane: the bins' running count passes `need` once
    }
    __syncthreads();
    kn = sel[2];
    if (kn == 0) break;                                         // (uniform) nothing to select: every masked row stays masked
    prefix = (prefix << 8) | (uint32_t)sel[0];
    need = sel[1];
  }
  if (kn == 0) { prefix = 0xFFFFFFFFu; need = 0; }              // above every key
}

// One workgroup (256 threads) per sample: the radix select above on the scores' keys.  The last pass walks d in ascending chunks
// of 256: a ballot per wave, the waves' counts through LDS (two buffers, so one barrier a chunk) and a running base put every row
// at the threshold key in its ascending-d position.
__global__ __launch_bounds__(64 * AWV) void k_absorb_commit(const AbsorbCommitArgs a) {
  __shared__ int hist[256];
  __shared__ int sel[3];                                        // digit, rows still wanted inside it, k_n
  __shared__ int wcnt[2][AWV];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, D = a.D, m = a.mask_state;
  const size_t base = (size_t)blockIdx.x * D;
  const int32_t* __restrict__ x = a.x + base;
  const float* __restrict__ sc = a.score + base;
  uint32_t prefix;
  int need, kn;
  radix_select(
      x, D, m, [&](int d) { return score_key(sc[d]); },
      [&](int M) { return a.counts ? min(M, max(0, a.counts[blockIdx.x])) : min(M, (int)ceil((double)a.p * (double)M)); }, hist, sel, prefix,
      need, kn);
  int seen = 0;                                                 // rows at the threshold key in the chunks before this one
  for (int c0 = 0, buf = 0; c0 < D; c0 += 64 * AWV, buf ^= 1) {
    const int d = c0 + tid;
    int xo = 0;
    uint32_t key = 0u;
    bool masked = false;
    if (d < D) {
      xo = x[d];
      masked = xo == m;
      if (masked) key = score_key(sc[d]);
    }
    const bool tie = masked && key == prefix;
    const unsigned long long bal = __ballot(tie);
    if (lane == 0) wcnt[buf][wave] = __popcll(bal);
    __syncthreads();
    int before = seen + __popcll(bal & ((1ull << lane) - 1ull)), all = 0;
#pragma unroll
    for (int w = 0; w < AWV; ++w) {
      const int c = wcnt[buf][w];
      if (w < wave) before += c;
      all += c;
    }
    seen += all;
    if (d < D) a.out_x[base + d] = (masked && (key > prefix || (tie && before < need))) ? a.cand[base + d] : xo;
  }
  if (tid == 0 && a.changed && kn > 0) atomicAdd(a.changed, kn);
}

// ---------------------------------------------------------------- held-out bound: per-row -log p(x0), then per-sample fp64 sums
struct AbsorbNllArgs {
  const float* logits;
  const int32_t *x0, *xt;
  int D, S, mask_state;
  int vec;
  int chunks, iters;          // workgroups per sample; row groups (of AWV * 64 / LPR rows) a workgroup walks
  float* row_nll;
  int32_t* masked;
  int32_t* hit;
};

// The row pass: k_absorb_propose's layout in argmax mode (the pick is absorb_pick's, so a hit is judged by the step's own rule).
// A row without a term is not read and stores 0.0f.  A workgroup stays inside one sample -- chunk c of sample n walks `iters`
// consecutive groups of AWV * 64 / LPR rows -- so the two counters take one integer atomic per workgroup each (integers: exact in any
// order), not one per wave or row: the counters of all samples share a few cache lines.
template <int LPR, int PER>
__global__ __launch_bounds__(64 * AWV) void k_absorb_nll_rows(const AbsorbNllArgs a) {
  __shared__ int red[2][AWV];
  constexpr int RPW = WAVE / LPR, RPB = AWV * RPW;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, j = lane % LPR, s0 = j * PER, S = a.S, m = a.mask_state;
  const int n = blockIdx.x / a.chunks, c = blockIdx.x % a.chunks;
  const int64_t base = (int64_t)n * a.D;
  int nt = 0, nh = 0;                                           // the lane's rows with a term, and the hits among them
  for (int it = 0; it < a.iters; ++it) {
    const int64_t d = ((int64_t)c * a.iters + it) * RPB + wave * RPW + lane / LPR;
    const bool in = d < a.D;
    const int64_t row = base + d;
    int x0 = -1;
    bool need = false;                                          // uniform over the row's group
    if (in) {
      x0 = a.x0[row];
      need = a.xt[row] == m && x0 != m && x0 >= 0 && x0 < S;
    }
    float v[PER];
    absorb_load<PER>(a.logits + (size_t)(in ? row : 0) * S, S, s0, m, a.vec, need, v);
    float mx, z;
    const int pick = absorb_pick<LPR, PER>(v, S, m, j, true, 0.0f, mx, z);
    if (!(mx > -INFINITY)) mx = 0.0f;                           // rows that were not read
    float lx = 0.0f;
    z = 0.0f;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      z += expf(v[k] - mx);                                     // exp(-inf) = 0: the mask state and the states past S
      if (s0 + k == x0) lx = v[k] - mx;
    }
    z = grp_sum<LPR>(z);
    lx = grp_sum<LPR>(lx);
    if (in && j == 0) a.row_nll[row] = need ? logf(z) - lx : 0.0f;
    if (need && j == 0) {
      ++nt;
      nh += pick == x0;
    }
  }
  if (a.masked || a.hit) {                                      // (uniform)
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      nt += __shfl_xor(nt, o, WAVE);
      nh += __shfl_xor(nh, o, WAVE);
    }
    if (lane == 0) { red[0][wave] = nt; red[1][wave] = nh; }
    __syncthreads();
    if (threadIdx.x == 0) {
      int t = 0, h = 0;
#pragma unroll
      for (int i = 0; i < AWV; ++i) { t += red[0][i]; h += red[1][i]; }
      if (a.masked && t) atomicAdd(a.masked + n, t);
      if (a.hit && h) atomicAdd(a.hit + n, h);
    }
  }
}

struct AbsorbNllSumArgs {
  const float* row_nll;
  const float* w;
  int D;
  double* out;
};

// One workgroup (256 threads) per sample, no atomics, the order of include/ctdd_absorb.h: thread i adds the rows d = i, i + 256, ..
// in ascending d; the 64 lanes of a wave combine by the xor butterfly 32, 16, .. 1; thread 0 adds the four waves' sums in wave order.
__global__ __launch_bounds__(64 * AWV) void k_absorb_nll_sum(const AbsorbNllSumArgs a) {
  __shared__ double red[AWV];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, D = a.D;
  const float* __restrict__ r = a.row_nll + (size_t)blockIdx.x * D;
  double t = 0.0;
  for (int d = tid; d < D; d += 64 * AWV) t += (double)r[d];
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) t += __shfl_xor(t, o, WAVE);
  if (lane == 0) red[wave] = t;
  __syncthreads();
  if (tid == 0) {
    double tot = red[0];
#pragma unroll
    for (int i = 1; i < AWV; ++i) tot += red[i];
    a.out[blockIdx.x] += (a.w ? (double)a.w[blockIdx.x] : 1.0) * tot;
  }
}

// ---------------------------------------------------------------- one reverse step with remasking
struct AbsorbRemaskArgs {
  const float* logits;
  const int32_t* x;
  const uint8_t* held;        // or nullptr
  const float* conf_in;       // or nullptr (with conf_out)
  const float* norm;          // (N, 2) or nullptr
  int64_t rows;
  int D, S, mask_state;
  int vec;
  float p, sigma, temp;
  uint32_t flags;
  uint64_t seed, offset;
  int32_t* out_x;
  float* conf_out;
  int32_t* counts;
};

// k_absorb_step's grid, row ownership, Philox block and pick, so a masked row ends where the plain step puts it.  A held row and a
// free unmasked row read no logits; an unmasked row computes its Philox block (for component 3) only when sigma > 0.  Every lane of
// a row's group reads x / held / conf_in of the row before lane 0 of the group writes the row's outputs (one wave, in program
// order): out_x == x and conf_out == conf_in are fine.
template <int LPR, int PER>
__global__ __launch_bounds__(64 * AWV) void k_absorb_remask_step(const AbsorbRemaskArgs a) {
  __shared__ int red[2][AWV];
  constexpr int RPW = WAVE / LPR;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, j = lane % LPR, s0 = j * PER, S = a.S, m = a.mask_state;
  const int64_t row = ((int64_t)blockIdx.x * AWV + wave) * RPW + lane / LPR;
  const bool in = row < a.rows, by_conf = (a.flags & CTDD_ABSORB_REMASK_CONF) != 0;
  const int xo = in ? a.x[row] : 0;
  const bool hd = in && a.held && a.held[row] != 0;
  const float ci = (in && a.conf_in) ? a.conf_in[row] : 0.0f;
  const bool masked = in && !hd && xo == m, placed = in && !hd && xo != m;   // (uniform over the row's group)
  bool need = masked, remask = false;
  float u1 = 0.0f;
  if (masked || (placed && a.sigma > 0.0f)) {
    const u4 r = philox_row(a.seed, a.offset, (uint64_t)row, 0u);
    if (masked) {
      need = u01(r.x) < a.p;
      u1 = u01(r.y);
    } else {
      float sg = a.sigma;
      if (by_conf) {
        const float U = a.norm[2 * (row / a.D)], Z = a.norm[2 * (row / a.D) + 1];
        sg = Z > 0.0f ? fminf(1.0f, ((a.sigma * U) * expf(-ci / a.temp)) / Z) : 0.0f;
      }
      remask = u01(r.w) < sg;
    }
  }
  float v[PER];
  absorb_load<PER>(a.logits + (size_t)(in ? row : 0) * S, S, s0, m, a.vec, need, v);
  float mx, z;
  const int pick = absorb_pick<LPR, PER>(v, S, m, j, false, u1, mx, z);
  float co = ci;                                                // held and kept rows: the bits that came in
  if (a.conf_out) {                                             // (uniform)
    float lc = 0.0f;                                            // l[pick] - mx: one lane of the group holds it
#pragma unroll
    for (int k = 0; k < PER; ++k)
      if (s0 + k == pick) lc = v[k] - mx;
    lc = grp_sum<LPR>(lc);
    if (masked) co = need ? expf(lc) / z : 0.0f;
    else if (remask) co = 0.0f;
  }
  if (in && j == 0) {
    a.out_x[row] = need ? pick : (remask ? m : xo);
    if (a.conf_out) a.conf_out[row] = co;
  }
  if (a.counts) {                                               // (uniform)
    int nu = (need && j == 0) ? 1 : 0, nr = (remask && j == 0) ? 1 : 0;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      nu += __shfl_xor(nu, o, WAVE);
      nr += __shfl_xor(nr, o, WAVE);
    }
    if (lane == 0) { red[0][wave] = nu; red[1][wave] = nr; }
    __syncthreads();
    if (threadIdx.x == 0) {
      int tu = 0, tr = 0;
#pragma unroll
      for (int i = 0; i < AWV; ++i) { tu += red[0][i]; tr += red[1][i]; }
      if (tu) atomicAdd(a.counts, tu);
      if (tr) atomicAdd(a.counts + 1, tr);
    }
  }
}

struct AbsorbRemaskNormArgs {
  const int32_t* x;
  const uint8_t* held;
  const float* conf;
  int D, mask_state;
  float temp;
  float* out;
};

// One workgroup (256 threads) per sample, no atomics, k_absorb_nll_sum's order: thread i adds its rows d = i, i + 256, .. in
// ascending d (the weights in fp64, the count as an integer), the xor butterfly over the wave, thread 0 adds the waves in wave order.
__global__ __launch_bounds__(64 * AWV) void k_absorb_remask_norm(const AbsorbRemaskNormArgs a) {
  __shared__ double red[AWV];
  __shared__ int cnt[AWV];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, D = a.D;
  const size_t base = (size_t)blockIdx.x * D;
  double t = 0.0;
  int u = 0;
  for (int d = tid; d < D; d += 64 * AWV)
    if (a.x[base + d] != a.mask_state && !(a.held && a.held[base + d] != 0)) {
      t += (double)expf(-a.conf[base + d] / a.temp);
      ++u;
    }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    t += __shfl_xor(t, o, WAVE);
    u += __shfl_xor(u, o, WAVE);
  }
  if (lane == 0) { red[wave] = t; cnt[wave] = u; }
  __syncthreads();
  if (tid == 0) {
    double tot = red[0];
    int n = cnt[0];
#pragma unroll
    for (int i = 1; i < AWV; ++i) { tot += red[i]; n += cnt[i]; }
    a.out[2 * (size_t)blockIdx.x] = (float)n;
    a.out[2 * (size_t)blockIdx.x + 1] = (float)tot;
  }
}

// ---------------------------------------------------------------- first-hitting sampling: per-sample event levels
struct AbsorbHitTimeArgs {
  const int32_t* x;
  const double* logc_in;
  int N, D, mask_state, kmax;
  double log_cmin;
  int t_func;
  double rate_const, alpha_eps, time_base, time_exp, t_min, t_max;
  uint64_t seed, offset;
  int32_t* counts;
  float* t_eval;
  double* logc_out;
};

// the inverse of alpha_t in fp64 (include/ctdd_absorb.h; DeviceForwardProcess.time_of_alpha states the same forms)
__device__ inline double absorb_time_of_alpha(const AbsorbHitTimeArgs& a, double al) {
  switch (a.t_func) {
    case CTDD_ABSORB_T_LOGLINEAR: return (1.0 - al) / (1.0 - a.alpha_eps);
    case CTDD_ABSORB_T_LOG_SQR: return sqrt(pow(al, -1.0 / a.rate_const) - 1.0);
    case CTDD_ABSORB_T_SQRT_COS: {
      const double r = fmin(fmax(1.0 + log(al) / a.rate_const, 0.0), 1.0);
      return (2.0 / 3.14159265358979323846) * acos(r * r);
    }
    default: return log(1.0 - log(al) / (a.rate_const * a.time_base)) / log(a.time_exp);
  }
}

// One workgroup (256 threads) per sample: the masked rows are counted by all (integers: exact in any order), then thread 0 walks the
// level recursion in fp64 -- at most kmax steps of one log and one division each, a Philox block every fourth.  M_n and the level
// never leave the device.  logc_out may be logc_in: thread 0 reads its sample's entry before it writes it.
__global__ __launch_bounds__(64 * AWV) void k_absorb_hit_time(const AbsorbHitTimeArgs a) {
  __shared__ int red[AWV];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, D = a.D, n = blockIdx.x;
  const int32_t* __restrict__ x = a.x + (size_t)n * D;
  int c = 0;
  for (int d = tid; d < D; d += 64 * AWV) c += x[d] == a.mask_state;
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) c += __shfl_xor(c, o, WAVE);
  if (lane == 0) red[wave] = c;
  __syncthreads();
  if (tid != 0) return;
  int M = 0;
#pragma unroll
  for (int i = 0; i < AWV; ++i) M += red[i];
  double L = a.logc_in[n], L1 = L;
  const int K = min(a.kmax, M);
  int acc = 0;
  u4 r = {0u, 0u, 0u, 0u};
  for (int i = 0; i < K; ++i) {
    if ((i & 3) == 0) r = philox_row(a.seed, a.offset, (uint64_t)a.N * (uint64_t)D + (uint64_t)n, (uint32_t)(i >> 2));
    const uint32_t w = (i & 3) == 0 ? r.x : (i & 3) == 1 ? r.y : (i & 3) == 2 ? r.z : r.w;
    const double Ln = L + log((double)u01(w)) / (double)(M - i);
    if (!(Ln >= a.log_cmin)) {                                  // the first refusal ends the sample
      L = a.log_cmin;
      break;
    }
    L = Ln;
    if (i == 0) L1 = Ln;
    ++acc;
  }
  a.counts[n] = acc;
  a.logc_out[n] = L;                                            // (M_n == 0: the bits that came in)
  double t = a.t_min;
  if (acc > 0) t = fmin(fmax(absorb_time_of_alpha(a, 1.0 - exp(L1)), a.t_min), a.t_max);   // (fmax / fmin drop a NaN)
  a.t_eval[n] = (float)t;
}

// ---------------------------------------------------------------- first-hitting sampling: k_n uniform rows per sample take a state
struct AbsorbHitStepArgs {
  const float* logits;
  const int32_t* x;
  const int32_t* counts;
  int D, S, mask_state;
  int vec;
  uint32_t flags;
  uint64_t seed, offset;
  int32_t* out_x;
  int32_t* changed;
};

// One workgroup (256 threads) per sample.  k_absorb_commit's radix select on the rows' Philox keys (draw 1), then its last pass
// with a second ballot: per chunk of 256 rows the rows above the threshold key and the rows at it that are still wanted are
// compacted, in ascending d, into an LDS list, and the four waves' row groups -- k_absorb_step's packing, load and pick (draw 0,
// component 1) -- walk that list.  Logits are read for the selected rows only.  out_x may be x (no __restrict__ on either): the
// select reads x before anything is written, and in the last pass a row is read by its chunk's thread before the chunk's barrier and
// written after it, by that thread (copied) or by one row group (selected), never both.
template <int LPR, int PER>
__global__ __launch_bounds__(64 * AWV) void k_absorb_hit_step(const AbsorbHitStepArgs a) {
  __shared__ int hist[256];
  __shared__ int sel[3];                                        // digit, rows still wanted inside it, k_n
  __shared__ int wcnt[2][2][AWV];                               // [buffer][above / at the threshold key][wave]
  __shared__ int list[64 * AWV];                                // the selected rows of one chunk
  constexpr int RPW = WAVE / LPR, RPB = AWV * RPW;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane % LPR, D = a.D, S = a.S, m = a.mask_state;
  const bool greedy = (a.flags & CTDD_ABSORB_ARGMAX) != 0;
  const size_t base = (size_t)blockIdx.x * D;
  const int32_t* x = a.x + base;
  int32_t* out = a.out_x + base;
  const auto key_of = [&](int d) { return philox_row(a.seed, a.offset, (uint64_t)(base + d), 1u).x; };
  uint32_t prefix;
  int need, kn;
  radix_select(x, D, m, key_of, [&](int M) { return min(M, max(0, a.counts[blockIdx.x])); }, hist, sel, prefix, need, kn);
  if (kn == 0) {                                                // (uniform) nothing moves in this sample
    if (out != x)
      for (int d = tid; d < D; d += 64 * AWV) out[d] = x[d];
    return;
  }
  int seen = 0, done = 0;                                       // rows at the threshold key / rows selected in the chunks before this one
  for (int c0 = 0, buf = 0; c0 < D; c0 += 64 * AWV, buf ^= 1) {
    if (done == kn && out == x) break;                          // (uniform) in place: the rest stays as it is
    const int d = c0 + tid;
    int xo = 0;
    uint32_t key = 0u;
    bool masked = false;
    if (d < D) {
      xo = x[d];
      masked = xo == m;
      if (masked) key = key_of(d);
    }
    const bool above = masked && key > prefix, tie = masked && key == prefix;
    const unsigned long long ba = __ballot(above), bt = __ballot(tie);
    if (lane == 0) { wcnt[buf][0][wave] = __popcll(ba); wcnt[buf][1][wave] = __popcll(bt); }
    __syncthreads();
    const unsigned long long lower = (1ull << lane) - 1ull;
    int ab = __popcll(ba & lower), tb = seen + __popcll(bt & lower), aall = 0, tall = 0;
#pragma unroll
    for (int w = 0; w < AWV; ++w) {
      const int ca = wcnt[buf][0][w], ct = wcnt[buf][1][w];
      if (w < wave) { ab += ca; tb += ct; }
      aall += ca;
      tall += ct;
    }
    const int t0 = min(seen, need);                             // rows at the threshold key taken in earlier chunks
    const bool take = above || (tie && tb < need);
    const int nsel = aall + min(seen + tall, need) - t0;        // (uniform) the chunk's selected rows
    if (d < D && !take && out != x) out[d] = xo;
    if (nsel > 0) {
      if (take) list[ab + min(tb, need) - t0] = d;              // ascending d: the selected rows before this one in the chunk
      __syncthreads();
      for (int i0 = 0; i0 < nsel; i0 += RPB) {
        const int idx = i0 + wave * RPW + lane / LPR;
        const bool have = idx < nsel;                           // (uniform over the row's group)
        const int ds = have ? list[idx] : 0;
        const size_t row = base + ds;
        float u1 = 0.0f;
        if (have && !greedy) u1 = u01(philox_row(a.seed, a.offset, (uint64_t)row, 0u).y);
        float v[PER];
        absorb_load<PER>(a.logits + row * S, S, j * PER, m, a.vec, have, v);
        float mx, z;
        const int pick = absorb_pick<LPR, PER>(v, S, m, j, greedy, u1, mx, z);
        if (have && j == 0) out[ds] = pick;
      }
    }
    seen += tall;
    done += nsel;
  }
  if (tid == 0 && a.changed) atomicAdd(a.changed, kn);
}

// ---------------------------------------------------------------- temperature, top-k and top-p (nucleus) truncation of the masked rows
struct AbsorbFilterArgs {
  const float* logits;
  const int32_t* x;
  int64_t rows;
  int S, mask_state;
  int vec;
  float temp;
  int k;                      // 0: no top-k
  float p;                    // 1: no top-p
  float* out;                 // logits itself, or a buffer that does not overlap it
};

// the number of the group's held keys that are >= t.  One row a wave with few states a lane: a ballot and a scalar popcount per
// held state; otherwise a lane count and the shuffle sum.
template <int LPR, int PER>
__device__ inline int grp_count_ge(const uint32_t (&key)[PER], uint32_t t) {
  int c = 0;
  if constexpr (LPR == WAVE && PER <= 8) {
#pragma unroll
    for (int k = 0; k < PER; ++k) c += __popcll(__ballot(key[k] >= t));
    return c;
  } else {
#pragma unroll
    for (int k = 0; k < PER; ++k) c += key[k] >= t;
    return grp_sum_i<LPR>(c);
  }
}

// the largest t with enough(t), for a predicate that holds at 0 and is monotone (true up to some key, false above it) and uniform
// over the group: 32 rounds, most significant bit first
template <class Enough>
__device__ inline uint32_t key_search(Enough enough) {
  uint32_t t = 0u;
#pragma unroll 1
  for (int b = 31; b >= 0; --b) {
    const uint32_t c = t | (1u << b);
    if (enough(c)) t = c;
  }
  return t;
}

// the number of the group's keys equal to t at lower states than the lane's first (an exclusive scan of the lanes' counts: lane j
// holds the states PER j .., so lane order is state order)
template <int LPR, int PER>
__device__ inline int grp_ties_before(const uint32_t (&key)[PER], uint32_t t, int j) {
  int n = 0;
#pragma unroll
  for (int k = 0; k < PER; ++k) n += key[k] == t;
  int inc = n;
#pragma unroll
  for (int o = 1; o < LPR; o <<= 1) {
    const int up = __shfl_up(inc, o, LPR);
    if (j >= o) inc += up;
  }
  return inc - n;
}

// k_absorb_step's grid and row ownership.  The row is held in full -- v = l / T, the key of v (score_key; 0 marks what is not or no
// longer a candidate: the mask state, the states past S, the states dropped so far) and, for top-p, the weights -- before anything is
// stored, so out may be logits.  Both selections are searches over the key's 32 bits (key_search) on a group count / a group sum, then
// an index scan over the states at the threshold key; no LDS, no sort.  The sums of top-p all go through one function of the
// threshold (mass_ge: the lane's states in ascending k, then the xor butterfly): it is monotone in the threshold, as every fp32 add
// of non-negative terms is in each operand, which is what the search needs.  A wave none of whose rows is masked returns at once.
template <int LPR, int PER>
__global__ __launch_bounds__(64 * AWV) void k_absorb_filter(const AbsorbFilterArgs a) {
  constexpr int RPW = WAVE / LPR;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, j = lane % LPR, s0 = j * PER, S = a.S, m = a.mask_state;
  const int64_t row = ((int64_t)blockIdx.x * AWV + wave) * RPW + lane / LPR;
  const bool in = row < a.rows;
  const bool need = in && a.x[in ? row : 0] == m;              // uniform over the row's group
  if (__ballot(need) == 0ull) return;                           // (uniform over the wave; the kernel has no barrier)
  const size_t at = (size_t)(in ? row : 0) * S;
  float v[PER];
  uint32_t key[PER];
  absorb_load<PER>(a.logits + at, S, s0, -1, a.vec, need, v);   // the raw row: no state is the mask state -1
  float mx = -INFINITY;
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    const int s = s0 + k;
    const bool real = s < S && s != m;
    float q = v[k] / a.temp;                                    // IEEE quotient (-fno-fast-math): T == 1 keeps the bits
    if (!(q == q)) q = -INFINITY;                               // NaN counts as -inf
    v[k] = real ? q : -INFINITY;
    key[k] = real ? score_key(v[k]) : 0u;                       // a real state's key is at least that of -inf, 0x007FFFFF
    mx = fmaxf(mx, v[k]);
  }
  mx = grp_max<LPR>(mx);
  const bool finite = mx > -INFINITY;                           // (uniform over the row's group)
  if (a.k > 0 && a.k < S - 1) {                                 // (uniform over the launch) top-k: thr is the k-th largest key
    const uint32_t thr = key_search([&](uint32_t c) { return grp_count_ge<LPR, PER>(key, c) >= a.k; });
    const int want = a.k - grp_count_ge<LPR, PER>(key, thr + 1u);      // states at thr that are kept: the lowest `want` of them
    int before = grp_ties_before<LPR, PER>(key, thr, j);
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const bool tie = key[k] == thr;
      if (key[k] < thr || (tie && before >= want)) key[k] = 0u;
      before += tie;
    }
  }
  if (a.p < 1.0f) {                                             // (uniform over the launch) top-p over the states kept so far
    const float base_mx = finite ? mx : 0.0f;
    float w[PER];
#pragma unroll
    for (int k = 0; k < PER; ++k) w[k] = key[k] != 0u ? expf(v[k] - base_mx) : 0.0f;
    const auto mass_ge = [&](uint32_t c) {
      float t = 0.0f;
#pragma unroll
      for (int k = 0; k < PER; ++k) t += key[k] >= c ? w[k] : 0.0f;
      return grp_sum<LPR>(t);
    };
    const float target = a.p * mass_ge(1u);                     // p z; fl(p z) <= z = mass_ge(0), so the search's predicate holds at 0
    const uint32_t tau = key_search([&](uint32_t c) { return mass_ge(c) >= target; });
    const float above = mass_ge(tau + 1u);                      // < target by the search: the first state at tau is always kept
    int before = grp_ties_before<LPR, PER>(key, tau, j);
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const bool tie = key[k] == tau;
      if (key[k] < tau || (tie && !(above + (float)before * w[k] < target))) key[k] = 0u;
      before += tie;
    }
  }
  if (!need) return;
  if (finite) {
#pragma unroll
    for (int k = 0; k < PER; ++k)
      if (key[k] == 0u) v[k] = -INFINITY;
    absorb_store<PER>(a.out + at, S, s0, a.vec, v);
  } else if (a.out != a.logits) {                               // no finite real-state logit: the row as it came
    absorb_load<PER>(a.logits + at, S, s0, -1, a.vec, true, v);
    absorb_store<PER>(a.out + at, S, s0, a.vec, v);
  }
}

// (LPR, PER) of a row width; rows per workgroup = AWV * 64 / LPR
#define ABSORB_SHAPE(S, CALL)                                                       \
  if ((S) <= 4) { constexpr int LPR = 1, PER = 4; CALL; }                           \
  else if ((S) <= 16) { constexpr int LPR = 4, PER = 4; CALL; }                     \
  else if ((S) <= 64) { constexpr int LPR = 16, PER = 4; CALL; }                    \
  else if ((S) <= 256) { constexpr int LPR = 64, PER = 4; CALL; }                   \
  else if ((S) <= 512) { constexpr int LPR = 64, PER = 8; CALL; }                   \
  else { constexpr int LPR = 64, PER = 16; CALL; }

static inline int absorb_lpr(int S) { return S <= 4 ? 1 : S <= 16 ? 4 : S <= 64 ? 16 : 64; }
static inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace ctdd

using namespace ctdd;

extern "C" int ctdd_absorb_noise(const int32_t* x0, const float* alpha, int B, int D, int mask_state, uint64_t seed, uint64_t offset,
                                 int32_t* out_xt, void* stream) {
  CTDD_REQUIRE(x0 && alpha && out_xt, CTDD_EINVAL, "absorb noise: null buffer");
  CTDD_REQUIRE(B > 0 && D > 0 && mask_state >= 0, CTDD_ERANGE, "absorb noise: B=%d D=%d mask_state=%d", B, D, mask_state);
  const int64_t n = (int64_t)B * D, threads = (n + 3) / 4;
  const int64_t blocks = (threads + 255) / 256;
  CTDD_REQUIRE(blocks <= INT32_MAX, CTDD_ERANGE, "absorb noise: B D = %lld entries", (long long)n);
  hipLaunchKernelGGL(k_absorb_noise, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x0, alpha, n, D, mask_state, seed, offset,
                     out_xt);
  return finish_launch("k_absorb_noise");
}

extern "C" int64_t ctdd_absorb_scratch_bytes(void) { return 16; }

extern "C" int ctdd_absorb_elbo_loss(const float* logits, const int32_t* x0, const int32_t* xt, const float* w, float nll_scale, int B,
                                     int D, int S, int mask_state, void* scratch, float* out_loss, float* grad_logits, void* stream) {
  CTDD_REQUIRE(logits && x0 && xt && w && scratch && out_loss, CTDD_EINVAL, "absorb loss: null buffer");
  CTDD_REQUIRE(B > 0 && D > 0 && S >= 2 && S <= CTDD_MAX_S && mask_state >= 0 && mask_state < S, CTDD_ERANGE,
               "absorb loss: B=%d D=%d S=%d mask_state=%d (2 <= S <= %d, 0 <= mask_state < S)", B, D, S, mask_state, CTDD_MAX_S);
  const int64_t rows = (int64_t)B * D;
  const int rpb = AWV * WAVE / absorb_lpr(S);
  const int64_t blocks = (rows + rpb - 1) / rpb;
  CTDD_REQUIRE(blocks <= INT32_MAX, CTDD_ERANGE, "absorb loss: B D = %lld rows", (long long)rows);
  const int vec = S % 4 == 0 && aligned16(logits) && (!grad_logits || aligned16(grad_logits));
  AbsorbLossArgs a = {logits, x0, xt, w, nll_scale, 1.0f / (float)B, rows, D, S, mask_state, vec,
                      (double*)scratch, (unsigned int*)((char*)scratch + 8), out_loss, grad_logits};
  ABSORB_SHAPE(S, hipLaunchKernelGGL(HIP_KERNEL_NAME(k_absorb_loss<LPR, PER>), dim3((unsigned)blocks), dim3(64 * AWV), 0, (hipStream_t)stream, a));
  return finish_launch("k_absorb_loss");
}

extern "C" int ctdd_absorb_step(const float* logits, const int32_t* x, int N, int D, int S, int mask_state, float p_unmask, uint32_t flags,
                                uint64_t seed, uint64_t offset, int32_t* out_x, int32_t* out_changed, void* stream) {
  CTDD_REQUIRE(logits && x && out_x, CTDD_EINVAL, "absorb step: null buffer");
  CTDD_REQUIRE(N > 0 && D > 0 && S >= 2 && S <= CTDD_MAX_S && mask_state >= 0 && mask_state < S, CTDD_ERANGE,
               "absorb step: N=%d D=%d S=%d mask_state=%d (2 <= S <= %d, 0 <= mask_state < S)", N, D, S, mask_state, CTDD_MAX_S);
  CTDD_REQUIRE((flags & ~CTDD_ABSORB_ARGMAX) == 0, CTDD_EINVAL, "absorb step: unknown flags %u", flags);
  const int64_t rows = (int64_t)N * D;
  const int rpb = AWV * WAVE / absorb_lpr(S);
  const int64_t blocks = (rows + rpb - 1) / rpb;
  CTDD_REQUIRE(blocks <= INT32_MAX, CTDD_ERANGE, "absorb step: N D = %lld rows", (long long)rows);
  AbsorbStepArgs a = {logits, x, rows, S, mask_state, S % 4 == 0 && aligned16(logits), p_unmask, flags, seed, offset, out_x, out_changed};
  ABSORB_SHAPE(S, hipLaunchKernelGGL(HIP_KERNEL_NAME(k_absorb_step<LPR, PER>), dim3((unsigned)blocks), dim3(64 * AWV), 0, (hipStream_t)stream, a));
  return finish_launch("k_absorb_step");
}

extern "C" int ctdd_absorb_propose(const float* logits, const int32_t* x, int N, int D, int S, int mask_state, float noise, uint32_t flags,
                                   uint64_t seed, uint64_t offset, int32_t* out_cand, float* out_score, void* stream) {
  CTDD_REQUIRE(logits && x && out_cand && out_score, CTDD_EINVAL, "absorb propose: null buffer");
  CTDD_REQUIRE(N > 0 && D > 0 && S >= 2 && S <= CTDD_MAX_S && mask_state >= 0 && mask_state < S, CTDD_ERANGE,
               "absorb propose: N=%d D=%d S=%d mask_state=%d (2 <= S <= %d, 0 <= mask_state < S)", N, D, S, mask_state, CTDD_MAX_S);
  CTDD_REQUIRE((flags & ~CTDD_ABSORB_ARGMAX) == 0, CTDD_EINVAL, "absorb propose: unknown flags %u", flags);
  CTDD_REQUIRE(noise == noise && noise - noise == 0.0f, CTDD_ERANGE, "absorb propose: noise=%g is not finite", (double)noise);
  const int64_t rows = (int64_t)N * D;
  const int rpb = AWV * WAVE / absorb_lpr(S);
  const int64_t blocks = (rows + rpb - 1) / rpb;
  CTDD_REQUIRE(blocks <= INT32_MAX, CTDD_ERANGE, "absorb propose: N D = %lld rows", (long long)rows);
  AbsorbProposeArgs a = {logits, x, rows, S, mask_state, S % 4 == 0 && aligned16(logits), noise, flags, seed, offset, out_cand, out_score};
  ABSORB_SHAPE(S, hipLaunchKernelGGL(HIP_KERNEL_NAME(k_absorb_propose<LPR, PER>), dim3((unsigned)blocks), dim3(64 * AWV), 0, (hipStream_t)stream, a));
  return finish_launch("k_absorb_propose");
}

extern "C" int ctdd_absorb_commit(const int32_t* x, const int32_t* cand, const float* score, int N, int D, int mask_state, float p_unmask,
                                  const int32_t* counts, int32_t* out_x, int32_t* out_changed, void* stream) {
  CTDD_REQUIRE(x && cand && score && out_x, CTDD_EINVAL, "absorb commit: null buffer");
  CTDD_REQUIRE(out_x != x, CTDD_EINVAL, "absorb commit: out_x aliases x");
  CTDD_REQUIRE(N > 0 && D > 0 && D <= (1 << 30) && mask_state >= 0, CTDD_ERANGE, "absorb commit: N=%d D=%d mask_state=%d (1 <= D <= 2^30)", N, D,
               mask_state);
  CTDD_REQUIRE(counts || (p_unmask >= 0.0f && p_unmask <= 1.0f), CTDD_ERANGE, "absorb commit: p_unmask=%g outside [0, 1]", (double)p_unmask);
  AbsorbCommitArgs a = {x, cand, score, D, mask_state, p_unmask, counts, out_x, out_changed};
  hipLaunchKernelGGL(k_absorb_commit, dim3((unsigned)N), dim3(64 * AWV), 0, (hipStream_t)stream, a);
  return finish_launch("k_absorb_commit");
}

extern "C" int ctdd_absorb_nll(const float* logits, const int32_t* x0, const int32_t* xt, const float* w, int N, int D, int S, int mask_state,
                               float* row_nll, double* out_nll, int32_t* out_masked, int32_t* out_hit, void* stream) {
  CTDD_REQUIRE(logits && x0 && xt && row_nll && out_nll, CTDD_EINVAL, "absorb nll: null buffer");
  CTDD_REQUIRE(N > 0 && D > 0 && D <= (1 << 30) && S >= 2 && S <= CTDD_MAX_S && mask_state >= 0 && mask_state < S, CTDD_ERANGE,
               "absorb nll: N=%d D=%d S=%d mask_state=%d (1 <= D <= 2^30, 2 <= S <= %d, 0 <= mask_state < S)", N, D, S, mask_state, CTDD_MAX_S);
  const int rpb = AWV * WAVE / absorb_lpr(S);
  const int groups = (D + rpb - 1) / rpb, iters = groups < 8 ? groups : 8;      // up to eight row groups a workgroup
  const int chunks = (int)(((int64_t)D + (int64_t)rpb * iters - 1) / ((int64_t)rpb * iters));
  const int64_t blocks = (int64_t)N * chunks;
  CTDD_REQUIRE(blocks <= INT32_MAX, CTDD_ERANGE, "absorb nll: N = %d samples of %d workgroups", N, chunks);
  AbsorbNllArgs a = {logits, x0, xt, D, S, mask_state, S % 4 == 0 && aligned16(logits), chunks, iters, row_nll, out_masked, out_hit};
  ABSORB_SHAPE(S, hipLaunchKernelGGL(HIP_KERNEL_NAME(k_absorb_nll_rows<LPR, PER>), dim3((unsigned)blocks), dim3(64 * AWV), 0, (hipStream_t)stream, a));
  if (int rc = finish_launch("k_absorb_nll_rows")) return rc;
  AbsorbNllSumArgs b = {row_nll, w, D, out_nll};
  hipLaunchKernelGGL(k_absorb_nll_sum, dim3((unsigned)N), dim3(64 * AWV), 0, (hipStream_t)stream, b);
  return finish_launch("k_absorb_nll_sum");
}

extern "C" int ctdd_absorb_remask_step(const float* logits, const int32_t* x, const uint8_t* held, const float* conf_in, const float* norm, int N,
                                       int D, int S, int mask_state, float p_unmask, float sigma, float temp, uint32_t flags, uint64_t seed,
                                       uint64_t offset, int32_t* out_x, float* conf_out, int32_t* out_counts, void* stream) {
  CTDD_REQUIRE(logits && x && out_x, CTDD_EINVAL, "absorb remask step: null buffer");
  CTDD_REQUIRE(N > 0 && D > 0 && S >= 2 && S <= CTDD_MAX_S && mask_state >= 0 && mask_state < S, CTDD_ERANGE,
               "absorb remask step: N=%d D=%d S=%d mask_state=%d (2 <= S <= %d, 0 <= mask_state < S)", N, D, S, mask_state, CTDD_MAX_S);
  CTDD_REQUIRE((flags & ~CTDD_ABSORB_REMASK_CONF) == 0, CTDD_EINVAL, "absorb remask step: flags %u (CTDD_ABSORB_REMASK_CONF or 0)", flags);
  CTDD_REQUIRE(p_unmask >= 0.0f && p_unmask <= 1.0f, CTDD_ERANGE, "absorb remask step: p_unmask=%g outside [0, 1]", (double)p_unmask);
  CTDD_REQUIRE(sigma >= 0.0f && sigma <= 1.0f, CTDD_ERANGE, "absorb remask step: sigma=%g outside [0, 1]", (double)sigma);
  CTDD_REQUIRE(temp >= 0.02f, CTDD_ERANGE, "absorb remask step: temp=%g below 0.02", (double)temp);
  CTDD_REQUIRE((conf_in != nullptr) == (conf_out != nullptr), CTDD_EINVAL, "absorb remask step: conf_in and conf_out go together");
  CTDD_REQUIRE(!(flags & CTDD_ABSORB_REMASK_CONF) || (conf_in && conf_out && norm), CTDD_EINVAL,
               "absorb remask step: CTDD_ABSORB_REMASK_CONF needs conf_in, conf_out and norm");
  const int64_t rows = (int64_t)N * D;
  const int rpb = AWV * WAVE / absorb_lpr(S);
  const int64_t blocks = (rows + rpb - 1) / rpb;
  CTDD_REQUIRE(blocks <= INT32_MAX, CTDD_ERANGE, "absorb remask step: N D = %lld rows", (long long)rows);
  AbsorbRemaskArgs a = {logits, x, held, conf_in, norm, rows, D, S, mask_state, S % 4 == 0 && aligned16(logits), p_unmask, sigma, temp, flags,
                        seed, offset, out_x, conf_out, out_counts};
  ABSORB_SHAPE(S, hipLaunchKernelGGL(HIP_KERNEL_NAME(k_absorb_remask_step<LPR, PER>), dim3((unsigned)blocks), dim3(64 * AWV), 0, (hipStream_t)stream, a));
  return finish_launch("k_absorb_remask_step");
}

extern "C" int ctdd_absorb_remask_norm(const int32_t* x, const uint8_t* held, const float* conf, int N, int D, int mask_state, float temp,
                                       float* out_norm, void* stream) {
  CTDD_REQUIRE(x && conf && out_norm, CTDD_EINVAL, "absorb remask norm: null buffer");
  CTDD_REQUIRE(N > 0 && D > 0 && D <= (1 << 24) && mask_state >= 0, CTDD_ERANGE, "absorb remask norm: N=%d D=%d mask_state=%d (1 <= D <= 2^24)", N, D,
               mask_state);
  CTDD_REQUIRE(temp >= 0.02f, CTDD_ERANGE, "absorb remask norm: temp=%g below 0.02", (double)temp);
  AbsorbRemaskNormArgs a = {x, held, conf, D, mask_state, temp, out_norm};
  hipLaunchKernelGGL(k_absorb_remask_norm, dim3((unsigned)N), dim3(64 * AWV), 0, (hipStream_t)stream, a);
  return finish_launch("k_absorb_remask_norm");
}

extern "C" int ctdd_absorb_hit_time(const int32_t* x, const double* logc_in, int N, int D, int mask_state, int kmax, double log_cmin, int t_func,
                                    double rate_const, double alpha_eps, double time_base, double time_exp, double t_min, double t_max,
                                    uint64_t seed, uint64_t offset, int32_t* out_counts, float* out_t_eval, double* logc_out, void* stream) {
  CTDD_REQUIRE(x && logc_in && out_counts && out_t_eval && logc_out, CTDD_EINVAL, "absorb hit time: null buffer");
  CTDD_REQUIRE(N > 0 && D > 0 && D <= (1 << 30) && mask_state >= 0 && kmax >= 1, CTDD_ERANGE,
               "absorb hit time: N=%d D=%d mask_state=%d kmax=%d (1 <= D <= 2^30, kmax >= 1)", N, D, mask_state, kmax);
  CTDD_REQUIRE(t_func >= CTDD_ABSORB_T_LOGLINEAR && t_func <= CTDD_ABSORB_T_LOG, CTDD_EINVAL, "absorb hit time: unknown t_func %d", t_func);
  CTDD_REQUIRE(log_cmin == log_cmin, CTDD_ERANGE, "absorb hit time: log_cmin is NaN");
  CTDD_REQUIRE(t_min <= t_max, CTDD_ERANGE, "absorb hit time: t_min=%g t_max=%g (t_min <= t_max)", t_min, t_max);
  if (t_func == CTDD_ABSORB_T_LOGLINEAR)
    CTDD_REQUIRE(alpha_eps < 1.0, CTDD_ERANGE, "absorb hit time: loglinear alpha_eps=%g (below 1)", alpha_eps);
  else
    CTDD_REQUIRE(rate_const > 0.0, CTDD_ERANGE, "absorb hit time: rate_const=%g (positive)", rate_const);
  if (t_func == CTDD_ABSORB_T_LOG)
    CTDD_REQUIRE(time_base > 0.0 && time_exp > 1.0, CTDD_ERANGE, "absorb hit time: log schedule time_base=%g time_exp=%g (positive, above 1)",
                 time_base, time_exp);
  AbsorbHitTimeArgs a = {x, logc_in, N, D, mask_state, kmax, log_cmin, t_func, rate_const, alpha_eps, time_base, time_exp, t_min, t_max,
                         seed, offset, out_counts, out_t_eval, logc_out};
  hipLaunchKernelGGL(k_absorb_hit_time, dim3((unsigned)N), dim3(64 * AWV), 0, (hipStream_t)stream, a);
  return finish_launch("k_absorb_hit_time");
}

extern "C" int ctdd_absorb_hit_step(const float* logits, const int32_t* x, const int32_t* counts, int N, int D, int S, int mask_state,
                                    uint32_t flags, uint64_t seed, uint64_t offset, int32_t* out_x, int32_t* out_changed, void* stream) {
  CTDD_REQUIRE(logits && x && counts && out_x, CTDD_EINVAL, "absorb hit step: null buffer");
  CTDD_REQUIRE(N > 0 && D > 0 && D <= (1 << 30) && S >= 2 && S <= CTDD_MAX_S && mask_state >= 0 && mask_state < S, CTDD_ERANGE,
               "absorb hit step: N=%d D=%d S=%d mask_state=%d (1 <= D <= 2^30, 2 <= S <= %d, 0 <= mask_state < S)", N, D, S, mask_state, CTDD_MAX_S);
  CTDD_REQUIRE((flags & ~CTDD_ABSORB_ARGMAX) == 0, CTDD_EINVAL, "absorb hit step: unknown flags %u", flags);
  AbsorbHitStepArgs a = {logits, x, counts, D, S, mask_state, S % 4 == 0 && aligned16(logits), flags, seed, offset, out_x, out_changed};
  ABSORB_SHAPE(S, hipLaunchKernelGGL(HIP_KERNEL_NAME(k_absorb_hit_step<LPR, PER>), dim3((unsigned)N), dim3(64 * AWV), 0, (hipStream_t)stream, a));
  return finish_launch("k_absorb_hit_step");
}

extern "C" int ctdd_absorb_filter(const float* logits, const int32_t* x, int N, int D, int S, int mask_state, float temperature, int top_k,
                                  float top_p, float* out, void* stream) {
  CTDD_REQUIRE(logits && x && out, CTDD_EINVAL, "absorb filter: null buffer");
  CTDD_REQUIRE(N > 0 && D > 0 && S >= 2 && S <= CTDD_MAX_S && mask_state >= 0 && mask_state < S, CTDD_ERANGE,
               "absorb filter: N=%d D=%d S=%d mask_state=%d (2 <= S <= %d, 0 <= mask_state < S)", N, D, S, mask_state, CTDD_MAX_S);
  CTDD_REQUIRE(temperature > 0.0f && temperature - temperature == 0.0f, CTDD_ERANGE, "absorb filter: temperature=%g (positive, finite)",
               (double)temperature);
  CTDD_REQUIRE(top_k >= 0, CTDD_ERANGE, "absorb filter: top_k=%d (0 or a count)", top_k);
  CTDD_REQUIRE(top_p > 0.0f && top_p <= 1.0f, CTDD_ERANGE, "absorb filter: top_p=%g outside (0, 1]", (double)top_p);
  const int64_t rows = (int64_t)N * D;
  const int rpb = AWV * WAVE / absorb_lpr(S);
  const int64_t blocks = (rows + rpb - 1) / rpb;
  CTDD_REQUIRE(blocks <= INT32_MAX, CTDD_ERANGE, "absorb filter: N D = %lld rows", (long long)rows);
  AbsorbFilterArgs a = {logits, x, rows, S, mask_state, S % 4 == 0 && aligned16(logits) && aligned16(out), temperature, top_k, top_p, out};
  ABSORB_SHAPE(S, hipLaunchKernelGGL(HIP_KERNEL_NAME(k_absorb_filter<LPR, PER>), dim3((unsigned)blocks), dim3(64 * AWV), 0, (hipStream_t)stream, a));
  return finish_launch("k_absorb_filter");
}
