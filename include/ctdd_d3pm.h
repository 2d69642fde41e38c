/* ctdd_d3pm.h -- C ABI of the D3PM baseline kernels (csrc/d3pm.hip): the variational-bound objective with its logit
 * gradient, and one ancestral sampling step.  Conventions as in ctdd.h: device pointers, row-major, int status
 * (CTDD_OK == 0, message through ctdd_last_error), `stream` a hipStream_t.  2 <= S <= 256.  State values (x0, xt, x) outside
 * [0, S) are clamped into range by the kernels, as the other entry points of libctdd do: a range check on the host would cost a
 * device synchronisation per call. */
#ifndef CTDD_D3PM_H
#define CTDD_D3PM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of `scratch` for ctdd_d3pm_loss (two (B, D, S) fp32 operands of the matrix-core path + the fp64 row values). */
int64_t ctdd_d3pm_scratch_bytes(int B, int D, int S);

/* Per-sample D3PM losses (bits per dimension) and d loss_b / d logits[b] in one chain.
 *   logits (B, D, S) predicted x_start logits; x0, xt (B, D); t (B,) in [0, T)
 *   qprev (B, S, S) = Qbar_{max(t_b - 1, 0)}, qprevT its transpose, q1T (B, S, S) = Q_{t_b}^T  (gathered per sample)
 * Row (b, d), p = softmax(l):
 *   t_b > 0:  f1[s] = q1T[x_t][s], f2 = p @ qprev, model = log(f1 + eps) + log(f2 + eps),
 *             true = log(f1 + eps) + log(qprev[x0][:] + eps), vb = KL(softmax(true) || softmax(model))
 *   t_b == 0: vb = -log_softmax(l)[x0]
 *   ce = -log_softmax(l)[x0]
 * out_vb[b] = mean_d vb / ln 2, out_ce[b] = mean_d ce / ln 2, out_loss[b] = vb_scale out_vb[b] + ce_scale out_ce[b].
 * grad_logits (B, D, S) or NULL (values only).  S % 32 == 0: row passes around the exact-fp32 matrix-core GEMM;
 * otherwise one launch of fp32 FMA chains.  Row values are summed in fp64 by a second launch (no atomics). */
int ctdd_d3pm_loss(const float* logits, const int32_t* x0, const int32_t* xt, const int32_t* t, const float* qprev,
                   const float* qprevT, const float* q1T, int B, int D, int S, float eps, float vb_scale, float ce_scale,
                   void* scratch, float* grad_logits, float* out_loss, float* out_vb, float* out_ce, void* stream);

/* One ancestral step x_{t-1} ~ p(. | x_t) at one t for the whole batch.
 *   logits (N, D, S), x (N, D); qprev (S, S) = Qbar_{max(t - 1, 0)}, qprevT its transpose, q1T (S, S) = Q_t^T
 *   t > 0: model = log(q1T[x][:] + eps) + log(softmax(l) @ qprev + eps), out_x = argmax_s(model[s] - log(-log(u[s])))
 *   t == 0: model = l, out_x = argmax_s l[s]                              (first index on ties, both)
 * u: noise (N, D, S) clamped to [FLT_MIN, 1], or NULL: component s & 3 of Philox(seed, offset, row n D + d, s >> 2)
 * mapped to (0, 1) as ctdd_philox_uniform does.  scratch: 2 N D S floats when S % 32 == 0 (else unused, may be NULL).
 * out_logits (N, D, S) or NULL: the model logits. */
int ctdd_d3pm_step(const float* logits, const int32_t* x, const float* qprev, const float* qprevT, const float* q1T, int t,
                   int N, int D, int S, float eps, const float* noise, uint64_t seed, uint64_t offset, float* scratch,
                   int32_t* out_x, float* out_logits, void* stream);

#ifdef __cplusplus
}
#endif
#endif
