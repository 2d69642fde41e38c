/* ctdd_absorb.h -- C ABI of the absorbing-state ("masked") diffusion kernels (csrc/absorb.hip): forward noising, the negative
 * ELBO with its logit gradient, one reverse (unmasking) step, the two halves of a confidence-ordered unmasking step
 * (ctdd_absorb_propose, ctdd_absorb_commit), the per-sample terms of the held-out likelihood bounds (ctdd_absorb_nll), and the
 * reverse step with remasking and its per-sample normaliser (ctdd_absorb_remask_step, ctdd_absorb_remask_norm), and the two halves
 * of a first-hitting step (ctdd_absorb_hit_time, ctdd_absorb_hit_step), and the temperature / top-k / top-p truncation of the
 * masked rows' logits that any of the steps may be given (ctdd_absorb_filter).
 * Conventions as in ctdd.h: device pointers, row-major, int status (CTDD_OK == 0, message through ctdd_last_error), `stream` a
 * hipStream_t.  Logits fp32 (B, D, S) contiguous, states int32,
 * 2 <= S <= CTDD_MAX_S (S counts the mask state: S = 2 is one real state plus the mask), 0 <= mask_state < S.
 *
 * The process: with alpha_t = exp(-c(t)) the probability that an entry is still unmasked at t, an entry of x_t is mask_state with
 * probability 1 - alpha_t and x0 otherwise, independently.  No S x S table enters any of the kernels.
 *
 * Softmax excluding the mask state (every softmax below): over the states s != m = mask_state only.  l[m] takes no part in the
 * row maximum, its weight is exactly 0 and its gradient entry is exactly 0:
 *   mx = max_{s != m} l[s],  e[s] = exp(l[s] - mx) (e[m] = 0),  z = sum_s e[s],  lp[s] = (l[s] - mx) - log z.
 * Rows are packed 64, 16, 4 or 1 to a wave (S <= 4, 16, 64, above); every row is read once, and not at all where it carries no
 * term (loss) or does not move (step). */
#ifndef CTDD_ABSORB_H
#define CTDD_ABSORB_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CTDD_ABSORB_ARGMAX 1u   /* ctdd_absorb_step / _propose: every masked row takes argmax_{s != m} l[s] (lowest index on ties), no draw */

/* x_t[b][d] = mask_state iff u >= alpha[b], else x0[b][d].   x0, out_xt (B, D); alpha (B,) on the device.
 * u: one Philox uniform per entry.  Entry e = b D + d reads component (e & 3) of the block Philox(key = seed,
 * counter = (row = e >> 2, offset, draw = 0)), mapped to (0, 1) as ctdd_philox_uniform does: the uniforms of the call are
 * ctdd_philox_uniform(seed, offset, ceil(B D / 4), 1) read in row-major order. */
int ctdd_absorb_noise(const int32_t* x0, const float* alpha, int B, int D, int mask_state, uint64_t seed, uint64_t offset,
                      int32_t* out_xt, void* stream);

/* Bytes of `scratch` for ctdd_absorb_elbo_loss.  The caller zeroes it once; a call leaves it zeroed. */
int64_t ctdd_absorb_scratch_bytes(void);

/* Negative ELBO (a weighted masked cross entropy) and d loss / d logits.   x0, xt (B, D); w (B,) on the device.
 *   loss = (1/B) sum_b w[b] sum_{d: xt[b][d] == m, x0[b][d] != m} -lp[b][d][x0]  +  nll_scale sum_{(b,d): x0 != m} -lp[b][d][x0]
 * Row (b, d) has the weight wt = [xt == m] w[b] / B + nll_scale if x0 != m (and x0 in [0, S)), else 0:
 *   grad[b][d][s] = wt (e[s] / z - [s == x0]);   a row with wt == 0 is not read and its gradient row is exact zeros.
 * *out_loss += loss (row terms are summed in fp64: one fp64 atomic per workgroup into `scratch`, the last workgroup rounds once).
 * grad_logits (B, D, S) is written full shape, or NULL (value only). */
int ctdd_absorb_elbo_loss(const float* logits, const int32_t* x0, const int32_t* xt, const float* w, float nll_scale, int B, int D,
                          int S, int mask_state, void* scratch, float* out_loss, float* grad_logits, void* stream);

/* One reverse step for N D rows.   logits (N, D, S), x, out_x (N, D).
 *   x != m: out_x = x, bit for bit; the row's logits are not read.
 *   x == m: the row r = n D + d reads ONE block Philox(key = seed, counter = (row = r, offset, draw = 0)):
 *     component 0: u0 -- the row unmasks iff u0 < p_unmask (else out_x = m; the logits are not read);
 *     component 1: u1 -- the new state, by inverse CDF over the weights e[s] of the softmax excluding the mask state:
 *                  the first s whose running sum e[0] + .. + e[s] exceeds u1 z.  Never m.
 *   flags & CTDD_ABSORB_ARGMAX: every masked row takes argmax_{s != m} l[s], lowest index on ties; no draw, p_unmask unused.
 * out_changed (int32[1] or NULL) += the number of rows that left the mask state (one atomic per workgroup). */
int ctdd_absorb_step(const float* logits, const int32_t* x, int N, int D, int S, int mask_state, float p_unmask, uint32_t flags,
                     uint64_t seed, uint64_t offset, int32_t* out_x, int32_t* out_changed, void* stream);

/* Confidence-ordered unmasking, first half: a candidate state and a confidence score for every masked row.
 *   logits (N, D, S), x (N, D); out_cand int32 (N, D), out_score fp32 (N, D).
 *   x != m: the row's logits are not read and nothing is written for it (out_cand / out_score keep what they held).
 *   x == m: the row r = n D + d reads ONE block Philox(key = seed, counter = (row = r, offset, draw = 0)), laid out as the step's:
 *     component 0: unused (the step's unmasking coin), so that component 1 is the step's;
 *     component 1: u1 -- the candidate, by the inverse-CDF rule of ctdd_absorb_step (the same device code): for the same
 *                  (seed, offset) the candidate IS the state ctdd_absorb_step would draw for the row.  Never m.
 *     component 2: u2 -- the ranking noise, read only when noise != 0.
 *   flags & CTDD_ABSORB_ARGMAX: the candidate is argmax_{s != m} l[s], lowest index on ties (u1 unused).
 *   score = lp[cand] = (l[cand] - mx) - log z   (the softmax excluding the mask state, above),
 *           + noise * (-log(-log u2))             when noise != 0 (a standard Gumbel variate scaled by `noise`). */
int ctdd_absorb_propose(const float* logits, const int32_t* x, int N, int D, int S, int mask_state, float noise, uint32_t flags,
                        uint64_t seed, uint64_t offset, int32_t* out_cand, float* out_score, void* stream);

/* Confidence-ordered unmasking, second half: per sample, the k_n masked rows with the largest score take their candidate.
 *   x, cand, out_x int32 (N, D); score fp32 (N, D); out_x does not alias x.  One workgroup per sample, 1 <= D <= 2^30.
 *   M_n = the number of rows d of sample n with x[n][d] == m.  The number of rows to commit:
 *     counts != NULL (int32 (N,) on the device): k_n = min(M_n, max(0, counts[n]));
 *     counts == NULL: k_n = min(M_n, (int)ceil((double)p_unmask * M_n)), 0 <= p_unmask <= 1 (CTDD_ERANGE otherwise; p_unmask is
 *                     unused when counts is given).  The fp64 product of an fp32 and an int below 2^29 is exact: the host can restate k_n.
 *   x != m: out_x = x, bit for bit; cand and score are not read there.
 *   x == m: out_x = cand for the k_n rows first in the order below, m for the others.
 *   Order: descending by the 32-bit key of the score, equal keys in ascending d.  With b the score's bits:
 *     NaN (either sign)            key = 0            (below -inf)
 *     -0                           counts as +0       (b = 0)
 *     sign bit clear (+0 .. +inf)  key = b | 0x80000000
 *     sign bit set   (-inf .. <0)  key = ~b
 *   so key(a) < key(b) iff a < b for all non-NaN a, b, and -inf has the key 0x007FFFFF.
 *   Selection is a radix select over the key: four passes of 8-bit digit histograms (256 LDS bins), most significant digit first,
 *   find the key T of the k_n-th row and how many rows at T are still wanted; one pass over d in ascending chunks of 256 (ballots
 *   and prefix counts) then takes every key > T and exactly that many of the rows at T.  Keys are recomputed from `score` in each
 *   pass (4 bytes a row, from L2); nothing but the histogram is kept in LDS, so D has no bound set by it.
 * out_changed (int32[1] or NULL) += sum_n k_n (one atomic per workgroup). */
int ctdd_absorb_commit(const int32_t* x, const int32_t* cand, const float* score, int N, int D, int mask_state, float p_unmask,
                       const int32_t* counts, int32_t* out_x, int32_t* out_changed, void* stream);

/* Per-row and per-sample negative log-likelihood of x0 at the masked rows of x_t: the terms of the held-out likelihood bounds.
 *   logits (N, D, S), x0, xt (N, D); w (N,) on the device or NULL (every weight 1).
 *   Row (n, d) carries a term iff xt == m, x0 != m and 0 <= x0 < S:
 *     row_nll[n][d] = log z - (l[x0] - mx)   (the softmax excluding the mask state, above; fp32)
 *   Every other row's logits are not read and its row_nll is stored as exact 0.0f.  row_nll (N, D) is written in full.
 *   out_nll[n]    += (double)w[n] * sum_d row_nll[n][d]                                    (fp64 (N,))
 *   out_masked[n] += the number of rows of sample n that carry a term                      (int32 (N,) or NULL)
 *   out_hit[n]    += the number of those whose argmax_{s != m} l[s], lowest index on ties (ctdd_absorb_step's rule), is x0  (or NULL)
 * The sum is deterministic: no floating-point atomic enters it, and repeated calls on the same inputs add the same bits.  Two
 * launches: the row pass (rows packed as above inside one sample: a workgroup walks up to eight groups of 256 / LPR rows of its sample
 * and sends one integer atomic per counter -- integers are exact in any order), then one
 * workgroup of 256 threads per sample in this order: thread i adds row_nll[n][d] for d = i, i + 256, i + 512, .. in ascending d,
 * in fp64; the 64 lanes of a wave combine by the xor butterfly with the offsets 32, 16, 8, 4, 2, 1; the four waves' sums are added in
 * wave order 0, 1, 2, 3; the total is multiplied by w[n] and added to out_nll[n] by that workgroup's one thread.  Nothing of a sample
 * is kept in LDS but the four wave sums: 1 <= D <= 2^30. */
int ctdd_absorb_nll(const float* logits, const int32_t* x0, const int32_t* xt, const float* w, int N, int D, int S, int mask_state,
                    float* row_nll, double* out_nll, int32_t* out_masked, int32_t* out_hit, void* stream);

/* One reverse step with remasking (ReMDM-style) for N D rows: ctdd_absorb_step's grid and row ownership, plus held rows, a remask
 * coin for the committed rows and an optional record of the confidence at which a row committed.
 *   logits (N, D, S), x, out_x int32 (N, D); held uint8 (N, D) or NULL (non-zero = held; NULL: nothing is held);
 *   conf_in, conf_out fp32 (N, D), both given or both NULL; norm fp32 (N, 2) or NULL (ctdd_absorb_remask_norm's output).
 *   0 <= p_unmask, sigma <= 1; temp >= 0.02; flags: CTDD_ABSORB_REMASK_CONF or 0 (CTDD_ABSORB_ARGMAX is refused: CTDD_EINVAL).
 * The row r = n D + d reads ONE block Philox(key = seed, counter = (row = r, offset, draw = 0)), laid out as ctdd_absorb_step's:
 *     component 0: u0 -- the unmask coin of a masked row            (ctdd_absorb_step's)
 *     component 1: u1 -- the state draw of a row that unmasks        (ctdd_absorb_step's, the same device code)
 *     component 2: unused here (ctdd_absorb_propose's ranking noise)
 *     component 3: u3 -- the remask coin of a free unmasked row
 *   held row (held[r] != 0, whatever x is): out_x = x and conf_out = conf_in, bit for bit; no draw, the logits are not read.
 *   masked row (x == m, not held): ctdd_absorb_step's rule with p_unmask -- for the same (seed, offset, p_unmask) out_x IS what
 *     ctdd_absorb_step writes.  If it unmasks, conf_out = exp(l[out_x] - mx) / z, the probability of the state written under the
 *     softmax excluding the mask state (above), in (0, 1]; if it stays masked, conf_out = 0 and the logits are not read.
 *   free unmasked row (x != m, not held): remasked iff u3 < sigma_row; the logits are never read.
 *     flags == 0:                       sigma_row = sigma
 *     flags & CTDD_ABSORB_REMASK_CONF:  sigma_row = min(1, ((sigma U_n) exp(-conf_in / temp)) / Z_n) in fp32, (U_n, Z_n) = norm[n]
 *                                       (0 where Z_n is not positive); needs conf_in, conf_out and norm (CTDD_EINVAL otherwise).
 *       The weights exp(-conf / temp) lie in [exp(-1 / temp), 1] for conf in [0, 1] (a normal fp32 for temp >= 0.02), so the mean
 *       sigma_row over the free unmasked rows of a sample is sigma whenever no row clamps at 1, e.g. for sigma <= exp(-1 / temp).
 *     remasked: out_x = m, conf_out = 0.   kept: out_x = x, conf_out = conf_in, bit for bit.
 *   sigma == 0: no Philox block is computed for an unmasked row; the call costs what ctdd_absorb_step costs.
 * out_x may be x and conf_out may be conf_in (in place): a row reads and writes its own entries only.
 * out_counts (int32[2] or NULL): [0] += the rows that left the mask state, [1] += the rows remasked (one atomic per workgroup each). */
#define CTDD_ABSORB_REMASK_CONF 2u   /* ctdd_absorb_remask_step: the remask probability of a row follows the confidence it committed at */
int ctdd_absorb_remask_step(const float* logits, const int32_t* x, const uint8_t* held, const float* conf_in, const float* norm, int N, int D,
                            int S, int mask_state, float p_unmask, float sigma, float temp, uint32_t flags, uint64_t seed, uint64_t offset,
                            int32_t* out_x, float* conf_out, int32_t* out_counts, void* stream);

/* The per-sample normaliser of the confidence-weighted remask probability.   x int32, conf fp32 (N, D); held uint8 (N, D) or NULL;
 * out_norm fp32 (N, 2), written in full; temp >= 0.02; 1 <= D <= 2^24 (U_n is exact in fp32).
 *   out_norm[n] = (U_n, Z_n):  U_n = the number of free unmasked rows d of sample n (x != m, not held),
 *                              Z_n = the sum over those rows of exp(-conf[n][d] / temp)   (expf of the fp32 quotient, summed in fp64).
 * A sample without a free unmasked row gets (0, 0): ctdd_absorb_remask_step then remasks nothing in it.
 * Deterministic, no floating-point atomic (the order of ctdd_absorb_nll's sum): one workgroup of 256 threads per sample; thread i adds
 * its rows d = i, i + 256, .. in ascending d in fp64; the 64 lanes of a wave combine by the xor butterfly 32, 16, 8, 4, 2, 1; the four
 * waves' sums are added in wave order; the total is rounded to fp32 once.  Repeated calls write the same bits. */
int ctdd_absorb_remask_norm(const int32_t* x, const uint8_t* held, const float* conf, int N, int D, int mask_state, float temp,
                            float* out_norm, void* stream);

/* First-hitting sampling (Zheng et al., "Masked diffusion models are secretly time-agnostic masked models and exploit inaccurate
 * categorical sampling"): the reverse chain of a fixed network simulated event by event, without a time grid.  Write the masking
 * level of time t as c(t) = 1 - alpha_t.  Given that an entry is masked at level c, the level at which it was masked is uniform on
 * (0, c), independently over the entries; so with M entries masked at level c the next one to unmask is uniform among the M, and it
 * unmasks at the largest of M uniforms on (0, c), c u^(1/M) with u uniform on (0, 1).  In logs, L = log c:
 *   L' = L + log(u) / M,   then M - 1 entries are masked at level exp(L').
 * ctdd_absorb_hit_time walks that recursion per sample before the network runs; ctdd_absorb_hit_step, after it, picks which masked
 * rows the events fall on and draws their states.
 *
 * ctdd_absorb_hit_time: per-sample event levels.   x int32 (N, D); logc_in, logc_out fp64 (N,), logc_out may be logc_in;
 * counts int32 (N,), t_eval fp32 (N,), both written in full; kmax >= 1; 1 <= D <= 2^30.  One workgroup of 256 threads per sample.
 *   M_n = the number of rows d with x[n][d] == m (ballots, then an integer sum over the four waves: exact).
 *   In fp64, by one thread:  L_0 = logc_in[n];  L_{i+1} = L_i + log((double)u_i) / (double)(M_n - i),  i = 0 .. min(kmax, M_n) - 1.
 *   Event i is accepted iff L_{i+1} >= log_cmin (log_cmin may be -inf: every event is accepted).  The first refusal ends the sample:
 *   no later event is accepted and logc_out[n] = log_cmin.
 *   counts[n]   = the number of accepted events, in [0, min(kmax, M_n)];
 *   logc_out[n] = the level after the last accepted event if none was refused (logc_in[n], bit for bit, if M_n == 0);
 *   t_eval[n]   = (float)min(max(T(1 - exp(L_1)), t_min), t_max) if at least one event is accepted, else (float)t_min, with
 *                 T the inverse of alpha_t in fp64, by t_func:
 *     CTDD_ABSORB_T_LOGLINEAR  T(a) = (1 - a) / (1 - alpha_eps)
 *     CTDD_ABSORB_T_LOG_SQR    T(a) = sqrt(a^(-1 / rate_const) - 1)
 *     CTDD_ABSORB_T_SQRT_COS   T(a) = (2 / pi) acos(r^2),  r = 1 + ln a / rate_const clamped to [0, 1]
 *     CTDD_ABSORB_T_LOG        T(a) = ln(1 - ln a / (rate_const time_base)) / ln(time_exp)
 *   (parameters a schedule does not name are unused; a = 0 gives +inf or the clamp: t_max).
 *   u_i: component (i & 3) of the block Philox(key = seed, counter = (row = N D + n, offset, draw = i >> 2)), mapped to (0, 1) as
 *   ctdd_philox_uniform does.  The rows N D .. N D + N - 1 lie past every entry row n D + d, so no block of
 *   ctdd_absorb_hit_step (or of ctdd_absorb_step) under the same (seed, offset) is read twice. */
#define CTDD_ABSORB_T_LOGLINEAR 0
#define CTDD_ABSORB_T_LOG_SQR 1
#define CTDD_ABSORB_T_SQRT_COS 2
#define CTDD_ABSORB_T_LOG 3
int ctdd_absorb_hit_time(const int32_t* x, const double* logc_in, int N, int D, int mask_state, int kmax, double log_cmin, int t_func,
                         double rate_const, double alpha_eps, double time_base, double time_exp, double t_min, double t_max, uint64_t seed,
                         uint64_t offset, int32_t* out_counts, float* out_t_eval, double* logc_out, void* stream);

/* ctdd_absorb_hit_step: per sample, k_n masked rows drawn uniformly without replacement take a state from the network's logits.
 *   logits (N, D, S); x, out_x int32 (N, D), out_x may be x; counts int32 (N,) on the device (ctdd_absorb_hit_time's);
 *   flags: CTDD_ABSORB_ARGMAX or 0.  One workgroup of 256 threads per sample, 1 <= D <= 2^30, 2 <= S <= CTDD_MAX_S.
 *   M_n = the number of rows d with x[n][d] == m;  k_n = min(M_n, max(0, counts[n])).
 *   Selection: the key of a masked row d is the uint32 component 0 of the block Philox(key = seed, counter = (row = n D + d, offset,
 *   draw = 1)); the k_n masked rows first in the order (key descending, equal keys in ascending d) are selected -- the keys are
 *   i.i.d., so this is a uniform draw of k_n of the M_n rows.  It is ctdd_absorb_commit's radix select (the same device code) on
 *   these keys: four passes of 8-bit digit histograms, then one pass over d in ascending chunks of 256.  The keys are recomputed in
 *   every pass; nothing of a sample is kept in LDS but the histogram and one chunk's list of selected rows.
 *   Draw: a selected row r = n D + d takes the state ctdd_absorb_step gives it at p_unmask = 1 under the same (seed, offset) (the
 *   same device code in the same row packing): u1 = component 1 of the block (row = r, offset, draw = 0), the first s whose running
 *   sum of e[s] exceeds u1 z; argmax_{s != m} l[s] with the lowest index on ties under CTDD_ABSORB_ARGMAX.  Never m.
 *   Order of operations in the last pass, per chunk of 256 rows: two ballots per wave (keys above the threshold, keys at it), the
 *   waves' counts through LDS, the selected rows of the chunk written to an LDS list in ascending d, then the four waves' row groups
 *   (64, 16, 4 or 1 rows a wave, by S) walk the list: logits are read for the selected rows only.
 *   Every other row: out_x = x, bit for bit; its logits are not read.  A sample with k_n == 0 is finished after the count (and
 *   copied to out_x when out_x != x).
 * out_changed (int32[1] or NULL) += sum_n k_n (one atomic per workgroup with k_n > 0). */
int ctdd_absorb_hit_step(const float* logits, const int32_t* x, const int32_t* counts, int N, int D, int S, int mask_state, uint32_t flags,
                         uint64_t seed, uint64_t offset, int32_t* out_x, int32_t* out_changed, void* stream);

/* ctdd_absorb_filter: temperature, top-k and top-p (nucleus) truncation of the logits of the masked rows, ahead of any of the step
 * kernels above (ctdd_absorb_step, _propose, _remask_step, _hit_step), which then draw from -- or take the argmax, the score, the
 * confidence of -- the tempered, truncated and renormalised distribution without a change: a logit of -inf has the weight exactly 0.
 *   logits, out fp32 (N, D, S); x int32 (N, D).  out may be logits (in place); otherwise the two do not overlap.
 *   temperature T > 0 and finite; top_k >= 0; 0 < top_p <= 1 (CTDD_ERANGE otherwise).  ctdd_absorb_step's grid and row packing.
 *   x != m: the row is neither read nor written (out keeps what it held).
 *   x == m: over the real states s != m, in this order:
 *     1. v[s] = l[s] / T, the IEEE fp32 quotient: T == 1 keeps the bits.  A NaN counts as -inf from here on.
 *     2. The states are ordered by (v descending, s ascending); v is compared through the 32-bit key of ctdd_absorb_commit.
 *     3. top_k = k with 1 <= k < S - 1: the first k states of the order stay candidates.  k = 0 or k >= S - 1: all of them do.
 *     4. top_p = p < 1: with e[s] = exp(v[s] - mx) over the candidates (mx their maximum) and z their sum, the shortest prefix of the
 *        order whose sum of e reaches p z stays: state i of the order stays iff the sum over the states before it is below p z, so
 *        the first always does.  The sums are fp32 (over the states above the boundary value as one group sum, plus a multiple of
 *        the common weight for states that tie at the boundary value): a prefix whose mass lies within about 1e-6 z of p z may be
 *        judged either way.  p = 1: every candidate stays.
 *     5. out[s] = v[s] for a state that stays, -inf for one that does not, -inf for s == m.
 *     6. A row without a finite real-state logit (every v is -inf) is left as it came: out's row = the row of logits, bit for bit.
 *   A quotient that overflows to +inf (or a logit of +inf) is outside the contract, as it is for the step kernels.
 *   With T == 1, k off and p == 1 the call only sets the masked rows' mask column and NaNs to -inf; callers skip it.
 * The row is held in registers in full before anything is stored.  Selection, per row group (64, 16, 4 or 1 rows a wave, by S):
 * the k-th largest key by a search over the key's 32 bits, most significant first, one group count a round; the states at that key
 * by an exclusive index scan; for top-p a second 32-round search for the largest key tau whose set {key >= tau} carries at least
 * p z, on one summation function of the threshold (monotone in it), and the same index scan at tau.  No LDS, no sort; one read and
 * one write of a masked row.  A wave without a masked row returns after reading x. */
int ctdd_absorb_filter(const float* logits, const int32_t* x, int N, int D, int S, int mask_state, float temperature, int top_k,
                       float top_p, float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
