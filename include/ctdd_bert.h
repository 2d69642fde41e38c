/* ctdd_bert.h -- C ABI of what the single-stream transformer score models add to the hollow-transformer kernels
 * (libctdd.so, gfx950).  Reference: TAUnSDDM/lib/networks/hollow_networks.py (TransformerEncoder 450-493, MaskedTransformer
 * 859-914, EnumerativeTransformer 917-960, BertEnumTransformer 963-1031).  The encoder blocks, the FiLM readout and the GEMMs
 * are the entry points of ctdd_hollow.h; the encoder's attention is ctdd_hollow_attention / _bf16 with mode 3 (unmasked).
 * Conventions as there: fp32 device buffers, caller-owned; 0 or a negative CTDD_E* code. */
#ifndef CTDD_BERT_H
#define CTDD_BERT_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* out[r] = [temb_b, emb(x_b0) .. emb(x_b,D-1)] + pe, (rows, D + 1, E); temb and emb(x) = w_in (2 x / (S - 1) - 1) + b_in as
 * ctdd_hollow_embed computes them.  enumerate = 0: rows == B, b = r.  enumerate = 1 (the masked model): row r is sequence
 * g = *r0 + r of the (B D') enumeration, D' = D - cond: b = g / D', and token p = cond + g % D' enters as the mask value S.
 * r0 is a device scalar (null: 0), so one captured launch serves every chunk; rows with g >= B D' repeat the last sequence.
 * temb (B, E), optional, receives the time embedding of every sample that owns a row with p == cond (plain mode: of all). */
typedef struct {
  const int64_t* x64; const int32_t* x32; const float* t; const float* w_in; const float* b_in; const float* pe;
  int B, D, E, S; float temb_scale; float* out; float* temb;
  int enumerate, cond, rows; const int32_t* r0;
} ctdd_bert_embed_args;
int ctdd_bert_embed(const void* embed_args, void* stream);

/* ctdd_hollow_attention's contract (a ctdd_hollow_attn_args block, ctdd_hollow.h) for mode 3 with Tq <= 64 and Tk <= 64, head
 * dimension 4, 8, 16 or 32: one wave per (sequence, head) with its keys and values resident in LDS, fp32 arithmetic; `split` is
 * ignored.  Anything else returns CTDD_EINVAL / CTDD_ERANGE and launches nothing. */
int ctdd_bert_attention_short(const void* attn_args, void* stream);

/* readout input from the encoder output enc (rows', D + 1, E), as fp32 and / or bf16 hi (+ lo).  enumerate = 0: rows == B (D - cond),
 * out row g = b (D - cond) + j takes row 1 + cond + j of sequence b (r0 unused).  enumerate = 1: chunk row r is sequence
 * g = *r0 + r = (b, p) as in ctdd_bert_embed; its row 1 + p goes to row g of out (B D', E); rows with g >= B D' are dropped */
int ctdd_bert_gather(const float* enc, const int32_t* r0, int rows, int enumerate, int B, int D, int cond, int E, float* out, void* out_bf16,
                     void* out_lo, void* stream);

/* backward of ctdd_bert_embed in plain mode: g (B, D + 1, E) is the gradient of `out`; dw_in[e] += sum_{b,d} g[b][1 + d][e]
 * (2 x_bd / (S - 1) - 1), db_in[e] += sum_{b,d} g[b][1 + d][e] (fp32 atomics: the caller zeroes dw and db).  Row 0, the time
 * embedding, has no parameters. */
typedef struct {
  const int64_t* x64; const int32_t* x32; const float* g; int B, D, E, S; float* dw; float* db;
} ctdd_bert_embed_bwd_args;
int ctdd_bert_embed_bwd(const void* embed_bwd_args, void* stream);

/* backward of ctdd_bert_gather in plain mode with cond = 0 (anything else: CTDD_EINVAL): d_out (B D, E) goes to rows 1..D of
 * d_enc (B, D + 1, E), row 0 of every sequence is written as zero. */
int ctdd_bert_gather_bwd(const float* d_out, int B, int D, int cond, int E, float* d_enc, void* stream);

/* backward of ctdd_bert_embed in enumerate mode over the window [r0, r0 + rows) of the (B D') enumeration (r0 a host value; the
 * window may cross sample borders): g (rows, D + 1, E) is the gradient of the chunk's `out`; with chunk row r = sequence
 * (b, p) as there,  dw_in[e] += sum_{r,d} g[r][1 + d][e] xn(r, d),  db_in[e] += sum_{r,d} g[r][1 + d][e],  xn = 2 x / (S - 1) - 1
 * with x the mask value S at d == p.  dw and db are ACCUMULATED into (one fp32 atomic per column and workgroup), so the chunks
 * of one enumeration add up: the caller zeroes them before the first.  A window outside the enumeration: CTDD_ERANGE. */
typedef struct {
  const int64_t* x64; const int32_t* x32; const float* g; int B, D, E, S, cond, rows; int64_t r0; float* dw; float* db;
} ctdd_bert_embed_enum_bwd_args;
int ctdd_bert_embed_enum_bwd(const void* embed_enum_bwd_args, void* stream);

/* backward of ctdd_bert_gather in enumerate mode over the same window: row g = r0 + r of d_out (B D', E) goes to row 1 + p of
 * sequence r of d_enc (rows, D + 1, E); every other row of d_enc is written as zero (every element is written), and rows of
 * d_out outside the window are never read. */
int ctdd_bert_gather_enum_bwd(const float* d_out, int64_t r0, int rows, int B, int D, int cond, int E, float* d_enc, void* stream);

/* training attention for short sequences on ctdd_hollow_attention_train / _bwd's contract (a ctdd_hollow_attn_train_args block,
 * ctdd_hollow_train.h: same strides, same stats rows, the same Philox keep bits on equal {seed, step, layer}) for mode 3 with
 * Tq == Tk <= 64 and head dimension 4 or 8, rows and buffers 16-byte aligned: one wave per (sequence, head) with the pair's
 * operands resident in LDS, fp32 arithmetic, the backward one launch without atomics.  Anything else returns CTDD_EINVAL /
 * CTDD_ERANGE and launches nothing. */
int ctdd_bert_attention_short_train(const void* attn_train_args, void* stream);
int ctdd_bert_attention_short_bwd(const void* attn_train_args, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CTDD_BERT_H */
