"""ctypes binding of the C ABI declared in include/ctdd.h.

torch is used for device memory and streams only: every wrapper checks dtype / device /
contiguity, passes raw device pointers + the current HIP stream, and raises CtddError with the
library's message on a non-zero status.  There is NO fallback: if libctdd.so is missing or an
operand is not on a GPU the call fails loudly (the CPU restatement lives in /oracle and is test
infrastructure only).
"""
import ctypes as C
import os

import torch

_HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_LIB = None

BRANCH_CTELBO, BRANCH_CRM = 0, 1
LOGIT_TYPES = {"direct": 0, "reverse_prob": 1, "reverse_logscale": 2}
STEP_ORDINAL, STEP_CORRECTOR, STEP_COUNT_RAW, STEP_CRM, STEP_COUNT_JUMPS, STEP_BF16, STEP_LOGITS_BF16 = 1, 2, 4, 8, 16, 32, 64


class CtddError(RuntimeError):
    pass


def lib_path():
    """libctdd.so next to the package; CTDD_LIBRARY names another build of it (A/B measurements of one kernel change)."""
    return os.environ.get("CTDD_LIBRARY") or os.path.join(_HERE, "libctdd.so")


_P, _I, _F, _U64, _U32, _I64, _D = C.c_void_p, C.c_int, C.c_float, C.c_uint64, C.c_uint32, C.c_int64, C.c_double
_SIGS = {
    "ctdd_abi_version": ([], _I),
    "ctdd_last_error": ([], C.c_char_p),
    "ctdd_rate_table": ([_P, _P, _P, _P, _P, _P, _I, _I, _I, _F, _P, _P, _P, _P, _P], _I),
    "ctdd_noise_categorical": ([_P, _P, _P, _P, _U64, _U64, _I, _I, _I, _P, _P], _I),
    "ctdd_xtilde_sample": ([_P, _P, _P, _P, _P, _U64, _U64, _I, _I, _I, _P, _P, _P, _P], _I),
    "ctdd_xtilde_sample_masked": ([_P, _P, _P, _P, _P, _P, _U64, _U64, _I, _I, _I, _P, _P, _P, _P], _I),
    "ctdd_logprob": ([_P, _P, _P, _P, _I, _I, _I, _I, _P, _P, _P], _I),
    "ctdd_reverse_rates": ([_I, _I, _P, _P, _P, _P, _P, _F, _I, _I, _I, _P, _P, _P], _I),
    "ctdd_tauleap_apply": ([_P, _P, _P, _I, _I, _I, _I, _P, _P, _P], _I),
    "ctdd_tauleap_draw": ([_P, _P, _P, _F, _U32, _U64, _U64, _I, _I, _I, _P, _P, _P], _I),
    "ctdd_tauleap_step": ([_I, _I, _P, _P, _P, _P, _P, _F, _F, _F, _U32, _U64, _U64, _I, _I, _I, _P, _P, _P], _I),
    "ctdd_tauleap_step_rows": ([_I, _I, _P, _P, _P, _P, _P, _F, _F, _F, _U32, _U64, _U64, _I, _I, _I, _P, _I, _P, _P, _P], _I),
    "ctdd_lbjf_step": ([_I, _I, _P, _P, _P, _P, _F, _F, _F, _U32, _P, _U64, _U64, _I, _I, _I, _P, _P, _P, _P], _I),
    "ctdd_logprob_rp_mfma": ([_P, _P, _P, _I, _I, _I, _P, _P, _P, _P], _I),
    "ctdd_logprob_rp_bwd_mfma": ([_P, _P, _P, _P, _P, _F, _I, _I, _I, _P, _P, _P, _P, _P], _I),
    "ctdd_exact_step": ([_P, _P, _P, _P, _P, _U64, _U64, _I, _I, _I, _P, _P, _P, _P], _I),
    "ctdd_midpoint_predict": ([_I, _I, _P, _P, _P, _P, _F, _F, _F, _I, _I, _I, _P, _P], _I),
    "ctdd_lbjf_from_rates": ([_P, _P, _F, _P, _U64, _U64, _I, _I, _I, _P, _P, _P, _P], _I),
    "ctdd_midpoint_from_rates": ([_P, _P, _F, _I, _I, _I, _P, _P], _I),
    "ctdd_lbjf_step_rows": ([_I, _I, _P, _P, _P, _P, _F, _F, _F, _U32, _P, _U64, _U64, _I, _I, _I, _P, _I, _P, _P, _P, _P], _I),
    "ctdd_midpoint_predict_rows": ([_I, _I, _P, _P, _P, _P, _F, _F, _F, _I, _I, _I, _P, _I, _P, _P], _I),
    "ctdd_exact_step_rows": ([_P, _P, _P, _P, _P, _U64, _U64, _I, _I, _I, _P, _I, _P, _P, _P, _P], _I),
    "ctdd_lbjf_from_rates_rows": ([_P, _P, _F, _P, _U64, _U64, _I, _I, _I, _P, _I, _P, _P, _P, _P], _I),
    "ctdd_midpoint_from_rates_rows": ([_P, _P, _F, _I, _I, _I, _P, _I, _P, _P], _I),
    "ctdd_argmax": ([_P, _I, _I, _I, _P, _P], _I),
    "ctdd_initial_samples": ([_P, _U64, _U64, _I, _I, _I, _P, _P], _I),
    "ctdd_philox_uniform": ([_U64, _U64, _I64, _I, _P, _P], _I),
    "ctdd_s256_step_table_bytes": ([], _I64),
    "ctdd_s256_prepare": ([_P, _P, _F, _I, _P, _P, _P, _P], _I),
    "ctdd_s256_prepare_crm": ([_P, _P, _I, _P, _P, _P, _P], _I),
    "ctdd_tauleap_step_s256": ([_P, _P, _P, _P, _P, _P, _F, _F, _U32, _U64, _U64, _I, _I, _P, _P, _P, _P], _I),
    "ctdd_tauleap_step_s256_rows": ([_P, _P, _P, _P, _P, _P, _F, _F, _U32, _U64, _U64, _I, _I, _P, _I, _P, _P, _P, _P], _I),
    "ctdd_crm_loss": ([_P, _P, _P, _P, _I, _I, _I, _I, _F, _F, _P, _P, _P, _P], _I),
    "ctdd_ctelbo_scratch_bytes": ([_I, _I, _I], _I64),
    "ctdd_ctelbo_loss": ([_P, _P, _P, _P, _P, _P, _I, _I, _I, _F, _F, _F, _P, _P, _P, _P], _I),
    "ctdd_ctelbo_loss_terms": ([_P, _P, _P, _P, _P, _P, _I, _I, _I, _F, _F, _F, _F, _P, _P, _P, _P], _I),
    "ctdd_ctelbo_loss_window": ([_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _F, _F, _F, _F, _P, _P, _P, _P], _I),
    "ctdd_ctelbo_loss_masked": ([_P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _F, _F, _F, _F, _P, _P, _P, _P], _I),
    "ctdd_score_elbo_loss": ([_P, _P, _P, _P, _P, _P, _I, _I, _I, _F, _F, _P, _P, _P, _P], _I),
    "ctdd_crm_loss_ll": ([_P, _P, _P, _I, _I, _I, _I, _F, _P, _P, _P, _P], _I),
    "ctdd_score_elbo_loss_ll": ([_P, _P, _P, _P, _P, _P, _I, _I, _I, _F, _F, _P, _P, _P, _P], _I),
    "ctdd_logprob_bwd": ([_I, _P, _P, _P, _P, _P, _F, _I, _I, _I, _P, _P, _P, _P], _I),
    "ctdd_crm_loss_masked": ([_P, _P, _P, _P, _P, _I, _I, _I, _I, _F, _F, _P, _P, _P, _P], _I),
    "ctdd_crm_loss_ll_masked": ([_P, _P, _P, _P, _I, _I, _I, _I, _F, _P, _P, _P, _P], _I),
    "ctdd_score_elbo_loss_masked": ([_P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _F, _F, _P, _P, _P, _P], _I),
    "ctdd_score_elbo_loss_ll_masked": ([_P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _F, _F, _P, _P, _P, _P], _I),
    "ctdd_opt_chunk_elems": ([], _I),
    "ctdd_adam_ema_step": ([_P, _P, _I, _F, _F, _F, _F, _I64, _F, _F, _P, _P], _I),
    "ctdd_grad_sumsq": ([_P, _P, _I, _P, _I, _P], _I),
    "ctdd_adam_ema_apply": ([_P, _P, _I, _F, _F, _F, _F, _I64, _F, _F, _P, _P], _I),
    "ctdd_d3pm_scratch_bytes": ([_I, _I, _I], _I64),
    "ctdd_d3pm_loss": ([_P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _F, _F, _F, _P, _P, _P, _P, _P, _P], _I),
    "ctdd_d3pm_step": ([_P, _P, _P, _P, _P, _I, _I, _I, _I, _F, _P, _U64, _U64, _P, _P, _P, _P], _I),
    "ctdd_absorb_noise": ([_P, _P, _I, _I, _I, _U64, _U64, _P, _P], _I),
    "ctdd_absorb_scratch_bytes": ([], _I64),
    "ctdd_absorb_elbo_loss": ([_P, _P, _P, _P, _F, _I, _I, _I, _I, _P, _P, _P, _P], _I),
    "ctdd_absorb_step": ([_P, _P, _I, _I, _I, _I, _F, _U32, _U64, _U64, _P, _P, _P], _I),
    "ctdd_absorb_propose": ([_P, _P, _I, _I, _I, _I, _F, _U32, _U64, _U64, _P, _P, _P], _I),
    "ctdd_absorb_commit": ([_P, _P, _P, _I, _I, _I, _F, _P, _P, _P, _P], _I),
    "ctdd_absorb_nll": ([_P, _P, _P, _P, _I, _I, _I, _I, _P, _P, _P, _P, _P], _I),
    "ctdd_absorb_remask_step": ([_P, _P, _P, _P, _P, _I, _I, _I, _I, _F, _F, _F, _U32, _U64, _U64, _P, _P, _P, _P], _I),
    "ctdd_absorb_remask_norm": ([_P, _P, _P, _I, _I, _I, _F, _P, _P], _I),
    "ctdd_absorb_hit_time": ([_P, _P, _I, _I, _I, _I, _D, _I, _D, _D, _D, _D, _D, _D, _U64, _U64, _P, _P, _P, _P], _I),
    "ctdd_absorb_hit_step": ([_P, _P, _P, _I, _I, _I, _I, _U32, _U64, _U64, _P, _P, _P], _I),
    "ctdd_absorb_filter": ([_P, _P, _I, _I, _I, _I, _F, _I, _F, _P, _P], _I),
}
UNET_EXPORTS = ("ctdd_unet_conv", "ctdd_unet_conv_patch", "ctdd_unet_conv_res", "ctdd_unet_conv_ring", "ctdd_unet_conv_up_phases", "ctdd_unet_upsample2x", "ctdd_unet_first_conv", "ctdd_unet_gn_apply", "ctdd_unet_gn_onepass", "ctdd_unet_channel_stats",
                "ctdd_unet_time", "ctdd_unet_time_uniform", "ctdd_unet_attention", "ctdd_unet_logistic_head", "ctdd_unet_resblock_small",
                "ctdd_unet_resblock_mid", "ctdd_unet_conv_rows", "ctdd_unet_conv_rows_w4", "ctdd_unet_conv_rows_head", "ctdd_unet_conv_rows_head_w4", "ctdd_unet_attention_block")    # bound in ctdd/unet_engine.py
HOLLOW_EXPORTS = ("ctdd_gemm_bf16", "ctdd_hollow_small_linear", "ctdd_hollow_embed", "ctdd_hollow_layernorm", "ctdd_hollow_add", "ctdd_hollow_put_rows", "ctdd_hollow_attention", "ctdd_hollow_attention_bf16")
UNET_TRAIN_EXPORTS = ("ctdd_unet_wgrad", "ctdd_unet_gn_bwd", "ctdd_unet_dropout", "ctdd_unet_colsum", "ctdd_unet_sum_batch", "ctdd_unet_sum_jobs", "ctdd_unet_accumulate",
                      "ctdd_unet_downsum2x", "ctdd_unet_upsample2x_f32", "ctdd_unet_cast_rows", "ctdd_unet_attention_bwd",
                      "ctdd_unet_first_conv_wgrad", "ctdd_unet_first_conv_wgrad_scratch", "ctdd_unet_pack_weights",
                      "ctdd_unet_unpack_grads", "ctdd_unet_gn_bwd_plan", "ctdd_unet_attention_bwd_plan")    # bound in ctdd/unet_train.py
HOLLOW_TRAIN_EXPORTS = ("ctdd_hollow_layernorm_bwd", "ctdd_hollow_attention_train", "ctdd_hollow_attention_bwd", "ctdd_hollow_attention_train_bf16", "ctdd_hollow_attention_bwd_bf16", "ctdd_hollow_act", "ctdd_hollow_relu_bf16", "ctdd_hollow_colsum", "ctdd_hollow_dropout",
                        "ctdd_hollow_embed_bwd")                                       # bound in ctdd/hollow_train.py
BERT_EXPORTS = ("ctdd_bert_embed", "ctdd_bert_gather", "ctdd_bert_attention_short",                               # bound in ctdd/bert_engine.py
                "ctdd_bert_embed_bwd", "ctdd_bert_gather_bwd",                                                    # bound in ctdd/bert_train.py
                "ctdd_bert_embed_enum_bwd", "ctdd_bert_gather_enum_bwd",                                          # bound in ctdd/masked_train.py
                "ctdd_bert_attention_short_train", "ctdd_bert_attention_short_bwd")                               # bound in ctdd/hollow_train.py
EXPORTS = tuple(_SIGS) + UNET_EXPORTS + HOLLOW_EXPORTS + UNET_TRAIN_EXPORTS + HOLLOW_TRAIN_EXPORTS + BERT_EXPORTS


def load():
    """dlopen libctdd.so once; raise (never fall back) when it is absent."""
    global _LIB
    if _LIB is None:
        path = lib_path()
        if not os.path.exists(path):
            raise CtddError(f"{path} not found: build it with `python __graft_entry__.py` "
                            "(hipcc --offload-arch=gfx950); there is no CPU fallback")
        lib = C.CDLL(path)
        for name, (argt, rest) in _SIGS.items():
            fn = getattr(lib, name)
            fn.argtypes, fn.restype = argt, rest
        _LIB = lib
    return _LIB


def _ptr(t, dtype=None, name="tensor"):
    if t is None:
        return None
    if not isinstance(t, torch.Tensor):
        raise CtddError(f"{name}: expected a torch tensor, got {type(t)}")
    if not t.is_cuda:
        raise CtddError(f"{name}: must live on a GPU (got {t.device}); libctdd has no CPU path")
    if dtype is not None and t.dtype != dtype:
        raise CtddError(f"{name}: expected {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise CtddError(f"{name}: must be contiguous")
    return t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _check(rc, what):
    if rc != 0:
        msg = load().ctdd_last_error().decode(errors="replace")
        raise CtddError(f"{what} failed with status {rc}: {msg}")


f32, i32 = torch.float32, torch.int32

LAUNCH_COUNTS = {}      # entry point -> calls (tests assert that an objective really ran through the HIP path)


def _count(name):
    LAUNCH_COUNTS[name] = LAUNCH_COUNTS.get(name, 0) + 1


def rate_table(eigvecs, right, eigvals, base_rate, integral, beta, S, normalise, clamp_below=1e-8,
               want_qt0=True, want_qt0T=False, want_rate=False, want_noise_probs=False):
    nT = integral.numel()
    dev = integral.device
    mk = lambda want: torch.empty((nT, S, S), dtype=f32, device=dev) if want else None
    q, qT, r, pn = mk(want_qt0), mk(want_qt0T), mk(want_rate), mk(want_noise_probs)
    rc = load().ctdd_rate_table(_ptr(eigvecs, f32, "eigvecs"), _ptr(right, f32, "right"), _ptr(eigvals, f32, "eigvals"),
                                _ptr(base_rate, f32, "base_rate"), _ptr(integral, f32, "integral"),
                                _ptr(beta, f32, "beta"), nT, S, int(bool(normalise)), float(clamp_below),
                                _ptr(q), _ptr(qT), _ptr(r), _ptr(pn), _stream())
    _check(rc, "ctdd_rate_table")
    return q, qT, r, pn


def noise_categorical(probs, x0, tidx=None, E=None, seed=0, offset=0):
    B, D = x0.shape
    S = probs.shape[-1]
    out = torch.empty((B, D), dtype=i32, device=x0.device)
    rc = load().ctdd_noise_categorical(_ptr(probs, f32, "probs"), _ptr(tidx, i32, "tidx"), _ptr(x0, i32, "x0"),
                                       _ptr(E, f32, "E"), seed, offset, B, D, S, _ptr(out), _stream())
    _check(rc, "ctdd_noise_categorical")
    return out


def xtilde_sample(rate, x_t, tidx=None, E_dim=None, E_val=None, seed=0, offset=0):
    B, D = x_t.shape
    S = rate.shape[-1]
    dev = x_t.device
    dims = torch.empty((B,), dtype=i32, device=dev)
    newval = torch.empty((B,), dtype=i32, device=dev)
    xt = torch.empty((B, D), dtype=i32, device=dev)
    rc = load().ctdd_xtilde_sample(_ptr(rate, f32, "rate"), _ptr(tidx, i32, "tidx"), _ptr(x_t, i32, "x_t"),
                                   _ptr(E_dim, f32, "E_dim"), _ptr(E_val, f32, "E_val"), seed, offset, B, D, S,
                                   _ptr(dims), _ptr(newval), _ptr(xt), _stream())
    _check(rc, "ctdd_xtilde_sample")
    return dims, newval, xt


def _free_mask(free, B, D, what):
    """The (B, D) mask of free entries as the kernels read it: uint8 (a bool tensor is reinterpreted, not copied)."""
    if not isinstance(free, torch.Tensor) or free.dtype not in (torch.bool, torch.uint8):
        raise CtddError(f"{what}: free must be a bool or uint8 tensor, got {getattr(free, 'dtype', type(free))}")
    if tuple(free.shape) != (B, D):
        raise CtddError(f"{what}: free {tuple(free.shape)} against states {(B, D)}")
    return _ptr(free.view(torch.uint8) if free.dtype == torch.bool else free, torch.uint8, "free")


def xtilde_sample_masked(rate, x_t, free, tidx=None, E_dim=None, E_val=None, seed=0, offset=0):
    """K3 with the jump restricted to the free entries (`free` (B, D) bool / uint8): (dims, newval, x~); a sample without a
    free entry comes back unchanged with dims = -1.  All free: xtilde_sample bit for bit under the same seed."""
    B, D = x_t.shape
    S = rate.shape[-1]
    dev = x_t.device
    fp = _free_mask(free, B, D, "xtilde_sample_masked")
    if E_dim is not None and tuple(E_dim.shape) != (B, D):
        raise CtddError(f"xtilde_sample_masked: E_dim {tuple(E_dim.shape)} against states {(B, D)}")
    if E_val is not None and tuple(E_val.shape) != (B, S):
        raise CtddError(f"xtilde_sample_masked: E_val {tuple(E_val.shape)} against {(B, S)}")
    dims = torch.empty((B,), dtype=i32, device=dev)
    newval = torch.empty((B,), dtype=i32, device=dev)
    xt = torch.empty((B, D), dtype=i32, device=dev)
    _count("ctdd_xtilde_sample_masked")
    rc = load().ctdd_xtilde_sample_masked(_ptr(rate, f32, "rate"), _ptr(tidx, i32, "tidx"), _ptr(x_t, i32, "x_t"), fp,
                                          _ptr(E_dim, f32, "E_dim"), _ptr(E_val, f32, "E_val"), seed, offset, B, D, S,
                                          _ptr(dims), _ptr(newval), _ptr(xt), _stream())
    _check(rc, "ctdd_xtilde_sample_masked")
    return dims, newval, xt


def _rp_mfma_ok(logit_type, logits, qt0):
    N, D, S = logits.shape
    return logit_type == "reverse_prob" and S % 32 == 0 and 32 <= S <= 256 and qt0 is not None and qt0.dim() == 3 and qt0.shape[0] == N


def logprob(logits, x, qt0, logit_type, tidx=None, qt0T=None):
    """get_logprob_with_logits.  qt0T given (per-sample transposed tables), reverse_prob, S % 32 == 0: the matrix-core path."""
    N, D, S = logits.shape
    ll_all = torch.empty_like(logits)
    ll_xt = torch.empty((N, D), dtype=f32, device=logits.device)
    if qt0T is not None and _rp_mfma_ok(logit_type, logits, qt0):
        scratch = torch.empty_like(logits)
        rc = load().ctdd_logprob_rp_mfma(_ptr(logits, f32, "logits"), _ptr(x, i32, "x"), _ptr(qt0T, f32, "qt0T"), N, D, S, _ptr(scratch),
                                         _ptr(ll_all), _ptr(ll_xt), _stream())
        _check(rc, "ctdd_logprob_rp_mfma")
        _count("ctdd_logprob")
        return ll_all, ll_xt
    rc = load().ctdd_logprob(_ptr(logits, f32, "logits"), _ptr(x, i32, "x"), _ptr(qt0, f32, "qt0"),
                             _ptr(tidx, i32, "tidx"), LOGIT_TYPES[logit_type], N, D, S, _ptr(ll_all), _ptr(ll_xt),
                             _stream())
    _check(rc, "ctdd_logprob")
    return ll_all, ll_xt


def reverse_rates(branch, logit_type, logits, x, qt0, rate, eps, tidx=None, want_ratio=True):
    N, D, S = logits.shape
    rr = torch.empty_like(logits)
    ratio = torch.empty_like(logits) if want_ratio else None
    rc = load().ctdd_reverse_rates(branch, LOGIT_TYPES[logit_type], _ptr(logits, f32, "logits"), _ptr(x, i32, "x"),
                                   _ptr(qt0, f32, "qt0"), _ptr(rate, f32, "rate"), _ptr(tidx, i32, "tidx"),
                                   float(eps), N, D, S, _ptr(rr), _ptr(ratio), _stream())
    _check(rc, "ctdd_reverse_rates")
    return rr, ratio


def tauleap_apply(x, jump_nums, is_ordinal, x_base=None, changed=None):
    N, D, S = jump_nums.shape
    out = torch.empty((N, D), dtype=i32, device=x.device)
    rc = load().ctdd_tauleap_apply(_ptr(x, i32, "x"), _ptr(x_base, i32, "x_base"), _ptr(jump_nums, f32, "jump_nums"),
                                   int(bool(is_ordinal)), N, D, S, _ptr(out), _ptr(changed, i32, "changed"), _stream())
    _check(rc, "ctdd_tauleap_apply")
    return out


def tauleap_draw(rates, x, h, is_ordinal, seed, offset, x_base=None, changed=None):
    N, D, S = rates.shape
    out = torch.empty((N, D), dtype=i32, device=x.device)
    rc = load().ctdd_tauleap_draw(_ptr(rates, f32, "rates"), _ptr(x, i32, "x"), _ptr(x_base, i32, "x_base"), float(h),
                                  STEP_ORDINAL if is_ordinal else 0, seed, offset, N, D, S, _ptr(out),
                                  _ptr(changed, i32, "changed"), _stream())
    _check(rc, "ctdd_tauleap_draw")
    return out


# ---------------------------------------------------------------- the sampler steps: one binding per family, row list optional
# `rows` None: every row is stepped and `out` is fresh.  `rows` given (ascending, distinct int32 indices into the N*D rows, on the
# device): the `_rows` entry of the family runs the same kernels on those rows only -- listed rows bit-identical to the full
# launch's, unlisted rows of `out` / `probs` / `rates` not written (so `out` must not alias x; its default is a copy of x).
def _row_list(rows, N, D):
    if rows.dim() != 1:
        raise CtddError(f"rows: expected a 1-D int32 tensor, got shape {tuple(rows.shape)}")
    if rows.numel() > N * D:
        raise CtddError(f"rows: {rows.numel()} entries for {N * D} rows")
    return _ptr(rows, i32, "rows"), int(rows.numel())


def _prefilled(out, x, N, D):
    """The output state of a row-list step: unlisted rows are not written, so it starts as one device copy of x."""
    if out is None:
        return x.clone()
    if out.data_ptr() == x.data_ptr():
        raise CtddError("out must not alias x: the row-list step leaves unlisted rows of out untouched")
    if tuple(out.shape) != (N, D):
        raise CtddError(f"out: expected shape {(N, D)}, got {tuple(out.shape)}")
    return out


def _step_entry(name, rows, out, x, N, D, want_x=True):
    """-> (C entry, its (rows, n_rows) arguments -- they follow the shape integers in every `_rows` signature --, output state)."""
    rl = () if rows is None else _row_list(rows, N, D)
    if not want_x:
        out = None
    elif rows is not None:
        out = _prefilled(out, x, N, D)
    elif out is None:
        out = torch.empty((N, D), dtype=i32, device=x.device)
    return name if rows is None else name + "_rows", rl, out


def _buffer(want, buf, like, what):
    """A full-size f32 output (`probs`, `rates`): `buf` when given, else a fresh uninitialised tensor; None when not wanted."""
    if not want:
        return None
    if buf is None:
        return torch.empty(like.shape, dtype=f32, device=like.device)
    if tuple(buf.shape) != tuple(like.shape):
        raise CtddError(f"{what}: expected shape {tuple(like.shape)}, got {tuple(buf.shape)}")
    return buf


def _launched(rc, name):
    _check(rc, name)
    _count(name)


def _tauleap(branch, logit_type, logits, x, qt0, base_rate, beta, eps, h, flags, seed, offset, rows=None, x_base=None, out=None,
             changed=None):
    N, D, S = logits.shape
    name, rl, out = _step_entry("ctdd_tauleap_step", rows, out, x, N, D)
    _launched(getattr(load(), name)(branch, LOGIT_TYPES[logit_type], _ptr(logits, f32, "logits"), _ptr(x, i32, "x"),
                                    _ptr(x_base, i32, "x_base"), _ptr(qt0, f32, "qt0"), _ptr(base_rate, f32, "base_rate"),
                                    float(beta), float(eps), float(h), int(flags), seed, offset, N, D, S, *rl,
                                    _ptr(out, i32, "out"), _ptr(changed, i32, "changed"), _stream()), name)
    return out


def _lbjf(branch, logit_type, logits, x, qt0, base_rate, beta, eps, h, rows=None, flags=0, E=None, seed=0, offset=0, out=None,
          want_probs=False, probs=None, changed=None):
    N, D, S = logits.shape
    name, rl, out = _step_entry("ctdd_lbjf_step", rows, out, x, N, D)
    probs = _buffer(want_probs, probs, logits, "probs")
    _launched(getattr(load(), name)(branch, LOGIT_TYPES[logit_type], _ptr(logits, f32, "logits"), _ptr(x, i32, "x"),
                                    _ptr(qt0, f32, "qt0"), _ptr(base_rate, f32, "base_rate"), float(beta), float(eps), float(h),
                                    int(flags), _ptr(E, f32, "E"), seed, offset, N, D, S, *rl, _ptr(out, i32, "out"),
                                    _ptr(probs, f32, "probs"), _ptr(changed, i32, "changed"), _stream()), name)
    return (out, probs) if want_probs else out


def _exact(logits, x, q_lo, q_step, rows=None, E=None, seed=0, offset=0, out=None, want_probs=False, probs=None, changed=None):
    N, D, S = logits.shape
    name, rl, out = _step_entry("ctdd_exact_step", rows, out, x, N, D)
    probs = _buffer(want_probs, probs, logits, "probs")
    _launched(getattr(load(), name)(_ptr(logits, f32, "logits"), _ptr(x, i32, "x"), _ptr(q_lo, f32, "q_lo"),
                                    _ptr(q_step, f32, "q_step"), _ptr(E, f32, "E"), seed, offset, N, D, S, *rl,
                                    _ptr(out, i32, "out"), _ptr(probs, f32, "probs"), _ptr(changed, i32, "changed"), _stream()), name)
    return (out, probs) if want_probs else out


def _midpoint(branch, logit_type, logits, x, qt0, base_rate, beta, eps, h, rows=None, out=None):
    N, D, S = logits.shape
    name, rl, out = _step_entry("ctdd_midpoint_predict", rows, out, x, N, D)
    _launched(getattr(load(), name)(branch, LOGIT_TYPES[logit_type], _ptr(logits, f32, "logits"), _ptr(x, i32, "x"),
                                    _ptr(qt0, f32, "qt0"), _ptr(base_rate, f32, "base_rate"), float(beta), float(eps), float(h),
                                    N, D, S, *rl, _ptr(out, i32, "out"), _stream()), name)
    return out


def _lbjf_rates(rates, x, h, rows=None, E=None, seed=0, offset=0, out=None, want_probs=False, probs=None, changed=None):
    N, D, S = rates.shape
    name, rl, out = _step_entry("ctdd_lbjf_from_rates", rows, out, x, N, D)
    probs = _buffer(want_probs, probs, rates, "probs")
    _launched(getattr(load(), name)(_ptr(rates, f32, "rates"), _ptr(x, i32, "x"), float(h), _ptr(E, f32, "E"), seed, offset,
                                    N, D, S, *rl, _ptr(out, i32, "out"), _ptr(probs, f32, "probs"),
                                    _ptr(changed, i32, "changed"), _stream()), name)
    return (out, probs) if want_probs else out


def _midpoint_rates(rates, x, h, rows=None, out=None):
    N, D, S = rates.shape
    name, rl, out = _step_entry("ctdd_midpoint_from_rates", rows, out, x, N, D)
    _launched(getattr(load(), name)(_ptr(rates, f32, "rates"), _ptr(x, i32, "x"), float(h), N, D, S, *rl, _ptr(out, i32, "out"),
                                    _stream()), name)
    return out


# The public names keep their positional signatures (`rows` sits where each C signature's callers expect it).
def tauleap_step(branch, logit_type, logits, x, qt0, base_rate, beta, eps, h, flags, seed, offset,
                 x_base=None, out=None, changed=None):
    return _tauleap(branch, logit_type, logits, x, qt0, base_rate, beta, eps, h, flags, seed, offset, None, x_base, out, changed)


def tauleap_step_rows(branch, logit_type, logits, x, qt0, base_rate, beta, eps, h, flags, seed, offset, rows,
                      x_base=None, out=None, changed=None):
    """tauleap_step on the listed rows: the other rows of the result are `out` as given (default: a copy of x)."""
    return _tauleap(branch, logit_type, logits, x, qt0, base_rate, beta, eps, h, flags, seed, offset, rows, x_base, out, changed)


def lbjf_step(branch, logit_type, logits, x, qt0, base_rate, beta, eps, h, flags=0, E=None, seed=0, offset=0,
              want_probs=False, changed=None):
    return _lbjf(branch, logit_type, logits, x, qt0, base_rate, beta, eps, h, None, flags, E, seed, offset, None, want_probs, None, changed)


def lbjf_step_rows(branch, logit_type, logits, x, qt0, base_rate, beta, eps, h, rows, flags=0, E=None, seed=0, offset=0,
                   out=None, want_probs=False, probs=None, changed=None):
    """lbjf_step on the listed rows: the other rows of the state / probabilities are `out` / `probs` as given (default: a copy of
    x / uninitialised).  E, when given, is the full (N*D, S) noise: a listed row reads its own row of it."""
    return _lbjf(branch, logit_type, logits, x, qt0, base_rate, beta, eps, h, rows, flags, E, seed, offset, out, want_probs, probs, changed)


def exact_step(logits, x, q_lo, q_step, E=None, seed=0, offset=0, want_probs=False, changed=None):
    """ExactSampling step: x_new ~ Categorical((softmax(logits) @ q_lo) * q_step[:, x]) per dimension (K5-style contraction +
    exponential race in one launch)."""
    return _exact(logits, x, q_lo, q_step, None, E, seed, offset, None, want_probs, None, changed)


def exact_step_rows(logits, x, q_lo, q_step, rows, E=None, seed=0, offset=0, out=None, want_probs=False, probs=None, changed=None):
    """exact_step on the listed rows (see lbjf_step_rows)."""
    return _exact(logits, x, q_lo, q_step, rows, E, seed, offset, out, want_probs, probs, changed)


def midpoint_predict(branch, logit_type, logits, x, qt0, base_rate, beta, eps, h):
    return _midpoint(branch, logit_type, logits, x, qt0, base_rate, beta, eps, h)


def midpoint_predict_rows(branch, logit_type, logits, x, qt0, base_rate, beta, eps, h, rows, out=None):
    """midpoint_predict on the listed rows: every other row of the result is `out` as given (default: a copy of x, i.e. x' = x)."""
    return _midpoint(branch, logit_type, logits, x, qt0, base_rate, beta, eps, h, rows, out)


def lbjf_from_rates(rates, x, h, E=None, seed=0, offset=0, want_probs=False, changed=None):
    """LBJF posterior + draw on masked reverse rates (N, D, S) that are already computed (tauleap_step_s256(want_rates=True))."""
    return _lbjf_rates(rates, x, h, None, E, seed, offset, None, want_probs, None, changed)


def lbjf_from_rates_rows(rates, x, h, rows, E=None, seed=0, offset=0, out=None, want_probs=False, probs=None, changed=None):
    """lbjf_from_rates on the listed rows: `rates` (N, D, S) is read at the listed rows only (what
    tauleap_step_s256_rows(want_rates=True) wrote there)."""
    return _lbjf_rates(rates, x, h, rows, E, seed, offset, out, want_probs, probs, changed)


def midpoint_from_rates(rates, x, h):
    return _midpoint_rates(rates, x, h)


def midpoint_from_rates_rows(rates, x, h, rows, out=None):
    """midpoint_from_rates on the listed rows (see midpoint_predict_rows, lbjf_from_rates_rows)."""
    return _midpoint_rates(rates, x, h, rows, out)


def argmax(logits):
    N, D, S = logits.shape
    out = torch.empty((N, D), dtype=i32, device=logits.device)
    _check(load().ctdd_argmax(_ptr(logits, f32, "logits"), N, D, S, _ptr(out), _stream()), "ctdd_argmax")
    return out


def initial_samples(N, D, S, device, seed, offset, cdf=None):
    out = torch.empty((N, D), dtype=i32, device=device)
    if not out.is_cuda:
        raise CtddError("initial_samples: device must be a GPU")
    _check(load().ctdd_initial_samples(_ptr(cdf, f32, "cdf"), seed, offset, N, D, S, _ptr(out), _stream()),
           "ctdd_initial_samples")
    return out


def philox_uniform(seed, offset, nrows, nblk, device):
    out = torch.empty((nrows, nblk * 4), dtype=f32, device=device)
    _check(load().ctdd_philox_uniform(seed, offset, nrows, nblk, _ptr(out), _stream()), "ctdd_philox_uniform")
    return out


def dropout_seed():
    """Seed of a network's dropout stream: drawn from torch's CPU generator (reproducible under torch.manual_seed) and mixed with
    the data-parallel rank, so that ranks seeded alike still drop different units."""
    seed = int(torch.randint(0, 2**62, (1,), dtype=torch.int64).item())
    try:
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized():
            seed = (seed + dist.get_rank() * 0x9E3779B97F4A7C15) % (2**62)
    except Exception:
        pass
    return seed


def logprob_bwd(logit_type, logits, qt0, qt0T, dll, x0=None, nll_scale=0.0, ll_all=None):
    """d/dlogits of ll_all = get_logprob_with_logits(logits) for the reverse logit types given dll = d loss / d ll_all;
    x0: also the cross-entropy term nll_scale * sum -log_softmax(logits)[x0] (gradient added, value returned).
    ll_all (the forward's output) given, reverse_prob, S % 32 == 0: the matrix-core path."""
    B, D, S = logits.shape
    grad = torch.empty_like(logits)
    ce_rows = torch.zeros((B * D,), dtype=torch.float64, device=logits.device) if x0 is not None else None
    out_ce = torch.zeros((1,), dtype=torch.float32, device=logits.device)
    if ll_all is not None and _rp_mfma_ok(logit_type, logits, qt0):
        scratch = torch.empty((2,) + tuple(logits.shape), dtype=torch.float32, device=logits.device)
        _check(load().ctdd_logprob_rp_bwd_mfma(_ptr(logits, torch.float32, "logits"), _ptr(qt0, torch.float32, "qt0"), _ptr(ll_all, torch.float32, "ll_all"),
                                               _ptr(dll, torch.float32, "dll"), _ptr(x0, torch.int32, "x0") if x0 is not None else None,
                                               float(nll_scale), B, D, S, _ptr(scratch), _ptr(grad), _ptr(ce_rows) if ce_rows is not None else None,
                                               _ptr(out_ce), _stream()), "ctdd_logprob_rp_bwd_mfma")
        _count("ctdd_logprob_bwd")
        return grad, out_ce[0]
    _check(load().ctdd_logprob_bwd(LOGIT_TYPES[logit_type], _ptr(logits, torch.float32, "logits"), _ptr(qt0, torch.float32, "qt0"),
                                   _ptr(qt0T, torch.float32, "qt0T"), _ptr(dll, torch.float32, "dll"),
                                   _ptr(x0, torch.int32, "x0") if x0 is not None else None, float(nll_scale), B, D, S, _ptr(grad),
                                   _ptr(ce_rows) if ce_rows is not None else None, _ptr(out_ce), _stream()), "ctdd_logprob_bwd")
    _count("ctdd_logprob_bwd")
    return grad, out_ce[0]


def d3pm_loss(logits, x0, xt, t, qprev, qprevT, q1T, eps, vb_scale, ce_scale, want_grad=True):
    """D3PM objective (csrc/d3pm.hip): (loss, vb, ce) per sample, each (B,), in bits per dimension, and d loss_b / d logits[b]
    (B, D, S) (None without `want_grad`).  Tables per sample (B, S, S): Qbar_{t-1}, its transpose, Q_t^T."""
    if logits.dim() != 3:
        raise CtddError(f"d3pm_loss: logits {tuple(logits.shape)}, expected (B, D, S)")
    B, D, S = logits.shape
    if tuple(x0.shape) != (B, D) or tuple(xt.shape) != (B, D) or tuple(t.shape) != (B,):
        raise CtddError(f"d3pm_loss: x0 {tuple(x0.shape)} / xt {tuple(xt.shape)} / t {tuple(t.shape)} against logits {tuple(logits.shape)}")
    for name, tab in (("qprev", qprev), ("qprevT", qprevT), ("q1T", q1T)):
        if tuple(tab.shape) != (B, S, S):
            raise CtddError(f"d3pm_loss: {name} {tuple(tab.shape)}, expected {(B, S, S)}")
    lib = load()
    dev = logits.device
    scratch = torch.empty((int(lib.ctdd_d3pm_scratch_bytes(B, D, S)),), dtype=torch.uint8, device=dev)
    grad = torch.empty_like(logits) if want_grad else None
    out = torch.empty((3, B), dtype=f32, device=dev)
    _count("ctdd_d3pm_loss")
    _check(lib.ctdd_d3pm_loss(_ptr(logits, f32, "logits"), _ptr(x0, i32, "x0"), _ptr(xt, i32, "xt"), _ptr(t, i32, "t"),
                              _ptr(qprev, f32, "qprev"), _ptr(qprevT, f32, "qprevT"), _ptr(q1T, f32, "q1T"), B, D, S, float(eps),
                              float(vb_scale), float(ce_scale), _ptr(scratch), _ptr(grad), _ptr(out[0]), _ptr(out[1]), _ptr(out[2]),
                              _stream()), "ctdd_d3pm_loss")
    return out[0], out[1], out[2], grad


def d3pm_step(logits, x, qprev, qprevT, q1T, t, eps, noise=None, seed=0, offset=0, want_logits=False):
    """One D3PM ancestral step at one `t` for the whole batch (csrc/d3pm.hip): x_{t-1} (N, D) int32 [, the model logits].
    Tables (S, S): Qbar_{max(t-1, 0)}, its transpose, Q_t^T.  noise (N, D, S) uniforms, or None for the rows' Philox streams."""
    if logits.dim() != 3:
        raise CtddError(f"d3pm_step: logits {tuple(logits.shape)}, expected (N, D, S)")
    N, D, S = logits.shape
    if tuple(x.shape) != (N, D):
        raise CtddError(f"d3pm_step: x {tuple(x.shape)} against logits {tuple(logits.shape)}")
    for name, tab in (("qprev", qprev), ("qprevT", qprevT), ("q1T", q1T)):
        if tuple(tab.shape) != (S, S):
            raise CtddError(f"d3pm_step: {name} {tuple(tab.shape)}, expected {(S, S)}")
    if noise is not None and tuple(noise.shape) != (N, D, S):
        raise CtddError(f"d3pm_step: noise {tuple(noise.shape)}, expected {(N, D, S)}")
    dev = logits.device
    scratch = torch.empty((2, N, D, S), dtype=f32, device=dev) if S % 32 == 0 and int(t) != 0 else None
    out = torch.empty((N, D), dtype=i32, device=dev)
    model = torch.empty((N, D, S), dtype=f32, device=dev) if want_logits else None
    _count("ctdd_d3pm_step")
    _check(load().ctdd_d3pm_step(_ptr(logits, f32, "logits"), _ptr(x, i32, "x"), _ptr(qprev, f32, "qprev"), _ptr(qprevT, f32, "qprevT"),
                                 _ptr(q1T, f32, "q1T"), int(t), N, D, S, float(eps), _ptr(noise, f32, "noise"), int(seed), int(offset),
                                 _ptr(scratch), _ptr(out), _ptr(model), _stream()), "ctdd_d3pm_step")
    return (out, model) if want_logits else out


# ---------------------------------------------------------------- absorbing-state diffusion (csrc/absorb.hip, include/ctdd_absorb.h)
ABSORB_ARGMAX = 1
ABSORB_MAX_S = 1024          # CTDD_MAX_S


def _absorb_shapes(what, logits, states):
    """(B, D, S) of fp32 logits (B, D, S) against int32 states (B, D) each, given as (name, tensor) pairs."""
    if not isinstance(logits, torch.Tensor) or logits.dim() != 3:
        raise CtddError(f"{what}: logits {tuple(getattr(logits, 'shape', ()))}, expected (B, D, S)")
    B, D, S = (int(v) for v in logits.shape)
    for name, x in states:
        if not isinstance(x, torch.Tensor) or tuple(x.shape) != (B, D):
            raise CtddError(f"{what}: {name} {tuple(getattr(x, 'shape', ()))} against logits {tuple(logits.shape)}")
    return B, D, S


def absorb_noise(x0, alpha, mask_state, seed=0, offset=0):
    """x_t (B, D) int32: entry (b, d) is mask_state iff its Philox uniform is >= alpha[b], else x0 (ctdd_absorb_noise)."""
    if not isinstance(x0, torch.Tensor) or x0.dim() != 2 or not isinstance(alpha, torch.Tensor) or tuple(alpha.shape) != (x0.shape[0],):
        raise CtddError(f"absorb_noise: x0 {tuple(getattr(x0, 'shape', ()))} / alpha {tuple(getattr(alpha, 'shape', ()))}, expected (B, D) / (B,)")
    B, D = (int(v) for v in x0.shape)
    out = torch.empty_like(x0) if x0.is_cuda else None
    _count("ctdd_absorb_noise")
    _check(load().ctdd_absorb_noise(_ptr(x0, i32, "x0"), _ptr(alpha, f32, "alpha"), B, D, int(mask_state), int(seed), int(offset), _ptr(out),
                                    _stream()), "ctdd_absorb_noise")
    return out


def absorb_elbo_loss(logits, x0, xt, w, nll_scale, mask_state, want_grad=True):
    """(value (0-d fp32), d value / d logits (B, D, S) or None): the absorbing-state negative ELBO
    (1/B) sum_b w[b] sum_{d masked} -lp[x0] + nll_scale sum_{rows} -lp[x0] with the softmax over s != mask_state."""
    B, D, S = _absorb_shapes("absorb_elbo_loss", logits, (("x0", x0), ("xt", xt)))
    if not isinstance(w, torch.Tensor) or tuple(w.shape) != (B,):
        raise CtddError(f"absorb_elbo_loss: w {tuple(getattr(w, 'shape', ()))}, expected {(B,)}")
    ptrs = (_ptr(logits, f32, "logits"), _ptr(x0, i32, "x0"), _ptr(xt, i32, "xt"), _ptr(w, f32, "w"))
    lib, dev = load(), logits.device
    scratch = torch.zeros((int(lib.ctdd_absorb_scratch_bytes()),), dtype=torch.uint8, device=dev)
    out = torch.zeros((1,), dtype=f32, device=dev)
    grad = torch.empty_like(logits) if want_grad else None
    _count("ctdd_absorb_elbo_loss")
    _check(lib.ctdd_absorb_elbo_loss(*ptrs, float(nll_scale), B, D, S, int(mask_state), _ptr(scratch), _ptr(out), _ptr(grad), _stream()),
           "ctdd_absorb_elbo_loss")
    return out[0], grad


def absorb_step(logits, x, mask_state, p_unmask, flags=0, seed=0, offset=0, out=None, changed=None):
    """One reverse step (ctdd_absorb_step): rows of x (N, D) int32 at mask_state unmask with probability p_unmask to a draw from
    the softmax over s != mask_state (flags = ABSORB_ARGMAX: all of them, to its argmax); the others are copied through.
    changed: int32[1] device counter of the rows that left the mask state, incremented."""
    N, D, S = _absorb_shapes("absorb_step", logits, (("x", x),))
    ptrs = (_ptr(logits, f32, "logits"), _ptr(x, i32, "x"))
    if out is None:
        out = torch.empty_like(x)
    _count("ctdd_absorb_step")
    _check(load().ctdd_absorb_step(*ptrs, N, D, S, int(mask_state), float(p_unmask), int(flags), int(seed), int(offset), _ptr(out, i32, "out"),
                                   _ptr(changed, i32, "changed"), _stream()), "ctdd_absorb_step")
    return out


def absorb_propose(logits, x, mask_state, noise=0.0, flags=0, seed=0, offset=0):
    """(cand int32 (N, D), score fp32 (N, D)) of the rows of x at mask_state (ctdd_absorb_propose): the state ctdd_absorb_step
    would draw for the same (seed, offset) (flags = ABSORB_ARGMAX: the argmax) and its log-probability under the softmax over
    s != mask_state, plus noise times a standard Gumbel variate when noise != 0.  Entries of the other rows are not written."""
    N, D, S = _absorb_shapes("absorb_propose", logits, (("x", x),))
    ptrs = (_ptr(logits, f32, "logits"), _ptr(x, i32, "x"))
    cand, score = torch.empty_like(x), torch.empty(x.shape, dtype=f32, device=x.device)
    _count("ctdd_absorb_propose")
    _check(load().ctdd_absorb_propose(*ptrs, N, D, S, int(mask_state), float(noise), int(flags), int(seed), int(offset), _ptr(cand),
                                      _ptr(score), _stream()), "ctdd_absorb_propose")
    return cand, score


def absorb_commit(x, cand, score, mask_state, p_unmask=None, counts=None, out=None, changed=None):
    """x with, per sample n, the k_n rows at mask_state that have the largest score set to cand (ctdd_absorb_commit; ties in
    ascending d, NaN below -inf).  Exactly one of p_unmask (k_n = ceil(p_unmask M_n) over the sample's M_n masked rows) and counts
    (int32 (N,) on the device, k_n = counts[n] clamped to [0, M_n]).  changed: int32[1] device counter, incremented by sum k_n."""
    if not isinstance(x, torch.Tensor) or x.dim() != 2:
        raise CtddError(f"absorb_commit: x {tuple(getattr(x, 'shape', ()))}, expected (N, D)")
    N, D = (int(v) for v in x.shape)
    for name, t in (("cand", cand), ("score", score)):
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != (N, D):
            raise CtddError(f"absorb_commit: {name} {tuple(getattr(t, 'shape', ()))} against x {(N, D)}")
    if (p_unmask is None) == (counts is None):
        raise CtddError("absorb_commit: exactly one of p_unmask and counts")
    if counts is not None and (not isinstance(counts, torch.Tensor) or tuple(counts.shape) != (N,)):
        raise CtddError(f"absorb_commit: counts {tuple(getattr(counts, 'shape', ()))}, expected {(N,)}")
    ptrs = (_ptr(x, i32, "x"), _ptr(cand, i32, "cand"), _ptr(score, f32, "score"))
    if out is None:
        out = torch.empty_like(x)
    elif not isinstance(out, torch.Tensor) or tuple(out.shape) != (N, D):
        raise CtddError(f"absorb_commit: out {tuple(getattr(out, 'shape', ()))} against x {(N, D)}")
    _count("ctdd_absorb_commit")
    _check(load().ctdd_absorb_commit(*ptrs, N, D, int(mask_state), 0.0 if p_unmask is None else float(p_unmask), _ptr(counts, i32, "counts"),
                                     _ptr(out, i32, "out"), _ptr(changed, i32, "changed"), _stream()), "ctdd_absorb_commit")
    return out


def absorb_nll(logits, x0, xt, mask_state, w=None, out=None, masked=None, hit=None):
    """(row_nll fp32 (N, D), out fp64 (N,)): -log p(x0) under the softmax over s != mask_state at every row with xt == mask_state
    (and x0 a real state), exact 0 at the others, which are not read; out[n] += w[n] * sum_d row_nll[n][d] in fp64, in a fixed order
    (ctdd_absorb_nll: repeated calls give the same bits).  w: fp32 (N,) or None (1).  out: fp64 (N,), e.g. a row of a (K, N) buffer, is
    accumulated into (None: a fresh zeroed one).  masked / hit: int32 (N,) device counters, incremented by the sample's rows with a
    term / by those of them whose argmax over s != mask_state (lowest index on ties) is x0."""
    N, D, S = _absorb_shapes("absorb_nll", logits, (("x0", x0), ("xt", xt)))
    for name, t in (("w", w), ("out", out), ("masked", masked), ("hit", hit)):
        if t is not None and (not isinstance(t, torch.Tensor) or tuple(t.shape) != (N,)):
            raise CtddError(f"absorb_nll: {name} {tuple(getattr(t, 'shape', ()))}, expected {(N,)}")
    ptrs = (_ptr(logits, f32, "logits"), _ptr(x0, i32, "x0"), _ptr(xt, i32, "xt"), _ptr(w, f32, "w"))
    if out is None:
        out = torch.zeros((N,), dtype=torch.float64, device=logits.device)
    row = torch.empty((N, D), dtype=f32, device=logits.device)
    tail = (_ptr(row), _ptr(out, torch.float64, "out"), _ptr(masked, i32, "masked"), _ptr(hit, i32, "hit"))
    _count("ctdd_absorb_nll")
    _check(load().ctdd_absorb_nll(*ptrs, N, D, S, int(mask_state), *tail, _stream()), "ctdd_absorb_nll")
    return row, out


ABSORB_REMASK_CONF = 2


def _held_mask(held, N, D, what):
    """The (N, D) mask of held entries as the kernels read it: uint8 (a bool tensor is reinterpreted, not copied), or None."""
    if held is None:
        return None
    if not isinstance(held, torch.Tensor) or held.dtype not in (torch.bool, torch.uint8):
        raise CtddError(f"{what}: held must be a bool or uint8 tensor, got {getattr(held, 'dtype', type(held))}")
    if tuple(held.shape) != (N, D):
        raise CtddError(f"{what}: held {tuple(held.shape)} against states {(N, D)}")
    return _ptr(held.view(torch.uint8) if held.dtype == torch.bool else held, torch.uint8, "held")


def absorb_remask_step(logits, x, mask_state, p_unmask, sigma, held=None, conf=None, norm=None, temp=1.0, flags=0, seed=0, offset=0, out=None,
                       conf_out=None, counts=None):
    """(out_x, conf_out or None): one reverse step with remasking (ctdd_absorb_remask_step).  A masked free row follows absorb_step's
    rule with p_unmask (the same state under the same seed and offset); a free unmasked row returns to mask_state with probability
    sigma (flags = ABSORB_REMASK_CONF: sigma U_n exp(-conf / temp) / Z_n, clamped at 1, (U_n, Z_n) = norm[n] from absorb_remask_norm);
    a held row (held (N, D) bool / uint8) is copied through.  conf: fp32 (N, D), the probability at which each entry committed; given,
    conf_out (default a fresh tensor; conf itself for an in-place call) takes that probability for a row that unmasks, 0 for a row
    that is or becomes masked, conf's bits otherwise.  out may be x.  counts: int32[2] device counters, incremented by the rows that
    left the mask state and by the rows remasked."""
    N, D, S = _absorb_shapes("absorb_remask_step", logits, (("x", x),))
    hp = _held_mask(held, N, D, "absorb_remask_step")
    for name, t in (("conf", conf), ("conf_out", conf_out), ("out", out)):
        if t is not None and (not isinstance(t, torch.Tensor) or tuple(t.shape) != (N, D)):
            raise CtddError(f"absorb_remask_step: {name} {tuple(getattr(t, 'shape', ()))} against x {(N, D)}")
    if norm is not None and (not isinstance(norm, torch.Tensor) or tuple(norm.shape) != (N, 2)):
        raise CtddError(f"absorb_remask_step: norm {tuple(getattr(norm, 'shape', ()))}, expected {(N, 2)}")
    if counts is not None and (not isinstance(counts, torch.Tensor) or tuple(counts.shape) != (2,)):
        raise CtddError(f"absorb_remask_step: counts {tuple(getattr(counts, 'shape', ()))}, expected (2,)")
    if conf is None and conf_out is not None:
        raise CtddError("absorb_remask_step: conf_out without conf")
    ptrs = (_ptr(logits, f32, "logits"), _ptr(x, i32, "x"), hp, _ptr(conf, f32, "conf"), _ptr(norm, f32, "norm"))
    if out is None:
        out = torch.empty_like(x)
    if conf is not None and conf_out is None:
        conf_out = torch.empty_like(conf)
    _count("ctdd_absorb_remask_step")
    _check(load().ctdd_absorb_remask_step(*ptrs, N, D, S, int(mask_state), float(p_unmask), float(sigma), float(temp), int(flags), int(seed),
                                          int(offset), _ptr(out, i32, "out"), _ptr(conf_out, f32, "conf_out"), _ptr(counts, i32, "counts"),
                                          _stream()), "ctdd_absorb_remask_step")
    return out, conf_out


def absorb_remask_norm(x, mask_state, conf, held=None, temp=1.0, out=None):
    """norm fp32 (N, 2) = (U_n, Z_n) per sample (ctdd_absorb_remask_norm): the number of free unmasked entries of x (N, D) -- not at
    mask_state, not held -- and the sum of exp(-conf / temp) over them, in a fixed order (repeated calls give the same bits); (0, 0)
    for a sample without one."""
    if not isinstance(x, torch.Tensor) or x.dim() != 2:
        raise CtddError(f"absorb_remask_norm: x {tuple(getattr(x, 'shape', ()))}, expected (N, D)")
    N, D = (int(v) for v in x.shape)
    if not isinstance(conf, torch.Tensor) or tuple(conf.shape) != (N, D):
        raise CtddError(f"absorb_remask_norm: conf {tuple(getattr(conf, 'shape', ()))} against x {(N, D)}")
    hp = _held_mask(held, N, D, "absorb_remask_norm")
    ptrs = (_ptr(x, i32, "x"), hp, _ptr(conf, f32, "conf"))
    if out is None:
        out = torch.empty((N, 2), dtype=f32, device=x.device)
    elif not isinstance(out, torch.Tensor) or tuple(out.shape) != (N, 2):
        raise CtddError(f"absorb_remask_norm: out {tuple(getattr(out, 'shape', ()))}, expected {(N, 2)}")
    _count("ctdd_absorb_remask_norm")
    _check(load().ctdd_absorb_remask_norm(*ptrs, N, D, int(mask_state), float(temp), _ptr(out, f32, "out"), _stream()), "ctdd_absorb_remask_norm")
    return out


ABSORB_T_FUNCS = {"loglinear": 0, "log_sqr": 1, "sqrt_cos": 2, "log": 3}      # CTDD_ABSORB_T_*


def absorb_hit_time(x, logc, mask_state, kmax, log_cmin, schedule, t_min, t_max, seed=0, offset=0, counts=None, t_eval=None, out=None):
    """(counts int32 (N,), t_eval fp32 (N,), logc_out fp64 (N,)): the first-hitting events of one step, per sample
    (ctdd_absorb_hit_time).  With M_n entries of x[n] (x (N, D) int32) at mask_state and the log level logc[n] (fp64 (N,)), up to
    min(kmax, M_n) events L <- L + log(u) / (M_n - i) are taken while L stays at or above log_cmin (a float, -inf allowed); counts:
    how many; logc_out: the level after them (log_cmin once an event was refused); t_eval: the time of the first event's level,
    clamped to [t_min, t_max] (t_min without an event).  schedule: the absorbing process's parameters (DeviceForwardProcess.p:
    t_func, rate_const and alpha_eps or time_base / time_exp as the t_func needs).  out: logc itself for an in-place call."""
    if not isinstance(x, torch.Tensor) or x.dim() != 2:
        raise CtddError(f"absorb_hit_time: x {tuple(getattr(x, 'shape', ()))}, expected (N, D)")
    N, D = (int(v) for v in x.shape)
    for name, t in (("logc", logc), ("counts", counts), ("t_eval", t_eval), ("out", out)):
        if (t is not None or name == "logc") and (not isinstance(t, torch.Tensor) or tuple(t.shape) != (N,)):
            raise CtddError(f"absorb_hit_time: {name} {tuple(getattr(t, 'shape', ()))}, expected {(N,)}")
    f = schedule.get("t_func")
    if f not in ABSORB_T_FUNCS:
        raise CtddError(f"absorb_hit_time: t_func {f!r}, expected one of {tuple(ABSORB_T_FUNCS)}")
    par = [float(schedule.get(k, 0.0)) for k in ("rate_const", "alpha_eps", "time_base", "time_exp")]
    ptrs = (_ptr(x, i32, "x"), _ptr(logc, torch.float64, "logc"))
    if counts is None:
        counts = torch.empty((N,), dtype=i32, device=x.device)
    if t_eval is None:
        t_eval = torch.empty((N,), dtype=f32, device=x.device)
    if out is None:
        out = torch.empty_like(logc)
    _count("ctdd_absorb_hit_time")
    _check(load().ctdd_absorb_hit_time(*ptrs, N, D, int(mask_state), int(kmax), float(log_cmin), ABSORB_T_FUNCS[f], *par, float(t_min),
                                       float(t_max), int(seed), int(offset), _ptr(counts, i32, "counts"), _ptr(t_eval, f32, "t_eval"),
                                       _ptr(out, torch.float64, "out"), _stream()), "ctdd_absorb_hit_time")
    return counts, t_eval, out


def absorb_hit_step(logits, x, counts, mask_state, flags=0, seed=0, offset=0, out=None, changed=None):
    """x with, per sample n, k_n = counts[n] (int32 (N,) on the device, clamped to [0, M_n]) of its M_n rows at mask_state, drawn
    uniformly without replacement from Philox keys, set to the state absorb_step draws for the row at p_unmask = 1 under the same
    seed and offset (flags = ABSORB_ARGMAX: its argmax); every other row is copied and its logits are not read
    (ctdd_absorb_hit_step).  out may be x.  changed: int32[1] device counter, incremented by sum k_n."""
    N, D, S = _absorb_shapes("absorb_hit_step", logits, (("x", x),))
    if not isinstance(counts, torch.Tensor) or tuple(counts.shape) != (N,):
        raise CtddError(f"absorb_hit_step: counts {tuple(getattr(counts, 'shape', ()))}, expected {(N,)}")
    if out is not None and (not isinstance(out, torch.Tensor) or tuple(out.shape) != (N, D)):
        raise CtddError(f"absorb_hit_step: out {tuple(getattr(out, 'shape', ()))} against x {(N, D)}")
    ptrs = (_ptr(logits, f32, "logits"), _ptr(x, i32, "x"), _ptr(counts, i32, "counts"))
    if out is None:
        out = torch.empty_like(x)
    _count("ctdd_absorb_hit_step")
    _check(load().ctdd_absorb_hit_step(*ptrs, N, D, S, int(mask_state), int(flags), int(seed), int(offset), _ptr(out, i32, "out"),
                                       _ptr(changed, i32, "changed"), _stream()), "ctdd_absorb_hit_step")
    return out


def absorb_filter_is_neutral(temperature=1.0, top_k=0, top_p=1.0):
    """Whether (temperature, top_k, top_p) leave every distribution as it is: the samplers launch nothing then."""
    return float(temperature) == 1.0 and int(top_k) == 0 and float(top_p) == 1.0


def absorb_filter(logits, x, mask_state, temperature=1.0, top_k=0, top_p=1.0, out=None):
    """logits (N, D, S) fp32 with the rows of x (N, D) int32 at mask_state tempered and truncated (ctdd_absorb_filter): over the
    states s != mask_state, v = l / temperature; ordered by (v descending, s ascending), the first top_k stay (0: all), then the
    shortest prefix whose softmax mass reaches top_p (1: all; one state at least); a state that stays gets v, every other one and the
    mask state's column -inf, so the step kernels draw from the truncated, renormalised distribution.  A row without a finite real-state
    logit comes back as it was.  The other rows are neither read nor written.  out: logits itself for the in-place call; None returns a
    copy of logits with the masked rows rewritten."""
    N, D, S = _absorb_shapes("absorb_filter", logits, (("x", x),))
    ptrs = (_ptr(logits, f32, "logits"), _ptr(x, i32, "x"))
    if out is None:
        out = logits.clone()
    elif not isinstance(out, torch.Tensor) or tuple(out.shape) != (N, D, S):
        raise CtddError(f"absorb_filter: out {tuple(getattr(out, 'shape', ()))} against logits {(N, D, S)}")
    elif out.data_ptr() != logits.data_ptr() and abs(out.data_ptr() - logits.data_ptr()) < 4 * N * D * S:
        raise CtddError("absorb_filter: out overlaps logits without being it")
    _count("ctdd_absorb_filter")
    _check(load().ctdd_absorb_filter(*ptrs, N, D, S, int(mask_state), float(temperature), min(int(top_k), S), float(top_p), _ptr(out, f32, "out"),
                                     _stream()), "ctdd_absorb_filter")
    return out


# ---------------------------------------------------------------- the fused training objectives (csrc/losses.hip)
# One routine per family -- CT-ELBO (K11), CRM (K12), ScoreElbo -- behind the public wrappers, which only name their ABI entry and pass
# its optional parts: a mask of free rows, a row window, the ll_all form of the reverse logit types.
_CRM_TYPES = {"rm": 0, "mle": 1, "elbo": 2}


def _loss_operands(what, first, logits, states, tables, grad_out, width=None):
    """Host checks shared by the objectives, on shapes alone (no copy, no synchronisation): `logits` (B, Dl, S), named `first` in
    messages; `states` (B, D) each and `tables` (B, S, S) each as (name, tensor) pairs, None skipped; D = Dl unless `width` names
    the operand whose second extent it is (the row window).  Returns (B, D, S, gradient buffer)."""
    if not isinstance(logits, torch.Tensor) or logits.dim() != 3:
        raise CtddError(f"{what}: {first} {tuple(getattr(logits, 'shape', ()))}, expected (B, D, S)")
    B, D, S = logits.shape
    like = ""
    if width is not None and width[1].dim() == 2:
        D, like = int(width[1].shape[1]), f" (the window is {width[0]}'s, {tuple(width[1].shape)})"
    for name, x in states:
        if x is not None and tuple(x.shape) != (B, D):
            raise CtddError(f"{what}: {name} {tuple(x.shape)}, expected {(B, D)}{like}")
    for name, tab in tables:
        if tab is not None and tuple(tab.shape) != (B, S, S):
            raise CtddError(f"{what}: {name} {tuple(tab.shape)}, expected {(B, S, S)}")
    grad = torch.empty_like(logits) if grad_out is None else grad_out
    if grad.shape != logits.shape:
        raise CtddError(f"{what}: grad_out {tuple(grad.shape)} against {first} {tuple(logits.shape)}")
    return B, D, S, grad


def _seq_free_mask(free, logits, B, D, what):
    """_free_mask for the sequence objectives, which take a bool mask on the logits' device only."""
    if not isinstance(free, torch.Tensor) or free.dtype != torch.bool:
        raise CtddError(f"{what}: free must be a bool tensor, got {getattr(free, 'dtype', type(free))}")
    if free.device != logits.device:
        raise CtddError(f"{what}: free on {free.device}, logits on {logits.device}")
    return _free_mask(free, B, D, what)


def _ctelbo(name, logits, x0, x_tilde, qt0, qt0T, rate, eps, scales, nll_scale, free=None, d_off=None, grad_out=None):
    """The four ctdd_ctelbo_loss* entries: `scales` the term weights the entry takes, `free` for _masked, `d_off` for _window."""
    what = name[5:]
    B, D, S, grad = _loss_operands(what, "logits", logits, (("x0", x0), ("x_tilde", x_tilde)), (("qt0", qt0), ("qt0T", qt0T), ("rate", rate)),
                                   grad_out, width=None if d_off is None else ("x0", x0))
    mask, window = (), ()
    if name.endswith("_masked"):
        mask = (_free_mask(free, B, D, what),)
    if d_off is not None:
        Dl = logits.shape[1]
        if not (0 <= int(d_off) and D >= 1 and int(d_off) + D <= Dl):
            raise CtddError(f"{what}: rows [{d_off}, {d_off} + {D}) of {Dl}")
        window = (Dl, int(d_off))
    head = (_ptr(logits, f32, "logits"), _ptr(x0, i32, "x0"), _ptr(x_tilde, i32, "x_tilde"), *mask, _ptr(qt0, f32, "qt0"),
            _ptr(qt0T, f32, "qt0T"), _ptr(rate, f32, "rate"), B, D, S, *window, float(eps), *map(float, scales), float(nll_scale))
    lib = load()
    scratch = torch.empty((int(lib.ctdd_ctelbo_scratch_bytes(B, D, S)),), dtype=torch.uint8, device=logits.device)
    out = torch.empty((1,), dtype=f32, device=logits.device)
    _check(getattr(lib, name)(*head, _ptr(scratch), _ptr(grad, f32, "grad_out"), _ptr(out), _stream()), name)
    _count(name)                                   # (a call the library accepted)
    return out[0], grad


def _crm(name, logits, xt, x0, free, qt0, loss_type, scale, nll_scale, grad_out=None):
    """The four ctdd_crm_loss* entries: the _ll ones take ll_all for the logits and have no x0 / nll_scale; `free` for _masked."""
    what, ll = name[5:], "_loss_ll" in name
    first = "ll_all" if ll else "logits"
    B, D, S, grad = _loss_operands(what, first, logits, (("xt", xt), ("x0", x0)), (("qt0", qt0),), grad_out)
    mask = (_seq_free_mask(free, logits, B, D, what),) if name.endswith("_masked") else ()
    ce, nll = ((), ()) if ll else ((_ptr(x0, i32, "x0"),), (float(nll_scale),))
    head = (_ptr(logits, f32, first), _ptr(xt, i32, "xt"), *ce, *mask, _ptr(qt0, f32, "qt0"), B, D, S, _CRM_TYPES[loss_type],
            float(scale), *nll)
    rows = torch.empty((B * D,), dtype=torch.float64, device=logits.device)
    out = torch.empty((1,), dtype=f32, device=logits.device)
    _check(getattr(load(), name)(*head, _ptr(grad, f32, "grad_out"), _ptr(rows), _ptr(out), _stream()), name)
    _count(name)                                   # (a call the library accepted)
    return out[0], grad


def _score_elbo(name, logits, x0, x_tilde, reg_x, free, qt0, rate, eps, nll_scale, grad_out=None):
    """The four ctdd_score_elbo_loss* entries: the _ll ones take ll_all for the logits; `free` for _masked."""
    what, first = name[5:], "ll_all" if "_loss_ll" in name else "logits"
    B, D, S, grad = _loss_operands(what, first, logits, (("x0", x0), ("x_tilde", x_tilde), ("reg_x", reg_x)),
                                   (("qt0", qt0), ("rate", rate)), grad_out)
    mask = (_seq_free_mask(free, logits, B, D, what),) if name.endswith("_masked") else ()
    head = (_ptr(logits, f32, first), _ptr(x0, i32, "x0"), _ptr(x_tilde, i32, "x_tilde"), _ptr(reg_x, i32, "reg_x"), *mask,
            _ptr(qt0, f32, "qt0"), _ptr(rate, f32, "rate"), B, D, S, float(eps), float(nll_scale))
    lib = load()
    scratch = torch.empty((int(lib.ctdd_ctelbo_scratch_bytes(B, D, S)),), dtype=torch.uint8, device=logits.device)
    out = torch.empty((1,), dtype=f32, device=logits.device)
    _check(getattr(lib, name)(*head, _ptr(scratch), _ptr(grad, f32, "grad_out"), _ptr(out), _stream()), name)
    _count(name)                                   # (a call the library accepted)
    return out[0], grad


def ctelbo_loss(logits, x0, x_tilde, qt0, qt0T, rate, eps, elbo_scale, nll_scale, reg_scale=None):
    """K11: (loss scalar tensor, d loss / d logits) of the tauLDR CT-ELBO.  `reg_scale` None: the one-forward-pass objective
    (both ELBO terms weighted `elbo_scale`); otherwise the signal term is weighted `elbo_scale` and the regulariser
    `reg_scale`, every term evaluated at the state passed as `x_tilde` (one half of the two-forward-pass objective)."""
    if reg_scale is None:
        return _ctelbo("ctdd_ctelbo_loss", logits, x0, x_tilde, qt0, qt0T, rate, eps, (elbo_scale,), nll_scale)
    return _ctelbo("ctdd_ctelbo_loss_terms", logits, x0, x_tilde, qt0, qt0T, rate, eps, (elbo_scale, reg_scale), nll_scale)


def ctelbo_loss_window(logits_full, x0, x_tilde, qt0, qt0T, rate, eps, sig_scale, reg_scale, nll_scale, d_off, grad_out=None):
    """K11 on rows [d_off, d_off + D) of the (B, Dl, S) logits, read in place; x0 / x_tilde are the compact (B, D) window.
    Returns (loss scalar tensor, d loss / d logits_full): full shape, zeros on the rows outside the window, every element
    written by the call (`grad_out`: write into this (B, Dl, S) buffer instead of a fresh one).  Terms and weights as
    ctelbo_loss with `reg_scale` given."""
    return _ctelbo("ctdd_ctelbo_loss_window", logits_full, x0, x_tilde, qt0, qt0T, rate, eps, (sig_scale, reg_scale), nll_scale,
                   d_off=d_off, grad_out=grad_out)


def ctelbo_loss_masked(logits, x0, x_tilde, free, qt0, qt0T, rate, eps, sig_scale, reg_scale, nll_scale, grad_out=None):
    """K11 on the free rows of every sample (`free` (B, D) bool / uint8; logits (B, D, S) read in place, x0 / x_tilde full shape).
    Returns (loss scalar tensor, d loss / d logits): full shape, exact zeros on held rows, every element written by the call
    (`grad_out`: write into this buffer instead of a fresh one).  Terms and weights as ctelbo_loss with `reg_scale` given."""
    return _ctelbo("ctdd_ctelbo_loss_masked", logits, x0, x_tilde, qt0, qt0T, rate, eps, (sig_scale, reg_scale), nll_scale,
                   free=free, grad_out=grad_out)


def crm_loss(logits, xt, x0, qt0, loss_type, scale, nll_scale):
    """K12: (loss scalar tensor, d loss / d logits) for the CRM objectives with direct logits."""
    return _crm("ctdd_crm_loss", logits, xt, x0, None, qt0, loss_type, scale, nll_scale)


def crm_loss_ll(ll_all, xt, qt0, loss_type, scale):
    """K12 on ll_all (reverse logit types): (loss scalar tensor, d loss / d ll_all)."""
    return _crm("ctdd_crm_loss_ll", ll_all, xt, None, None, qt0, loss_type, scale, 0.0)


def crm_loss_masked(logits, xt, x0, free, qt0, loss_type, scale, nll_scale, grad_out=None):
    """K12 on the free rows (`free` (B, D) bool; logits (B, D, S) read in place, xt / x0 full shape):
    scale * sum_free loss_bd + nll_scale * sum_free CE(logits_bd, x0_bd) (x0 None: no CE term).  Returns (loss scalar tensor,
    d loss / d logits): full shape, exact zeros on held rows, every element written by the call (`grad_out`: into this buffer)."""
    return _crm("ctdd_crm_loss_masked", logits, xt, x0, free, qt0, loss_type, scale, nll_scale, grad_out)


def crm_loss_ll_masked(ll_all, xt, free, qt0, loss_type, scale, grad_out=None):
    """K12 on ll_all (reverse logit types) over the free rows: (loss scalar tensor, d loss / d ll_all), zero rows where held."""
    return _crm("ctdd_crm_loss_ll_masked", ll_all, xt, None, free, qt0, loss_type, scale, 0.0, grad_out)


def score_elbo_loss(logits, x0, x_tilde, reg_x, qt0, rate, eps, nll_scale):
    """(loss scalar tensor, d loss / d logits) of ScoreElbo with direct logits."""
    return _score_elbo("ctdd_score_elbo_loss", logits, x0, x_tilde, reg_x, None, qt0, rate, eps, nll_scale)


def score_elbo_loss_ll(ll_all, x0, x_tilde, reg_x, qt0, rate, eps, nll_scale):
    """ScoreElbo on ll_all (reverse logit types): (loss scalar tensor, d loss / d ll_all)."""
    return _score_elbo("ctdd_score_elbo_loss_ll", ll_all, x0, x_tilde, reg_x, None, qt0, rate, eps, nll_scale)


def score_elbo_loss_masked(logits, x0, x_tilde, reg_x, free, qt0, rate, eps, nll_scale, grad_out=None):
    """ScoreElbo (direct logits) with every sum over dimensions restricted to the free rows of each sample (`free` (B, D) bool;
    everything else full shape; nll_scale = nll_weight / B).  Returns (loss scalar tensor, d loss / d logits): exact zeros on held
    rows, every element written by the call (`grad_out`: into this buffer).  A sample without a free row adds zero."""
    return _score_elbo("ctdd_score_elbo_loss_masked", logits, x0, x_tilde, reg_x, free, qt0, rate, eps, nll_scale, grad_out)


def score_elbo_loss_ll_masked(ll_all, x0, x_tilde, reg_x, free, qt0, rate, eps, nll_scale, grad_out=None):
    """The same on ll_all (reverse logit types): (loss scalar tensor, d loss / d ll_all), zero rows where held."""
    return _score_elbo("ctdd_score_elbo_loss_ll_masked", ll_all, x0, x_tilde, reg_x, free, qt0, rate, eps, nll_scale, grad_out)


# ---------------------------------------------------------------- S = 256 fast path
class S256Tables:
    """Derived tables for the MFMA tau-leaping kernel: per-step blocks (resident for the whole
    time grid) + the two per-model base-rate views."""

    def __init__(self, qt0, base_rate, eps, crm=False, bf16=False):
        """crm: tables of the CRM branch with logit_type reverse_prob (unit left scaling; step calls carry STEP_CRM).
        bf16: step calls carry STEP_BF16 -- one bf16 product for the S x S contraction (csrc/steps_s256_b16.hip; the mode of
        the bf16 score network, relative rate error <= 3 * 2^-8) instead of the three split-bf16 products of the parity mode."""
        self.crm = bool(crm)
        self.bf16 = bool(bf16)
        nT, S, _ = qt0.shape
        if S != 256:
            raise CtddError("S256Tables needs S == 256")
        self.block = int(load().ctdd_s256_step_table_bytes())
        dev = qt0.device
        self.steps = torch.empty((nT, self.block), dtype=torch.uint8, device=dev)
        self.RT0 = torch.empty((S, S), dtype=f32, device=dev)
        self.R0 = torch.empty((S, S), dtype=f32, device=dev)
        if self.crm:
            rc = load().ctdd_s256_prepare_crm(_ptr(qt0, f32, "qt0"), _ptr(base_rate, f32, "base_rate"), nT,
                                              _ptr(self.steps), _ptr(self.RT0), _ptr(self.R0), _stream())
        else:
            rc = load().ctdd_s256_prepare(_ptr(qt0, f32, "qt0"), _ptr(base_rate, f32, "base_rate"), float(eps), nT,
                                          _ptr(self.steps), _ptr(self.RT0), _ptr(self.R0), _stream())
        _check(rc, "ctdd_s256_prepare")

    def step_ptr(self, i):
        return self.steps.data_ptr() + i * self.block


def _tauleap_s256(logits, x, tables, i, beta, h, flags, seed, offset, rows=None, x_base=None, out=None, changed=None,
                  want_rates=False, rates=None, want_x=True):
    """The S = 256 member of the step families above (same `rows` contract).  want_rates: also the masked reverse rates, into
    `rates` (N, D, 256) f32 when given, else into a fresh uninitialised tensor.  want_x=False (with want_rates): the rates only --
    no draw, no state, the returned state is None (the first half of an S = 256 LBJF / midpoint step)."""
    N, D, S = logits.shape
    name = "ctdd_tauleap_step_s256" if rows is None else "ctdd_tauleap_step_s256_rows"
    if S != 256:
        raise CtddError(f"{name[5:]} needs S == 256")
    if not want_x and not want_rates:
        raise CtddError(f"{name[5:]}: want_x=False needs want_rates=True")
    name, rl, out = _step_entry("ctdd_tauleap_step_s256", rows, out, x, N, D, want_x)
    rates = _buffer(want_rates, rates, logits, "rates")
    bf16_logits = logits.dtype == torch.bfloat16             # (the bf16 U-Net engine's output): bf16 step only
    if bf16_logits and not tables.bf16:
        raise CtddError(f"{name[5:]}: bf16 logits need S256Tables(..., bf16=True)")
    flags = (int(flags) | (STEP_CRM if tables.crm else 0) | (STEP_BF16 if tables.bf16 else 0)
             | (STEP_LOGITS_BF16 if bf16_logits else 0))
    _launched(getattr(load(), name)(_ptr(logits, torch.bfloat16 if bf16_logits else f32, "logits"), _ptr(x, i32, "x"),
                                    _ptr(x_base, i32, "x_base"), tables.step_ptr(i), _ptr(tables.RT0), _ptr(tables.R0),
                                    float(beta), float(h), flags, seed, offset, N, D, *rl, _ptr(rates, f32, "rates"),
                                    _ptr(out, i32, "out"), _ptr(changed, i32, "changed"), _stream()), name)
    return (out, rates) if want_rates else out


def tauleap_step_s256(logits, x, tables, i, beta, h, flags, seed, offset, x_base=None, out=None, changed=None,
                      want_rates=False, want_x=True):
    return _tauleap_s256(logits, x, tables, i, beta, h, flags, seed, offset, None, x_base, out, changed, want_rates, None, want_x)


def tauleap_step_s256_rows(logits, x, tables, i, beta, h, flags, seed, offset, rows, x_base=None, out=None, changed=None,
                           want_rates=False, rates=None, want_x=True):
    """tauleap_step_s256 on the listed rows (see tauleap_step_rows); `rates`: unlisted rows untouched."""
    return _tauleap_s256(logits, x, tables, i, beta, h, flags, seed, offset, rows, x_base, out, changed, want_rates, rates, want_x)
