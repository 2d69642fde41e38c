"""GPU: the visibility matrix and the dropout keep bits of every masked-attention kernel, read back EXACTLY (tests/attn_cases.py:
q = 0 makes every visible key's probability 1 / n_i, a one-hot V block -- or a one-hot dO block through dV -- turns each (query,
key) pair into one output entry that is non-zero exactly when the pair is visible and kept).  No tolerance on the pattern: one
wrongly admitted or dropped pair fails, which the numeric tests cannot promise (at 225 queries one pair moves a readout row by
0.4 %, far under the bf16 bars).  The sweep over every Tq from 1 to 130 crosses the 32-key chunk, the 32-query wave tile and the
128-query workgroup, and takes Tq + 1 (where the readout's second key window starts) through every residue mod 32 with and without
a tile that chunk_full may declare free of mask arithmetic."""
import ctypes as C

import pytest
import torch

import attn_cases as ac

pytestmark = pytest.mark.gpu

SWEEP = [(16, Tq) for Tq in range(1, 131)]
EDGES = (31, 32, 33, 63, 64, 65, 96, 97, 129)
BF16_P_REL = 2.0 ** -8          # a probability 1 / n rounded to nearest bf16 (8 significant bits: at most 2^-8 / (1 + 2^-8) relative), the
                                # matrix-core backward's P operand; measured 3.418e-3 (the fp32 kernels and all five forwards: 0)


def _cases(name, backward=False):
    """(hd, Tq): the full sweep at hd 16, the tile edges at hd 32; the fp32 kernels also at hd 8, the inference one at hd 64"""
    cases = SWEEP + [(32, Tq) for Tq in EDGES]
    if name.endswith("fp32"):
        cases += [(8, Tq) for Tq in EDGES]
    if name == "infer_fp32" and not backward:
        cases += [(64, Tq) for Tq in EDGES]
    return cases


def _check(pat, vals, mode, Tq, rel, what):
    ok = ac.allowed(mode, Tq)
    assert torch.isfinite(vals).all(), what
    assert pat.shape == (pat.shape[0],) + tuple(ok.shape), what
    wrong = pat != ok
    assert not wrong.any(), f"{what}: (head, query, key) {wrong.nonzero()[:8].tolist()} read back as {pat[wrong][:8].tolist()}"
    want = (ok / ac.visible_counts(mode, Tq)[:, None]).expand_as(vals)
    err = float(((vals.double() - want).abs() / want.clamp_min(1e-30))[pat].max())
    assert err < rel, f"{what}: a visible entry is off 1 / n_i by {err:.3e} relative (bar {rel:.1e})"
    return err


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("name", ac.FORWARDS)
def test_forward_visibility_is_the_mask(name, mode):
    """Every forward entry, every Tq in 1..130 (hd 16, two heads; block index = batch index, so one launch reads the whole
    matrix under several b and h): pattern == allowed, every visible value 1 / n_i to 1e-6 (all five write fp32, and with q = 0
    their probabilities are exactly 1 before the division), every output finite."""
    fwd = ac.forward_entry(name)
    worst = 0.0
    for hd, Tq in _cases(name):
        pat, vals = ac.read_visibility(lambda q, k, v: fwd(q, k, v, mode), mode, Tq, hd, 2, seed=Tq)
        worst = max(worst, _check(pat, vals, mode, Tq, 1e-6, f"{name} mode {mode} Tq={Tq} hd={hd}"))
    print(f"forward visibility {name} mode {mode}: largest deviation from 1 / n_i {worst:.3e} relative (bar 1e-6)")


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("name", ac.BACKWARDS)
def test_backward_visibility_is_the_mask(name, mode):
    """ctdd_hollow_attention_bwd / _bwd_bf16 over the same sweep, read through dV: pattern == allowed; dV entries 1 / n_i to 1e-6
    (fp32 kernels) or to a bf16 rounding of the probability (matrix cores: P is a bf16 operand of dV = P^T dO); dq, dk, dv finite."""
    bwd = ac.backward_entry(name)
    rel = 1e-6 if name == "train_fp32" else BF16_P_REL
    worst = 0.0
    for hd, Tq in _cases(name, backward=True):
        def run(q, k, v, d_out):
            dq, dk, dv = bwd(q, k, v, d_out, mode)
            assert torch.isfinite(dq).all() and torch.isfinite(dk).all()
            return dv
        pat, vals = ac.read_visibility_bwd(run, mode, Tq, hd, 2, seed=Tq)
        worst = max(worst, _check(pat, vals, mode, Tq, rel, f"{name} backward mode {mode} Tq={Tq} hd={hd}"))
    print(f"backward visibility {name} mode {mode}: largest deviation from 1 / n_i {worst:.3e} relative (bar {rel:.1e})")


# ------------------------------------------------------------------------------------------------ dropout keep bits
DROP_TQ = (1, 7, 33, 64, 97, 129)
DROP_B, DROP_H, DROP_HD, DROP_P = 2, 2, 16, 0.25           # p = 0.25: thr = 16384, the rate in force is exactly 1 / 4


def read_keep(name, mode, Tq, rng, layer, backward=False, B=DROP_B, H=DROP_H, hd=DROP_HD):
    """allowed & keep of one kernel family, [B, H, Tq, Tk], and the values"""
    drop = dict(p=DROP_P, rng=rng, layer=layer)
    if backward:
        bwd = ac.backward_entry(name)
        return ac.read_visibility_bwd(lambda q, k, v, d: bwd(q, k, v, d, mode, **drop)[2], mode, Tq, hd, H, B=B, seed=Tq)
    fwd = ac.forward_entry(name)
    return ac.read_visibility(lambda q, k, v: fwd(q, k, v, mode, **drop), mode, Tq, hd, H, B=B, seed=Tq)


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_dropout_keep_bits_are_one_pattern(mode):
    """p = 0.25 at Tq in {1, 7, 33, 64, 97, 129}: the forward of the fp32 kernels, the forward of the matrix-core kernels and the dV
    readbacks of both backwards return the SAME bits, inside the mask; the fp32 forward's kept entries are 1 / (n_i (1 - p)) -- the
    normaliser counts the dropped keys; the bits change with the layer id and with the step of rng, and repeat for the same pair.
    Kept fraction over every visible pair of the six lengths (B = H = 2: 6.3e4 pairs in the modes 0 / 1, more in 2 / 3) within
    0.02 of 0.75, the margin of the rate tests of test_gpu_hollow_train.py / test_gpu_bert_train.py."""
    rng = torch.tensor([4321, 9], dtype=torch.int64, device="cuda")
    rng_next = torch.tensor([4321, 10], dtype=torch.int64, device="cuda")
    kept = pairs = 0
    for Tq in DROP_TQ:
        ok = ac.allowed(mode, Tq)
        base, vals = read_keep("train_fp32", mode, Tq, rng, 5)
        assert torch.isfinite(vals).all() and not (base & ~ok).any(), f"Tq={Tq}: an entry outside the mask"
        want = (1.0 / (1.0 - DROP_P)) / ac.visible_counts(mode, Tq)[:, None].double()
        err = float(((vals.double() - want).abs() / want)[base].max()) if base.any() else 0.0
        assert err < 1e-6, f"Tq={Tq}: a kept entry is off 1 / (n_i (1 - p)) by {err:.3e} relative"
        for name, backward in (("train_mfma", False), ("train_fp32", True), ("train_mfma", True)):
            got, v = read_keep(name, mode, Tq, rng, 5, backward)
            assert torch.isfinite(v).all()
            diff = got != base
            assert not diff.any(), f"Tq={Tq}: {name} {'backward' if backward else 'forward'} draws other bits at (b, h, i, j) {diff.nonzero()[:8].tolist()}"
        assert torch.equal(read_keep("train_fp32", mode, Tq, rng, 5)[0], base)
        if Tq >= 33:                                                            # (>= 2e3 visible pairs: equal patterns cannot be chance)
            assert not torch.equal(read_keep("train_fp32", mode, Tq, rng, 6)[0], base), f"Tq={Tq}: the layer id does not move the bits"
            assert not torch.equal(read_keep("train_fp32", mode, Tq, rng_next, 5)[0], base), f"Tq={Tq}: the step does not move the bits"
        kept += int(base.sum())
        pairs += int(ok.sum()) * DROP_B * DROP_H
    assert pairs >= 20000
    frac = kept / pairs
    print(f"dropout bits mode {mode}: kept {kept} of {pairs} visible pairs = {frac:.4f} (0.75 +- 0.02)")
    assert abs(frac - 0.75) < 0.02


# ------------------------------------------------------------------------------------------------ launcher checks
BAD_SHAPES = [dict(Tq=0, Tk=0), dict(Tq=-3, Tk=-3), dict(Tk=0), dict(Tk=-1), dict(mode=0, Tk=34), dict(mode=1, Tk=32), dict(mode=0, Tk=67),
              dict(B=0), dict(B=-1), dict(H=0), dict(H=-2), dict(mode=3, Tq=0), dict(mode=3, Tk=0), dict(mode=2, Tq=0, Tk=1)]


@pytest.mark.parametrize("bad", BAD_SHAPES, ids=lambda d: "-".join(f"{k}{v}" for k, v in d.items()))
def test_training_attention_refuses_bad_shapes_and_launches_nothing(bad):
    """Non-positive B, H, Tq or Tk, and Tk != Tq in the modes 0 / 1 (the inference launchers' rules): both forward and both
    backward entries return a negative code and leave the pre-filled outputs and stats alone."""
    from ctdd import hollow_train as ht
    lib = ht.lib()
    B, T, H, hd = 2, 33, 4, 16
    E = H * hd
    st = torch.cuda.current_stream().cuda_stream
    qkv = torch.randn((B * 2 * T, 3 * E), device="cuda")                 # (room for the keys a bad Tk names)
    dout = torch.randn((B * T, E), device="cuda")
    for fwd, bwd in ((lib.ctdd_hollow_attention_train, lib.ctdd_hollow_attention_bwd),
                     (lib.ctdd_hollow_attention_train_bf16, lib.ctdd_hollow_attention_bwd_bf16)):
        nan = lambda shape, dt=torch.float32: torch.full(shape, float("nan"), device="cuda", dtype=dt)
        out, stats, dqkv = nan((B * T, E)), nan((B, H, T, 4)), nan((B * 2 * T, 3 * E))
        out_hi, dqkv_hi = nan((B * T, E), torch.bfloat16), nan((B * 2 * T, 3 * E), torch.bfloat16)
        a = ht._attn_args(qkv, None, None, B, T, T, H, hd, bad.get("mode", 0), 0.0, None, 1)
        a.out, a.stats, a.out_bf16, a.d_out = out.data_ptr(), stats.data_ptr(), out_hi.data_ptr(), dout.data_ptr()
        a.dq, a.dk, a.dv = dqkv.data_ptr(), dqkv.data_ptr() + 4 * E, dqkv.data_ptr() + 8 * E
        a.dq_bf16, a.dk_bf16, a.dv_bf16 = dqkv_hi.data_ptr(), dqkv_hi.data_ptr() + 2 * E, dqkv_hi.data_ptr() + 4 * E
        a.dq_bs = a.dk_bs = a.dv_bs = T * 3 * E
        a.dq_rs = a.dk_rs = a.dv_rs = 3 * E
        for field, value in bad.items():
            setattr(a, field, value)
        assert fwd(C.byref(a), st) < 0
        assert bwd(C.byref(a), st) < 0
        torch.cuda.synchronize()
        for buf in (out, stats, dqkv, out_hi, dqkv_hi):
            assert torch.isnan(buf.float()).all()
