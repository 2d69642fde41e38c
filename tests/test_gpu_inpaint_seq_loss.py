"""GPU: inpainting training of the sequence models -- the masked row kernels of the two SDDM objectives (ctdd_crm_loss_masked,
ctdd_crm_loss_ll_masked, ctdd_score_elbo_loss_masked, ctdd_score_elbo_loss_ll_masked) and the InpaintCatRM / InpaintScoreElbo
losses on them.
1. under an all-free mask every entry is its unmasked sibling: value, gradient, nothing written outside the gradient buffer;
2. ragged masks (a single free row that is the last one, a fully held sample, a whole held workgroup between live ones, both ends
   in both roles) against autograd in fp64 through the per-sample composition of oracle.losses.crm_family / score_elbo on the
   gathered free rows; held gradient rows are exact zeros, through the whole reverse-logit chain too;
3. refusals before any launch;
4. the two losses on pinned noise under a ragged mask: the same reference, and only the masked entries ran;
5. the two inpainting configs end to end on the HIP hollow trainer, and ConditionalLBJF.inpaint on the trained maze model."""
import functools
import warnings

import numpy as np
import pytest
import torch

from inpaint_seq_cases import CE_COEFF, EPS, ragged_mask, ref_crm, ref_score_elbo, states

pytestmark = pytest.mark.gpu

KEYS = ("ctdd_crm_loss_masked", "ctdd_crm_loss_ll_masked", "ctdd_score_elbo_loss_masked", "ctdd_score_elbo_loss_ll_masked",
        "ctdd_crm_loss_ll", "ctdd_score_elbo_loss_ll", "ctdd_logprob_bwd")
DIRECT = [(3, 5, 15),              # S below a wave
          (37, 4, 21),             # rows not divisible by the 4 of a workgroup
          (100, 3, 9),             # lane strides with a tail
          (256, 3, 37)]            # four lane strides
REVERSE = [(256, 3, 50), (32, 4, 37),      # ctdd_logprob* on the matrix cores
           (3, 5, 15), (100, 3, 9)]        # ... and the generic kernels
LOSS_TYPES = ["rm", "mle", "elbo"]
NLLW = 0.3
GUARD = 1024                       # floats of sentinel on either side of the gradient buffer


def _delta(before):
    from ctdd import native
    return {k: native.LAUNCH_COUNTS.get(k, 0) - before.get(k, 0) for k in KEYS}


def _only(**ran):
    return {k: ran.get(k[5:], 0) for k in KEYS}


def _guarded(B, D, S):
    """A NaN-filled (B, D, S) gradient buffer inside a larger allocation of sentinels."""
    buf = torch.full((B * D * S + 2 * GUARD,), 777.0, device="cuda")
    grad = buf[GUARD:GUARD + B * D * S].view(B, D, S)
    grad.fill_(float("nan"))
    return buf, grad


def _intact(buf):
    return bool((buf[:GUARD] == 777.0).all() and (buf[-GUARD:] == 777.0).all())


@functools.lru_cache(maxsize=None)
def _inputs(S, B, D, kind):
    """Tables, a mask and the states as the losses build them, random logits.  Everything on the device; shared and never written.
    Uniform rates at every S: the Gaussian S = 256 table puts q(x0 -> x_t) below fp32 resolution for random pairs.  A uniform
    chain leaves a state at rate 1.7 (S - 1), so t is drawn with 1.7 S t in [0.3, 2]: q_{t|0} keeps 16 % to 75 % of its mass on
    the diagonal at every S.  (At t in [0.05, 0.95] the tables of S >= 32 are stationary to fp32 resolution, log p_t(. | x) no
    longer depends on the logits and the reverse-logit chain would be compared on gradients of 1e-18.)"""
    from ctdd.process import DeviceForwardProcess
    gen = torch.Generator().manual_seed(S * 1000 + D * 10 + B)
    proc = DeviceForwardProcess("uniform", S, "cuda", rate_const=1.7, t_func="sqrt_cos")
    ts = ((torch.rand(B, generator=gen) * 1.7 + 0.3) / (1.7 * S)).cuda()
    qt0, qT, rate, _ = proc.tables(ts, want_qt0=True, want_qt0T=True, want_rate=True)
    x0 = torch.randint(0, S, (B, D), generator=gen)
    free = torch.ones(B, D, dtype=torch.bool) if kind == "all" else ragged_mask(B, D, seed=S + D)
    x_t, x_tilde = states(x0, torch.randint(0, S, (B, D), generator=gen), free, S)
    logits = torch.randn(B, D, S, generator=gen).cuda()
    i32 = lambda t: t.int().cuda()
    return dict(ts=ts, qt0=qt0, qT=qT, rate=rate, x0=i32(x0), x_t=i32(x_t), x_tilde=i32(x_tilde), free=free.cuda(), logits=logits)


def _close_to_sibling(tag, val, grad, sval, sgrad):
    """The bar of test_masked_entry_is_the_dense_and_the_window_entry (tests/test_gpu_inpaint_loss.py) for the same claim."""
    assert torch.isfinite(sval) and torch.isfinite(sgrad).all() and sgrad.abs().max().item() > 0
    scale = sgrad.abs().max().item()
    err = (grad - sgrad).abs().max().item()
    print(f"{tag}: value {val.item():.9g} vs {sval.item():.9g}; max |grad diff| {err:.3e} (bar {1e-6 * scale:.3e})")
    np.testing.assert_allclose(val.item(), sval.item(), rtol=1e-6)
    assert err <= 1e-6 * scale


# ------------------------------------------------------------------------------------------------ 1: all free = the sibling
@pytest.mark.parametrize("S,B,D", DIRECT)
def test_all_free_is_the_unmasked_sibling(S, B, D):
    from ctdd import native
    c = _inputs(S, B, D, "all")
    la, free, qt0, rate, x0, x_t, x_tilde = c["logits"], c["free"], c["qt0"], c["rate"], c["x0"], c["x_t"], c["x_tilde"]
    ll = torch.log_softmax(la, -1).contiguous()                                   # a valid ll_all for the two _ll entries
    keep = (la.clone(), ll.clone())
    scale, nll = (1.0 - CE_COEFF) / B, NLLW / (B * D)
    bufs = []

    def guarded():
        bufs.append(_guarded(B, D, S))
        return bufs[-1][1]
    before = dict(native.LAUNCH_COUNTS)
    for lt in LOSS_TYPES:
        q = qt0 if lt == "elbo" else None
        val, grad = native.crm_loss_masked(la, x_t, x0, free, q, lt, scale, nll, grad_out=guarded())
        assert grad.data_ptr() == bufs[-1][1].data_ptr()
        _close_to_sibling(f"crm {lt} S={S}", val, grad, *native.crm_loss(la, x_t, x0, q, lt, scale, nll))
        val, grad = native.crm_loss_masked(la, x_t, None, free, q, lt, scale, 0.0, grad_out=guarded())
        _close_to_sibling(f"crm {lt} (no CE) S={S}", val, grad, *native.crm_loss(la, x_t, None, q, lt, scale, 0.0))
        val, grad = native.crm_loss_ll_masked(ll, x_t, free, q, lt, scale, grad_out=guarded())
        _close_to_sibling(f"crm_ll {lt} S={S}", val, grad, *native.crm_loss_ll(ll, x_t, q, lt, scale))
    for role, reg_x in (("x~", x_tilde), ("x_t", x_t)):                           # one forward pass / two
        val, grad = native.score_elbo_loss_masked(la, x0, x_tilde, reg_x, free, qt0, rate, EPS, NLLW / B, grad_out=guarded())
        _close_to_sibling(f"score-elbo reg_x={role} S={S}", val, grad, *native.score_elbo_loss(la, x0, x_tilde, reg_x, qt0, rate, EPS, NLLW / B))
        val, grad = native.score_elbo_loss_ll_masked(ll, x0, x_tilde, reg_x, free, qt0, rate, EPS, NLLW / B, grad_out=guarded())
        _close_to_sibling(f"score-elbo_ll reg_x={role} S={S}", val, grad,
                          *native.score_elbo_loss_ll(ll, x0, x_tilde, reg_x, qt0, rate, EPS, NLLW / B))
    torch.cuda.synchronize()
    assert _delta(before) == _only(crm_loss_masked=6, crm_loss_ll_masked=3, score_elbo_loss_masked=2, score_elbo_loss_ll_masked=2,
                                   crm_loss_ll=3, score_elbo_loss_ll=2)
    assert torch.equal(la, keep[0]) and torch.equal(ll, keep[1])                  # read in place, never written
    for buf, grad in bufs:
        assert torch.isfinite(grad).all() and _intact(buf)                        # (NaN before the call: every element was written)


# ------------------------------------------------------------------------------------------------ 2: ragged masks against fp64
def _host(c):
    h = lambda t: t.detach().cpu()
    return (h(c["x0"]).long(), h(c["x_t"]).long(), h(c["x_tilde"]).long(), h(c["free"]), h(c["qt0"]).double(), h(c["rate"]).double(),
            h(c["logits"]).double())


@functools.lru_cache(maxsize=None)
def _ref_crm(S, B, D, logit_type, loss_type, nllw):
    x0, x_t, _, free, qt0, _, logits = _host(_inputs(S, B, D, "ragged"))
    lg = logits.requires_grad_()
    val = ref_crm(lg, x0, x_t, free, qt0, logit_type=logit_type, loss_type=loss_type, ce_coeff=CE_COEFF, nll_weight=nllw)
    grad, = torch.autograd.grad(val, lg)
    return val.item(), grad.float().cuda()


@functools.lru_cache(maxsize=None)
def _ref_selbo(S, B, D, logit_type, one_pass, nllw=NLLW):
    x0, x_t, x_tilde, free, qt0, rate, logits = _host(_inputs(S, B, D, "ragged"))
    lg = logits.requires_grad_()
    val = ref_score_elbo(lg, x0, x_t, x_tilde, free, qt0, rate, logit_type=logit_type, nll_weight=nllw, one_forward_pass=one_pass)
    grad, = torch.autograd.grad(val, lg)
    return val.item(), grad.float().cuda()


def _check_ragged(tag, chain, c, val, grad, want_val, want_grad):
    free, B = c["free"], c["free"].shape[0]
    assert torch.isfinite(val) and torch.isfinite(grad).all()                     # ... the fully held sample included
    assert (grad[~free] == 0).all() and (B < 3 or (grad[2] == 0).all())           # held rows: exact zeros
    err, top = (grad - want_grad).abs().max().item(), want_grad.abs().max().item()
    print(f"{tag}: value {val.item():.8g} vs fp64 {want_val:.10g}; max |d/dlogits - fp64| = {err:.3e}, max |d/dlogits| = {top:.3e}")
    assert top > 0
    if chain == "direct":
        np.testing.assert_allclose(val.item(), want_val, rtol=2e-5)
        np.testing.assert_allclose(grad.cpu().numpy(), want_grad.cpu().numpy(), rtol=2e-4, atol=2e-6)
    else:
        np.testing.assert_allclose(val.item(), want_val, rtol=3e-5)
        np.testing.assert_allclose(grad.cpu().numpy(), want_grad.cpu().numpy(), rtol=5e-4, atol=1e-6 * top + 1e-9)


def _ragged_is_ragged(c):
    free = c["free"]
    B, D = free.shape
    assert int(free[0].sum()) == 1 and free[0, D - 1] and free[1, 0] and not free[1, D - 1] and (B < 3 or not free[2].any())
    flat = free.view(-1)
    groups = flat[:flat.numel() // 4 * 4].view(-1, 4).any(1)                      # the 4-row workgroups of the row kernels
    held = (~groups).nonzero().view(-1)
    assert held.numel() > 0
    if D >= 14:                                                                   # (the mask holds a run of 8 rows inside sample 1)
        assert [int(g) for g in held if groups[:g].any() and groups[g + 1:].any()], "no fully held workgroup between live ones"


@pytest.mark.parametrize("S,B,D", DIRECT)
def test_direct_chain_against_fp64_on_ragged_masks(S, B, D):
    from ctdd import native
    c = _inputs(S, B, D, "ragged")
    _ragged_is_ragged(c)
    la, free, qt0, rate, x0, x_t, x_tilde = c["logits"], c["free"], c["qt0"], c["rate"], c["x0"], c["x_t"], c["x_tilde"]
    n_free = int(free.sum())
    keep = la.clone()
    bufs, got = [], []
    before = dict(native.LAUNCH_COUNTS)
    for lt in LOSS_TYPES:
        bufs.append(_guarded(B, D, S))
        got.append((f"crm {lt}", native.crm_loss_masked(la, x_t, x0, free, qt0 if lt == "elbo" else None, lt, (1.0 - CE_COEFF) / B, NLLW / n_free,
                                                        grad_out=bufs[-1][1]), _ref_crm(S, B, D, "direct", lt, NLLW)))
    for one_pass in (True, False):
        bufs.append(_guarded(B, D, S))
        got.append((f"score-elbo one_pass={one_pass}",
                    native.score_elbo_loss_masked(la, x0, x_tilde, x_tilde if one_pass else x_t, free, qt0, rate, EPS, NLLW / B, grad_out=bufs[-1][1]),
                    _ref_selbo(S, B, D, "direct", one_pass)))
    torch.cuda.synchronize()
    assert _delta(before) == _only(crm_loss_masked=3, score_elbo_loss_masked=2)
    assert torch.equal(la, keep)
    for buf, grad in bufs:
        assert not torch.isnan(grad).any() and _intact(buf)
    for tag, (val, grad), (want_val, want_grad) in got:
        _check_ragged(f"{tag} S={S}", "direct", c, val, grad, want_val, want_grad)


@pytest.mark.parametrize("logit_type", ["reverse_prob", "reverse_logscale"])
@pytest.mark.parametrize("S,B,D", REVERSE)
def test_reverse_chain_against_fp64_on_ragged_masks(S, B, D, logit_type):
    """ctdd_logprob -> the masked _ll entry -> ctdd_logprob_bwd (the matrix-core pair for reverse_prob with S % 32 == 0): a zero
    d/d ll_all row comes out as an exact-zero logit-gradient row."""
    from ctdd import native
    c = _inputs(S, B, D, "ragged")
    _ragged_is_ragged(c)
    la, free, qt0, qT, rate, x0, x_t, x_tilde = c["logits"], c["free"], c["qt0"], c["qT"], c["rate"], c["x0"], c["x_t"], c["x_tilde"]
    keep = la.clone()
    tidx = torch.arange(B, dtype=torch.int32, device="cuda")
    mfma = native._rp_mfma_ok(logit_type, la, qt0)
    assert mfma == (logit_type == "reverse_prob" and S % 32 == 0)
    bufs, got = [], []
    before = dict(native.LAUNCH_COUNTS)
    ll_all, _ = native.logprob(la, x_t, qt0, logit_type, tidx, qt0T=qT)
    for lt in LOSS_TYPES:
        bufs.append(_guarded(B, D, S))
        val, dll = native.crm_loss_ll_masked(ll_all, x_t, free, qt0 if lt == "elbo" else None, lt, (1.0 - CE_COEFF) / B, grad_out=bufs[-1][1])
        assert (dll[~free] == 0).all()
        grad, _ = native.logprob_bwd(logit_type, la, qt0, qT, dll, ll_all=ll_all)
        got.append((f"crm {lt}", (val, grad), _ref_crm(S, B, D, logit_type, lt, 0.0)))
    ll_tilde, _ = native.logprob(la, x_tilde, qt0, logit_type, tidx, qt0T=qT)
    for one_pass in (True, False):
        bufs.append(_guarded(B, D, S))
        val, dll = native.score_elbo_loss_ll_masked(ll_tilde, x0, x_tilde, x_tilde if one_pass else x_t, free, qt0, rate, EPS, NLLW / B,
                                                    grad_out=bufs[-1][1])
        assert (dll[~free] == 0).all()
        grad, _ = native.logprob_bwd(logit_type, la, qt0, qT, dll, ll_all=ll_tilde)
        got.append((f"score-elbo one_pass={one_pass}", (val, grad), _ref_selbo(S, B, D, logit_type, one_pass)))
    torch.cuda.synchronize()
    assert _delta(before) == _only(crm_loss_ll_masked=3, score_elbo_loss_ll_masked=2, logprob_bwd=5)
    assert torch.equal(la, keep)
    for buf, dll in bufs:
        assert not torch.isnan(dll).any() and _intact(buf)
    for tag, (val, grad), (want_val, want_grad) in got:
        _check_ragged(f"{tag} {logit_type} S={S}", "reverse", c, val, grad, want_val, want_grad)


# ------------------------------------------------------------------------------------------------ 3: refusals
@pytest.mark.parametrize("bad", ["free_none", "free_shape", "free_dtype", "free_cpu", "null_free_abi", "S_257", "elbo_without_qt0"])
def test_refusals_before_any_launch(bad):
    from ctdd import native
    S, B, D = 16, 2, 10
    c = _inputs(S, B, D, "ragged")
    la, free, qt0, rate, x0, x_t, x_tilde = c["logits"], c["free"], c["qt0"], c["rate"], c["x0"], c["x_t"], c["x_tilde"]
    grad = torch.full_like(la, 5.0)
    lib = native.load()
    before = dict(native.LAUNCH_COUNTS)

    def all_four(fr, logits=la, q=qt0, r=rate, g=grad):
        return [lambda: native.crm_loss_masked(logits, x_t, x0, fr, q, "rm", 1.0, 0.1, grad_out=g),
                lambda: native.crm_loss_ll_masked(logits, x_t, fr, q, "rm", 1.0, grad_out=g),
                lambda: native.score_elbo_loss_masked(logits, x0, x_tilde, x_tilde, fr, q, r, EPS, 0.1, grad_out=g),
                lambda: native.score_elbo_loss_ll_masked(logits, x0, x_tilde, x_tilde, fr, q, r, EPS, 0.1, grad_out=g)]
    if bad in ("free_none", "free_shape", "free_dtype", "free_cpu"):            # the binding's host checks
        fr = {"free_none": None, "free_shape": free[:, :D - 1].contiguous(), "free_dtype": free.int(), "free_cpu": free.cpu()}[bad]
        calls = all_four(fr)
    elif bad == "S_257":                                                         # ... the rest: the library itself
        big, tab = torch.zeros(B, D, 257, device="cuda"), torch.zeros(B, 257, 257, device="cuda")
        calls = all_four(free, logits=big, q=tab, r=tab, g=torch.full_like(big, 5.0))[2:]
    elif bad == "elbo_without_qt0":
        calls = [lambda: native.crm_loss_masked(la, x_t, x0, free, None, "elbo", 1.0, 0.1, grad_out=grad),
                 lambda: native.crm_loss_ll_masked(la, x_t, free, None, "elbo", 1.0, grad_out=grad)]
    else:
        calls = []
        p, st = (lambda t: t.data_ptr()), torch.cuda.current_stream().cuda_stream
        rows, out = torch.zeros(B * D, dtype=torch.float64, device="cuda"), torch.zeros(1, device="cuda")
        scratch = torch.empty(int(lib.ctdd_ctelbo_scratch_bytes(B, D, S)), dtype=torch.uint8, device="cuda")
        assert lib.ctdd_crm_loss_masked(p(la), p(x_t), p(x0), None, p(qt0), B, D, S, 0, 1.0, 0.1, p(grad), p(rows), p(out), st) != 0
        assert lib.ctdd_crm_loss_ll_masked(p(la), p(x_t), None, p(qt0), B, D, S, 0, 1.0, p(grad), p(rows), p(out), st) != 0
        for fn in (lib.ctdd_score_elbo_loss_masked, lib.ctdd_score_elbo_loss_ll_masked):
            assert fn(p(la), p(x0), p(x_tilde), p(x_tilde), None, p(qt0), p(rate), B, D, S, EPS, 0.1, p(scratch), p(grad), p(out), st) != 0
        assert out.item() == 0.0
    for call in calls:
        with pytest.raises(native.CtddError):
            call()
    torch.cuda.synchronize()
    assert _delta(before) == _only()
    assert (grad == 5.0).all()                                                   # refused before any launch


# ------------------------------------------------------------------------------------------------ 4: the losses on pinned noise
class FixedLogits:
    """An embedding-free model: fixed logits whatever the state, the device process for the tables."""

    def __init__(self, S, logits):
        from ctdd.process import DeviceForwardProcess
        self.process = DeviceForwardProcess("uniform", S, "cuda", rate_const=1.7, t_func="sqrt_cos")
        self.device, self.logits, self.calls = torch.device("cuda"), logits.clone().requires_grad_(), []

    def __call__(self, x, t):
        self.calls.append(x.clone())
        return self.logits

    def transition(self, t):
        return self.process.transition(t)

    def rate(self, t):
        return self.process.rate(t)


def _cfg(name, S, D, **loss):
    from config.synthetic_config.config_hollow_synthetic_inpaint import get_config
    c = get_config()
    c.data.S, c.model.concat_dim = S, D
    c.loss.update(name=name, ce_coeff=CE_COEFF, nll_weight=NLLW, eps_ratio=EPS, mask="bernoulli", mask_rate=[0.1, 0.9])
    c.loss.update(**loss)
    return c


def _run_pinned(name, S, B, D, **loss):
    import lib.losses.losses as L
    import lib.losses.losses_utils as lu
    from ctdd import native
    c = _inputs(S, B, D, "ragged")
    model = FixedLogits(S, c["logits"])
    L._FIXED_NOISE = {"ts": c["ts"], "x_t": c["x_t"], "x_tilde": c["x_tilde"], "free": c["free"].cpu()}
    before = dict(native.LAUNCH_COUNTS)
    try:
        val = lu.get_loss(_cfg(name, S, D, **loss)).calc_loss(c["x0"].long(), {"model": model, "n_iter": 0})
        grad, = torch.autograd.grad(val, model.logits)
    finally:
        L._FIXED_NOISE = None
    return c, model, val.detach(), grad, _delta(before)


@pytest.mark.parametrize("nllw", [0.0, NLLW])
@pytest.mark.parametrize("loss_type", ["rm", "elbo"])
@pytest.mark.parametrize("logit_type,S,B,D", [("direct", 37, 4, 21), ("reverse_prob", 37, 4, 21), ("reverse_prob", 32, 4, 37)])
def test_inpaint_catrm_on_pinned_noise(logit_type, S, B, D, loss_type, nllw):
    c, model, val, grad, ran = _run_pinned("InpaintCatRM", S, B, D, logit_type=logit_type, loss_type=loss_type, nll_weight=nllw)
    if logit_type == "direct":
        assert ran == _only(crm_loss_masked=1)                                   # the CE term rides in the same launch
    else:                                                                        # ... and is one extra pass, when asked for
        assert ran == _only(crm_loss_ll_masked=1, logprob_bwd=1, crm_loss_masked=1 if nllw else 0)
    assert len(model.calls) == 1 and torch.equal(model.calls[0], c["x_t"].long())
    assert torch.equal(model.calls[0][~c["free"]], c["x0"].long()[~c["free"]])   # the network sees the held values
    want_val, want_grad = _ref_crm(S, B, D, logit_type, loss_type, nllw)
    _check_ragged(f"InpaintCatRM {logit_type} {loss_type} nll_weight={nllw}", "direct" if logit_type == "direct" else "reverse", c, val, grad,
                  want_val, want_grad)


@pytest.mark.parametrize("one_pass", [True, False])
@pytest.mark.parametrize("logit_type,S,B,D", [("direct", 37, 4, 21), ("reverse_prob", 37, 4, 21), ("reverse_prob", 32, 4, 37)])
def test_inpaint_score_elbo_on_pinned_noise(logit_type, S, B, D, one_pass):
    c, model, val, grad, ran = _run_pinned("InpaintScoreElbo", S, B, D, logit_type=logit_type, one_forward_pass=one_pass)
    assert ran == (_only(score_elbo_loss_masked=1) if logit_type == "direct" else _only(score_elbo_loss_ll_masked=1, logprob_bwd=1))
    assert len(model.calls) == 1 and torch.equal(model.calls[0], (c["x_tilde"] if one_pass else c["x_t"]).long())
    want_val, want_grad = _ref_selbo(S, B, D, logit_type, one_pass)
    _check_ragged(f"InpaintScoreElbo {logit_type} one_pass={one_pass}", "direct" if logit_type == "direct" else "reverse", c, val, grad,
                  want_val, want_grad)


def test_fused_false_runs_the_torch_restatements():
    """cfg.loss.fused = False: no HIP objective runs; the torch restatement (fp32 device ops) agrees with the fused chain.  Both
    are within the reverse chain's bars of the fp64 reference, so of each other within twice them."""
    S, B, D = 37, 4, 21
    for name, key in (("InpaintCatRM", "crm_loss_ll_masked"), ("InpaintScoreElbo", "score_elbo_loss_ll_masked")):
        _, _, val, grad, ran = _run_pinned(name, S, B, D, logit_type="reverse_prob", loss_type="rm", one_forward_pass=True)
        c, _, val2, grad2, ran2 = _run_pinned(name, S, B, D, logit_type="reverse_prob", loss_type="rm", one_forward_pass=True, fused=False)
        assert ran[f"ctdd_{key}"] == 1 and ran2 == _only()
        print(f"{name}: fused {val.item():.8g} | torch ops {val2.item():.8g}")
        np.testing.assert_allclose(val2.item(), val.item(), rtol=2 * 3e-5)
        assert (grad2[~c["free"]] == 0).all()
        top = grad.abs().max().item()
        np.testing.assert_allclose(grad2.cpu().numpy(), grad.cpu().numpy(), rtol=2 * 5e-4, atol=2 * (1e-6 * top + 1e-9))


# ------------------------------------------------------------------------------------------------ 5: end to end
def _registries():
    import lib.models.models  # noqa: F401
    import lib.models.model_utils as mu
    import lib.sampling.sampling  # noqa: F401
    import lib.sampling.sampling_utils as su
    import lib.losses.losses  # noqa: F401
    import lib.losses.losses_utils as lu
    import lib.training.training  # noqa: F401
    import lib.training.training_utils as tu
    import lib.optimizers.optimizers  # noqa: F401
    import lib.optimizers.optimizers_utils as ou
    return mu, su, lu, tu, ou


def _three_steps(cfg, batch):
    """Three Standard.step calls on the HIP hollow trainer (cfg.model.engine_train at its default): finite losses, parameters
    move, no fallback warning."""
    from ctdd import native
    from ctdd.hollow_train import training_supported
    mu, _, lu, tu, ou = _registries()
    assert getattr(cfg.model, "engine_train", None) is None
    torch.manual_seed(0)
    model = mu.create_model(cfg, torch.device("cuda"))
    assert training_supported(model)
    state = {"model": model, "optimizer": ou.get_optimizer(model.parameters(), cfg), "n_iter": 0}
    step, loss = tu.get_train_step(cfg), lu.get_loss(cfg)
    w0 = [p.detach().clone() for p in model.parameters()]
    S, shape = int(cfg.data.S), [batch] + list(cfg.data.shape)
    before = dict(native.LAUNCH_COUNTS)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        for i in range(3):
            out = step.step(state, loss, torch.randint(0, S, shape, device="cuda"))
            assert out.dim() == 0 and torch.isfinite(out) and float(out) < 1e8
    assert not [w for w in caught if issubclass(w.category, RuntimeWarning)], [str(w.message) for w in caught]
    assert model._trainer is not None                                            # the steps ran on the HIP hollow trainer
    assert sum(int(not torch.equal(p, q)) for p, q in zip(w0, model.parameters())) > 0
    return model, _delta(before)


def test_maze_inpaint_config_trains_and_inpaints():
    from config.maze_config.config_hollow_maze_inpaint import get_config
    _, su, _, _, _ = _registries()
    cfg = get_config()
    cfg.device = "cuda"
    cfg.model.num_layers = 2
    cfg.sampler.num_steps = 8
    assert int(cfg.model.concat_dim) == 225 and int(cfg.data.S) == 3
    model, ran = _three_steps(cfg, 4)
    assert ran == _only(score_elbo_loss_ll_masked=3, logprob_bwd=3)
    model.eval()
    x_known = torch.randint(0, 3, (4, 225), generator=torch.Generator().manual_seed(3))
    held = torch.zeros(4, 15, 15, dtype=torch.bool)
    held[:, :7] = True                                                           # the top 7 rows, a held box, a free box, scattered cells
    held[1] = False
    held[1, 4:11, 3:9] = True
    held[2] = ~held[1]
    held[3] = torch.rand(15, 15, generator=torch.Generator().manual_seed(4)) < 0.5
    held = held.view(4, 225)
    sampler = su.get_sampler(cfg)
    sampler.seed = 11
    out = sampler.inpaint(model, x_known, held)
    out = np.asarray(out[0] if isinstance(out, tuple) else out)
    assert out.shape == (4, 225) and out.min() >= 0 and out.max() < 3
    assert (out[held.numpy()] == x_known.numpy()[held.numpy()]).all()
    model.train()


def test_synthetic_inpaint_config_trains():
    from config.synthetic_config.config_hollow_synthetic_inpaint import get_config
    cfg = get_config()
    cfg.device = "cuda"
    _, ran = _three_steps(cfg, 8)
    assert ran == _only(crm_loss_ll_masked=3, logprob_bwd=3)
