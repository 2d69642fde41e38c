"""GPU: conditional LBJF / midpoint / exact sampling on the row-list step kernels.

1. the row-list entry points (ctdd_lbjf_step_rows, ctdd_midpoint_predict_rows, ctdd_exact_step_rows, ctdd_lbjf_from_rates_rows,
   ctdd_midpoint_from_rates_rows) against the full launches: listed rows of every output bit-identical, unlisted rows
   untouched, counters over listed rows only -- every kernel path, every call kind (shapes and row lists of
   tests/test_gpu_conditional.py);
2. ConditionalLBJF / ConditionalMidPointTauL / ConditionalExactSampling in law against the oracle's own loops
   (oracle.samplers.lbjf_sample / midpoint_sample / exact_sample) run on the free part of a score that couples the dimensions;
3. identities on a deterministic model: all free = the parent sampler bit for bit, all held = x_known and no launch (also for
   ConditionalTauLeaping / ConditionalPCTauLeaping against TauL / PCTauL, whose loops they share);
4. the samplers on the HIP engines (maze hollow transformer, masked synthetic transformer)."""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import samplers as osamp
from oracle.forward_process import ForwardProcess
from oracle.toy_model import toy_logits

GAUSS = dict(rate_sigma=6.0, Q_sigma=512.0, time_exp=100.0, time_base=3.0)
UNIVAR = dict(rate_const=1.7, t_func="sqrt_cos")
ROWS_ENTRIES = ("ctdd_lbjf_step_rows", "ctdd_midpoint_predict_rows", "ctdd_exact_step_rows", "ctdd_lbjf_from_rates_rows",
                "ctdd_midpoint_from_rates_rows", "ctdd_tauleap_step_rows", "ctdd_tauleap_step_s256_rows")


def _delta(before):
    from ctdd import native
    return {k: native.LAUNCH_COUNTS.get(k, 0) - before.get(k, 0) for k in ROWS_ENTRIES}


# ------------------------------------------------------------------------------------------------ 1. kernel contract
# S -> kernel: 2, 3 k_rows_small (bit-exact with k_rows at G = 1); 5 k_rows_small, S > 4; 37 k_rows at G = 64, EPT = 1;
# 100 k_rows at EPT = 2; 256 k_rows at EPT = 4 (the generic steps called directly at S = 256).  The exact step has no small-S
# kernel: S <= 4 runs k_rows at G = 1, S = 5 at G = 8.
SIZES = [2, 3, 5, 37, 100, 256]
N_, D_ = 5, 131                    # 655 rows: five 128-row tiles and a partial sixth
R_ = N_ * D_
HS = (0.05, 0.5)


def _row_lists(R):
    g = torch.Generator().manual_seed(5)
    runs = torch.cat([torch.arange(120, 136), torch.arange(250, 262), torch.arange(383, 390), torch.arange(500, 640),
                      torch.arange(645, R)])
    return {"random": (torch.rand(R, generator=g) < 0.5).nonzero().view(-1), "empty": torch.zeros(0, dtype=torch.int64),
            "all": torch.arange(R), "single": torch.tensor([R // 3]), "last": torch.tensor([R - 1]), "tile_edges": runs}


def _process(S):
    from ctdd.process import DeviceForwardProcess
    return DeviceForwardProcess("univar", S, "cuda", **UNIVAR) if S <= 5 else DeviceForwardProcess("gaussian", S, "cuda", **GAUSS)


def _inputs(S, need_q=True):
    pr = _process(S)
    t32 = torch.tensor([0.5])
    qt0 = pr.tables(t32, want_qt0=True)[0][0] if need_q else None
    g = torch.Generator().manual_seed(11)
    logits = (torch.randn(N_, D_, S, generator=g) * 3.0).cuda()
    x = torch.randint(0, S, (N_, D_), generator=g).to(torch.int32).cuda()
    E = torch.empty(R_, S).exponential_(1.0, generator=g).cuda()
    return pr, qt0, float(pr.beta(t32)[0]), logits, x, E


def _bits(t):
    return t.contiguous().view(torch.int32)


def _check_lists(label, x, full, step_rows, full_probs=None, counted=True):
    """step_rows(rows_d, out, probs, changed) -> state: every row list against the full launch's `full` (and `full_probs`)."""
    S = full_probs.shape[-1] if full_probs is not None else 0
    moved = (full != x).view(-1).cpu()
    fv = full.view(-1).cpu()
    for name, rows in _row_lists(R_).items():
        rows_d = rows.to(torch.int32).cuda()
        out = torch.full((N_, D_), -7, dtype=torch.int32, device="cuda")
        probs = torch.full((N_, D_, S), -1.0, device="cuda") if full_probs is not None else None
        ch = torch.zeros(1, dtype=torch.int32, device="cuda")
        got = step_rows(rows_d, out, probs, ch)
        assert got.data_ptr() == out.data_ptr()
        listed = torch.zeros(R_, dtype=torch.bool)
        listed[rows] = True
        gv = got.view(-1).cpu()
        assert torch.equal(gv[listed], fv[listed]), (label, name)
        assert (gv[~listed] == -7).all(), (label, name)
        if counted:
            assert int(ch) == int(moved[listed].sum()), (label, name)
        if full_probs is not None:
            pg, pf = probs.view(R_, S).cpu(), full_probs.view(R_, S).cpu()
            assert torch.equal(_bits(pg[listed]), _bits(pf[listed])), (label, name)
            assert (pg[~listed] == -1.0).all(), (label, name)
    return int(moved.sum())


def _lbjf_case(S, branch, lt, call):
    from ctdd import native
    pr, qt0, beta, logits, x, E = _inputs(S, need_q=not (branch == native.BRANCH_CRM and lt == "direct"))
    flags = native.STEP_CORRECTOR if call == "corrector" else 0
    Ev = E if call == "E" else None
    wp = call == "probs"
    seed, offset = 987654321, 3
    moved_any = 0
    for h in HS:
        ch_full = torch.zeros(1, dtype=torch.int32, device="cuda")
        full = native.lbjf_step(branch, lt, logits, x, qt0, pr.base_rate, beta, 1e-9, h, flags, Ev, seed, offset, want_probs=wp,
                                changed=ch_full)
        full, fprobs = full if wp else (full, None)
        assert int(ch_full) == int((full != x).sum())

        def rows_step(rows_d, out, probs, ch):
            got = native.lbjf_step_rows(branch, lt, logits, x, qt0, pr.base_rate, beta, 1e-9, h, rows_d, flags, Ev, seed, offset,
                                        out=out, want_probs=wp, probs=probs, changed=ch)
            return got[0] if wp else got
        moved_any += _check_lists((S, lt, call, h), x, full, rows_step, fprobs)
    assert moved_any > 0


@pytest.mark.parametrize("call", ["plain", "corrector", "E", "probs"])
@pytest.mark.parametrize("S", SIZES)
def test_lbjf_rows_matches_full_launch(S, call):
    from ctdd import native
    _lbjf_case(S, native.BRANCH_CTELBO, "direct", call)


def _midpoint_case(S, branch, lt):
    from ctdd import native
    pr, qt0, beta, logits, x, _ = _inputs(S, need_q=not (branch == native.BRANCH_CRM and lt == "direct"))
    moved_any = 0
    for h in HS:
        full = native.midpoint_predict(branch, lt, logits, x, qt0, pr.base_rate, beta, 1e-9, h)
        rows_step = lambda rows_d, out, probs, ch: native.midpoint_predict_rows(branch, lt, logits, x, qt0, pr.base_rate, beta,
                                                                                1e-9, h, rows_d, out=out)
        moved_any += _check_lists((S, lt, h), x, full, rows_step, counted=False)
    assert moved_any > 0


@pytest.mark.parametrize("S", SIZES)
def test_midpoint_predict_rows_matches_full_launch(S):
    from ctdd import native
    _midpoint_case(S, native.BRANCH_CTELBO, "direct")


@pytest.mark.parametrize("lt", ["direct", "reverse_prob", "reverse_logscale"])
@pytest.mark.parametrize("S", [3, 37])
@pytest.mark.parametrize("mode", ["lbjf", "lbjf_corrector", "midpoint"])
def test_crm_rows_matches_full_launch(mode, S, lt):
    from ctdd import native
    if mode == "midpoint":
        _midpoint_case(S, native.BRANCH_CRM, lt)
    else:
        _lbjf_case(S, native.BRANCH_CRM, lt, "corrector" if mode == "lbjf_corrector" else "plain")


@pytest.mark.parametrize("call", ["plain", "E"])
@pytest.mark.parametrize("S", SIZES)
def test_exact_rows_matches_full_launch(S, call):
    from ctdd import native
    pr, _, _, logits, x, E = _inputs(S, need_q=False)
    t_lo, t_hi = torch.tensor([0.45]), torch.tensor([0.5])
    q_lo = pr.tables(t_lo, want_qt0=True)[0][0].contiguous()
    q_step = pr.transit_between(t_lo, t_hi)[0].contiguous()
    Ev = E if call == "E" else None
    seed, offset = 13579, 2
    ch_full = torch.zeros(1, dtype=torch.int32, device="cuda")
    full, fprobs = native.exact_step(logits, x, q_lo, q_step, Ev, seed, offset, want_probs=True, changed=ch_full)
    assert int(ch_full) == int((full != x).sum())
    rows_step = lambda rows_d, out, probs, ch: native.exact_step_rows(logits, x, q_lo, q_step, rows_d, Ev, seed, offset, out=out,
                                                                      want_probs=True, probs=probs, changed=ch)[0]
    assert _check_lists((S, call), x, full, rows_step, fprobs) > 0


@pytest.mark.parametrize("mode", ["x3", "bf16"])
def test_s256_tails_rows_match_full_launch(mode):
    """The pre_rates tails on listed rows: rates of the full S = 256 step, and the chain the samplers run (the listed rows' rates
    from ctdd_tauleap_step_s256_rows into a sentinel-filled buffer, then the tail)."""
    from ctdd import native
    S = 256
    pr, qt0, beta, logits, x, E = _inputs(S)
    tabs = native.S256Tables(qt0.unsqueeze(0), pr.base_rate, 1e-9, bf16=mode == "bf16")
    seed, offset = 24680, 5
    moved_l = moved_m = 0
    for h in HS:
        for flags in (0, native.STEP_CORRECTOR):
            _, rates_full = native.tauleap_step_s256(logits, x, tabs, 0, beta, h, flags, seed, offset, want_rates=True, want_x=False)
            ch_full = torch.zeros(1, dtype=torch.int32, device="cuda")
            full, fprobs = native.lbjf_from_rates(rates_full, x, h, None, seed, offset, want_probs=True, changed=ch_full)
            assert int(ch_full) == int((full != x).sum())
            full_E = native.lbjf_from_rates(rates_full, x, h, E, seed, offset)
            full_m = native.midpoint_from_rates(rates_full, x, h)

            def chain(tail):
                def run(rows_d, out, probs, ch):
                    rates = torch.full((N_, D_, S), -1.0, device="cuda")
                    none, got = native.tauleap_step_s256_rows(logits, x, tabs, 0, beta, h, flags, seed, offset, rows_d,
                                                              want_rates=True, rates=rates, want_x=False)
                    assert none is None and got.data_ptr() == rates.data_ptr()
                    listed = torch.zeros(R_, dtype=torch.bool, device="cuda")
                    listed[rows_d.long()] = True
                    assert (rates.view(R_, S)[~listed] == -1.0).all()
                    assert torch.equal(_bits(rates.view(R_, S)[listed]), _bits(rates_full.view(R_, S)[listed]))
                    return tail(rates, rows_d, out, probs, ch)
                return run
            lbjf = lambda rates, rows_d, out, probs, ch: native.lbjf_from_rates_rows(rates, x, h, rows_d, None, seed, offset, out=out,
                                                                                    want_probs=True, probs=probs, changed=ch)[0]
            lbjf_E = lambda rates, rows_d, out, probs, ch: native.lbjf_from_rates_rows(rates, x, h, rows_d, E, seed, offset, out=out,
                                                                                      changed=ch)
            mid = lambda rates, rows_d, out, probs, ch: native.midpoint_from_rates_rows(rates, x, h, rows_d, out=out)
            label = (mode, h, flags)
            moved_l += _check_lists(label + ("lbjf",), x, full, lambda *a: lbjf(rates_full, *a), fprobs)
            _check_lists(label + ("lbjf_E",), x, full_E, lambda *a: lbjf_E(rates_full, *a))
            moved_m += _check_lists(label + ("mid",), x, full_m, lambda *a: mid(rates_full, *a), counted=False)
            _check_lists(label + ("chain lbjf",), x, full, chain(lbjf), fprobs)
            _check_lists(label + ("chain mid",), x, full_m, chain(mid), counted=False)
    assert moved_l > 0 and moved_m > 0


def test_rows_defaults_aliasing_and_range():
    from ctdd import native
    S = 37
    pr, qt0, beta, logits, x, _ = _inputs(S)
    rows = torch.tensor([3, 141, 654], dtype=torch.int32).cuda()
    keep = torch.ones(R_, dtype=torch.bool, device="cuda")
    keep[rows.long()] = False
    q_step = pr.transit_between(torch.tensor([0.45]), torch.tensor([0.5]))[0].contiguous()
    calls = {
        "ctdd_lbjf_step_rows": lambda **k: native.lbjf_step_rows(native.BRANCH_CTELBO, "direct", logits, x, qt0, pr.base_rate, beta, 1e-9, 0.5, rows, **k),
        "ctdd_midpoint_predict_rows": lambda **k: native.midpoint_predict_rows(native.BRANCH_CTELBO, "direct", logits, x, qt0, pr.base_rate, beta, 1e-9, 0.5, rows, **k),
        "ctdd_exact_step_rows": lambda **k: native.exact_step_rows(logits, x, qt0, q_step, rows, **k),
        "ctdd_lbjf_from_rates_rows": lambda **k: native.lbjf_from_rates_rows(logits.abs(), x, 0.5, rows, **k),
        "ctdd_midpoint_from_rates_rows": lambda **k: native.midpoint_from_rates_rows(logits.abs(), x, 0.5, rows, **k),
    }
    for entry, call in calls.items():
        before = native.LAUNCH_COUNTS.get(entry, 0)
        out = call()
        assert native.LAUNCH_COUNTS.get(entry, 0) == before + 1
        assert out.data_ptr() != x.data_ptr() and torch.equal(out.view(-1)[keep], x.view(-1)[keep]), entry
        with pytest.raises(native.CtddError):
            call(out=x)                                           # unlisted rows are not written: aliasing refused
    # the C entry points themselves: n_rows == 0 a no-op, n_rows out of range (ERANGE), null list and aliasing (both EINVAL)
    lib = native.load()
    out = torch.empty_like(x)
    rates = logits.abs().contiguous()
    args = lambda rp, nr, o: (rates.data_ptr(), x.data_ptr(), 0.5, N_, D_, S, rp, nr, o, None)
    assert lib.ctdd_midpoint_from_rates_rows(*args(rows.data_ptr(), 0, out.data_ptr())) == 0
    rc_range = lib.ctdd_midpoint_from_rates_rows(*args(rows.data_ptr(), R_ + 1, out.data_ptr()))
    rc_null = lib.ctdd_midpoint_from_rates_rows(*args(None, 3, out.data_ptr()))
    rc_alias = lib.ctdd_midpoint_from_rates_rows(*args(rows.data_ptr(), 3, x.data_ptr()))
    assert rc_range != 0 and rc_null != 0 and rc_alias != 0 and rc_null == rc_alias and rc_range != rc_null


# ------------------------------------------------------------------------------------------------ 2. law
def coupled_logits(x, t, S, scale=2.0):
    """The coupled toy score of tests/test_gpu_conditional.py: peaked around a t-dependent shrink towards S/2 of a mix of the own
    state and the sample's MEAN state, so what is held changes the law of what is free."""
    x = x.to(torch.float32)
    N, D = x.shape
    s = torch.arange(S, dtype=torch.float32, device=x.device).view(1, 1, S)
    tt = t.to(torch.float32).view(N, 1, 1)
    mix = (0.3 * x + 0.7 * x.mean(1, keepdim=True)).unsqueeze(-1)
    centre = mix * (1.0 - 0.5 * tt) + 0.5 * tt * (S / 2.0)
    width = 0.05 * S + 0.25 * S * tt + 0.5
    return scale * (-0.5 * ((s - centre) / width) ** 2)


class CoupledToy:
    def __init__(self, kind, S, **p):
        from ctdd.process import DeviceForwardProcess
        self.process = DeviceForwardProcess(kind, S, "cuda", **p)
        self.S, self.device = S, torch.device("cuda")

    def __call__(self, x, t):
        return coupled_logits(x, t, self.S)


class FreePart:
    """The oracle's model object for the free dimensions: net(x_free, t) = coupled_logits(cat(cond, x_free), t)[:, cd:].  Every
    sample shares the time, so the (N, S, S) tables are one table expanded (no N copies of an S x S eigen-product)."""

    def __init__(self, proc, cond, S):
        self.proc, self.cond, self.S, self.cd = proc, cond, S, cond.shape[1]

    def __call__(self, x, t, *a):
        return coupled_logits(torch.cat((self.cond, x), 1), t, self.S)[:, self.cd:]

    def _one(self, f, *ts):
        return f(*(t[:1] for t in ts)).expand(ts[0].shape[0], self.S, self.S)

    def transition(self, t):
        return self._one(self.proc.transition, t)

    def rate(self, t):
        return self._one(self.proc.rate, t)

    def rate_mat(self, y, t):
        return self.rate(t)[torch.arange(y.shape[0]).view(-1, 1), y.long()]

    def transit_between(self, t1, t2):
        return self._one(self.proc.transit_between, t1, t2)


def _two_sample_chi2(a, b, S):
    ca = np.bincount(a.ravel(), minlength=S).astype(np.float64)
    cb = np.bincount(b.ravel(), minlength=S).astype(np.float64)
    m = (ca + cb) > 0
    k1, k2 = np.sqrt(cb.sum() / ca.sum()), np.sqrt(ca.sum() / cb.sum())
    return (((k1 * ca - k2 * cb) ** 2)[m] / (ca + cb)[m]).sum(), int(m.sum()) - 1


def _law_cfg(name, S, D, cd, loss="CTElbo", logit_type="direct", **over):
    from config.mnist_config.config_tauUnet_mnist import get_config
    c = get_config()
    c.data.S, c.model.concat_dim = S, D
    c.loss.name, c.loss.logit_type = loss, logit_type
    c.sampler.name, c.sampler.condition_dim = name, cd
    c.sampler.num_steps = 10
    c.sampler.num_corrector_steps = 0
    c.sampler.step_precision = "fp32"
    for k, v in over.items():
        c.sampler[k] = v
    return c


def law_reference(name, cfg, cond, D, S, loss, lt):
    """The oracle's own loop of the parent sampler on the D - cd free dimensions (x_init=None), the conditioner in front."""
    N, cd = cond.shape
    s = cfg.sampler
    om = FreePart(ForwardProcess("gaussian", S, **GAUSS), cond, S)
    common = dict(max_t=cfg.training.max_t, min_t=s.min_t, num_steps=s.num_steps, initial_dist=s.initial_dist,
                  init_std=cfg.model.Q_sigma, x_init=None)
    if name == "ConditionalLBJF":
        ref = osamp.lbjf_sample(om, N, D - cd, S, eps_ratio=s.eps_ratio, loss_name=loss, logit_type=lt,
                                corrector_entry_time=s.corrector_entry_time, num_corrector_steps=s.num_corrector_steps, **common)
    elif name == "ConditionalMidPointTauL":
        ref = osamp.midpoint_sample(om, N, D - cd, S, eps_ratio=s.eps_ratio, is_ordinal=s.is_ordinal, loss_name=loss,
                                    logit_type=lt, **common)
    else:
        ref = osamp.exact_sample(om, N, D - cd, S, **common)
    return np.concatenate((cond.numpy().astype(int), ref[0]), 1)


# (name, S, loss, logit type, N).  N = 2000 everywhere but the CRM case: without the final argmax its samples keep the noise of
# min_t, and on the CPU restatement ALONE two constant conditioners reach only chi2 = 223 against the bound 256 in one free
# dimension at N = 2000; the statistic grows linearly in N, so that case runs 4000 samples (the bound stays).
LAW_CASES = [("ConditionalLBJF", 3, "CTElbo", "direct", 2000), ("ConditionalLBJF", 37, "CTElbo", "direct", 2000),
             ("ConditionalLBJF", 256, "CTElbo", "direct", 2000), ("ConditionalLBJF", 37, "CatRM", "reverse_prob", 4000),
             ("ConditionalMidPointTauL", 3, "CTElbo", "direct", 2000), ("ConditionalMidPointTauL", 37, "CTElbo", "direct", 2000),
             ("ConditionalMidPointTauL", 256, "CTElbo", "direct", 2000),
             ("ConditionalExactSampling", 3, "CTElbo", "direct", 2000), ("ConditionalExactSampling", 37, "CTElbo", "direct", 2000)]
LAW_D, LAW_CD = 12, 4


def law_cfg(name, S, loss, lt):
    # the grid starts at cfg.training.max_t = 1.0, where sqrt_cos schedules are singular: the Gaussian process at every S
    over = dict(initial_dist="uniform" if S == 3 else "gaussian")
    if name == "ConditionalLBJF":
        over.update(corrector_entry_time=0.6, num_corrector_steps=1)     # (the grid runs 1.0 ... 0.01: correctors on its lower half)
    return _law_cfg(name, S, LAW_D, LAW_CD, loss, lt, **over)


def law_conditioner(S, N):
    return torch.randint(0, S, (N, LAW_CD), generator=torch.Generator().manual_seed(2))


def assert_same_law(a, b, S, cd):
    N, D = a.shape
    for d in range(cd, D):
        chi2, dof = _two_sample_chi2(a[:, d], b[:, d], S)
        assert chi2 < dof + 6 * np.sqrt(2 * dof) + 10, (d, chi2, dof)
    se = np.sqrt(a[:, cd:].var(0) / N + b[:, cd:].var(0) / N) + 1e-9
    assert (np.abs(a[:, cd:].mean(0) - b[:, cd:].mean(0)) / se).max() < 5.5


def assert_conditioner_matters(lo, hi, S, cd):
    for d in range(cd, lo.shape[1]):
        chi2, dof = _two_sample_chi2(lo[:, d], hi[:, d], S)
        assert chi2 > dof + 20 * np.sqrt(2 * dof) + 50, (d, chi2, dof)


@pytest.mark.parametrize("name,S,loss,lt,N", LAW_CASES)
def test_conditional_law_matches_oracle_on_free_part(name, S, loss, lt, N):
    """Criteria of test_conditional_law_matches_reference_restatement (per free dimension two-sample chi-square, standardised
    mean difference, two constant conditioners apart).  The reference alone passes them at these shapes: each CPU restatement
    run twice with different torch seeds agrees with itself within the same bounds (checked on the CPU for every case)."""
    import lib.sampling.sampling  # noqa: F401
    import lib.sampling.sampling_utils as su
    from ctdd import native
    D, cd = LAW_D, LAW_CD
    cfg = law_cfg(name, S, loss, lt)
    sampler = su.get_sampler(cfg)
    sampler.seed = 4321
    assert sampler.branch == (native.BRANCH_CTELBO if loss == "CTElbo" else native.BRANCH_CRM) and sampler.logit_type == lt
    model = CoupledToy("gaussian", S, **GAUSS)
    cond = law_conditioner(S, N)
    before = dict(native.LAUNCH_COUNTS)
    out = sampler.sample(model, N, cond)
    d = _delta(before)
    hip = out[0]
    if name == "ConditionalLBJF":
        ran = ("ctdd_tauleap_step_s256_rows", "ctdd_lbjf_from_rates_rows") if S == 256 else ("ctdd_lbjf_step_rows",)
        assert len(out) == 2 and len(out[1]) == cfg.sampler.num_steps
    elif name == "ConditionalMidPointTauL":
        ran = (("ctdd_tauleap_step_s256_rows", "ctdd_midpoint_from_rates_rows") if S == 256
               else ("ctdd_midpoint_predict_rows", "ctdd_tauleap_step_rows"))
        assert len(out) == 5
    else:
        ran = ("ctdd_exact_step_rows",)
        assert len(out) == 2 and len(out[1]) == cfg.sampler.num_steps
    assert all(d[e] > 0 for e in ran), d
    assert hip.shape == (N, D) and hip.dtype.kind == "i" and hip.min() >= 0 and hip.max() < S
    assert (hip[:, :cd] == cond.numpy()).all()
    torch.manual_seed(7)
    ref = law_reference(name, cfg, cond, D, S, loss, lt)
    assert_same_law(hip, ref, S, cd)
    lo = sampler.sample(model, N, torch.full((N, cd), S // 5))[0]
    hi = sampler.sample(model, N, torch.full((N, cd), S - 1 - S // 5))[0]
    assert_conditioner_matters(lo, hi, S, cd)


# ------------------------------------------------------------------------------------------------ 3. identities
class DeterministicToy:
    def __init__(self, S):
        from ctdd.process import DeviceForwardProcess
        self.process = DeviceForwardProcess("gaussian", S, "cuda", **GAUSS)
        self.S, self.device = S, torch.device("cuda")

    def __call__(self, x, t):
        return toy_logits(x, t, self.S, 2.0)


def _id_cfg(name, S, D=23):
    c = _law_cfg(name, S, D, 5, initial_dist="uniform" if S == 3 else "gaussian")
    c.sampler.num_steps = 6
    pc = name in ("PCTauL", "ConditionalPCTauLeaping")
    if name.endswith("LBJF") or pc:
        c.sampler.corrector_entry_time, c.sampler.num_corrector_steps = 0.6, 1
    if name in ("TauL", "ConditionalTauLeaping"):                # TauL set to what ConditionalTauLeaping fixes (no corrector: _law_cfg)
        c.training.max_t, c.sampler.is_ordinal = 1.0, True
    if pc and S == 256:
        c.model.Q_sigma = 200                                    # the initial std PCTauL hard-codes (S = 3 starts uniform)
    return c


# parent -> (its conditional sampler, length of the return tuple; 0: a bare array from the conditional sampler)
ID_PAIRS = {"LBJF": ("ConditionalLBJF", 2), "MidPointTauL": ("ConditionalMidPointTauL", 5), "ExactSampling": ("ConditionalExactSampling", 2),
            "TauL": ("ConditionalTauLeaping", 0), "PCTauL": ("ConditionalPCTauLeaping", 0)}


def _same(a, b):
    if isinstance(a, np.ndarray):
        return a.shape == b.shape and (a == b).all()
    return len(a) == len(b) and all(u == v or (u != u and v != v) for u, v in zip(a, b))


@pytest.mark.parametrize("S", [3, 256])
@pytest.mark.parametrize("parent", list(ID_PAIRS))
def test_all_free_mask_is_the_parent_sampler(parent, S):
    import lib.sampling.sampling  # noqa: F401
    import lib.sampling.sampling_utils as su
    from ctdd import native
    N, D = 37, 23
    model = DeterministicToy(S)
    child, n_out = ID_PAIRS[parent]
    ps = su.get_sampler(_id_cfg(parent, S))
    cs = su.get_sampler(_id_cfg(child, S))
    ps.seed = cs.seed = 99
    want = ps.sample(model, N)
    before = dict(native.LAUNCH_COUNTS)
    got = cs.inpaint(model, torch.zeros((N, D), dtype=torch.int64), torch.zeros(D, dtype=torch.bool))
    assert sum(_delta(before).values()) > 0
    if n_out == 0:                                               # (x, changed) from TauL, a bare array from PCTauL and both children
        want, got, n_out = (want[0] if parent == "TauL" else want,), (got,), 1
    assert len(got) == len(want) == n_out
    for k, (a, b) in enumerate(zip(got, want)):
        assert _same(a, b), (parent, S, k)
    assert (want[0] != want[0][:1]).any()                        # (the run does move: not a constant state)


@pytest.mark.parametrize("S", [3, 256])
@pytest.mark.parametrize("parent", list(ID_PAIRS))
def test_all_held_mask_returns_known_and_launches_nothing(parent, S):
    import lib.sampling.sampling  # noqa: F401
    import lib.sampling.sampling_utils as su
    from ctdd import native
    N, D = 9, 23
    child, n_out = ID_PAIRS[parent]
    cs = su.get_sampler(_id_cfg(child, S))
    xk = torch.randint(0, S, (N, D), generator=torch.Generator().manual_seed(1))
    before = dict(native.LAUNCH_COUNTS)
    out = cs.inpaint(DeterministicToy(S), xk, torch.ones((N, D), dtype=torch.bool))
    if n_out == 0:
        out, n_out = (out,), 1
    assert (out[0] == xk.numpy()).all() and len(out) == n_out
    assert all(native.LAUNCH_COUNTS.get(k, 0) == before.get(k, 0) for k in native.LAUNCH_COUNTS)


# ------------------------------------------------------------------------------------------------ 4. engines
def _run(cfg, name, how, seed=77, **over):
    import lib.sampling.sampling_utils as su
    from ctdd import native
    c = copy.deepcopy(cfg)
    c.sampler.name = name
    for k, v in over.items():
        c.sampler[k] = v
    sampler = su.get_sampler(c)
    sampler.seed = seed
    before = dict(native.LAUNCH_COUNTS)
    out = how(sampler)
    return sampler, out, _delta(before)


@pytest.fixture(scope="module")
def maze_hollow():
    import lib.models.models  # noqa: F401
    import lib.models.model_utils as mu
    import lib.sampling.sampling  # noqa: F401
    from config.maze_config.config_hollow_maze import get_config
    cfg = get_config()
    torch.manual_seed(0)
    model = mu.create_model(cfg, torch.device("cuda"))
    model.eval()
    return cfg, model


@pytest.mark.parametrize("name,entry", [("ConditionalLBJF", "ctdd_lbjf_step_rows"),
                                        ("ConditionalMidPointTauL", "ctdd_midpoint_predict_rows")])
def test_maze_hollow_inpaint(maze_hollow, name, entry):
    from ctdd import native
    cfg, model = maze_hollow
    N, D, S = 64, cfg.model.concat_dim, cfg.data.S
    g = torch.Generator().manual_seed(4)
    x_known = torch.randint(0, S, (N, D), generator=g)
    mask = torch.rand(N, D, generator=g) < 0.5
    how = lambda s: s.inpaint(model, x_known, mask)
    sampler, out, delta = _run(cfg, name, how, num_steps=6)
    assert sampler.branch == native.BRANCH_CRM and sampler.logit_type == cfg.loss.logit_type
    x = out[0]
    assert x.shape == (N, D) and x.min() >= 0 and x.max() < S
    assert (x[mask.numpy()] == x_known.numpy()[mask.numpy()]).all()
    assert (x[~mask.numpy()] != x_known.numpy()[~mask.numpy()]).any()
    assert delta[entry] > 0
    _, again, _ = _run(cfg, name, how, num_steps=6)
    assert (again[0] == x).all()                                  # fixed seed: the same samples


def test_masked_synthetic_prefix_sample():
    import lib.models.models  # noqa: F401
    import lib.models.model_utils as mu
    import lib.sampling.sampling  # noqa: F401
    from config.synthetic_config.config_masked_synthetic import get_config
    cfg = get_config()
    D, S = cfg.model.concat_dim, cfg.data.S
    k = max(1, D // 4)
    cfg.model.conditional_dim = cfg.sampler.condition_dim = k
    torch.manual_seed(0)
    model = mu.create_model(cfg, torch.device("cuda"))
    model.eval()
    N = 64
    cond = torch.randint(0, S, (N, k), generator=torch.Generator().manual_seed(3))
    how = lambda s: s.sample(model, N, cond)
    _, out, delta = _run(cfg, "ConditionalLBJF", how, num_steps=6)
    x = out[0]
    assert x.shape == (N, D) and x.min() >= 0 and x.max() < S
    assert (x[:, :k] == cond.numpy()).all()
    assert delta["ctdd_lbjf_step_rows"] > 0
    _, again, _ = _run(cfg, "ConditionalLBJF", how, num_steps=6)
    assert (again[0] == x).all()
