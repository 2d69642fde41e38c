"""GPU: ctdd_absorb_filter (csrc/absorb.hip) and the temperature / top_k / top_p keys of the four absorbing samplers -- the kept sets
against the fp64 replay of tests/absorb_filter_cases.py (top-k alone: every masked row; with top-p: every row whose boundary the
replay does not call near, and at most the boundary state on the others), the kept values bit for bit, untouched and unread rows,
the in-place call, the exact and the in-law composition with ctdd_absorb_step, the samplers, the argument errors."""
import functools
import math

import numpy as np
import pytest
import torch

import absorb_filter_cases as fc
from ctdd import native, process
from oracle.toy_model import toy_logits

pytestmark = pytest.mark.gpu

DEV = "cuda"
ARGMAX = native.ABSORB_ARGMAX
NAME = "ctdd_absorb_filter"
NINF = np.float32(-np.inf)


@functools.lru_cache(maxsize=None)
def _on_device(case, mode):
    return fc.inputs(case).to(DEV), fc.x_of(case, mode).to(DEV)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _launches():
    return native.LAUNCH_COUNTS.get(NAME, 0)


def _check_against_replay(case, mode, T, k, p):
    """One in-place call against the replay.  Returns (masked rows, rows left out of the exact comparison)."""
    S, m = case
    lg, x = _on_device(case, mode)
    flat = fc.inputs(case).view(-1, S).numpy()
    masked = (fc.x_of(case, mode).view(-1) == m).numpy()
    rep = fc.replay(flat, m, T, k, p)
    work = lg.clone()
    before = _launches()
    ret = native.absorb_filter(work, x, m, T, k, p, out=work)
    assert _launches() == before + 1 and ret.data_ptr() == work.data_ptr()
    got = work.view(-1, S).cpu().numpy()
    # rows that are not masked: the bits that came in
    assert (_bits(got[~masked]) == _bits(flat[~masked])).all(), "an unmasked row was written"
    # the row without a finite real-state logit comes back as it was; the other masked rows have -inf at the mask state
    live = masked & ~rep["dead"]
    assert (_bits(got[masked & rep["dead"]]) == _bits(flat[masked & rep["dead"]])).all(), "a row without a finite logit was rewritten"
    assert (got[live][:, m] == NINF).all(), "the mask state's column is not -inf"
    # values: a finite output is the fp32 quotient bit for bit, everything else is -inf (never NaN)
    kept = np.isfinite(got) & live[:, None]
    assert (_bits(got[kept]) == _bits(rep["v"][kept])).all(), "a kept output is not the fp32 quotient"
    assert (got[live[:, None] & ~kept] == NINF).all(), "a dropped output is neither -inf nor finite"
    assert kept[live].any(axis=1).all(), "a masked row kept nothing"
    # kept sets
    wrong = (kept != rep["kept"]).any(axis=1) & live
    assert not (wrong & ~rep["near"]).any(), f"kept set differs from the replay's on rows {np.nonzero(wrong & ~rep['near'])[0][:8]}"
    for r in np.nonzero(wrong)[0]:                                       # near rows: the one state at the boundary
        diff = np.nonzero(kept[r] != rep["kept"][r])[0]
        assert diff.size == 1 and diff[0] in rep["edge"][r], f"row {r}: states {diff} differ, boundary {rep['edge'][r]}"
    return int(live.sum()), int((rep["near"] & live).sum())


@pytest.mark.parametrize("mode", fc.MODES)
@pytest.mark.parametrize("case", fc.CASES, ids=fc.IDS)
def test_top_k_alone(case, mode):
    S, m = case
    for T in fc.TEMPS:
        for k in fc.k_options(S):
            rows, near = _check_against_replay(case, mode, T, k, 1.0)
            assert near == 0                                             # only comparisons are involved: no row is left out
    assert (rows == 0) == (mode == "none")


@pytest.mark.parametrize("mode", ("mix", "all"))
@pytest.mark.parametrize("case", fc.CASES, ids=fc.IDS)
def test_top_p_and_top_k_with_top_p(case, mode):
    S, m = case
    for T in fc.TEMPS:
        for p in fc.PS:
            for k in (0, 5):
                rows, near = _check_against_replay(case, mode, T, k, p)
                print(f"S={S} {mode} T={T} k={k} p={p}: {near} of {rows} masked rows left out of the exact comparison ({near / rows:.3%})")
                assert near <= 0.03 * rows
    _check_against_replay(case, mode, 1.0, 0, 1e-6)                      # the shortest prefix is the first state
    _check_against_replay(case, mode, 0.7, 2, 0.999)


@pytest.mark.parametrize("case", fc.CASES, ids=fc.IDS)
def test_untouched_and_unread_rows(case):
    S, m = case
    lg, x = _on_device(case, "mix")
    flat = fc.inputs(case).view(-1, S).numpy()
    masked = (fc.x_of(case, "mix").view(-1) == m).numpy()
    T, k, p = 0.7, 5, 0.9
    before = _launches()
    out = native.absorb_filter(lg, x, m, T, k, p)                        # out of place
    assert _launches() == before + 1 and out.data_ptr() != lg.data_ptr()
    assert (_bits(lg.view(-1, S).cpu().numpy()) == _bits(flat)).all(), "the out-of-place call wrote into logits"
    got = out.view(-1, S).cpu().numpy()
    assert (_bits(got[~masked]) == _bits(flat[~masked])).all()
    assert (_bits(got[fc.ROW_INF]) == _bits(flat[fc.ROW_INF])).all() and masked[fc.ROW_INF]
    nan_at = np.isnan(flat[fc.ROW_NAN])
    assert nan_at.sum() == 1 and masked[fc.ROW_NAN]
    if S == 2:                                                           # the one real state is the NaN: a row without a finite logit
        assert (_bits(got[fc.ROW_NAN]) == _bits(flat[fc.ROW_NAN])).all()
    else:
        assert (got[fc.ROW_NAN, nan_at] == NINF).all() and np.isfinite(got[fc.ROW_NAN]).any(), "the NaN was kept"
    into = torch.full_like(lg, 7.0)                                      # a given buffer: the unmasked rows are not written
    native.absorb_filter(lg, x, m, T, k, p, out=into)
    into = into.view(-1, S).cpu().numpy()
    assert (into[~masked] == 7.0).all() and (_bits(into[masked]) == _bits(got[masked])).all()
    work = lg.clone()                                                    # in place: the same bits
    native.absorb_filter(work, x, m, T, k, p, out=work)
    assert (_bits(work.view(-1, S).cpu().numpy()) == _bits(got)).all()
    poisoned = lg.clone()                                                # NaN at every unmasked row: those rows are not read
    poisoned.view(-1, S)[torch.from_numpy(~masked).to(DEV)] = float("nan")
    native.absorb_filter(poisoned, x, m, T, k, p, out=poisoned)
    again = poisoned.view(-1, S).cpu().numpy()
    assert (_bits(again[masked]) == _bits(got[masked])).all() and np.isnan(again[~masked]).all()
    # nothing masked: nothing moves
    none = lg.clone()
    native.absorb_filter(none, _on_device(case, "none")[1], m, T, k, p, out=none)
    assert (_bits(none.view(-1, S).cpu().numpy()) == _bits(flat)).all()
    # an unaligned base (the scalar path where S % 4 == 0 would take float4)
    if S % 4 == 0:
        pad = torch.empty(lg.numel() + 1, device=DEV)
        off = pad[1:].view(lg.shape)
        off.copy_(lg)
        native.absorb_filter(off, x, m, T, k, p, out=off)
        assert (_bits(off.view(-1, S).cpu().numpy()) == _bits(got)).all()


# ------------------------------------------------------------------------------------------------ composition with the step
def _ordinary(case, mode):
    """The masked rows with a finite real-state logit and no NaN (the argmax of the others is not defined)."""
    S, m = case
    flat = fc.inputs(case).view(-1, S).numpy()
    rows = (fc.x_of(case, mode).view(-1) == m).numpy().copy()
    rows[[fc.ROW_INF, fc.ROW_NAN]] = False
    return rows, flat


@pytest.mark.parametrize("case", fc.CASES, ids=fc.IDS)
def test_one_state_left_is_the_argmax(case):
    S, m = case
    lg, x = _on_device(case, "mix")
    rows, flat = _ordinary(case, "mix")
    greedy = native.absorb_step(lg, x, m, 1.0, ARGMAX, 5, 0).view(-1).cpu().numpy()
    l = flat.astype(np.float64).copy()
    l[:, m] = -np.inf
    assert (greedy[rows] == l.argmax(axis=1)[rows]).all()                # (lowest index on ties)
    for kw in (dict(top_k=1), dict(top_p=1e-6), dict(temperature=0.7, top_k=1, top_p=0.5)):
        filtered = native.absorb_filter(lg, x, m, **kw)
        assert (np.isfinite(filtered.view(-1, S).cpu().numpy()[rows]).sum(axis=1) == 1).all()
        for offset in range(2):
            drawn = native.absorb_step(filtered, x, m, 1.0, 0, 0xF117E5 + S, offset).view(-1).cpu().numpy()
            assert (drawn[rows] == greedy[rows]).all(), f"{kw}: a draw from one state left is not the argmax"


@pytest.mark.parametrize("case", fc.CASES, ids=fc.IDS)
def test_no_draw_outside_the_kept_set(case):
    S, m = case
    lg, x = _on_device(case, "all")
    rows, _ = _ordinary(case, "all")
    filtered = native.absorb_filter(lg, x, m, 1.0, 5, 0.9)
    kept = np.isfinite(filtered.view(-1, S).cpu().numpy())
    idx = np.nonzero(rows)[0]
    for offset in range(8):
        drawn = native.absorb_step(filtered, x, m, 1.0, 0, 0xD0A5 + S, offset).view(-1).cpu().numpy()
        assert kept[idx, drawn[idx]].all(), "a draw fell outside the kept set"


@pytest.mark.parametrize("S,m,k,scale", [(5, 2, 3, 1.5), (257, 256, 40, 3.0)])
def test_draws_follow_the_truncated_law(S, m, k, scale):
    """One logit row ~ N(0, scale^2) 40 000 times (S = 5: top_k cuts four states to three and top_p keeps them; S = 257: top_k cuts to 40
    and top_p to 11): after the filter at T = 0.7, top_k = k, top_p = 0.9 the picks of ctdd_absorb_step at p = 1 are
    Binomial(R, q_s) / R with q the fp64 tempered, truncated, renormalised probabilities; bars: five standard deviations;
    outside the kept set the frequency is exactly zero."""
    R, T, p = 40000, 0.7, 0.9
    g = torch.Generator().manual_seed(77 + S)
    row = scale * torch.randn(S, generator=g)
    row[m] = row.max() + 50.0
    q = fc.probs(row.numpy(), m, T, k, p)
    assert 1 < (q > 0).sum() <= k and q[m] == 0.0
    lg = row.to(DEV).expand(R, 1, S).contiguous()
    x = torch.full((R, 1), m, dtype=torch.int32, device=DEV)
    native.absorb_filter(lg, x, m, T, k, p, out=lg)
    drawn = native.absorb_step(lg, x, m, 1.0, 0, 0x1A3 + S, 3).view(-1).cpu().numpy()
    freq = np.bincount(drawn, minlength=S) / R
    bar = 5 * np.sqrt(q * (1 - q) / R)
    worst = np.abs(freq - q)[q > 0] / bar[q > 0]
    print(f"S={S}: {(q > 0).sum()} states kept; largest |freq - q| / bar = {worst.max():.3f}")
    assert (freq[q == 0] == 0).all() and (np.abs(freq - q)[q > 0] <= bar[q > 0]).all()


# ------------------------------------------------------------------------------------------------ the samplers
S_, M_, N_, D_, K_ = 5, 2, 16, 50, 12
SEED = 20250611
SAMPLERS = ("AbsorbingLeap", "AbsorbingConfidence", "AbsorbingRemask", "AbsorbingFirstHit")


class _ToyModel:
    """toy_logits of the state itself (the mask state read as a value), the time and the dimension."""

    def __init__(self):
        self.S, self.device = S_, DEV
        self.process = process.DeviceForwardProcess("absorbing", S_, DEV, rate_const=1.0, t_func="loglinear", alpha_eps=1e-3, mask_state=M_)

    def __call__(self, x, t):
        return toy_logits(x, t, self.S, scale=3.0)


def _sampler(name, **kw):
    import lib.sampling.sampling  # noqa: F401
    import lib.sampling.sampling_utils as su
    from ctdd.config_dict import ConfigDict
    cfg = ConfigDict()
    for sec in ("data", "model", "sampler", "training", "loss"):
        cfg[sec] = ConfigDict()
    cfg.data.S, cfg.model.concat_dim, cfg.training.max_t = S_, D_, 1.0
    cfg.sampler.update(name=name, num_steps=K_, min_t=0.01)
    if name == "AbsorbingRemask":
        cfg.sampler.update(remask="conf", remask_eta=0.05)
    cfg.sampler.update(**kw)
    sampler = su.get_sampler(cfg)
    sampler.seed = SEED
    return sampler


def _iterations(sampler):
    return sampler.plan(D_)[1] if type(sampler).__name__ == "AbsorbingFirstHit" else K_


@pytest.mark.parametrize("name", SAMPLERS)
def test_neutral_keys_change_nothing(name):
    model = _ToyModel()
    x0, c0 = _sampler(name).sample(model, N_)
    before = _launches()
    x1, c1 = _sampler(name, temperature=1, top_k=0, top_p=1).sample(model, N_)
    assert _launches() == before, "the filter was launched at the neutral values"
    assert (x0 == x1).all() and c0 == c1
    assert (x0 != M_).all()


def test_top_k_one_makes_the_sampled_candidate_the_argmax():
    model = _ToyModel()
    a, ca = _sampler("AbsorbingFirstHit", candidate="sample", top_k=1).sample(model, N_)
    b, cb = _sampler("AbsorbingFirstHit", candidate="argmax").sample(model, N_)
    plain, _ = _sampler("AbsorbingFirstHit", candidate="sample").sample(model, N_)
    assert (a == b).all() and ca == cb
    assert (plain != b).any(), "the unfiltered draw is the argmax everywhere: the test shows nothing"


@pytest.mark.parametrize("name", SAMPLERS)
def test_one_filter_launch_per_iteration(name):
    model = _ToyModel()
    sampler = _sampler(name, temperature=0.7, top_k=3, top_p=0.9)
    before = _launches()
    x, _ = sampler.sample(model, N_)
    assert _launches() - before == _iterations(sampler), "one launch per loop iteration, none for the closing step"
    assert x.shape == (N_, D_) and (x != M_).all() and ((x >= 0) & (x < S_)).all()
    again, _ = sampler.sample(model, N_)
    assert (again == x).all()                                            # a fixed seed fixes the sample
    # top_k = 1 at every step: every entry is its step's argmax, whatever the sampler
    greedy, _ = _sampler(name, top_k=1).sample(model, N_)
    assert (greedy != M_).all()


@pytest.mark.parametrize("name", SAMPLERS)
def test_inpaint_keeps_its_held_entries(name):
    model = _ToyModel()
    g = torch.Generator().manual_seed(5)
    x_known = torch.randint(0, S_ - 1, (N_, D_), generator=g)
    x_known = x_known + (x_known >= M_).long()                           # skips the mask state
    held = torch.rand(N_, D_, generator=g) < 0.4
    sampler = _sampler(name, temperature=0.8, top_p=0.8)
    before = _launches()
    out = sampler.inpaint(model, x_known, held)
    assert _launches() > before
    hn = held.numpy()
    assert out.shape == (N_, D_) and (out[hn] == x_known.numpy()[hn]).all(), "a held entry moved"
    assert (out != M_).all() and ((out >= 0) & (out < S_)).all()


# ------------------------------------------------------------------------------------------------ argument errors
def test_filter_argument_errors():
    lg = torch.zeros(2, 3, 4, device=DEV)
    x = torch.full((2, 3), 3, dtype=torch.int32, device=DEV)
    buf = torch.zeros(32, device=DEV)
    call, E = native.absorb_filter, native.CtddError
    bad_calls = [
        lambda: call(lg, x, 3, 0.0),                                                                 # T <= 0, non-finite T
        lambda: call(lg, x, 3, -1.0),
        lambda: call(lg, x, 3, math.inf),
        lambda: call(lg, x, 3, math.nan),
        lambda: call(lg, x, 3, 1.0, -1),                                                             # k < 0
        lambda: call(lg, x, 3, 1.0, 0, 0.0),                                                         # p outside (0, 1]
        lambda: call(lg, x, 3, 1.0, 0, 1.5),
        lambda: call(lg, x, 3, 1.0, 0, -0.5),
        lambda: call(lg, x, 3, 1.0, 0, math.nan),
        lambda: call(torch.zeros(1, 2, native.ABSORB_MAX_S + 1, device=DEV), x[:1, :2].contiguous(), 3),   # S > CTDD_MAX_S
        lambda: call(lg, x, 4),                                                                      # mask_state outside [0, S)
        lambda: call(lg, x, -1),
        lambda: call(lg.double(), x, 3),                                                             # dtypes
        lambda: call(lg, x.long(), 3),
        lambda: call(lg, x, 3, out=torch.zeros(2, 3, 4, dtype=torch.float64, device=DEV)),
        lambda: call(lg, x[:, :2].contiguous(), 3),                                                  # shapes
        lambda: call(lg, x, 3, out=torch.zeros(2, 3, 5, device=DEV)),
        lambda: call(lg[0], x[0], 3),
        lambda: call(lg, x, 3, out=torch.zeros(2, 4, 3, device=DEV).transpose(1, 2)),                # not contiguous
        lambda: call(buf[:24].view(2, 3, 4), x, 3, out=buf[4:28].view(2, 3, 4)),                     # out overlaps logits without being it
    ]
    for i, c in enumerate(bad_calls):
        with pytest.raises(E):
            c()
            pytest.fail(f"bad call {i} went through")
    out = call(lg, x, 3, 0.5, 1, 0.5)
    got = out.cpu().numpy()
    assert (got[..., 0] == 0.0).all() and (got[..., 1:] == NINF).all()   # all-equal logits: the lowest state stays
