"""GPU: the first-hitting sampler on ctdd_absorb_hit_time / ctdd_absorb_hit_step (csrc/absorb.hip) -- the event counts, levels and
evaluation times against the fp64 replay on all four schedules (counts exact away from the closing level, levels to 1e-12 relative,
times to one fp32 ulp); the selected rows against the replay of the Philox keys, their states against ctdd_absorb_step itself at
p = 1 under the same seed and offset, bit for bit; untouched rows, the in-place calls, the counter, logits that are never read; and
the AbsorbingFirstHit sampler's statistics against the law of the exact chain (bars from the binomial law)."""
import math

import numpy as np
import pytest
import torch

import absorb_cases as ac
import absorb_hit_cases as hc
from ctdd import native, process
from oracle.toy_model import toy_logits

pytestmark = pytest.mark.gpu

DEV = "cuda"
ARGMAX = native.ABSORB_ARGMAX


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(DEV)


# ------------------------------------------------------------------------------------------------ hit_time
T_MIN, T_MAX = hc.T_MIN, hc.T_MAX


@pytest.mark.parametrize("t_func,rate_const", hc.SCHEDULES)
@pytest.mark.parametrize("N,D", hc.TIME_SHAPES)
def test_hit_time_against_the_replay(N, D, t_func, rate_const):
    pr = hc.proc(t_func, rate_const)
    m = pr.mask_state
    x, logc = hc.time_inputs(N, D, pr)
    xd, ld = _dev(x, torch.int32), _dev(logc, torch.float64)
    M = (x == m).sum(1)
    assert M[0] == 0 and M[1] > 0
    for kmax in hc.KMAX:
        seed, offset = hc.time_seed(D, kmax)
        cuts, big, big_count = hc.closing_levels(x, logc, m, kmax, pr, seed, offset)
        for log_cmin in cuts:
            counts, out, t64, near = hc.hit_time_replay(x, logc, m, kmax, log_cmin, pr, T_MIN, T_MAX, seed, offset)
            assert not near.any(), "the seed puts an event within 1e-9 of the closing level"
            before = native.LAUNCH_COUNTS.get("ctdd_absorb_hit_time", 0)
            gc, gt, go = native.absorb_hit_time(xd, ld, m, kmax, log_cmin, pr.p, T_MIN, T_MAX, seed, offset)
            assert native.LAUNCH_COUNTS["ctdd_absorb_hit_time"] == before + 1
            assert gc.dtype == torch.int32 and gt.dtype == torch.float32 and go.dtype == torch.float64
            gc, gt, go = gc.cpu().numpy(), gt.cpu().numpy(), go.cpu().numpy()
            t32 = t64.astype(np.float32)
            err = np.abs(go - out)
            print(f"{t_func} N={N} D={D} kmax={kmax} log_cmin={log_cmin:.4f}: M {M.tolist()} counts {gc.tolist()}; level error "
                  f"{err.tolist()} at {out.tolist()}; t_eval {gt.tolist()} against {t64.tolist()}")
            assert (gc == counts).all()
            assert (err <= 1e-12 * np.abs(out)).all() and (go[counts < np.minimum(kmax, M)] == log_cmin).all()
            assert (np.abs(gt.astype(np.float64) - t32.astype(np.float64)) <= np.spacing(t32).astype(np.float64)).all()
            assert (gt >= np.float32(T_MIN)).all() and (gt <= np.float32(T_MAX)).all()
            # a sample with nothing masked is untouched
            assert gc[0] == 0 and go[0].tobytes() == logc[0].tobytes() and gt[0] == np.float32(T_MIN)
            if log_cmin > -math.inf:
                assert gc[big] == big_count and go[big] == log_cmin
            # the aliased level buffer
            la = ld.clone()
            ac_, at_, ao_ = native.absorb_hit_time(xd, la, m, kmax, log_cmin, pr.p, T_MIN, T_MAX, seed, offset, out=la)
            assert ao_.data_ptr() == la.data_ptr()
            assert (ac_.cpu().numpy() == gc).all() and at_.cpu().numpy().tobytes() == gt.tobytes() and la.cpu().numpy().tobytes() == go.tobytes()
            assert ld.cpu().numpy().tobytes() == logc.tobytes(), "the out-of-place call wrote into logc"


def test_hit_time_argument_errors():
    x = torch.full((2, 3), 3, dtype=torch.int32, device=DEV)
    logc = torch.zeros(2, dtype=torch.float64, device=DEV)
    ok = dict(t_func="log", rate_const=0.5, time_base=3.0, time_exp=100.0)
    call, E = native.absorb_hit_time, native.CtddError
    bad_calls = [
        lambda: call(x, logc, 3, 0, -1.0, ok, 0.01, 1.0),                                            # kmax < 1
        lambda: call(x, logc, -1, 1, -1.0, ok, 0.01, 1.0),                                           # mask_state < 0
        lambda: call(x, logc, 3, 1, math.nan, ok, 0.01, 1.0),                                        # NaN closing level
        lambda: call(x, logc, 3, 1, -1.0, ok, 0.5, 0.1),                                             # t_min > t_max
        lambda: call(x, logc, 3, 1, -1.0, dict(ok, rate_const=0.0), 0.01, 1.0),
        lambda: call(x, logc, 3, 1, -1.0, dict(ok, time_exp=1.0), 0.01, 1.0),
        lambda: call(x, logc, 3, 1, -1.0, dict(ok, time_base=0.0), 0.01, 1.0),
        lambda: call(x, logc, 3, 1, -1.0, dict(t_func="loglinear", alpha_eps=1.0), 0.01, 1.0),
        lambda: call(x, logc, 3, 1, -1.0, dict(t_func="linear"), 0.01, 1.0),
        lambda: call(x, logc.float(), 3, 1, -1.0, ok, 0.01, 1.0),                                    # dtypes, shapes
        lambda: call(x.long(), logc, 3, 1, -1.0, ok, 0.01, 1.0),
        lambda: call(x, logc[:1].contiguous(), 3, 1, -1.0, ok, 0.01, 1.0),
        lambda: call(x, logc, 3, 1, -1.0, ok, 0.01, 1.0, counts=torch.zeros(3, dtype=torch.int32, device=DEV)),
        lambda: call(x, logc, 3, 1, -1.0, ok, 0.01, 1.0, t_eval=torch.zeros(2, dtype=torch.float64, device=DEV)),
    ]
    for i, c in enumerate(bad_calls):
        with pytest.raises(E):
            c()
            pytest.fail(f"bad call {i} went through")
    counts, t_eval, out = call(x, logc, 3, 1, -math.inf, ok, 0.01, 1.0)
    assert counts.cpu().tolist() == [1, 1] and bool((out < 0).all()) and bool(((t_eval >= 0.01) & (t_eval <= 1.0)).all())


# ------------------------------------------------------------------------------------------------ hit_step
def _check_step(logits, x, m, counts, seed, offset):
    """One set of counts on one (logits, x): out of place, in place, under the argmax flag, and with NaN at every unselected row."""
    N, D, S = logits.shape
    lg, xd, cd = logits.to(DEV), _dev(x, torch.int32), _dev(counts, torch.int32)
    sel = hc.hit_select_replay(x, m, counts, seed, offset)
    chosen = np.zeros((N, D), dtype=bool)
    for n in range(N):
        chosen[n, sel[n]] = True
    total = int(chosen.sum())
    plain = native.absorb_step(lg, xd, m, 1.0, 0, seed, offset).cpu().numpy()
    changed = torch.full((1,), 7, dtype=torch.int32, device=DEV)
    before = native.LAUNCH_COUNTS.get("ctdd_absorb_hit_step", 0)
    out = native.absorb_hit_step(lg, xd, cd, m, 0, seed, offset, changed=changed)
    assert native.LAUNCH_COUNTS["ctdd_absorb_hit_step"] == before + 1
    got = out.cpu().numpy()
    assert ((got != x) == chosen).all(), "the set of changed rows differs from the selection replay"
    assert (got[chosen] == plain[chosen]).all(), "a selected row's state differs from ctdd_absorb_step at p = 1"
    assert (got[chosen] != m).all() and (got[~chosen] == x[~chosen]).all()
    assert int(changed.cpu()) == 7 + total
    assert bool((xd.cpu() == torch.from_numpy(x)).all()), "the out-of-place call wrote into x"
    pick, margin = hc.picks(logits.numpy(), m, seed, offset)
    sure = chosen.reshape(-1) & (margin > 1e-5)
    assert (got.reshape(-1)[sure] == pick[sure]).all(), "a selected row's state differs from the replay's pick"
    # in place
    xi = xd.clone()
    same = native.absorb_hit_step(lg, xi, cd, m, 0, seed, offset, out=xi, changed=changed)
    assert same.data_ptr() == xi.data_ptr() and bool((xi == out).all()) and int(changed.cpu()) == 7 + 2 * total
    # the argmax flag: the same rows, the fp64 argmax (exact on fp32 inputs, lowest index on ties)
    best, _ = ac.argmax_f64(logits.numpy(), m)
    greedy = native.absorb_hit_step(lg, xd, cd, m, ARGMAX, seed, offset).cpu().numpy()
    assert ((greedy != x) == chosen).all() and (greedy.reshape(-1)[chosen.reshape(-1)] == best[chosen.reshape(-1)]).all()
    assert (greedy == native.absorb_step(lg, xd, m, 1.0, ARGMAX, seed, offset).cpu().numpy())[chosen].all()
    # NaN logits at every unselected row change nothing: those rows are not read
    poisoned = logits.clone()
    poisoned[torch.from_numpy(~chosen)] = float("nan")
    for flags, want in ((0, got), (ARGMAX, greedy)):
        again = native.absorb_hit_step(poisoned.to(DEV), xd, cd, m, flags, seed, offset).cpu().numpy()
        assert (again == want).all(), "an unselected row's logits were read"
    return total


@pytest.mark.parametrize("mode", ("mix", "all"))
@pytest.mark.parametrize("case", ac.CASES, ids=ac.IDS)
def test_hit_step_selection_and_states(case, mode):
    S, m, B, D = case
    logits, _, _ = ac.inputs(case)
    x = ac.x_t_of(case, mode).to(torch.int32).numpy()
    M = (x == m).sum(1)
    moved = 0
    for c in range(-(-6 // B)):                                          # every count option at some sample
        counts = np.array([hc.count_options(int(M[n]))[(B * c + n) % 6] for n in range(B)], dtype=np.int32)
        moved += _check_step(logits, x, m, counts, 0xAB5000 + S, c)
    assert moved > 0
    # no sample has an event: one launch, nothing moves, the copy is made
    zero = torch.zeros(B, dtype=torch.int32, device=DEV)
    xd = _dev(x, torch.int32)
    out = native.absorb_hit_step(logits.to(DEV), xd, zero, m, 0, 1, 0)
    assert out.data_ptr() != xd.data_ptr() and bool((out == xd).all())


def test_hit_step_long_sample():
    """N = 1, D = 70001 (274 chunks of 256 rows, the last one partial), S = 5: every count option."""
    S, m, D = 5, 2, 70001
    g = torch.Generator().manual_seed(70001)
    logits = (2.0 * torch.randn(1, D, S, generator=g)).contiguous()
    x = torch.where(torch.rand(1, D, generator=g) < 0.5, torch.full((), m), torch.zeros((), dtype=torch.long)).to(torch.int32).numpy()
    M = int((x == m).sum())
    for offset, k in enumerate(hc.count_options(M)):
        assert _check_step(logits, x, m, np.array([k], dtype=np.int32), 0x70001, offset) == hc.clamp_count(k, M)


def test_hit_step_argument_errors():
    lg = torch.zeros(2, 3, 4, device=DEV)
    x = torch.full((2, 3), 3, dtype=torch.int32, device=DEV)
    counts = torch.ones(2, dtype=torch.int32, device=DEV)
    step, E = native.absorb_hit_step, native.CtddError
    bad_calls = [
        lambda: step(lg, x[:, :2].contiguous(), counts, 3),                                          # shapes
        lambda: step(lg, x, counts[:1].contiguous(), 3),
        lambda: step(lg, x, counts, 3, out=x[:1].contiguous()),
        lambda: step(lg, x, None, 3),
        lambda: step(lg, x.long(), counts, 3),                                                       # dtypes
        lambda: step(lg.double(), x, counts, 3),
        lambda: step(lg, x, counts.long(), 3),
        lambda: step(lg, x, counts, 4),                                                              # mask_state outside [0, S)
        lambda: step(lg, x, counts, -1),
        lambda: step(torch.zeros(1, 2, native.ABSORB_MAX_S + 1, device=DEV), x[:1, :2].contiguous(), counts[:1].contiguous(), 3),
        lambda: step(lg, x, counts, 3, flags=2),                                                     # unknown flags
    ]
    for i, c in enumerate(bad_calls):
        with pytest.raises(E):
            c()
            pytest.fail(f"bad call {i} went through")
    out = step(lg, x, counts, 3)
    assert bool(((out != 3).sum(1) == 1).all())


# ------------------------------------------------------------------------------------------------ the sampler
class _TimeOnlyModel:
    """Logits that depend on the time (and the dimension) only: toy_logits at x = 0."""

    def __init__(self, S, m):
        self.S, self.device = S, DEV
        self.process = process.DeviceForwardProcess("absorbing", S, DEV, rate_const=1.0, t_func="loglinear", alpha_eps=1e-3, mask_state=m)

    def __call__(self, x, t):
        return toy_logits(torch.zeros_like(x), t, self.S, scale=3.0)


S_, M_, N_, D_ = 5, 2, 64, 50
MIN_T, MAX_T = 0.01, 1.0
SEED = 20250117
LAUNCHES = ("ctdd_absorb_hit_time", "ctdd_absorb_hit_step", "ctdd_absorb_step")


def _sampler(num_steps, **kw):
    import lib.sampling.sampling  # noqa: F401
    import lib.sampling.sampling_utils as su
    from ctdd.config_dict import ConfigDict
    cfg = ConfigDict()
    for sec in ("data", "model", "sampler", "training", "loss"):
        cfg[sec] = ConfigDict()
    cfg.data.S, cfg.model.concat_dim, cfg.training.max_t = S_, D_, MAX_T
    cfg.sampler.update(name="AbsorbingFirstHit", num_steps=num_steps, min_t=MIN_T)
    cfg.sampler.update(**kw)
    sampler = su.get_sampler(cfg)
    sampler.seed = SEED
    return sampler


def _launches():
    return [native.LAUNCH_COUNTS.get(k, 0) for k in LAUNCHES]


def test_exact_sampler_one_event_per_forward():
    model, sampler = _TimeOnlyModel(S_, M_), _sampler(D_)
    before = _launches()
    x, changed = sampler.sample(model, N_)
    assert [a - b for a, b in zip(_launches(), before)] == [D_, D_, 1], "two launches per iteration and the closing step"
    times = sampler.times
    assert x.shape == (N_, D_) and len(changed) == D_ and times.shape == (D_, N_) and times.dtype == np.float32
    assert (x != M_).all() and ((x >= 0) & (x < S_)).all(), "an entry is masked after the closing step"
    assert all(0.0 <= c <= 1.0 for c in changed), "an iteration changed more than one entry per sample"
    assert (np.diff(times, axis=0) <= 0).all() and (times >= np.float32(MIN_T)).all() and (times <= np.float32(MAX_T)).all()
    # an iteration without an event reports min_t; the others unmask one entry at their time.  Every entry's masking level is uniform
    # on (0, c(max_t)): the share of the N D entries unmasked at a time above t* is Binomial(N D, q) / (N D),
    # q = 1 - (1 - alpha(t*)) / (1 - alpha(max_t)); the entries left to the closing step were unmasked below min_t < t*
    pr = hc.proc()
    events = times[times > np.float32(MIN_T)]
    print(f"{events.size} of {N_ * D_} entries unmasked by an event; per-iteration changed sums to {sum(changed) * N_:.0f}")
    assert round(sum(changed) * N_) == events.size                      # (an accepted event lies at or above the level of min_t)
    for t_star in (0.25, 0.5, 0.75):
        q = 1 - float((1 - pr.alpha(torch.tensor(t_star, dtype=torch.float64))) / (1 - pr.alpha(torch.tensor(MAX_T, dtype=torch.float64))))
        share, bar = float((times > np.float32(t_star)).sum()) / (N_ * D_), 4 * math.sqrt(q * (1 - q) / (N_ * D_))
        print(f"share of entries unmasked above t = {t_star}: {share:.4f}, law {q:.4f}, bar {bar:.4f}")
        assert abs(share - q) <= bar
    # a fixed seed fixes the sample
    again, changed_again = sampler.sample(model, N_)
    assert (again == x).all() and changed_again == changed and sampler.times.tobytes() == times.tobytes()


def test_fewer_forwards_take_k_events_each():
    model, sampler = _TimeOnlyModel(S_, M_), _sampler(8, candidate="argmax")
    assert sampler.plan(D_) == (7, 8)
    before = _launches()
    x, changed = sampler.sample(model, N_)
    assert [a - b for a, b in zip(_launches(), before)] == [8, 8, 1]
    assert len(changed) == 8 and sampler.times.shape == (8, N_) and all(0.0 <= c <= 7.0 for c in changed)
    assert (x != M_).all() and ((x >= 0) & (x < S_)).all() and (np.diff(sampler.times, axis=0) <= 0).all()


def test_inpaint_follows_the_largest_masked_count():
    model, sampler = _TimeOnlyModel(S_, M_), _sampler(D_)
    N = 6
    g = torch.Generator().manual_seed(3)
    x_known = torch.randint(0, S_ - 1, (N, D_), generator=g)
    x_known = x_known + (x_known >= M_).long()                           # skips the mask state
    free = [1, 3, 10, 17, 4, 2]                                          # sample 0: everything held but one entry
    held = torch.ones(N, D_, dtype=torch.bool)
    for n, f in enumerate(free):
        held[n, torch.randperm(D_, generator=g)[:f]] = False
    before = _launches()
    out = sampler.inpaint(model, x_known, held)
    assert [a - b for a, b in zip(_launches(), before)] == [17, 17, 1], "the iterations follow the largest masked count"
    hn = held.numpy()
    assert out.shape == (N, D_) and (out[hn] == x_known.numpy()[hn]).all(), "a held entry moved"
    assert (out != M_).all() and ((out >= 0) & (out < S_)).all()
    times = sampler.times
    assert times.shape == (17, N)
    for n, f in enumerate(free):                                         # a sample that has finished takes no further event
        assert (times[f:, n] == np.float32(MIN_T)).all() and (np.diff(times[:, n]) <= 0).all()
    assert (times[:1] > np.float32(MIN_T)).any()
    again = sampler.inpaint(model, x_known, held)
    assert (again == out).all()
    before = _launches()
    same = sampler.inpaint(model, x_known, torch.ones(D_, dtype=torch.bool))
    assert (same == x_known.numpy()).all() and _launches() == before
