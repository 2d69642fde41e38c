"""GPU: confidence-ordered unmasking on ctdd_absorb_propose / ctdd_absorb_commit (csrc/absorb.hip) -- the commit against its CPU
replay bit for bit over score patterns that load each radix pass, the proposal's candidates against the step's replay and the step
kernel itself, its scores against fp64 (bar: 8 times the error of the fp32 numpy evaluation, floor 1e-6 max(1, |score|)), the pair
end to end, the AbsorbingConfidence sampler's counts, and the refusals."""
import numpy as np
import pytest
import torch

import absorb_cases as ac
import absorb_conf_cases as cc
from ctdd import native, process
from oracle.toy_model import toy_logits

pytestmark = pytest.mark.gpu

DEV = "cuda"
M_STATE = 5                                                              # the commit tests' mask state (the kernel never sees S)


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(DEV)


# ------------------------------------------------------------------------------------------------ the commit
SHAPES = ((3, 1), (2, 5), (3, 64), (2, 65), (3, 257), (2, 1500))        # D around the wave (64) and the chunk (256), several chunks
PATTERNS = ("normal", "last_digit", "pow2", "few", "equal", "special")
P_VALUES = (0.0, 0.25, 0.3, 0.5, 1.0)
COUNT_MODES = (lambda M: 0, lambda M: 1, lambda M: M - 1, lambda M: M, lambda M: M + 3, lambda M: -2)


def _scores(pattern, N, D, rng):
    n = N * D
    if pattern == "normal":
        s = rng.standard_normal(n)
    elif pattern == "last_digit":                                        # 1 + i 2^-23: the keys differ in their last byte(s) only
        s = 1.0 + rng.permutation(n) * 2.0 ** -23
    elif pattern == "pow2":                                              # +-2^e: the first pass decides, signs crossed
        s = np.where(rng.random(n) < 0.5, -1.0, 1.0) * 2.0 ** rng.integers(-126, 128, n)
    elif pattern == "few":
        s = np.array([-1.0, -0.0, 0.0, 2.0])[rng.integers(0, 4, n)]
    elif pattern == "equal":
        s = np.full(n, 0.37)
    else:
        s = rng.standard_normal(n)
        kind = rng.integers(0, 10, n)
        s[kind == 0], s[kind == 1], s[kind == 2] = -np.inf, np.inf, np.nan
    return s.astype(np.float32).reshape(N, D)


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("N,D", SHAPES)
def test_commit_matches_the_replay_exactly(N, D, pattern):
    rng = np.random.default_rng(100 * D + PATTERNS.index(pattern))
    score = _scores(pattern, N, D, rng)
    cand = rng.integers(0, M_STATE, (N, D)).astype(np.int32)
    launches = 0
    for shift in range(3):                                               # sample n is masked with share (0, 0.5, 1)[(n + shift) % 3]
        share = np.array([0.0, 0.5, 1.0])[(np.arange(N) + shift) % 3][:, None]
        masked = rng.random((N, D)) < share
        x = np.where(masked, M_STATE, rng.integers(0, M_STATE, (N, D))).astype(np.int32)
        # poison where the kernel must not look: NaN scores and out-of-range candidates at the unmasked rows
        c_in = np.where(masked, cand, np.where(rng.random((N, D)) < 0.5, 2 ** 31 - 1, -7)).astype(np.int32)
        s_in = np.where(masked, score, np.float32(np.nan)).astype(np.float32)
        M = masked.sum(1)
        xd, cd, sd = _dev(x, torch.int32), _dev(c_in, torch.int32), _dev(s_in, torch.float32)
        modes = [dict(p=p) for p in P_VALUES] + [dict(counts=np.array([f(int(v)) for v in M], dtype=np.int32)) for f in COUNT_MODES]
        for mode in modes:
            changed = torch.full((1,), 7, dtype=torch.int32, device=DEV)
            kw = dict(p_unmask=mode["p"]) if "p" in mode else dict(counts=_dev(mode["counts"], torch.int32))
            out = native.absorb_commit(xd, cd, sd, M_STATE, changed=changed, **kw).cpu().numpy()
            want, k = cc.commit_replay(x, c_in, s_in, M_STATE, **mode)
            assert (out == want).all(), f"shift {shift} {mode}: {(out != want).sum()} entries differ from the replay"
            assert int(changed.cpu()) == 7 + k, f"shift {shift} {mode}"
            assert (out[~masked] == x[~masked]).all()
            launches += 1
    print(f"commit ({N}, {D}) {pattern}: {launches} launches equal the replay")


@pytest.mark.parametrize("pattern", ["normal", "few"])
def test_commit_on_a_sample_longer_than_65536(pattern):
    """No cap on D below 65 536: one sample of 70 001 rows (274 chunks of the last pass, mass ties across them with "few")."""
    N, D = 1, 70001
    rng = np.random.default_rng(7)
    score = _scores(pattern, N, D, rng)
    cand = rng.integers(0, M_STATE, (N, D)).astype(np.int32)
    x = np.where(rng.random((N, D)) < 0.6, M_STATE, rng.integers(0, M_STATE, (N, D))).astype(np.int32)
    xd, cd, sd = _dev(x, torch.int32), _dev(cand, torch.int32), _dev(score, torch.float32)
    M = int((x == M_STATE).sum())
    for mode in (dict(p=0.3), dict(counts=np.array([M - 1], dtype=np.int32)), dict(counts=np.array([17], dtype=np.int32))):
        changed = torch.zeros(1, dtype=torch.int32, device=DEV)
        kw = dict(p_unmask=mode["p"]) if "p" in mode else dict(counts=_dev(mode["counts"], torch.int32))
        out = native.absorb_commit(xd, cd, sd, M_STATE, changed=changed, **kw).cpu().numpy()
        want, k = cc.commit_replay(x, cand, score, M_STATE, **mode)
        assert (out == want).all() and int(changed.cpu()) == k


# ------------------------------------------------------------------------------------------------ the proposal
MASKS = ("mix", "all")


def _case(case, mask):
    S, m, B, D = case
    logits, _, _ = ac.inputs(case)
    x = ac.x_t_of(case, mask).to(torch.int32)
    masked = x.numpy().reshape(-1) == m
    return logits, x, masked, logits.to(DEV), x.to(DEV)


@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("case", ac.CASES, ids=ac.IDS)
def test_propose_candidates_match_the_replay_and_the_step(case, mask):
    """Draw mode: the candidates are step_replay's picks wherever the pick's margin is at least 1e-5, and ctdd_absorb_step's own
    states (p = 1, same seed and offset) everywhere; over at least 1000 picks the share left out stays under the step's bars (2 %,
    5 % at S = 1024).  Argmax mode: the fp64 argmax with the lowest index on ties -- exactly, since comparing fp32 logits rounds
    nothing."""
    S, m, B, D = case
    logits, x, masked, lg, xd = _case(case, mask)
    rows = int(masked.sum())
    seed, compared, left_out = 0xC0FFEE00 + S, 0, 0
    poison = np.int32(-123)
    for offset in range(-(-1000 // rows)):
        cand, score = native.absorb_propose(lg, xd, m, 0.0, 0, seed, offset)
        step = native.absorb_step(lg, xd, m, 1.0, 0, seed, offset).cpu().numpy().reshape(-1)
        cand = cand.cpu().numpy().reshape(-1)
        pick, margin, _ = cc.propose_picks(logits.numpy(), m, seed, offset)
        assert (cand[masked] == step[masked]).all(), "the candidate is not the state the step kernel draws"
        assert ((cand[masked] >= 0) & (cand[masked] < S) & (cand[masked] != m)).all()
        decided = masked & (margin >= 1e-5)
        assert (cand[decided] == pick[decided]).all(), "candidate differs from categorical_icdf"
        compared += rows
        left_out += int((masked & ~decided).sum())
    print(f"S={S} {mask}: {left_out} of {compared} candidates left out (margin < 1e-5)")
    assert compared >= 1000 and left_out / compared <= (0.05 if S == 1024 else 0.02)
    # nothing is written for a row that is not masked
    cand = torch.full((B, D), int(poison), dtype=torch.int32, device=DEV)
    score = torch.full((B, D), -777.0, device=DEV)
    native._check(native.load().ctdd_absorb_propose(lg.data_ptr(), xd.data_ptr(), B, D, S, m, 0.0, native.ABSORB_ARGMAX, seed, 0,
                                                    cand.data_ptr(), score.data_ptr(), native._stream()), "ctdd_absorb_propose")
    cand, score = cand.cpu().numpy().reshape(-1), score.cpu().numpy().reshape(-1)
    assert (cand[~masked] == poison).all() and (score[~masked] == -777.0).all()
    best, _ = ac.argmax_f64(logits.numpy(), m)
    assert (cand[masked] == best[masked]).all(), "argmax mode differs from the fp64 argmax"
    step = native.absorb_step(lg, xd, m, 0.0, native.ABSORB_ARGMAX, seed, 0).cpu().numpy().reshape(-1)
    assert (cand[masked] == step[masked]).all()


@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("case", ac.CASES, ids=ac.IDS)
def test_propose_scores_against_fp64(case, mask):
    """Every masked row's score at the device's own candidate against the fp64 evaluation (Gumbel from the exact fp32 u2): within
    max(8 E32, 1e-6 max(1, |score|)), E32 the largest error of the same formula in fp32 numpy over the rows of the call."""
    S, m, B, D = case
    logits, x, masked, lg, xd = _case(case, mask)
    rows = np.nonzero(masked)[0]
    seed = 0xBEEF0000 + S
    for flags in (0, native.ABSORB_ARGMAX):
        for offset, noise in enumerate((0.0, 0.7)):
            cand, score = native.absorb_propose(lg, xd, m, noise, flags, seed, offset)
            cand, score = cand.cpu().numpy().reshape(-1)[rows], score.cpu().numpy().reshape(-1)[rows]
            u2 = cc.propose_picks(logits.numpy(), m, seed, offset)[2][rows]
            s64 = cc.propose_scores(logits.numpy(), m, rows, cand, noise, u2, np.float64)
            s32 = cc.propose_scores(logits.numpy(), m, rows, cand, noise, u2, np.float32)
            err, e32 = np.abs(score.astype(np.float64) - s64), float(np.abs(s32.astype(np.float64) - s64).max())
            bar = np.maximum(8 * e32, 1e-6 * np.maximum(1.0, np.abs(s64)))
            print(f"S={S} {mask} flags={flags} noise={noise}: score error kernel {err.max():.2e} / fp32 {e32:.2e}; "
                  f"worst error / bar {float((err / bar).max()):.3f}; scores in [{s64.min():.2f}, {s64.max():.2f}]")
            assert np.isfinite(score).all()
            assert (err <= bar).all()
            if noise == 0.0:
                assert (score <= 0).all(), "a log-probability above 0"


@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("case", ac.CASES, ids=ac.IDS)
def test_propose_then_commit_matches_the_replay(case, mask):
    S, m, B, D = case
    logits, x, masked, lg, xd = _case(case, mask)
    cand, score = native.absorb_propose(lg, xd, m, 0.7, 0, 0xFACE + S, 2)
    ch, sh = cand.cpu().numpy(), score.cpu().numpy()
    M = (x.numpy() == m).sum(1)
    for mode in (dict(p=0.3), dict(p=1.0), dict(counts=(M // 2).astype(np.int32))):
        changed = torch.zeros(1, dtype=torch.int32, device=DEV)
        kw = dict(p_unmask=mode["p"]) if "p" in mode else dict(counts=_dev(mode["counts"], torch.int32))
        out = native.absorb_commit(xd, cand, score, m, changed=changed, **kw).cpu().numpy()
        want, k = cc.commit_replay(x.numpy(), ch, sh, m, **mode)
        assert (out == want).all() and int(changed.cpu()) == k
        assert int((out != x.numpy()).sum()) == k                        # exactly k rows left the mask state


# ------------------------------------------------------------------------------------------------ the sampler
class _TimeOnlyModel:
    """Logits that depend on the time (and the dimension) only: toy_logits at x = 0."""

    def __init__(self, S, m):
        self.S, self.device = S, DEV
        self.process = process.DeviceForwardProcess("absorbing", S, DEV, rate_const=1.0, t_func="loglinear", alpha_eps=1e-3, mask_state=m)

    def __call__(self, x, t):
        return toy_logits(torch.zeros_like(x), t, self.S, scale=3.0)


S_, M_, N_, D_, K_ = 6, 2, 16, 30, 6


def _sampler(**kw):
    import lib.sampling.sampling  # noqa: F401
    import lib.sampling.sampling_utils as su
    from ctdd.config_dict import ConfigDict
    cfg = ConfigDict()
    for sec in ("data", "model", "sampler", "training", "loss"):
        cfg[sec] = ConfigDict()
    cfg.data.S, cfg.model.concat_dim, cfg.training.max_t = S_, D_, 1.0
    cfg.sampler.update(name="AbsorbingConfidence", rule="ancestral", num_steps=K_, min_t=0.01)
    cfg.sampler.update(**kw)
    sampler = su.get_sampler(cfg)
    sampler.seed = 20240611
    return sampler


def _step_probs(model):
    """The sampler's host-side fp64 p of every step, restated."""
    ts = torch.from_numpy(np.concatenate((np.linspace(1.0, 0.01, K_), [0.0])))
    return torch.clamp(model.process.unmask_prob(ts[:-1], ts[:-1] - ts[1:], "ancestral"), 0.0, 1.0).tolist()


def _launches():
    return [native.LAUNCH_COUNTS.get(k, 0) for k in ("ctdd_absorb_propose", "ctdd_absorb_commit", "ctdd_absorb_step")]


def test_sampler_commits_the_scheduled_counts():
    model, sampler = _TimeOnlyModel(S_, M_), _sampler()
    before = _launches()
    x, changed = sampler.sample(model, N_)
    assert [a - b for a, b in zip(_launches(), before)] == [K_, K_, 1]
    assert x.shape == (N_, D_) and len(changed) == K_ and (x != M_).all() and ((x >= 0) & (x < S_)).all()
    M = D_
    for i, p in enumerate(_step_probs(model)):
        k = cc.count_rule(p, M)
        print(f"step {i}: p {p:.4f}, {M} masked a sample, {k} committed; counter {changed[i] * N_}")
        assert changed[i] * N_ == N_ * k
        M -= k
    assert M == 0                                                        # the last step's p is 1
    again, changed_again = sampler.sample(model, N_)
    assert (again == x).all() and changed_again == changed, "a fixed seed does not fix the sample"
    assert not all((x[n] == x[0]).all() for n in range(1, N_)), "sixteen drawn samples are identical"


def test_greedy_sampler_is_deterministic_across_samples():
    model, sampler = _TimeOnlyModel(S_, M_), _sampler(conf_temp=0.0, candidate="argmax")
    x, _ = sampler.sample(model, N_)
    assert (x != M_).all() and all((x[n] == x[0]).all() for n in range(1, N_))


def test_inpaint_counts_follow_each_samples_own_masked_rows():
    model, sampler = _TimeOnlyModel(S_, M_), _sampler()
    g = torch.Generator().manual_seed(3)
    x_known = torch.randint(0, S_ - 1, (N_, D_), generator=g)
    x_known = x_known + (x_known >= M_).long()                           # skips the mask state
    held = torch.rand(N_, D_, generator=g) < 0.4
    out = sampler.inpaint(model, x_known, held)
    hn = held.numpy()
    assert out.shape == (N_, D_) and (out[hn] == x_known.numpy()[hn]).all()
    assert (out != M_).all() and ((out >= 0) & (out < S_)).all()
    # the same run through the loop itself, for its per-step counters
    x0 = torch.where(held, x_known, torch.full((), M_, dtype=torch.int64)).to(torch.int32).to(DEV).contiguous()
    x, changed = sampler._loop(model, x0)
    assert (x == out).all()
    M = (~hn).sum(1)
    assert len(set(M.tolist())) > 1, "every sample has the same number of free entries: the case shows nothing"
    for i, p in enumerate(_step_probs(model)):
        k = np.array([cc.count_rule(p, int(v)) for v in M])
        assert round(changed[i] * N_) == int(k.sum()), f"step {i}"
        M = M - k
    assert (M == 0).all()
    before = _launches()
    same = sampler.inpaint(model, x_known, torch.ones(D_, dtype=torch.bool))
    assert (same == x_known.numpy()).all() and _launches() == before


# ------------------------------------------------------------------------------------------------ misuse
def test_argument_errors():
    lg = torch.zeros(2, 3, 4, device=DEV)
    x = torch.full((2, 3), 3, dtype=torch.int32, device=DEV)
    score, counts = torch.zeros(2, 3, device=DEV), torch.ones(2, dtype=torch.int32, device=DEV)
    E = native.CtddError
    with pytest.raises(E):
        native.absorb_commit(x, x, score, 3)                                           # neither p_unmask nor counts
    with pytest.raises(E):
        native.absorb_commit(x, x, score, 3, p_unmask=0.5, counts=counts)              # both
    with pytest.raises(E, match="p_unmask"):
        native.absorb_commit(x, x, score, 3, p_unmask=1.5)
    with pytest.raises(E, match="p_unmask"):
        native.absorb_commit(x, x, score, 3, p_unmask=-0.1)
    with pytest.raises(E):
        native.absorb_commit(x, x[:, :2].contiguous(), score, 3, p_unmask=0.5)
    with pytest.raises(E):
        native.absorb_commit(x, x, score[:1].contiguous(), 3, p_unmask=0.5)
    with pytest.raises(E):
        native.absorb_commit(x, x, score, 3, counts=counts[:1].contiguous())
    with pytest.raises(E):
        native.absorb_commit(x, x, score, 3, p_unmask=0.5, out=x)                      # out aliases x
    with pytest.raises(E):
        native.absorb_commit(x, x, score.double(), 3, p_unmask=0.5)
    with pytest.raises(E):
        native.absorb_commit(x.cpu(), x.cpu(), score.cpu(), 3, p_unmask=0.5)
    with pytest.raises(E):
        native.absorb_propose(lg, x[:, :2].contiguous(), 3)
    with pytest.raises(E):
        native.absorb_propose(lg, x, 4)                                                # mask_state outside [0, S)
    with pytest.raises(E):
        native.absorb_propose(lg, x, 3, flags=2)
    with pytest.raises(E):
        native.absorb_propose(lg, x, 3, noise=float("nan"))
    with pytest.raises(E):
        native.absorb_propose(lg.cpu(), x.cpu(), 3)
    # and the well-formed calls go through
    cand, score = native.absorb_propose(lg, x, 3)
    assert (native.absorb_commit(x, cand, score, 3, p_unmask=1.0) != 3).all()
