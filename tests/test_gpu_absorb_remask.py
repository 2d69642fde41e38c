"""GPU: remasking on ctdd_absorb_remask_step / ctdd_absorb_remask_norm (csrc/absorb.hip) -- the step against ctdd_absorb_step itself
(sigma = 0: bit for bit; masked rows at any sigma), its remask decisions against the CPU replay of Philox component 3, held rows, the
confidence record against fp64 (bar: 8 times the error of the fp32 numpy evaluation, floor 1e-6), the per-sample normaliser, the
confidence-weighted step, the in-place call, the refusals, and the AbsorbingRemask sampler's statistics against its schedule."""
import numpy as np
import pytest
import torch

import absorb_cases as ac
import absorb_remask_cases as rc
from ctdd import native, process
from oracle.toy_model import toy_logits

pytestmark = pytest.mark.gpu

DEV = "cuda"
CONF = native.ABSORB_REMASK_CONF


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(DEV)


def _case(case, mode):
    S, m, B, D = case
    logits, _, _ = ac.inputs(case)
    x = ac.x_t_of(case, mode).to(torch.int32)
    return logits, x.numpy(), logits.to(DEV), x.to(DEV)


def _counts():
    return torch.zeros(2, dtype=torch.int32, device=DEV)


# ------------------------------------------------------------------------------------------------ sigma = 0: the plain step
@pytest.mark.parametrize("mode", ac.MODES)
@pytest.mark.parametrize("case", ac.CASES, ids=ac.IDS)
def test_sigma_zero_is_the_plain_step(case, mode):
    S, m, B, D = case
    _, x, lg, xd = _case(case, mode)
    seed = rc.step_seed(S)
    for offset, p in enumerate(rc.P_VALUES):
        changed, counts = torch.zeros(1, dtype=torch.int32, device=DEV), _counts()
        want = native.absorb_step(lg, xd, m, p, 0, seed, offset, changed=changed)
        before = native.LAUNCH_COUNTS.get("ctdd_absorb_remask_step", 0)
        out, conf = native.absorb_remask_step(lg, xd, m, p, 0.0, seed=seed, offset=offset, counts=counts)
        assert native.LAUNCH_COUNTS["ctdd_absorb_remask_step"] == before + 1 and conf is None
        assert bool((out == want).all()), f"p = {p}: {int((out != want).sum())} entries differ from ctdd_absorb_step"
        assert counts.cpu().tolist() == [int(changed.cpu()), 0]


# ------------------------------------------------------------------------------------------------ remask coin, held rows
@pytest.mark.parametrize("mode", ac.MODES)
@pytest.mark.parametrize("case", ac.CASES, ids=ac.IDS)
def test_remask_decisions_and_held_rows(case, mode):
    S, m, B, D = case
    _, x, lg, xd = _case(case, mode)
    held = rc.held_pattern(case)
    hd, seed = _dev(held, torch.bool), rc.step_seed(S)
    xf, hf = x.reshape(-1), held.reshape(-1)
    masked_free = (xf == m) & ~hf
    for offset, p in enumerate(rc.P_VALUES):
        plain = native.absorb_step(lg, xd, m, p, 0, seed, offset).cpu().numpy().reshape(-1)
        counts = _counts()
        out = native.absorb_remask_step(lg, xd, m, p, rc.SIGMA, held=hd, seed=seed, offset=offset, counts=counts)[0].cpu().numpy().reshape(-1)
        remask, sg, u3, free = rc.remask_replay(x, held, m, rc.SIGMA, seed, offset)
        assert (out[masked_free] == plain[masked_free]).all(), "a masked free row differs from ctdd_absorb_step"
        assert (out[hf] == xf[hf]).all(), "a held row moved"
        near = free & (np.abs(u3.astype(np.float64) - float(np.float32(rc.SIGMA))) < 1e-6)
        print(f"S={S} {mode} p={p}: {int(free.sum())} free unmasked rows, {int(near.sum())} left out (|u3 - sigma| < 1e-6), "
              f"{int((free & (out == m)).sum())} remasked")
        assert near.sum() <= 0.01 * free.sum()
        sure = free & ~near
        assert ((out[sure] == m) == remask[sure]).all(), "remask decision differs from the replay"
        kept = free & (out != m)
        assert (out[kept] == xf[kept]).all(), "a kept row was not copied"
        assert counts.cpu().tolist() == [int((masked_free & (out != m)).sum()), int((free & (out == m)).sum())]
    # sigma = 1: every free unmasked row returns to the mask state; p = 0, sigma = 0: nothing moves
    counts = _counts()
    out = native.absorb_remask_step(lg, xd, m, 0.0, 1.0, held=hd, seed=seed, offset=7, counts=counts)[0].cpu().numpy().reshape(-1)
    free = (xf != m) & ~hf
    assert (out[free] == m).all() and (out[~free] == xf[~free]).all() and counts.cpu().tolist() == [0, int(free.sum())]
    counts = _counts()
    out = native.absorb_remask_step(lg, xd, m, 0.0, 0.0, held=hd, seed=seed, offset=8, counts=counts)[0].cpu().numpy().reshape(-1)
    assert (out == xf).all() and counts.cpu().tolist() == [0, 0]


# ------------------------------------------------------------------------------------------------ the confidence record
@pytest.mark.parametrize("mode", ac.MODES)
@pytest.mark.parametrize("case", ac.CASES, ids=ac.IDS)
def test_conf_out(case, mode):
    """conf_out of the newly unmasked rows against the fp64 probability of the state written, within max(8 E32, 1e-6), E32 the
    largest error of the same formula in fp32 numpy over the call; exact 0 on rows left masked or remasked; conf_in's bits on kept
    and held rows (a -0.0 and a NaN payload among them)."""
    S, m, B, D = case
    logits, x, lg, xd = _case(case, mode)
    held = rc.held_pattern(case)
    conf = rc.conf_pattern(case)
    cf = conf.reshape(-1).view(np.uint32).copy()
    cf[-1] = 0x80000000                                                  # -0.0 on the last row (held) ...
    cf[np.nonzero(held.reshape(-1))[0][0]] = 0x7FC00123                  # ... and a NaN payload on the first held row
    conf = cf.view(np.float32).reshape(B, D)
    hd, cd, seed = _dev(held, torch.bool), _dev(conf, torch.float32), rc.step_seed(S)
    xf, hf = x.reshape(-1), held.reshape(-1)
    masked_free, free = (xf == m) & ~hf, (xf != m) & ~hf
    out, co = native.absorb_remask_step(lg, xd, m, 0.6, rc.SIGMA, held=hd, conf=cd, seed=seed, offset=3)
    same = native.absorb_remask_step(lg, xd, m, 0.6, rc.SIGMA, held=hd, seed=seed, offset=3)[0]
    assert bool((out == same).all()), "the states depend on whether the confidence is recorded"
    out, co = out.cpu().numpy().reshape(-1), co.cpu().numpy().reshape(-1)
    rows = np.nonzero(masked_free & (out != m))[0]
    if rows.size:
        p64 = rc.state_probability(logits.numpy(), m, rows, out[rows], np.float64)
        p32 = rc.state_probability(logits.numpy(), m, rows, out[rows], np.float32)
        err, e32 = np.abs(co[rows].astype(np.float64) - p64), float(np.abs(p32.astype(np.float64) - p64).max())
        print(f"S={S} {mode}: {rows.size} rows unmasked; conf error kernel {err.max():.2e} / fp32 {e32:.2e}; conf in [{p64.min():.2e}, {p64.max():.2e}]")
        assert (err <= max(8 * e32, 1e-6)).all()
        assert ((co[rows] > 0) | (p64 < 1e-30)).all() and (co[rows] <= 1).all()
    gone = (masked_free | free) & (out == m)
    assert (co[gone].view(np.uint32) == 0).all(), "a masked row's confidence is not +0"
    kept = hf | (free & (out != m))
    assert (co[kept].view(np.uint32) == cf[kept]).all(), "a kept or held row's confidence was not copied bit for bit"


# ------------------------------------------------------------------------------------------------ the normaliser
@pytest.mark.parametrize("D", [5, 37, 130, 300])
def test_norm_against_fp64(D):
    N, S, m, temp = 3, 6, 2, 0.7
    rng = np.random.default_rng(50 + D)
    x = np.where(rng.random((N, D)) < 0.4, m, rng.integers(3, 6, (N, D))).astype(np.int32)
    held = rng.random((N, D)) < 0.3
    held[1] |= x[1] != m                                                 # sample 1: every entry masked or held
    conf = (1.0 - rng.random((N, D))).astype(np.float32)
    xd, hd, cd = _dev(x, torch.int32), _dev(held, torch.bool), _dev(conf, torch.float32)
    before = native.LAUNCH_COUNTS.get("ctdd_absorb_remask_norm", 0)
    norm = native.absorb_remask_norm(xd, m, cd, hd, temp)
    again = native.absorb_remask_norm(xd, m, cd, hd, temp)
    assert native.LAUNCH_COUNTS["ctdd_absorb_remask_norm"] == before + 2
    assert norm.shape == (N, 2) and norm.dtype == torch.float32
    assert bool((norm.view(torch.int32) == again.view(torch.int32)).all()), "two calls differ"
    norm = norm.cpu().numpy()
    U, Z64 = rc.norm_replay(x, held, conf, m, temp, np.float64)
    _, Z32 = rc.norm_replay(x, held, conf, m, temp, np.float32)
    e32 = float(np.abs(Z32.astype(np.float64) - Z64).max())
    err = np.abs(norm[:, 1].astype(np.float64) - Z64)
    print(f"D={D}: U {U.tolist()}, Z {Z64.tolist()}; error kernel {err.max():.2e} / fp32 {e32:.2e}")
    assert (norm[:, 0] == U).all() and U[1] == 0 and U[0] > 0 and U[2] > 0
    assert (err <= np.maximum(8 * e32, 1e-6 * Z64)).all()
    assert norm[1].tolist() == [0.0, 0.0]
    free_all, _ = rc.norm_replay(x, None, conf, m, temp)
    assert (native.absorb_remask_norm(xd, m, cd, None, temp).cpu().numpy()[:, 0] == free_all).all()
    # the step leaves a sample with the norm (0, 0) alone (and remasks in the others)
    lg = torch.randn(N, D, S, generator=torch.Generator().manual_seed(D)).to(DEV)
    counts = _counts()
    out, co = native.absorb_remask_step(lg, xd, m, 0.0, 1.0, held=hd, conf=cd, norm=_dev(norm, torch.float32), temp=temp, flags=CONF, seed=9,
                                        counts=counts)
    out, co = out.cpu().numpy(), co.cpu().numpy()
    assert (out[1] == x[1]).all() and (co[1][held[1]] == conf[1][held[1]]).all() and (co[1][~held[1]] == 0).all()   # (not held there: masked)
    assert counts.cpu().tolist() == [0, int((out != x).sum())] and (out != x).any()


# ------------------------------------------------------------------------------------------------ the confidence-weighted step
@pytest.mark.parametrize("mode", ac.MODES)
@pytest.mark.parametrize("case", ac.CASES, ids=ac.IDS)
def test_conf_step_matches_the_replay(case, mode):
    S, m, B, D = case
    _, x, lg, xd = _case(case, mode)
    held, conf = rc.held_pattern(case), rc.conf_pattern(case)
    hd, cd, seed = _dev(held, torch.bool), _dev(conf, torch.float32), rc.step_seed(S)
    xf, hf, cf = x.reshape(-1), held.reshape(-1), conf.reshape(-1)
    masked_free = (xf == m) & ~hf
    norm = native.absorb_remask_norm(xd, m, cd, hd, 1.0)
    nh = norm.cpu().numpy()
    for offset, sigma in enumerate((rc.SIGMA_CONF, 1.0)):
        counts = _counts()
        out, co = native.absorb_remask_step(lg, xd, m, 0.3, sigma, held=hd, conf=cd, norm=norm, temp=1.0, flags=CONF, seed=seed, offset=10 + offset,
                                            counts=counts)
        out, co = out.cpu().numpy().reshape(-1), co.cpu().numpy().reshape(-1)
        plain = native.absorb_step(lg, xd, m, 0.3, 0, seed, 10 + offset).cpu().numpy().reshape(-1)
        assert (out[masked_free] == plain[masked_free]).all() and (out[hf] == xf[hf]).all()
        remask, sg, u3, free = rc.remask_replay(x, held, m, sigma, seed, 10 + offset, conf=conf, norm=nh, temp=1.0)
        near = free & (np.abs(u3.astype(np.float64) - sg.astype(np.float64)) < 1e-5)
        print(f"S={S} {mode} sigma={sigma}: {int(free.sum())} free unmasked rows, {int(near.sum())} left out (|u3 - sigma_row| < 1e-5), "
              f"{int((free & (out == m)).sum())} remasked; sigma_row in [{sg[free].min() if free.any() else 0:.3f}, {sg[free].max() if free.any() else 0:.3f}]")
        assert near.sum() <= 0.01 * free.sum()
        sure = free & ~near
        assert ((out[sure] == m) == remask[sure]).all(), "remask decision differs from the replay"
        kept = free & (out != m)
        assert (out[kept] == xf[kept]).all() and (co[kept] == cf[kept]).all() and (co[free & (out == m)] == 0).all()
        assert counts.cpu().tolist() == [int((masked_free & (out != m)).sum()), int((free & (out == m)).sum())]
        if sigma <= 1.0 / np.e:                                          # nothing clamps: the mean over a sample's free unmasked rows is sigma
            for n in range(B):
                rows = free.reshape(B, D)[n]
                if rows.any():
                    mean = float(sg.reshape(B, D)[n][rows].astype(np.float64).mean())
                    assert sg.reshape(B, D)[n][rows].max() < 1.0 and abs(mean - sigma) <= 1e-5, (n, mean)


# ------------------------------------------------------------------------------------------------ in place
@pytest.mark.parametrize("flags", [0, CONF])
@pytest.mark.parametrize("case", ac.CASES, ids=ac.IDS)
def test_in_place_call_equals_the_out_of_place_call(case, flags):
    S, m, B, D = case
    _, x, lg, xd = _case(case, "mix")
    hd, cd, seed = _dev(rc.held_pattern(case), torch.bool), _dev(rc.conf_pattern(case), torch.float32), rc.step_seed(S)
    norm = native.absorb_remask_norm(xd, m, cd, hd, 1.0)
    c1, c2 = _counts(), _counts()
    kw = dict(held=hd, norm=norm, temp=1.0, flags=flags, seed=seed, offset=20)
    want_x, want_c = native.absorb_remask_step(lg, xd, m, 0.5, rc.SIGMA, conf=cd, counts=c1, **kw)
    xi, ci = xd.clone(), cd.clone()
    got_x, got_c = native.absorb_remask_step(lg, xi, m, 0.5, rc.SIGMA, conf=ci, out=xi, conf_out=ci, counts=c2, **kw)
    assert got_x.data_ptr() == xi.data_ptr() and got_c.data_ptr() == ci.data_ptr()
    assert bool((xi == want_x).all()) and bool((ci.view(torch.int32) == want_c.view(torch.int32)).all())
    assert c1.cpu().tolist() == c2.cpu().tolist() and sum(c1.cpu().tolist()) > 0
    assert bool((xd.cpu() == torch.from_numpy(x)).all()), "the out-of-place call wrote into x"


# ------------------------------------------------------------------------------------------------ misuse
def test_argument_errors():
    lg = torch.zeros(2, 3, 4, device=DEV)
    x = torch.full((2, 3), 3, dtype=torch.int32, device=DEV)
    conf, norm, held = torch.ones(2, 3, device=DEV), torch.ones(2, 2, device=DEV), torch.zeros(2, 3, dtype=torch.bool, device=DEV)
    E, step, nrm = native.CtddError, native.absorb_remask_step, native.absorb_remask_norm
    bad_calls = [
        lambda: step(lg.cpu(), x.cpu(), 3, 0.5, 0.1),                                                # CPU tensors
        lambda: nrm(x.cpu(), 3, conf.cpu()),
        lambda: step(lg, x[:, :2].contiguous(), 3, 0.5, 0.1),                                        # shapes
        lambda: step(lg, x, 3, 0.5, 0.1, held=held[:, :2].contiguous()),
        lambda: step(lg, x, 3, 0.5, 0.1, conf=conf[:1].contiguous()),
        lambda: step(lg, x, 3, 0.5, 0.1, conf=conf, conf_out=conf[:1].contiguous()),
        lambda: step(lg, x, 3, 0.5, 0.1, conf=conf, norm=norm[:1].contiguous(), flags=CONF),
        lambda: step(lg, x, 3, 0.5, 0.1, counts=torch.zeros(1, dtype=torch.int32, device=DEV)),
        lambda: step(lg, x, 3, 0.5, 0.1, out=x[:1].contiguous()),
        lambda: nrm(x, 3, conf[:1].contiguous()),
        lambda: nrm(x, 3, conf, held[:1].contiguous()),
        lambda: nrm(x, 3, conf, out=norm[:1].contiguous()),
        lambda: step(lg, x.long(), 3, 0.5, 0.1),                                                     # dtypes
        lambda: step(lg.double(), x, 3, 0.5, 0.1),
        lambda: step(lg, x, 3, 0.5, 0.1, held=held.int()),
        lambda: step(lg, x, 3, 0.5, 0.1, conf=conf.double()),
        lambda: step(lg, x, 3, 0.5, 0.1, counts=torch.zeros(2, device=DEV)),
        lambda: nrm(x, 3, conf.double()),
        lambda: nrm(x.long(), 3, conf),
        lambda: step(lg, x, 4, 0.5, 0.1),                                                            # mask_state outside [0, S)
        lambda: step(lg, x, -1, 0.5, 0.1),
        lambda: step(torch.zeros(1, 2, native.ABSORB_MAX_S + 1, device=DEV), x[:1, :2].contiguous(), 3, 0.5, 0.1),   # S > CTDD_MAX_S
        lambda: step(lg, x, 3, 1.5, 0.1),                                                            # p_unmask, sigma outside [0, 1]
        lambda: step(lg, x, 3, -0.1, 0.1),
        lambda: step(lg, x, 3, float("nan"), 0.1),
        lambda: step(lg, x, 3, 0.5, 1.01),
        lambda: step(lg, x, 3, 0.5, -0.01),
        lambda: step(lg, x, 3, 0.5, float("nan")),
        lambda: step(lg, x, 3, 0.5, 0.1, norm=norm, flags=CONF),                                     # the conf flag without conf / norm
        lambda: step(lg, x, 3, 0.5, 0.1, conf=conf, flags=CONF),
        lambda: step(lg, x, 3, 0.5, 0.1, conf_out=conf),                                             # conf_out without conf_in
        lambda: step(lg, x, 3, 0.5, 0.1, conf=conf, norm=norm, temp=0.019, flags=CONF),              # temp < 0.02
        lambda: step(lg, x, 3, 0.5, 0.1, temp=float("nan")),
        lambda: nrm(x, 3, conf, temp=0.019),
        lambda: step(lg, x, 3, 0.5, 0.1, flags=native.ABSORB_ARGMAX),                                # ARGMAX is refused; unknown bits
        lambda: step(lg, x, 3, 0.5, 0.1, conf=conf, norm=norm, flags=CONF | 4),
        lambda: step(lg, x, 3, 0.5, 0.1, flags=8),
    ]
    for i, call in enumerate(bad_calls):
        with pytest.raises(E):
            call()
            pytest.fail(f"bad call {i} went through")
    # and the well-formed calls go through, at the edge of every range
    out, co = step(lg, x, 3, 1.0, 1.0, held=held, conf=conf, norm=nrm(x, 3, conf, held, 0.02), temp=0.02, flags=CONF)
    assert bool((out != 3).all()) and bool((co > 0).all())
    out, co = step(lg, x, 3, 0.0, 0.0)
    assert bool((out == 3).all()) and co is None


# ------------------------------------------------------------------------------------------------ the sampler
class _TimeOnlyModel:
    """Logits that depend on the time (and the dimension) only: toy_logits at x = 0."""

    def __init__(self, S, m):
        self.S, self.device = S, DEV
        self.process = process.DeviceForwardProcess("absorbing", S, DEV, rate_const=1.0, t_func="loglinear", alpha_eps=1e-3, mask_state=m)

    def __call__(self, x, t):
        return toy_logits(torch.zeros_like(x), t, self.S, scale=3.0)


S_, M_, N_, D_, K_ = 6, 2, 100, 30, 10
SEED = 20240921
LAUNCHES = ("ctdd_absorb_remask_norm", "ctdd_absorb_remask_step", "ctdd_absorb_step")


def _sampler(name="AbsorbingRemask", rule="ancestral", num_steps=K_, **kw):
    import lib.sampling.sampling  # noqa: F401
    import lib.sampling.sampling_utils as su
    from ctdd.config_dict import ConfigDict
    cfg = ConfigDict()
    for sec in ("data", "model", "sampler", "training", "loss"):
        cfg[sec] = ConfigDict()
    cfg.data.S, cfg.model.concat_dim, cfg.training.max_t = S_, D_, 1.0
    cfg.sampler.update(name=name, rule=rule, num_steps=num_steps, min_t=0.01)
    cfg.sampler.update(**kw)
    sampler = su.get_sampler(cfg)
    sampler.seed = SEED
    return sampler


def _launches():
    return [native.LAUNCH_COUNTS.get(k, 0) for k in LAUNCHES]


def _known(N):
    g = torch.Generator().manual_seed(3)
    x_known = torch.randint(0, S_ - 1, (N, D_), generator=g)
    return x_known + (x_known >= M_).long(), torch.rand(N, D_, generator=g) < 0.4     # (skips the mask state)


def test_eta_zero_is_absorbing_leap():
    model = _TimeOnlyModel(S_, M_)
    want_x, want_changed = _sampler("AbsorbingLeap").sample(model, N_)
    for strategy in ("cap", "rescale", "conf"):
        sampler = _sampler(remask=strategy, remask_eta=0.0)
        x, changed = sampler.sample(model, N_)
        assert (x == want_x).all() and changed == want_changed, strategy
        assert sampler.remasked == [0.0] * K_
    x_known, held = _known(N_)
    assert (_sampler(remask_eta=0.0).inpaint(model, x_known, held) == _sampler("AbsorbingLeap").inpaint(model, x_known, held)).all()


@pytest.mark.parametrize("strategy,eta", [("cap", 0.05), ("rescale", 0.5)])
def test_ancestral_statistics_follow_the_schedule(strategy, eta):
    from lib.sampling.sampling import remask_schedule
    model, sampler = _TimeOnlyModel(S_, M_), _sampler(remask=strategy, remask_eta=eta)
    before = _launches()
    x, changed = sampler.sample(model, N_)
    assert [a - b for a, b in zip(_launches(), before)] == [0, K_, 1]
    remasked = sampler.remasked
    assert x.shape == (N_, D_) and len(changed) == len(remasked) == K_ and (x != M_).all() and ((x >= 0) & (x < S_)).all()
    # the schedule, restated: AbsorbingLeap's p, then remask_schedule (tests/test_absorb_remask_cpu.py holds it to exact rationals)
    ts = np.concatenate((np.linspace(1.0, 0.01, K_), [0.0]))
    t64 = torch.from_numpy(ts)
    p = torch.clamp(model.process.unmask_prob(t64[:-1], t64[:-1] - t64[1:], "ancestral"), 0.0, 1.0).tolist()
    sigma, pp = remask_schedule(p, strategy, eta)
    surv = np.concatenate(([1.0], np.cumprod(1.0 - np.asarray(p))))
    share = 1.0 - np.cumsum((np.asarray(changed) - np.asarray(remasked)) * N_) / (N_ * D_)
    for k in (0, 4, 8):
        want = surv[k + 1]
        sd = np.sqrt(want * (1 - want) / (N_ * D_))
        print(f"{strategy}: masked share after step {k}: {share[k]:.4f}, expected {want:.4f} (sigma {sd:.4f}); remasked {remasked[k] * N_:.0f}")
        assert abs(share[k] - want) <= 5 * sd
    assert abs(share[-1]) < 1e-12 and sigma[-1] == 0.0
    print(f"{strategy}: {sum(remasked) * N_:.0f} entries remasked in all, expected {N_ * D_ * sum(s * (1 - v) for s, v in zip(sigma, surv)):.1f}")
    assert sum(remasked) > 0
    # an entry unmasks for the last time at step k with probability pi_k, and then holds a draw from the softmax at t_k over s != m
    pi = np.array([surv[k] * pp[k] * np.prod([1.0 - s for s in sigma[k + 1:]]) for k in range(K_)])
    assert abs(pi.sum() - 1.0) < 1e-12
    t32 = torch.from_numpy(ts[:-1]).float()
    probs = np.zeros((D_, S_))
    for k in range(K_):
        l = toy_logits(torch.zeros(1, D_), t32[k:k + 1], S_, scale=3.0)[0].double()
        l[:, M_] = -np.inf
        probs += pi[k] * torch.softmax(l, -1).numpy()
    want = probs.mean(0)
    freq = np.bincount(x.reshape(-1), minlength=S_) / (N_ * D_)
    for s in range(S_):
        sd = np.sqrt(max(want[s] * (1 - want[s]), 1e-12) / (N_ * D_))
        print(f"{strategy}: state {s} frequency {freq[s]:.4f}, expected {want[s]:.4f} (sigma {sd:.4f})")
        assert abs(freq[s] - want[s]) <= 5 * sd
    again, changed_again = sampler.sample(model, N_)
    assert (again == x).all() and changed_again == changed and sampler.remasked == remasked, "a fixed seed does not fix the sample"


@pytest.mark.parametrize("rule", ["euler", "tauleap"])
def test_other_rules_finish_without_a_mask_state(rule):
    model, sampler = _TimeOnlyModel(S_, 5), _sampler(rule=rule, num_steps=6, remask_eta=0.05)
    x, changed = sampler.sample(model, N_)
    assert x.shape == (N_, D_) and (x != 5).all() and ((x >= 0) & (x < S_)).all() and len(changed) == 6 and len(sampler.remasked) == 6
    assert sum(changed) > 0


def test_inpaint_under_full_rescale_keeps_held_entries():
    model, sampler = _TimeOnlyModel(S_, M_), _sampler(remask="rescale", remask_eta=1.0)
    x_known, held = _known(16)
    out = sampler.inpaint(model, x_known, held)
    hn = held.numpy()
    assert out.shape == (16, D_) and (out[hn] == x_known.numpy()[hn]).all()
    assert (out != M_).all() and ((out >= 0) & (out < S_)).all() and sum(sampler.remasked) > 0
    before = _launches()
    same = sampler.inpaint(model, x_known, torch.ones(D_, dtype=torch.bool))
    assert (same == x_known.numpy()).all() and _launches() == before
    bad = x_known.clone()
    bad[0, 0] = M_
    with pytest.raises(ValueError, match="mask state"):
        sampler.inpaint(model, bad, torch.ones(D_, dtype=torch.bool))


def test_conf_strategy_runs_norm_and_step_per_grid_step():
    model, sampler = _TimeOnlyModel(S_, M_), _sampler(remask="conf", remask_eta=0.2, remask_temp=0.5)
    before = _launches()
    x, changed = sampler.sample(model, N_)
    assert [a - b for a, b in zip(_launches(), before)] == [K_, K_, 1]
    assert x.shape == (N_, D_) and (x != M_).all() and ((x >= 0) & (x < S_)).all() and len(changed) == K_
    remasked = sampler.remasked
    assert sum(remasked) > 0
    again, changed_again = sampler.sample(model, N_)
    assert (again == x).all() and changed_again == changed and sampler.remasked == remasked
    x_known, held = _known(16)
    out = sampler.inpaint(model, x_known, held)
    hn = held.numpy()
    assert (out[hn] == x_known.numpy()[hn]).all() and (out != M_).all() and ((out >= 0) & (out < S_)).all()
