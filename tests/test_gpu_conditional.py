"""GPU: conditional sampling on the row-list tau-leap step kernels.

1. the row-list entry points (ctdd_tauleap_step_rows, ctdd_tauleap_step_s256_rows) against the full launches: listed rows
   bit-identical, unlisted rows untouched, counters over listed rows only -- every kernel path, every call kind;
2. ConditionalTauLeaping / ConditionalPCTauLeaping against a CPU restatement of the reference loops
   (TAUnSDDM/lib/sampling/sampling.py:649-758, 761-905) on a score function that couples the dimensions;
3. the samplers on the HIP engines (MNIST U-Net, maze hollow transformer)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import ctmc_ops as ops
from oracle import samplers as osamp
from oracle.forward_process import ForwardProcess

GAUSS = dict(rate_sigma=6.0, Q_sigma=512.0, time_exp=100.0, time_base=3.0)
UNIVAR = dict(rate_const=1.7, t_func="sqrt_cos")


# ------------------------------------------------------------------------------------------------ 1. kernel contract
PATHS = ["s2", "s3", "s37", "s256_x3", "s256_bf16", "s256_bf16_l16"]
CALLS = ["plain", "ordinal", "corrector", "x_base"]
N_, D_ = 5, 131                    # 655 rows: five 128-row tiles and a partial sixth


def _row_lists(R):
    g = torch.Generator().manual_seed(5)
    runs = torch.cat([torch.arange(120, 136), torch.arange(250, 262), torch.arange(383, 390), torch.arange(500, 640),
                      torch.arange(645, R)])
    return {"random": (torch.rand(R, generator=g) < 0.5).nonzero().view(-1), "empty": torch.zeros(0, dtype=torch.int64),
            "all": torch.arange(R), "single": torch.tensor([R // 3]), "last": torch.tensor([R - 1]), "tile_edges": runs}


def _process(S):
    from ctdd.process import DeviceForwardProcess
    return DeviceForwardProcess("univar", S, "cuda", **UNIVAR) if S <= 3 else DeviceForwardProcess("gaussian", S, "cuda", **GAUSS)


@pytest.mark.parametrize("call", CALLS)
@pytest.mark.parametrize("path", PATHS)
def test_row_list_step_matches_full_launch(path, call):
    from ctdd import native
    S = {"s2": 2, "s3": 3, "s37": 37}.get(path, 256)
    R = N_ * D_
    pr = _process(S)
    t32 = torch.tensor([0.5])
    qt0 = pr.tables(t32, want_qt0=True)[0]
    beta = float(pr.beta(t32)[0])
    g = torch.Generator().manual_seed(11)
    logits = (torch.randn(N_, D_, S, generator=g) * 3.0).cuda()
    if path == "s256_bf16_l16":
        logits = logits.to(torch.bfloat16)
    x = torch.randint(0, S, (N_, D_), generator=g).to(torch.int32).cuda()
    xb = torch.randint(0, S, (N_, D_), generator=g).to(torch.int32).cuda() if call == "x_base" else None
    flags = {"plain": 0, "ordinal": native.STEP_ORDINAL, "corrector": native.STEP_ORDINAL | native.STEP_CORRECTOR,
             "x_base": native.STEP_ORDINAL}[call]
    tabs = native.S256Tables(qt0, pr.base_rate, 1e-9, bf16=path != "s256_x3") if S == 256 else None
    seed, offset = 987654321, 3
    moved_any = 0
    for h in (0.004, 0.3):
        for want_rates in ((False, True) if S == 256 else (False,)):
            ch_full = torch.zeros(1, dtype=torch.int32, device="cuda")
            if S == 256:
                full = native.tauleap_step_s256(logits, x, tabs, 0, beta, h, flags, seed, offset, x_base=xb, changed=ch_full,
                                                want_rates=want_rates)
                full, rates_full = full if want_rates else (full, None)
            else:
                full = native.tauleap_step(native.BRANCH_CTELBO, "direct", logits, x, qt0[0], pr.base_rate, beta, 1e-9, h, flags,
                                           seed, offset, x_base=xb, changed=ch_full)
            moved = (full != x).view(-1).cpu()
            assert int(ch_full) == int(moved.sum())
            moved_any += int(moved.sum())
            for name, rows in _row_lists(R).items():
                rows_d = rows.to(torch.int32).cuda()
                out = torch.full((N_, D_), -7, dtype=torch.int32, device="cuda")
                ch = torch.zeros(1, dtype=torch.int32, device="cuda")
                if S == 256:
                    rates = torch.full((N_, D_, S), -1.0, device="cuda") if want_rates else None
                    got = native.tauleap_step_s256_rows(logits, x, tabs, 0, beta, h, flags, seed, offset, rows_d, x_base=xb, out=out,
                                                        changed=ch, want_rates=want_rates, rates=rates)
                    got = got[0] if want_rates else got
                else:
                    got = native.tauleap_step_rows(native.BRANCH_CTELBO, "direct", logits, x, qt0[0], pr.base_rate, beta, 1e-9, h,
                                                   flags, seed, offset, rows_d, x_base=xb, out=out, changed=ch)
                assert got.data_ptr() == out.data_ptr()
                listed = torch.zeros(R, dtype=torch.bool)
                listed[rows] = True
                gv, fv = got.view(-1).cpu(), full.view(-1).cpu()
                assert torch.equal(gv[listed], fv[listed]), (path, call, h, name)
                assert (gv[~listed] == -7).all(), (path, call, h, name)
                assert int(ch) == int(moved[listed].sum()), (path, call, h, name)
                if want_rates:
                    rg, rf = rates.view(R, S).cpu(), rates_full.view(R, S).cpu()
                    assert torch.equal(rg[listed].view(torch.int32), rf[listed].view(torch.int32)), (path, call, h, name)
                    assert (rg[~listed] == -1.0).all()
    assert moved_any > 0


def test_row_list_default_out_is_copy_and_aliasing_refused():
    from ctdd import native
    S = 37
    pr = _process(S)
    t32 = torch.tensor([0.5])
    qt0 = pr.tables(t32, want_qt0=True)[0]
    logits = torch.randn(2, 40, S).cuda()
    x = torch.randint(0, S, (2, 40)).to(torch.int32).cuda()
    rows = torch.tensor([3, 41, 79], dtype=torch.int32).cuda()
    before = dict(native.LAUNCH_COUNTS)
    out = native.tauleap_step_rows(native.BRANCH_CTELBO, "direct", logits, x, qt0[0], pr.base_rate, float(pr.beta(t32)[0]), 1e-9,
                                   0.5, native.STEP_ORDINAL, 1, 0, rows)
    assert native.LAUNCH_COUNTS.get("ctdd_tauleap_step_rows", 0) == before.get("ctdd_tauleap_step_rows", 0) + 1
    keep = torch.ones(80, dtype=torch.bool)
    keep[[3, 41, 79]] = False
    assert out.data_ptr() != x.data_ptr() and torch.equal(out.view(-1)[keep.cuda()], x.view(-1)[keep.cuda()])
    with pytest.raises(native.CtddError):
        native.tauleap_step_rows(native.BRANCH_CTELBO, "direct", logits, x, qt0[0], pr.base_rate, 1.0, 1e-9, 0.5, 0, 1, 0, rows, out=x)


# ------------------------------------------------------------------------------------------------ 2. law
def coupled_logits(x, t, S, scale=2.0):
    """Peaked around a t-dependent shrink towards S/2 of a mix of the own state and the sample's MEAN state: every
    dimension depends on all others, so what is held changes the law of what is free."""
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


def _ref_rates(proc, logits, x, t, eps):
    """CT-ELBO reverse rates, own state zeroed, at the scalar time t (all samples share it: one table, rows flattened)."""
    N, D, S = logits.shape
    tt = torch.tensor([t], dtype=torch.float64).to(torch.float32)
    q, r = proc.transition(tt), proc.rate(tt)
    rr, _ = ops.reverse_rates_ctelbo(logits.reshape(1, N * D, S), x.reshape(1, N * D), q, r, eps)
    return ops.zero_own_state(rr, x.reshape(1, N * D)).view(N, D, S), ops.transpose_forward_rates(r, x.reshape(1, N * D)).view(N, D, S)


def _ref_conditional(proc, cond, D, S, *, pc, min_t, num_steps, init_std, initial_dist, eps, reject_multiple_jumps=False,
                     corrector_entry_time=0.0, num_corrector_steps=0, corrector_step_size_multiplier=1.5):
    """CPU restatement of ConditionalTauLeaping (sampling.py:649-758, pc=False) / ConditionalPCTauLeaping (761-905, pc=True)."""
    N, cd = cond.shape
    sD = D - cd
    x = osamp.initial_samples(N, sD, S, initial_dist, init_std)
    net = lambda xx, t: coupled_logits(torch.cat((cond, xx), 1), t * torch.ones((N,)), S)[:, cd:]
    if not pc:
        ts = np.concatenate((np.linspace(1.0, min_t, num_steps), np.array([0])))
        for idx, t in enumerate(ts[:-1]):
            h = ts[idx] - ts[idx + 1]
            rr, _ = _ref_rates(proc, net(x, t), x, t, eps)
            x = ops.tauleap_apply(x, torch.poisson(rr * h), True)       # (line 744 overwrites the reject branch)
    else:
        h = 1.0 / num_steps
        ts = np.linspace(1.0, min_t + h, num_steps)
        for idx, t in enumerate(ts[:-1]):
            h = ts[idx] - ts[idx + 1]
            rr, _ = _ref_rates(proc, net(x, t), x, t, eps)
            x = ops.tauleap_apply(x, torch.poisson(rr * h), not reject_multiple_jumps)
            if t <= corrector_entry_time:
                for _ in range(num_corrector_steps):
                    rr, tf = _ref_rates(proc, net(x, t - h), x, t - h, eps)
                    corr = ops.zero_own_state(tf + rr, x)
                    x = ops.tauleap_apply(x, torch.poisson(corr * (corrector_step_size_multiplier * h)), not reject_multiple_jumps)
    x0 = torch.max(F.softmax(net(x, min_t), dim=2), dim=2)[1]
    return torch.cat((cond, x0), 1).numpy().astype(int)


def _two_sample_chi2(a, b, S):
    ca = np.bincount(a.ravel(), minlength=S).astype(np.float64)
    cb = np.bincount(b.ravel(), minlength=S).astype(np.float64)
    m = (ca + cb) > 0
    k1, k2 = np.sqrt(cb.sum() / ca.sum()), np.sqrt(ca.sum() / cb.sum())
    return (((k1 * ca - k2 * cb) ** 2)[m] / (ca + cb)[m]).sum(), int(m.sum()) - 1


def _law_cfg(name, S, D, cd, **over):
    from config.mnist_config.config_tauUnet_mnist import get_config
    c = get_config()
    c.data.S, c.model.concat_dim = S, D
    c.sampler.name, c.sampler.condition_dim = name, cd
    c.sampler.num_steps = 10
    c.sampler.num_corrector_steps = 0
    c.sampler.step_precision = "fp32"
    for k, v in over.items():
        c.sampler[k] = v
    return c


@pytest.mark.parametrize("S", [3, 37, 256])
@pytest.mark.parametrize("name", ["ConditionalTauLeaping", "ConditionalPCTauLeaping"])
def test_conditional_law_matches_reference_restatement(name, S):
    import lib.sampling.sampling  # noqa: F401
    import lib.sampling.sampling_utils as su
    from ctdd import native
    N, D, cd = 2000, 12, 4
    kind, params = "gaussian", GAUSS                             # (the grid starts at t = 1.0: sqrt_cos schedules are singular there)
    over = dict(initial_dist="uniform" if S == 3 else "gaussian")
    if name == "ConditionalPCTauLeaping":
        over.update(corrector_entry_time=0.6, num_corrector_steps=2)
    cfg = _law_cfg(name, S, D, cd, **over)
    sampler = su.get_sampler(cfg)
    sampler.seed = 4321
    model = CoupledToy(kind, S, **params)
    g = torch.Generator().manual_seed(2)
    cond = torch.randint(0, S, (N, cd), generator=g)
    before = dict(native.LAUNCH_COUNTS)
    hip = sampler.sample(model, N, cond)
    entry = "ctdd_tauleap_step_s256_rows" if S == 256 else "ctdd_tauleap_step_rows"
    assert native.LAUNCH_COUNTS.get(entry, 0) > before.get(entry, 0)
    assert hip.shape == (N, D) and hip.dtype.kind == "i" and hip.min() >= 0 and hip.max() < S
    assert (hip[:, :cd] == cond.numpy()).all()
    torch.manual_seed(7)
    s = cfg.sampler
    ref = _ref_conditional(ForwardProcess(kind, S, **params), cond, D, S, pc=name == "ConditionalPCTauLeaping", min_t=s.min_t,
                           num_steps=s.num_steps, init_std=cfg.model.Q_sigma, initial_dist=s.initial_dist, eps=s.eps_ratio,
                           corrector_entry_time=s.corrector_entry_time, num_corrector_steps=s.num_corrector_steps,
                           corrector_step_size_multiplier=s.corrector_step_size_multiplier)
    # marginal of each free dimension on its own: the coupled score makes the dimensions of a sample strongly correlated, so
    # counts pooled over dimensions are not independent draws (their chi-square is over-dispersed)
    for d in range(cd, D):
        chi2, dof = _two_sample_chi2(hip[:, d], ref[:, d], S)
        assert chi2 < dof + 6 * np.sqrt(2 * dof) + 10, (d, chi2, dof)
    se = np.sqrt(hip[:, cd:].var(0) / N + ref[:, cd:].var(0) / N) + 1e-9
    assert (np.abs(hip[:, cd:].mean(0) - ref[:, cd:].mean(0)) / se).max() < 5.5
    # the conditioner matters: two constant conditioners give clearly different free marginals
    lo = sampler.sample(model, N, torch.full((N, cd), S // 5))
    hi = sampler.sample(model, N, torch.full((N, cd), S - 1 - S // 5))
    for d in range(cd, D):
        chi2, dof = _two_sample_chi2(lo[:, d], hi[:, d], S)
        assert chi2 > dof + 20 * np.sqrt(2 * dof) + 50, (d, chi2, dof)


# ------------------------------------------------------------------------------------------------ 3. engines
@pytest.fixture(scope="module")
def unet():
    import lib.models.models  # noqa: F401
    import lib.models.model_utils as mu
    import lib.sampling.sampling  # noqa: F401
    from config.mnist_config.config_tauUnet_mnist import get_config
    cfg = get_config()
    cfg.sampler.num_steps = 5
    # one stream per forward: the GroupNorm statistics meet in float atomics, and only a single plan in flight makes the
    # network's logits -- and so a fixed-seed sampler run -- bit-reproducible
    cfg.model.engine_streams = 1
    torch.manual_seed(0)
    model = mu.create_model(cfg, torch.device("cuda"))
    model.eval()
    return cfg, model


def _run(cfg, model, name, how, N, seed=77, **over):
    import copy
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
    delta = {k: native.LAUNCH_COUNTS.get(k, 0) - before.get(k, 0) for k in native.LAUNCH_COUNTS}
    return sampler, out, delta


@pytest.mark.parametrize("case", ["taul_n64", "taul_n256_pipelined", "pc_correctors", "inpaint_random_mask"])
def test_unet_engine_conditional(unet, case):
    cfg, model = unet
    D, S = cfg.model.concat_dim, cfg.data.S
    N = 256 if case == "taul_n256_pipelined" else 64
    g = torch.Generator().manual_seed(9)
    x_known = torch.randint(0, S, (N, D), generator=g)
    if case == "inpaint_random_mask":
        mask = torch.rand(N, D, generator=g) < 0.4
    else:
        mask = torch.zeros(D, dtype=torch.bool)
        mask[:392] = True                                         # the top half of the digit
    name = "ConditionalPCTauLeaping" if case == "pc_correctors" else "ConditionalTauLeaping"
    over = dict(condition_dim=392, num_steps=5, pipeline_sub_batches=2 if case == "taul_n256_pipelined" else 1)
    if case == "pc_correctors":
        over.update(corrector_entry_time=0.9, num_corrector_steps=1)
    if case in ("taul_n64", "taul_n256_pipelined"):
        how = lambda s: s.sample(model, N, x_known[:, :392])
    else:
        how = lambda s: s.inpaint(model, x_known, mask)
    sampler, out, delta = _run(cfg, model, name, how, N, **over)
    if case == "taul_n256_pipelined":
        assert sampler._pipeline_parts(model, N) == 2
    if case == "taul_n64":
        assert sampler._pipeline_parts(model, N) == 1
    m = mask.expand(N, D).numpy()
    assert out.shape == (N, D) and out.min() >= 0 and out.max() < S
    assert (out[m] == x_known.numpy()[m]).all()
    assert delta.get("ctdd_tauleap_step_s256_rows", 0) > 0 and delta.get("ctdd_tauleap_step_rows", 0) == 0
    _, again, _ = _run(cfg, model, name, how, N, **over)
    if case == "taul_n256_pipelined":       # two plans in flight: the last bits of some logits may move
        assert (again != out).mean() < 1e-3
    else:
        assert (again == out).all()                               # fixed seed: the same samples


def test_unet_engine_all_held_launches_nothing(unet):
    cfg, model = unet
    D, S = cfg.model.concat_dim, cfg.data.S
    x_known = torch.randint(0, S, (16, D))
    _, out, delta = _run(cfg, model, "ConditionalTauLeaping", lambda s: s.inpaint(model, x_known, torch.ones(D, dtype=torch.bool)), 16)
    assert (out == x_known.numpy()).all() and all(v == 0 for v in delta.values())


def test_maze_hollow_inpaint():
    import lib.models.models  # noqa: F401
    import lib.models.model_utils as mu
    import lib.sampling.sampling  # noqa: F401
    from config.maze_config.config_hollow_maze import get_config
    cfg = get_config()
    torch.manual_seed(0)
    model = mu.create_model(cfg, torch.device("cuda"))
    model.eval()
    N, D, S = 64, cfg.model.concat_dim, cfg.data.S
    g = torch.Generator().manual_seed(4)
    x_known = torch.randint(0, S, (N, D), generator=g)
    mask = torch.rand(N, D, generator=g) < 0.5
    how = lambda s: s.inpaint(model, x_known, mask)
    _, out, delta = _run(cfg, model, "ConditionalTauLeaping", how, N, num_steps=6, condition_dim=100)
    assert out.shape == (N, D) and out.min() >= 0 and out.max() < S
    assert (out[mask.numpy()] == x_known.numpy()[mask.numpy()]).all()
    assert delta.get("ctdd_tauleap_step_rows", 0) > 0 and delta.get("ctdd_tauleap_step_s256_rows", 0) == 0
    _, again, _ = _run(cfg, model, "ConditionalTauLeaping", how, N, num_steps=6, condition_dim=100)
    assert (again == out).all()
    _, held, delta = _run(cfg, model, "ConditionalPCTauLeaping", lambda s: s.inpaint(model, x_known, torch.ones(N, D, dtype=torch.bool)), N,
                          num_steps=6)
    assert (held == x_known.numpy()).all() and all(v == 0 for v in delta.values())
