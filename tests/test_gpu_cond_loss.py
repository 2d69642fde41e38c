"""GPU: prefix-conditioned training -- K11 on a window of rows (ctdd_ctelbo_loss_window) and the CondCTElbo loss on it.
1. the window entry against the dense entry on the contiguous slice: bit-identical value and window gradient, exact zeros on
   the held rows, nothing written outside the gradient buffer -- every kernel path and its tile boundaries;
2. the window entry against the differentiable restatement in fp64;
3. CondCTElbo.calc_loss on the noise the reference drew (tests/golden/cond_losses.npz): value, d/dtheta, what reached the model,
   which entry points ran, and the torch-op path (cfg.loss.fused = False);
4. the HIP noising inside the loss;
5. the conditional MNIST config end to end: one training step, then ConditionalTauLeaping on the trained object."""
import ast

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

T = torch.from_numpy
GAUSS = dict(rate_sigma=6.0, Q_sigma=512.0, time_exp=100.0, time_base=3.0)
KEYS = ("ctdd_ctelbo_loss", "ctdd_ctelbo_loss_terms", "ctdd_ctelbo_loss_window")


def _device_process(kind, S, t_func="sqrt_cos"):
    from ctdd.process import DeviceForwardProcess
    return DeviceForwardProcess(kind, S, "cuda", **(GAUSS if kind == "gaussian" else dict(rate_const=1.7, t_func=t_func)))


def _delta(before):
    from ctdd import native
    return {k: native.LAUNCH_COUNTS.get(k, 0) - before.get(k, 0) for k in KEYS}


# ------------------------------------------------------------------------------------------------ 1 / 2: the kernel
#          S    B  Dl   off D
SHAPES = [(256, 3, 21, 4, 17),        # wave path: 16 rows per workgroup, plus tail
          (256, 2, 140, 3, 137),      # crosses the 128-row GEMM tile, window ends at the buffer end
          (32, 2, 140, 3, 137),       # thread-per-state + GEMM
          (96, 2, 12, 5, 7),          # thread-per-state + GEMM
          (37, 4, 20, 7, 13),         # FMA path, tail of the 8-row workgroup
          (3, 5, 15, 7, 8),           # exactly one 8-row workgroup
          (16, 2, 15, 2, 9),          # held rows on both sides
          (16, 3, 6, 5, 1)]           # d = 1
W_, NLLW_, EPS_ = 0.7, 0.3, 1e-9
GUARD = 1024                          # floats of sentinel on either side of the gradient buffer


def _inputs(S, B, Dl, off, D):
    gen = torch.Generator().manual_seed(S * 1000 + Dl * 10 + off)
    # (the S = 256 Gaussian tables on fewer states put q(x0 -> x_t) below fp32 resolution for random pairs: uniform rates there)
    proc = _device_process("gaussian" if S == 256 else "uniform", S)
    ts = (torch.rand(B, generator=gen) * 0.9 + 0.05).cuda()
    qt0, qT, rate, _ = proc.tables(ts, want_qt0=True, want_qt0T=True, want_rate=True)
    x0 = torch.randint(0, S, (B, D), generator=gen).cuda()
    x_t = torch.randint(0, S, (B, D), generator=gen).cuda()
    x_tilde = x_t.clone()
    x_tilde[:, min(1, D - 1)] = (x_tilde[:, min(1, D - 1)] + 1) % S
    la = torch.randn(B, Dl, S, generator=gen).cuda()
    lb = torch.randn(B, Dl, S, generator=gen).cuda()
    return qt0, qT, rate, x0, x_t, x_tilde, la, lb


def _guarded(B, Dl, S):
    """A NaN-filled (B, Dl, S) gradient buffer inside a larger allocation of sentinels."""
    buf = torch.full((B * Dl * S + 2 * GUARD,), 777.0, device="cuda")
    grad = buf[GUARD:GUARD + B * Dl * S].view(B, Dl, S)
    grad.fill_(float("nan"))
    return buf, grad


@pytest.mark.parametrize("weights", ["one_pass", "reg_half", "sig_half"])
@pytest.mark.parametrize("S,B,Dl,off,D", SHAPES)
def test_window_entry_is_the_dense_entry_on_the_slice(S, B, Dl, off, D, weights):
    from ctdd import native
    qt0, qT, rate, x0, x_t, x_tilde, la, _ = _inputs(S, B, Dl, off, D)
    nll = NLLW_ / (B * D)
    sig, reg, nll, xs = {"one_pass": (1.0, 1.0, nll, x_tilde), "reg_half": (0.0, W_, 0.0, x_t), "sig_half": (W_, 0.0, nll, x_tilde)}[weights]
    keep = la.clone()
    buf, grad = _guarded(B, Dl, S)
    before = dict(native.LAUNCH_COUNTS)
    val, got = native.ctelbo_loss_window(la, x0.int(), xs.int(), qt0, qT, rate, EPS_, sig, reg, nll, off, grad_out=grad)
    assert _delta(before) == {"ctdd_ctelbo_loss": 0, "ctdd_ctelbo_loss_terms": 0, "ctdd_ctelbo_loss_window": 1}
    assert got.data_ptr() == grad.data_ptr() and got.shape == (B, Dl, S)
    dval, dgrad = native.ctelbo_loss(la[:, off:off + D].contiguous(), x0.int(), xs.int(), qt0, qT, rate, EPS_, sig, nll, reg_scale=reg)
    torch.cuda.synchronize()
    assert torch.equal(la, keep)                                             # the logits are read in place, never written
    assert torch.isfinite(dval) and torch.isfinite(dgrad).all() and dgrad.abs().max().item() > 0
    assert torch.equal(val, dval), (val.item(), dval.item())
    assert torch.equal(got[:, off:off + D], dgrad), (got[:, off:off + D] - dgrad).abs().max().item()
    held = torch.ones(Dl, dtype=torch.bool, device="cuda")
    held[off:off + D] = False
    assert (got[:, held] == 0).all()                                         # (NaN before the call: every held element was written)
    assert (buf[:GUARD] == 777.0).all() and (buf[-GUARD:] == 777.0).all()    # nothing before or past the buffer
    # a fresh gradient tensor (no grad_out) is the same
    val2, got2 = native.ctelbo_loss_window(la, x0.int(), xs.int(), qt0, qT, rate, EPS_, sig, reg, nll, off)
    assert torch.equal(val2, val) and torch.equal(got2, got)


def test_window_over_the_whole_tensor_is_the_dense_entry():
    from ctdd import native
    S, B, D = 256, 2, 21
    qt0, qT, rate, x0, _, x_tilde, la, _ = _inputs(S, B, D, 0, D)
    val, got = native.ctelbo_loss_window(la, x0.int(), x_tilde.int(), qt0, qT, rate, EPS_, W_, 0.5, 0.01, 0)
    dval, dgrad = native.ctelbo_loss(la, x0.int(), x_tilde.int(), qt0, qT, rate, EPS_, W_, 0.01, reg_scale=0.5)
    assert torch.equal(val, dval) and torch.equal(got, dgrad)


@pytest.mark.parametrize("bad", ["off_negative", "past_the_end", "x_shape"])
def test_window_entry_refuses_bad_windows(bad):
    from ctdd import native
    S, B, Dl, D = 16, 2, 10, 4
    qt0, qT, rate, x0, _, x_tilde, la, _ = _inputs(S, B, Dl, 3, D)
    off = {"off_negative": -1, "past_the_end": Dl - D + 1, "x_shape": 3}[bad]
    xt = x_tilde[:, :3] if bad == "x_shape" else x_tilde
    with pytest.raises(native.CtddError):
        native.ctelbo_loss_window(la, x0.int(), xt.int().contiguous(), qt0, qT, rate, EPS_, 1.0, 1.0, 0.0, off)
    lib = native.load()                                                      # ... and the library itself, not only the wrapper
    scratch = torch.empty(int(lib.ctdd_ctelbo_scratch_bytes(B, D, S)), dtype=torch.uint8, device="cuda")
    grad, out = torch.full_like(la, 5.0), torch.zeros(1, device="cuda")
    p = lambda t: t.data_ptr()
    x0i, xti = x0.int(), x_tilde.int()
    for o in (-1, Dl - D + 1):
        rc = lib.ctdd_ctelbo_loss_window(p(la), p(x0i), p(xti), p(qt0), p(qT), p(rate), B, D, S, Dl, o, EPS_, 1.0, 1.0, 0.0,
                                         p(scratch), p(grad), p(out), torch.cuda.current_stream().cuda_stream)
        assert rc != 0
    torch.cuda.synchronize()
    assert (grad == 5.0).all()                                               # refused before any launch


@pytest.mark.parametrize("S,B,Dl,off,D", [SHAPES[0], SHAPES[4]])
def test_window_entry_against_fp64(S, B, Dl, off, D):
    """Value and per-element d/dlogits (full shape) of the two-pass composition -- regulariser at model(x_t), signal and cross
    entropy at model(x~), as CondCTElbo -- and of the one-pass objective against _ct_elbo_terms + cross entropy in fp64 on the
    slices; the bounds test_ctelbo_term_weights_compose_the_two_pass_objective applies to the same kernels."""
    import lib.losses.losses as L
    from ctdd import native
    qt0, qT, rate, x0, x_t, x_tilde, la, lb = _inputs(S, B, Dl, off, D)
    la.requires_grad_()
    lb.requires_grad_()
    nll = NLLW_ / (B * D)
    sl = lambda l: l[:, off:off + D].double()
    ref = W_ * L._ct_elbo_terms(sl(la), sl(lb), x0, x_t, x_tilde, qt0.double(), rate.double(), EPS_) + \
        NLLW_ * F.cross_entropy(sl(lb).permute(0, 2, 1), x0)
    ga, gb = torch.autograd.grad(ref, (la, lb))
    va, da = native.ctelbo_loss_window(la.detach(), x0.int(), x_t.int(), qt0, qT, rate, EPS_, 0.0, W_, 0.0, off)
    vb, db = native.ctelbo_loss_window(lb.detach(), x0.int(), x_tilde.int(), qt0, qT, rate, EPS_, W_, 0.0, nll, off)
    print(f"two-pass S={S}: value {(va + vb).item():.8g} vs fp64 {ref.item():.10g}")
    np.testing.assert_allclose((va + vb).item(), ref.item(), rtol=2e-5)
    scale = max(ga.abs().max().item(), gb.abs().max().item())
    for got, want in ((da, ga), (db, gb)):
        err = (got - want.float()).abs().max().item()
        print(f"  max |d/dlogits - fp64| = {err:.3e} (bar {1e-3 * scale:.3e})")
        assert err <= 1e-3 * scale, (err, scale)
    ref1 = L._ct_elbo_terms(sl(lb), sl(lb), x0, x_tilde, x_tilde, qt0.double(), rate.double(), EPS_) + \
        NLLW_ * F.cross_entropy(sl(lb).permute(0, 2, 1), x0)
    g1, = torch.autograd.grad(ref1, lb)
    v1, d1 = native.ctelbo_loss_window(lb.detach(), x0.int(), x_tilde.int(), qt0, qT, rate, EPS_, 1.0, 1.0, nll, off)
    err = (d1 - g1.float()).abs().max().item()
    print(f"one-pass S={S}: value {v1.item():.8g} vs fp64 {ref1.item():.10g}; max |d/dlogits - fp64| = {err:.3e} (bar {1e-3 * g1.abs().max().item():.3e})")
    np.testing.assert_allclose(v1.item(), ref1.item(), rtol=2e-5)
    assert err <= 1e-3 * g1.abs().max().item()


# ------------------------------------------------------------------------------------------------ 3: the loss on golden noise
CASES = ["g16b", "g256", "u3", "g32", "g16"]


class DeviceThetaToy:
    """The toy score function scaled by one trainable scalar, on the device process; records what it was called with."""

    def __init__(self, kind, S, t_func, theta):
        from oracle.toy_model import toy_logits
        self.process = _device_process(kind, S, t_func)
        self.S, self.device, self.f = S, torch.device("cuda"), toy_logits
        self.theta = torch.tensor(float(theta), device="cuda", requires_grad=True)
        self.calls = []

    def __call__(self, x, t, *a):
        self.calls.append(x.detach().clone())
        return self.f(x, t, self.S, 1.0) * self.theta

    def transition(self, t):
        return self.process.transition(t)

    def rate(self, t):
        return self.process.rate(t)


def _cfg(m, **loss_over):
    from config.mnist_config.config_tauUnet_mnist import get_config
    c = get_config()
    c.data.S, c.model.concat_dim = m["S"], m["D"]
    c.loss.update(name="CondCTElbo", eps_ratio=m["eps_ratio"], nll_weight=m["nll_weight"], min_time=m["min_time"],
                  one_forward_pass=m["one_forward_pass"], condition_dim=m["condition_dim"], **loss_over)
    return c


def _golden_case(golden, tag):
    g = golden("cond_losses")
    m = ast.literal_eval(str(g[f"{tag}__meta"]))
    return g, m, {k: T(g[f"{tag}__{k}"]) for k in ("x0", "ts", "x_t", "x_tilde")}


def _run_fixed(m, a, **loss_over):
    import lib.losses.losses as L
    import lib.losses.losses_utils as lu
    model = DeviceThetaToy(m["kind"], m["S"], m["t_func"], m["theta"])
    loss = lu.get_loss(_cfg(m, **loss_over))
    L._FIXED_NOISE = {"ts": a["ts"], "x_t": a["x_t"], "x_tilde": a["x_tilde"]}
    try:
        val = loss.calc_loss(a["x0"].cuda(), {"model": model, "n_iter": 0})
        grad, = torch.autograd.grad(val, model.theta)
    finally:
        L._FIXED_NOISE = None
    return model, val, grad


@pytest.mark.parametrize("tag", CASES)
def test_cond_ctelbo_on_golden_noise(golden, tag):
    from ctdd import native
    g, m, a = _golden_case(golden, tag)
    k, one = m["condition_dim"], m["one_forward_pass"]
    assert a["x_t"].shape == a["x_tilde"].shape == (m["B"], m["D"] - k)
    before = dict(native.LAUNCH_COUNTS)
    model, val, grad = _run_fixed(m, a)
    assert _delta(before) == {"ctdd_ctelbo_loss": 0, "ctdd_ctelbo_loss_terms": 0, "ctdd_ctelbo_loss_window": 1 if one else 2}
    # what reached the model: the conditioner as an exact prefix, then x~ (one pass) or x_t and x~ (two)
    x0 = a["x0"].cuda()
    want = [a["x_tilde"]] if one else [a["x_t"], a["x_tilde"]]
    assert len(model.calls) == len(want)
    for inp, suffix in zip(model.calls, want):
        assert inp.shape == x0.shape and torch.equal(inp[:, :k], x0[:, :k]) and torch.equal(inp[:, k:].cpu(), suffix.long())
    ref, ref64, g64 = float(g[f"{tag}__loss"]), float(g[f"{tag}__loss64"]), float(g[f"{tag}__grad64"])
    print(f"{tag}: loss {val.item():.8g} | reference {ref:.8g} | fp64 {ref64:.10g};  d/dtheta {grad.item():.6g} | fp64 {g64:.6g}")
    # the GPU builds q_{t|0} itself (K1): the bar of test_objective_matches_oracle_on_identical_noise against the reference's value
    np.testing.assert_allclose(val.item(), ref, rtol=3e-4, atol=1e-6)
    if tag != "g16":       # g16: |d/dtheta| = 2e-3, where torch's own fp32 autograd is 6.6e-3 off fp64 -- value only
        assert abs(g64) >= 0.1
        np.testing.assert_allclose(grad.item(), g64, rtol=2e-3, atol=1e-5 if one else 1e-4)
    # the torch-op path on the slices (cfg.loss.fused = False): no launch of K11, the same value
    before = dict(native.LAUNCH_COUNTS)
    model2, val2, _ = _run_fixed(m, a, fused=False)
    assert _delta(before) == {"ctdd_ctelbo_loss": 0, "ctdd_ctelbo_loss_terms": 0, "ctdd_ctelbo_loss_window": 0}
    assert all(torch.equal(p, q) for p, q in zip(model.calls, model2.calls))
    print(f"{tag}: fused {val.item():.8g} | torch ops {val2.item():.8g}")
    np.testing.assert_allclose(val2.item(), val.item(), rtol=2e-5)


def test_cond_ctelbo_accepts_both_argument_orders_and_images(golden):
    import lib.losses.losses as L
    import lib.losses.losses_utils as lu
    _, m, a = _golden_case(golden, "g16")
    model = DeviceThetaToy(m["kind"], m["S"], m["t_func"], m["theta"])
    loss = lu.get_loss(_cfg(m))
    x0 = a["x0"].cuda()
    L._FIXED_NOISE = {"ts": a["ts"], "x_t": a["x_t"], "x_tilde": a["x_tilde"]}
    try:
        state = {"model": model, "n_iter": 0}
        v = [loss.calc_loss(x0, state), loss.calc_loss(state, x0), loss.calc_loss(x0.view(m["B"], 1, 3, 4), state)]   # 4-D: row-major
    finally:
        L._FIXED_NOISE = None
    assert torch.equal(v[0], v[1]) and torch.equal(v[0], v[2])


# ------------------------------------------------------------------------------------------------ 4: HIP noising inside the loss
def test_hip_noising_inside_cond_loss(golden, monkeypatch):
    import lib.losses.losses as L
    import lib.losses.losses_utils as lu
    from oracle import ctmc_ops as ops, losses as ol
    from oracle.forward_process import ForwardProcess
    from oracle.toy_model import toy_logits
    _, m, a = _golden_case(golden, "g16b")
    S, k, nllw, theta = m["S"], m["condition_dim"], m["nll_weight"], m["theta"]
    assert not m["one_forward_pass"]
    model = DeviceThetaToy(m["kind"], S, m["t_func"], theta)
    loss = lu.get_loss(_cfg(m))
    x0 = a["x0"].cuda().repeat(64, 1)                             # bigger batch: tighter mean
    B, D = x0.shape
    vals = []
    for seed in range(6):
        torch.manual_seed(seed)
        model.calls.clear()
        v = loss.calc_loss(x0, {"model": model, "n_iter": 0})
        assert torch.isfinite(v) and v.requires_grad
        vals.append(v.item())
        for inp in model.calls:
            assert torch.equal(inp[:, :k], x0[:, :k]) and inp.min() >= 0 and inp.max() < S
    # the oracle's mean over its own draws (torch CPU RNG), same batch: the CT-ELBO of the free rows (oracle.losses.neg_ct_elbo on
    # the slices) + the cross entropy on the signal forward
    proc = ForwardProcess("gaussian", S, **GAUSS)
    x0c = x0.cpu()
    cond, data = x0c[:, :k], x0c[:, k:]
    d = D - k
    ovals = []
    for seed in range(6):
        torch.manual_seed(100 + seed)
        ts = torch.rand(B) * (1.0 - m["min_time"]) + m["min_time"]
        qt0, rate = proc.transition(ts), proc.rate(ts)
        x_t = ops.noise_xt(qt0, data, torch.empty(B * d, S).exponential_(1))
        _, _, xtl = ops.xtilde_sample(rate, x_t, torch.empty(B, d).exponential_(1), torch.empty(B, S).exponential_(1))
        l_reg = (toy_logits(torch.cat((cond, x_t), 1), ts, S, 1.0) * theta)[:, k:]
        l_sig = (toy_logits(torch.cat((cond, xtl), 1), ts, S, 1.0) * theta)[:, k:]
        ov = ol.neg_ct_elbo(l_reg, l_sig, data, x_t, xtl, qt0, rate, m["eps_ratio"]) + nllw * F.cross_entropy(l_sig.permute(0, 2, 1), data)
        ovals.append(ov.item())
    p, q = np.array(vals), np.array(ovals)
    se = np.sqrt(p.var(ddof=1) / len(p) + q.var(ddof=1) / len(q)) + 1e-9
    print(f"HIP noising: mean {p.mean():.6g} | oracle mean {q.mean():.6g} | se {se:.3g}")
    assert abs(p.mean() - q.mean()) < 6 * se + 0.02 * abs(q.mean()), (p, q)
    # ts pinned (the draws still come from the HIP kernels): x~ is x_t with exactly one free position changed
    monkeypatch.setattr(L, "_draw_ts", lambda B_, device, lo, hi: torch.full((B_,), 0.5, device=device))
    torch.manual_seed(7)
    model.calls.clear()
    loss.calc_loss(x0, {"model": model, "n_iter": 0})
    in_t, in_tilde = model.calls
    diff = in_t != in_tilde
    assert (diff.sum(1) == 1).all() and not diff[:, :k].any()
    assert (in_t[:, k:] != x0[:, k:]).any()                       # ... and x_t is noised


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


def _step(cfg, model, mb):
    from ctdd import native
    _, _, lu, tu, ou = _registries()
    state = {"model": model, "optimizer": ou.get_optimizer(model.parameters(), cfg), "n_iter": 0}
    w0 = [p.detach().clone() for p in model.parameters()]
    before = dict(native.LAUNCH_COUNTS)
    out = tu.get_train_step(cfg).step(state, lu.get_loss(cfg), mb)
    assert out.dim() == 0 and torch.isfinite(out) and float(out) < 1e8
    assert _delta(before) == {"ctdd_ctelbo_loss": 0, "ctdd_ctelbo_loss_terms": 0, "ctdd_ctelbo_loss_window": 1}
    assert sum(int(not torch.equal(p, q)) for p, q in zip(w0, model.parameters())) > 0


def test_conditional_mnist_config_trains_and_samples():
    mu, su, _, _, _ = _registries()
    from config.mnist_config.config_tauUnet_mnist_cond import get_config
    cfg = get_config()
    cfg.sampler.num_steps = 3
    torch.manual_seed(0)
    model = mu.create_model(cfg, torch.device("cuda"))
    _step(cfg, model, torch.randint(0, 256, (2, 1, 28, 28), device="cuda"))
    model.eval()
    cond = torch.randint(0, 256, (2, 392), generator=torch.Generator().manual_seed(3))
    sampler = su.get_sampler(cfg)
    sampler.seed = 11
    out = sampler.sample(model, 2, cond)
    out = np.asarray(out[0] if isinstance(out, tuple) else out)
    assert out.shape == (2, 784) and out.min() >= 0 and out.max() <= 255
    assert (out[:, :392] == cond.numpy()).all()
    model.train()


def test_masked_transformer_trains_with_cond_ctelbo():
    """A tiny UniVarMaskedEMA net with conditional_dim = condition_dim: it trains on its autograd module, the objective still
    runs in the window kernel."""
    mu = _registries()[0]
    from config.synthetic_config.config_masked_synthetic import get_config
    cfg = get_config()
    cfg.device = "cuda"
    cfg.data.shape = [16]
    cfg.model.update(embed_dim=16, qkv_dim=16, num_layers=1, num_heads=4, mlp_dim=16, concat_dim=16, num_output_ffresiduals=1,
                     conditional_dim=4)
    cfg.loss.update(name="CondCTElbo", condition_dim=4, one_forward_pass=True, nll_weight=0.01, min_time=0.01)
    torch.manual_seed(0)
    model = mu.create_model(cfg, torch.device("cuda"))
    _step(cfg, model, torch.randint(0, cfg.data.S, (6, 16), device="cuda"))
