"""GPU: training under arbitrary per-sample masks -- K11 on a per-sample set of free rows (ctdd_ctelbo_loss_masked), the masked
x~ draw (ctdd_xtilde_sample_masked) and the InpaintCTElbo loss on them.
1. the masked entry under an all-free mask against the dense entry and under a prefix mask against the window entry: value,
   gradient, exact zeros on held rows, nothing written outside the gradient buffer, logits untouched -- every kernel family;
2. ragged masks (a single free row, a fully held sample, a whole held row group, both ends in both roles) against the
   per-sample composition of oracle.losses.neg_ct_elbo on the gathered free rows in fp64, one-pass and two-pass;
3. refusals before any launch;
4. the masked x~ draw: all-free = the unmasked draw bit for bit, planted noise, a fully held sample, the law of the dimension;
5. InpaintCTElbo with a prefix mask on the noise the reference drew (tests/golden/cond_losses.npz);
6. the HIP noising inside the loss under a ragged mask;
7. the inpainting MNIST config end to end on the U-Net training plan, and the x0-prediction transformer on the HIP encoder."""
import ast
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

T = torch.from_numpy
GAUSS = dict(rate_sigma=6.0, Q_sigma=512.0, time_exp=100.0, time_base=3.0)
KEYS = ("ctdd_ctelbo_loss", "ctdd_ctelbo_loss_terms", "ctdd_ctelbo_loss_window", "ctdd_ctelbo_loss_masked")
ONLY_MASKED = lambda n: {"ctdd_ctelbo_loss": 0, "ctdd_ctelbo_loss_terms": 0, "ctdd_ctelbo_loss_window": 0, "ctdd_ctelbo_loss_masked": n}


def _device_process(kind, S, t_func="sqrt_cos"):
    from ctdd.process import DeviceForwardProcess
    return DeviceForwardProcess(kind, S, "cuda", **(GAUSS if kind == "gaussian" else dict(rate_const=1.7, t_func=t_func)))


def _delta(before):
    from ctdd import native
    return {k: native.LAUNCH_COUNTS.get(k, 0) - before.get(k, 0) for k in KEYS}


# ------------------------------------------------------------------------------------------------ 1 / 2 / 3: the kernel
#          S    B  D       the kernel families and tile edges of SHAPES in test_gpu_cond_loss.py
SHAPES = [(256, 3, 21),           # wave path: 16 rows per workgroup, plus tail
          (256, 2, 140),          # crosses the 128-row GEMM tile
          (32, 2, 140),           # thread-per-state + GEMM
          (96, 2, 12),            # thread-per-state + GEMM
          (37, 4, 20),            # FMA path, tail of the 8-row workgroup
          (3, 5, 15),             # FMA path, S < a wave
          (16, 3, 6)]             # fewer rows than one workgroup
W_, NLLW_, EPS_ = 0.7, 0.3, 1e-9
GUARD = 1024                      # floats of sentinel on either side of the gradient buffer


def _mask(kind, S, B, D):
    """(B, D) bool on the device, True = free."""
    free = torch.ones(B, D, dtype=torch.bool)
    if kind == "prefix":
        free[:, :max(1, D // 3)] = False
    elif kind == "ragged":
        gen = torch.Generator().manual_seed(S + 7 * D)
        free = torch.rand(B, D, generator=gen) < 0.6
        g = 16 if S == 256 else 8                         # rows of one workgroup of the row passes
        free[0] = False
        free[0, D - 1] = True                             # one free row (the last): every full row group before it is held, row 0 too
        free[1, 0], free[1, D - 1] = True, False          # ... and the two ends the other way round
        if D >= 3 * g:
            free[1, g:2 * g] = False                      # a held group between live ones
        if B >= 3:
            free[2] = False                               # nothing free
        assert D <= g or not free[0, :g].any()
    else:
        assert kind == "all"
    return free.cuda()


def _inputs(S, B, D):
    gen = torch.Generator().manual_seed(S * 1000 + D * 10)
    # (the S = 256 Gaussian tables on fewer states put q(x0 -> x_t) below fp32 resolution for random pairs: uniform rates there)
    proc = _device_process("gaussian" if S == 256 else "uniform", S)
    ts = (torch.rand(B, generator=gen) * 0.9 + 0.05).cuda()
    qt0, qT, rate, _ = proc.tables(ts, want_qt0=True, want_qt0T=True, want_rate=True)
    x0 = torch.randint(0, S, (B, D), generator=gen).cuda()
    x_t = torch.randint(0, S, (B, D), generator=gen).cuda()
    la = torch.randn(B, D, S, generator=gen).cuda()
    lb = torch.randn(B, D, S, generator=gen).cuda()
    return qt0, qT, rate, x0, x_t, la, lb


def _states(x0, x_t, free, S):
    """Full-shape x_t / x~ as the loss builds them: x0 on held entries; x~ = x_t with the first free entry of every sample moved."""
    x_t = torch.where(free, x_t, x0)
    x_tilde = x_t.clone()
    for b in range(free.shape[0]):
        idx = free[b].nonzero().view(-1)
        if idx.numel():
            d = idx[min(1, idx.numel() - 1)]
            x_tilde[b, d] = (x_tilde[b, d] + 1) % S
    return x_t, x_tilde


def _guarded(B, D, S):
    """A NaN-filled (B, D, S) gradient buffer inside a larger allocation of sentinels."""
    buf = torch.full((B * D * S + 2 * GUARD,), 777.0, device="cuda")
    grad = buf[GUARD:GUARD + B * D * S].view(B, D, S)
    grad.fill_(float("nan"))
    return buf, grad


def _weights(weights, nll, x_t, x_tilde):
    return {"one_pass": (1.0, 1.0, nll, x_tilde), "reg_half": (0.0, W_, 0.0, x_t), "sig_half": (W_, 0.0, nll, x_tilde)}[weights]


@pytest.mark.parametrize("weights", ["one_pass", "reg_half", "sig_half"])
@pytest.mark.parametrize("kind", ["all", "prefix"])
@pytest.mark.parametrize("S,B,D", SHAPES)
def test_masked_entry_is_the_dense_and_the_window_entry(S, B, D, kind, weights):
    """The per-row fp32 arithmetic is that of the existing entries (base_sum included: free rows are summed in rank order); only
    the fp64 sums over rows run in another order: value rtol 1e-6, gradient within 1e-6 of its largest magnitude."""
    from ctdd import native
    qt0, qT, rate, x0, x_t, la, _ = _inputs(S, B, D)
    free = _mask(kind, S, B, D)
    off = int((~free[0]).sum())
    x_t, x_tilde = _states(x0, x_t, free, S)
    sig, reg, nll, xs = _weights(weights, NLLW_ / (B * (D - off)), x_t, x_tilde)
    keep = la.clone()
    buf, grad = _guarded(B, D, S)
    before = dict(native.LAUNCH_COUNTS)
    val, got = native.ctelbo_loss_masked(la, x0.int(), xs.int(), free, qt0, qT, rate, EPS_, sig, reg, nll, grad_out=grad)
    assert _delta(before) == ONLY_MASKED(1)
    assert got.data_ptr() == grad.data_ptr() and got.shape == (B, D, S)
    if kind == "all":
        dval, dgrad = native.ctelbo_loss(la, x0.int(), xs.int(), qt0, qT, rate, EPS_, sig, nll, reg_scale=reg)
    else:
        dval, dgrad = native.ctelbo_loss_window(la, x0[:, off:].int().contiguous(), xs[:, off:].int().contiguous(), qt0, qT, rate, EPS_,
                                                sig, reg, nll, off)
    torch.cuda.synchronize()
    assert torch.equal(la, keep)                                             # the logits are read in place, never written
    assert torch.isfinite(dval) and torch.isfinite(dgrad).all() and dgrad.abs().max().item() > 0
    scale = dgrad.abs().max().item()
    err = (got - dgrad).abs().max().item()
    print(f"S={S} {kind} {weights}: value {val.item():.9g} vs {dval.item():.9g}; max |grad diff| {err:.3e} (bar {1e-6 * scale:.3e})")
    np.testing.assert_allclose(val.item(), dval.item(), rtol=1e-6)
    assert err <= 1e-6 * scale
    assert (got[~free] == 0).all()                                           # (NaN before the call: every held element was written)
    assert torch.isfinite(got).all()
    assert (buf[:GUARD] == 777.0).all() and (buf[-GUARD:] == 777.0).all()    # nothing before or past the buffer
    val2, got2 = native.ctelbo_loss_masked(la, x0.int(), xs.int(), free.to(torch.uint8), qt0, qT, rate, EPS_, sig, reg, nll)
    assert torch.equal(val2, val) and torch.equal(got2, got)                 # a fresh gradient tensor, a uint8 mask: the same


def _ref_objective(l_reg, l_sig, x0, reg_x, x_tilde, free, qt0, rate, w, nllw):
    """The per-sample composition in fp64 on the host: w * neg_ct_elbo of sample b alone on its gathered free rows (B = 1,
    D = n_b), averaged over ALL samples, + nllw * (cross entropy summed over free rows) / (number of free rows)."""
    from oracle import losses as ol
    B = x0.shape[0]
    total, ce = torch.zeros((), dtype=torch.float64), torch.zeros((), dtype=torch.float64)
    for b in range(B):
        idx = free[b].nonzero().view(-1)
        if idx.numel() == 0:
            continue
        g = lambda t: t[b:b + 1][:, idx]
        total = total + ol.neg_ct_elbo(g(l_reg), g(l_sig), g(x0), g(reg_x), g(x_tilde), qt0[b:b + 1], rate[b:b + 1], EPS_)
        ce = ce + F.cross_entropy(l_sig[b, idx], x0[b, idx], reduction="sum")
    return w * total / B + nllw * ce / max(int(free.sum()), 1)


@functools.lru_cache(maxsize=None)
def _ragged_case(S, B, D):
    """Inputs and the fp64 references (values, per-element gradients) of one shape, computed once."""
    qt0, qT, rate, x0, x_t, la, lb = _inputs(S, B, D)
    free = _mask("ragged", S, B, D)
    x_t, x_tilde = _states(x0, x_t, free, S)
    c = lambda t: t.detach().cpu()
    a64, b64 = c(la).double().requires_grad_(), c(lb).double().requires_grad_()
    args = (c(free), c(qt0).double(), c(rate).double())
    two = _ref_objective(a64, b64, c(x0), c(x_t), c(x_tilde), *args, W_, NLLW_)
    ga, gb = torch.autograd.grad(two, (a64, b64))
    one = _ref_objective(b64, b64, c(x0), c(x_tilde), c(x_tilde), *args, 1.0, NLLW_)
    g1, = torch.autograd.grad(one, b64)
    ref = dict(two=two.item(), ga=ga.float().cuda(), gb=gb.float().cuda(), one=one.item(), g1=g1.float().cuda())
    return (qt0, qT, rate, x0, x_t, x_tilde, la, lb, free), ref


@pytest.mark.parametrize("S,B,D", SHAPES)
def test_masked_entry_against_fp64_on_ragged_masks(S, B, D):
    """The bars of test_window_entry_against_fp64: value rtol 2e-5, gradient error <= 1e-3 of the largest reference gradient."""
    from ctdd import native
    (qt0, qT, rate, x0, x_t, x_tilde, la, lb, free), ref = _ragged_case(S, B, D)
    n_free = int(free.sum())
    assert int(free[0].sum()) == 1 and (B < 3 or not free[2].any()) and free[1, 0] and not free[0, 0] and free[0, D - 1] and not free[1, D - 1]
    nll = NLLW_ / n_free
    keep = (la.clone(), lb.clone())
    bufs = [_guarded(B, D, S) for _ in range(3)]
    before = dict(native.LAUNCH_COUNTS)
    va, da = native.ctelbo_loss_masked(la, x0.int(), x_t.int(), free, qt0, qT, rate, EPS_, 0.0, W_, 0.0, grad_out=bufs[0][1])
    vb, db = native.ctelbo_loss_masked(lb, x0.int(), x_tilde.int(), free, qt0, qT, rate, EPS_, W_, 0.0, nll, grad_out=bufs[1][1])
    v1, d1 = native.ctelbo_loss_masked(lb, x0.int(), x_tilde.int(), free, qt0, qT, rate, EPS_, 1.0, 1.0, nll, grad_out=bufs[2][1])
    torch.cuda.synchronize()
    assert _delta(before) == ONLY_MASKED(3)
    assert torch.equal(la, keep[0]) and torch.equal(lb, keep[1])
    print(f"two-pass S={S}: value {(va + vb).item():.8g} vs fp64 {ref['two']:.10g}")
    print(f"one-pass S={S}: value {v1.item():.8g} vs fp64 {ref['one']:.10g}")
    for got, want in ((da, ref["ga"]), (db, ref["gb"]), (d1, ref["g1"])):
        assert torch.isfinite(got).all()                                     # ... the fully held sample included
        assert (got[~free] == 0).all()
        if B >= 3:
            assert (got[2] == 0).all()
    for buf, _ in bufs:
        assert (buf[:GUARD] == 777.0).all() and (buf[-GUARD:] == 777.0).all()
    assert torch.isfinite(va) and torch.isfinite(vb) and torch.isfinite(v1)
    scale2 = max(ref["ga"].abs().max().item(), ref["gb"].abs().max().item())
    errs = [((da - ref["ga"]).abs().max().item(), scale2), ((db - ref["gb"]).abs().max().item(), scale2),
            ((d1 - ref["g1"]).abs().max().item(), ref["g1"].abs().max().item())]
    for err, scale in errs:
        print(f"  max |d/dlogits - fp64| = {err:.3e} (bar {1e-3 * scale:.3e})")
    np.testing.assert_allclose((va + vb).item(), ref["two"], rtol=2e-5)
    np.testing.assert_allclose(v1.item(), ref["one"], rtol=2e-5)
    for err, scale in errs:
        assert err <= 1e-3 * scale, (err, scale)


@pytest.mark.parametrize("bad", ["free_shape", "free_dtype", "x_shape", "S_257", "null_free", "null_logits", "null_grad"])
def test_masked_entry_refuses_before_any_launch(bad):
    from ctdd import native
    S, B, D = 16, 2, 10
    qt0, qT, rate, x0, x_t, la, _ = _inputs(S, B, D)
    free = _mask("prefix", S, B, D)
    x0i, xti = x0.int(), x_t.int()
    grad = torch.full_like(la, 5.0)
    lib = native.load()
    scratch = torch.empty(int(lib.ctdd_ctelbo_scratch_bytes(B, D, S)), dtype=torch.uint8, device="cuda")
    out = torch.zeros(1, device="cuda")
    p = lambda t: t.data_ptr()
    f8 = free.to(torch.uint8)
    before = dict(native.LAUNCH_COUNTS)

    def raw(logits=la, fr=f8, g=grad, s=S):
        return lib.ctdd_ctelbo_loss_masked(p(logits) if logits is not None else None, p(x0i), p(xti), p(fr) if fr is not None else None,
                                           p(qt0), p(qT), p(rate), B, D, s, EPS_, 1.0, 1.0, 0.0, p(scratch),
                                           p(g) if g is not None else None, p(out), torch.cuda.current_stream().cuda_stream)
    if bad in ("free_shape", "free_dtype", "x_shape"):                       # shapes and dtypes: the binding
        fr = {"free_shape": free[:, :D - 1].contiguous(), "free_dtype": free.int(), "x_shape": free}[bad]
        xt = xti[:, :D - 1].contiguous() if bad == "x_shape" else xti
        with pytest.raises(native.CtddError):
            native.ctelbo_loss_masked(la, x0i, xt, fr, qt0, qT, rate, EPS_, 1.0, 1.0, 0.0, grad_out=grad)
        assert _delta(before) == ONLY_MASKED(0)
    elif bad == "S_257":                                                     # ... the rest: the library itself
        big = torch.zeros(B, D, 257, device="cuda")
        tab = torch.zeros(B, 257, 257, device="cuda")
        with pytest.raises(native.CtddError):
            native.ctelbo_loss_masked(big, x0i, xti, free, tab, tab, tab, EPS_, 1.0, 1.0, 0.0)
        assert raw(s=257) != 0 and raw(s=1) != 0
    else:
        rc = {"null_free": lambda: raw(fr=None), "null_logits": lambda: raw(logits=None), "null_grad": lambda: raw(g=None)}[bad]()
        assert rc != 0
    torch.cuda.synchronize()
    assert (grad == 5.0).all() and out.item() == 0.0                         # refused before any launch


# ------------------------------------------------------------------------------------------------ 4: the masked x~ draw
def _rate(S, B, kind="uniform"):
    proc = _device_process(kind, S)
    ts = torch.linspace(0.2, 0.8, B).cuda()
    return proc.tables(ts, want_rate=True)[2]


@pytest.mark.parametrize("S,B,D", [(256, 3, 784), (5, 4, 300), (16, 2, 7)])
def test_xtilde_masked_all_free_is_the_unmasked_draw(S, B, D):
    from ctdd import native
    rate = _rate(S, B, "gaussian" if S == 256 else "uniform")
    x_t = torch.randint(0, S, (B, D), generator=torch.Generator().manual_seed(D)).int().cuda()
    free = torch.ones(B, D, dtype=torch.bool, device="cuda")
    before = dict(native.LAUNCH_COUNTS)
    for seed in (3, 2**40 + 17):
        want = native.xtilde_sample(rate, x_t, seed=seed, offset=5)
        got = native.xtilde_sample_masked(rate, x_t, free, seed=seed, offset=5)
        assert all(torch.equal(p, q) for p, q in zip(got, want))
    assert native.LAUNCH_COUNTS.get("ctdd_xtilde_sample_masked", 0) - before.get("ctdd_xtilde_sample_masked", 0) == 2
    gen = torch.Generator().manual_seed(1)
    E_dim, E_val = torch.empty(B, D).exponential_(1, generator=gen).cuda(), torch.empty(B, S).exponential_(1, generator=gen).cuda()
    want = native.xtilde_sample(rate, x_t, E_dim=E_dim, E_val=E_val)
    got = native.xtilde_sample_masked(rate, x_t, free.to(torch.uint8), E_dim=E_dim, E_val=E_val)
    assert all(torch.equal(p, q) for p, q in zip(got, want))
    with pytest.raises(native.CtddError):
        native.xtilde_sample_masked(rate, x_t, free[:, :D - 1].contiguous(), seed=1)


def test_xtilde_masked_planted_noise_and_a_held_sample():
    """The smallest E_dim (the race's winner without a mask) sits on a held dimension, the next smallest -- a thousand times
    larger, a thousand times smaller than every other -- on a chosen free one: that one moves, whatever the weights."""
    from ctdd import native
    from oracle import ctmc_ops as ops
    S, B, D = 7, 6, 300
    rate = _rate(S, B)
    gen = torch.Generator().manual_seed(4)
    x_t = torch.randint(0, S, (B, D), generator=gen).int()
    free = torch.rand(B, D, generator=gen) < 0.5
    free[B - 1] = False                                                       # the last sample holds everything
    E_dim = torch.empty(B, D).uniform_(1.0, 2.0, generator=gen)
    E_val = torch.empty(B, S).exponential_(1, generator=gen)
    planted = []
    for b in range(B - 1):
        held, fr = (~free[b]).nonzero().view(-1), free[b].nonzero().view(-1)
        h, f = held[b % held.numel()], fr[(3 * b) % fr.numel()]
        if b == 0:
            h, f, free[0, 0], free[0, D - 1] = 0, D - 1, False, True          # the two ends
        if b == 1:
            h, f, free[1, 0], free[1, D - 1] = D - 1, 0, True, False
        E_dim[b, h], E_dim[b, f] = 1e-9, 1e-6
        planted.append(int(f))
    dims, newval, xt = native.xtilde_sample_masked(rate, x_t.cuda(), free.cuda(), E_dim=E_dim.cuda(), E_val=E_val.cuda())
    dims, newval, xt = dims.cpu(), newval.cpu(), xt.cpu()
    assert dims[:B - 1].tolist() == planted and dims[B - 1].item() == -1
    assert torch.equal(xt[B - 1], x_t[B - 1])                                 # nothing free: x_t comes back
    for b in range(B - 1):
        d = planted[b]
        assert free[b, d] and xt[b, d] == newval[b] != x_t[b, d]
        off = torch.ones(D, dtype=torch.bool)
        off[d] = False
        assert torch.equal(xt[b, off], x_t[b, off])
        # the new value is the oracle's draw on the free rows alone (same E_val row)
        idx = free[b].nonzero().view(-1)
        od, ov, _ = ops.xtilde_sample(rate[b:b + 1].cpu(), x_t[b:b + 1, idx].long(), E_dim[b:b + 1, idx], E_val[b:b + 1])
        assert int(idx[od[0]]) == d and int(ov[0]) == int(newval[b])


@pytest.mark.parametrize("rates", ["uniform", "unequal"])
def test_xtilde_masked_law_of_the_dimension(rates):
    """4096 copies of one x_t (D = 6, S = 4, three free in unequal states; uniform rates, and a rate matrix whose states leave at
    unequal rates): each free dimension's pick frequency within 5 binomial standard errors of rs[x_d] / sum_free rs, held
    dimensions never."""
    from ctdd import native
    S, D, N = 4, 6, 4096
    if rates == "uniform":
        R = _rate(S, 1)[0].cpu()
    else:
        R = torch.tensor([[0.0, 1.0, 0.5, 0.5], [0.25, 0.0, 0.25, 0.5], [2.0, 1.0, 0.0, 1.0], [0.5, 0.5, 0.5, 0.0]])
        R = R - torch.diag(R.sum(1))                                          # rs = (2, 1, 4, 1.5)
    x = torch.tensor([2, 0, 1, 2, 3, 0])
    free = torch.tensor([False, True, True, False, True, False])             # free states 0, 1, 3 (unequal: rs 2, 1, 1.5)
    rate = R.view(1, S, S).contiguous().cuda()
    tidx = torch.zeros(N, dtype=torch.int32, device="cuda")
    dims, newval, xt = native.xtilde_sample_masked(rate, x.int().repeat(N, 1).cuda(), free.repeat(N, 1).cuda(), tidx=tidx, seed=99)
    dims, xt = dims.cpu().long(), xt.cpu().long()
    rs = -torch.diagonal(R)[x]
    want = torch.where(free, rs, torch.zeros(())) / rs[free].sum()
    freq = torch.bincount(dims, minlength=D).double() / N
    print("pick frequencies", freq.tolist(), "against", want.tolist())
    for d in range(D):
        if not free[d]:
            assert freq[d] == 0
        else:
            p = want[d].item()
            assert abs(freq[d].item() - p) <= 5 * (p * (1 - p) / N) ** 0.5, (d, freq[d].item(), p)
    moved = xt != x.view(1, D)
    assert (moved.sum(1) == 1).all() and moved[torch.arange(N), dims].all()


# ------------------------------------------------------------------------------------------------ 5: the loss on golden noise
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
    c.loss.update(name="InpaintCTElbo", mask="prefix", eps_ratio=m["eps_ratio"], nll_weight=m["nll_weight"], min_time=m["min_time"],
                  one_forward_pass=m["one_forward_pass"], condition_dim=m["condition_dim"], **loss_over)
    return c


def _golden_case(golden, tag):
    g = golden("cond_losses")
    m = ast.literal_eval(str(g[f"{tag}__meta"]))
    a = {k: T(g[f"{tag}__{k}"]) for k in ("x0", "ts", "x_t", "x_tilde")}
    k = m["condition_dim"]
    for key in ("x_t", "x_tilde"):                                           # the compact draws scattered behind the conditioner
        a[key + "_full"] = torch.cat((a["x0"][:, :k].long(), a[key].long()), dim=1)
    return g, m, a


def _run_fixed(m, a, **loss_over):
    import lib.losses.losses as L
    import lib.losses.losses_utils as lu
    model = DeviceThetaToy(m["kind"], m["S"], m["t_func"], m["theta"])
    loss = lu.get_loss(_cfg(m, **loss_over))
    L._FIXED_NOISE = {"ts": a["ts"], "x_t": a["x_t_full"], "x_tilde": a["x_tilde_full"]}
    try:
        val = loss.calc_loss(a["x0"].cuda(), {"model": model, "n_iter": 0})
        grad, = torch.autograd.grad(val, model.theta)
    finally:
        L._FIXED_NOISE = None
    return model, val, grad


@pytest.mark.parametrize("tag", CASES)
def test_inpaint_ctelbo_with_a_prefix_mask_on_golden_noise(golden, tag):
    """With mask = "prefix" the objective is CondCTElbo term for term: the reference's values, at the bars
    test_cond_ctelbo_on_golden_noise applies."""
    from ctdd import native
    g, m, a = _golden_case(golden, tag)
    k, one = m["condition_dim"], m["one_forward_pass"]
    before = dict(native.LAUNCH_COUNTS)
    model, val, grad = _run_fixed(m, a)
    assert _delta(before) == ONLY_MASKED(1 if one else 2)
    x0 = a["x0"].cuda()
    want = [a["x_tilde_full"]] if one else [a["x_t_full"], a["x_tilde_full"]]
    assert len(model.calls) == len(want)
    for inp, full in zip(model.calls, want):
        assert inp.shape == x0.shape and torch.equal(inp[:, :k], x0[:, :k]) and torch.equal(inp.cpu(), full)
    ref, ref64, g64 = float(g[f"{tag}__loss"]), float(g[f"{tag}__loss64"]), float(g[f"{tag}__grad64"])
    print(f"{tag}: loss {val.item():.8g} | reference {ref:.8g} | fp64 {ref64:.10g};  d/dtheta {grad.item():.6g} | fp64 {g64:.6g}")
    np.testing.assert_allclose(val.item(), ref, rtol=3e-4, atol=1e-6)
    if tag != "g16":       # g16: |d/dtheta| = 2e-3, where torch's own fp32 autograd is 6.6e-3 off fp64 -- value only
        assert abs(g64) >= 0.1
        np.testing.assert_allclose(grad.item(), g64, rtol=2e-3, atol=1e-5 if one else 1e-4)
    before = dict(native.LAUNCH_COUNTS)
    model2, val2, _ = _run_fixed(m, a, fused=False)
    assert _delta(before) == ONLY_MASKED(0)
    assert all(torch.equal(p, q) for p, q in zip(model.calls, model2.calls))
    print(f"{tag}: fused {val.item():.8g} | torch ops {val2.item():.8g}")
    np.testing.assert_allclose(val2.item(), val.item(), rtol=2e-5)


def test_inpaint_ctelbo_accepts_both_argument_orders_images_and_a_pinned_mask(golden):
    import lib.losses.losses as L
    import lib.losses.losses_utils as lu
    _, m, a = _golden_case(golden, "g16")
    model = DeviceThetaToy(m["kind"], m["S"], m["t_func"], m["theta"])
    loss = lu.get_loss(_cfg(m))
    x0 = a["x0"].cuda()
    free = torch.ones(m["B"], m["D"], dtype=torch.bool)
    free[:, :m["condition_dim"]] = False
    L._FIXED_NOISE = {"ts": a["ts"], "x_t": a["x_t_full"], "x_tilde": a["x_tilde_full"]}
    try:
        state = {"model": model, "n_iter": 0}
        v = [loss.calc_loss(x0, state), loss.calc_loss(state, x0), loss.calc_loss(x0.view(m["B"], 1, 3, 4), state)]   # 4-D: row-major
        L._FIXED_NOISE["free"] = free
        v.append(loss.calc_loss(x0, state))
        # a pinned ragged mask, fused against the torch-op path; the sample without a free entry adds nothing and nothing is NaN
        free = torch.rand(m["B"], m["D"], generator=torch.Generator().manual_seed(0)) < 0.5
        free[1] = False
        L._FIXED_NOISE["free"] = free
        model.calls.clear()
        r = loss.calc_loss(x0, state)
        g_r, = torch.autograd.grad(r, model.theta)
        assert all(torch.equal(inp[~free.cuda()], x0[~free.cuda()]) for inp in model.calls)
        loss2 = lu.get_loss(_cfg(m, fused=False))
        r2 = loss2.calc_loss(x0, state)
        g_r2, = torch.autograd.grad(r2, model.theta)
        L._FIXED_NOISE["free"] = free[:, :-1]
        with pytest.raises(ValueError):
            loss.calc_loss(x0, state)
    finally:
        L._FIXED_NOISE = None
    assert all(torch.equal(v[0], w) for w in v[1:])
    print(f"ragged pinned mask: fused {r.item():.8g} | torch ops {r2.item():.8g};  d/dtheta {g_r.item():.6g} | {g_r2.item():.6g}")
    assert torch.isfinite(r) and torch.isfinite(g_r)
    np.testing.assert_allclose(r2.item(), r.item(), rtol=2e-5)


# ------------------------------------------------------------------------------------------------ 6: HIP noising inside the loss
def test_hip_noising_inside_inpaint_loss(golden, monkeypatch):
    import lib.losses.losses as L
    import lib.losses.losses_utils as lu
    import lib.losses.masks as masks
    from oracle import ctmc_ops as ops, losses as ol
    from oracle.forward_process import ForwardProcess
    from oracle.toy_model import toy_logits
    _, m, a = _golden_case(golden, "g16b")
    S, nllw, theta = m["S"], m["nll_weight"], m["theta"]
    assert not m["one_forward_pass"]
    model = DeviceThetaToy(m["kind"], S, m["t_func"], theta)
    loss = lu.get_loss(_cfg(m))
    x0 = a["x0"].cuda().repeat(32, 1)                             # bigger batch: tighter mean
    B, D = x0.shape
    free = torch.rand(B, D, generator=torch.Generator().manual_seed(5)) < 0.5
    free[0], free[1] = False, False
    free[0, 0], free[1, D - 1] = True, True                       # single free entries at the two ends
    assert free.any(1).all()
    monkeypatch.setattr(masks, "sample_free", lambda cfg, B_, D_: free.clone())
    fd = free.cuda()
    vals = []
    for seed in range(6):
        torch.manual_seed(seed)
        model.calls.clear()
        v = loss.calc_loss(x0, {"model": model, "n_iter": 0})
        assert torch.isfinite(v) and v.requires_grad
        vals.append(v.item())
        in_t, in_tilde = model.calls
        for inp in (in_t, in_tilde):
            assert torch.equal(inp[~fd], x0[~fd]) and inp.min() >= 0 and inp.max() < S      # held entries reach the model bit for bit
        diff = in_t != in_tilde
        assert (diff.sum(1) == 1).all() and not diff[~fd].any()   # x~ is x_t with exactly one free position changed
        assert (in_t[fd] != x0[fd]).any()                         # ... and free entries are noised
    # the oracle's mean over its own draws (torch CPU RNG) of the same objective: x_t noised on free entries, x~ by the oracle's
    # draw on the gathered free rows of each sample, neg_ct_elbo per sample on them + the cross entropy on the signal forward
    proc = ForwardProcess("gaussian", S, **GAUSS)
    x0c = x0.cpu()
    ovals = []
    for seed in range(6):
        torch.manual_seed(100 + seed)
        ts = torch.rand(B) * (1.0 - m["min_time"]) + m["min_time"]
        qt0, rate = proc.transition(ts), proc.rate(ts)
        x_t = torch.where(free, ops.noise_xt(qt0, x0c, torch.empty(B * D, S).exponential_(1)), x0c)
        xtl = x_t.clone()
        for b in range(B):
            idx = free[b].nonzero().view(-1)
            _, _, xb = ops.xtilde_sample(rate[b:b + 1], x_t[b:b + 1, idx], torch.empty(1, idx.numel()).exponential_(1), torch.empty(1, S).exponential_(1))
            xtl[b, idx] = xb[0]
        l_reg = toy_logits(x_t, ts, S, 1.0) * theta
        l_sig = toy_logits(xtl, ts, S, 1.0) * theta
        tot, ce = 0.0, 0.0
        for b in range(B):
            idx = free[b].nonzero().view(-1)
            gth = lambda t: t[b:b + 1][:, idx]
            tot += ol.neg_ct_elbo(gth(l_reg), gth(l_sig), gth(x0c), gth(x_t), gth(xtl), qt0[b:b + 1], rate[b:b + 1], m["eps_ratio"]).item()
            ce += F.cross_entropy(l_sig[b, idx], x0c[b, idx], reduction="sum").item()
        ovals.append(tot / B + nllw * ce / int(free.sum()))
    p, q = np.array(vals), np.array(ovals)
    se = np.sqrt(p.var(ddof=1) / len(p) + q.var(ddof=1) / len(q)) + 1e-9
    print(f"HIP noising: mean {p.mean():.6g} | oracle mean {q.mean():.6g} | se {se:.3g}")
    assert abs(p.mean() - q.mean()) < 6 * se + 0.02 * abs(q.mean()), (p, q)


# ------------------------------------------------------------------------------------------------ 7: end to end
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
    assert _delta(before) == ONLY_MASKED(1)
    assert sum(int(not torch.equal(p, q)) for p, q in zip(w0, model.parameters())) > 0


def test_inpaint_mnist_config_trains_and_inpaints():
    mu, su, _, _, _ = _registries()
    from config.mnist_config.config_tauUnet_mnist_inpaint import get_config
    from ctdd.unet_engine import training_supported
    cfg = get_config()
    cfg.sampler.num_steps = 3
    torch.manual_seed(0)
    model = mu.create_model(cfg, torch.device("cuda"))
    assert training_supported(model)                              # the step below runs on the U-Net HIP training plan
    _step(cfg, model, torch.randint(0, 256, (2, 1, 28, 28), device="cuda"))
    assert model._engine is not None and getattr(model._engine, "_train_plans", None), "the training plan did not run"
    model.eval()
    x_known = torch.randint(0, 256, (2, 784), generator=torch.Generator().manual_seed(3))
    held = torch.ones(2, 28, 28, dtype=torch.bool)
    held[0, 5:19, 8:23] = False                                   # a free box in one sample, a held box in the other
    held[1] = ~held[0]
    held = held.view(2, 784)
    sampler = su.get_sampler(cfg)
    sampler.seed = 11
    out = sampler.inpaint(model, x_known, held)
    out = np.asarray(out[0] if isinstance(out, tuple) else out)
    assert out.shape == (2, 784) and out.min() >= 0 and out.max() < 256
    assert (out[held.numpy()] == x_known.numpy()[held.numpy()]).all()
    model.train()


def test_bert_hip_encoder_trains_with_bernoulli_masks():
    import importlib
    mu = _registries()[0]
    cfg = importlib.import_module("config.synthetic_config.config_bert_synthetic").get_config()
    cfg.device = "cuda"
    cfg.model.update(engine_train="hip-encoder")
    cfg.loss.update(name="InpaintCTElbo", mask="bernoulli", mask_rate=[0.2, 0.8])
    torch.manual_seed(0)
    model = mu.create_model(cfg, torch.device("cuda"))
    _step(cfg, model, torch.randint(0, cfg.data.S, (6, int(cfg.model.concat_dim)), device="cuda"))
    assert model._trainer is not None                             # the step ran on the HIP encoder
