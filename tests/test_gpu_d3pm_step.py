"""GPU: ctdd_d3pm_step (csrc/d3pm.hip) against fp64: the model logits within the fp32 logit bar (atol 1e-4), and the Gumbel-max
draw equal to the fp64 argmax of model + gumbel on every row whose fp64 top-two gap is at least 1e-3.  For Gumbel-max that gap is
stochastically no smaller than Exp(1), so at most ~0.1 % of rows fall below it for any logits; rows below are skipped and at
most 1 % may be (every case has >= 2000 rows)."""
import math

import pytest
import torch

import d3pm_cases as dc

pytestmark = pytest.mark.gpu
GAP, MAX_SKIP = 1e-3, 0.01


def _setup(case):
    import lib.d3pm as d3pm
    S, bands, kind, _, D, T = case
    N = math.ceil(2000 / D)
    dif = d3pm.make_diffusion(dc.spec(kind, bands, S, T, device="cuda"))
    g = torch.Generator().manual_seed(2000 + S + (100 if kind == "absorbing" else 0))
    logits = (2.0 * torch.randn((N, D, S), generator=g)).cuda().contiguous()
    x = torch.randint(0, S, (N, D), generator=g).cuda()
    noise = torch.rand((N, D, S), generator=g).cuda().contiguous()
    return dif, logits, x, noise, N, D, S, T


def _step(dif, logits, x, t, **kw):
    from ctdd import native
    t1 = max(t - 1, 0)
    return native.d3pm_step(logits, x.int().contiguous(), dif.q_mats[t1], dif.q_mats_T[t1], dif.transpose_q_onestep_mats[t], t, dif.eps, **kw)


def _check_draw(out, model64, u, t):
    """out against argmax_s(model + gumbel(u)) in fp64 where the top two are >= GAP apart."""
    v = model64
    if t != 0:
        u = torch.clamp(u, min=torch.finfo(torch.float32).tiny, max=1.0).double()
        v = v - torch.log(-torch.log(u))
    top = torch.topk(v, 2, dim=-1)
    decided = (top.values[..., 0] - top.values[..., 1]) >= GAP
    assert float((~decided).float().mean()) <= MAX_SKIP
    assert torch.equal(out.long()[decided], top.indices[..., 0][decided])


@pytest.mark.parametrize("tsel", ["0", "1", "T-1"])
@pytest.mark.parametrize("case", dc.GPU_CASES, ids=dc.GPU_IDS)
def test_step_logits_and_draws(case, tsel):
    from ctdd import native
    dif, logits, x, noise, N, D, S, T = _setup(case)
    t = {"0": 0, "1": 1, "T-1": T - 1}[tsel]
    tb = torch.full((N,), t, dtype=torch.int64, device="cuda")
    model64, _ = dc.model_logits_f64(dif, logits, x, tb)
    n0 = native.LAUNCH_COUNTS.get("ctdd_d3pm_step", 0)
    out, model = _step(dif, logits, x, t, noise=noise, want_logits=True)
    assert native.LAUNCH_COUNTS["ctdd_d3pm_step"] == n0 + 1
    assert out.shape == (N, D) and int(out.min()) >= 0 and int(out.max()) < S
    err = float((model.double() - model64).abs().max())
    print(f"S={S} {case[2]} t={t}: model logits max abs err {err:.3e}")
    assert err <= 1e-4
    _check_draw(out, model64, noise, t)
    if t == 0:
        assert torch.equal(model, logits)
    # the rows' own Philox streams, replayed
    out_p = _step(dif, logits, x, t, seed=77, offset=t)
    u = native.philox_uniform(77, t, N * D, (S + 3) // 4, logits.device)[:, :S].reshape(N, D, S)
    assert int(out_p.min()) >= 0 and int(out_p.max()) < S
    _check_draw(out_p, model64, u, t)
    assert torch.equal(out_p, _step(dif, logits, x, t, seed=77, offset=t))
    # against the torch-op p_sample with the same uniforms (fp32 on both sides: the same rows decided)
    ref, _ = dc_fallback(dif).p_sample(lambda xx, tt: logits, x=x, t=tb, noise=noise)
    assert float((ref != out.long()).float().mean()) <= MAX_SKIP


def dc_fallback(dif):
    import copy
    d = copy.copy(dif)
    d.fused = False
    return d


def test_absorbing_starts_from_the_absorbing_state_and_loop_counts_steps():
    import lib.d3pm as d3pm
    from ctdd import native
    S, T = 16, 12
    dif = d3pm.make_diffusion(dc.spec("absorbing", None, S, T, device="cuda"))
    net = dc.ToyNet(S, T).cuda().eval()
    n0 = native.LAUNCH_COUNTS.get("ctdd_d3pm_step", 0)
    torch.manual_seed(4)
    x_init, x = dif.p_sample_loop(net, (6, 9), 5, return_x_init=True)
    assert native.LAUNCH_COUNTS["ctdd_d3pm_step"] == n0 + 5
    assert bool((x_init == S // 2).all()) and x.shape == (6, 9) and int(x.min()) >= 0 and int(x.max()) < S
    torch.manual_seed(4)
    assert torch.equal(x, dif.p_sample_loop(net, (6, 9), 5))
    uni = d3pm.make_diffusion(dc.spec("uniform", None, S, T, device="cuda"))
    xi, xe = uni.p_sample_loop(net, (3, 1, 2, 4), 3, return_x_init=True)                   # image-shaped states
    assert xe.shape == (3, 1, 2, 4) and len(torch.unique(xi)) > 1 and int(xe.max()) < S


class HookNet(dc.ToyNet):
    """ToyNet with the engine's sampler hooks: records what p_sample_loop sets around each forward."""
    _engine_int32_states = True

    def __init__(self, S, T):
        super().__init__(S, T)
        self.seen = []

    def engine_time_table(self, times):
        return times.to(torch.float32).view(-1, 1) + 0.25            # row n stands for times[n]

    def forward(self, x, t):
        row = getattr(self, "_engine_time_row", None)
        self.seen.append((float(t[0]), None if row is None else float(row[0]), bool(getattr(self, "_borrow_engine_output", False)),
                          bool(getattr(self, "_engine_uniform_time", False)), x.dtype))
        return super().forward(x, t)


def test_fused_loop_is_the_step_by_step_chain():
    """p_sample_loop on the fused path against the same chain written out: table indices, Philox offsets, the time handed to
    the network, the time-table row of each step, and the engine hooks set only inside the loop."""
    import lib.d3pm as d3pm
    S, T, steps, shape = 16, 12, 5, (6, 9)
    dif = d3pm.make_diffusion(dc.spec("uniform", 2, S, T, device="cuda"))
    net = HookNet(S, T).cuda().eval()
    torch.manual_seed(21)
    x_init, x_end = dif.p_sample_loop(net, shape, steps, return_x_init=True)
    assert [s[0] for s in net.seen] == [4.0, 3.0, 2.0, 1.0, 0.0]
    assert [s[1] for s in net.seen] == [t + 0.25 for t in (4.0, 3.0, 2.0, 1.0, 0.0)]
    assert all(s[2] and s[3] and s[4] == torch.int32 for s in net.seen)
    assert getattr(net, "_engine_time_row", None) is None and not getattr(net, "_borrow_engine_output", False)
    torch.manual_seed(21)
    x = dif._x_init(shape, torch.device("cuda"))
    seed = d3pm._seed()
    assert torch.equal(x, x_init)
    plain = dc.ToyNet(S, T).cuda().eval()
    for i in reversed(range(steps)):
        tb = torch.full((shape[0],), float(i), device="cuda")
        x = _step(dif, plain(x, tb).contiguous(), x, i, seed=seed, offset=i).long()
    assert torch.equal(x, x_end.long())
