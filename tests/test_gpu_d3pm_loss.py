"""GPU: ctdd_d3pm_loss (csrc/d3pm.hip) against an fp64 torch evaluation of its formulas (d3pm_cases.loss_f64).

Tolerance: the same inputs three ways -- fp64, the fp32 torch-op fallback on the device (d3pm_fused = False), the kernels.  The
kernels' error against fp64 may be at most twice the fallback's on the same inputs (both are fp32 and differ in summation
order only: GEMM chunks of 16, sums inside the wave), plus a floor of 4 fp32 ulps of the largest term.  Values are compared
relatively, the gradient as max-abs over the max-abs of the fp64 gradient.  Both errors are printed for every case."""
import pytest
import torch

import d3pm_cases as dc

pytestmark = pytest.mark.gpu
ULP = 2.0 ** -23
COEFF = 0.01


def _inputs(case, peaked):
    import lib.d3pm as d3pm
    S, bands, kind, B, D, T = case
    dev = torch.device("cuda")
    fused = d3pm.make_diffusion(dc.spec(kind, bands, S, T, loss_type="hybrid", device="cuda"))
    fall = d3pm.make_diffusion(dc.spec(kind, bands, S, T, loss_type="hybrid", device="cuda", d3pm_fused=False))
    g = torch.Generator().manual_seed(1000 + S + (7 if peaked else 0) + (100 if kind == "absorbing" else 0))
    x0 = torch.randint(0, S, (B, D), generator=g).to(dev)
    assert B >= 3
    t = torch.tensor(([0, 1, T - 1] + [T // 2] * B)[:B], dtype=torch.int64, device=dev)
    x_t = fall.q_sample(x0, t, torch.rand((B, D, S), generator=g).to(dev))
    if peaked:
        logits = 20.0 * torch.nn.functional.one_hot(torch.randint(0, S, (B, D), generator=g), S).float()
    else:
        logits = 2.0 * torch.randn((B, D, S), generator=g)
    return fused, fall, logits.to(dev).contiguous(), x0, x_t, t


def _three_ways(case, peaked):
    from ctdd import native
    fused, fall, logits, x0, x_t, t = _inputs(case, peaked)
    ref = dc.loss_f64(fall, logits, x0, x_t, t, 1.0, COEFF)
    lf = logits.clone().requires_grad_(True)
    net = lambda x, tt: lf
    vb_f, pred = fall.vb_terms_bpd(net, x_start=x0, x_t=x_t, t=t)
    ce_f = fall.cross_entropy_x_start(x0, pred)
    loss_f = vb_f + COEFF * ce_f
    grad_f, = torch.autograd.grad(loss_f.sum(), lf)
    qprev, qprevT, q1T = fused._tables(t)
    ker = native.d3pm_loss(logits, x0.int(), x_t.int(), t.int(), qprev, qprevT, q1T, fused.eps, 1.0, COEFF)
    torch.cuda.synchronize()
    return ref, (loss_f.detach(), vb_f.detach(), ce_f.detach(), grad_f), ker, (fused, logits, x0, x_t, t)


@pytest.mark.parametrize("peaked", [False, True], ids=["normal", "peaked"])
@pytest.mark.parametrize("case", dc.GPU_CASES, ids=dc.GPU_IDS)
def test_loss_and_gradient_against_fp64(case, peaked):
    ref, fb, ker, (fused, logits, x0, x_t, t) = _three_ways(case, peaked)
    for name, r, f, k in zip(("loss", "vb", "ce"), ref, fb, ker):
        ef = float(((f.double() - r).abs() / r.abs()).max())
        ek = float(((k.double() - r).abs() / r.abs()).max())
        print(f"S={case[0]} {case[2]} {'peaked' if peaked else 'normal'} {name}: fallback rel err {ef:.3e}  kernel rel err {ek:.3e}")
        bound = 2.0 * ef * r.abs() + 4.0 * ULP * r.abs().max()
        assert bool(((k.double() - r).abs() <= bound).all()), (name, ek, ef)
    gmax = float(ref[3].abs().max())
    ef = float((fb[3].double() - ref[3]).abs().max()) / gmax
    ek = float((ker[3].double() - ref[3]).abs().max()) / gmax
    print(f"S={case[0]} {case[2]} {'peaked' if peaked else 'normal'} grad: fallback err {ef:.3e}  kernel err {ek:.3e}  (over max |grad| {gmax:.3e})")
    assert ek <= 2.0 * ef + 4.0 * ULP, (ek, ef)
    # samples at t = 0: the decoder term and the cross entropy are both -log_softmax(l)[x0]
    S, D = case[0], case[4]
    w = (1.0 + COEFF) / (D * 0.6931471805599453)
    z = (t == 0)
    p = torch.softmax(logits[z].double(), -1)
    want = w * (p - torch.nn.functional.one_hot(x0[z], S).double())
    assert float((ker[3][z].double() - want).abs().max()) <= 16.0 * ULP * w


def test_value_only_form_matches_and_counts_launches():
    from ctdd import native
    case = dc.GPU_CASES[3]
    fused, fall, logits, x0, x_t, t = _inputs(case, False)
    net = lambda x, tt: logits
    n0 = native.LAUNCH_COUNTS.get("ctdd_d3pm_loss", 0)
    with torch.no_grad():
        vb, pred = fused.vb_terms_bpd(net, x_start=x0, x_t=x_t, t=t)
    assert native.LAUNCH_COUNTS["ctdd_d3pm_loss"] == n0 + 1 and pred.shape == logits.shape
    qprev, qprevT, q1T = fused._tables(t)
    full = native.d3pm_loss(logits, x0.int(), x_t.int(), t.int(), qprev, qprevT, q1T, fused.eps, 1.0, 0.0)
    assert torch.equal(vb, full[1]) and torch.equal(full[0], full[1])
    img = lambda v: v.reshape(v.shape[0], 1, 5, 8, *v.shape[2:])            # (B, C, H, W) states, x.shape + (S,) logits
    with torch.no_grad():
        vbi, predi = fused.vb_terms_bpd(lambda x, tt: img(logits), x_start=img(x0), x_t=img(x_t), t=t)
    assert torch.equal(vb, vbi) and predi.shape == (3, 1, 5, 8, 32)


class ThetaNet(torch.nn.Module):
    """toy logits scaled by one trainable parameter."""

    def __init__(self, S, T, dtype=torch.float32):
        super().__init__()
        self.S, self.T = S, T
        self.theta = torch.nn.Parameter(torch.tensor(1.3, dtype=dtype))

    def forward(self, x, t):
        from oracle.toy_model import toy_logits
        return toy_logits(x.reshape(x.shape[0], -1), t.to(torch.float32) / self.T, self.S).to(self.theta.dtype) * self.theta


@pytest.mark.parametrize("case", [dc.GPU_CASES[2], dc.GPU_CASES[3]], ids=["S16", "S32"])
def test_calc_loss_backward_reaches_the_parameter(case, monkeypatch):
    import lib.d3pm as d3pm
    from ctdd import native
    from lib.losses import losses
    S, bands, kind, B, D, T = case
    fused, fall, _, x0, x_t, t = _inputs(case, False)
    monkeypatch.setattr(d3pm, "_FIXED_NOISE", {"x_t": x_t})
    cfg = dc.ConfigDict()
    cfg.device = "cuda"
    cfg.model = dc.spec(kind, bands, S, T, loss_type="hybrid", device="cuda")
    grads = {}
    for name, dif in (("fused", fused), ("fallback", fall)):
        net = ThetaNet(S, T).cuda()
        n0 = native.LAUNCH_COUNTS.get("ctdd_d3pm_loss", 0)
        torch.manual_seed(5)
        val = losses.d3pm_loss(cfg, dif).calc_loss(x0, {"model": net})
        val.backward()
        assert native.LAUNCH_COUNTS.get("ctdd_d3pm_loss", 0) == n0 + (1 if name == "fused" else 0)
        assert torch.isfinite(val) and torch.isfinite(net.theta.grad)
        grads[name] = float(net.theta.grad)
    torch.manual_seed(5)
    tt = torch.randint(low=0, high=T, size=(B,)).cuda()
    net64 = ThetaNet(S, T, torch.float64).cuda()
    l64 = net64(x_t, tt)
    _, _, _, g64 = dc.loss_f64(fall, l64.detach(), x0, x_t, tt, 1.0, COEFF)
    want = float((g64 * (l64.detach() / 1.3)).sum() / B)
    ef, ek = abs(grads["fallback"] - want) / abs(want), abs(grads["fused"] - want) / abs(want)
    print(f"S={S} d loss / d theta: fp64 {want:.9e}  fallback rel err {ef:.3e}  kernel rel err {ek:.3e}")
    assert ek <= 2.0 * ef + 4.0 * ULP
