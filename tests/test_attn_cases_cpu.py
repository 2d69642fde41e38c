"""CPU: the reference of the masked-attention GPU tests (tests/attn_cases.py), pinned before anything trusts it: the restated
masks against the ones the torch module builds, attention_fp64 against torch's scaled_dot_product_attention and against finite
differences of itself, and the visibility readback against the mask it was given."""
import pytest
import torch

import attn_cases as ac

DMAX = 70


def _config():
    from config.maze_config.config_hollow_maze import get_config
    cfg = get_config()
    cfg.device = "cpu"
    cfg.model.update(embed_dim=2 * DMAX + 2, qkv_dim=2 * DMAX + 2, num_heads=1, mlp_dim=4, num_layers=1, concat_dim=DMAX,
                     dropout_rate=0.0, attention_dropout_rate=0.0)
    return cfg


@pytest.fixture(scope="module")
def module_masks():
    """Tq -> (blocked of the l2r transformer, blocked of the r2l transformer, allow of the readout), as the module computes them:
    the additive masks handed to the first transformer block, and the support of the readout's softmax read off its output."""
    from lib.networks import hollow_networks as hn
    cfg = _config()
    E = cfg.model.embed_dim
    torch.manual_seed(0)
    nets = {d: hn.UniDirectionalTransformer(cfg, d).eval() for d in ("l2r", "r2l")}
    seen = {}
    for d, net in nets.items():
        net.trans_block_layers[0].register_forward_pre_hook(
            lambda mod, args, kwargs, d=d: seen.__setitem__(d, kwargs["masks"] if "masks" in kwargs else args[1]), with_kwargs=True)
    cross = hn.CrossAttention(cfg).eval()
    with torch.no_grad():                    # q = 0: uniform weights over the allowed keys; identity value / output maps: out = weights
        cross.dense_query.weight.zero_()
        for lin in (cross.dense_val, cross.out_linear):
            lin.weight.copy_(torch.eye(E))
            lin.bias.zero_()
    out = {}
    with torch.no_grad():
        for D in range(1, DMAX + 1):
            for d, net in nets.items():
                net(torch.zeros(1, D, E), torch.zeros(1, E))
            eye = torch.eye(2 * D + 1, E)                            # key j = e_j
            w = cross(eye[1:D + 1][None], eye[D + 1:][None], eye[0][None])[0]          # [D, E]
            assert float(w[:, 2 * D + 1:].abs().max()) == 0.0                      # (no weight outside the 2 D + 1 keys)
            out[D] = (seen["l2r"] == float("-inf"), seen["r2l"] == float("-inf"), w[:, :2 * D + 1] != 0)
    return out


@pytest.mark.parametrize("Tq", range(1, DMAX + 1))
def test_allowed_restates_the_modules_masks(module_masks, Tq):
    blocked_l2r, blocked_r2l, allow = module_masks[Tq]
    assert blocked_l2r.shape == blocked_r2l.shape == (Tq, Tq) and allow.shape == (Tq, 2 * Tq + 1)
    assert torch.equal(ac.allowed(0, Tq), ~blocked_l2r)
    assert torch.equal(ac.allowed(1, Tq), ~blocked_r2l)
    assert torch.equal(ac.allowed(2, Tq), allow)
    assert torch.equal(ac.allowed(2, Tq, 2 * Tq + 1), allow)
    assert bool(ac.allowed(3, Tq, Tq + 3).all()) and ac.allowed(3, Tq, Tq + 3).shape == (Tq, Tq + 3)
    assert torch.equal(ac.visible_counts(2, Tq), allow.sum(-1))


def _operands(mode, Tq, hd, B=2, H=3, seed=0):
    g = torch.Generator().manual_seed(seed)
    Tk = ac.n_keys(mode, Tq)
    return [torch.randn((B, H, T, hd), generator=g, dtype=torch.float64) for T in (Tq, Tk, Tk)]


@pytest.mark.parametrize("mode", ac.MODES)
@pytest.mark.parametrize("Tq,hd", [(1, 8), (7, 4), (33, 16), (70, 32)])
def test_reference_without_dropout_is_scaled_dot_product_attention(mode, Tq, hd):
    q, k, v = _operands(mode, Tq, hd, seed=mode + Tq)
    out, lse = ac.attention_fp64(q, k, v, mode)
    ok = ac.allowed(mode, Tq)
    ref = torch.nn.functional.scaled_dot_product_attention(q, k, v, attn_mask=ok)
    assert out.dtype == torch.float64 and float((out - ref).abs().max()) < 1e-13
    s = ((q @ k.transpose(-1, -2)) / hd ** 0.5).masked_fill(~ok, float("-inf"))
    assert float((lse - torch.log(torch.exp(s).sum(-1))).abs().max()) < 1e-12


@pytest.mark.parametrize("mode", ac.MODES)
@pytest.mark.parametrize("Tq,hd", [(1, 4), (5, 4), (9, 8)])
def test_reference_with_a_keep_mask_has_the_gradients_of_its_finite_differences(mode, Tq, hd):
    """O = (softmax(s) keep / (1 - p)) v with the normaliser over ALL visible keys: autograd's dq, dk, dv against central
    differences of the weighted output along random directions, in fp64."""
    B, H, p = 2, 2, 0.25
    g = torch.Generator().manual_seed(11 * mode + Tq)
    q, k, v = _operands(mode, Tq, hd, B, H, seed=3 + mode + Tq)
    Tk = k.shape[2]
    keep = torch.rand((B, H, Tq, Tk), generator=g) >= p
    wgt = torch.randn(q.shape, generator=g, dtype=torch.float64)
    f = lambda q_, k_, v_: (ac.attention_fp64(q_, k_, v_, mode, keep, 1 / (1 - p))[0] * wgt).sum()
    ins = [t.clone().requires_grad_(True) for t in (q, k, v)]
    f(*ins).backward()
    # the dropped probabilities still count in the normaliser: a row's kept weights sum to (kept mass) / (1 - p), not to one
    pr = torch.softmax(((q @ k.transpose(-1, -2)) / hd ** 0.5).masked_fill(~ac.allowed(mode, Tq), float("-inf")), -1)
    out = ac.attention_fp64(q, k, torch.ones_like(v), mode, keep, 1 / (1 - p))[0]
    assert float((out[..., 0] - (pr * keep).sum(-1) / (1 - p)).abs().max()) < 1e-13
    eps = 1e-6
    for n, t in enumerate(ins):
        d = torch.randn(t.shape, generator=g, dtype=torch.float64)
        plus = [x.detach() + (eps * d if m == n else 0) for m, x in enumerate(ins)]
        minus = [x.detach() - (eps * d if m == n else 0) for m, x in enumerate(ins)]
        fd = float(f(*plus) - f(*minus)) / (2 * eps)
        an = float((t.grad * d).sum())
        assert abs(fd - an) < 1e-7 * max(1.0, abs(an)), (n, fd, an)


@pytest.mark.parametrize("mode", ac.MODES)
@pytest.mark.parametrize("Tq,hd", [(1, 4), (7, 4), (33, 16), (40, 8)])
def test_readback_decodes_the_mask_it_was_given(mode, Tq, hd):
    """The decoders on attention_fp64's own output and autograd's own dV: exactly allowed (one call, batch = block) and exactly
    allowed & keep (one call per block), values 1 / n_i and 1 / (n_i (1 - p))."""
    H, B, p = 2, 3, 0.25
    Tk = ac.n_keys(mode, Tq)
    ok = ac.allowed(mode, Tq)
    n = ok.sum(-1).double()
    keep = torch.rand((B, H, Tq, Tk), generator=torch.Generator().manual_seed(mode + Tq)) >= p

    def fwd(kp):
        return lambda q, k, v: ac.attention_fp64(q.double(), k.double(), v.double(), mode, kp, 1.0 if kp is None else 1 / (1 - p))[0]

    def bwd(kp):
        def run(q, k, v, d_out):
            v = v.double().requires_grad_(True)
            out = ac.attention_fp64(q.double(), k.double(), v, mode, kp, 1.0 if kp is None else 1 / (1 - p))[0]
            return torch.autograd.grad(out, v, d_out.double())[0]
        return run

    for reader, make in ((ac.read_visibility, fwd), (ac.read_visibility_bwd, bwd)):
        pat, vals = reader(make(None), mode, Tq, hd, H)
        assert pat.shape == (H, Tq, Tk) and torch.equal(pat, ok.expand(H, Tq, Tk))
        assert float((vals - ok / n[:, None]).abs().max()) < 1e-15
        pat, vals = reader(make(keep), mode, Tq, hd, H, B=B)
        assert pat.shape == (B, H, Tq, Tk) and torch.equal(pat, ok & keep)
        assert float((vals - (ok & keep) / n[:, None] / (1 - p)).abs().max()) < 1e-15
    # a reader must not return what it is told: a forward with another mask reads as that other mask
    other = (mode + 1) % 2
    if mode < 2 and Tq > 1:
        pat, _ = ac.read_visibility(lambda q, k, v: ac.attention_fp64(q.double(), k.double(), v.double(), other)[0], mode, Tq, hd, H)
        assert torch.equal(pat, ac.allowed(other, Tq).expand(H, Tq, Tk)) and not torch.equal(pat, ok.expand(H, Tq, Tk))


def test_bf16_log_sum_exp_bar_is_four_times_the_measured_rounding_effect():
    """The matrix-core kernels' log-sum-exp bar (test_gpu_attention_fp64.py) is derived from the reference alone: the largest
    deviation rounding the operands to bf16 causes over the numeric cases, 8.123e-3, times four = 3.249e-2."""
    measured = ac.bf16_lse_deviation()
    assert abs(measured - ac.BF16_LSE_DEVIATION) < 1e-3 * ac.BF16_LSE_DEVIATION, measured
    assert ac.BF16_LSE_BAR == 4 * ac.BF16_LSE_DEVIATION


def test_operand_layouts_round_trip():
    B, H, Tq, hd = 2, 3, 5, 4
    for mode in ac.MODES:
        q, k, v = _operands(mode, Tq, hd, B, H)
        ops = ac.engine_operands(q, k, v, mode, device="cpu")
        E = H * hd
        if mode == 2:
            assert [tuple(t.shape) for t in ops] == [(B * Tq, E), (B * (2 * Tq + 1), E), (B * (2 * Tq + 1), E)]
            back = ac.split_gradients(tuple(ops), B, H)
        else:
            assert [tuple(t.shape) for t in ops] == [(B * Tq, 3 * E)]
            back = ac.split_gradients((ops[0], None, None), B, H)
        for t, r in zip((q, k, v), back):
            assert torch.equal(t.float(), r)
        # row (b, i), columns h hd .. of the engine's rows hold q[b, h, i]
        assert torch.equal(ops[0][1 * Tq + 2, 2 * hd:3 * hd], q[1, 2, 2].float())
