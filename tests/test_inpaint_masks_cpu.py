"""CPU: the mask distributions of InpaintCTElbo (lib/losses/masks.py) -- shape, dtype, at least one free entry, reproducibility
under torch.manual_seed, the geometry of each family, the bernoulli rate -- and the loss's registry entry, argument checks
(before any device work), entry points and shipped config."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIX = [["half", 1.0], ["box", 2.0], ["bernoulli", 1.0], ["prefix", 0.5]]


def _cfg(mask, shape=(1, 6, 6), **loss_over):
    from config.mnist_config.config_tauUnet_mnist import get_config
    c = get_config()
    D = 1
    for v in shape:
        D *= v
    c.data.S, c.data.shape, c.model.concat_dim = 5, list(shape), D
    c.loss.update(name="InpaintCTElbo", nll_weight=0.1, mask=mask, condition_dim=D // 3, mask_rate=[0.2, 0.6], mask_mixture=MIX)
    c.loss.update(**loss_over)
    return c, D


class NoDevice:
    """A model stand-in whose every use fails: the checks must raise before the loss touches it."""

    def __getattr__(self, k):
        raise AssertionError(f"model.{k} used before the arguments were checked")

    def __call__(self, *a, **k):
        raise AssertionError("model called before the arguments were checked")


NAMES = ["prefix", "bernoulli", "half", "box", "mixture"]


@pytest.mark.parametrize("name", NAMES)
def test_shape_dtype_free_entry_and_seed(name):
    from lib.losses.masks import sample_free
    cfg, D = _cfg(name)
    torch.manual_seed(5)
    draws = [sample_free(cfg, 8, D) for _ in range(200)]
    for free in draws:
        assert free.shape == (8, D) and free.dtype == torch.bool and free.device.type == "cpu" and free.is_contiguous()
        assert free.any(dim=1).all()                                   # at least one free entry in every sample
    torch.manual_seed(5)
    again = [sample_free(cfg, 8, D) for _ in range(200)]
    assert all(torch.equal(p, q) for p, q in zip(draws, again))        # the global CPU generator, nothing else
    if name != "prefix":
        assert any(not torch.equal(draws[0], d) for d in draws[1:])    # ... and they are draws
        assert not all(d.all() for d in draws)                         # something is held


def test_prefix_is_the_cond_ctelbo_split():
    from lib.losses.masks import sample_free
    cfg, D = _cfg("prefix", shape=(2, 3, 4), condition_dim=7)
    free = sample_free(cfg, 3, D)
    want = torch.zeros(D, dtype=torch.bool)
    want[7:] = True                                                    # CondCTElbo: x0[:, :k] conditioner, x0[:, k:] data
    assert (free == want).all()


def _rect(m):
    """m (H, W) bool with at least one True: whether its True set is one full axis-aligned rectangle."""
    r, c = m.any(1).nonzero().view(-1), m.any(0).nonzero().view(-1)
    box = torch.zeros_like(m)
    box[r.min():r.max() + 1, c.min():c.max() + 1] = True
    return torch.equal(box, m)


@pytest.mark.parametrize("name", ["half", "box"])
def test_half_and_box_geometry(name):
    from lib.losses.masks import sample_free
    C, H, W = 3, 4, 5
    cfg, D = _cfg(name, shape=(C, H, W))
    torch.manual_seed(1)
    free = torch.cat([sample_free(cfg, 8, D) for _ in range(50)]).view(-1, C, H, W)
    assert (free == free[:, :1]).all()                                 # the same in every channel
    seen = set()
    for m in free[:, 0]:
        assert m.any()
        if name == "half":
            held = ~m
            assert _rect(held)
            rows, cols = held.any(1), held.any(0)
            full_w, full_h = bool(cols.all()), bool(rows.all())
            assert full_w != full_h                                    # a band over the full width or the full height ...
            n = int(rows.sum()) if full_w else int(cols.sum())
            L = H if full_w else W
            assert n in (L // 2, L - L // 2)                           # ... of half the other side
            assert bool(rows[0] if full_w else cols[0]) != bool(rows[-1] if full_w else cols[-1])      # touching one edge
            seen.add((full_w, bool(rows[0] if full_w else cols[0])))
        else:
            assert _rect(m) or _rect(~m)                               # the rectangle is the free set or the held set
            seen.add((_rect(m), bool(m.all())))
    assert len(seen) >= (4 if name == "half" else 2)                   # top, bottom, left, right / free box and held box


def test_bernoulli_hold_share():
    """2000 samples of D = 36 with r ~ U(0.35, 0.45): the hold share against the mean rate 0.4, within 5 binomial standard
    errors sqrt(0.4 * 0.6 / (2000 * 36)).  (The spread of r adds Var(r) / 2000 = 4e-7 to the 3.3e-6 binomial variance of the share:
    5 binomial standard errors are 4.7 of the true ones.  P(a sample holds all 36) < 0.45^36: the forced free entry plays no part.)"""
    from lib.losses.masks import sample_free
    cfg, D = _cfg("bernoulli", mask_rate=[0.35, 0.45])
    torch.manual_seed(0)
    free = sample_free(cfg, 2000, D)
    share, se = 1.0 - free.float().mean().item(), (0.4 * 0.6 / (2000 * D)) ** 0.5
    print(f"bernoulli hold share {share:.5f} against 0.4 (5 se = {5 * se:.5f})")
    assert abs(share - 0.4) <= 5 * se
    per_sample = 1.0 - free.float().mean(1)
    assert per_sample.min() < 0.3 and per_sample.max() > 0.5           # (binomial spread at D = 36 is 0.08)
    # the per-sample rate is a draw: with r ~ U(0, 1) the per-sample shares spread far beyond one binomial's width
    cfg.loss.mask_rate = [0.0, 1.0]
    wide = 1.0 - sample_free(cfg, 2000, D).float().mean(1)
    assert wide.std().item() > 0.2                                     # U(0,1): 0.289; a fixed rate 0.5 at D = 36: 0.083


def test_mixture_draws_every_component():
    from lib.losses.masks import sample_free
    cfg, D = _cfg("mixture", mask_mixture=[["prefix", 1.0], ["half", 1.0]], condition_dim=1)
    torch.manual_seed(2)
    free = sample_free(cfg, 400, D)
    is_prefix = (~free).sum(1) == 1                                    # prefix holds one entry, a half holds 18
    assert 120 < int(is_prefix.sum()) < 280 and ((~free).sum(1)[~is_prefix] == 18).all()
    cfg.loss.mask_mixture = [["prefix", 0.0], ["half", 3.0]]           # a zero weight is never drawn
    assert ((~sample_free(cfg, 100, D)).sum(1) == 18).all()


BAD = [dict(mask="stripes"), dict(mask=None), dict(mask=3),
       dict(mask="prefix", condition_dim=0), dict(mask="prefix", condition_dim=36), dict(mask="prefix", condition_dim=None),
       dict(mask="bernoulli", mask_rate=None), dict(mask="bernoulli", mask_rate=[0.5]), dict(mask="bernoulli", mask_rate=[0.6, 0.2]),
       dict(mask="bernoulli", mask_rate=[-0.1, 0.5]), dict(mask="bernoulli", mask_rate=[0.5, 1.5]),
       dict(mask="mixture", mask_mixture=None), dict(mask="mixture", mask_mixture=[]), dict(mask="mixture", mask_mixture=[["half", -1.0]]),
       dict(mask="mixture", mask_mixture=[["half", 0.0]]), dict(mask="mixture", mask_mixture=[["stripes", 1.0]]),
       dict(mask="mixture", mask_mixture=[["mixture", 1.0]]), dict(mask="mixture", mask_mixture=[["bernoulli", 1.0]], mask_rate=None)]


@pytest.mark.parametrize("bad", BAD, ids=lambda b: "-".join(f"{k}={v}" for k, v in b.items()))
def test_bad_fields_raise_before_device_work(bad):
    import lib.losses.losses_utils as lu
    import lib.losses.losses  # noqa: F401
    from lib.losses.masks import sample_free
    cfg, D = _cfg(bad["mask"], **{k: v for k, v in bad.items() if k != "mask"})
    with pytest.raises(ValueError):
        sample_free(cfg, 4, D)
    loss = lu.get_loss(cfg)
    with pytest.raises(ValueError):
        loss.calc_loss(torch.zeros((3, D), dtype=torch.int64), {"model": NoDevice()})
    with pytest.raises(ValueError):
        loss.calc_loss({"model": NoDevice()}, torch.zeros((3, D), dtype=torch.int64))


@pytest.mark.parametrize("name", ["half", "box"])
@pytest.mark.parametrize("shape", [[16], [4, 4], [2, 2, 2, 2], None, [1, 3, 5]])
def test_image_masks_need_image_data(name, shape):
    from lib.losses.masks import sample_free
    cfg, _ = _cfg(name, shape=(1, 4, 4))
    cfg.data.shape = shape                                             # 1-D data, or a shape that is not the model's D = 16
    with pytest.raises(ValueError):
        sample_free(cfg, 2, 16)
    cfg.loss.update(mask="mixture", mask_mixture=[["bernoulli", 1.0], [name, 1.0]])
    with pytest.raises(ValueError):
        sample_free(cfg, 2, 16)


def test_half_of_a_single_row_or_pixel():
    from lib.losses.masks import sample_free
    cfg, D = _cfg("half", shape=(2, 1, 4))
    free = sample_free(cfg, 16, D).view(16, 2, 1, 4)                   # one row: left or right only
    assert ((~free).sum((1, 2, 3)) == 4).all() and free.any(3).all()
    cfg, D = _cfg("half", shape=(1, 1, 1))
    with pytest.raises(ValueError):
        sample_free(cfg, 2, D)


@pytest.mark.parametrize("shape", [(3, 35), (3, 37), (3, 1, 5, 7), (0, 36)])
def test_minibatch_width(shape):
    import lib.losses.losses_utils as lu
    import lib.losses.losses  # noqa: F401
    loss = lu.get_loss(_cfg("half")[0])
    with pytest.raises(ValueError):
        loss.calc_loss(torch.zeros(shape, dtype=torch.int64), {"model": NoDevice()})


def test_registry_and_entry_points():
    import lib.losses.losses as L
    import lib.losses.losses_utils as lu
    from ctdd import native
    loss = lu.get_loss(_cfg("box")[0])
    assert type(loss) is L.InpaintCTElbo and type(loss).__name__ == "InpaintCTElbo"
    assert loss.mask == "box" and loss.nll_weight == 0.1 and loss.min_time == 0.01 and loss.one_forward_pass is True and loss.ratio_eps == 1e-9
    hdr = open(os.path.join(ROOT, "include", "ctdd.h")).read()
    for name, fn in (("ctdd_ctelbo_loss_masked", native.ctelbo_loss_masked), ("ctdd_xtilde_sample_masked", native.xtilde_sample_masked)):
        assert re.search(r"^int\s+" + name + r"\s*\(", hdr, flags=re.M)
        assert name in native.EXPORTS and callable(fn)


def test_inpaint_mnist_config():
    from config.mnist_config.config_tauUnet_mnist import get_config as base
    from config.mnist_config.config_tauUnet_mnist_inpaint import get_config
    import lib.losses.losses as L
    import lib.losses.losses_utils as lu
    import lib.sampling.sampling as ls
    import lib.sampling.sampling_utils as su
    from lib.losses.masks import sample_free
    c, b = get_config(), base()
    assert c.loss.name == "InpaintCTElbo" and c.sampler.name == "ConditionalTauLeaping" and c.loss.mask == "mixture"
    assert sorted(n for n, _ in c.loss.mask_mixture) == ["bernoulli", "box", "half"]
    assert type(lu.get_loss(c)) is L.InpaintCTElbo and type(su.get_sampler(c)) is ls.ConditionalTauLeaping
    for sec in ("model", "data", "training", "optimizer"):             # the network and the data are the MNIST config's
        assert c[sec].to_dict() == b[sec].to_dict(), sec
    for k in ("eps_ratio", "nll_weight", "min_time", "one_forward_pass"):
        assert c.loss[k] == b.loss[k]
    assert b.loss.name == "CTElbo" and b.sampler.name == "TauL" and "mask" not in b.loss      # the base config is untouched
    torch.manual_seed(0)
    free = sample_free(c, 64, c.model.concat_dim)
    assert free.shape == (64, 784) and free.any(1).all() and not free.all(1).all()
