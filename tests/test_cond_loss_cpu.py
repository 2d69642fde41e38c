"""CPU: the prefix-conditioned training loss CondCTElbo resolves from the registry, refuses bad arguments before any device work,
its window entry point is declared and exported, and the conditional MNIST config is self-consistent."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D_, S_ = 12, 5


def _cfg(condition_dim, D=D_, S=S_):
    from config.mnist_config.config_tauUnet_mnist import get_config
    c = get_config()
    c.data.S, c.model.concat_dim = S, D
    c.loss.update(name="CondCTElbo", nll_weight=0.1, condition_dim=condition_dim)
    return c


class NoDevice:
    """A model stand-in whose every use fails: the checks must raise before the loss touches it."""

    def __getattr__(self, k):
        raise AssertionError(f"model.{k} used before the arguments were checked")

    def __call__(self, *a, **k):
        raise AssertionError("model called before the arguments were checked")


def test_registry_resolves():
    import lib.losses.losses as L
    import lib.losses.losses_utils as lu
    loss = lu.get_loss(_cfg(4))
    assert type(loss) is L.CondCTElbo and type(loss).__name__ == "CondCTElbo"
    assert loss.condition_dim == 4 and loss.nll_weight == 0.1 and loss.min_time == 0.01 and loss.one_forward_pass is True
    assert loss.ratio_eps == 1e-9


def test_window_entry_point_declared_and_exported():
    from ctdd import native
    hdr = open(os.path.join(ROOT, "include", "ctdd.h")).read()
    assert re.search(r"^int\s+ctdd_ctelbo_loss_window\s*\(", hdr, flags=re.M)
    assert "ctdd_ctelbo_loss_window" in native.EXPORTS and callable(native.ctelbo_loss_window)


@pytest.mark.parametrize("cd", [0, D_, -1, None])
@pytest.mark.parametrize("order", ["minibatch_first", "state_first"])
def test_condition_dim_range(cd, order):
    import lib.losses.losses_utils as lu
    import lib.losses.losses  # noqa: F401
    loss = lu.get_loss(_cfg(cd))
    state, mb = {"model": NoDevice()}, torch.zeros((3, D_), dtype=torch.int64)
    with pytest.raises(ValueError):
        loss.calc_loss(mb, state) if order == "minibatch_first" else loss.calc_loss(state, mb)


@pytest.mark.parametrize("shape", [(3, D_ - 1), (3, D_ + 1), (3, 1, 2, 5), (3, 1, 4, 4)])
def test_minibatch_width(shape):
    import lib.losses.losses_utils as lu
    import lib.losses.losses  # noqa: F401
    loss = lu.get_loss(_cfg(4))
    with pytest.raises(ValueError):
        loss.calc_loss(torch.zeros(shape, dtype=torch.int64), {"model": NoDevice()})


def test_conditional_mnist_config():
    from config.mnist_config.config_tauUnet_mnist import get_config as base
    from config.mnist_config.config_tauUnet_mnist_cond import get_config
    import lib.losses.losses as L
    import lib.losses.losses_utils as lu
    import lib.sampling.sampling as ls
    import lib.sampling.sampling_utils as su
    c, b = get_config(), base()
    assert c.loss.name == "CondCTElbo" and c.sampler.name == "ConditionalTauLeaping"
    assert c.loss.condition_dim == c.sampler.condition_dim == 392 == 14 * 28          # the top 14 rows of the 28 x 28 image
    assert 0 < c.loss.condition_dim < c.model.concat_dim == 784
    assert type(lu.get_loss(c)) is L.CondCTElbo and type(su.get_sampler(c)) is ls.ConditionalTauLeaping
    for sec in ("model", "data", "training", "optimizer"):                             # the network and the data are the MNIST config's
        assert c[sec].to_dict() == b[sec].to_dict(), sec
    for k in ("eps_ratio", "nll_weight", "min_time", "one_forward_pass"):
        assert c.loss[k] == b.loss[k]
    assert b.loss.name == "CTElbo" and b.sampler.name == "TauL"                        # the base config is untouched
