"""CPU: the conditional samplers (ConditionalTauLeaping, ConditionalPCTauLeaping) resolve from the registry, their row-list
step entry points are declared and exported, and bad arguments are refused before any device work."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ConditionalTauLeaping", "ConditionalPCTauLeaping")


def _cfg(name, condition_dim=None, D=12, S=5):
    from config.mnist_config.config_tauUnet_mnist import get_config
    c = get_config()
    c.data.S, c.model.concat_dim = S, D
    c.sampler.name = name
    if condition_dim is not None:
        c.sampler.condition_dim = condition_dim
    return c


class NoDevice:
    """A model stand-in whose every use fails: the checks must raise before the sampler touches it."""

    def __getattr__(self, k):
        raise AssertionError(f"model.{k} used before the arguments were checked")

    def __call__(self, *a, **k):
        raise AssertionError("model called before the arguments were checked")


@pytest.mark.parametrize("name", NAMES)
def test_registry_resolves(name):
    import lib.sampling.sampling as ls
    import lib.sampling.sampling_utils as su
    s = su.get_sampler(_cfg(name, 4))
    assert type(s) is getattr(ls, name) and type(s).__name__ == name
    assert callable(s.sample) and callable(s.inpaint)
    assert s.branch == 0 and s.logit_type == "direct"          # CT-ELBO rates with direct logits whatever cfg.loss is


def test_row_list_entry_points_declared_and_exported():
    from ctdd import native
    hdr = open(os.path.join(ROOT, "include", "ctdd.h")).read()
    for sym in ("ctdd_tauleap_step_rows", "ctdd_tauleap_step_s256_rows"):
        assert re.search(r"^int\s+%s\s*\(" % sym, hdr, flags=re.M), sym
        assert sym in native.EXPORTS
    assert callable(native.tauleap_step_rows) and callable(native.tauleap_step_s256_rows)


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("cd", [None, 0, -1, 12, 13])
def test_condition_dim_range(name, cd):
    import lib.sampling.sampling_utils as su
    s = su.get_sampler(_cfg(name, cd))
    with pytest.raises(ValueError):
        s.sample(NoDevice(), 3, torch.zeros((3, cd if cd and cd > 0 else 1), dtype=torch.int64))


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("shape", [(3, 3), (4, 4), (3,), (3, 4, 1), (2, 4)])
def test_conditioner_shape(name, shape):
    import lib.sampling.sampling_utils as su
    s = su.get_sampler(_cfg(name, 4))
    with pytest.raises(ValueError):
        s.sample(NoDevice(), 3, torch.zeros(shape, dtype=torch.int64))


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("xshape,mshape", [((3, 11), (12,)), ((3, 12, 1), (12,)), ((12,), (12,)),
                                           ((3, 12), (11,)), ((3, 12), (2, 12)), ((3, 12), (3, 12, 1)), ((3, 12), (12, 3))])
def test_inpaint_shapes(name, xshape, mshape):
    import lib.sampling.sampling_utils as su
    s = su.get_sampler(_cfg(name))
    with pytest.raises(ValueError):
        s.inpaint(NoDevice(), torch.zeros(xshape, dtype=torch.int64), torch.zeros(mshape, dtype=torch.bool))


@pytest.mark.parametrize("name", NAMES)
def test_inpaint_dtypes_and_values(name):
    import lib.sampling.sampling_utils as su
    s = su.get_sampler(_cfg(name))
    ok_x, ok_m = torch.zeros((3, 12), dtype=torch.int64), torch.zeros(12, dtype=torch.bool)
    with pytest.raises(ValueError):                              # mask must be bool
        s.inpaint(NoDevice(), ok_x, ok_m.to(torch.int32))
    with pytest.raises(ValueError):                              # states must be integers
        s.inpaint(NoDevice(), ok_x.float(), ok_m)
    bad = ok_x.clone()
    bad[1, 2] = 5                                                # S = 5: held value out of range
    with pytest.raises(ValueError):
        s.inpaint(NoDevice(), bad, ok_m | (torch.arange(12) == 2))


@pytest.mark.parametrize("name", NAMES)
def test_all_held_returns_known_without_device_work(name):
    import lib.sampling.sampling_utils as su
    s = su.get_sampler(_cfg(name))
    xk = torch.randint(0, 5, (4, 12))
    out = s.inpaint(NoDevice(), xk, torch.ones(12, dtype=torch.bool))
    assert out.shape == (4, 12) and out.dtype.kind == "i" and (out == xk.numpy()).all()
