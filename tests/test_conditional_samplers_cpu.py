"""CPU: ConditionalLBJF, ConditionalMidPointTauL and ConditionalExactSampling resolve from the registry, follow cfg.loss, their
row-list step entry points are declared, exported and bound, and bad arguments are refused before any device work."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ConditionalLBJF", "ConditionalMidPointTauL", "ConditionalExactSampling")
PARENT = {"ConditionalLBJF": "LBJF", "ConditionalMidPointTauL": "MidPointTauL", "ConditionalExactSampling": "ExactSampling"}
ENTRY_POINTS = ("ctdd_lbjf_step_rows", "ctdd_midpoint_predict_rows", "ctdd_exact_step_rows", "ctdd_lbjf_from_rates_rows",
                "ctdd_midpoint_from_rates_rows")


def _cfg(name, condition_dim=None, D=12, S=5, loss="CTElbo", logit_type="direct"):
    from config.mnist_config.config_tauUnet_mnist import get_config
    c = get_config()
    c.data.S, c.model.concat_dim = S, D
    c.loss.name, c.loss.logit_type = loss, logit_type
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
def test_registry_resolves_and_follows_the_parent(name):
    import lib.sampling.sampling as ls
    import lib.sampling.sampling_utils as su
    s = su.get_sampler(_cfg(name, 4))
    assert type(s) is getattr(ls, name) and type(s).__name__ == name
    assert isinstance(s, getattr(ls, PARENT[name])) and isinstance(s, ls._Conditioned)
    assert callable(s.sample) and callable(s.inpaint)
    assert s.branch == 0 and s.logit_type == "direct" and s.max_t == s.cfg.training.max_t
    # unlike the two tau-leaping samplers, branch and logit type come from cfg.loss
    s = su.get_sampler(_cfg(name, 4, loss="CatRM", logit_type="reverse_prob"))
    assert s.branch == 1 and s.logit_type == "reverse_prob"


def test_row_list_entry_points_declared_exported_and_bound():
    from ctdd import native
    hdr = open(os.path.join(ROOT, "include", "ctdd.h")).read()
    for sym in ENTRY_POINTS:
        assert re.search(r"^int\s+%s\s*\(" % sym, hdr, flags=re.M), sym
        assert sym in native.EXPORTS
        assert callable(getattr(native, sym[len("ctdd_"):]))
        # ... and the C argument count of the declaration is the binding's
        decl = re.search(r"^int\s+%s\s*\(([^;]*)\);" % sym, hdr, flags=re.M | re.S).group(1)
        assert len(decl.split(",")) == len(native._SIGS[sym][0]), sym


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
    for v in (5, -1):                                            # S = 5: held value out of range
        bad = ok_x.clone()
        bad[1, 2] = v
        with pytest.raises(ValueError):
            s.inpaint(NoDevice(), bad, ok_m | (torch.arange(12) == 2))


@pytest.mark.parametrize("mask_shape", ["D", "ND"])
@pytest.mark.parametrize("name", NAMES)
def test_all_held_returns_known_without_device_work(name, mask_shape):
    """Nothing free: x_known comes back in the parent's return shape, every per-step figure zero (no step ran)."""
    import lib.sampling.sampling_utils as su
    c = _cfg(name)
    c.sampler.num_steps = 7
    s = su.get_sampler(c)
    xk = torch.randint(0, 5, (4, 12))
    out = s.inpaint(NoDevice(), xk, torch.ones(12 if mask_shape == "D" else (4, 12), dtype=torch.bool))
    assert isinstance(out, tuple) and len(out) == (5 if name == "ConditionalMidPointTauL" else 2)
    assert out[0].shape == (4, 12) and out[0].dtype.kind == "i" and (out[0] == xk.numpy()).all()
    for traj in out[1:]:
        assert isinstance(traj, list) and len(traj) in (0, 7) and all(not v for v in traj if v == v)
