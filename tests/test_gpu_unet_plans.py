"""GPU: the launch sequence of the U-Net plans is pinned.  tests/golden/unet_plans.json holds, for a fixed list of plans that
together reach every dispatch branch of the plan construction (tools/dump_unet_plans.py: PLANS), one line per launch --
`fn name | label | flops`, forward then backward -- as the tool printed them before the plan construction became a builder
object.  The plans are rebuilt here with UNetEngine._build alone (allocation and weight packing, no launch) and must match the
file line for line: same launches, same kernel choices, same order."""
import json
import os

import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "unet_plans.json")


@pytest.fixture(scope="module")
def plans():
    import importlib.util
    spec = importlib.util.spec_from_file_location("dump_unet_plans", os.path.join(os.path.dirname(GOLDEN), "..", "..", "tools", "dump_unet_plans.py"))
    dump_unet_plans = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(dump_unet_plans)
    with open(GOLDEN) as f:
        want = json.load(f)
    assert list(want) == list(dump_unet_plans.PLANS)
    return want, dump_unet_plans.dump()


@pytest.mark.parametrize("name", ["a_mnist_bf16_b128_time_row", "b_mnist_bf16_b4_per_sample_t", "c_mnist_fp32_b4",
                                  "d_mnist_bf16_b64_train_dropout", "e_cifar_bf16_b32_logistic"])
def test_plan_matches_snapshot(plans, name):
    want, got = plans
    assert len(want[name]) > 20
    for i, (w, g) in enumerate(zip(want[name], got[name])):
        assert g == w, f"{name}: launch {i}"
    assert len(got[name]) == len(want[name])
