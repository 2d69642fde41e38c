"""Launch lists of a fixed set of U-Net plans, one line per launch: `fn name | label | flops`, forward then backward.  The plans are
built with UNetEngine._build only (allocation and weight packing, nothing is launched); together they reach every dispatch branch
of the plan construction.  tests/golden/unet_plans.json is this tool's output, tests/test_gpu_unet_plans.py compares against it.

    python tools/dump_unet_plans.py [--out tests/golden/unet_plans.json]

Plan build times (host work, once per plan) go to stderr.
"""
import argparse
import json
import os
import sys
import time

_R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [_R, os.path.join(_R, "continuous-time-diffusion-models-for-discrete-data_amd")]
import torch  # noqa: E402

# name -> (config, engine precision, batch, _build keywords, training plan with dropout)
PLANS = {
    "a_mnist_bf16_b128_time_row": ("mnist", "bf16", 128, dict(logits_bf16=True, uniform_t="row"), False),   # ring, fused 7x7 blocks, one-pass GN
    "b_mnist_bf16_b4_per_sample_t": ("mnist", "bf16", 4, dict(uniform_t=False), False),      # patch small tiles, automatic split-K, time launch
    "c_mnist_fp32_b4": ("mnist", "fp32", 4, dict(), False),                                  # igemm, SEG_3x3_UP, k_gn_apply everywhere
    "d_mnist_bf16_b64_train_dropout": ("mnist", "bf16", 64, dict(), True),                   # forward + backward, prologue, wgrad tables, sums
    "e_cifar_bf16_b32_logistic": ("cifar10", "bf16", 32, dict(logits_bf16=True), False),     # logistic head, N = 256 ring tiles, attention
}


def _model(config):
    import lib.models.models  # noqa: F401
    import lib.models.model_utils as mu
    if config == "mnist":
        from config.mnist_config.config_tauUnet_mnist import get_config
    else:
        from config.cifar10_config.config_tauUnet_cifar10 import get_config
    cfg = get_config()
    cfg.device = "cuda"
    # the snapshot pins the plans with the 14x14 blocks as four launches each (the plan cfg.model.resblock_fused_mid = 0 must keep,
    # launch for launch); the plans with ctdd_unet_resblock_mid are pinned by tests/test_gpu_resblock_mid.py
    cfg.model.resblock_fused_mid = 0
    # likewise the Upsample convolutions as ctdd_unet_upsample2x + a stride-1 ring launch (cfg.model.upsample_phases = 0); the plans
    # with ctdd_unet_conv_up_phases are pinned by tests/test_gpu_upsample_phases.py
    cfg.model.upsample_phases = 0
    # and the 28x28 GroupNorm + convolution pairs as two launches each (cfg.model.conv_rows = 0); the plans with
    # ctdd_unet_conv_rows are pinned by tests/test_gpu_conv_rows.py
    cfg.model.conv_rows = 0
    # and the mid attention block as qkv convolution + ctdd_unet_attention + proj convolution (cfg.model.attention_fused = 0); the
    # plans with ctdd_unet_attention_block are pinned by tests/test_gpu_attention_fused.py
    cfg.model.attention_fused = 0
    torch.manual_seed(0)
    return mu.create_model(cfg, torch.device("cuda"))


def _lines(plan):
    return [f"{step.label[0]} | {step.label[1]} | {step.flops}" for step in plan]


def dump(names=None, times=None):
    """{plan name: [line per launch]}; times (a dict) receives each plan's build time in seconds."""
    from ctdd import unet_train
    from ctdd.unet_engine import UNetEngine
    out, models = {}, {}
    for name in names or PLANS:
        config, precision, B, kw, train = PLANS[name]
        if config not in models:
            models[config] = _model(config)
        eng = UNetEngine(models[config], precision=precision)
        if train:
            unet_train.lib()
            kw = dict(kw, tc=unet_train.TrainCtx(eng, B, True))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        st = eng._build(B, torch.int64, None, **kw)
        torch.cuda.synchronize()
        if times is not None:
            times[name] = time.perf_counter() - t0
        out[name] = _lines(st.plan) + (["-- backward"] + _lines(st.bwd_plan) if train else [])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="write the JSON here (default: stdout)")
    a = ap.parse_args()
    times = {}
    text = json.dumps(dump(times=times), indent=0) + "\n"
    for name, s in times.items():
        print(f"build {name}: {s * 1e3:.0f} ms", file=sys.stderr)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    else:
        sys.stdout.write(text)


if __name__ == "__main__":
    main()
