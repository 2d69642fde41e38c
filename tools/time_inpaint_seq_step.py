"""Inpainting training of the hollow transformers: one Standard.step with the masked objective next to the unmasked one, at the
shipped configs and batch 128, random-init weights.

    config_hollow_maze       (ScoreElbo)   against  config_hollow_maze_inpaint       (InpaintScoreElbo, mixture of masks)
    config_hollow_synthetic  (ScoreElbo)   against  config_hollow_synthetic_inpaint  (InpaintCatRM, bernoulli masks)

The four cases alternate inside every repeat; a repeat is a device-synchronised window of `--steps` steps after a warm-up of every
case.  Reported: the median over the repeats and their min .. max (the run-to-run spread on this box).

    python tools/time_inpaint_seq_step.py [--repeats 5] [--steps 30] [--batch 128]
    rocprofv3 --kernel-trace --stats --output-format csv -d prof_out/seq -o seq -- python tools/time_inpaint_seq_step.py --profile maze_inpaint
--profile CASE (maze | maze_inpaint | synthetic | synthetic_inpaint) runs `--steps` steps of that case and nothing else.
"""
import argparse
import importlib
import os
import statistics
import sys
import time

_R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [_R, os.path.join(_R, "continuous-time-diffusion-models-for-discrete-data_amd")]

CASES = {"maze": "config.maze_config.config_hollow_maze", "maze_inpaint": "config.maze_config.config_hollow_maze_inpaint",
         "synthetic": "config.synthetic_config.config_hollow_synthetic",
         "synthetic_inpaint": "config.synthetic_config.config_hollow_synthetic_inpaint"}


def _window(torch, fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def _case(torch, name, batch):
    import lib.models.models, lib.losses.losses, lib.training.training, lib.optimizers.optimizers  # noqa: F401, E401
    import lib.models.model_utils as mu
    import lib.losses.losses_utils as lu
    import lib.training.training_utils as tu
    import lib.optimizers.optimizers_utils as ou
    cfg = importlib.import_module(CASES[name]).get_config()
    cfg.device = "cuda"
    torch.manual_seed(0)
    model = mu.create_model(cfg, torch.device("cuda"))
    state = {"model": model, "optimizer": ou.get_optimizer(model.parameters(), cfg), "n_iter": 0}
    step, loss = tu.get_train_step(cfg), lu.get_loss(cfg)
    mb = torch.randint(0, int(cfg.data.S), [batch] + list(cfg.data.shape), device="cuda")

    def one():
        step.step(state, loss, mb)
        state["n_iter"] += 1
    return f"{cfg.loss.name:17s} ({CASES[name].rsplit('.', 1)[1]})", one


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--profile", choices=tuple(CASES), default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("time_inpaint_seq_step.py measures on the GPU: no device found")
    print(torch.cuda.get_device_name(0))
    if a.profile is not None:
        label, one = _case(torch, a.profile, a.batch)
        for _ in range(3):
            one()
        print(f"{label}: {a.steps} steps, {_window(torch, one, a.steps) * 1e3:.2f} ms per step under the profiler")
        return
    cases = dict(_case(torch, name, a.batch) for name in CASES)
    for one in cases.values():                                       # warm-up: code objects, allocator, plans
        for _ in range(3):
            one()
    out = {k: [] for k in cases}
    for _ in range(a.repeats):
        for k, one in cases.items():
            out[k].append(_window(torch, one, a.steps) * 1e3)
    print(f"Standard.step, batch {a.batch}: {a.repeats} repeats x {a.steps} steps, ms per step (median, min .. max)")
    res = {k: (statistics.median(v), min(v), max(v)) for k, v in out.items()}
    for k, (med, lo, hi) in res.items():
        print(f"  {k:58s} {med:7.2f}  ({lo:.2f} .. {hi:.2f})")
    keys = list(res)
    for plain, masked in ((keys[0], keys[1]), (keys[2], keys[3])):
        (p, lo, hi), (m, _, _) = res[plain], res[masked]
        print(f"  masked / unmasked = {m / p:.3f}; spread of the unmasked step {100 * (hi - lo) / p:.1f} %   [{masked.split()[0]}]")


if __name__ == "__main__":
    main()
