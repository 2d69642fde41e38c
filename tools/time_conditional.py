"""Conditional vs unconditional sampling on the MNIST tauLDR U-Net (random-init weights, N = 256, bf16 defaults), sample-steps/s:
TauL, then ConditionalTauLeaping holding the top half of the digit (condition_dim = 392: its steps run the row-list S = 256 kernel
on the 392 free rows of every sample).  Each case: one warm-up call, then a device-synchronised timed call.
`--followers`: per sampler step, LBJF against ConditionalLBJF and MidPointTauL against ConditionalMidPointTauL with half of each
sample held (the first D / 2 entries), at the maze hollow config's sampling shape (S = 3, D = 225, N = 128) and at one S = 256
shape (the MNIST U-Net, D = 784, N = 256); median of three calls of --steps grid steps (default 50).

    python tools/time_conditional.py [--steps K]              # K grid steps per call (default: the config's grid, as bench.py)
    python tools/time_conditional.py --followers [--steps K]
    rocprofv3 --kernel-trace --stats --output-format csv -d prof_out/cond -o cond -- python tools/time_conditional.py --steps 50
    python tools/time_conditional.py --stats prof_out/cond/.../cond_kernel_stats.csv   # average time of the two step kernels
"""
import argparse
import csv
import os
import sys
import time

_R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [_R, os.path.join(_R, "continuous-time-diffusion-models-for-discrete-data_amd")]


def stats(path):
    """Average duration of the full and the row-list S = 256 bf16 step kernels in a rocprofv3 kernel_stats.csv."""
    with open(path) as f:
        for row in csv.DictReader(f):
            name = row.get("Name", "")
            if "k_tauleap_s256" in name:
                kind = "row list" if "Lb1EE" in name or ", true>" in name else "full"
                print(f"{kind:8s} {row.get('Calls', '?'):>6s} calls  avg {float(row['AverageNs']) / 1e3:8.2f} us  {name[:110]}")


def followers(steps):
    """LBJF / MidPointTauL against their conditional forms, half of each sample held: ms per sampler step."""
    import torch
    import lib.models.models  # noqa: F401
    import lib.sampling.sampling  # noqa: F401
    import lib.models.model_utils as mu
    import lib.sampling.sampling_utils as su
    from config.maze_config.config_hollow_maze import get_config as maze
    from config.mnist_config.config_tauUnet_mnist import get_config as mnist
    for label, get_config, N in (("maze hollow", maze, 128), ("MNIST U-Net", mnist, 256)):
        cfg = get_config()
        cfg.device = "cuda"
        cfg.sampler.num_steps = steps
        torch.manual_seed(0)
        model = mu.create_model(cfg, torch.device("cuda"))
        model.eval()
        D, S = cfg.model.concat_dim, cfg.data.S
        cd = D // 2
        cond = torch.randint(0, S, (N, cd))
        for parent in ("LBJF", "MidPointTauL"):
            ms = {}
            for name in (parent, "Conditional" + parent):
                cfg.sampler.name, cfg.sampler.condition_dim = name, cd
                s = su.get_sampler(cfg)
                s.seed = 1
                run = (lambda: s.sample(model, N)) if name == parent else (lambda: s.sample(model, N, cond))
                run()                                              # warm-up: plans, tables
                torch.cuda.synchronize()
                els = []
                for _ in range(3):
                    t0 = time.perf_counter()
                    nst = len(run()[-1])                           # (the last per-step list: the steps the grid really has)
                    torch.cuda.synchronize()
                    els.append(time.perf_counter() - t0)
                ms[name] = sorted(els)[1] / nst * 1e3
                print(f"{label:12s} S={S:3d} D={D} N={N} {name:24s} {nst} steps: {ms[name]:.3f} ms/step", flush=True)
            print(f"{label:12s} Conditional{parent} / {parent}: {ms['Conditional' + parent] / ms[parent]:.3f}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=None)
    ap.add_argument("--N", type=int, default=256)
    ap.add_argument("--stats", default=None)
    ap.add_argument("--followers", action="store_true")
    a = ap.parse_args()
    if a.stats is not None:
        return stats(a.stats)
    if a.followers:
        return followers(a.steps or 50)
    import torch
    import lib.models.models  # noqa: F401
    import lib.sampling.sampling  # noqa: F401
    import lib.models.model_utils as mu
    import lib.sampling.sampling_utils as su
    from config.mnist_config.config_tauUnet_mnist import get_config
    cfg = get_config()
    cfg.device = "cuda"
    steps = a.steps or cfg.sampler.num_steps
    torch.manual_seed(0)
    model = mu.create_model(cfg, torch.device("cuda"))
    model.eval()
    N, cd = a.N, 392
    cond = torch.randint(0, cfg.data.S, (N, cd))
    for name in ("TauL", "ConditionalTauLeaping"):
        cfg.sampler.name, cfg.sampler.condition_dim = name, cd

        def run(k):
            cfg.sampler.num_steps = k
            s = su.get_sampler(cfg)
            s.seed = 1
            return s.sample(model, N) if name == "TauL" else s.sample(model, N, cond)
        run(min(steps, 10))                                        # warm-up: plans, tables
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run(steps)
        torch.cuda.synchronize()
        el = time.perf_counter() - t0
        print(f"{name:22s} N={N} steps={steps}: {el:.2f} s -> {N * steps / el:.0f} sample-steps/s ({el / steps * 1e3:.2f} ms/step)")


if __name__ == "__main__":
    main()
