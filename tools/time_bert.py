"""Timings of the x0-prediction ("BERT") and masked transformer score models (needs a GPU).

    python tools/time_bert.py [--reps 5] [--out FILE.json]      forwards + samplers, one JSON document
    python tools/time_bert.py --profile                         one masked-synthetic forward per call (a rocprofv3 target)

Forward: the four shipped configs at their batch sizes -- the autograd module on torch device ops (cfg.model.engine = "torch"),
the HIP engine in its three precisions and, where T = D + 1 <= 64, the default precision with the short-sequence attention
kernel switched off (cfg.model.engine_attention_short = False).  Every variant is warmed up (plans built and captured), then
the variants are timed in alternation, `reps` rounds of a window of forwards each between device synchronisations; the figure
is the median round and the spread (max - min) / median over the rounds.
Samplers: TauL sample-steps/s for config_bert_maze at N = 128 and LBJF for config_masked_synthetic at N = 128, engine
(default precision) against the module, alternating, median of `reps` calls.
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

_R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [_R, os.path.join(_R, "continuous-time-diffusion-models-for-discrete-data_amd")]
import torch  # noqa: E402
import lib.models.models  # noqa: E402,F401
import lib.sampling.sampling  # noqa: E402,F401
import lib.models.model_utils as mu  # noqa: E402
import lib.sampling.sampling_utils as su  # noqa: E402
from ctdd.bert_engine import BertEngine  # noqa: E402

CONFIGS = ("maze_config.config_bert_maze", "synthetic_config.config_bert_synthetic", "synthetic_config.config_masked_synthetic",
           "maze_config.config_bert_mazemasked")


def build(mod):
    cfg = importlib.import_module("config." + mod).get_config()
    cfg.device = "cuda"
    torch.manual_seed(0)
    model = mu.create_model(cfg, torch.device("cuda"))
    model.eval()
    return cfg, model


def window(fn, min_seconds=0.3):
    """Seconds per call over a window of at least min_seconds (sized from one timed call), ending in a synchronise."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    n = max(3, min(200, int(min_seconds / max(time.perf_counter() - t0, 1e-5))))
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


def alternate(variants, reps):
    times = {k: [] for k in variants}
    for fn in variants.values():                       # warm-up: plans, graphs, library algorithm choices
        fn()
        fn()
    for _ in range(reps):
        for k, fn in variants.items():
            times[k].append(window(fn))
    return {k: dict(median_ms=1e3 * statistics.median(v), spread=(max(v) - min(v)) / statistics.median(v), rounds_ms=[round(1e3 * t, 4) for t in v])
            for k, v in times.items()}


def forwards(reps):
    out = {}
    for mod in CONFIGS:
        cfg, model = build(mod)
        B, D, S = cfg.data.batch_size, int(cfg.model.concat_dim), cfg.data.S
        x = torch.randint(0, S, (B, D), device="cuda")
        t = torch.rand(B, device="cuda")

        def module():
            cfg.model.engine = "torch"
            with torch.no_grad():
                model(x, t)
            cfg.model.engine = "hip"
        variants = {"module": module}
        with torch.no_grad():
            for p in ("fp32", "bf16x3", "bf16"):
                variants["engine " + p] = (lambda e: (lambda: e(x, t)))(BertEngine(model, precision=p))
            if D + 1 <= 64:
                cfg.model.engine_attention_short = False
                eng = BertEngine(model, precision="bf16x3")
                eng(x, t)                               # (the plan is built under the knob)
                variants["engine bf16x3, generic attention"] = (lambda e: (lambda: e(x, t)))(eng)
                cfg.model.engine_attention_short = True
            res = alternate(variants, reps)
        res["shape"] = dict(batch=B, D=D, S=S, sequences=B * D if "Masked" in cfg.model.name else B)
        out[mod.split(".")[-1]] = res
        print(mod, json.dumps({k: (round(v["median_ms"], 3), round(v["spread"], 3)) for k, v in res.items() if k != "shape"}), flush=True)
        del model
        torch.cuda.empty_cache()
    return out


def samplers(reps):
    out = {}
    for mod, name, steps in (("maze_config.config_bert_maze", "TauL", 50), ("synthetic_config.config_masked_synthetic", "LBJF", 50)):
        cfg, model = build(mod)
        cfg.sampler.name, cfg.sampler.num_steps = name, steps
        N = 128
        times = {"engine": [], "module": []}
        for rep in range(reps + 1):
            for k in times:
                cfg.model.engine = "hip" if k == "engine" else "torch"
                smp = su.get_sampler(cfg)
                smp.seed = 7
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                smp.sample(model, N)                    # (returns host arrays: synchronised)
                torch.cuda.synchronize()
                if rep:                                 # round 0 is the warm-up
                    times[k].append(time.perf_counter() - t0)
        cfg.model.engine = "hip"
        out[f"{mod.split('.')[-1]} {name} N={N}"] = {
            k: dict(sample_steps_per_s=N * steps / statistics.median(v), spread=(max(v) - min(v)) / statistics.median(v)) for k, v in times.items()}
        print(mod, name, json.dumps(out[f"{mod.split('.')[-1]} {name} N={N}"]), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--skip-samplers", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_bert.py needs a GPU")
    if a.profile:
        cfg, model = build("synthetic_config.config_masked_synthetic")
        x = torch.randint(0, cfg.data.S, (cfg.data.batch_size, int(cfg.model.concat_dim)), device="cuda")
        t = torch.rand(cfg.data.batch_size, device="cuda")
        with torch.no_grad():
            for _ in range(4):
                model(x, t)
        torch.cuda.synchronize()
        return
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "forward": forwards(a.reps)}
    if not a.skip_samplers:
        res["samplers"] = samplers(max(3, a.reps // 2 + 1))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
