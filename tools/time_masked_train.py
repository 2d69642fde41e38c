"""Timings of the masked ("enumerative") transformer's training path (needs a GPU).

    python tools/time_masked_train.py [--reps 5] [--only kernels|steps] [--out FILE.json]
    rocprofv3 --kernel-trace --stats -d prof_out -- python tools/time_masked_train.py --profile [--config maze] [--precision bf16]

(i) kernels: the forward + backward pair of the short-sequence training attention (ctdd_bert_attention_short_train / _bwd)
against the generic fp32 pair (ctdd_hollow_attention_train / _bwd) through the C ABI on the same preallocated buffers, packed
qkv rows at (B 4096, T 33, H 8, hd 8) -- the attention of one forward of config_masked_synthetic at batch 128 -- with dropout
0 and 0.1.  Device time between two events around a run of pairs; the two variants alternate, `reps` rounds each.
(ii) steps: one whole Standard.step (noising, network forward, objective, backward, gradient clipping, Adam + EMA) of
config_masked_synthetic at batch 128 and of config_bert_mazemasked at its batch 16 with their shipped dropout rates: the
autograd module (cfg.model.engine_train = "torch") against the HIP training kernels ("hip-masked", ctdd/masked_train.py) in
both training precisions.  Method of tools/time_bert.py: every variant is warmed up, then the variants are timed in alternation
in one process, `reps` rounds of a window of at least 0.3 s of steps between device synchronisations.  Next to each step time:
the peak of torch.cuda.max_memory_allocated() over one further step of that variant, and what was allocated before it.
Every figure is the median round and the spread (max - min) / median over the rounds.
--profile runs six steps of one HIP variant and nothing else (the target of one rocprofv3 kernel trace).
"""
import argparse
import ctypes as C
import importlib
import json
import os
import statistics
import sys

_R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [_R, os.path.join(_R, "continuous-time-diffusion-models-for-discrete-data_amd"), os.path.join(_R, "tools")]
import torch  # noqa: E402
import lib.models.models  # noqa: E402,F401
import lib.losses.losses  # noqa: E402,F401
import lib.training.training  # noqa: E402,F401
import lib.optimizers.optimizers  # noqa: E402,F401
import lib.models.model_utils as mu  # noqa: E402
import lib.losses.losses_utils as lu  # noqa: E402
import lib.training.training_utils as tu  # noqa: E402
import lib.optimizers.optimizers_utils as ou  # noqa: E402
from time_bert import alternate  # noqa: E402

CONFIGS = {"synthetic_config.config_masked_synthetic": 128, "maze_config.config_bert_mazemasked": 16}
VARIANTS = (("module", "torch", None), ("hip-masked fp32", "hip-masked", "fp32"), ("hip-masked bf16", "hip-masked", "bf16"))
KERNEL_SHAPE = dict(B=4096, T=33, H=8, hd=8)


def kernel_pairs(reps, pairs_per_round=50):
    from ctdd import hollow_train as ht
    lib = ht.lib()
    B, T, H, hd = (KERNEL_SHAPE[k] for k in ("B", "T", "H", "hd"))
    E = H * hd
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device="cuda").manual_seed(0)
    qkv = torch.randn((B * T, 3 * E), device="cuda", generator=g)
    dout = torch.randn((B * T, E), device="cuda", generator=g)
    out, stats, dqkv = torch.empty((B * T, E), device="cuda"), torch.empty((B, H, T, 4), device="cuda"), torch.empty_like(qkv)
    rng = torch.tensor([99, 5], dtype=torch.int64, device="cuda")
    res = {"shape": KERNEL_SHAPE, "pairs_per_round": pairs_per_round}
    for p in (0.0, 0.1):
        a = ht._attn_args(qkv, None, None, B, T, T, H, hd, 3, p, rng if p > 0 else None, 1)
        a.out, a.stats, a.d_out = out.data_ptr(), stats.data_ptr(), dout.data_ptr()
        a.dq, a.dk, a.dv = dqkv.data_ptr(), dqkv.data_ptr() + 4 * E, dqkv.data_ptr() + 8 * E
        a.dq_bs = a.dk_bs = a.dv_bs = T * 3 * E
        a.dq_rs = a.dk_rs = a.dv_rs = 3 * E
        fns = {"generic fp32": (lib.ctdd_hollow_attention_train, lib.ctdd_hollow_attention_bwd),
               "short": (lib.ctdd_bert_attention_short_train, lib.ctdd_bert_attention_short_bwd)}

        def run(name, n):
            fwd, bwd = fns[name]
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n):
                if fwd(C.byref(a), st) != 0 or bwd(C.byref(a), st) != 0:
                    sys.exit(f"{name}: launch refused")
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / n                  # ms per pair

        times = {k: [] for k in fns}
        for k in fns:
            run(k, 5)
        for _ in range(reps):
            for k in fns:
                times[k].append(run(k, pairs_per_round))
        r = {k: dict(median_ms=statistics.median(v), spread=(max(v) - min(v)) / statistics.median(v), rounds_ms=[round(t, 5) for t in v])
             for k, v in times.items()}
        res[f"p={p}"] = r
        print("attention pair", f"p={p}", json.dumps({k: (round(v["median_ms"], 4), round(v["spread"], 3)) for k, v in r.items()}), flush=True)
    return res


def stepper(mod, batch, engine_train, precision):
    """-> (cfg, model, a closure running one training step on a fixed random minibatch)."""
    cfg = importlib.import_module("config." + mod).get_config()
    cfg.device = "cuda"
    cfg.model.engine_train = engine_train
    if precision is not None:
        cfg.model.engine_train_precision = precision
    torch.manual_seed(0)
    model = mu.create_model(cfg, torch.device("cuda"))
    state = {"model": model, "optimizer": ou.get_optimizer(model.parameters(), cfg), "n_iter": 0}
    loss, step = lu.get_loss(cfg), tu.get_train_step(cfg)
    mb = torch.randint(0, cfg.data.S, (batch, int(cfg.model.concat_dim)), device="cuda")

    def run():
        step.step(state, loss, mb)
        state["n_iter"] += 1
    return cfg, model, run


def steps(reps):
    out = {}
    for mod, batch in CONFIGS.items():
        variants, models = {}, {}
        for name, engine_train, precision in VARIANTS:
            _, models[name], variants[name] = stepper(mod, batch, engine_train, precision)
        r = alternate(variants, reps)
        for name, engine_train, _ in VARIANTS:           # every variant ran the path it names
            assert (models[name]._trainer is not None) == (engine_train == "hip-masked"), name
        for name, fn in variants.items():
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            before = torch.cuda.memory_allocated()
            fn()
            torch.cuda.synchronize()
            r[name]["peak_MiB"] = round(torch.cuda.max_memory_allocated() / 2 ** 20, 1)
            r[name]["allocated_before_MiB"] = round(before / 2 ** 20, 1)
        r["batch"] = batch
        out[mod.split(".")[-1]] = r
        print(mod, f"batch {batch}", json.dumps({k: (round(v["median_ms"], 3), round(v["spread"], 3), v["peak_MiB"]) for k, v in r.items() if k != "batch"}),
              flush=True)
        del variants, models
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", choices=("kernels", "steps"), default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--config", choices=("synthetic", "maze"), default="maze")
    ap.add_argument("--precision", choices=("fp32", "bf16"), default="bf16")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_masked_train.py needs a GPU")
    if a.profile:
        mod = [m for m in CONFIGS if a.config in m][0]
        _, model, run = stepper(mod, CONFIGS[mod], "hip-masked", a.precision)
        for _ in range(6):
            run()
        torch.cuda.synchronize()
        assert model._trainer is not None
        return
    if a.reps < 5:
        sys.exit("at least five repeats")
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps}
    if a.only != "steps":
        res["attention_pair"] = kernel_pairs(a.reps)
    if a.only != "kernels":
        res["step"] = steps(a.reps)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
