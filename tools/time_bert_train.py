"""Timings of one whole training step of the x0-prediction ("BERT") transformer (needs a GPU).

    python tools/time_bert_train.py [--reps 5] [--out FILE.json]
    rocprofv3 --kernel-trace --stats -d prof_out -- python tools/time_bert_train.py --profile [--config maze] [--precision bf16]

One step is Standard.step with the configured loss (CTElbo with one forward pass): noising, network forward, objective,
backward, gradient clipping, Adam + EMA.  config_bert_maze and config_bert_synthetic at batch 128 with their shipped dropout
rates; the autograd module (cfg.model.engine_train = "torch") against the HIP training kernels (cfg.model.engine_train =
"hip-encoder", ctdd/bert_train.py) in both training precisions.  Method of tools/time_bert.py: every variant is warmed up, then
the variants are timed in alternation in one process, `reps` rounds of a window of at least 0.3 s of steps between device
synchronisations; the figure is the median round and the spread (max - min) / median over the rounds.
--profile runs a few steps of one HIP variant and nothing else (the target of one rocprofv3 kernel trace).
"""
import argparse
import importlib
import json
import os
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

CONFIGS = {"maze": "maze_config.config_bert_maze", "synthetic": "synthetic_config.config_bert_synthetic"}
VARIANTS = (("module", "torch", None), ("hip-encoder fp32", "hip-encoder", "fp32"), ("hip-encoder bf16", "hip-encoder", "bf16"))
BATCH = 128


def stepper(mod, engine_train, precision):
    """-> (cfg, model, a closure running one training step on a fixed random minibatch)."""
    cfg = importlib.import_module("config." + mod).get_config()
    cfg.device = "cuda"
    cfg.model.engine_train = engine_train
    if precision is not None:
        cfg.model.engine_train_precision = precision
    assert cfg.loss.name == "CTElbo" and cfg.loss.one_forward_pass
    torch.manual_seed(0)
    model = mu.create_model(cfg, torch.device("cuda"))
    state = {"model": model, "optimizer": ou.get_optimizer(model.parameters(), cfg), "n_iter": 0}
    loss, step = lu.get_loss(cfg), tu.get_train_step(cfg)
    mb = torch.randint(0, cfg.data.S, (BATCH, int(cfg.model.concat_dim)), device="cuda")

    def run():
        step.step(state, loss, mb)
        state["n_iter"] += 1
    return cfg, model, run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--config", choices=sorted(CONFIGS), default="maze")
    ap.add_argument("--precision", choices=("fp32", "bf16"), default="bf16")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_bert_train.py needs a GPU")
    if a.profile:
        _, model, run = stepper(CONFIGS[a.config], "hip-encoder", a.precision)
        for _ in range(6):
            run()
        torch.cuda.synchronize()
        assert model._trainer is not None
        return
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "batch": BATCH, "step": {}}
    for key, mod in CONFIGS.items():
        variants, models = {}, {}
        for name, engine_train, precision in VARIANTS:
            _, models[name], variants[name] = stepper(mod, engine_train, precision)
        r = alternate(variants, a.reps)
        for name, engine_train, _ in VARIANTS:           # every variant ran the path it names
            assert (models[name]._trainer is not None) == (engine_train == "hip-encoder"), name
        res["step"][mod.split(".")[-1]] = r
        print(mod, json.dumps({k: (round(v["median_ms"], 3), round(v["spread"], 3)) for k, v in r.items()}), flush=True)
        del variants, models
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
