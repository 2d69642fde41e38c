"""Held-out likelihood of an absorbing-state model: bits per dimension and perplexity under both bounds of lib/likelihood.py.

    python tools/eval_likelihood.py config.maze_config.config_bert_maze_absorb [--checkpoint model_5000.pt] [--max-batches 10]
                                    [--batch-size B] [--data-root DIR] [--n-times 16] [--seed 0] [--device cuda] [--random-data N]

Builds the config's model (random init without --checkpoint, which says nothing about a trained model), walks the config's dataset
(--random-data N: N uniform random samples instead, for a dry run without the data file) and prints eval_likelihood's dict for
spacing = "alpha" (the continuous-time bound) and spacing = "grid" (the bound of the config's own AbsorbingLeap grid), one JSON
line each.  Both bounds close the chain with a sampled step at min_t; the sampler's own closing argmax has no finite bound.
"""
import argparse
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "continuous-time-diffusion-models-for-discrete-data_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("config", help="config module with get_config(), e.g. config.maze_config.config_bert_maze_absorb")
    ap.add_argument("--checkpoint")
    ap.add_argument("--max-batches", type=int)
    ap.add_argument("--batch-size", type=int)
    ap.add_argument("--data-root")
    ap.add_argument("--n-times", type=int, default=16)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--device", default="cuda" if torch.cuda.is_available() else "cpu")
    ap.add_argument("--random-data", type=int, metavar="N")
    args = ap.parse_args()
    import lib.datasets.dataset_utils as dataset_utils
    import lib.datasets.maze  # noqa: F401  (these three register the dataset classes)
    import lib.datasets.mnist  # noqa: F401
    import lib.datasets.synthetic  # noqa: F401
    import lib.likelihood as lk
    import lib.models.model_utils as model_utils
    import lib.models.models  # noqa: F401
    import lib.optimizers.optimizers  # noqa: F401
    import lib.optimizers.optimizers_utils as optimizers_utils
    import lib.utils.bookkeeping as bookkeeping
    from ctdd.config_dict import ConfigDict

    cfg = importlib.import_module(args.config).get_config()
    cfg.device = args.device
    device = torch.device(args.device)
    if device.type != "cuda":
        cfg.model.engine = "torch"
    torch.manual_seed(args.seed)
    model = model_utils.create_model(cfg, device)
    if args.checkpoint:
        state = {"model": model, "optimizer": optimizers_utils.get_optimizer(model.parameters(), cfg), "n_iter": 0}
        bookkeeping.load_state(state, args.checkpoint, device)
    model.eval()
    batch = args.batch_size or cfg.data.batch_size
    if args.random_data:
        x = torch.randint(0, cfg.data.S - 1, (args.random_data, int(cfg.model.concat_dim)))
        x = x + (x >= model.process.mask_state).long()
        loader = list(torch.split(x, batch))
    else:
        dataset = dataset_utils.get_dataset(cfg, device, args.data_root)
        loader = torch.utils.data.DataLoader(dataset, batch_size=batch, shuffle=False)
    if getattr(cfg, "eval", None) is None:
        cfg["eval"] = ConfigDict()
    for spacing in ("alpha", "grid"):
        cfg.eval.update(spacing=spacing, n_times=args.n_times, seed=args.seed)
        out = lk.eval_likelihood(cfg, model, loader, max_batches=args.max_batches)
        print(json.dumps(dict(out, spacing=spacing, config=args.config, checkpoint=args.checkpoint)))


if __name__ == "__main__":
    main()
