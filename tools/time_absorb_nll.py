"""Times the held-out likelihood kernel pair (ctdd_absorb_nll, csrc/absorb.hip) against the same per-sample sums in torch ops, and a
whole "alpha" evaluation (lib/likelihood.py) fused against fused = False.  GPU only.

    python tools/time_absorb_nll.py [--iters 20]

  (a) the call alone on fixed logits, half the rows masked, with both counters: native.absorb_nll vs torch ops in fp64 (what
      fused = False runs: lib.likelihood._terms_torch) and vs torch ops in fp32 with an fp64 sum, at (N, D, S) =
      (128, 225, S of config_bert_maze_absorb) and (128, 784, 257); and the call with against without its two counters
  (b) absorbing_nll_bound(spacing="alpha", n_times=16) on one batch of config_bert_maze_absorb (random-init network): fused vs fused=False
Device events; everything warmed up; five alternating (fused, torch) pairs in one process, each pair and the spread printed.  For (a)
also the kernels' bytes, from the shapes, over the fused time.
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "continuous-time-diffusion-models-for-discrete-data_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

PAIRS = 5


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def pairs(label, fused, fallback, iters):
    for fn in (fused, fallback):
        for _ in range(3):
            fn()
    rows = [(timed(fused, iters), timed(fallback, iters)) for _ in range(PAIRS)]
    for i, (f, b) in enumerate(rows):
        print(f"{label} pair {i}: fused {f:9.4f} ms   torch {b:9.4f} ms")
    fs, bs = [r[0] for r in rows], [r[1] for r in rows]
    wins = max(fs) < min(bs)
    print(f"{label}: fused median {statistics.median(fs):.4f} ms (spread {min(fs):.4f}-{max(fs):.4f}), torch median "
          f"{statistics.median(bs):.4f} ms (spread {min(bs):.4f}-{max(bs):.4f}), every fused run beats every torch run: {wins}")
    return statistics.median(fs), statistics.median(bs)


def terms_fp32(logits, x0, xt, m, w):
    """The per-sample sums and counters in fp32 torch ops (row terms in fp32, summed in fp64)."""
    real = torch.arange(logits.shape[-1], device=logits.device) != m
    l = logits.masked_fill(~real, float("-inf"))
    term = (xt == m) & (x0 != m)
    idx = torch.where(term, x0, torch.full_like(x0, (m + 1) % logits.shape[-1])).long()
    nlp = -torch.log_softmax(l, -1).gather(-1, idx.unsqueeze(-1)).squeeze(-1)
    rows = torch.where(term, nlp, torch.zeros_like(nlp))
    return w.double() * rows.double().sum(1), term.sum(1), (term & (l.argmax(-1) == idx)).sum(1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_absorb_nll.py needs a GPU (there is no CPU fallback for the kernels it times)")
    import lib.likelihood as lk
    import lib.models.model_utils as model_utils
    import lib.models.models  # noqa: F401
    from config.maze_config.config_bert_maze_absorb import get_config
    from ctdd import native

    cfg = get_config()
    dev = torch.device("cuda")
    print(f"device {torch.cuda.get_device_name(0)}")

    # (a) the call alone
    for N, D, S in ((cfg.data.batch_size, cfg.model.concat_dim, cfg.data.S), (128, 784, 257)):
        m = S - 1
        torch.manual_seed(0)
        logits = (2.0 * torch.randn((N, D, S), device=dev)).contiguous()
        x0 = torch.randint(0, S - 1, (N, D), device=dev, dtype=torch.int32)
        xt = native.absorb_noise(x0, torch.full((N,), 0.5, device=dev), m, seed=1)
        w = (0.5 + torch.rand(N, device=dev)).contiguous()
        out = torch.zeros(N, dtype=torch.float64, device=dev)
        masked, hit = (torch.zeros(N, dtype=torch.int32, device=dev) for _ in range(2))
        n_masked = int((xt == m).sum())
        label = f"(a) N={N} D={D} S={S}"
        want, _, _ = lk._terms_torch(logits, x0, xt, m, w)
        _, got = native.absorb_nll(logits, x0, xt, m, w=w)
        print(f"{label}: {n_masked} of {N * D} rows masked; fused against fp64 torch ops, largest relative difference "
              f"{float(((got - want).abs() / want.abs().clamp(min=1.0)).max()):.2e}")
        fused = lambda: native.absorb_nll(logits, x0, xt, m, w=w, out=out, masked=masked, hit=hit)
        fa, _ = pairs(label + " vs torch fp64", fused, lambda: lk._terms_torch(logits, x0, xt, m, w), args.iters)
        pairs(label + " vs torch fp32", fused, lambda: terms_fp32(logits, x0, xt, m, w), args.iters)
        pairs(label + " with / without the two counters (second column: without)", fused,
              lambda: native.absorb_nll(logits, x0, xt, m, w=w, out=out), args.iters)
        nbytes = 4 * (n_masked * S + 2 * N * D + 2 * N * D + N) + 8 * 2 * N
        print(f"{label}: kernel bytes {nbytes} ({n_masked} rows read, x0, x_t, row_nll written and read back, w, out): "
              f"{nbytes / fa / 1e6:.2f} GB/s over the fused time (two launches and the row_nll allocation included)")

    # (b) a whole "alpha" evaluation of one batch
    N, D, S = cfg.data.batch_size, cfg.model.concat_dim, cfg.data.S
    torch.manual_seed(0)
    model = model_utils.create_model(cfg, dev)
    model.eval()
    x0 = torch.randint(0, S - 1, (N, D), device=dev)
    kw = dict(spacing="alpha", n_times=16, min_t=cfg.sampler.min_t, max_t=cfg.training.max_t, seed=3)
    a, b = lk.absorbing_nll_bound(model, x0, **kw), lk.absorbing_nll_bound(model, x0, fused=False, **kw)
    print(f"(b) bits per dimension fused {float(a.bits_per_dim.mean()):.6f}, fused=False {float(b.bits_per_dim.mean()):.6f}; largest "
          f"per-sample difference {float((a.nll - b.nll).abs().max()):.2e} nats")
    pairs(f"(b) alpha evaluation, 17 forwards, N={N} D={D} S={S}", lambda: lk.absorbing_nll_bound(model, x0, **kw),
          lambda: lk.absorbing_nll_bound(model, x0, fused=False, **kw), max(args.iters // 4, 2))


if __name__ == "__main__":
    main()
