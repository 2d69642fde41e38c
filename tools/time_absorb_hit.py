"""Times the first-hitting step (ctdd_absorb_hit_time, ctdd_absorb_hit_step; csrc/absorb.hip) at config_bert_maze_absorb_hit's shape
(N = 128, D = 225, S = 4) and at (128, 784, 257).  GPU only.

    python tools/time_absorb_hit.py [--iters 20] [--kmax 1]

  (a) the two launches (per-sample masked count, level recursion and evaluation time; uniform selection of the events' rows and their
      draw) against the same update in torch device ops (written here only): the masked count, the cumulative log-uniform recursion,
      a random top-k through argsort, a softmax draw
  (b) a whole AbsorbingFirstHit iteration (hit_time + network forward with per-sample times + hit_step) against a whole AbsorbingLeap
      step (forward with one time + ctdd_absorb_step), on config_bert_maze_absorb_hit's network at its shape, and on the same network
      rebuilt for D = 784, S = 257
Device events; everything warmed up; five alternating pairs in one process, each pair and the spread printed.
"""
import argparse
import math
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


def pairs(label, first, second, iters, names):
    for fn in (first, second):
        for _ in range(3):
            fn()
    rows = [(timed(first, iters), timed(second, iters)) for _ in range(PAIRS)]
    for i, (f, b) in enumerate(rows):
        print(f"{label} alternation {i}: {names[0]} {f:9.4f} ms   {names[1]} {b:9.4f} ms")
    fs, bs = [r[0] for r in rows], [r[1] for r in rows]
    print(f"{label}: {names[0]} median {statistics.median(fs):.4f} ms (spread {min(fs):.4f}-{max(fs):.4f}), {names[1]} median "
          f"{statistics.median(bs):.4f} ms (spread {min(bs):.4f}-{max(bs):.4f}); {names[0]} faster in every alternation: "
          f"{all(f < b for f, b in rows)}; every {names[0]} run beats every {names[1]} run: {max(fs) < min(bs)}; "
          f"difference of the medians {statistics.median(fs) - statistics.median(bs):+.4f} ms against the larger spread "
          f"{max(max(fs) - min(fs), max(bs) - min(bs)):.4f} ms")


def torch_step(logits, x, logc, m, kmax, log_cmin, t_of_c, t_min, t_max, changed):
    """The same update in torch device ops, with torch's generator: the masked count per sample, kmax cumulative log-uniform events
    with the closing level, the first event's time, a uniform top-k of the masked rows through argsort of random keys, a softmax draw
    for every row (multinomial has no row subset) and the select.  No host sync."""
    N, D, S = logits.shape
    masked = x == m
    M = masked.sum(1)
    i = torch.arange(kmax, device=x.device)
    left = (M.unsqueeze(1) - i).clamp_min(1).to(torch.float64)
    steps = torch.log(torch.rand((N, kmax), device=x.device, dtype=torch.float64)) / left
    levels = logc.unsqueeze(1) + torch.cumsum(steps, 1)
    ok = torch.cumprod(((levels >= log_cmin) & (i < M.unsqueeze(1))).to(torch.int32), 1)
    counts = ok.sum(1)
    refused = counts < torch.minimum(M, torch.full_like(M, kmax))
    last = torch.where(counts > 0, levels.gather(1, (counts - 1).clamp_min(0).unsqueeze(1)).squeeze(1), logc)
    logc_out = torch.where(refused, torch.full_like(logc, log_cmin), last)
    t_eval = torch.where(counts > 0, t_of_c(torch.exp(levels[:, 0])).clamp(t_min, t_max), torch.full_like(logc, t_min)).float()
    keys = torch.where(masked, torch.rand((N, D), device=x.device), torch.full((), -1.0, device=x.device))
    rank = torch.argsort(torch.argsort(keys, dim=1, descending=True), dim=1)
    take = masked & (rank < counts.unsqueeze(1))
    real = torch.arange(S, device=logits.device) != m
    cand = torch.multinomial(torch.softmax(logits.masked_fill(~real, float("-inf")), dim=-1).view(-1, S), 1).view(N, D)
    changed += take.sum().to(changed.dtype)
    return torch.where(take, cand.to(x.dtype), x), logc_out, t_eval


def kernels_at(native, N, D, S, m, kmax, iters):
    dev = torch.device("cuda")
    torch.manual_seed(0)
    logits = (2.0 * torch.randn((N, D, S), device=dev)).contiguous()
    x = torch.where(torch.rand((N, D), device=dev) < 0.5, torch.full((), m, device=dev), torch.randint(0, S - 1, (N, D), device=dev)).int()
    x = x.contiguous()
    sched = dict(t_func="loglinear", rate_const=1.0, alpha_eps=1e-3)
    logc = torch.full((N,), math.log(0.5), dtype=torch.float64, device=dev)
    log_cmin, t_min, t_max = math.log((1 - 1e-3) * 0.007), 0.007, 0.995
    counts = torch.empty((N,), dtype=torch.int32, device=dev)
    t_eval = torch.empty((N,), device=dev)
    out = torch.empty_like(logc)
    changed = torch.zeros(1, dtype=torch.int32, device=dev)
    tag = f"N={N} D={D} S={S} kmax={kmax}"
    print(f"{tag}: {int((x == m).sum())} masked of {N * D} rows")

    def fused():
        native.absorb_hit_time(x, logc, m, kmax, log_cmin, sched, t_min, t_max, 3, 0, counts=counts, t_eval=t_eval, out=out)
        return native.absorb_hit_step(logits, x, counts, m, 0, 3, 0, changed=changed)

    pairs(f"(a) {tag} hit_time + hit_step vs torch ops", fused,
          lambda: torch_step(logits, x, logc, m, kmax, log_cmin, lambda c: c / (1 - 1e-3), t_min, t_max, changed), iters, ("fused", "torch"))


def iteration_at(native, models, model, N, D, S, m, kmax, iters, tag):
    dev = torch.device("cuda")
    xs = torch.where(torch.rand((N, D), device=dev) < 0.5, torch.full((), m, device=dev), torch.randint(0, S - 1, (N, D), device=dev)).int()
    xs = xs.contiguous()
    pr = model.process
    logc = torch.full((N,), math.log(0.5), dtype=torch.float64, device=dev)
    log_cmin = float(torch.log(1 - pr.alpha(torch.tensor(0.007, dtype=torch.float64))))
    counts = torch.empty((N,), dtype=torch.int32, device=dev)
    t_eval = torch.empty((N,), device=dev)
    out = torch.empty_like(logc)
    tb = torch.full((N,), 0.5, device=dev)
    changed = torch.zeros(1, dtype=torch.int32, device=dev)

    def hit():
        with torch.no_grad(), models.borrow_engine_output(model, uniform_time=False):
            native.absorb_hit_time(xs, logc, m, kmax, log_cmin, pr.p, 0.007, 0.995, 3, 0, counts=counts, t_eval=t_eval, out=out)
            native.absorb_hit_step(model(xs, t_eval).float().contiguous(), xs, counts, m, 0, 3, 0, changed=changed)

    def leap():
        with torch.no_grad(), models.borrow_engine_output(model, uniform_time=True):
            native.absorb_step(model(xs, tb).float().contiguous(), xs, m, 0.3, 0, 3, 0, changed=changed)

    pairs(f"(b) whole sampler iteration {tag} kmax={kmax}: AbsorbingFirstHit vs AbsorbingLeap", hit, leap, iters, ("hit", "leap"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--kmax", type=int, default=1, help="events per forward (1: the exact sampler)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_absorb_hit.py needs a GPU (there is no CPU fallback for the kernels it times)")
    import lib.models.model_utils as model_utils
    import lib.models.models as models
    from config.maze_config.config_bert_maze_absorb_hit import get_config
    from ctdd import native

    cfg = get_config()
    S, D, N, m = cfg.data.S, cfg.model.concat_dim, cfg.data.batch_size, cfg.model.mask_state
    dev = torch.device("cuda")
    print(f"device {torch.cuda.get_device_name(0)}")
    kernels_at(native, N, D, S, m, args.kmax, args.iters)
    kernels_at(native, 128, 784, 257, 256, args.kmax, args.iters)

    torch.manual_seed(0)
    model = model_utils.create_model(cfg, dev)
    model.eval()
    iteration_at(native, models, model, N, D, S, m, args.kmax, args.iters, f"N={N} D={D} S={S}")
    big = get_config()                                                   # the same network at the second shape
    big.data.update(S=257, shape=[1, 28, 28], image_size=28)
    big.model.update(concat_dim=784, mask_state=256, out_dim=257, readout_dim=257)
    try:
        wide = model_utils.create_model(big, dev)
        wide.eval()
        with torch.no_grad():
            wide(torch.zeros((128, 784), dtype=torch.int32, device=dev), torch.full((128,), 0.5, device=dev))
        torch.cuda.synchronize()
    except (RuntimeError, ValueError, native.CtddError) as e:            # a shape the encoder's engine does not take: say so, do not guess
        print(f"(b) whole sampler iteration N=128 D=784 S=257: not measured -- the network does not build at this shape: {e}")
        return
    iteration_at(native, models, wide, 128, 784, 257, 256, args.kmax, args.iters, "N=128 D=784 S=257")


if __name__ == "__main__":
    main()
