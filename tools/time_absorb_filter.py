"""Times the temperature / top-k / top-p filter of the absorbing samplers (ctdd_absorb_filter; csrc/absorb.hip) at
config_bert_maze_absorb's shape (N = 128, D = 225, S = 4) and at (128, 784, 257).  GPU only.

    python tools/time_absorb_filter.py [--iters 20] [--temperature 0.7] [--top-k 0] [--top-p 0.9]

  (a) the filter launch against the same filtering in torch device ops (written here only): divide, sort, softmax, cumsum,
      scatter, select the masked rows
  (b) a whole AbsorbingLeap iteration with the filter (network forward + ctdd_absorb_filter + ctdd_absorb_step) against one without,
      on config_bert_maze_absorb's network at its shape, and on the same network rebuilt for D = 784, S = 257
Both at the first step of a trajectory (every row masked: the filter reads and writes every row) and at a mid-trajectory step (half
the rows masked).  Device events; everything warmed up; five alternating pairs in one process, each pair and the spread printed.
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
SHARES = (("first step (all rows masked)", 1.0), ("mid-trajectory step (half the rows masked)", 0.5))


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


def torch_filter(logits, x, m, T, k, p):
    """The same filtering in torch device ops, out of place: every row is filtered (the ops have no row subset), the masked rows are
    selected at the end.  No host sync."""
    N, D, S = logits.shape
    v = logits / T
    v[..., m] = float("-inf")
    vs, idx = torch.sort(v, dim=-1, descending=True, stable=True)
    keep = torch.ones_like(vs, dtype=torch.bool)
    if 0 < k < S - 1:
        keep[..., k:] = False
    if p < 1.0:
        w = torch.softmax(vs.masked_fill(~keep, float("-inf")), dim=-1)
        before = torch.cumsum(w, dim=-1) - w
        keep &= before < p
    out = torch.full_like(v, float("-inf")).scatter(-1, idx, vs.masked_fill(~keep, float("-inf")))
    return torch.where((x == m).unsqueeze(-1), out, logits)


def states(N, D, S, m, share, dev):
    x = torch.where(torch.rand((N, D), device=dev) < share, torch.full((), m, device=dev), torch.randint(0, S - 1, (N, D), device=dev))
    return x.int().contiguous()


def kernels_at(native, N, D, S, m, T, k, p, iters):
    dev = torch.device("cuda")
    torch.manual_seed(0)
    logits = (3.0 * torch.randn((N, D, S), device=dev)).contiguous()
    work = logits.clone()
    for name, share in SHARES:
        x = states(N, D, S, m, share, dev)
        tag = f"N={N} D={D} S={S} T={T} top_k={k} top_p={p}, {name}"
        print(f"{tag}: {int((x == m).sum())} masked of {N * D} rows")

        def fused():
            # (out of place into a second buffer: the reads and writes of the in-place call, on the same logits every time)
            native.absorb_filter(logits, x, m, T, k, p, out=work)

        pairs(f"(a) {tag}: ctdd_absorb_filter vs torch ops", fused, lambda: torch_filter(logits, x, m, T, k, p), iters,
              ("filter", "torch"))


def iteration_at(native, models, model, N, D, S, m, T, k, p, iters, tag):
    dev = torch.device("cuda")
    tb = torch.full((N,), 0.5, device=dev)
    changed = torch.zeros(1, dtype=torch.int32, device=dev)
    for name, share in SHARES:
        xs = states(N, D, S, m, share, dev)

        def filtered():
            with torch.no_grad(), models.borrow_engine_output(model, uniform_time=True):
                logits = model(xs, tb).float().contiguous()
                native.absorb_filter(logits, xs, m, T, k, p, out=logits)
                native.absorb_step(logits, xs, m, 0.3, 0, 3, 0, changed=changed)

        def plain():
            with torch.no_grad(), models.borrow_engine_output(model, uniform_time=True):
                native.absorb_step(model(xs, tb).float().contiguous(), xs, m, 0.3, 0, 3, 0, changed=changed)

        pairs(f"(b) whole AbsorbingLeap iteration {tag}, {name}: with the filter vs without", filtered, plain, iters, ("filtered", "plain"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--temperature", type=float, default=0.7)
    ap.add_argument("--top-k", type=int, default=0)
    ap.add_argument("--top-p", type=float, default=0.9)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_absorb_filter.py needs a GPU (there is no CPU fallback for the kernels it times)")
    import lib.models.model_utils as model_utils
    import lib.models.models as models
    from config.maze_config.config_bert_maze_absorb import get_config
    from ctdd import native

    cfg = get_config()
    S, D, N, m = cfg.data.S, cfg.model.concat_dim, cfg.data.batch_size, cfg.model.mask_state
    T, k, p = args.temperature, args.top_k, args.top_p
    dev = torch.device("cuda")
    print(f"device {torch.cuda.get_device_name(0)}")
    kernels_at(native, N, D, S, m, T, k, p, args.iters)
    kernels_at(native, 128, 784, 257, 256, T, k, p, args.iters)

    torch.manual_seed(0)
    model = model_utils.create_model(cfg, dev)
    model.eval()
    iteration_at(native, models, model, N, D, S, m, T, k, p, args.iters, f"N={N} D={D} S={S}")
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
        print(f"(b) whole AbsorbingLeap iteration N=128 D=784 S=257: not measured -- the network does not build at this shape: {e}")
        return
    iteration_at(native, models, wide, 128, 784, 257, 256, T, k, p, args.iters, "N=128 D=784 S=257")


if __name__ == "__main__":
    main()
