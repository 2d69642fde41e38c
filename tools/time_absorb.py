"""Times the absorbing-state diffusion kernels (csrc/absorb.hip) against their torch-op statements at config_bert_maze_absorb's
shape: S = 4, D = 225, batch 128.  GPU only.

    python tools/time_absorb.py [--iters 20]

  (a) the objective alone on fixed logits (value + logit gradient): ctdd_absorb_elbo_loss vs lib.losses.losses._absorbing_elbo_terms
  (b) the reverse step alone on fixed logits: ctdd_absorb_step vs torch ops (softmax over s != m, multinomial, where)
  (c) a whole Standard.step: cfg.loss.fused = True vs False (noising and objective; the network is the same)
  (d) a whole sampler step (network forward + step), both ways
Device events; everything warmed up; five alternating (fused, fallback) pairs in one process, each pair and the spread printed.
For (a) and (b) also the kernel's bytes, from the shapes, over its time.
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
        print(f"{label} pair {i}: fused {f:9.4f} ms   fallback {b:9.4f} ms")
    fs, bs = [r[0] for r in rows], [r[1] for r in rows]
    wins = max(fs) < min(bs)
    print(f"{label}: fused median {statistics.median(fs):.4f} ms (spread {min(fs):.4f}-{max(fs):.4f}), fallback median "
          f"{statistics.median(bs):.4f} ms (spread {min(bs):.4f}-{max(bs):.4f}), every fused run beats every fallback run: {wins}")
    return statistics.median(fs), statistics.median(bs)


def torch_step(logits, x, m, p, changed):
    """The reverse step in torch ops: what ctdd_absorb_step computes, with torch's generator."""
    S = logits.shape[-1]
    real = torch.arange(S, device=logits.device) != m
    probs = torch.softmax(logits.masked_fill(~real, float("-inf")), dim=-1)
    draw = torch.multinomial(probs.view(-1, S), 1).view(x.shape).to(x.dtype)
    unmask = (x == m) & (torch.rand(x.shape, device=x.device) < p)
    changed += unmask.sum().to(changed.dtype)
    return torch.where(unmask, draw, x)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_absorb.py needs a GPU (there is no CPU fallback for the kernels it times)")
    import lib.losses.losses as losses
    import lib.losses.losses_utils as losses_utils
    import lib.models.model_utils as model_utils
    import lib.models.models as models
    import lib.optimizers.optimizers  # noqa: F401
    import lib.optimizers.optimizers_utils as optimizers_utils
    import lib.training.training  # noqa: F401
    import lib.training.training_utils as training_utils
    from config.maze_config.config_bert_maze_absorb import get_config
    from ctdd import native

    cfg = get_config()
    S, D, B, m = cfg.data.S, cfg.model.concat_dim, cfg.data.batch_size, cfg.model.mask_state
    dev = torch.device("cuda")
    print(f"device {torch.cuda.get_device_name(0)}; S={S} D={D} batch={B} mask_state={m}")
    torch.manual_seed(0)
    x0 = torch.randint(0, S - 1, (B, D), device=dev)
    ts = torch.rand(B, device=dev) * 0.98 + 0.01
    alpha = 1 - (1 - cfg.model.alpha_eps) * ts
    x_t = native.absorb_noise(x0.int(), alpha.float().contiguous(), m, seed=1)
    w = (1 / ts).float().contiguous()
    nll_scale = cfg.loss.nll_weight / (B * D)
    n_masked = int((x_t == m).sum())

    # (a) the objective alone
    logits = (2.0 * torch.randn((B, D, S), device=dev)).requires_grad_(True)
    x0i, xti, xtl = x0.int(), x_t.int().contiguous(), x_t.long()

    def obj_fused():
        logits.grad = None
        losses._HipValueGrad.apply(logits, lambda lg: native.absorb_elbo_loss(lg, x0i, xti, w, nll_scale, m)).backward()

    def obj_fall():
        logits.grad = None
        losses._absorbing_elbo_terms(logits, x0, xtl, w, nll_scale, m).backward()
    fa, _ = pairs("(a) objective, value + logit gradient", obj_fused, obj_fall, args.iters)
    rows_read = B * D if nll_scale else n_masked
    bytes_a = 4 * (rows_read * S + B * D * S + 2 * B * D + B)
    print(f"(a) kernel bytes {bytes_a} ({rows_read} rows read, {B * D} gradient rows written, x0, x_t, w): {bytes_a / fa / 1e6:.2f} GB/s over the "
          f"fused time (which includes the autograd wrapper and the output allocations)")

    # (b) the step alone
    lg = logits.detach().contiguous()
    p = 0.3
    changed = torch.zeros(1, dtype=torch.int32, device=dev)
    fb, _ = pairs("(b) reverse step", lambda: native.absorb_step(lg, xti, m, p, 0, 3, 0, changed=changed),
                  lambda: torch_step(lg, xti, m, p, changed), args.iters)
    bytes_b = 4 * (2 * B * D + int(p * n_masked) * S)
    print(f"(b) kernel bytes {bytes_b} (x read, x written, ~{int(p * n_masked)} unmasking rows read): {bytes_b / fb / 1e6:.2f} GB/s over the fused time")

    # (c) a whole Standard.step
    model = model_utils.create_model(cfg, dev)
    state = {"model": model, "optimizer": optimizers_utils.get_optimizer(model.parameters(), cfg), "n_iter": 0}
    step = training_utils.get_train_step(cfg)
    cfg_fb = get_config()
    cfg_fb.loss.fused = False
    lf, lb = losses_utils.get_loss(cfg), losses_utils.get_loss(cfg_fb)
    img = x0.view(B, *cfg.data.shape)
    pairs("(c) Standard.step", lambda: step.step(state, lf, img), lambda: step.step(state, lb, img), max(args.iters // 4, 2))

    # (d) a whole sampler step
    model.eval()
    N = B
    xs = xti.clone()
    tb = torch.full((N,), 0.5, device=dev)

    def whole(step_fn):
        def run():
            with torch.no_grad(), models.borrow_engine_output(model, uniform_time=True):
                out = model(xs, tb).float().contiguous()
                step_fn(out)
        return run
    pairs("(d) whole sampler step", whole(lambda out: native.absorb_step(out, xs, m, p, 0, 3, 0, changed=changed)),
          whole(lambda out: torch_step(out, xs, m, p, changed)), args.iters)


if __name__ == "__main__":
    main()
