"""Conditional training on the MNIST shapes (B = 64, D = 784, condition_dim = 392, S = 256), two measurements:

1. the objective: K11 on the window of free rows, in place (ctdd_ctelbo_loss_window), against what it replaces -- copy
   logits[:, 392:] to a contiguous tensor, ctdd_ctelbo_loss_terms on it, scatter the gradient into a zero-filled full tensor --
   and, for scale, the dense objective on all 784 rows.  The two conditional paths must agree bit for bit.  Next to them K11
   under a per-sample mask (ctdd_ctelbo_loss_masked) with the same prefix as a mask, and with one draw of the shipped mixture.
2. one Standard.step of config_tauUnet_mnist_cond (CondCTElbo) against one of config_tauUnet_mnist (CTElbo), and of InpaintCTElbo
   with the same prefix as its mask and with the mixture of config_tauUnet_mnist_inpaint, random-init weights.

The compared cases alternate inside every repeat; a repeat is a device-synchronised window of `--iters` calls after a warm-up of
every case.  Reported: the median over the repeats and their min .. max (the run-to-run spread on this box).

    python tools/time_cond_loss.py [--repeats 7] [--iters 400] [--steps 30] [--only objective|step]
    rocprofv3 --kernel-trace --stats --output-format csv -d prof_out/obj -o obj -- python tools/time_cond_loss.py --profile masked-prefix
--profile CASE (window | dense | masked-prefix | masked-mixture) runs `--iters` calls of that objective and nothing else.
"""
import argparse
import os
import statistics
import sys
import time

_R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [_R, os.path.join(_R, "continuous-time-diffusion-models-for-discrete-data_amd")]

B, DL, K, S = 64, 784, 392, 256


def _window(torch, fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def _alternate(torch, cases, repeats, iters, unit=1e6):
    """cases: {name: fn}.  Returns {name: (median, min, max)} in `unit`-ths of a second per call."""
    for fn in cases.values():                                    # warm-up: code objects, allocator, plans
        for _ in range(3):
            fn()
    out = {k: [] for k in cases}
    for _ in range(repeats):
        for k, fn in cases.items():
            out[k].append(_window(torch, fn, iters) * unit)
    return {k: (statistics.median(v), min(v), max(v)) for k, v in out.items()}


def objective(torch, repeats, iters, profile=None):
    from ctdd import native
    from ctdd.process import DeviceForwardProcess
    gen = torch.Generator().manual_seed(0)
    proc = DeviceForwardProcess("gaussian", S, "cuda", rate_sigma=6.0, Q_sigma=512.0, time_exp=100.0, time_base=3.0)
    ts = (torch.rand(B, generator=gen) * 0.99 + 0.01).cuda()
    qt0, qT, rate, probs = proc.tables(ts, want_qt0=True, want_qt0T=True, want_rate=True, want_noise_probs=True)
    x0 = torch.randint(0, S, (B, DL), generator=gen).to(torch.int32).cuda()
    x_t = native.noise_categorical(probs, x0, seed=1)
    _, _, x_tilde = native.xtilde_sample(rate, x_t, seed=2)
    logits = (torch.randn(B, DL, S, generator=gen) * 2.0).cuda()
    x0w, xtw = x0[:, K:].contiguous(), x_tilde[:, K:].contiguous()
    nll = 0.001 / (B * (DL - K))

    def window():
        return native.ctelbo_loss_window(logits, x0w, xtw, qt0, qT, rate, 1e-9, 1.0, 1.0, nll, K)

    def slice_pad():
        v, g = native.ctelbo_loss(logits[:, K:].contiguous(), x0w, xtw, qt0, qT, rate, 1e-9, 1.0, nll, reg_scale=1.0)
        full = torch.zeros_like(logits)
        full[:, K:] = g
        return v, full

    def dense():
        return native.ctelbo_loss(logits, x0, x_tilde, qt0, qT, rate, 1e-9, 1.0, 0.001 / (B * DL))

    # the masked entry: full-shape states (held entries at x0), the prefix as a mask and one draw of the shipped mixture
    import lib.losses.masks as masks
    from config.mnist_config.config_tauUnet_mnist_inpaint import get_config as inpaint
    free_p = torch.ones(B, DL, dtype=torch.bool)
    free_p[:, :K] = False
    torch.manual_seed(0)
    free_m = masks.sample_free(inpaint(), B, DL)
    share = free_m.float().mean().item()

    def masked_case(free_host):
        free = free_host.cuda()
        xt_f = torch.where(free, x_t, x0)
        _, _, xtl_f = native.xtilde_sample_masked(rate, xt_f, free, seed=2)
        nll_m = 0.001 / int(free_host.sum())
        return lambda: native.ctelbo_loss_masked(logits, x0, xtl_f, free, qt0, qT, rate, 1e-9, 1.0, 1.0, nll_m)

    masked_prefix, masked_mix = masked_case(free_p), masked_case(free_m)
    if profile is not None:
        fn = {"window": window, "dense": dense, "masked-prefix": masked_prefix, "masked-mixture": masked_mix}[profile]
        print(f"{profile}: {iters} calls, {_window(torch, fn, iters) * 1e6:.1f} us per call under the profiler")
        return
    (v1, g1), (v2, g2) = window(), slice_pad()
    assert torch.equal(v1, v2) and torch.equal(g1, g2), "the window entry and slice-copy-and-pad must agree bit for bit"
    res = _alternate(torch, {"window, in place": window, "slice copy + K11 + zero-pad scatter": slice_pad, "dense K11, all 784 rows": dense,
                             "masked, prefix 392 as a mask": masked_prefix, f"masked, mixture draw ({100 * share:.0f} % free)": masked_mix},
                     repeats, iters)
    print(f"objective, B {B}, D {DL}, condition_dim {K}, S {S}: {repeats} repeats x {iters} calls, us per call (median, min .. max)")
    for k, (med, lo, hi) in res.items():
        print(f"  {k:38s} {med:8.1f}  ({lo:.1f} .. {hi:.1f})")
    scratch = lambda d: int(native.load().ctdd_ctelbo_scratch_bytes(B, d, S)) / 2**20
    print(f"  scratch: window {scratch(DL - K):.1f} MiB, dense {scratch(DL):.1f} MiB; slice-copy-and-pad adds the slice and its gradient, "
          f"{2 * B * (DL - K) * S * 4 / 2**20:.1f} MiB")


def train_step(torch, repeats, steps):
    import lib.models.models, lib.losses.losses, lib.training.training, lib.optimizers.optimizers  # noqa: F401, E401
    import lib.models.model_utils as mu
    import lib.losses.losses_utils as lu
    import lib.training.training_utils as tu
    import lib.optimizers.optimizers_utils as ou
    from config.mnist_config.config_tauUnet_mnist import get_config as base
    from config.mnist_config.config_tauUnet_mnist_cond import get_config as cond
    from config.mnist_config.config_tauUnet_mnist_inpaint import get_config as inpaint

    def inpaint_prefix():
        c = inpaint()
        c.loss.update(mask="prefix", condition_dim=K)
        return c
    mb = torch.randint(0, S, (B, 1, 28, 28), device="cuda")
    cases = {}
    for name, get in (("CTElbo         (config_tauUnet_mnist)", base), ("CondCTElbo     (config_tauUnet_mnist_cond)", cond),
                      ("InpaintCTElbo  (mask = prefix 392)", inpaint_prefix), ("InpaintCTElbo  (config_tauUnet_mnist_inpaint)", inpaint)):
        cfg = get()
        torch.manual_seed(0)
        model = mu.create_model(cfg, torch.device("cuda"))
        state = {"model": model, "optimizer": ou.get_optimizer(model.parameters(), cfg), "n_iter": 0}
        step, loss = tu.get_train_step(cfg), lu.get_loss(cfg)

        def one(state=state, step=step, loss=loss):
            step.step(state, loss, mb)
            state["n_iter"] += 1
        cases[name] = one
    res = _alternate(torch, cases, repeats, steps, unit=1e3)
    print(f"Standard.step, batch {B}: {repeats} repeats x {steps} steps, ms per step (median, min .. max)")
    for k, (med, lo, hi) in res.items():
        print(f"  {k:42s} {med:7.2f}  ({lo:.2f} .. {hi:.2f})")
    (b_med, b_lo, b_hi), (c_med, _, _), (p_med, _, _), (m_med, _, _) = res.values()
    print(f"  conditional / unconditional = {c_med / b_med:.3f}; spread of the unconditional step {100 * (b_hi - b_lo) / b_med:.1f} %")
    print(f"  InpaintCTElbo / CondCTElbo: prefix mask {p_med / c_med:.3f}, mixture {m_med / c_med:.3f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=400)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--only", choices=("objective", "step"), default=None)
    ap.add_argument("--profile", choices=("window", "dense", "masked-prefix", "masked-mixture"), default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("time_cond_loss.py measures on the GPU: no device found")
    print(torch.cuda.get_device_name(0))
    if a.profile is not None:
        return objective(torch, a.repeats, a.iters, a.profile)
    if a.only != "step":
        objective(torch, a.repeats, a.iters)
    if a.only != "objective":
        train_step(torch, a.repeats, a.steps)


if __name__ == "__main__":
    main()
