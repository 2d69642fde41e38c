"""Times confidence-ordered unmasking (ctdd_absorb_propose + ctdd_absorb_commit, csrc/absorb.hip) at config_bert_maze_absorb_conf's
shape (N = 128, D = 225, S = 4) and at (128, 784, 257).  GPU only.

    python tools/time_absorb_conf.py [--iters 20]

  (a) the propose + commit pair against ctdd_absorb_step alone (what the coin-per-row step costs on the same logits)
  (b) the pair against the same selection in torch device ops (log_softmax, multinomial, gather, topk, scatter; written here only)
  (c) propose alone and commit alone, the commit on the proposal's log-probability scores (which share their top key byte, so the
      first histogram pass contends on few LDS bins) against the same commit on N(0, 1) scores
  (d) a whole AbsorbingConfidence sampler step (network forward + propose + commit) against a whole AbsorbingLeap step (forward +
      step), on config_bert_maze_absorb_conf's network
Device events; everything warmed up; five alternating pairs in one process, each pair and the spread printed.
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


def pairs(label, first, second, iters, names=("pair", "other")):
    for fn in (first, second):
        for _ in range(3):
            fn()
    rows = [(timed(first, iters), timed(second, iters)) for _ in range(PAIRS)]
    for i, (f, b) in enumerate(rows):
        print(f"{label} alternation {i}: {names[0]} {f:9.4f} ms   {names[1]} {b:9.4f} ms")
    fs, bs = [r[0] for r in rows], [r[1] for r in rows]
    print(f"{label}: {names[0]} median {statistics.median(fs):.4f} ms (spread {min(fs):.4f}-{max(fs):.4f}), {names[1]} median "
          f"{statistics.median(bs):.4f} ms (spread {min(bs):.4f}-{max(bs):.4f}); {names[0]} faster in every alternation: "
          f"{all(f < b for f, b in rows)}; every {names[0]} run beats every {names[1]} run: {max(fs) < min(bs)}")


def torch_pair(logits, x, m, p, noise, changed):
    """The same selection in torch device ops, with torch's generator: candidate, log-probability, Gumbel noise, per-sample rank
    of the masked rows, the ceil(p M_n) first of them take their candidate.  No host sync."""
    N, D, S = logits.shape
    real = torch.arange(S, device=logits.device) != m
    lp = torch.log_softmax(logits.masked_fill(~real, float("-inf")), dim=-1)
    cand = torch.multinomial(lp.exp().view(-1, S), 1).view(N, D)
    score = lp.gather(-1, cand.unsqueeze(-1)).squeeze(-1)
    if noise:
        score = score - noise * torch.log(-torch.log(torch.rand_like(score)))
    masked = x == m
    k = torch.ceil(p * masked.sum(1).double()).long()
    order = torch.topk(score.masked_fill(~masked, float("-inf")), D, dim=1).indices       # masked rows first, by score
    rank = torch.empty_like(order).scatter_(1, order, torch.arange(D, device=x.device).expand(N, D))
    take = masked & (rank < k[:, None])
    changed += take.sum().to(changed.dtype)
    return torch.where(take, cand.to(x.dtype), x)


def kernels_at(native, N, D, S, m, iters):
    dev = torch.device("cuda")
    torch.manual_seed(0)
    logits = (2.0 * torch.randn((N, D, S), device=dev)).contiguous()
    x = torch.where(torch.rand((N, D), device=dev) < 0.5, torch.full((), m, device=dev), torch.randint(0, S - 1, (N, D), device=dev)).int()
    x = x.contiguous()
    changed = torch.zeros(1, dtype=torch.int32, device=dev)
    p, noise = 0.3, 0.5
    tag = f"N={N} D={D} S={S}"
    print(f"{tag}: {int((x == m).sum())} of {N * D} rows masked, p = {p}, noise = {noise}")

    def pair():
        cand, score = native.absorb_propose(logits, x, m, noise, 0, 3, 0)
        return native.absorb_commit(x, cand, score, m, p_unmask=p, changed=changed)
    pairs(f"(a) {tag} propose + commit vs ctdd_absorb_step", pair, lambda: native.absorb_step(logits, x, m, p, 0, 3, 0, changed=changed), iters,
          ("pair", "step"))
    pairs(f"(b) {tag} propose + commit vs torch ops", pair, lambda: torch_pair(logits, x, m, p, noise, changed), iters, ("pair", "torch"))
    cand, score = native.absorb_propose(logits, x, m, 0.0, 0, 3, 0)
    pairs(f"(c) {tag} propose alone vs commit alone", lambda: native.absorb_propose(logits, x, m, noise, 0, 3, 0),
          lambda: native.absorb_commit(x, cand, score, m, p_unmask=p, changed=changed), iters, ("propose", "commit"))
    normal = torch.randn((N, D), device=dev)
    pairs(f"(c) {tag} commit on log-probability scores vs on N(0, 1) scores", lambda: native.absorb_commit(x, cand, score, m, p_unmask=p),
          lambda: native.absorb_commit(x, cand, normal, m, p_unmask=p), iters, ("log-prob", "normal"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_absorb_conf.py needs a GPU (there is no CPU fallback for the kernels it times)")
    import lib.models.model_utils as model_utils
    import lib.models.models as models
    from config.maze_config.config_bert_maze_absorb_conf import get_config
    from ctdd import native

    cfg = get_config()
    S, D, N, m = cfg.data.S, cfg.model.concat_dim, cfg.data.batch_size, cfg.model.mask_state
    dev = torch.device("cuda")
    print(f"device {torch.cuda.get_device_name(0)}")
    kernels_at(native, N, D, S, m, args.iters)
    kernels_at(native, 128, 784, 257, 256, args.iters)

    # (d) a whole sampler step of each kind on the maze network
    torch.manual_seed(0)
    model = model_utils.create_model(cfg, dev)
    model.eval()
    xs = torch.where(torch.rand((N, D), device=dev) < 0.5, torch.full((), m, device=dev), torch.randint(0, S - 1, (N, D), device=dev)).int()
    xs = xs.contiguous()
    tb = torch.full((N,), 0.5, device=dev)
    changed = torch.zeros(1, dtype=torch.int32, device=dev)

    def whole(step_fn):
        def run():
            with torch.no_grad(), models.borrow_engine_output(model, uniform_time=True):
                step_fn(model(xs, tb).float().contiguous())
        return run

    def confidence(out):
        cand, score = native.absorb_propose(out, xs, m, 0.5, 0, 3, 0)
        native.absorb_commit(xs, cand, score, m, p_unmask=0.3, changed=changed)
    pairs(f"(d) whole sampler step N={N} D={D} S={S}: AbsorbingConfidence vs AbsorbingLeap", whole(confidence),
          whole(lambda out: native.absorb_step(out, xs, m, 0.3, 0, 3, 0, changed=changed)), args.iters, ("confidence", "leap"))


if __name__ == "__main__":
    main()
