"""Regenerate tests/golden/cond_losses.npz: the reference's prefix-conditioned CT-ELBO (CondCTElbo.calc_loss) on the toy score
function, with the noise it drew.

Runs only where the reference checkout is present: it is imported through oracle/stubs with the helpers of oracle/gen_golden.py.
Per case: x0, ts, x_t, x~ (the three Categorical.sample calls of the loss are recorded while it runs; x~ is also what reached the
model), the reference's fp32 loss, and the value and d/dtheta of the restatement in fp64 -- oracle.losses.neg_ct_elbo on the free
rows plus the cross entropy on the signal forward's logits -- with theta scaling the toy logits.  The file holds data only.

    python tools/gen_golden_cond.py
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from oracle.gen_golden import base_cfg, make_ref_model, ref_losses, save  # noqa: E402  (puts the reference and its stubs on sys.path)
from oracle.losses import neg_ct_elbo  # noqa: E402
from oracle.toy_model import toy_logits  # noqa: E402

THETA, SEED = 1.5, 777
#        tag     kind        S    B  D    k  one_forward_pass nll_weight
CASES = (("g16b", "gaussian", 16, 4, 12, 5, False, 0.5),
         ("g256", "gaussian", 256, 3, 21, 4, True, 0.001),
         ("u3", "uniform", 3, 5, 15, 7, False, 0.1),
         ("g32", "gaussian", 32, 2, 140, 3, True, 0.01),
         ("g16", "gaussian", 16, 4, 12, 5, True, 0.001))


def main():
    arrs = {}
    for tag, kind, S, B, D, k, one_pass, nllw in CASES:
        cfg = base_cfg(S, D)
        cfg.loss.update(dict(name="CondCTElbo", one_forward_pass=one_pass, nll_weight=nllw, condition_dim=k))
        model = make_ref_model(kind, cfg)
        theta = torch.tensor(THETA, requires_grad=True)
        base_call = model.__class__.__call__

        def call(self, x, t, *a, _th=theta, _S=S):
            self.calls.append((x.clone(), t.clone()))
            return toy_logits(x, t, _S, 1.0) * _th
        model.__class__.__call__ = call
        loss = ref_losses.CondCTElbo(cfg)
        x0 = torch.randint(0, S, (B, D), generator=torch.Generator().manual_seed(17))
        Cat = torch.distributions.categorical.Categorical
        draws, cat_sample = [], Cat.sample

        def sample(self, *a, **kw):
            out = cat_sample(self, *a, **kw)
            draws.append(out.clone())
            return out
        Cat.sample = sample
        try:
            torch.manual_seed(SEED)
            val = loss.calc_loss(x0.clone(), {"model": model, "n_iter": 0})
        finally:
            Cat.sample = cat_sample
            model.__class__.__call__ = base_call
        d = D - k
        assert len(draws) == 3 and len(model.calls) == (1 if one_pass else 2)
        x_t = draws[0].view(B, d)
        x_tilde = x_t.clone()
        x_tilde[torch.arange(B), draws[1]] = draws[2]
        ts = model.calls[0][1]
        for inp, _ in model.calls:
            assert torch.equal(inp[:, :k], x0[:, :k])                       # the conditioner reaches the model unnoised
        assert torch.equal(model.calls[-1][0][:, k:], x_tilde) and ((x_tilde != x_t).sum(1) == 1).all()
        if not one_pass:
            assert torch.equal(model.calls[0][0][:, k:], x_t)
        # the restatement in fp64 on the same noise and tables
        th64 = torch.tensor(THETA, dtype=torch.float64, requires_grad=True)
        cond, data = x0[:, :k], x0[:, k:]
        l_sig = (toy_logits(torch.cat((cond, x_tilde), 1), ts, S, 1.0).double() * th64)[:, k:]
        l_reg = l_sig if one_pass else (toy_logits(torch.cat((cond, x_t), 1), ts, S, 1.0).double() * th64)[:, k:]
        qt0, rate = model.transition(ts).double(), model.rate(ts).double()
        v64 = neg_ct_elbo(l_reg, l_sig, data, x_tilde if one_pass else x_t, x_tilde, qt0, rate, cfg.loss.eps_ratio) + \
            nllw * F.cross_entropy(l_sig.permute(0, 2, 1), data)
        g64, = torch.autograd.grad(v64, th64)
        gref, = torch.autograd.grad(val, theta)
        print(f"{tag}: reference loss {val.item():.8g}  d/dtheta {gref.item():.6g} | fp64 restatement {v64.item():.10g}  d/dtheta {g64.item():.6g}")
        assert abs(v64.item() - val.item()) <= 1e-5 * abs(val.item()), tag
        meta = dict(kind=kind, S=S, B=B, D=D, condition_dim=k, one_forward_pass=one_pass, nll_weight=nllw, eps_ratio=cfg.loss.eps_ratio,
                    min_time=cfg.loss.min_time, theta=THETA, t_func=cfg.model.t_func, seed=SEED)
        arrs[f"{tag}__meta"] = np.array(repr(meta))
        arrs.update({f"{tag}__x0": x0, f"{tag}__ts": ts, f"{tag}__x_t": x_t, f"{tag}__x_tilde": x_tilde, f"{tag}__loss": val.detach(),
                     f"{tag}__grad_ref32": gref, f"{tag}__loss64": v64.detach(), f"{tag}__grad64": g64})
    save("cond_losses", **arrs)


if __name__ == "__main__":
    main()
