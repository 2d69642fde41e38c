"""Golden vectors of the D3PM baseline: runs the reference implementation's CategoricalDiffusion, unmodified, on the CPU and
records its tables and every public method's output in tests/golden/d3pm.npz (data only).

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_d3pm_golden.py <path of the reference checkout that holds lib/d3pm.py>

The reference is imported from the given path with oracle/stubs in front (loguru); its network is stood in for by
oracle.toy_model.toy_logits at time t / T.  tests/test_d3pm_cpu.py replays the same inputs through lib/d3pm.py.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.dont_write_bytecode = True

CASES = (   # name, transition type, bands, beta schedule, S, T
    ("uniform_full", "uniform", None, "cosine", 3, 8),
    ("uniform_band", "uniform", 2, "cosine", 16, 20),
    ("gaussian_full", "gaussian", None, "linear", 16, 8),
    ("gaussian_band", "gaussian", 2, "linear", 16, 20),
    ("absorbing_small", "absorbing", None, "jsd", 3, 20),
    ("absorbing", "absorbing", None, "jsd", 16, 8),
)
B, D = 4, 6


def spec(kind, bands, sched, S, T, loss_type="kl"):
    from ml_collections import ConfigDict
    m = ConfigDict()
    start, stop = (0.02, 1.0) if kind == "uniform" else (1e-4, 0.02)
    for k, v in dict(type=sched, start=start, stop=stop, num_timesteps=T, model_prediction="x_start", model_output="logits",
                     transition_mat_type=kind, transition_bands=bands, loss_type=loss_type, hybrid_coeff=0.01, num_pixel_vals=S,
                     device="cpu", is_img=False).items():
        m[k] = v
    return m


def toy_net(S, T):
    import torch
    from oracle.toy_model import toy_logits

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.dummy = torch.nn.Parameter(torch.zeros(1))

        def forward(self, x, t):
            return toy_logits(x.reshape(x.shape[0], -1), t.to(torch.float32) / T, S).reshape(tuple(x.shape) + (S,))

    return Net()


def main():
    ref = os.path.abspath(sys.argv[1])
    sys.path[:0] = [os.path.join(ROOT, "oracle", "stubs"), ref, ROOT]
    import numpy as np
    import torch
    import lib.d3pm as rd

    torch.set_num_threads(1)
    out = {"cases": np.array([c[0] for c in CASES])}
    for ci, (name, kind, bands, sched, S, T) in enumerate(CASES):
        dif = rd.make_diffusion(spec(kind, bands, sched, S, T))
        net = toy_net(S, T)
        g = torch.Generator().manual_seed(100 + ci)
        x0 = torch.randint(0, S, (B, D), generator=g)
        t = torch.tensor([0, 1, T - 1, T // 2], dtype=torch.int64)
        nq = torch.rand((B, D, S), generator=g)
        npn = torch.rand((B, D, S), generator=g)
        x_t = dif.q_sample(x0, t, nq)
        pred = net(x_t, t)
        sample, probs = dif.p_sample(net, x=x_t, t=t, noise=npn)
        model_logits, pred2 = dif.p_logits(net, x=x_t, t=t)
        vb, _ = dif.vb_terms_bpd(net, x_start=x0, x_t=x_t, t=t)
        rec = dict(S=S, T=T, bands=-1 if bands is None else bands, betas=dif.betas, q_onestep_mats=dif.q_onestep_mats, q_mats=dif.q_mats,
                   x_start=x0, t=t, noise_q=nq, noise_p=npn, q_probs=dif.q_probs(x0, t), x_t=x_t, pred=pred,
                   post_int=dif.q_posterior_logits(x0, x_t, t, x_start_logits=False),
                   post_logits=dif.q_posterior_logits(pred, x_t, t, x_start_logits=True),
                   model_logits=model_logits, p_sample=sample, p_sample_probs=probs, vb=vb, ce=dif.cross_entropy_x_start(x0, pred2))
        for lt in ("kl", "cross_entropy_x_start"):
            dl = rd.make_diffusion(spec(kind, bands, sched, S, T, lt))
            torch.manual_seed(7 + ci)
            xt_l = dl.q_sample(x0, t, torch.rand((B, D, S)))      # the draw training_losses makes first under this seed
            torch.manual_seed(7 + ci)
            rec["train_" + lt] = dl.training_losses(net, x0, t)
            rec["train_x_t"] = xt_l
        if kind != "absorbing":       # (the reference's prior_bpd raises a TypeError on its absorbing branch: not recorded there)
            rec["prior"] = dif.prior_bpd(x0)
            torch.manual_seed(11 + ci)
            bpd = dif.calc_bpd_loop(net, x0)
            rec.update(bpd_total=bpd["total"], bpd_vbterms=bpd["vbterms"], bpd_prior=bpd["prior"])
        torch.manual_seed(13 + ci)
        x_init, x_end = dif.p_sample_loop(net, (B, D), T, return_x_init=True)
        rec.update(loop_init=x_init, loop_end=x_end)
        for k, v in rec.items():
            out[f"{name}.{k}"] = v.detach().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
    path = os.path.join(ROOT, "tests", "golden", "d3pm.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main()
