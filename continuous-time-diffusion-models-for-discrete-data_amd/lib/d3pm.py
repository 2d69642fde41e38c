"""D3PM baseline: discrete-time diffusion on categorical data (Austin et al. 2021, "Structured Denoising Diffusion Models in
Discrete State-Spaces", arXiv:2107.03006), with the reference's names and call signatures (its lib/d3pm.py).

Time convention as there: the noisy states are x_0 .. x_{T-1}, the data is x_start (= x_{-1}).

States come as (B, D) or (B, C, H, W), a network output as (B, D, S) or x.shape + (S,); everything is computed on (B, D) and
handed back in the caller's shape.  The network gets `t` as passed (integer steps); on a GPU it is cast to float32, which is
what the HIP engines' time paths take.

Device selection: on a GPU with `fused` (cfg.model.d3pm_fused, default True) the objective and the ancestral step run on the
kernels of csrc/d3pm.hip (ctdd_d3pm_loss, ctdd_d3pm_step); with it off, and always on the CPU, the torch-op formulation below
runs -- the host path, the fallback and the yardstick of the kernels.  q_sample with explicit noise is always torch ops.
"""
import contextlib

import numpy as np
import scipy.special
import torch
import torch.nn.functional as F
from torch import nn

import lib.d3pm_utils as d3pm_utils
from lib.d3pm_utils import get_diffusion_betas  # noqa: F401  (the reference keeps it in this module)

_FIXED_NOISE = None      # test hook: {"x_t": (B, ...) ints} replaces training_losses' draw of the noisy state


def make_diffusion(hps):
    """cfg.model -> CategoricalDiffusion."""
    return CategoricalDiffusion(
        betas=get_diffusion_betas(hps), model_prediction=hps.model_prediction, model_output=hps.model_output,
        transition_mat_type=hps.transition_mat_type, transition_bands=hps.transition_bands, loss_type=hps.loss_type,
        hybrid_coeff=hps.hybrid_coeff, num_pixel_vals=hps.num_pixel_vals, device=hps.device,
        is_img=bool(hps.get("is_img", False)), fused=bool(hps.get("d3pm_fused", True)))


def _seed():
    return int(torch.randint(0, 2**62, (1,), dtype=torch.int64).item())


class _D3pmLossFn(torch.autograd.Function):
    """ctdd_d3pm_loss: the (B,) losses, with d loss_b / d logits[b] saved by the forward chain."""

    @staticmethod
    def forward(ctx, logits, x0, xt, t, qprev, qprevT, q1T, eps, vb_scale, ce_scale):
        from ctdd import native
        loss, _, _, grad = native.d3pm_loss(logits, x0, xt, t, qprev, qprevT, q1T, eps, vb_scale, ce_scale)
        ctx.save_for_backward(grad)
        return loss

    @staticmethod
    def backward(ctx, g):
        grad, = ctx.saved_tensors
        return (grad * g.to(grad.dtype).view(-1, 1, 1),) + (None,) * 9


class CategoricalDiffusion(nn.Module):
    """The forward process q (transition tables), the model posterior p and the variational bound."""

    def __init__(self, *, betas, model_prediction, model_output, transition_mat_type, transition_bands, loss_type,
                 hybrid_coeff, num_pixel_vals, device, is_img=False, fused=True):
        super().__init__()
        self.model_prediction = model_prediction      # 'x_start'
        self.model_output = model_output              # 'logits' | 'logistic_pars'
        self.loss_type = loss_type                    # 'kl' | 'cross_entropy_x_start' | 'hybrid'
        self.hybrid_coeff = hybrid_coeff
        self.num_pixel_vals = S = int(num_pixel_vals)
        self.transition_bands = transition_bands
        self.transition_mat_type = transition_mat_type
        self.eps = 1e-6
        self.device = device
        self.is_img = is_img
        self.fused = bool(fused)
        betas = torch.as_tensor(betas)
        if not ((betas > 0).all() and (betas <= 1).all()):
            raise ValueError("betas must be in (0, 1]")
        self.register("betas", betas)
        self.num_timesteps = T = int(betas.shape[0])
        build = {"uniform": self._uniform_mat, "gaussian": self._gaussian_mat, "absorbing": self._absorbing_mat}.get(transition_mat_type)
        if build is None:
            raise ValueError(f"transition_mat_type must be 'gaussian', 'uniform', 'absorbing', but is {transition_mat_type}")
        # one-step tables in fp64 (from the fp32 betas), kept as fp32 buffers.  Qbar_t = Q_0 Q_1 ... Q_t is the running fp32 product
        # of those buffers, as in the reference: its rounding drifts by an ulp or two over 20 steps (an fp64 product rounded once
        # is 1.8e-7 away from it at T = 20), and the baseline is compared on the reference's process, drift included
        step = torch.from_numpy(np.stack([build(float(self.betas[t])) for t in range(T)])).to(torch.float32)
        cum = [step[0]]
        for t in range(1, T):
            cum.append(torch.matmul(cum[-1], step[t]))
        self.register("q_onestep_mats", step.to(device))
        self.register("q_mats", torch.stack(cum).to(device))
        self.register("transpose_q_onestep_mats", self.q_onestep_mats.transpose(1, 2).contiguous())
        self.register("q_mats_T", self.q_mats.transpose(1, 2).contiguous())     # the GEMM kernels take the right operand as (N, K)
        assert self.q_mats.shape == self.q_onestep_mats.shape == (T, S, S)

    def register(self, name, tensor):
        self.register_buffer(name, tensor.type(torch.float32))

    # ---- one-step transition matrices Q_t (S, S), rows sum to one, fp64
    def _uniform_mat(self, beta):
        S, k = self.num_pixel_vals, self.transition_bands
        i = np.arange(S)
        band = np.ones((S, S), dtype=bool) if k is None else (np.abs(i[:, None] - i[None, :]) <= k)
        mat = np.where(band, beta / float(S), 0.0).astype(np.float64)
        np.fill_diagonal(mat, 0.0)
        np.fill_diagonal(mat, 1.0 - mat.sum(1))
        return mat

    def _gaussian_mat(self, beta):
        S = self.num_pixel_vals
        k = self.transition_bands if self.transition_bands else S - 1
        # off-diagonal weight of distance d: softmax over d = -k .. k of -(2 d (255 / (S - 1)) / (S - 1))^2 / beta
        v = np.linspace(0.0, 255.0, S, endpoint=True, dtype=np.float64) * 2.0 / (S - 1.0)
        v = -(v[:k + 1] ** 2) / beta
        w = scipy.special.softmax(np.concatenate([v[:0:-1], v]), axis=0)[k:]
        i = np.arange(S)
        dist = np.abs(i[:, None] - i[None, :])
        mat = np.where((dist >= 1) & (dist <= k), w[np.minimum(dist, k)], 0.0).astype(np.float64)
        np.fill_diagonal(mat, 1.0 - mat.sum(1))
        return mat

    def _absorbing_mat(self, beta):
        S = self.num_pixel_vals
        mat = np.diag(np.full((S,), 1.0 - beta, dtype=np.float64))
        mat[:, S // 2] += beta
        return mat

    # ---- shapes
    def _flat(self, x):
        return x.reshape(x.shape[0], -1)

    def _flat_logits(self, v, B):
        return v.reshape(B, -1, self.num_pixel_vals)

    def _at(self, a, t, x):
        """a[t_b][x[b, ...]][:]: (x.shape, S)."""
        xf = self._flat(x).to(torch.int64)
        return a[t.to(torch.int64).view(-1, 1), xf].reshape(tuple(x.shape) + (self.num_pixel_vals,))

    def _at_onehot(self, a, t, x):
        """x[b, ..., :] @ a[t_b]: x (.., S) probabilities."""
        B = x.shape[0]
        a_t = torch.index_select(a, 0, t.to(torch.int64))
        return torch.matmul(self._flat_logits(x, B), a_t).reshape(x.shape)

    def _call_model(self, model_fn, x, t):
        out = model_fn(x, t.to(torch.float32) if x.is_cuda else t)
        if self.model_output == "logits":
            logits = out
        elif self.model_output == "logistic_pars":
            logits = self._get_logits_from_logistic_pars(*out)
        else:
            raise NotImplementedError(self.model_output)
        return logits.reshape(tuple(x.shape) + (self.num_pixel_vals,))

    def _use_fused(self, x):
        return bool(self.fused and x.is_cuda)

    def _tables(self, t):
        t = t.to(torch.int64)
        t1 = torch.clamp(t - 1, min=0)
        return (self.q_mats.index_select(0, t1), self.q_mats_T.index_select(0, t1), self.transpose_q_onestep_mats.index_select(0, t))

    # ---- forward process
    def q_probs(self, x_start, t):
        """q(x_t | x_start): rows of Qbar_t."""
        return self._at(self.q_mats, t, x_start)

    def q_sample(self, x_start, t, noise):
        """x_t ~ q(x_t | x_start) by Gumbel-max on log(q + eps); noise: uniforms of shape x_start.shape + (S,)."""
        assert noise.shape == x_start.shape + (self.num_pixel_vals,)
        logits = torch.log(self.q_probs(x_start, t) + self.eps)
        noise = torch.clamp(noise, min=torch.finfo(noise.dtype).tiny, max=1.0)
        return torch.argmax(logits - torch.log(-torch.log(noise)), dim=-1)

    def _get_logits_from_logistic_pars(self, loc, log_scale):
        """Logits of a logistic distribution discretised on S bins over [-1, 1]."""
        S = self.num_pixel_vals
        loc, log_scale = loc.unsqueeze(-1), log_scale.unsqueeze(-1)
        inv_scale = torch.exp(-(log_scale - 2.0))
        half = 1.0 / (S - 1.0)
        centres = torch.linspace(-1.0, 1.0, S, device=loc.device) - loc
        lo = F.logsigmoid(inv_scale * (centres - half))
        hi = F.logsigmoid(inv_scale * (centres + half))
        return d3pm_utils.log_min_exp(hi, lo, self.eps)

    def q_posterior_logits(self, x_start, x_t, t, x_start_logits):
        """Logits of q(x_{t-1} | x_t, x_start); x_start integers, or logits of a distribution over it."""
        S = self.num_pixel_vals
        if x_start_logits:
            assert x_start.shape == x_t.shape + (S,), (x_start.shape, x_t.shape)
        else:
            assert x_start.shape == x_t.shape, (x_start.shape, x_t.shape)
        t1 = torch.where(t == 0, t, t - 1)
        fact1 = self._at(self.transpose_q_onestep_mats, t, x_t)
        if x_start_logits:
            fact2 = self._at_onehot(self.q_mats, t1, F.softmax(x_start, dim=-1))
            tzero = x_start
        else:
            fact2 = self._at(self.q_mats, t1, x_start)
            tzero = torch.log(F.one_hot(x_start.to(torch.int64), num_classes=S) + self.eps)
        out = torch.log(fact1 + self.eps) + torch.log(fact2 + self.eps)
        tb = t.reshape([out.shape[0]] + [1] * (out.dim() - 1))
        return torch.where(tb == 0, tzero, out)        # t = 0: the posterior of x_{-1} = x_start itself

    def p_logits(self, model_fn, *, x, t):
        """(logits of p(x_{t-1} | x_t), predicted x_start logits), both x.shape + (S,)."""
        assert t.shape == (x.shape[0],)
        pred = self._call_model(model_fn, x, t)
        if self.model_prediction != "x_start":
            raise NotImplementedError(self.model_prediction)
        tb = t.reshape([pred.shape[0]] + [1] * (pred.dim() - 1))
        model_logits = torch.where(tb == 0, pred, self.q_posterior_logits(pred, x, t, x_start_logits=True))
        return model_logits, pred

    # ---- sampling
    @torch.no_grad()
    def p_sample(self, model_fn, *, x, t, noise):
        """One ancestral step with explicit uniforms: (x_{t-1}, softmax of the predicted x_start logits)."""
        model_logits, pred = self.p_logits(model_fn=model_fn, x=x, t=t)
        assert noise.shape == model_logits.shape, noise.shape
        nonzero = (t != 0).to(x.dtype).reshape(x.shape[0], *([1] * x.dim()))
        noise = torch.clamp(noise, min=torch.finfo(noise.dtype).tiny, max=1.0)
        sample = torch.argmax(model_logits + nonzero * (-torch.log(-torch.log(noise))), dim=-1)
        return sample, F.softmax(pred, dim=-1)

    def _x_init(self, shape, device):
        S = self.num_pixel_vals
        if self.transition_mat_type in ("gaussian", "uniform"):       # stationary: uniform
            return torch.randint(size=shape, low=0, high=S).to(device)
        if self.transition_mat_type == "absorbing":                    # stationary: all mass on S // 2
            return torch.full(size=shape, fill_value=S // 2, dtype=torch.int32).to(device)
        raise ValueError(self.transition_mat_type)

    @torch.no_grad()
    def p_sample_loop(self, model_fn, shape, num_timesteps=None, return_x_init=False):
        """Ancestral sampling from the stationary state down to t = 0.  On the fused path: the network in its inference plan
        (borrowed output buffer, one time per batch), then one ctdd_d3pm_step per step on the rows' Philox streams."""
        shape = tuple(shape)
        params = getattr(model_fn, "parameters", None)
        device = next(params()).device if params is not None else torch.device(self.device)
        T = self.num_timesteps if num_timesteps is None else int(num_timesteps)
        x_init = self._x_init(shape, device)
        if self._use_fused(x_init):
            x = self._fused_loop(model_fn, x_init, T)
        else:
            x = x_init
            for i in reversed(range(T)):
                t = torch.full((shape[0],), i, dtype=torch.int64, device=device)
                x, _ = self.p_sample(model_fn=model_fn, x=x, t=t, noise=torch.rand(size=shape + (self.num_pixel_vals,)).to(device))
        assert x.shape == shape
        return (x_init, x) if return_x_init else x

    def _fused_loop(self, model_fn, x_init, T):
        from ctdd import native
        from lib.models.models import borrow_engine_output
        N, dev, seed = x_init.shape[0], x_init.device, _seed()
        i32_ok = bool(getattr(model_fn, "_engine_int32_states", False))
        borrow = borrow_engine_output(model_fn, uniform_time=True) if isinstance(model_fn, nn.Module) else contextlib.nullcontext()
        tt = getattr(model_fn, "engine_time_table", None)
        steps = torch.arange(T - 1, -1, -1, device=dev)
        temb = tt(steps.to(torch.float32)) if tt is not None and T > 0 else None
        x = self._flat(x_init).to(torch.int32).contiguous()
        with borrow:
            try:
                for n, i in enumerate(reversed(range(T))):
                    if temb is not None:
                        model_fn._engine_time_row = temb[n]
                    xin = (x if i32_ok else x.long()).reshape(x_init.shape)
                    logits = self._call_model(model_fn, xin, steps[n].expand(N))
                    logits = self._flat_logits(logits, N).float().contiguous()
                    i1 = max(i - 1, 0)
                    x = native.d3pm_step(logits, x, self.q_mats[i1], self.q_mats_T[i1], self.transpose_q_onestep_mats[i], i, self.eps,
                                         seed=seed, offset=i)
            finally:
                if temb is not None:
                    model_fn._engine_time_row = None
        return x.reshape(x_init.shape).to(x_init.dtype)

    # ---- the bound
    def _fused_terms(self, pred, x_start, x_t, t, vb_scale, ce_scale):
        """(loss, vb, ce), each (B,), of ctdd_d3pm_loss; differentiable in `pred` when it needs a gradient."""
        from ctdd import native
        B = x_start.shape[0]
        logits = self._flat_logits(pred, B).float().contiguous()
        x0 = self._flat(x_start).to(torch.int32).contiguous()
        xt = self._flat(x_t).to(torch.int32).contiguous()
        ti = t.to(torch.int32).contiguous()
        tabs = self._tables(t)
        if torch.is_grad_enabled() and logits.requires_grad:
            return _D3pmLossFn.apply(logits, x0, xt, ti, *tabs, self.eps, vb_scale, ce_scale), None, None
        loss, vb, ce, _ = native.d3pm_loss(logits.detach(), x0, xt, ti, *tabs, self.eps, vb_scale, ce_scale, want_grad=False)
        return loss, vb, ce

    def _vb_from_logits(self, model_logits, x_start, x_t, t):
        true_logits = self.q_posterior_logits(x_start, x_t, t, x_start_logits=False)
        kl = d3pm_utils.categorical_kl_logits(logits1=true_logits, logits2=model_logits)
        kl = d3pm_utils.meanflat(kl) / d3pm_utils.LN2
        nll = -d3pm_utils.categorical_log_likelihood(x_start, model_logits)
        nll = d3pm_utils.meanflat(nll) / d3pm_utils.LN2
        assert kl.shape == nll.shape == t.shape == (x_start.shape[0],)
        return torch.where(t == 0, nll, kl)

    def vb_terms_bpd(self, model_fn, *, x_start, x_t, t):
        """(term t_b of the variational bound in bits per dimension, (B,): KL(q(x_{t-1} | x_t, x_start) || p(x_{t-1} | x_t)),
        the decoder NLL at t = 0; predicted x_start logits)."""
        if self._use_fused(x_t):
            pred = self._call_model(model_fn, x_t, t)
            return self._fused_terms(pred, x_start, x_t, t, 1.0, 0.0)[0], pred
        model_logits, pred = self.p_logits(model_fn, x=x_t, t=t)
        return self._vb_from_logits(model_logits, x_start, x_t, t), pred

    def prior_bpd(self, x_start):
        """KL(q(x_{T-1} | x_start) || stationary distribution), bits per dimension."""
        S = self.num_pixel_vals
        t = torch.full((x_start.shape[0],), self.num_timesteps - 1, dtype=torch.int64, device=x_start.device)
        q = self.q_probs(x_start=x_start, t=t)
        if self.transition_mat_type in ("gaussian", "uniform"):
            prior = torch.ones_like(q) / S
        elif self.transition_mat_type == "absorbing":
            prior = F.one_hot(torch.full(q.shape[:-1], S // 2, dtype=torch.int64, device=q.device), num_classes=S)
        else:
            raise ValueError(self.transition_mat_type)
        return d3pm_utils.meanflat(d3pm_utils.categorical_kl_probs(q, prior)) / d3pm_utils.LN2

    def cross_entropy_x_start(self, x_start, pred_x_start_logits):
        """-log_softmax(pred)[x_start], mean over dimensions, bits: (B,)."""
        ce = -d3pm_utils.categorical_log_likelihood(x_start, pred_x_start_logits.reshape(tuple(x_start.shape) + (self.num_pixel_vals,)))
        return d3pm_utils.meanflat(ce) / d3pm_utils.LN2

    def _loss_weights(self):
        if self.loss_type == "kl":
            return 1.0, 0.0
        if self.loss_type == "cross_entropy_x_start":
            return 0.0, 1.0
        if self.loss_type == "hybrid":
            return 1.0, float(self.hybrid_coeff)
        raise NotImplementedError(self.loss_type)

    def _noisy(self, x_start, t):
        if _FIXED_NOISE is not None:
            return torch.as_tensor(_FIXED_NOISE["x_t"]).to(x_start.device).reshape(x_start.shape).to(x_start.dtype)
        if self._use_fused(x_start):
            # exact categorical draw on the rows of Qbar_t (no eps inside a log: 1e-6 off the Gumbel draw on log(q + eps))
            from ctdd import native
            xt = native.noise_categorical(self.q_mats, self._flat(x_start).to(torch.int32).contiguous(),
                                          tidx=t.to(torch.int32).contiguous(), seed=_seed())
            return xt.reshape(x_start.shape).to(x_start.dtype)
        noise = torch.rand(size=tuple(x_start.shape) + (self.num_pixel_vals,)).to(x_start.device)
        return self.q_sample(x_start=x_start, t=t, noise=noise)

    def training_losses(self, model_fn, x_start, t):
        """(B,) training losses of `loss_type`: 'kl' the bound's term, 'cross_entropy_x_start', or 'hybrid' = kl + hybrid_coeff ce."""
        vb_scale, ce_scale = self._loss_weights()
        x_t = self._noisy(x_start, t)
        if self._use_fused(x_t):
            pred = self._call_model(model_fn, x_t, t)
            losses = self._fused_terms(pred, x_start, x_t, t, vb_scale, ce_scale)[0]
        elif self.loss_type == "kl":
            losses, _ = self.vb_terms_bpd(model_fn=model_fn, x_start=x_start, x_t=x_t, t=t)
        elif self.loss_type == "cross_entropy_x_start":
            _, pred = self.p_logits(model_fn, x=x_t, t=t)
            losses = self.cross_entropy_x_start(x_start=x_start, pred_x_start_logits=pred)
        else:
            vb, pred = self.vb_terms_bpd(model_fn=model_fn, x_start=x_start, x_t=x_t, t=t)
            losses = vb + self.hybrid_coeff * self.cross_entropy_x_start(x_start=x_start, pred_x_start_logits=pred)
        assert losses.shape == t.shape
        return losses

    @torch.no_grad()
    def calc_bpd_loop(self, model_fn, x_start):
        """The whole bound: {'total' (B,), 'vbterms' (B, T), 'prior' (B,)}, one draw of x_t per step."""
        B = x_start.shape[0]
        terms = []
        for i in reversed(range(self.num_timesteps)):
            t = torch.full((B,), i, dtype=torch.int64, device=x_start.device)
            noise = torch.rand(size=tuple(x_start.shape) + (self.num_pixel_vals,)).to(x_start.device)
            vb, _ = self.vb_terms_bpd(model_fn=model_fn, x_start=x_start, t=t, x_t=self.q_sample(x_start=x_start, t=t, noise=noise))
            terms.append(vb)
        vb_tb = torch.stack(terms, dim=0)
        prior = self.prior_bpd(x_start=x_start)
        return {"total": vb_tb.sum(dim=0) + prior, "vbterms": vb_tb.T, "prior": prior}
