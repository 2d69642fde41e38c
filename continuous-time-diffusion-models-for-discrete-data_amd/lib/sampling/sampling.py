"""Samplers behind the reference's registry names (lib/sampling/sampling.py): TauL 82-234,
LBJF 238-356, MidPointTauL 360-526, PCTauL 530-646, ConditionalTauLeaping 649-758,
ConditionalPCTauLeaping 761-905, ExactSampling 975-1061; ConditionalLBJF, ConditionalMidPointTauL and
ConditionalExactSampling (not in the reference) hold entries the way its two conditional samplers do; AbsorbingLeap (not in the
reference either) is the absorbing-state process's sampler, on its own step kernel; AbsorbingConfidence, AbsorbingRemask and AbsorbingFirstHit build on it.

Same constructor `(cfg)`, same `sample(model, N)` return shapes; the per-step work is one fused
libctdd launch (reverse rates -> jump draw -> state update) on int32 device state.  Differences
that are deliberate and documented in DESIGN.md:
  * one q_{t|0} table per step instead of N identical copies; all steps' tables are
    built in one launch and stay resident in HBM;
  * no host sync inside the loop: the per-step `changed` counters are read back once at the end;
  * Poisson draws come from Philox (seeded from torch's global generator) -- distributional,
    not stream, parity with torch.poisson.
"""
import numpy as np
import torch

import lib.sampling.sampling_utils as sampling_utils
from ctdd import native
from lib.models.model_utils import get_logprob_with_logits  # noqa: F401  (re-exported like the reference)
from lib.models.models import borrow_engine_output

_CTELBO_LOSSES = ("CTElbo", "NLL", "CTElboLambda")


def get_initial_samples(N, D, device, S, initial_dist, initial_dist_std=None, seed=None, mask_state=None):
    """sampling.py:14-28.  Returns int64 (N,D) on `device` (uniform randint, or the discretised
    Gaussian centred at S//2 drawn by inverse CDF on the device; "absorbing": every entry at mask_state, default S - 1)."""
    if initial_dist == "absorbing":
        m = S - 1 if mask_state is None else int(mask_state)
        if not 0 <= m < S:
            raise ValueError(f"mask_state {m} outside [0, S = {S})")
        return torch.full((N, D), m, dtype=torch.int64, device=device)
    if seed is None:
        seed = _fresh_seed()
    if initial_dist == "uniform":
        cdf = None
    elif initial_dist == "gaussian":
        k = np.arange(1, S + 1)
        pmf = np.exp(-((k - S // 2) ** 2) / (2 * initial_dist_std**2))
        cdf = torch.from_numpy(np.cumsum(pmf / np.sum(pmf))).float().to(device)
    else:
        raise NotImplementedError("Unrecognized initial dist " + initial_dist)
    return native.initial_samples(N, D, S, torch.device(device), seed, 0xFFFF0000, cdf).long()


def _fresh_seed():
    """One 62-bit Philox key per call, taken from torch's global CPU generator so that
    torch.manual_seed() makes sampling reproducible."""
    return int(torch.randint(0, 2**62, (1,), dtype=torch.int64).item())


def _branch(cfg):
    """Which arm of get_reverse_rates applies (sampling.py:32 / 61: the elif is always truthy)."""
    return native.BRANCH_CTELBO if cfg.loss.name in _CTELBO_LOSSES else native.BRANCH_CRM


def _refuse_absorbing(model):
    """The general S x S samplers have not been checked on a rate matrix with a zero row: an absorbing model goes to AbsorbingLeap."""
    if getattr(getattr(model, "process", None), "kind", None) == "absorbing":
        raise ValueError("this sampler runs the general S x S path, which does not cover the absorbing process: use AbsorbingLeap")


def get_reverse_rates(model, logits, x, t_ones, cfg, N, D, S):
    """sampling.py:31-78: (reverse_rates, ratio), both (N,D,S); own state not zeroed."""
    _refuse_absorbing(model)
    branch = _branch(cfg)
    lt = getattr(cfg.loss, "logit_type", "direct") if branch == native.BRANCH_CRM else "direct"
    need_q = branch == native.BRANCH_CTELBO or lt != "direct"
    pr = model.process
    qt0, _, rate, _ = pr.tables(t_ones, want_qt0=need_q, want_rate=True)
    tidx = torch.arange(N, dtype=torch.int32, device=logits.device)
    return native.reverse_rates(branch, lt, logits.float().contiguous(), x.to(torch.int32).contiguous(), qt0, rate,
                                cfg.sampler.eps_ratio, tidx)


class _GridSampler:
    """Shared plumbing: config, device state, resident per-step tables, final denoise."""

    def __init__(self, cfg):
        self.cfg = cfg
        self.D = cfg.model.concat_dim
        self.S = cfg.data.S
        s = cfg.sampler
        self.num_steps, self.min_t, self.initial_dist = s.num_steps, s.min_t, s.initial_dist
        self.eps_ratio = s.eps_ratio
        self.loss_name = cfg.loss.name
        self.branch = _branch(cfg)
        self.logit_type = getattr(cfg.loss, "logit_type", "direct") if self.branch == native.BRANCH_CRM else "direct"
        self.seed = None              # set to an int for a fixed Philox key
        self.rank_stream = 0          # added to the key by the multi-GPU driver (ctdd/distributed.py)

    # -- pieces
    def _key(self):
        return (self.seed if self.seed is not None else _fresh_seed()) + self.rank_stream

    def _needs_qt0(self):
        return self.branch == native.BRANCH_CTELBO or self.logit_type != "direct"

    def _tables(self, model, times):
        """All steps' q_{t|0} in one launch, resident in HBM; beta(t) as host floats.
        `times` is float64 numpy; it reaches the schedules as float32 like `t*torch.ones(N)`."""
        t32 = torch.from_numpy(np.asarray(times, dtype=np.float64)).to(torch.float32)
        pr = model.process
        qt0 = pr.tables(t32, want_qt0=True)[0] if self._needs_qt0() else None
        return t32, qt0, pr.beta(t32).tolist()

    def _initial(self, model, N, key, std):
        _refuse_absorbing(model)                     # (every loop of this family starts here)
        return get_initial_samples(N, self.D, model.device, self.S, self.initial_dist, std, seed=key).to(torch.int32)

    def _final_argmax(self, model, x, N):
        t = torch.full((N,), float(np.float32(self.min_t)), device=x.device)
        return native.argmax(model(x.long(), t).float().contiguous())

    def _fast_tables(self, model, qt0):
        """S = 256, CT-ELBO branch or CRM branch with reverse_prob logits: derived tables for the MFMA kernel (csrc/steps_s256.hip)."""
        if self.S != 256 or qt0 is None or not getattr(self.cfg.sampler, "fast_s256", True):
            return None
        bf16 = self._step_bf16(model)
        if self.branch == native.BRANCH_CTELBO:
            return native.S256Tables(qt0, model.process.base_rate, self.eps_ratio, bf16=bf16)
        if self.logit_type == "reverse_prob":                    # CRM branch: the same contraction with a unit left scaling
            return native.S256Tables(qt0, model.process.base_rate, 0.0, crm=True, bf16=bf16)
        return None

    def _borrow(self, model):
        """Context for the sampler loops: the engine's own logits buffer is borrowed (no copy per step), and when the S = 256
        step runs its single-product bf16 mode the U-Net engine's output convolution writes the logits in bf16
        (cfg.sampler.logits_bf16, default True: half the bytes of the step's one large write and read; the rounding, 2^-8 of a
        logit, is below the bf16 network's own error)."""
        bf = (self.S == 256 and self._needs_qt0() and getattr(self.cfg.sampler, "fast_s256", True)
              and (self.branch == native.BRANCH_CTELBO or self.logit_type == "reverse_prob")
              and self._step_bf16(model) and bool(getattr(self.cfg.sampler, "logits_bf16", True)))
        return borrow_engine_output(model, bf16_logits=bf, uniform_time=True)      # (every sampler passes t * ones((N,)))

    @staticmethod
    def _net_logits(model, x, t, fast=None):
        """model(x, t) as the step kernels take it: bf16 straight through to the bf16 step (fast.bf16), fp32 otherwise."""
        # (the step kernels hand back int32 states; the U-Net engine's plans take them as they are -- no widening pass per step)
        out = model(x if (x.dtype == torch.int32 and getattr(model, "_engine_int32_states", False)) else x.long(), t)
        if out.dtype == torch.bfloat16 and fast is not None and fast.bf16:
            return out.contiguous()
        return out.float().contiguous()

    def _step_bf16(self, model):
        """cfg.sampler.step_precision: "bf16" = one bf16 product for the S x S ratio contraction (relative rate error <= 3 * 2^-8),
        "fp32" = three split-bf16 products (<= 3e-5, the parity mode), "auto" (default) = bf16 exactly when the score network
        itself runs single bf16 operands (cfg.model.engine == "hip" with engine_precision "bf16": its logits carry ~1e-2)."""
        mode = getattr(self.cfg.sampler, "step_precision", "auto")
        if mode == "auto":
            m = self.cfg.model
            default = "bf16" if hasattr(model, "data_shape") else "bf16x3"     # U-Net engine / hollow engine defaults
            return getattr(m, "engine", "hip") == "hip" and getattr(m, "engine_precision", default) == "bf16"
        if mode not in ("bf16", "fp32"):
            raise ValueError(f"sampler.step_precision must be 'auto', 'bf16' or 'fp32', got {mode!r}")
        return mode == "bf16"

    # -- the steps.  rows None: every row moves; an int32 device tensor of row indices into the N*D rows: only those do, and the
    # other rows of the returned state are those of x (the `_rows` entries of the same kernels, see ctdd/native.py)
    def _leap(self, model, logits, x, q_i, fast, i, beta, h, flags, key, offset, x_base=None, changed=None, rows=None):
        """One fused reverse-rate / jump / update launch (MFMA path when prepared, else generic)."""
        if fast is not None:
            return native._tauleap_s256(logits, x, fast, i, beta, h, flags, key, offset, rows, x_base=x_base, changed=changed)
        return native._tauleap(self.branch, self.logit_type, logits, x, q_i, model.process.base_rate, beta, self.eps_ratio, h,
                               flags, key, offset, rows, x_base=x_base, changed=changed)

    def _lbjf(self, model, logits, x, q_i, fast, i, beta, h, flags, key, offset, changed=None, rows=None, rates=None):
        """One Euler / LBJF step; at S = 256 the reverse rates come from the matrix-core kernel (into `rates` (N, D, 256) when
        given: the buffer a row-list sampler allocates once per call), the posterior and the categorical draw run on them."""
        if fast is not None:
            _, rates = native._tauleap_s256(logits, x, fast, i, beta, h, flags & native.STEP_CORRECTOR, key, offset, rows,
                                            want_rates=True, rates=rates, want_x=False)
            return native._lbjf_rates(rates, x, h, rows, None, key, offset, changed=changed)
        return native._lbjf(self.branch, self.logit_type, logits, x, q_i, model.process.base_rate, beta, self.eps_ratio, h, rows,
                            flags, None, key, offset, changed=changed)

    def _midpoint_predict(self, model, logits, x, q_i, fast, i, beta, h, key, rows=None, rates=None):
        """The deterministic half-step drift x' of midpoint tau-leaping (x' = x on unlisted rows); S = 256 as in _lbjf."""
        if fast is not None:
            _, rates = native._tauleap_s256(logits, x, fast, i, beta, float(np.float32(h)), 0, key, 0, rows, want_rates=True,
                                            rates=rates, want_x=False)
            return native._midpoint_rates(rates, x, h, rows)
        return native._midpoint(self.branch, self.logit_type, logits, x, q_i, model.process.base_rate, beta, self.eps_ratio, h, rows)

    def _grid(self):
        """linspace(max_t, min_t, num_steps) followed by 0."""
        return np.concatenate((np.linspace(self.max_t, self.min_t, self.num_steps), np.array([0])))

    def _pc_loop(self, model, N, std, flags, held=None):
        """The predictor-corrector tau-leaping loop of PCTauL and ConditionalPCTauLeaping: h = 1 / num_steps, grid
        linspace(1.0, min_t + h, num_steps) walked over ts[:-1], correctors at t - h once t <= corrector_entry_time, argmax at
        min_t.  std: of the initial draw; held as in LBJF._loop.  Returns the (N, D) int array."""
        s = self.cfg.sampler
        dev = torch.device(model.device)
        key = self._key()
        with torch.no_grad(), self._borrow(model):
            x = self._initial(model, N, key, std)
            rows = None
            if held is not None:
                xk, m, rows = held
                x = torch.where(m, xk, x)
            h0 = 1.0 / s.num_steps
            ts = np.linspace(1.0, s.min_t + h0, s.num_steps)
            pr = model.process
            t32, qt0, betas = self._tables(model, ts)
            fast = self._fast_tables(model, qt0)
            sub = 1 + max(int(s.num_corrector_steps), 0)
            for i, t in enumerate(ts[:-1]):
                h = ts[i] - ts[i + 1]
                logits = self._net_logits(model, x, self._t_ones(t32, i, N, dev), fast)
                x = self._leap(model, logits, x, qt0[i], fast, i, betas[i], float(np.float32(h)), flags, key, i * sub, rows=rows)
                if t <= s.corrector_entry_time:
                    tc = torch.tensor([t - h], dtype=torch.float64).to(torch.float32)
                    qc = pr.tables(tc, want_qt0=True)[0][0]
                    bc = float(pr.beta(tc)[0])
                    t_c = torch.full((N,), float(tc[0]), device=dev)
                    fast_c = self._fast_tables(model, qc.unsqueeze(0)) if fast is not None else None
                    for c in range(s.num_corrector_steps):
                        logits = self._net_logits(model, x, t_c, fast_c)
                        x = self._leap(model, logits, x, qc, fast_c, 0, bc, float(np.float32(s.corrector_step_size_multiplier * h)),
                                       flags | native.STEP_CORRECTOR, key, i * sub + 1 + c, rows=rows)
            x = self._final_argmax(model, x, N)
            if held is not None:
                x = torch.where(m, xk, x)
            return x.cpu().numpy().astype(int)

    @staticmethod
    def _t_ones(t32, i, N, device):
        return torch.full((N,), float(t32[i]), device=device, dtype=torch.float32)


@sampling_utils.register_sampler
class TauL(_GridSampler):
    """Tau-leaping with optional corrector steps (sampling.py:82-234)."""

    def __init__(self, cfg):
        super().__init__(cfg)
        s = cfg.sampler
        self.max_t = cfg.training.max_t
        self.corrector_entry_time = s.corrector_entry_time
        self.num_corrector_steps = s.num_corrector_steps
        self.is_ordinal = s.is_ordinal

    # The loop is split into begin / advance / finish so that a driver (bench.py, the multi-GPU
    # sharder) can time or interleave exact sampler steps; sample() is their composition.
    def _pipeline_parts(self, model, N):
        """Independent sub-batches the loop drives on parallel streams (cfg.sampler.pipeline_sub_batches; default: the U-Net
        engine's `engine_streams`, 2).  Samples never interact, so each sub-batch runs its own chain
        forward -> fused step -> forward -> ... with NO join per step: one chain's tau-leap launch (vector ALU / memory) runs
        under the other's convolutions (matrix cores) instead of on the critical path of both."""
        p = getattr(self.cfg.sampler, "pipeline_sub_batches", None)
        unet = hasattr(model, "_engine_forward") and getattr(self.cfg.model, "engine", "hip") == "hip" and str(model.device) != "cpu"
        if p is None:
            p = int(getattr(self.cfg.model, "engine_streams", 2)) if unet else 1
        p = int(p)
        return p if (unet and p > 1 and N % p == 0 and N // p >= 32) else 1

    def begin(self, model, N, pipeline=None, held=None):
        """held = (x_known int32, mask bool, free-row lists: one per sub-batch and relative to it), all on the device
        (ConditionalTauLeaping): the held entries are scattered in after the initial draw and every launch moves the listed rows only."""
        dev = torch.device(model.device)
        st = type("TauLState", (), {})()
        st.model, st.N, st.dev, st.key = model, N, dev, self._key()
        st.x = self._initial(model, N, st.key, self.cfg.model.Q_sigma)
        st.rows = None
        if held is not None:
            xk, m, st.rows = held
            st.x = torch.where(m, xk, st.x)
        st.ts = self._grid()
        st.t32, st.qt0, st.betas = self._tables(model, st.ts[:-1])
        st.fast = self._fast_tables(model, st.qt0)
        # the grid's times are known here: the U-Net engine computes every step's time-projection row in one launch and the
        # per-step plans run without their time path (cfg.sampler.time_table, default True; None: the model has no such plan)
        tt = getattr(model, "engine_time_table", None) if getattr(self.cfg.sampler, "time_table", True) else None
        st.t_dev = st.t32.to(dev)
        st.temb = tt(st.t_dev) if tt is not None else None
        st.changed = torch.zeros(self.num_steps, dtype=torch.int32, device=dev)
        st.flags = native.STEP_ORDINAL if self.is_ordinal else 0
        st.sub = 1 + max(int(self.num_corrector_steps), 0)
        st.parts = self._pipeline_parts(model, N) if pipeline is None else (int(pipeline) if pipeline else 1)
        if st.parts > 1:
            P = st.parts
            n = N // P
            st.xs = [st.x[j * n:(j + 1) * n].clone() for j in range(P)]
            st.x = None                                     # (joined again by finish / state_x)
            st.changed_p = torch.zeros((P, self.num_steps), dtype=torch.int32, device=dev)
            main = torch.cuda.current_stream(dev)
            st.streams = [main] + [torch.cuda.Stream(device=dev) for _ in range(P - 1)]
            for s_ in st.streams[1:]:
                s_.wait_stream(main)                        # tables, initial state and plans' weights are ready
        return st

    def state_x(self, st):
        """The current state (N, D) of all samples (joins the sub-batch streams when the loop is pipelined)."""
        if st.parts == 1:
            return st.x
        main = st.streams[0]
        for s_ in st.streams[1:]:
            main.wait_stream(s_)
        return torch.cat(st.xs, 0)

    def advance(self, st, i):
        """Step i of the grid: network forward, fused reverse-rate/jump/update launch, correctors."""
        model = st.model
        with self._borrow(model):
            try:
                if st.temb is not None:
                    model._engine_time_row = st.temb[i]
                if st.parts == 1:
                    st.x = self._advance_one(st, i, st.x, st.N, st.key, st.changed[i:i + 1])
                    return
                for j in range(st.parts):
                    with torch.cuda.stream(st.streams[j]):
                        model._engine_slot = j
                        # a Philox key per sub-batch (the rows of a launch are numbered from 0)
                        st.xs[j] = self._advance_one(st, i, st.xs[j], st.N // st.parts, st.key + 7919 * j, st.changed_p[j, i:i + 1],
                                                     part=j)
            finally:
                model._engine_slot = None
                if st.temb is not None:
                    model._engine_time_row = None

    def _advance_one(self, st, i, x, N, key, changed, part=0):
        model = st.model
        t = st.ts[i]
        h = float(np.float32(st.ts[i] - st.ts[i + 1]))
        # (with the time table the plans never read the times: a stride-0 view of the grid value instead of a fill launch per step)
        t_ones = st.t_dev[i].expand(N) if st.temb is not None else self._t_ones(st.t32, i, N, st.dev)
        q_i = st.qt0[i] if st.qt0 is not None else None
        rows = st.rows[part] if st.rows is not None else None
        logits = self._net_logits(model, x, t_ones, st.fast)
        x = self._leap(model, logits, x, q_i, st.fast, i, st.betas[i], h, st.flags, key, i * st.sub, changed=changed, rows=rows)
        if t <= self.corrector_entry_time:
            for c in range(self.num_corrector_steps):
                logits = self._net_logits(model, x, t_ones, st.fast)
                x = self._leap(model, logits, x, q_i, st.fast, i, st.betas[i], h, st.flags | native.STEP_CORRECTOR, key, i * st.sub + 1 + c,
                               rows=rows)
        return x

    def finish(self, st):
        x = self.state_x(st)
        changed = st.changed if st.parts == 1 else st.changed_p.sum(0)
        if self.loss_name in ("CTElbo", "NLL"):
            x = self._final_argmax(st.model, x, st.N)
        return x.cpu().numpy().astype(int), (changed.cpu().numpy() / st.N).tolist()

    def sample(self, model, N):
        with torch.no_grad(), self._borrow(model):
            st = self.begin(model, N)
            for i in range(self.num_steps):
                self.advance(st, i)
            return self.finish(st)


@sampling_utils.register_sampler
class LBJF(_GridSampler):
    """Euler / 'LBJF' sampler: one categorical draw per dimension per step (sampling.py:238-356)."""

    def __init__(self, cfg):
        super().__init__(cfg)
        s = cfg.sampler
        self.max_t = cfg.training.max_t
        self.corrector_entry_time = s.corrector_entry_time
        self.num_corrector_steps = s.num_corrector_steps

    def sample(self, model, N):
        return self._loop(model, N)

    def _loop(self, model, N, held=None):
        """The sampler loop.  held = (x_known int32, mask bool, free-row list), all on the device (ConditionalLBJF): the held
        entries are scattered in after the initial draw, every step moves the listed rows only, and they are restored at the end."""
        dev = torch.device(model.device)
        key = self._key()
        with torch.no_grad(), self._borrow(model):
            x = self._initial(model, N, key, self.cfg.model.Q_sigma)
            ts = self._grid()
            t32, qt0, betas = self._tables(model, ts[:-1])
            changed = torch.zeros(self.num_steps, dtype=torch.int32, device=dev)
            fast = self._fast_tables(model, qt0)
            sub = 1 + max(int(self.num_corrector_steps), 0)
            rows = rates = None
            if held is not None:
                xk, m, rows = held
                x = torch.where(m, xk, x)
                rates = torch.empty((N, self.D, self.S), dtype=torch.float32, device=dev) if fast is not None else None
            for i, t in enumerate(ts[:-1]):
                h = float(np.float32(ts[i] - ts[i + 1]))
                t_ones = self._t_ones(t32, i, N, dev)
                q_i = qt0[i] if qt0 is not None else None
                logits = self._net_logits(model, x, t_ones, fast)
                x = self._lbjf(model, logits, x, q_i, fast, i, betas[i], h, 0, key, i * sub, changed=changed[i:i + 1], rows=rows,
                               rates=rates)
                if t <= self.corrector_entry_time:
                    for c in range(self.num_corrector_steps):
                        logits = self._net_logits(model, x, t_ones, fast)
                        x = self._lbjf(model, logits, x, q_i, fast, i, betas[i], h, native.STEP_CORRECTOR, key, i * sub + 1 + c,
                                       rows=rows, rates=rates)
            if self.loss_name == "CTElbo":
                x = self._final_argmax(model, x, N)
            if held is not None:
                x = torch.where(m, xk, x)
            return x.cpu().numpy().astype(int), (changed.cpu().numpy() / N).tolist()


@sampling_utils.register_sampler
class MidPointTauL(_GridSampler):
    """Midpoint tau-leaping: deterministic half-step drift, then a Poisson step with rates taken
    at (x', t-h/2) (sampling.py:360-526).  The reference indexes a `state_change[s][x] = s - x`
    table (loaded from a file that is not in the repo for MNIST); the kernels compute
    s - x directly, for any S."""

    def __init__(self, cfg):
        super().__init__(cfg)
        self.max_t = cfg.training.max_t
        self.is_ordinal = cfg.sampler.is_ordinal
        self.device = cfg.device

    def sample(self, model, N):
        return self._loop(model, N)

    def _times(self):
        """(h, the times of the full steps): max_t, max_t - h, ... while the half step stays above min_t."""
        h = (self.max_t - self.min_t) / self.num_steps
        full, t = [], self.max_t
        while t - 0.5 * h > self.min_t:
            full.append(t)
            t = t - h
        return h, full

    def _loop(self, model, N, held=None):
        """The sampler loop; held as in LBJF._loop (ConditionalMidPointTauL): both stages move the listed rows only, so x' = x
        on the held rows."""
        dev = torch.device(model.device)
        key = self._key()
        with torch.no_grad(), self._borrow(model):
            x = self._initial(model, N, key, self.cfg.model.Q_sigma)
            rows = None
            if held is not None:
                xk, m, rows = held
                x = torch.where(m, xk, x)
            h, full = self._times()
            # t_05 = float32(t)*ones - 0.5*h evaluated in float32, as in the reference
            t32 = torch.tensor(full, dtype=torch.float64).to(torch.float32)
            t32_half = t32 - 0.5 * h
            nst = len(full)
            pr = model.process
            need_q = self._needs_qt0()
            q_full = pr.tables(t32, want_qt0=True)[0] if need_q else None
            q_half = pr.tables(t32_half, want_qt0=True)[0] if need_q else None
            b_full, b_half = pr.beta(t32).tolist(), pr.beta(t32_half).tolist()
            fast_half = self._fast_tables(model, q_half)
            fast_full = self._fast_tables(model, q_full)
            # per step: [final changes, dims with >= 1 jump event, dims with > 1, first-stage changes, 1to2 changes]
            cnt = torch.zeros(nst, 5, dtype=torch.int32, device=dev)
            flags = (native.STEP_ORDINAL if self.is_ordinal else 0) | native.STEP_COUNT_RAW | native.STEP_COUNT_JUMPS
            hf = float(np.float32(h))
            rates = (torch.empty((N, self.D, self.S), dtype=torch.float32, device=dev)
                     if held is not None and fast_full is not None else None)
            for i in range(nst):
                t_ones = torch.full((N,), float(t32[i]), device=dev)
                t_05 = torch.full((N,), float(t32_half[i]), device=dev)
                logits = self._net_logits(model, x, t_ones, fast_full)
                x_prime = self._midpoint_predict(model, logits, x, q_full[i] if need_q else None, fast_full, i, b_full[i], h, key,
                                                 rows=rows, rates=rates)
                logits_p = self._net_logits(model, x_prime, t_05, fast_half)
                # (x_base = x' also on the held rows, where x' = x: it is only read at the listed rows)
                x_new = self._leap(model, logits_p, x, q_half[i] if need_q else None, fast_half, i, b_half[i], hf,
                                   flags, key, i, x_base=x_prime, changed=cnt[i, 0:3], rows=rows)
                cnt[i, 3] = (x != x_prime).sum()
                cnt[i, 4] = (x_prime != x_new).sum()
                x = x_new
            if self.loss_name == "CTElbo":
                x = self._final_argmax(model, x, N)
            if held is not None:
                x = torch.where(m, xk, x)
            raw = cnt.cpu().numpy().astype(np.float64)
            c = raw / (N * self.D)
            # (samples, change_jump, change_dim, change_dim_first, change_1to2); change_jump = share of the jumping
            # dimensions that drew more than one event, appended only when is_ordinal (sampling.py:489-495; 0/0 -> nan there too)
            with np.errstate(divide="ignore", invalid="ignore"):
                change_jump = (raw[:, 2] / raw[:, 1]).tolist() if self.is_ordinal else []
            return x.cpu().numpy().astype(int), change_jump, c[:, 0].tolist(), c[:, 3].tolist(), c[:, 4].tolist()


@sampling_utils.register_sampler
class PCTauL(_GridSampler):
    """Original tauLDR predictor-corrector (sampling.py:530-646): CT-ELBO rates, ordinal update,
    t grid from 1.0, initial std 200, bare ndarray return."""

    def __init__(self, cfg):
        super().__init__(cfg)
        self.branch, self.logit_type = native.BRANCH_CTELBO, "direct"

    def sample(self, model, N):
        return self._pc_loop(model, N, 200, native.STEP_ORDINAL)


class _Conditioned:
    """Shared part of the conditional samplers: argument checks (all before any device work) and the held / free split.

    `inpaint(model, x_known, mask)`: x_known (N, D) integer states, mask (D,) or (N, D) bool, True = held at x_known.  The
    state is always the full (N, D): held entries are scattered in once after the initial draw, so the network sees them at
    every step, and every step launch moves only the free rows (the step helpers' `rows` list: a held row costs no softmax,
    no S x S contraction and no draw).  The final argmax is taken at min_t and the held entries are restored in the result.
    `sample(model, N, conditioner)` (the reference's call) is `inpaint` with the first cfg.sampler.condition_dim columns
    held.  D is cfg.model.concat_dim (the reference reads cfg.data.shape[0], which is D only for 1-D data); for image data
    the flattened order is the row-major (C, H, W) one, so a prefix of the dimensions is the top rows of the image."""

    def sample(self, model, N, conditioner):
        x_known, mask = self._prefix(N, conditioner)
        return self.inpaint(model, x_known, mask)

    def _prefix(self, N, conditioner):
        cd = getattr(self.cfg.sampler, "condition_dim", None)
        if cd is None or not 0 < int(cd) < self.D:
            raise ValueError(f"cfg.sampler.condition_dim must satisfy 0 < condition_dim < D = {self.D}, got {cd!r}")
        cd, N = int(cd), int(N)
        cond = torch.as_tensor(conditioner)
        if tuple(cond.shape) != (N, cd):
            raise ValueError(f"conditioner: expected shape {(N, cd)}, got {tuple(cond.shape)}")
        x_known = torch.zeros((N, self.D), dtype=torch.int64)
        x_known[:, :cd] = cond.cpu().to(torch.int64)
        mask = torch.zeros(self.D, dtype=torch.bool)
        mask[:cd] = True
        return x_known, mask

    def _held(self, x_known, mask):
        """-> (N, x_known int32 (N, D), mask bool (N, D)) on the host, after the shape / dtype / value checks."""
        xk = torch.as_tensor(x_known)
        if xk.dim() != 2 or xk.shape[1] != self.D:
            raise ValueError(f"x_known: expected shape (N, {self.D}), got {tuple(xk.shape)}")
        if xk.dtype.is_floating_point or xk.dtype.is_complex or xk.dtype == torch.bool:
            raise ValueError(f"x_known: expected an integer tensor, got {xk.dtype}")
        N = int(xk.shape[0])
        m = torch.as_tensor(mask)
        if m.dtype != torch.bool:
            raise ValueError(f"mask: expected a bool tensor, got {m.dtype}")
        if tuple(m.shape) == (self.D,):
            m = m.view(1, self.D).expand(N, self.D)
        elif tuple(m.shape) != (N, self.D):
            raise ValueError(f"mask: expected shape ({self.D},) or {(N, self.D)}, got {tuple(m.shape)}")
        if N < 1:
            raise ValueError("x_known: no samples")
        xk, m = xk.cpu().to(torch.int32), m.cpu().contiguous()         # (the call's one host round trip, before the loop)
        held = xk[m]
        if held.numel() and (int(held.min()) < 0 or int(held.max()) >= self.S):
            raise ValueError(f"x_known: held values must lie in [0, {self.S})")
        return N, xk, m

    @staticmethod
    def _free_rows(m, parts, dev):
        """Free-row lists (int32, ascending, on the device), one per sub-batch and relative to it."""
        N = m.shape[0]
        n = N // parts
        return [(~m[j * n:(j + 1) * n]).reshape(-1).nonzero().view(-1).to(torch.int32).to(dev) for j in range(parts)]


@sampling_utils.register_sampler
class ConditionalTauLeaping(_Conditioned, TauL):
    """Conditional tau-leaping (sampling.py:649-758), see _Conditioned: CT-ELBO rates with direct logits whatever cfg.loss is,
    ordinal sum-and-clamp update (the reference overwrites its reject_multiple_jumps branch, line 744), initial std
    cfg.model.Q_sigma, grid linspace(1.0, min_t, num_steps) + [0], no corrector, argmax at min_t.  The loop is TauL's
    begin / advance / finish, so on the U-Net engine it runs as two pipelined sub-batch chains, each with its own row list."""

    def __init__(self, cfg):
        super().__init__(cfg)
        self.branch, self.logit_type = native.BRANCH_CTELBO, "direct"
        self.max_t = 1.0
        self.num_corrector_steps = 0
        self.is_ordinal = True

    def inpaint(self, model, x_known, mask):
        N, xk, m = self._held(x_known, mask)
        if bool(m.all()):
            return xk.numpy().astype(int)
        dev = torch.device(model.device)
        parts = self._pipeline_parts(model, N)
        rows = self._free_rows(m, parts, dev)
        xk, m = xk.to(dev), m.to(dev)
        with torch.no_grad(), self._borrow(model):
            st = self.begin(model, N, pipeline=parts, held=(xk, m, rows))
            for i in range(self.num_steps):
                self.advance(st, i)
            x = self._final_argmax(model, self.state_x(st), N)
            return torch.where(m, xk, x).cpu().numpy().astype(int)


@sampling_utils.register_sampler
class ConditionalPCTauLeaping(_Conditioned, _GridSampler):
    """Conditional predictor-corrector tau-leaping (sampling.py:761-905), see _Conditioned: CT-ELBO rates with direct logits,
    initial std cfg.model.Q_sigma, h = 1 / num_steps, grid linspace(1.0, min_t + h, num_steps) walked over ts[:-1];
    correctors at t - h with step corrector_step_size_multiplier * h when t <= corrector_entry_time; sum-and-clamp update
    (cfg.sampler.reject_multiple_jumps, default False, keeps only single-event dimensions, as the reference's
    take_poisson_step does); argmax at min_t."""

    def __init__(self, cfg):
        super().__init__(cfg)
        self.branch, self.logit_type = native.BRANCH_CTELBO, "direct"

    def inpaint(self, model, x_known, mask):
        N, xk, m = self._held(x_known, mask)
        if bool(m.all()):
            return xk.numpy().astype(int)
        dev = torch.device(model.device)
        rows = self._free_rows(m, 1, dev)[0]
        flags = 0 if bool(getattr(self.cfg.sampler, "reject_multiple_jumps", False)) else native.STEP_ORDINAL
        return self._pc_loop(model, N, self.cfg.model.Q_sigma, flags, held=(xk.to(dev), m.to(dev), rows))


@sampling_utils.register_sampler
class ExactSampling(_GridSampler):
    """Exact one-step posterior sampling for SDDM models (sampling.py:975-1061):
    x_{t-h}^d ~ sum_{x0} p_theta(x0 | x_t^{\\d}) q_{t-h|0}(.|x0) q_{t|t-h}(x_t^d | .)   per dimension.
    The (N,D,S,S) log-sum-exp of the reference is the matrix product
    softmax(logits) @ q_{t-h|0} times the column x_t of q_{t|t-h}; contraction, normalisation and the categorical
    draw (exponential race, the K7 rule) are one HIP launch per step: `ctdd_exact_step`."""

    def __init__(self, cfg):
        super().__init__(cfg)
        self.max_t = cfg.training.max_t

    def sample(self, model, N):
        return self._loop(model, N)

    def _loop(self, model, N, held=None):
        """The sampler loop; held as in LBJF._loop (ConditionalExactSampling)."""
        dev = torch.device(model.device)
        key = self._key()
        with torch.no_grad(), borrow_engine_output(model, uniform_time=True):
            x = self._initial(model, N, key, self.cfg.model.Q_sigma).long()
            rows = None
            if held is not None:
                xk, m, rows = held
                x = torch.where(m, xk.long(), x)
            ts = self._grid()
            pr = model.process
            t_hi = torch.from_numpy(ts[:-1]).to(torch.float32)
            t_lo = torch.from_numpy(ts[:-1] - (ts[:-1] - ts[1:])).to(torch.float32)
            q_lo = pr.tables(t_lo, want_qt0=True)[0]                      # q_{t-h|0}  (steps,S,S)
            q_step = pr.transit_between(t_lo, t_hi)                       # q_{t|t-h}  (steps,S,S)
            q_lo, q_step = q_lo.contiguous(), q_step.contiguous()
            x = x.to(torch.int32).contiguous()
            moved = torch.zeros(self.num_steps, dtype=torch.int32, device=dev)
            for i in range(self.num_steps):
                t_ones = self._t_ones(t_hi, i, N, dev)
                logits = model(x.long(), t_ones).float().contiguous()
                # softmax, the S x S contraction with q_{t-h|0}, the column x_t of q_{t|t-h}, normalisation and the categorical
                # draw (exponential race on Philox(key, i, row, s)) in ONE launch: ctdd_exact_step
                x = native._exact(logits, x, q_lo[i], q_step[i], rows, None, key, i, changed=moved[i:i + 1])
            change = moved.float() / float(N * self.D)
            return x.cpu().numpy().astype(int), change.cpu().tolist()


class _ConditionedLoop(_Conditioned):
    """ConditionalLBJF / ConditionalMidPointTauL / ConditionalExactSampling: the parent's loop (`_loop`) with held entries, see
    _Conditioned.  Unlike the two tau-leaping samplers above, these follow the parent in everything but the held rows: branch
    and logit type from cfg.loss, the grid from cfg.training.max_t, initial std cfg.model.Q_sigma, corrector / ordinal settings,
    the final argmax exactly when the parent takes it, the parent's return tuple, and per-step counters with the parent's
    normalisation that count free rows only.  The Philox counter is keyed by the row of the N*D space, so an all-free mask
    returns the parent's samples bit for bit under the same seed on a deterministic model."""

    def inpaint(self, model, x_known, mask):
        N, xk, m = self._held(x_known, mask)
        if bool(m.all()):
            return self._all_held(xk.numpy().astype(int))
        dev = torch.device(model.device)
        rows = self._free_rows(m, 1, dev)[0]
        return self._loop(model, N, held=(xk.to(dev), m.to(dev), rows))

    def _grid_len(self):
        return self.num_steps

    def _all_held(self, x):
        """Nothing is free: x_known in the parent's return shape (no step ran, so every per-step counter is zero)."""
        return x, [0.0] * self._grid_len()


@sampling_utils.register_sampler
class ConditionalLBJF(_ConditionedLoop, LBJF):
    """LBJF with held entries (see _ConditionedLoop): `ctdd_lbjf_step_rows` per step and corrector; at S = 256 (CT-ELBO, or CRM
    with reverse_prob logits) `ctdd_tauleap_step_s256_rows` for the listed rows' rates, then `ctdd_lbjf_from_rates_rows`."""


@sampling_utils.register_sampler
class ConditionalMidPointTauL(_ConditionedLoop, MidPointTauL):
    """Midpoint tau-leaping with held entries (see _ConditionedLoop): stage 1 `ctdd_midpoint_predict_rows` (S = 256: the rates
    pair with `ctdd_midpoint_from_rates_rows`), held rows of x' equal x; stage 2 the row-list tau-leap step with x_base = x'."""

    def _grid_len(self):
        return len(self._times()[1])

    def _all_held(self, x):
        z = [0.0] * self._grid_len()
        return x, ([float("nan")] * len(z) if self.is_ordinal else []), list(z), list(z), list(z)


@sampling_utils.register_sampler
class ConditionalExactSampling(_ConditionedLoop, ExactSampling):
    """ExactSampling with held entries (see _ConditionedLoop): `ctdd_exact_step_rows` per step; no argmax at the end."""


def lbjf_corrector_step(cfg, model, xt, t, h, N, device, xt_target=None, seed=None, E=None, want_probs=False):
    """One Euler corrector step with SDDM ratios (sampling.py:1064-1085):
    posterior = h * (exp(ll_all - ll_xt) + 1) * R_t[x_t, :] off the diagonal, clip(1 - sum, 0) on it, normalised, then one
    categorical draw per dimension.  That is the Euler posterior of the corrector rates R^ + R_t[x_t, :], i.e. ONE
    `ctdd_lbjf_step` launch with CTDD_STEP_CORRECTOR on the CRM branch (K5 + K7 fused).
    The reference body only runs when D == S (it multiplies the (N,D,S) ratios by the (N,S,S) `model.rate(t)` and so
    takes the rate row of the DIMENSION index, and it passes log-probabilities to Categorical as `probs`); nothing calls
    it.  This is the formula its docstring and the LBJF corrector (sampling.py:296-341) state: rate row of the STATE
    x_t, Categorical(logits=log posterior).  Parity: oracle restatement `oracle.samplers.lbjf_corrector_posterior`
    (reference fixture impossible: parity unpinned).  `t` may be a tensor only if all its entries are equal."""
    if torch.is_tensor(t):
        tv = t.reshape(-1)
        if tv.numel() > 1 and not bool((tv == tv[0]).all()):
            raise ValueError("lbjf_corrector_step: every sample shares one time (the reference multiplies a scalar t by ones((N,)))")
        t = float(tv[0])
    t32 = torch.tensor([t], dtype=torch.float64).to(torch.float32)
    t_ones = torch.full((N,), float(t32[0]), device=device, dtype=torch.float32)
    with torch.no_grad():
        logits = model(xt.long(), t_ones).float().contiguous()
    lt = getattr(cfg.loss, "logit_type", "direct")
    _refuse_absorbing(model)
    pr = model.process
    q = pr.tables(t32, want_qt0=True)[0][0] if lt != "direct" else None
    beta = float(pr.beta(t32)[0])
    key = seed if seed is not None else _fresh_seed()
    xi = xt.to(torch.int32).contiguous()
    if xt_target is None or xt_target is xt or torch.equal(xt_target, xt):
        out = native.lbjf_step(native.BRANCH_CRM, lt, logits, xi, q, pr.base_rate, beta, cfg.sampler.eps_ratio, float(h),
                               native.STEP_CORRECTOR, E, key, 0, want_probs=want_probs)
    else:
        # xt_target != xt (sampling.py:1064-1067, 1076-1080): ratios and forward-rate row of x_t, the own-state mask and the
        # diagonal at x_target.  K5 gives R^ = ratio * R_t[x_t, :]; add the corrector's forward row, zero the target's entry,
        # and the Euler posterior + categorical draw of K7 run on those rates with x_target as the state.  The rate row's own
        # entry R_t[x_t, x_t] = -sum of the row is not a jump rate: it is zeroed too (as written, the reference leaves that
        # negative number in the "posterior" whenever x_target != x_t and its log is NaN).
        rate_t = pr.rate(t32)                                               # (1, S, S) = beta(t) R
        rr, _ = native.reverse_rates(native.BRANCH_CRM, lt, logits, xi, q.unsqueeze(0) if q is not None else None, rate_t,
                                     cfg.sampler.eps_ratio, want_ratio=False)
        rr = rr + rate_t[0][xt.long()]
        tgt = xt_target.to(torch.int32).contiguous()
        rr.scatter_(-1, xt.long().unsqueeze(-1), 0.0)
        rr.scatter_(-1, tgt.long().unsqueeze(-1), 0.0)
        out = native.lbjf_from_rates(rr.contiguous(), tgt, float(h), E, key, 0, want_probs=want_probs)
    return (out[0].long(), out[1]) if want_probs else out.long()


# Names that shipped configs still use but the reference never registers: resolve
# them to the sampler the authors' scripts substitute by hand.
for _alias, _cls in (("TauLeaping", TauL), ("ElboTauL", TauL), ("CRMTauL", TauL), ("LBJFSampling", LBJF),
                     ("CRMLBJF", LBJF), ("ElboLBJF", LBJF), ("CRMebmLBJF", LBJF), ("PCTauLeaping", PCTauL)):
    sampling_utils.register_alias(_alias, _cls)


@sampling_utils.register_sampler
class AbsorbingLeap(_Conditioned):
    """Reverse sampler of the absorbing-state ("masked") process (lib.models.forward_model.AbsorbingRate; not in the reference).
    Unmasked entries never move; per step a masked entry unmasks with one scalar probability and then takes a state drawn from
    the network's softmax over the states other than the mask: one network forward and one ctdd_absorb_step launch
    (csrc/absorb.hip) per step, no table, no Poisson draw, no host sync inside the loop.

    cfg.sampler.rule: "ancestral" (default; (a(t-h) - a(t)) / (1 - a(t)), the exact posterior for a fixed network), "euler"
    (min(1, h w(t))) or "tauleap" (lam exp(-lam), lam = h w(t)) -- AbsorbingRate.unmask_prob.  num_steps and min_t as in TauL: the
    grid is linspace(max_t, min_t, num_steps) followed by 0; after the loop one forward at min_t assigns every entry that is
    still masked its argmax.  `sample(model, N)` starts from the all-mask state and returns (x int (N, D), changed per step / N);
    `inpaint(model, x_known, mask)` (mask True = held, as in the conditional samplers) starts the held entries at their known
    value, which is all it takes: they are not masked, so no step touches them.

    cfg.sampler.temperature (default 1.0, positive), cfg.sampler.top_k (default 0: off) and cfg.sampler.top_p (default 1.0, in (0, 1]),
    here and in the three samplers built on this one: a masked entry's state is drawn from the softmax of logits / temperature,
    truncated to its top_k most likely states and then to the shortest prefix of them whose mass reaches top_p, and renormalised.
    Unless all three are at their defaults, every iteration launches ctdd_absorb_filter once, in place on the network's logits,
    before its step kernel (one more read and write of the masked rows); the closing forward is not filtered, the argmax being the
    same.  At the defaults nothing is launched and the sampler is bit for bit what it is without the keys.  Held entries of `inpaint`
    are not masked, so their rows are skipped.  The likelihood bounds of lib/likelihood.py describe the unfiltered samplers only."""

    def __init__(self, cfg):
        self.cfg = cfg
        self.D = cfg.model.concat_dim
        self.S = cfg.data.S
        s = cfg.sampler
        self.num_steps, self.min_t, self.max_t = s.num_steps, s.min_t, cfg.training.max_t
        self.rule = getattr(s, "rule", "ancestral")
        from ctdd.process import UNMASK_RULES
        if self.rule not in UNMASK_RULES:
            raise ValueError(f"sampler.rule must be one of {UNMASK_RULES}, got {self.rule!r}")
        temperature, top_k, top_p = getattr(s, "temperature", 1.0), getattr(s, "top_k", 0), getattr(s, "top_p", 1.0)
        try:
            self.temperature = float(temperature)
        except (TypeError, ValueError):
            self.temperature = float("nan")
        if not 0.0 < self.temperature < float("inf"):
            raise ValueError(f"sampler.temperature must be positive and finite, got {temperature!r}")
        if isinstance(top_k, bool) or not isinstance(top_k, (int, np.integer)) or top_k < 0:
            raise ValueError(f"sampler.top_k must be a non-negative integer (0: off), got {top_k!r}")
        self.top_k = int(top_k)
        try:
            self.top_p = float(top_p)
        except (TypeError, ValueError):
            self.top_p = float("nan")
        if not 0.0 < self.top_p <= 1.0:
            raise ValueError(f"sampler.top_p must lie in (0, 1], got {top_p!r}")
        self.filtered = not native.absorb_filter_is_neutral(self.temperature, self.top_k, self.top_p)
        self.seed = None              # set to an int for a fixed Philox key
        self.rank_stream = 0          # added to the key by the multi-GPU driver (ctdd/distributed.py)

    _key = _GridSampler._key

    def _filter(self, logits, x, m):
        """The step's logits with the masked rows tempered and truncated, in place (the sampler owns them for the length of a step:
        borrow_engine_output); nothing is launched at the neutral values."""
        if self.filtered:
            native.absorb_filter(logits, x, m, self.temperature, self.top_k, self.top_p, out=logits)
        return logits

    @staticmethod
    def _process(model):
        pr = getattr(model, "process", None)
        if getattr(pr, "kind", None) != "absorbing":
            raise ValueError("AbsorbingLeap needs a model on the absorbing process (AbsorbingRate, e.g. AbsorbingBertEMA)")
        return pr

    def sample(self, model, N):
        m = self._process(model).mask_state
        x = torch.full((int(N), self.D), m, dtype=torch.int32, device=torch.device(model.device))
        return self._loop(model, x)

    def inpaint(self, model, x_known, mask):
        m = self._process(model).mask_state
        N, xk, held = self._held(x_known, mask)
        if bool((xk[held] == m).any()):
            raise ValueError(f"x_known: a held entry is the mask state {m}")
        if bool(held.all()):
            return xk.numpy().astype(int)
        dev = torch.device(model.device)
        x = torch.where(held.to(dev), xk.to(dev), torch.full((), m, dtype=torch.int32, device=dev))
        return self._loop(model, x.contiguous())[0]

    def _advance(self, logits, x, m, p, key, i, changed):
        """Step i of the grid on the network's logits: every masked entry unmasks with probability p."""
        return native.absorb_step(logits, x, m, p, 0, key, i, changed=changed)

    def _loop(self, model, x):
        pr = self._process(model)
        m, N, dev, key = pr.mask_state, x.shape[0], x.device, self._key()
        ts = np.concatenate((np.linspace(self.max_t, self.min_t, self.num_steps), np.array([0])))
        t64 = torch.from_numpy(ts)
        # every step's unmasking probability on the host, before the loop (fp64 schedules; the network sees the fp32 times)
        p = torch.clamp(pr.unmask_prob(t64[:-1], t64[:-1] - t64[1:], self.rule), 0.0, 1.0).tolist()
        t32 = t64[:-1].to(torch.float32)
        changed = torch.zeros(self.num_steps + 1, dtype=torch.int32, device=dev)
        with torch.no_grad(), borrow_engine_output(model, bf16_logits=False, uniform_time=True):
            for i in range(self.num_steps):
                logits = self._filter(_GridSampler._net_logits(model, x, _GridSampler._t_ones(t32, i, N, dev)), x, m)
                x = self._advance(logits, x, m, p[i], key, i, changed[i:i + 1])
            logits = _GridSampler._net_logits(model, x, torch.full((N,), float(np.float32(self.min_t)), device=dev))
            x = native.absorb_step(logits, x, m, 1.0, native.ABSORB_ARGMAX, key, self.num_steps, changed=changed[self.num_steps:])
        return x.cpu().numpy().astype(int), (changed[:self.num_steps].cpu().numpy() / N).tolist()


@sampling_utils.register_sampler
class AbsorbingConfidence(AbsorbingLeap):
    """Confidence-ordered unmasking for the absorbing-state process (MaskGIT-style decoding; not in the reference).  Grid, rules,
    seed, rank_stream, `sample` and `inpaint` are AbsorbingLeap's, and so is the host-side fp64 p of every step -- but p is spent as a
    count, not as a coin per row: a step proposes a candidate for every masked entry (ctdd_absorb_propose: the state the plain step
    would draw, or the argmax, with its log-probability as the score) and commits, per sample, the ceil(p M_n) candidates with the
    largest score among the sample's own M_n masked entries (ctdd_absorb_commit).  One network forward and two launches per step,
    no host sync inside the loop.  Held entries of `inpaint` are not masked: they are neither counted nor moved.

    cfg.sampler.conf_temp (default 1.0): step i of num_steps adds conf_temp (1 - (i + 1) / num_steps) times a standard Gumbel variate
    to the scores, an annealed randomisation of the ranking (0 ranks by the log-probability alone).  cfg.sampler.candidate: "sample"
    (default) or "argmax".  The closing forward at min_t with its argmax step is the parent's.  Under a temperature / top_k / top_p
    filter (AbsorbingLeap) the score is the candidate's log-probability under the filtered distribution."""

    CANDIDATES = ("sample", "argmax")

    def __init__(self, cfg):
        super().__init__(cfg)
        self.conf_temp = float(getattr(cfg.sampler, "conf_temp", 1.0))
        self.candidate = getattr(cfg.sampler, "candidate", "sample")
        if self.candidate not in self.CANDIDATES:
            raise ValueError(f"sampler.candidate must be one of {self.CANDIDATES}, got {self.candidate!r}")

    def _advance(self, logits, x, m, p, key, i, changed):
        """Step i of the grid: a candidate and a score for every masked entry, then per sample the ceil(p M_n) best-scored commit."""
        flags = native.ABSORB_ARGMAX if self.candidate == "argmax" else 0
        cand, score = native.absorb_propose(logits, x, m, self.conf_temp * (1.0 - (i + 1) / self.num_steps), flags, key, i)
        return native.absorb_commit(x, cand, score, m, p_unmask=p, changed=changed)


REMASK_STRATEGIES = ("cap", "rescale", "conf")


def remask_schedule(p, strategy, eta, active=None):
    """(sigma, p_prime), two lists of fp64: the per-step remask probability of a committed entry and the raised unmasking probability
    that keeps the expected masked share of AbsorbingLeap's chain.  p: AbsorbingLeap's per-step unmasking probabilities in [0, 1];
    active: per-step booleans (None: every step), sigma_k = 0 where false.  Host arithmetic only.

    With surv_0 = 1 and surv_{k+1} = surv_k (1 - p_k) the masked share AbsorbingLeap has before step k, a step that unmasks with p'_k
    and remasks the unmasked share with sigma_k leaves surv_k (1 - p'_k) + (1 - surv_k) sigma_k masked; equating that to surv_{k+1} gives
        p'_k = p_k + sigma_k (1 - surv_k) / surv_k                (p'_k = p_k where surv_k == 0: nothing is masked),
    and p'_k <= 1 iff sigma_k <= sigma_max_k = min(1, surv_{k+1} / (1 - surv_k)) (sigma_k = 0 at surv_k == 1: nothing is unmasked).
    "cap" and "conf": sigma_k = min(eta, sigma_max_k); "rescale": sigma_k = eta sigma_max_k.  eta = 0 returns p itself."""
    if strategy not in REMASK_STRATEGIES:
        raise ValueError(f"remask strategy must be one of {REMASK_STRATEGIES}, got {strategy!r}")
    eta = float(eta)
    if not 0.0 <= eta <= 1.0:
        raise ValueError(f"remask eta must lie in [0, 1], got {eta!r}")
    p = [float(v) for v in p]
    if any(not 0.0 <= v <= 1.0 for v in p):
        raise ValueError("remask_schedule: every p must lie in [0, 1]")
    active = [True] * len(p) if active is None else [bool(v) for v in active]
    if len(active) != len(p):
        raise ValueError(f"remask_schedule: {len(active)} active flags for {len(p)} steps")
    sigma, p_prime, surv = [], [], 1.0
    for pk, on in zip(p, active):
        nxt = surv * (1.0 - pk)
        sk = 0.0
        if on and surv < 1.0:
            smax = min(1.0, nxt / (1.0 - surv))
            sk = eta * smax if strategy == "rescale" else min(eta, smax)
        sigma.append(sk)
        p_prime.append(min(1.0, pk + sk * (1.0 - surv) / surv) if surv > 0.0 and sk > 0.0 else pk)
        surv = nxt
    return sigma, p_prime


@sampling_utils.register_sampler
class AbsorbingRemask(AbsorbingLeap):
    """AbsorbingLeap with remasking (after ReMDM, Wang et al.; not in the reference): at every step each committed free entry returns to
    the mask state with a small probability sigma_k, and the unmasking probability is raised to p'_k so that the expected masked share
    after every step stays AbsorbingLeap's (remask_schedule; derived for this chain, which starts all-masked at max_t).  The trained
    network is used as is; a remasked entry is drawn again at a later step, from the logits of that step.  Grid, rules, seed,
    rank_stream, `sample`, `inpaint` and the closing argmax forward are the parent's; sigma and p' of every step are computed on the
    host before the loop; one network forward and one ctdd_absorb_remask_step launch per step, no host sync inside the loop.

    cfg.sampler.remask: "cap" (default; sigma_k = min(eta, sigma_max_k)), "rescale" (eta sigma_max_k) or "conf" (cap's sigma_k as the
    per-sample mean, spread over the committed entries in proportion to exp(-conf / remask_temp), conf the probability at which the
    entry committed: a second launch per step, ctdd_absorb_remask_norm, and a conf buffer carried across the steps, 1 at the start so
    that held entries weigh least).  cfg.sampler.remask_eta in [0, 1] (default 0.02, untuned; 0: AbsorbingLeap bit for bit under the same seed);
    cfg.sampler.remask_temp (default 1.0, at least 0.02); cfg.sampler.remask_window = (t_on, t_off) (default: the whole grid): step k
    remasks iff t_off <= t_k <= t_on.  `inpaint` hands the held mask to the kernel: a held entry is never remasked.  After a run
    `remasked` holds the per-step number of remasked entries over N, as `changed` holds the entries that left the mask state.  Under a
    temperature / top_k / top_p filter (AbsorbingLeap) the "conf" weight is the probability the entry committed at under the filtered
    distribution."""

    def __init__(self, cfg):
        super().__init__(cfg)
        s = cfg.sampler
        self.remask = getattr(s, "remask", "cap")
        if self.remask not in REMASK_STRATEGIES:
            raise ValueError(f"sampler.remask must be one of {REMASK_STRATEGIES}, got {self.remask!r}")
        self.remask_eta = float(getattr(s, "remask_eta", 0.02))
        if not 0.0 <= self.remask_eta <= 1.0:
            raise ValueError(f"sampler.remask_eta must lie in [0, 1], got {self.remask_eta!r}")
        self.remask_temp = float(getattr(s, "remask_temp", 1.0))
        if not self.remask_temp >= 0.02:
            raise ValueError(f"sampler.remask_temp must be at least 0.02, got {self.remask_temp!r}")
        window = getattr(s, "remask_window", None)
        if window is None:
            window = (float("inf"), float("-inf"))
        try:
            t_on, t_off = (float(v) for v in window)
        except (TypeError, ValueError):
            raise ValueError(f"sampler.remask_window must be a pair (t_on, t_off), got {window!r}") from None
        if not t_on >= t_off:
            raise ValueError(f"sampler.remask_window = (t_on, t_off) needs t_on >= t_off, got {window!r}")
        self.remask_window = (t_on, t_off)
        self.remasked = []

    def inpaint(self, model, x_known, mask):
        m = self._process(model).mask_state
        N, xk, held = self._held(x_known, mask)
        if bool((xk[held] == m).any()):
            raise ValueError(f"x_known: a held entry is the mask state {m}")
        if bool(held.all()):
            return xk.numpy().astype(int)
        dev = torch.device(model.device)
        held = held.to(dev)
        x = torch.where(held, xk.to(dev), torch.full((), m, dtype=torch.int32, device=dev))
        return self._loop(model, x.contiguous(), held.contiguous())[0]

    def schedule(self, pr):
        """(t64 of the grid with its closing 0, sigma, p') of a run on the process pr: the host side of the loop."""
        ts = np.concatenate((np.linspace(self.max_t, self.min_t, self.num_steps), np.array([0])))
        t64 = torch.from_numpy(ts)
        p = torch.clamp(pr.unmask_prob(t64[:-1], t64[:-1] - t64[1:], self.rule), 0.0, 1.0).tolist()
        t_on, t_off = self.remask_window
        sigma, p_prime = remask_schedule(p, self.remask, self.remask_eta, [t_off <= t <= t_on for t in ts[:-1].tolist()])
        return t64, sigma, p_prime

    def _loop(self, model, x, held=None):
        pr = self._process(model)
        m, N, dev, key, K = pr.mask_state, x.shape[0], x.device, self._key(), self.num_steps
        t64, sigma, p = self.schedule(pr)
        t32 = t64[:-1].to(torch.float32)
        counts = torch.zeros((K, 2), dtype=torch.int32, device=dev)
        closing = torch.zeros(1, dtype=torch.int32, device=dev)
        by_conf = self.remask == "conf"
        conf = torch.ones(x.shape, dtype=torch.float32, device=dev) if by_conf else None
        norm = torch.empty((N, 2), dtype=torch.float32, device=dev) if by_conf else None
        with torch.no_grad(), borrow_engine_output(model, bf16_logits=False, uniform_time=True):
            for i in range(K):
                logits = self._filter(_GridSampler._net_logits(model, x, _GridSampler._t_ones(t32, i, N, dev)), x, m)
                if by_conf:
                    native.absorb_remask_norm(x, m, conf, held, self.remask_temp, out=norm)
                    native.absorb_remask_step(logits, x, m, p[i], sigma[i], held, conf, norm, self.remask_temp, native.ABSORB_REMASK_CONF, key, i,
                                              out=x, conf_out=conf, counts=counts[i])
                else:
                    native.absorb_remask_step(logits, x, m, p[i], sigma[i], held, seed=key, offset=i, out=x, counts=counts[i])
            logits = _GridSampler._net_logits(model, x, torch.full((N,), float(np.float32(self.min_t)), device=dev))
            x = native.absorb_step(logits, x, m, 1.0, native.ABSORB_ARGMAX, key, K, changed=closing)
        counts = counts.cpu().numpy()
        self.remasked = (counts[:, 1] / N).tolist()
        return x.cpu().numpy().astype(int), (counts[:, 0] / N).tolist()


@sampling_utils.register_sampler
class AbsorbingFirstHit(AbsorbingLeap):
    """First-hitting sampler for the absorbing-state process (Zheng et al., "Masked diffusion models are secretly time-agnostic masked
    models and exploit inaccurate categorical sampling"; not in the reference): the reverse chain of the fixed network simulated event
    by event, with no time grid and so no time-discretisation error.  Write c(t) = 1 - alpha(t).  Given that an entry is masked at
    level c, the level at which it was masked is uniform on (0, c), independently over the entries; with M entries masked at level c
    the next one to unmask is therefore uniform among the M, and it unmasks at the largest of M uniforms on (0, c), c u^(1/M).  In
    logs: L <- L + log(u) / M, then M - 1 entries are masked.  The network is evaluated at the time of that level,
    DeviceForwardProcess.time_of_alpha(1 - exp(L)), per sample: this is the continuous-time sampler whose likelihood
    lib/likelihood.py's spacing = "alpha" bound describes.

    Seed, rank_stream, `sample`, `inpaint` and the closing argmax forward at min_t are AbsorbingLeap's.  Mmax, the largest masked count
    at the start (D for `sample`, from the held mask for `inpaint`), sets k = ceil(Mmax / num_steps) events per forward and
    ceil(Mmax / k) iterations: num_steps >= D is the exact sampler, one event and one forward each; a smaller num_steps buys fewer
    forwards by drawing k events from the logits at the first event's time, which is an approximation (the later events of an
    iteration see neither the earlier ones' states nor their own, later, times).  Per iteration: ctdd_absorb_hit_time (each sample's
    masked count, event levels, event count and network time, all kept on the device), model(x, t_eval) with per-sample times, then
    ctdd_absorb_hit_step in place (that many masked entries, uniformly, each with the state AbsorbingLeap's step would draw for it).
    Two launches per iteration, no host sync inside the loop.  Events that would fall below the level of min_t are not taken: their
    entries are left to the closing step, as the grid samplers leave theirs.  A sample with fewer masked entries than Mmax runs out
    of events early and is left alone from then on.

    cfg.sampler.candidate: "sample" (default) or "argmax".  cfg.sampler.rule has no meaning here: anything but the default is refused.
    `sample` returns (x, changed per iteration / N); after a run `times` holds the (iterations, N) fp32 evaluation times (min_t where
    a sample had no event).  A temperature / top_k / top_p filter (AbsorbingLeap) is applied to every iteration's logits before
    ctdd_absorb_hit_step: with top_k = 1 the "sample" candidate is the "argmax" candidate."""

    def __init__(self, cfg):
        super().__init__(cfg)
        if self.rule != "ancestral":
            raise ValueError(f"sampler.rule does not apply to AbsorbingFirstHit (it has no grid step to fill), got {self.rule!r}")
        self.candidate = getattr(cfg.sampler, "candidate", "sample")
        if self.candidate not in AbsorbingConfidence.CANDIDATES:
            raise ValueError(f"sampler.candidate must be one of {AbsorbingConfidence.CANDIDATES}, got {self.candidate!r}")
        if int(self.num_steps) < 1:
            raise ValueError(f"sampler.num_steps must be at least 1, got {self.num_steps!r}")
        self.times = np.zeros((0, 0), dtype=np.float32)

    def inpaint(self, model, x_known, mask):
        m = self._process(model).mask_state
        N, xk, held = self._held(x_known, mask)
        if bool((xk[held] == m).any()):
            raise ValueError(f"x_known: a held entry is the mask state {m}")
        if bool(held.all()):
            return xk.numpy().astype(int)
        mmax = int((~held).sum(dim=1).max())                     # on the host, before the loop
        dev = torch.device(model.device)
        x = torch.where(held.to(dev), xk.to(dev), torch.full((), m, dtype=torch.int32, device=dev))
        return self._loop(model, x.contiguous(), mmax)[0]

    def plan(self, mmax):
        """(k, iterations): events per forward and forwards for a largest starting masked count of mmax."""
        k = -(-int(mmax) // int(self.num_steps))
        return k, -(-int(mmax) // k)

    def _loop(self, model, x, mmax=None):
        pr = self._process(model)
        m, N, dev, key = pr.mask_state, x.shape[0], x.device, self._key()
        k, iters = self.plan(x.shape[1] if mmax is None else mmax)
        # the start and closing levels on the host in fp64, before the loop
        logc0, log_cmin = torch.log(1 - pr.alpha(torch.tensor([self.max_t, self.min_t], dtype=torch.float64))).tolist()
        logc = torch.full((N,), logc0, dtype=torch.float64, device=dev)
        counts = torch.empty((N,), dtype=torch.int32, device=dev)
        times = torch.empty((iters, N), dtype=torch.float32, device=dev)
        changed = torch.zeros(iters + 1, dtype=torch.int32, device=dev)
        flags = native.ABSORB_ARGMAX if self.candidate == "argmax" else 0
        with torch.no_grad(), borrow_engine_output(model, bf16_logits=False, uniform_time=False):
            for i in range(iters):
                native.absorb_hit_time(x, logc, m, k, log_cmin, pr.p, self.min_t, self.max_t, key, i, counts=counts, t_eval=times[i], out=logc)
                logits = self._filter(_GridSampler._net_logits(model, x, times[i]), x, m)
                native.absorb_hit_step(logits, x, counts, m, flags, key, i, out=x, changed=changed[i:i + 1])
            logits = _GridSampler._net_logits(model, x, torch.full((N,), float(np.float32(self.min_t)), device=dev))
            x = native.absorb_step(logits, x, m, 1.0, native.ABSORB_ARGMAX, key, iters, changed=changed[iters:])
        self.times = times.cpu().numpy()
        return x.cpu().numpy().astype(int), (changed[:iters].cpu().numpy() / N).tolist()
