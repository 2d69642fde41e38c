"""Device-resident CTMC forward process: eigendecomposition on the host at construction (numpy
float64, exactly as lib/models/forward_model.py does), per-t tables by the K1 HIP kernel.

One object serves the four reference processes and the absorbing-state one (closed-form eigensystem, plus the scalars
alpha / time_of_alpha / elbo_weight / unmask_prob that its own objective and samplers run on); `lib.models.forward_model` wraps it with the
reference's class / attribute names."""
import math

import numpy as np
import torch

from . import native


def gaussian_target_rate_matrix(S, rate_sigma, Q_sigma):
    """Rate matrix with a discretised-Gaussian stationary law (forward_model.py:216-236).
    Pass 1 lays down the symmetric jump kernel exp(-k^2/rate_sigma^2) inside the 'hourglass'
    |i-j| < dist-to-border; pass 2 rescales, in place and in row-major order, every entry whose
    mirror is positive by the detailed-balance factor of the target."""
    R = np.zeros((S, S))
    kern = np.exp(-np.arange(0, S) ** 2 / (rate_sigma**2))
    mid = S // 2
    for i in range(S):
        if i < mid:
            j = np.arange(i + 1, S - i)
            R[i, j] = kern[j - i - 1]
        elif i > mid:
            j = np.arange(S - i, i)
            R[i, j] = kern[i - j - 1]
    denom = 2 * Q_sigma**2
    for i in range(S):
        ip = i + 1
        for j in range(S):
            mirror = R[j, i]
            if mirror > 0.0:
                jp = j + 1
                R[i, j] = mirror * np.exp(-(jp**2 - ip**2 + S * ip - S * jp) / denom)
    R = R - np.diag(np.diag(R))
    return R - np.diag(np.sum(R, axis=1))


def uniform_rate_matrix(S, rate_const):
    R = rate_const * (np.ones((S, S)) - np.eye(S))
    return R - np.diag(np.sum(R, axis=1))


def birth_death_rate_matrix(S):
    R = np.diag(np.ones((S - 1,)), 1) + np.diag(np.ones((S - 1,)), -1)
    return R - np.diag(np.sum(R, axis=1))


def absorbing_rate_matrix(S, rate_const, mask_state):
    """Every state jumps to `mask_state` at rate_const; the mask state's row is zero."""
    R = np.zeros((S, S))
    R[:, mask_state] = rate_const
    R -= rate_const * np.eye(S)
    R[mask_state, :] = 0.0
    return R


def absorbing_eigensystem(S, rate_const, mask_state):
    """(eigenvalues, V, W = V^-1) of absorbing_rate_matrix in closed form: V = I + (1 - e_m) e_m^T, W = I - (1 - e_m) e_m^T,
    eigenvalue 0 at index m and -rate_const elsewhere (an (S - 1)-fold eigenvalue: no numerical eigensolver)."""
    col = np.ones(S)
    col[mask_state] = 0.0
    V, W = np.eye(S), np.eye(S)
    V[:, mask_state] += col
    W[:, mask_state] -= col
    lam = np.full(S, -float(rate_const))
    lam[mask_state] = 0.0
    return lam, V, W


ABSORBING_T_FUNCS = ("loglinear", "log_sqr", "sqrt_cos", "log")
UNMASK_RULES = ("ancestral", "euler", "tauleap")


class DeviceForwardProcess:
    KINDS = ("gaussian", "uniform", "univar", "birthdeath", "absorbing")

    def __init__(self, kind, S, device, **p):
        if kind not in self.KINDS:
            raise ValueError(f"unknown forward process {kind}")
        self.kind, self.S, self.p, self.device = kind, int(S), dict(p), torch.device(device)
        if kind == "gaussian":
            R = gaussian_target_rate_matrix(S, p["rate_sigma"], p["Q_sigma"])
            lam, V = np.linalg.eig(R)
            W = np.linalg.inv(V)
        elif kind == "absorbing":
            m = self.mask_state = int(p["mask_state"])
            if not 0 <= m < self.S or self.S < 2:
                raise ValueError(f"absorbing process: mask_state {m} outside [0, S = {self.S})")
            if p["t_func"] not in ABSORBING_T_FUNCS:
                raise ValueError("Unknown t_func %s" % p["t_func"])
            if p["t_func"] == "loglinear" and float(p["rate_const"]) != 1.0:
                raise ValueError(f"absorbing process: t_func 'loglinear' takes rate_const = 1, got {p['rate_const']!r}")
            R = absorbing_rate_matrix(self.S, p["rate_const"], m)
            lam, V, W = absorbing_eigensystem(self.S, p["rate_const"], m)
        else:
            R = {"uniform": lambda: uniform_rate_matrix(S, p["rate_const"]),
                 "univar": lambda: uniform_rate_matrix(S, p["rate_const"]),
                 "birthdeath": lambda: birth_death_rate_matrix(S)}[kind]()
            lam, V = np.linalg.eigh(R)
            W = V.T
        f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a)).float().to(self.device).contiguous()
        self.base_rate, self.eigvals, self.eigvecs, self.right = f32(R), f32(lam), f32(V), f32(W)
        self.eigvecsT = f32(np.ascontiguousarray(V.T))
        self.normalise = kind != "uniform"       # UniformRate.transition does not row-normalise (A3)

    # ---- scalar schedules; t is a float32 tensor (any device) -> same device
    def integral(self, t):
        k, p = self.kind, self.p
        if k == "absorbing" and p["t_func"] == "loglinear":
            return -torch.log(1 - (1 - p["alpha_eps"]) * t)
        if k == "absorbing":
            k = "univar"                             # log_sqr / sqrt_cos / log: the time-warped uniform process's schedules
        if k == "gaussian" or (k == "univar" and p["t_func"] == "log"):
            return p["time_base"] * (p["time_exp"] ** t) - p["time_base"]
        if k == "uniform":
            return t
        if k == "univar":
            if p["t_func"] == "log_sqr":
                return torch.log(t**2 + 1)
            if p["t_func"] == "sqrt_cos":
                return -torch.sqrt(torch.cos(torch.pi / 2 * t))
            raise ValueError("Unknown t_func %s" % p["t_func"])
        smin, smax = p["sigma_min"], p["sigma_max"]
        return 0.5 * smin**2 * (smax / smin) ** (2 * t) - 0.5 * smin**2

    def beta(self, t):
        k, p = self.kind, self.p
        if k == "absorbing" and p["t_func"] == "loglinear":
            return (1 - p["alpha_eps"]) / (1 - (1 - p["alpha_eps"]) * t)
        if k == "absorbing":
            k = "univar"
        if k == "gaussian" or (k == "univar" and p["t_func"] == "log"):
            return p["time_base"] * math.log(p["time_exp"]) * (p["time_exp"] ** t)
        if k == "uniform":
            return torch.ones_like(t)
        if k == "univar":
            if p["t_func"] == "log_sqr":
                return 2 * t / (t**2 + 1)
            if p["t_func"] == "sqrt_cos":
                a = torch.pi / 2 * t
                return torch.pi / 4.0 * (torch.sin(a) / torch.sqrt(torch.cos(a)))
            raise ValueError("Unknown t_func %s" % p["t_func"])
        smin, smax = p["sigma_min"], p["sigma_max"]
        return smin**2 * (smax / smin) ** (2 * t) * math.log(smax / smin)

    def exponent(self, t, t_from=None):
        """Scalar multiplying the eigenvalues in q_{t|t_from}."""
        c = self.integral(t)
        if t_from is not None:
            c = c - self.integral(t_from)
        elif self.kind in ("univar", "absorbing"):   # transition(t) = transit_between(0,t) (:202-204)
            c = c - self.integral(torch.zeros_like(t))
        return c

    # ---- tables through the HIP kernel
    def _dev(self, t):
        return t.to(device=self.device, dtype=torch.float32).contiguous()

    def tables(self, t, *, t_from=None, between=False, want_qt0=True, want_qt0T=False, want_rate=False,
               want_noise_probs=False):
        """(qt0, qt0T, rate, noise_probs), each (nT,S,S) or None.  Scalars are evaluated on the
        device `t` lives on (host float32 for the samplers' grids = the reference's CPU values)."""
        c, b = self._dev(self.exponent(t, t_from)), self._dev(self.beta(t))
        right = self.right
        normalise = self.normalise
        if between:
            if self.kind == "birthdeath":
                raise AttributeError("BirthDeathForwardBase has no transit_between")
            if self.kind == "gaussian":
                right = self.eigvecsT              # reference uses eigvecs.T here (:298), kept
            normalise = self.kind != "uniform"
        return native.rate_table(self.eigvecs, right, self.eigvals, self.base_rate, c, b, self.S, normalise, 1e-8,
                                 want_qt0, want_qt0T, want_rate, want_noise_probs)

    def transition(self, t):
        return self.tables(t)[0]

    def rate(self, t):
        return self.tables(t, want_qt0=False, want_rate=True)[2]

    def transit_between(self, t1, t2):
        if self.kind == "uniform":
            return self.tables(t2 - t1)[0]
        return self.tables(t2, t_from=t1, between=True)[0]

    def rate_mat(self, y, t):
        """rate(t)[b, y, :] without materialising (B,S,S): beta(t) * base_rate[y]."""
        b = self._dev(self.beta(t)).view(-1, *([1] * y.dim()))
        return self.base_rate[y.long()] * b

    # ---- absorbing-state scalars; t a float tensor on any device -> same device (the kernels of csrc/absorb.hip take these, no table)
    def _absorbing(self, what):
        if self.kind != "absorbing":
            raise ValueError(f"{what} is defined for the absorbing process only (this one is {self.kind!r})")

    def alpha(self, t):
        """exp(-c(t)): the probability that an entry is still unmasked at t.  c(t) = rate_const (I(t) - I(0))."""
        self._absorbing("alpha")
        if self.p["t_func"] == "loglinear":
            return 1 - (1 - self.p["alpha_eps"]) * t
        return torch.exp(-self.p["rate_const"] * self.exponent(t))

    def time_of_alpha(self, a):
        """The inverse of alpha: the t with alpha(t) = a, in closed form for each of ABSORBING_T_FUNCS; a a float tensor, the dtype
        follows it (fp64 in: the reference of ctdd_absorb_hit_time, which states the same forms).
        loglinear (1 - a) / (1 - alpha_eps); log_sqr sqrt(a^(-1/rc) - 1); sqrt_cos (2 / pi) acos(r^2) with r = 1 + ln a / rc clamped
        to [0, 1] (a below alpha(1) = exp(-rc) has no preimage: t = 1); log log_{time_exp}(1 - ln a / (rc time_base))."""
        self._absorbing("time_of_alpha")
        p, a = self.p, torch.as_tensor(a)
        f, rc = p["t_func"], p["rate_const"]
        if f == "loglinear":
            return (1 - a) / (1 - p["alpha_eps"])
        if f == "log_sqr":
            return torch.sqrt(a ** (-1.0 / rc) - 1)
        if f == "sqrt_cos":
            r = torch.clamp(1 + torch.log(a) / rc, 0.0, 1.0)
            return (2 / math.pi) * torch.acos(r * r)
        return torch.log(1 - torch.log(a) / (rc * p["time_base"])) / math.log(p["time_exp"])

    def elbo_weight(self, t):
        """c'(t) alpha_t / (1 - alpha_t) with c' = rate_const beta(t): the weight of the masked cross entropy in the negative ELBO
        (1 / t for loglinear, where rate_const = 1)."""
        self._absorbing("elbo_weight")
        if self.p["t_func"] == "loglinear":
            return 1 / t
        a = self.alpha(t)
        return self.p["rate_const"] * self.beta(t) * a / (1 - a)

    def unmask_prob(self, t, h, rule="ancestral"):
        """Probability that a masked entry unmasks in the reverse step t -> t - h.  ancestral: (a(t-h) - a(t)) / (1 - a(t)), the
        exact posterior for a fixed p_theta (1 at t - h = 0); euler: min(1, h elbo_weight(t)); tauleap: lam exp(-lam) with
        lam = h elbo_weight(t), exactly one Poisson event (several are rejected, as TauL does for non-ordinal data)."""
        self._absorbing("unmask_prob")
        t = torch.as_tensor(t)
        if rule == "ancestral":
            a = self.alpha(t)
            return (self.alpha(t - h) - a) / (1 - a)
        lam = h * self.elbo_weight(t)
        if rule == "euler":
            return torch.clamp(lam, max=1.0)
        if rule == "tauleap":
            return lam * torch.exp(-lam)
        raise ValueError(f"unknown unmasking rule {rule!r}: one of {UNMASK_RULES}")
