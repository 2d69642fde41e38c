"""Shared cases of the masked-attention tests (test_attn_cases_cpu.py, test_gpu_attention_masks.py, test_gpu_attention_fp64.py):
the mask of every attention mode restated in torch, an fp64 reference of softmax attention with dropout on the probabilities,
the operand layouts of the engine, thin drivers of the seven attention entry points, and the exact readback of a kernel's
visibility matrix.  Nothing here touches the GPU at import; the drivers import the package inside the functions.

Canonical tensors are [B, H, T, hd]; the engine's rows are (B*T, E) with E = H hd, head h in columns h hd .. h hd + hd - 1.

The readback.  With q = 0 every visible key of query i gets probability 1 / n_i (n_i = its number of visible keys), whatever k
holds.  With V one-hot over a block of hd keys (V[j0 + c, c] = 1) output column c of query i is p_i,j0+c keep_i,j0+c / (1 - p):
non-zero exactly when key j0 + c is visible and kept.  Through the backward the same holds for dV with dO one-hot over a block of
hd queries: dV[j, c] = p_i0+c,j keep_i0+c,j / (1 - p).  Both read a kernel's mask (and its dropout bits) exactly, in bf16 too, since
1 / n and 1 / (n (1 - p)) are far from the underflow of either format."""
import math

import torch

MODES = (0, 1, 2, 3)


def n_keys(mode, Tq):
    """Keys of a mode with Tq queries: the readout attends [temb | l2r | r2l]; mode 3 is taken square here."""
    return 2 * Tq + 1 if mode == 2 else Tq


def allowed(mode, Tq, Tk=None):
    """bool [Tq, Tk]: query i sees key j (attn_allowed of csrc/hollow_train_kernels.hip; mode 3: every key)."""
    Tk = n_keys(mode, Tq) if Tk is None else Tk
    i = torch.arange(Tq)[:, None]
    j = torch.arange(Tk)[None, :]
    if mode == 0:
        return j <= i
    if mode == 1:
        return j >= i
    if mode == 2:
        assert Tk == 2 * Tq + 1
        return (j == 0) | ((j >= 1) & (j <= Tq) & (j - 1 <= i)) | ((j > Tq) & (j - Tq - 1 >= i))
    if mode == 3:
        return torch.ones((Tq, Tk), dtype=torch.bool)
    raise ValueError(f"attention mode {mode}")


def attention_fp64(q, k, v, mode, keep=None, inv_keep=1.0):
    """q [B, H, Tq, hd], k / v [B, H, Tk, hd] (double) -> (O [B, H, Tq, hd], row log-sum-exp [B, H, Tq]).
    P = softmax(mask(q k^T / sqrt(hd))), O = (P keep inv_keep) @ v: the normaliser runs over every visible key, the dropout acts on
    the normalised probabilities (nn.MultiheadAttention).  Differentiable."""
    assert q.dtype == k.dtype == v.dtype == torch.float64
    ok = allowed(mode, q.shape[2], k.shape[2]).to(q.device)
    s = (q @ k.transpose(-1, -2)) / math.sqrt(q.shape[-1])
    s = s.masked_fill(~ok, float("-inf"))
    lse = torch.logsumexp(s, -1)
    p = torch.exp(s - lse[..., None])
    if keep is not None:
        p = p * (keep.to(p.dtype) * inv_keep)
    return p @ v, lse


# ---------------------------------------------------------------------------------------------------- the numeric cases
FP64_TQ = (1, 33, 64, 97, 129)          # one query; one past a 32-tile; two whole tiles; ragged; one past the 128-query workgroup
FP64_B, FP64_H = 2, 3


def case_operands(mode, Tq, hd, B=FP64_B, H=FP64_H):
    """N(0, 1) q, k, v and the output weight of one numeric case, fp32 values drawn on the CPU (the same on every machine)."""
    g = torch.Generator().manual_seed(1000 * mode + 10 * Tq + hd)
    Tk = n_keys(mode, Tq)
    return [torch.randn((B, H, T, hd), generator=g) for T in (Tq, Tk, Tk, Tq)]


def bf16_lse_deviation(hds=(16, 32)):
    """Largest |log-sum-exp of attention_fp64 on bf16-rounded operands - on the operands themselves| over the numeric cases of
    the matrix-core kernels: what rounding q and k to bf16 alone does to the row statistics."""
    worst = 0.0
    for mode in (0, 1, 2):
        for Tq in FP64_TQ:
            for hd in hds:
                q, k, v, _ = case_operands(mode, Tq, hd)
                exact = attention_fp64(q.double(), k.double(), v.double(), mode)[1]
                r = lambda t: t.to(torch.bfloat16).double()
                worst = max(worst, float((attention_fp64(r(q), r(k), r(v), mode)[1] - exact).abs().max()))
    return worst


BF16_LSE_DEVIATION = 8.123e-3           # bf16_lse_deviation(), pinned by test_attn_cases_cpu.py
BF16_LSE_BAR = 4 * BF16_LSE_DEVIATION   # the matrix-core kernels' bar: four times that, room for the fp32 accumulation order


# ---------------------------------------------------------------------------------------------------- operand layouts
def rows(x):
    """[B, H, T, hd] -> (B*T, H hd)"""
    B, H, T, hd = x.shape
    return x.permute(0, 2, 1, 3).reshape(B * T, H * hd)


def heads(x, B, H):
    """(B*T, H hd) -> [B, H, T, hd]"""
    return x.reshape(B, x.shape[0] // B, H, x.shape[1] // H).permute(0, 2, 1, 3)


def packed_layout(mode, Tq, Tk):
    """Self-attention (modes 0 / 1, square mode 3) reads q, k, v out of the in-projection's (B*T, 3E) rows."""
    return mode in (0, 1) or (mode == 3 and Tq == Tk)


def engine_operands(q, k, v, mode, device="cuda"):
    """The engine's operands, fp32 on `device`: [qkv (B*T, 3E)] for the self-attention modes, [q (B*Tq, E), k, v (B*Tk, E)] for
    the readout."""
    if packed_layout(mode, q.shape[2], k.shape[2]):
        return [torch.cat([rows(q), rows(k), rows(v)], 1).float().contiguous().to(device)]
    return [rows(t).float().contiguous().to(device) for t in (q, k, v)]


def split_gradients(grads, B, H):
    """(dqkv, None, None) or (dq, dk, dv) in engine rows -> [dq, dk, dv] as [B, H, T, hd]"""
    if grads[1] is None:
        E = grads[0].shape[1] // 3
        grads = [grads[0][:, c * E:(c + 1) * E] for c in range(3)]
    return [heads(g, B, H) for g in grads]


def _shape(q, k):
    B, H, Tq, hd = q.shape
    return B, H, Tq, k.shape[2], hd


# ---------------------------------------------------------------------------------------------------- drivers
def inference_forward(kind, q, k, v, mode):
    """ctdd_hollow_attention (kind "fp32") / ctdd_hollow_attention_bf16 ("mfma": one bf16 product, "split": hi + lo pairs)
    -> (out fp32, out_hi, out_lo) as [B, H, Tq, hd]."""
    import ctypes as C
    from ctdd.hollow_engine import _AttnArgs, _lib
    lib = _lib()
    B, H, Tq, Tk, hd = _shape(q, k)
    E = H * hd
    ops = engine_operands(q, k, v, mode)
    dev = ops[0].device
    out = torch.full((B * Tq, E), float("nan"), device=dev)
    out_hi = torch.zeros((B * Tq, E), device=dev, dtype=torch.bfloat16)
    out_lo = torch.zeros((B * Tq, E), device=dev, dtype=torch.bfloat16)
    a = _AttnArgs()
    if len(ops) == 1:
        a.q, a.k, a.v = ops[0].data_ptr(), ops[0].data_ptr() + 4 * E, ops[0].data_ptr() + 8 * E
        a.q_bs = a.k_bs = a.v_bs = Tq * 3 * E
        a.q_rs = a.k_rs = a.v_rs = 3 * E
    else:
        a.q, a.k, a.v = (t.data_ptr() for t in ops)
        a.q_bs, a.k_bs, a.v_bs, a.q_rs, a.k_rs, a.v_rs = Tq * E, Tk * E, Tk * E, E, E, E
    a.B, a.Tq, a.Tk, a.H, a.hd, a.mode, a.scale = B, Tq, Tk, H, hd, mode, 1.0 / math.sqrt(hd)
    a.out, a.out_rs, a.out_hi, a.out_lo, a.split = out.data_ptr(), E, out_hi.data_ptr(), out_lo.data_ptr(), 1 if kind == "split" else 0
    fn = lib.ctdd_hollow_attention if kind == "fp32" else lib.ctdd_hollow_attention_bf16
    rc = fn(C.byref(a), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, (kind, mode, Tq, Tk, hd, rc)
    torch.cuda.synchronize()
    return tuple(heads(t, B, H) for t in (out, out_hi, out_lo))


class TrainForward:
    """One training forward (ctdd.hollow_train._attention_fwd; bf16: the matrix-core kernels, head dimension 16 / 32) and what
    its backward needs.  out / out_bf16 as [B, H, Tq, hd], stats [B, H, Tq, 4]."""

    def __init__(self, bf16, q, k, v, mode, p=0.0, rng=None, layer=0):
        from ctdd import hollow_train as ht
        B, H, Tq, Tk, hd = _shape(q, k)
        assert not bf16 or hd in (16, 32)
        self.meta = (B, Tq, Tk, H, hd, mode, float(p), rng if p > 0 else None, int(layer), bool(bf16))
        self.ops = engine_operands(q, k, v, mode)
        self.qkv = (self.ops + [None, None])[:3]
        self.out_rows, self.out_hi_rows, self.stats = ht._attention_fwd(*self.qkv, *self.meta)
        self.out = heads(self.out_rows, B, H)
        self.out_bf16 = None if self.out_hi_rows is None else heads(self.out_hi_rows, B, H)

    def backward(self, d_out, want_f32=True):
        """d_out [B, H, Tq, hd] -> ([dq, dk, dv] fp32 or None, their bf16 copies or None), each [B, H, T, hd]."""
        from ctdd import hollow_train as ht
        B, H = self.meta[0], self.meta[3]
        do = rows(d_out).float().contiguous().to(self.out_rows.device)
        grads, hi = ht._attention_bwd(*self.qkv, self.out_rows, self.stats, do, *self.meta, want_f32=want_f32)
        f32 = split_gradients(grads, B, H) if grads[0] is not None else None
        b16 = split_gradients(hi, B, H) if hi[0] is not None else None
        return f32, b16


FORWARDS = ("infer_fp32", "infer_mfma", "infer_split", "train_fp32", "train_mfma")
BACKWARDS = ("train_fp32", "train_mfma")


def forward_entry(name):
    """name in FORWARDS -> f(q, k, v, mode, **dropout) -> out fp32 [B, H, Tq, hd] (dropout: the training entries only)"""
    if name.startswith("infer_"):
        return lambda q, k, v, mode: inference_forward(name[6:], q, k, v, mode)[0]
    return lambda q, k, v, mode, **drop: TrainForward(name == "train_mfma", q, k, v, mode, **drop).out


def backward_entry(name):
    """name in BACKWARDS -> f(q, k, v, d_out, mode, **dropout) -> [dq, dk, dv] fp32: the forward of the same family, then the backward"""
    return lambda q, k, v, d_out, mode, **drop: TrainForward(name == "train_mfma", q, k, v, mode, **drop).backward(d_out)[0]


# ---------------------------------------------------------------------------------------------------- visibility readback
def _blocks(T, hd):
    return (T + hd - 1) // hd


def _one_hot_block(B, H, T, hd, blk):
    """[B, H, T, hd]: row blk hd + c holds e_c (block `blk` of hd rows; blk None: batch b carries block b)"""
    x = torch.zeros((B, H, T, hd))
    if blk is None:
        r = torch.arange(T)
        x[r // hd, :, r, r % hd] = 1.0
    else:
        r = torch.arange(blk * hd, min(T, (blk + 1) * hd))
        x[:, :, r, r - blk * hd] = 1.0
    return x


def read_visibility(forward, mode, Tq, hd, H, B=None, seed=0):
    """forward(q, k, v) -> out [., H, Tq, hd].  -> (pattern, values): [H, Tq, Tk] from ONE call whose batch index is the block
    index (B None: no dropout; the pattern must then hold whatever b and h), or [B, H, Tq, Tk] from one call per block with the
    same B and H (dropout: the Philox counter contains b)."""
    Tk = n_keys(mode, Tq)
    nblk = _blocks(Tk, hd)
    nb = nblk if B is None else B
    q = torch.zeros((nb, H, Tq, hd))
    k = torch.randn((nb, H, Tk, hd), generator=torch.Generator().manual_seed(seed))
    if B is None:
        out = forward(q, k, _one_hot_block(nb, H, Tk, hd, None)).detach().cpu()
        vals = out.permute(1, 2, 0, 3).reshape(H, Tq, nblk * hd)
    else:
        vals = torch.cat([forward(q, k, _one_hot_block(nb, H, Tk, hd, blk)).detach().cpu() for blk in range(nblk)], -1)
    vals = vals[..., :Tk]
    return vals != 0, vals


def read_visibility_bwd(backward, mode, Tq, hd, H, B=None, seed=0):
    """backward(q, k, v, d_out) -> dV [., H, Tk, hd] (a forward with q = 0 for the stats, then the backward).  Same returns as
    read_visibility, read from dV[j, c] = p(i0 + c, j) keep / (1 - p)."""
    Tk = n_keys(mode, Tq)
    nblk = _blocks(Tq, hd)
    nb = nblk if B is None else B
    g = torch.Generator().manual_seed(seed)
    q = torch.zeros((nb, H, Tq, hd))
    k = torch.randn((nb, H, Tk, hd), generator=g)
    v = torch.randn((nb, H, Tk, hd), generator=g)
    if B is None:
        dv = backward(q, k, v, _one_hot_block(nb, H, Tq, hd, None)).detach().cpu()             # [nblk, H, Tk, hd]
        vals = dv.permute(1, 0, 3, 2).reshape(H, nblk * hd, Tk)
    else:
        vals = torch.cat([backward(q, k, v, _one_hot_block(nb, H, Tq, hd, blk)).detach().cpu().transpose(-1, -2) for blk in range(nblk)], -2)
    vals = vals[..., :Tq, :]
    return vals != 0, vals


def visible_counts(mode, Tq):
    """n_i: visible keys of query i, [Tq]"""
    return allowed(mode, Tq).sum(-1)
