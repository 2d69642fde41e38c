"""Training path of the masked ("enumerative") transformer on hand-written HIP kernels (reference: forward + `l.backward()`
through TAUnSDDM/lib/networks/hollow_networks.py:450-493 (TransformerEncoder), 859-960 (MaskedTransformer,
EnumerativeTransformer) and 90-132 (FiLM residual readout)).

`MaskedTrainer(model)(x, t)` computes the logits of an `EnumerativeTransformer` the way `BertTrainer` (ctdd/bert_train.py)
computes the x0-prediction transformer's.  logits[b, p] = readout(encoder(x_b with token p masked)[p]): the (B D') sequences
"sample b with token p masked" (D' = D - conditional_dim) exist as indices only and run through the encoder in chunks of
hollow_networks.enum_chunk_size() sequences, the last chunk with its true row count.

  per chunk     `ctdd_bert_embed` in enumerate mode over the window [r0, r0 + n) / `ctdd_bert_embed_enum_bwd`; the two dropouts;
                hollow_train.Forward.encoder: per layer `AttnBlockFn` and `MlpBlockFn` with Tq = Tk = T = D + 1 and attention mode 3 -- on
                `ctdd_bert_attention_short_train` / `_bwd` where T <= 64 and the head dimension is 4 or 8 (both shipped masked
                configs at D = 32; the maze config's T = 226 runs the generic kernels); `ctdd_bert_gather` in enumerate mode
                into the chunk's rows of ONE (B D', E) readout input / `ctdd_bert_gather_enum_bwd`
  after them    hollow_train.film_readout once over all (B D') rows; a conditional prefix gets all-zero logits

Parameters enter every chunk's Functions, so autograd sums their gradients over the chunks.  The (B, E) time embedding: the
embed kernel writes temb[b] from the sequence with p == conditional_dim, which every sample owns exactly once in the
enumeration, so the buffer all chunks share is complete when the last chunk has run -- and the readout runs after it.
Dropout masks are Philox(seed, step * 4096 + layer, element) with chunk-local element indices: every chunk takes its own
{seed, step} (a row of one cloned table, steps advancing by one per chunk), and the trainer's step moves past all of them, so
neither two chunks nor two forwards share a stream and a forward's masks stay put until its backward.
Precisions "fp32" (parity mode) and "bf16" (default) as BertTrainer.  The MLP readout has no training Functions:
`training_supported` is false for it.
"""
import ctypes as C

import torch

from . import bert_engine, native
from .bert_engine import _BertEmbedArgs
from .bert_train import lib as _bert_lib
from .hollow_train import Forward, Trainer, _ck, _st, film_readout, short_attention_applies
from .plan_launch import set_state_ptr, unwrap

_P, _I, _I64 = C.c_void_p, C.c_int, C.c_int64
MAX_CHUNK = 65535              # sequences per launch (a grid dimension of the embed and attention kernels)


class _BertEmbedEnumBwdArgs(C.Structure):
    _fields_ = [("x64", _P), ("x32", _P), ("g", _P), ("B", _I), ("D", _I), ("E", _I), ("S", _I), ("cond", _I), ("rows", _I),
                ("r0", _I64), ("dw", _P), ("db", _P)]


_sigs_done = False


def lib():
    global _sigs_done
    l = _bert_lib()
    if not _sigs_done:
        for name, argt in (("ctdd_bert_embed_enum_bwd", [_P, _P]), ("ctdd_bert_gather_enum_bwd", [_P, _I64, _I, _I, _I, _I, _I, _P, _P])):
            fn = getattr(l, name)
            fn.argtypes, fn.restype = argt, _I
        _sigs_done = True
    return l


def chunk_walk(total, chunk):
    """The windows (r0, n) of the enumeration [0, total) in chunks of `chunk` sequences; the last one is ragged."""
    chunk = max(1, min(int(chunk), MAX_CHUNK))
    return [(r0, min(chunk, total - r0)) for r0 in range(0, total, chunk)]


class EnumEmbedFn(torch.autograd.Function):
    """(B, D) integer states, (B,) times, the window [r0, r0 + n) -> the encoder input (n, D + 1, E) of its sequences; temb (B, E),
    shared by the chunks, receives the time embedding of every sample whose first masked sequence lies in the window."""

    @staticmethod
    def forward(ctx, x, t, w_in, b_in, pe, temb, r0_dev, meta):
        S, temb_scale, cond, r0, n = meta
        B, D = x.shape
        E = w_in.numel()
        out = torch.empty((n, D + 1, E), dtype=torch.float32, device=x.device)
        a = _BertEmbedArgs()
        set_state_ptr(a, x, "MaskedTrainer")
        wv, bv = w_in.detach().reshape(-1).contiguous(), b_in.detach().contiguous()
        a.t, a.w_in, a.b_in, a.pe = t.data_ptr(), wv.data_ptr(), bv.data_ptr(), pe.data_ptr()
        a.B, a.D, a.E, a.S, a.temb_scale = B, D, E, S, float(temb_scale)
        a.out, a.temb, a.enumerate, a.cond, a.rows, a.r0 = out.data_ptr(), temb.data_ptr(), 1, cond, n, r0_dev.data_ptr()
        _ck(lib().ctdd_bert_embed(C.byref(a), _st()), "ctdd_bert_embed")
        ctx.save_for_backward(x)
        ctx.meta = (S, cond, r0, n, w_in.shape)
        return out

    @staticmethod
    def backward(ctx, dout):
        (x,) = ctx.saved_tensors
        S, cond, r0, n, wshape = ctx.meta
        B, D = x.shape
        E = dout.shape[-1]
        dout = dout.contiguous()
        dwb = torch.zeros((2, E), dtype=torch.float32, device=x.device)
        a = _BertEmbedEnumBwdArgs()
        set_state_ptr(a, x, "MaskedTrainer")
        a.g, a.B, a.D, a.E, a.S, a.cond, a.rows, a.r0 = dout.data_ptr(), B, D, E, S, cond, n, r0
        a.dw, a.db = dwb[0].data_ptr(), dwb[1].data_ptr()
        _ck(lib().ctdd_bert_embed_enum_bwd(C.byref(a), _st()), "ctdd_bert_embed_enum_bwd")
        return None, None, dwb[0].view(wshape), dwb[1], None, None, None, None


class EnumGatherFn(torch.autograd.Function):
    """Row 1 + p of every sequence (b, p) of the chunk's encoder output (n, D + 1, E) -> rows [r0, r0 + n) of the readout input
    `rows` (B D', E), in place: the chunks write disjoint windows of one buffer, whose gradient passes through unchanged (a
    chunk's backward reads its own window only)."""

    @staticmethod
    def forward(ctx, rows, enc, r0_dev, meta):
        B, D, cond, r0, n = meta
        E = enc.shape[-1]
        enc = enc.contiguous()
        _ck(lib().ctdd_bert_gather(enc.data_ptr(), r0_dev.data_ptr(), n, 1, B, D, cond, E, rows.data_ptr(), None, None, _st()), "ctdd_bert_gather")
        ctx.meta = meta + (E,)
        ctx.mark_dirty(rows)
        return rows

    @staticmethod
    def backward(ctx, drows):
        B, D, cond, r0, n, E = ctx.meta
        drows = drows.contiguous()
        denc = torch.empty((n, D + 1, E), dtype=torch.float32, device=drows.device)
        _ck(lib().ctdd_bert_gather_enum_bwd(drows.data_ptr(), r0, n, B, D, cond, E, denc.data_ptr(), _st()), "ctdd_bert_gather_enum_bwd")
        return (drows if ctx.needs_input_grad[0] else None), denc, None, None


def training_supported(model):
    """The masked net with the FiLM residual readout, inside the inference engine's coverage and the training kernels' shape limits
    (those of hollow_train.training_supported)."""
    net = unwrap(getattr(model, "net", None))
    if net is None or net.__class__.__name__ != "EnumerativeTransformer":
        return False
    m = net.config.model
    if m.readout != "resnet" or not bert_engine.supports(model):
        return False
    return (m.embed_dim // m.num_heads) in (4, 8, 16, 32) and m.embed_dim <= 256 and m.embed_dim % 16 == 0 and m.mlp_dim % 16 == 0


class MaskedTrainer(Trainer):
    def __init__(self, model, precision=None):
        if not training_supported(model):
            raise native.CtddError("MaskedTrainer: network outside the training kernels' coverage (see masked_train.training_supported)")
        super().__init__(model, precision)
        lib()
        self._walk, self.chunk_rngs = None, None

    def __call__(self, x, times):
        from lib.networks.hollow_networks import enum_chunk_size
        net, tf = self.net, self.net.transformer
        m = net.config.model
        E, S = m.embed_dim, net.S
        shape = tuple(x.shape)
        x = x.view(x.shape[0], -1).contiguous()
        B, D = x.shape
        T = D + 1
        c = int(getattr(m, "conditional_dim", 0) or 0)
        Dp = D - c
        total = B * Dp
        walk = chunk_walk(total, enum_chunk_size(net.config, total))
        if self._walk is None or self._walk[0] != walk:
            self._walk = (walk, torch.tensor([r0 for r0, _ in walk], dtype=torch.int32, device=self.dev))
        r0s = self._walk[1]
        fw = Forward(self, clone=False)
        if fw.training:
            # one {seed, step} per chunk, cloned: this forward's masks stay put whatever runs before its backward, and the
            # trainer's own step moves past the chunks' so the next forward shares none of them
            rngs = self.rng.repeat(len(walk), 1)
            rngs[:, 1] += torch.arange(len(walk), dtype=torch.int64, device=self.dev)
            self.rng[1] += len(walk) - 1
            self.chunk_rngs = rngs                            # (the last training forward's table: the tests read it)
        short = short_attention_applies(T, T, fw.hd, 3)
        enc = tf.trans_encoder
        pe = self.pos_table(enc.pos_embed, T)
        tv = times.float().contiguous()
        temb = torch.empty((B, E), dtype=torch.float32, device=self.dev)       # complete after the last chunk (module docstring)
        rows = torch.empty((total, E), dtype=torch.float32, device=self.dev)
        w_emb, b_emb = tf.input_embedding.weight, tf.input_embedding.bias
        for i, (r0, n) in enumerate(walk):
            fw.restart(rngs[i] if fw.training else self.rng)
            h = EnumEmbedFn.apply(x, tv, w_emb, b_emb, pe, temb, r0s[i:i + 1], (S, float(net.temb_scale), c, r0, n))
            h = fw.encoder(h, enc.trans_block_layers, n, T, 3, short=short)
            rows = EnumGatherFn.apply(rows, h, r0s[i:i + 1], (B, D, c, r0, n))
        logits = film_readout(tf.model, rows, temb, B, Dp, fw.bf, fw.pk)
        if c:                                                 # the never-masked prefix: all-zero logits, no gradient
            logits = torch.cat([torch.zeros((B, c, logits.shape[-1]), dtype=logits.dtype, device=self.dev), logits], dim=1)
        return logits.view(shape + (S,))
