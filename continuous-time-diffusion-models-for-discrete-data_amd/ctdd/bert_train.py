"""Training path of the x0-prediction ("BERT") transformer on hand-written HIP kernels (reference: forward + `l.backward()`
through TAUnSDDM/lib/networks/hollow_networks.py:450-493 (TransformerEncoder), 963-1031 (BertEnumTransformer) and 90-132 (FiLM
residual readout)).

`BertTrainer(model)(x, t)` computes the logits of a `BertEnumTransformer` the way `HollowTrainer` (ctdd/hollow_train.py) computes
the hollow transformer's: every operation a libctdd launch, autograd as the tape only, one Function per block.

  embedding     `ctdd_bert_embed` in plain mode ([temb | x_0..x_{D-1}] + pe, T = D + 1 tokens) / `ctdd_bert_embed_bwd`
  encoder       per layer `AttnBlockFn` and `MlpBlockFn` of hollow_train with Tq = Tk = T, packed qkv rows and attention mode 3
                (unmasked: `ctdd_hollow_attention_train(_bf16)` / `_bwd(_bf16)`)
  readout       `ctdd_bert_gather` (rows 1..D of every sequence) / `ctdd_bert_gather_bwd`, then hollow_train.film_readout

Precisions as there: "fp32" (parity mode) and "bf16" (default; head dimensions 16 and 32 run the matrix-core attention, 4 and 8
the fp32 kernels).  Dropout masks are Philox(seed, step, layer, element); every training forward carries its own {seed, step}.
The masked (enumerative) model trains on ctdd/masked_train.py (cfg.model.engine_train = "hip-masked"): `training_supported` here
is false for it.
"""
import ctypes as C

import torch

from . import bert_engine, native
from .bert_engine import _BertEmbedArgs
from .hollow_train import AttnBlockFn, DropoutFn, MlpBlockFn, WeightPacks, _ck, _st, film_readout, lib as _train_lib
from .unet_engine import _unwrap

_P, _I = C.c_void_p, C.c_int


class _BertEmbedBwdArgs(C.Structure):
    _fields_ = [("x64", _P), ("x32", _P), ("g", _P), ("B", _I), ("D", _I), ("E", _I), ("S", _I), ("dw", _P), ("db", _P)]


_sigs_done = False


def lib():
    global _sigs_done
    _train_lib()
    l = bert_engine._lib()
    if not _sigs_done:
        for name, argt in (("ctdd_bert_embed_bwd", [_P, _P]), ("ctdd_bert_gather_bwd", [_P, _I, _I, _I, _I, _P, _P])):
            fn = getattr(l, name)
            fn.argtypes, fn.restype = argt, _I
        _sigs_done = True
    return l


def _state_ptrs(a, x):
    if x.dtype == torch.int64:
        a.x64 = x.data_ptr()
    elif x.dtype == torch.int32:
        a.x32 = x.data_ptr()
    else:
        raise native.CtddError(f"BertTrainer expects integer states, got {x.dtype}")


class BertEmbedFn(torch.autograd.Function):
    """(B, D) integer states, (B,) times -> the encoder input (B, D + 1, E) and the time embedding temb (B, E)."""

    @staticmethod
    def forward(ctx, x, t, w_in, b_in, pe, S, temb_scale):
        B, D = x.shape
        E = w_in.numel()
        dev = x.device
        out = torch.empty((B, D + 1, E), dtype=torch.float32, device=dev)
        temb = torch.empty((B, E), dtype=torch.float32, device=dev)
        x = x.contiguous()
        a = _BertEmbedArgs()
        _state_ptrs(a, x)
        wv, bv, tv = w_in.detach().reshape(-1).contiguous(), b_in.detach().contiguous(), t.float().contiguous()
        a.t, a.w_in, a.b_in, a.pe = tv.data_ptr(), wv.data_ptr(), bv.data_ptr(), pe.data_ptr()
        a.B, a.D, a.E, a.S, a.temb_scale = B, D, E, S, float(temb_scale)
        a.out, a.temb, a.enumerate, a.cond, a.rows, a.r0 = out.data_ptr(), temb.data_ptr(), 0, 0, B, None
        _ck(lib().ctdd_bert_embed(C.byref(a), _st()), "ctdd_bert_embed")
        ctx.save_for_backward(x)
        ctx.meta = (S, w_in.shape)
        ctx.mark_non_differentiable(temb)
        return out, temb

    @staticmethod
    def backward(ctx, dout, _dtemb):
        (x,) = ctx.saved_tensors
        S, wshape = ctx.meta
        B, D = x.shape
        E = dout.shape[-1]
        dout = dout.contiguous()
        dwb = torch.zeros((2, E), dtype=torch.float32, device=x.device)
        a = _BertEmbedBwdArgs()
        _state_ptrs(a, x)
        a.g, a.B, a.D, a.E, a.S, a.dw, a.db = dout.data_ptr(), B, D, E, S, dwb[0].data_ptr(), dwb[1].data_ptr()
        _ck(lib().ctdd_bert_embed_bwd(C.byref(a), _st()), "ctdd_bert_embed_bwd")
        return None, None, dwb[0].view(wshape), dwb[1], None, None, None


class BertGatherFn(torch.autograd.Function):
    """Encoder output (B, D + 1, E) -> the readout input (B D, E): rows 1..D of every sequence."""

    @staticmethod
    def forward(ctx, enc):
        B, T, E = enc.shape
        enc = enc.contiguous()
        out = torch.empty((B * (T - 1), E), dtype=torch.float32, device=enc.device)
        _ck(lib().ctdd_bert_gather(enc.data_ptr(), None, B * (T - 1), 0, B, T - 1, 0, E, out.data_ptr(), None, None, _st()), "ctdd_bert_gather")
        ctx.shape = (B, T, E)
        return out

    @staticmethod
    def backward(ctx, dout):
        B, T, E = ctx.shape
        dout = dout.contiguous()
        denc = torch.empty((B, T, E), dtype=torch.float32, device=dout.device)
        _ck(lib().ctdd_bert_gather_bwd(dout.data_ptr(), B, T - 1, 0, E, denc.data_ptr(), _st()), "ctdd_bert_gather_bwd")
        return denc


def training_supported(model):
    """The x0-prediction net inside the inference engine's coverage and the training kernels' shape limits (those of
    hollow_train.training_supported)."""
    net = _unwrap(getattr(model, "net", None))
    if net is None or net.__class__.__name__ != "BertEnumTransformer" or not bert_engine.supports(model):
        return False
    m = net.config.model
    return (m.embed_dim // m.num_heads) in (4, 8, 16, 32) and m.embed_dim <= 256 and m.embed_dim % 16 == 0 and m.mlp_dim % 16 == 0


class BertTrainer:
    def __init__(self, model, precision=None):
        self.model, self.net = model, _unwrap(model.net)
        if not training_supported(model):
            raise native.CtddError("BertTrainer: network outside the training kernels' coverage (see bert_train.training_supported)")
        m = self.net.config.model
        self.precision = precision or getattr(m, "engine_train_precision", "bf16")
        if self.precision not in ("fp32", "bf16"):
            raise ValueError(f"unknown training precision {self.precision}")
        self.dev = next(self.net.parameters()).device
        if self.dev.type != "cuda":
            raise native.CtddError("BertTrainer needs the model on a GPU")
        lib()
        self.rng = torch.zeros(2, dtype=torch.int64, device=self.dev)
        self.rng[0] = native.dropout_seed()
        self.pe = None
        self.pk = WeightPacks(self.net, self.precision == "bf16", self.dev)

    def __call__(self, x, times):
        net = self.net
        m = net.config.model
        bf = self.precision == "bf16"
        E, H, S = m.embed_dim, m.num_heads, net.S
        hd = E // H
        x = x.view(x.shape[0], -1)
        B, D = x.shape
        T = D + 1
        training = bool(self.model.training)
        p_drop = float(m.dropout_rate) if training else 0.0
        p_att = float(m.attention_dropout_rate) if training else 0.0
        self.pk.refresh(self.rng if training else None)       # (+ one dropout stream per training forward)
        # every forward keeps its OWN {seed, step} (see HollowTrainer.__call__): two forwards before one backward keep their masks
        rng, pk = (self.rng.clone() if training else self.rng), self.pk
        layer = [0]

        def nxt():
            layer[0] += 1
            return layer[0]

        def drop(t, p):
            return DropoutFn.apply(t, p, rng, nxt()) if p > 0.0 else t

        enc = net.trans_encoder
        if self.pe is None or self.pe.shape[0] != T:
            self.pe = enc.pos_embed.pe[0, :T].to(self.dev).float().contiguous()
        h, temb = BertEmbedFn.apply(x, times, net.input_embedding.weight, net.input_embedding.bias, self.pe, S, float(net.temb_scale))
        h = drop(drop(h, p_drop), p_drop)                     # PositionalEncoding's dropout, then the encoder's (TransformerEncoder.forward)
        for blk in enc.trans_block_layers:
            sa, ff = blk.self_attention_block, blk.feed_forward_block
            mha = sa.self_attention
            h = AttnBlockFn.apply(h, sa.norm.weight, sa.norm.bias, mha.in_proj_weight, mha.in_proj_bias, mha.out_proj.weight,
                                  mha.out_proj.bias, rng,
                                  (B, T, H, hd, 3, p_att, p_drop, nxt(), nxt(), bf, sa.norm.eps, pk(mha.in_proj_weight), pk(mha.out_proj.weight)))
            h = MlpBlockFn.apply(h, ff.norm.weight, ff.norm.bias, ff.mlp.fc1.weight, ff.mlp.fc1.bias, ff.mlp.fc2.weight, rng,
                                 (B, T, E, p_drop, nxt(), nxt(), bf, ff.norm.eps, pk(ff.mlp.fc1.weight), pk(ff.mlp.fc2.weight)))
        return film_readout(net.model, BertGatherFn.apply(h), temb, B, D, bf, pk)
