"""Training path of the x0-prediction ("BERT") transformer on hand-written HIP kernels (reference: forward + `l.backward()`
through TAUnSDDM/lib/networks/hollow_networks.py:450-493 (TransformerEncoder), 963-1031 (BertEnumTransformer) and 90-132 (FiLM
residual readout)).

`BertTrainer(model)(x, t)` computes the logits of a `BertEnumTransformer` the way `HollowTrainer` (ctdd/hollow_train.py) computes
the hollow transformer's: every operation a libctdd launch, autograd as the tape only, one Function per block.

  embedding     `ctdd_bert_embed` in plain mode ([temb | x_0..x_{D-1}] + pe, T = D + 1 tokens) / `ctdd_bert_embed_bwd`
  encoder       hollow_train.Forward.encoder: per layer `AttnBlockFn` and `MlpBlockFn` with Tq = Tk = T, packed qkv rows and
                attention mode 3 (unmasked: `ctdd_hollow_attention_train(_bf16)` / `_bwd(_bf16)`)
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
from .hollow_train import Forward, Trainer, _ck, _st, film_readout, lib as _train_lib
from .plan_launch import set_state_ptr, unwrap

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
    set_state_ptr(a, x, "BertTrainer")


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
    net = unwrap(getattr(model, "net", None))
    if net is None or net.__class__.__name__ != "BertEnumTransformer" or not bert_engine.supports(model):
        return False
    m = net.config.model
    return (m.embed_dim // m.num_heads) in (4, 8, 16, 32) and m.embed_dim <= 256 and m.embed_dim % 16 == 0 and m.mlp_dim % 16 == 0


class BertTrainer(Trainer):
    def __init__(self, model, precision=None):
        if not training_supported(model):
            raise native.CtddError("BertTrainer: network outside the training kernels' coverage (see bert_train.training_supported)")
        super().__init__(model, precision)
        lib()

    def __call__(self, x, times):
        net = self.net
        x = x.view(x.shape[0], -1)
        B, D = x.shape
        T = D + 1
        fw = Forward(self)
        enc = net.trans_encoder
        pe = self.pos_table(enc.pos_embed, T)
        h, temb = BertEmbedFn.apply(x, times, net.input_embedding.weight, net.input_embedding.bias, pe, net.S, float(net.temb_scale))
        h = fw.encoder(h, enc.trans_block_layers, B, T, 3)    # (the generic attention kernels: short is MaskedTrainer's)
        return film_readout(net.model, BertGatherFn.apply(h), temb, B, D, fw.bf, fw.pk)
