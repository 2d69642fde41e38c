"""Hand-written HIP inference engine for the two single-stream transformer score models (lib/networks/hollow_networks.py:
BertEnumTransformer -- x0 prediction, "BERT" -- and EnumerativeTransformer -- the masked model; reference
TAUnSDDM/lib/networks/hollow_networks.py:450-493, 859-1031 + lib/models/models.py:617-658).

A PlanEngine like HollowEngine (ctdd/hollow_engine.py), its encoder blocks and readout emitted by the same PlanBuilder methods
(ctdd/plan_common.py): one plan per (batch, state dtype), replayed as HIP graphs, precisions "fp32" / "bf16x3" (default) /
"bf16", plans dropped when the weights move.  Here the plan is two launch lists, each with its graph:

  chunk plan:  ctdd_bert_embed -> PlanBuilder.encoder_blocks (per layer: LayerNorm -> QKV GEMM -> unmasked attention, mode 3, over
               T = D + 1 tokens -> out-proj GEMM (+residual) -> LayerNorm -> fc1 GEMM (ReLU) -> fc2 GEMM (+residual)) -> ctdd_bert_gather
  tail plan:   PlanBuilder.film_readout (FiLM residual MLPs, LayerNorm + FiLM, the logits GEMM) over the gathered rows

BERT runs one encoder pass over the B sequences and gathers rows 1..D of each.  The masked model runs the encoder over the
(B D') enumeration "sample b with token p masked", D' = D - conditional_dim, in chunks of enum_chunk_size() sequences: every
chunk replays ONE captured graph, which reads its first sequence number from device memory, and gathers row p of each of its
sequences (b, p) into the (B D', E) readout input.  The readout then runs once over all rows -- its FiLM parameters are per
sample, and chunk borders do not fall on sample borders -- and the logits land behind the all-zero conditional prefix.
"""
import ctypes as C
import types

import torch

from . import native
from .plan_common import PlanBuilder, PlanEngine, _lib as _hollow_lib, _P, _I, _F
from .plan_launch import graph_capture, set_state_ptr, unwrap

_NETS = ("BertEnumTransformer", "EnumerativeTransformer")


class _BertEmbedArgs(C.Structure):
    _fields_ = [("x64", _P), ("x32", _P), ("t", _P), ("w_in", _P), ("b_in", _P), ("pe", _P), ("B", _I), ("D", _I), ("E", _I),
                ("S", _I), ("temb_scale", _F), ("out", _P), ("temb", _P), ("enumerate", _I), ("cond", _I), ("rows", _I), ("r0", _P)]


_sigs_done = False


def _lib():
    global _sigs_done
    lib = _hollow_lib()
    if not _sigs_done:
        for name, argt in (("ctdd_bert_embed", [_P, _P]), ("ctdd_bert_attention_short", [_P, _P]),
                           ("ctdd_bert_gather", [_P, _P, _I, _I, _I, _I, _I, _I, _P, _P, _P, _P])):
            fn = getattr(lib, name)
            fn.argtypes, fn.restype = argt, _I
        _sigs_done = True
    return lib


def supports(model):
    net = unwrap(getattr(model, "net", None))
    if net is None or net.__class__.__name__ not in _NETS:
        return False
    m = net.config.model
    E, H = m.embed_dim, m.num_heads
    return (not m.use_cat and m.transformer_norm_type == "prenorm" and m.readout == "resnet" and E % H == 0
            and (E // H) in (4, 8, 16, 32, 64) and E % 16 == 0 and m.mlp_dim % 16 == 0)


class BertEngine(PlanEngine):
    def __init__(self, model, precision=None):
        if not supports(model):
            raise native.CtddError("BertEngine: network outside the kernels' coverage (see bert_engine.supports)")
        super().__init__(model, precision)
        self.masked = self.net.__class__.__name__ == "EnumerativeTransformer"
        self.inner = self.net.transformer if self.masked else self.net          # holds trans_encoder, model, input_embedding

    # ------------------------------------------------------------------ plan
    def _build(self, B, x_dtype):
        from lib.networks.hollow_networks import enum_chunk_size
        net, inner, lib, dev = self.net, self.inner, _lib(), self.dev
        m = net.config.model
        E, S = m.embed_dim, net.S
        D = int(m.concat_dim)
        T = D + 1
        c = int(getattr(m, "conditional_dim", 0) or 0) if self.masked else 0
        Dp = D - c
        total = B * Dp                                                # readout rows
        seqs = enum_chunk_size(net.config, total) if self.masked else B      # sequences per encoder pass
        st = types.SimpleNamespace()
        st.nchunks = -(-total // seqs) if self.masked else 1
        pb = PlanBuilder(self, B)
        keep, fast = pb.keep, self.fast
        f32, hi, lo, P, W, launch = pb.f32, pb.hi, pb.lo, pb.P, pb.W, pb.launch
        st.x_in = torch.zeros((B, D), dtype=x_dtype, device=dev)
        st.t_in = torch.zeros((B,), dtype=torch.float32, device=dev)
        st.r0 = torch.zeros((1,), dtype=torch.int32, device=dev)                       # first sequence of the chunk being run
        st.r0s = torch.arange(0, st.nchunks * seqs, seqs, dtype=torch.int32, device=dev)

        # ---- embedding
        xs, st.temb = f32(seqs, T, E), f32(B, E)
        pe = inner.trans_encoder.pos_embed.pe[0, :T].to(dev).float().contiguous()
        ea = _BertEmbedArgs()
        set_state_ptr(ea, st.x_in, "BertEngine")
        ea.t, ea.w_in, ea.b_in, ea.pe = P(st.t_in), P(W(inner.input_embedding.weight.reshape(-1))), P(W(inner.input_embedding.bias)), P(pe)
        ea.B, ea.D, ea.E, ea.S, ea.temb_scale = B, D, E, S, float(net.temb_scale)
        ea.out, ea.temb, ea.enumerate, ea.cond, ea.rows, ea.r0 = P(xs), P(st.temb), int(self.masked), c, seqs, P(st.r0)
        keep.extend([xs, pe, ea])
        launch(lib.ctdd_bert_embed, C.byref(ea), label=f"embed {seqs}x{T}")

        # ---- encoder
        # model.engine_attention_short (default on): T <= 64 runs one wave per (sequence, head) with K / V resident in LDS
        short = bool(getattr(m, "engine_attention_short", True)) and T <= 64 and pb.hd <= 32
        pb.encoder_blocks(xs, inner.trans_encoder.trans_block_layers, seqs, T, 3, pb.encoder_buffers(seqs * T),
                          attention_fn=lib.ctdd_bert_attention_short if short else None)

        # ---- readout input: BERT rows 1..D of every sequence; masked row 1 + p of sequence (b, p)
        xr, xr_hi, xr_lo = (None if fast else f32(total, E)), hi(total, E), lo(total, E)
        keep.extend([xr, xr_hi, xr_lo])
        launch(lib.ctdd_bert_gather, P(xs), P(st.r0) if self.masked else None, seqs if self.masked else total, int(self.masked), B, D, c, E,
               P(xr), P(xr_hi), P(xr_lo), label=f"gather {seqs if self.masked else total} rows")
        st.chunk_plan, pb.plan = pb.plan, []             # what follows is recorded as the readout plan

        # ---- FiLM residual readout over the (B, D', E) rows
        out_dim = inner.model.out_dim
        st.logits = logits = pb.film_readout(inner.model, xr, xr_hi, xr_lo, st.temb, B, Dp)
        if c:
            # the conditional prefix keeps the zeros it is allocated with; the D' computed columns go behind it (logits + 0, strided)
            n = Dp * out_dim
            st.logits = torch.zeros((B, D, out_dim), dtype=torch.float32, device=dev)
            zeros = torch.zeros((n,), dtype=torch.float32, device=dev)
            keep.extend([logits, zeros])
            launch(lib.ctdd_hollow_add, P(logits), n, P(zeros), 0, P(st.logits) + 4 * c * out_dim, None, None, D * out_dim, B, n,
                   label="logits behind the prefix")
        st.tail_plan, st.keep = pb.plan, keep
        st.chunk_graph = st.tail_graph = None
        return st

    # ------------------------------------------------------------------ execution
    @staticmethod
    def _run(st):
        """One forward: every chunk with its first sequence number in st.r0, then the readout (as graphs once captured)."""
        for k in range(st.nchunks):
            if st.nchunks > 1:
                st.r0.copy_(st.r0s[k:k + 1])
            if st.chunk_graph is not None:
                st.chunk_graph.replay()
            else:
                for step in st.chunk_plan:
                    step()
        if st.tail_graph is not None:
            st.tail_graph.replay()
        else:
            for step in st.tail_plan:
                step()

    @staticmethod
    def _capture(st):
        graphs = []
        for plan in (st.chunk_plan, st.tail_plan):            # (the chunk graph reads r0 on the device at replay)
            g = torch.cuda.CUDAGraph()
            with graph_capture(g):
                for step in plan:
                    step()
            graphs.append(g)
        st.chunk_graph, st.tail_graph = graphs
