"""Hand-written HIP inference engine for the two single-stream transformer score models (lib/networks/hollow_networks.py:
BertEnumTransformer -- x0 prediction, "BERT" -- and EnumerativeTransformer -- the masked model; reference
TAUnSDDM/lib/networks/hollow_networks.py:450-493, 859-1031 + lib/models/models.py:617-658).

Built like HollowEngine (ctdd/hollow_engine.py) from the same launch builders (ctdd/plan_common.py): one plan per
(batch, state dtype), replayed as HIP graphs, precisions "fp32" / "bf16x3" (default) / "bf16", plans dropped when the weights move.

  encoder pass:  ctdd_bert_embed -> per layer: LayerNorm -> QKV GEMM -> unmasked attention (mode 3) over T = D + 1 tokens ->
                 out-proj GEMM (+residual) -> LayerNorm -> fc1 GEMM (ReLU) -> fc2 GEMM (+residual) -> ctdd_bert_gather
  readout:       FiLM residual MLPs (GELU GEMMs, LayerNorm + FiLM) and the logits GEMM over the gathered rows

BERT runs one encoder pass over the B sequences and gathers rows 1..D of each.  The masked model runs the encoder over the
(B D') enumeration "sample b with token p masked", D' = D - conditional_dim, in chunks of enum_chunk_size() sequences: every
chunk replays ONE captured graph, which reads its first sequence number from device memory, and gathers row p of each of its
sequences (b, p) into the (B D', E) readout input.  The readout then runs once over all rows -- its FiLM parameters are per
sample, and chunk borders do not fall on sample borders -- and the logits land behind the all-zero conditional prefix.
"""
import ctypes as C

import torch

from . import native
from .plan_common import PlanBuilder, _lib as _hollow_lib, _P, _I, _F
from .plan_launch import graph_capture
from .unet_engine import _unwrap

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
    net = _unwrap(getattr(model, "net", None))
    if net is None or net.__class__.__name__ not in _NETS:
        return False
    m = net.config.model
    E, H = m.embed_dim, m.num_heads
    return (not m.use_cat and m.transformer_norm_type == "prenorm" and m.readout == "resnet" and E % H == 0
            and (E // H) in (4, 8, 16, 32, 64) and E % 16 == 0 and m.mlp_dim % 16 == 0)


class BertEngine:
    def __init__(self, model, precision=None):
        self.model, self.net = model, _unwrap(model.net)
        if not supports(model):
            raise native.CtddError("BertEngine: network outside the kernels' coverage (see bert_engine.supports)")
        self.masked = self.net.__class__.__name__ == "EnumerativeTransformer"
        self.inner = self.net.transformer if self.masked else self.net          # holds trans_encoder, model, input_embedding
        self.precision = precision or getattr(self.net.config.model, "engine_precision", "bf16x3")
        if self.precision not in ("fp32", "bf16", "bf16x3"):
            raise ValueError(f"unknown engine precision {self.precision}")
        self.fast = self.precision in ("bf16", "bf16x3")                         # as in HollowEngine
        self.split = self.precision == "bf16x3"
        self.single = set(getattr(self.net.config.model, "engine_bf16_linears", ()) or ())
        self.dev = next(self.net.parameters()).device
        if self.dev.type != "cuda":
            raise native.CtddError("BertEngine needs the model on a GPU")
        self._plans, self._wver = {}, None

    def _weights_version(self):
        return sum(p._version for p in self.net.parameters()) + 7919 * getattr(self.model, "_weights_version", 0)

    # ------------------------------------------------------------------ plan
    def _build(self, B, x_dtype):
        from lib.networks.hollow_networks import enum_chunk_size
        net, inner, lib, dev = self.net, self.inner, _lib(), self.dev
        m = net.config.model
        E, S, mlp = m.embed_dim, net.S, m.mlp_dim
        D = int(m.concat_dim)
        T = D + 1
        c = int(getattr(m, "conditional_dim", 0) or 0) if self.masked else 0
        Dp = D - c
        total = B * Dp                                                # readout rows
        seqs = enum_chunk_size(net.config, total) if self.masked else B      # sequences per encoder pass
        st = type("Plan", (), {})()
        st.nchunks = -(-total // seqs) if self.masked else 1
        pb = PlanBuilder(self, B)
        keep, fast, split = pb.keep, self.fast, self.split
        f32, hi, lo, P, W, launch, linear, layernorm, attention = (pb.f32, pb.hi, pb.lo, pb.P, pb.W, pb.launch, pb.linear, pb.layernorm,
                                                                   pb.attention)
        st.x_in = torch.zeros((B, D), dtype=x_dtype, device=dev)
        st.t_in = torch.zeros((B,), dtype=torch.float32, device=dev)
        st.r0 = torch.zeros((1,), dtype=torch.int32, device=dev)                       # first sequence of the chunk being run
        st.r0s = torch.arange(0, st.nchunks * seqs, seqs, dtype=torch.int32, device=dev)

        # ---- embedding
        xs, st.temb = f32(seqs, T, E), f32(B, E)
        pe = inner.trans_encoder.pos_embed.pe[0, :T].to(dev).float().contiguous()
        ea = _BertEmbedArgs()
        if x_dtype == torch.int64:
            ea.x64 = P(st.x_in)
        else:
            ea.x32 = P(st.x_in)
        ea.t, ea.w_in, ea.b_in, ea.pe = P(st.t_in), P(W(inner.input_embedding.weight.reshape(-1))), P(W(inner.input_embedding.bias)), P(pe)
        ea.B, ea.D, ea.E, ea.S, ea.temb_scale = B, D, E, S, float(net.temb_scale)
        ea.out, ea.temb, ea.enumerate, ea.cond, ea.rows, ea.r0 = P(xs), P(st.temb), int(self.masked), c, seqs, P(st.r0)
        keep.extend([xs, pe, ea])
        launch(lib.ctdd_bert_embed, C.byref(ea), label=f"embed {seqs}x{T}")

        # ---- encoder
        R = seqs * T
        # model.engine_attention_short (default on): T <= 64 runs one wave per (sequence, head) with K / V resident in LDS
        short = bool(getattr(m, "engine_attention_short", True)) and T <= 64 and pb.hd <= 32
        ln_buf, qkv, ctx, hid = (None if fast else f32(R, E)), f32(R, 3 * E), (None if fast else f32(R, E)), (None if fast else f32(R, mlp))
        ln_hi, ctx_hi, hid_hi = hi(R, E), hi(R, E), hi(R, mlp)
        ln_lo, ctx_lo, hid_lo = lo(R, E), lo(R, E), lo(R, mlp)
        keep.extend([ln_buf, qkv, ctx, hid, ln_hi, ctx_hi, hid_hi, ln_lo, ctx_lo, hid_lo])
        for blk in inner.trans_encoder.trans_block_layers:
            sa, ff = blk.self_attention_block, blk.feed_forward_block
            mha = sa.self_attention
            layernorm(xs, T * E, T, E, sa.norm, ln_buf, T * E, out_hi=ln_hi, out_hi_bs=T * E, out_lo=ln_lo, B=seqs)
            linear(ln_buf, R, E, mha.in_proj_weight, mha.in_proj_bias, qkv, label="qkv", x_hi=ln_hi, x_lo=ln_lo)
            attention(P(qkv), T * 3 * E, 3 * E, P(qkv) + 4 * E, T * 3 * E, 3 * E, P(qkv) + 8 * E, T * 3 * E, 3 * E, T, T, 3, ctx,
                      out_hi=ctx_hi, out_lo=ctx_lo, B=seqs, fn=lib.ctdd_bert_attention_short if short else None)
            linear(ctx, R, E, mha.out_proj.weight, mha.out_proj.bias, xs, res=xs, label="attn out", x_hi=ctx_hi, x_lo=ctx_lo)
            layernorm(xs, T * E, T, E, ff.norm, ln_buf, T * E, out_hi=ln_hi, out_hi_bs=T * E, out_lo=ln_lo, B=seqs)
            linear(ln_buf, R, E, ff.mlp.fc1.weight, ff.mlp.fc1.bias, hid, act=1, label="fc1", x_hi=ln_hi, x_lo=ln_lo, out_hi=hid_hi,
                   out_lo=hid_lo)
            linear(hid, R, mlp, ff.mlp.fc2.weight, None, xs, res=xs, label="fc2", x_hi=hid_hi, x_lo=hid_lo)

        # ---- readout input: BERT rows 1..D of every sequence; masked row 1 + p of sequence (b, p)
        xr, xr_hi, xr_lo = (None if fast else f32(total, E)), hi(total, E), lo(total, E)
        keep.extend([xr, xr_hi, xr_lo])
        launch(lib.ctdd_bert_gather, P(xs), P(st.r0) if self.masked else None, seqs if self.masked else total, int(self.masked), B, D, c, E,
               P(xr), P(xr_hi), P(xr_lo), label=f"gather {seqs if self.masked else total} rows")
        st.chunk_plan, pb.plan = pb.plan, []             # what follows is recorded as the readout plan

        # ---- FiLM residual readout over the (B, D', E) rows
        rr = inner.model
        E2 = 2 * E
        tm_h, tm = f32(B, mlp), f32(B, 4 * E)
        lin = [l for l in rr.mlp.layers if isinstance(l, torch.nn.Linear)]
        linear(st.temb, B, E, lin[0].weight, lin[0].bias, tm_h, act=2, label="temb mlp 1")
        linear(tm_h, B, mlp, lin[1].weight, lin[1].bias, tm, label="temb mlp 2")
        h, r, rh = f32(total, E2), f32(total, E2), (None if fast else f32(total, mlp))
        h_hi, rh_hi, h_lo, rh_lo = hi(total, E2), hi(total, mlp), lo(total, E2), lo(total, mlp)
        keep.extend([tm_h, tm, h, r, rh, h_hi, rh_hi, h_lo, rh_lo])
        linear(xr, total, E, rr.input_layer.weight, rr.input_layer.bias, h, label="readout in", x_hi=xr_hi, x_lo=xr_lo, out_hi=h_hi, out_lo=h_lo)
        for i in range(rr.n_res):
            mlp_i, ln_i = rr.resid_layers[2 * i], rr.resid_layers[2 * i + 1]
            li = [l for l in mlp_i.layers if isinstance(l, torch.nn.Linear)]
            linear(h, total, E2, li[0].weight, li[0].bias, rh, act=2, label="resid 1", x_hi=h_hi, x_lo=h_lo, out_hi=rh_hi, out_lo=rh_lo)
            linear(rh, total, mlp, li[1].weight, li[1].bias, r, label="resid 2", x_hi=rh_hi, x_lo=rh_lo)
            fl = f32(B, 4 * E)
            keep.append(fl)
            linear(tm, B, 4 * E, rr.film_layer[i].weight, rr.film_layer[i].bias, fl, label="film")          # per-sample path: fp32
            layernorm(h, Dp * E2, Dp, E2, ln_i, h, Dp * E2, y=r, y_bs=Dp * E2, film=fl, film_stride=4 * E, out_hi=h_hi, out_hi_bs=Dp * E2,
                      out_lo=h_lo)
        logits = f32(B, Dp, rr.out_dim)
        linear(h, total, E2, rr.logits_layer.weight, rr.logits_layer.bias, logits, label="logits", x_hi=h_hi, x_lo=h_lo)
        st.logits = logits
        if c:
            # the conditional prefix keeps the zeros it is allocated with; the D' computed columns go behind it (logits + 0, strided)
            n = Dp * rr.out_dim
            st.logits = torch.zeros((B, D, rr.out_dim), dtype=torch.float32, device=dev)
            zeros = torch.zeros((n,), dtype=torch.float32, device=dev)
            keep.extend([logits, zeros])
            launch(lib.ctdd_hollow_add, P(logits), n, P(zeros), 0, P(st.logits) + 4 * c * rr.out_dim, None, None, D * rr.out_dim, B, n,
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

    def __call__(self, x, times):
        B = x.shape[0]
        key = (B, x.dtype)
        ver = self._weights_version()
        if ver != self._wver:
            self._plans.clear()
            self._wver = ver
        st = self._plans.get(key)
        if st is None:
            if x.dtype not in (torch.int64, torch.int32):
                raise native.CtddError(f"BertEngine expects integer states, got {x.dtype}")
            st = self._plans[key] = self._build(B, x.dtype)
            st.x_in.copy_(x.reshape(st.x_in.shape))
            st.t_in.copy_(times.float())
            self._run(st)
            torch.cuda.synchronize()
            if getattr(self.net.config.model, "engine_graph", True):
                self._capture(st)
        st.x_in.copy_(x.reshape(st.x_in.shape))
        st.t_in.copy_(times.float())
        self._run(st)
        return st.logits
