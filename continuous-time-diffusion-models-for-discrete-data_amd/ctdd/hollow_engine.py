"""Hand-written HIP inference engine for the SDDM hollow transformer (lib/networks/hollow_networks.py;
reference TAUnSDDM/lib/networks/hollow_networks.py:668-755 + lib/models/models.py:495-525).

Walks a built `BidirectionalTransformer2` once, keeps pointers to its fp32 parameters (torch Linear layout
[out][in] is the [N][K] layout the GEMM kernel streams), allocates every intermediate for a batch size and
records the forward as a flat list of pre-bound libctdd launches, replayed as one HIP graph.  The engine wrapper (PlanEngine),
the prenorm encoder block and the FiLM residual readout are those of ctdd/plan_common.py, shared with ctdd/bert_engine.py; this
module adds the hollow embedding, the two causal stacks and the attention readout between them:

  embed (csrc/hollow_kernels.hip) -> per direction and layer (PlanBuilder.encoder_blocks, modes 0 and 1): LayerNorm -> QKV GEMM ->
  masked attention -> out-proj GEMM (+residual) -> LayerNorm -> fc1 GEMM (ReLU) -> fc2 GEMM (+residual) -> readout: two LayerNorms
  into the key buffer, l2r+r2l, Q / K / V GEMMs, readout attention, out GEMM (+residual) -> PlanBuilder.film_readout: FiLM
  residual MLPs (GELU GEMMs, LayerNorm+FiLM), logits GEMM.

precision = "fp32":  all arithmetic fp32, GEMMs on the exact-fp32 matrix instruction v_mfma_f32_32x32x2_f32 --
                     the network's bar is 1e-4 on the logits against the reference's golden outputs.
precision = "bf16":  the token-level GEMMs take bf16 operands (weights and the LayerNorm / attention / MLP outputs
                     that feed them) on v_mfma_f32_32x32x16_bf16 with fp32 accumulation; the residual streams,
                     LayerNorm, softmax and the per-sample FiLM path stay fp32.  Throughput mode, looser bar.
precision = "bf16x3" (default): hi + lo bf16 operand pairs, see PlanEngine.
"""
import ctypes as C
import types

import torch

from .plan_common import PlanBuilder, PlanEngine, _AttnArgs, _EmbedArgs, _GemmArgs, _lib  # noqa: F401  (tests and tools import the argument blocks from here)
from .plan_launch import set_state_ptr, unwrap


def supports(model):
    net = unwrap(getattr(model, "net", None))
    if net is None or net.__class__.__name__ != "BidirectionalTransformer2":
        return False
    m = net.config.model
    E, H = m.embed_dim, m.num_heads
    return (not net.use_cat and m.transformer_norm_type == "prenorm" and m.qkv_dim == E and E % H == 0 and (E // H) in (4, 8, 16, 32, 64)
            and E % 16 == 0 and m.mlp_dim % 16 == 0)


class HollowEngine(PlanEngine):
    def _build(self, B, x_dtype):
        net, lib, dev = self.net, _lib(), self.dev
        m = net.config.model
        E, S = m.embed_dim, net.S
        D = int(m.concat_dim)
        st = types.SimpleNamespace()
        pb = PlanBuilder(self, B)
        keep, fast, split = pb.keep, self.fast, self.split
        f32, hi, lo, P, W, launch, linear, layernorm = pb.f32, pb.hi, pb.lo, pb.P, pb.W, pb.launch, pb.linear, pb.layernorm
        st.x_in = torch.zeros((B, D), dtype=x_dtype, device=dev)
        st.t_in = torch.zeros((B,), dtype=torch.float32, device=dev)

        R = B * D
        # ---- embedding
        st.l2r, st.r2l, st.temb = f32(B, D, E), f32(B, D, E), f32(B, E)
        pe = net.module_l2r.pos_embed.pe[0, :D].to(dev).float().contiguous()
        keep.append(pe)
        ea = _EmbedArgs()
        set_state_ptr(ea, st.x_in, "HollowEngine")
        ea.t, ea.w_in, ea.b_in, ea.pe = P(st.t_in), P(W(net.input_embedding.weight.reshape(-1))), P(W(net.input_embedding.bias)), P(pe)
        ea.B, ea.D, ea.E, ea.S, ea.temb_scale = B, D, E, S, float(net.temb_scale)
        ea.l2r, ea.r2l, ea.temb = P(st.l2r), P(st.r2l), P(st.temb)
        keep.append(ea)
        launch(lib.ctdd_hollow_embed, C.byref(ea))

        # ---- the two causal stacks
        bufs = pb.encoder_buffers(R)
        for x, stack, mode in ((st.l2r, net.module_l2r, 0), (st.r2l, net.module_r2l, 1)):
            pb.encoder_blocks(x, stack.trans_block_layers, B, D, mode, bufs)

        # ---- attention readout
        ro = net.readout_module
        ca = ro.cross_attention
        Tk = 2 * D + 1
        ctx, ctx_hi, ctx_lo = bufs.ctx, bufs.ctx_hi, bufs.ctx_lo
        allk, allk_hi, allk_lo = f32(B, Tk, E), hi(B, Tk, E), lo(B, Tk, E)
        keep.extend([allk, allk_hi, allk_lo])
        launch(lib.ctdd_hollow_put_rows, P(st.temb), P(allk), P(allk_hi), P(allk_lo), Tk * E, B, E)
        layernorm(st.l2r, D * E, D, E, ro.ln1, allk[:, 1:], Tk * E, out_hi=None if not fast else allk_hi[:, 1:], out_hi_bs=Tk * E,
                  out_lo=None if not split else allk_lo[:, 1:])
        layernorm(st.r2l, D * E, D, E, ro.ln2, allk[:, D + 1:], Tk * E, out_hi=None if not fast else allk_hi[:, D + 1:], out_hi_bs=Tk * E,
                  out_lo=None if not split else allk_lo[:, D + 1:])
        qin, qin_hi, qin_lo, raw = (None if fast else f32(R, E)), hi(R, E), lo(R, E), f32(R, E)
        launch(lib.ctdd_hollow_add, P(allk) + 4 * E, Tk * E, P(allk) + 4 * (D + 1) * E, Tk * E, P(qin), P(qin_hi), P(qin_lo), D * E, B, D * E)
        launch(lib.ctdd_hollow_add, P(st.l2r), D * E, P(st.r2l), D * E, P(raw), None, None, D * E, B, D * E)
        qb, kb, vb = f32(R, E), f32(B * Tk, E), f32(B * Tk, E)
        keep.extend([qin, qin_hi, qin_lo, raw, qb, kb, vb])
        linear(qin, R, E, ca.dense_query.weight, None, qb, label="readout q", x_hi=qin_hi, x_lo=qin_lo)
        linear(allk, B * Tk, E, ca.dense_key.weight, ca.dense_key.bias, kb, label="readout k", x_hi=allk_hi, x_lo=allk_lo)
        linear(allk, B * Tk, E, ca.dense_val.weight, ca.dense_val.bias, vb, label="readout v", x_hi=allk_hi, x_lo=allk_lo)
        pb.attention(P(qb), D * E, E, P(kb), Tk * E, E, P(vb), Tk * E, E, D, Tk, 2, ctx, out_hi=ctx_hi, out_lo=ctx_lo)
        xr, xr_hi, xr_lo = (None if fast else f32(R, E)), hi(R, E), lo(R, E)
        keep.extend([xr, xr_hi, xr_lo])
        linear(ctx, R, E, ca.out_linear.weight, ca.out_linear.bias, xr, res=raw, label="readout out", x_hi=ctx_hi, x_lo=ctx_lo, out_hi=xr_hi,
               out_lo=xr_lo)

        st.logits = pb.film_readout(ro.model, xr, xr_hi, xr_lo, st.temb, B, D)
        st.plan, st.keep, st.graph = pb.plan, keep, None
        return st
