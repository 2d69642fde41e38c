"""Hand-written HIP inference engine for the SDDM hollow transformer (lib/networks/hollow_networks.py;
reference TAUnSDDM/lib/networks/hollow_networks.py:668-755 + lib/models/models.py:495-525).

Walks a built `BidirectionalTransformer2` once, keeps pointers to its fp32 parameters (torch Linear layout
[out][in] is the [N][K] layout the GEMM kernel streams), allocates every intermediate for a batch size and
records the forward as a flat list of pre-bound libctdd launches (the builders of ctdd/plan_common.py, shared with
ctdd/bert_engine.py), replayed as one HIP graph:

  embed (csrc/hollow_kernels.hip) -> per direction and layer: LayerNorm -> QKV GEMM -> masked attention ->
  out-proj GEMM (+residual) -> LayerNorm -> fc1 GEMM (ReLU) -> fc2 GEMM (+residual) -> readout: two LayerNorms
  into the key buffer, l2r+r2l, Q / K / V GEMMs, readout attention, out GEMM (+residual), FiLM residual MLPs
  (GELU GEMMs, LayerNorm+FiLM), logits GEMM.

precision = "fp32" (default): all arithmetic fp32, GEMMs on the exact-fp32 matrix instruction v_mfma_f32_32x32x2_f32 --
                     the network's bar is 1e-4 on the logits against the reference's golden outputs.
precision = "bf16":  the token-level GEMMs take bf16 operands (weights and the LayerNorm / attention / MLP outputs
                     that feed them) on v_mfma_f32_32x32x16_bf16 with fp32 accumulation; the residual streams,
                     LayerNorm, softmax and the per-sample FiLM path stay fp32.  Throughput mode, looser bar.
"""
import ctypes as C

import torch

from . import native
from .plan_common import PlanBuilder, _AttnArgs, _EmbedArgs, _GemmArgs, _LnArgs, _lib  # noqa: F401  (part of this module's interface)
from .plan_launch import graph_capture
from .unet_engine import _unwrap


def supports(model):
    net = _unwrap(getattr(model, "net", None))
    if net is None or net.__class__.__name__ != "BidirectionalTransformer2":
        return False
    m = net.config.model
    E, H = m.embed_dim, m.num_heads
    return (not net.use_cat and m.transformer_norm_type == "prenorm" and m.qkv_dim == E and E % H == 0 and (E // H) in (4, 8, 16, 32, 64)
            and E % 16 == 0 and m.mlp_dim % 16 == 0)


class HollowEngine:
    def __init__(self, model, precision=None):
        self.model, self.net = model, _unwrap(model.net)
        self.precision = precision or getattr(self.net.config.model, "engine_precision", "bf16x3")
        if self.precision not in ("fp32", "bf16", "bf16x3"):
            raise ValueError(f"unknown engine precision {self.precision}")
        # "fp32": exact-fp32 matrix instructions and fp32 FMA attention; "bf16": bf16 operands (~1e-3 absolute on the logits);
        # "bf16x3": every GEMM / attention operand as a hi + lo bf16 pair, three bf16 products per contraction with fp32
        # accumulation (x w ~ xh wh + xl wh + xh wl, dropped terms ~2^-17 relative): fp32-grade logits at bf16 matrix rates
        self.fast = self.precision in ("bf16", "bf16x3")
        self.split = self.precision == "bf16x3"
        # model.engine_bf16_linears: names of linear layers ("fc1", "fc2", "qkv", "attn out", "resid 1", ...) that take ONE bf16
        # product in the bf16x3 mode (their inputs' hi parts against the weights' hi parts): a third of their matrix work for a
        # measured logit error between the two pure modes (tests/test_gpu_hollow.py states it per setting)
        self.single = set(getattr(self.net.config.model, "engine_bf16_linears", ()) or ())
        self.dev = next(self.net.parameters()).device
        if self.dev.type != "cuda":
            raise native.CtddError("HollowEngine needs the model on a GPU")
        self._plans, self._wver = {}, None

    def _weights_version(self):
        return sum(p._version for p in self.net.parameters()) + 7919 * getattr(self.model, "_weights_version", 0)

    # ------------------------------------------------------------------ plan
    def _build(self, B, x_dtype):
        net, lib, dev = self.net, _lib(), self.dev
        m = net.config.model
        E, H, S, mlp = m.embed_dim, m.num_heads, net.S, m.mlp_dim
        D = int(m.concat_dim)
        hd = E // H
        st = type("Plan", (), {})()
        pb = PlanBuilder(self, B)
        plan, keep, fast, split = pb.plan, pb.keep, self.fast, self.split
        f32, hi, lo, P, W, launch, linear, layernorm, attention = (pb.f32, pb.hi, pb.lo, pb.P, pb.W, pb.launch, pb.linear, pb.layernorm,
                                                                   pb.attention)
        st.x_in = torch.zeros((B, D), dtype=x_dtype, device=dev)
        st.t_in = torch.zeros((B,), dtype=torch.float32, device=dev)

        R = B * D
        # ---- embedding
        st.l2r, st.r2l, st.temb = f32(B, D, E), f32(B, D, E), f32(B, E)
        pe = net.module_l2r.pos_embed.pe[0, :D].to(dev).float().contiguous()
        keep.append(pe)
        ea = _EmbedArgs()
        if x_dtype == torch.int64:
            ea.x64 = P(st.x_in)
        else:
            ea.x32 = P(st.x_in)
        ea.t, ea.w_in, ea.b_in, ea.pe = P(st.t_in), P(W(net.input_embedding.weight.reshape(-1))), P(W(net.input_embedding.bias)), P(pe)
        ea.B, ea.D, ea.E, ea.S, ea.temb_scale = B, D, E, S, float(net.temb_scale)
        ea.l2r, ea.r2l, ea.temb = P(st.l2r), P(st.r2l), P(st.temb)
        keep.append(ea)
        launch(lib.ctdd_hollow_embed, C.byref(ea))

        # ---- the two causal stacks
        ln_buf, qkv, ctx, hid = (None if fast else f32(R, E)), f32(R, 3 * E), (None if fast else f32(R, E)), (None if fast else f32(R, mlp))
        ln_hi, ctx_hi, hid_hi = hi(R, E), hi(R, E), hi(R, mlp)
        ln_lo, ctx_lo, hid_lo = lo(R, E), lo(R, E), lo(R, mlp)
        keep.extend([ln_buf, qkv, ctx, hid, ln_hi, ctx_hi, hid_hi, ln_lo, ctx_lo, hid_lo])
        for x, stack, mode in ((st.l2r, net.module_l2r, 0), (st.r2l, net.module_r2l, 1)):
            for blk in stack.trans_block_layers:
                sa, ff = blk.self_attention_block, blk.feed_forward_block
                mha = sa.self_attention
                layernorm(x, D * E, D, E, sa.norm, ln_buf, D * E, out_hi=ln_hi, out_hi_bs=D * E, out_lo=ln_lo)
                linear(ln_buf, R, E, mha.in_proj_weight, mha.in_proj_bias, qkv, label="qkv", x_hi=ln_hi, x_lo=ln_lo)
                attention(P(qkv), D * 3 * E, 3 * E, P(qkv) + 4 * E, D * 3 * E, 3 * E, P(qkv) + 8 * E, D * 3 * E, 3 * E, D, D, mode, ctx,
                          out_hi=ctx_hi, out_lo=ctx_lo)
                linear(ctx, R, E, mha.out_proj.weight, mha.out_proj.bias, x, res=x, label="attn out", x_hi=ctx_hi, x_lo=ctx_lo)   # in place: + inputs
                layernorm(x, D * E, D, E, ff.norm, ln_buf, D * E, out_hi=ln_hi, out_hi_bs=D * E, out_lo=ln_lo)
                linear(ln_buf, R, E, ff.mlp.fc1.weight, ff.mlp.fc1.bias, hid, act=1, label="fc1", x_hi=ln_hi, x_lo=ln_lo, out_hi=hid_hi,
                       out_lo=hid_lo)
                linear(hid, R, mlp, ff.mlp.fc2.weight, None, x, res=x, label="fc2", x_hi=hid_hi, x_lo=hid_lo)

        # ---- attention readout
        ro = net.readout_module
        ca = ro.cross_attention
        Tk = 2 * D + 1
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
        attention(P(qb), D * E, E, P(kb), Tk * E, E, P(vb), Tk * E, E, D, Tk, 2, ctx, out_hi=ctx_hi, out_lo=ctx_lo)
        xr, xr_hi, xr_lo = (None if fast else f32(R, E)), hi(R, E), lo(R, E)
        keep.extend([xr, xr_hi, xr_lo])
        linear(ctx, R, E, ca.out_linear.weight, ca.out_linear.bias, xr, res=raw, label="readout out", x_hi=ctx_hi, x_lo=ctx_lo, out_hi=xr_hi,
               out_lo=xr_lo)

        # ---- FiLM residual readout
        rr = ro.model
        E2 = 2 * E
        tm_h, tm = f32(B, mlp), f32(B, 4 * E)
        lin = [l for l in rr.mlp.layers if isinstance(l, torch.nn.Linear)]
        linear(st.temb, B, E, lin[0].weight, lin[0].bias, tm_h, act=2, label="temb mlp 1")
        linear(tm_h, B, mlp, lin[1].weight, lin[1].bias, tm, label="temb mlp 2")
        h, r, rh = f32(R, E2), f32(R, E2), (None if fast else f32(R, mlp))
        h_hi, rh_hi, h_lo, rh_lo = hi(R, E2), hi(R, mlp), lo(R, E2), lo(R, mlp)
        keep.extend([tm_h, tm, h, r, rh, h_hi, rh_hi, h_lo, rh_lo])
        linear(xr, R, E, rr.input_layer.weight, rr.input_layer.bias, h, label="readout in", x_hi=xr_hi, x_lo=xr_lo, out_hi=h_hi, out_lo=h_lo)
        for i in range(rr.n_res):
            mlp_i, ln_i = rr.resid_layers[2 * i], rr.resid_layers[2 * i + 1]
            li = [l for l in mlp_i.layers if isinstance(l, torch.nn.Linear)]
            linear(h, R, E2, li[0].weight, li[0].bias, rh, act=2, label="resid 1", x_hi=h_hi, x_lo=h_lo, out_hi=rh_hi, out_lo=rh_lo)
            linear(rh, R, mlp, li[1].weight, li[1].bias, r, label="resid 2", x_hi=rh_hi, x_lo=rh_lo)
            fl = f32(B, 4 * E)
            keep.append(fl)
            linear(tm, B, 4 * E, rr.film_layer[i].weight, rr.film_layer[i].bias, fl, label="film")          # per-sample path: fp32
            layernorm(h, D * E2, D, E2, ln_i, h, D * E2, y=r, y_bs=D * E2, film=fl, film_stride=4 * E, out_hi=h_hi, out_hi_bs=D * E2, out_lo=h_lo)
        st.logits = f32(B, D, rr.out_dim)
        linear(h, R, E2, rr.logits_layer.weight, rr.logits_layer.bias, st.logits, label="logits", x_hi=h_hi, x_lo=h_lo)
        st.plan, st.keep, st.graph = plan, keep, None
        return st

    # ------------------------------------------------------------------ execution
    def _run_plan(self, st):
        for step in st.plan:
            step()

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
                raise native.CtddError(f"HollowEngine expects integer states, got {x.dtype}")
            st = self._plans[key] = self._build(B, x.dtype)
            st.x_in.copy_(x.reshape(st.x_in.shape))
            st.t_in.copy_(times.float())
            self._run_plan(st)
            torch.cuda.synchronize()
            if getattr(self.net.config.model, "engine_graph", True):
                g = torch.cuda.CUDAGraph()
                with graph_capture(g):
                    self._run_plan(st)
                st.graph = g
        st.x_in.copy_(x.reshape(st.x_in.shape))
        st.t_in.copy_(times.float())
        if st.graph is not None:
            st.graph.replay()
        else:
            self._run_plan(st)
        return st.logits
