"""What the transformer inference engines (ctdd/hollow_engine.py, ctdd/bert_engine.py) share: the ctypes argument blocks of the
hollow-transformer entry points (include/ctdd_hollow.h); PlanBuilder, which records a forward as a flat list of pre-bound
libctdd launches -- linear layers on the GEMM kernels per engine precision, LayerNorm (+ FiLM), attention, and out of those the
prenorm encoder block (encoder_blocks) and the FiLM residual readout (film_readout) that both networks are made of; and
PlanEngine, the wrapper that caches one plan per (batch, state dtype), warms it, captures it and replays it."""
import ctypes as C
import math
import types

import torch

from . import native
from .plan_launch import bound_launch, graph_capture, patch_gemm_tiles, ptr, unwrap
from .unet_engine import _ConvArgs, _lib as _unet_lib, SEG_1x1

_P, _I, _F, _I64 = C.c_void_p, C.c_int, C.c_float, C.c_int64


class _EmbedArgs(C.Structure):
    _fields_ = [("x64", _P), ("x32", _P), ("t", _P), ("w_in", _P), ("b_in", _P), ("pe", _P), ("B", _I), ("D", _I), ("E", _I),
                ("S", _I), ("temb_scale", _F), ("l2r", _P), ("r2l", _P), ("temb", _P)]


class _LnArgs(C.Structure):
    _fields_ = [("x", _P), ("y", _P), ("x_bs", _I64), ("y_bs", _I64), ("out_bs", _I64), ("gamma", _P), ("beta", _P), ("eps", _F),
                ("film", _P), ("film_stride", _I), ("B", _I), ("T", _I), ("E", _I), ("out", _P), ("out_hi", _P), ("out_hi_bs", _I64), ("out_lo", _P)]


class _GemmArgs(C.Structure):
    _fields_ = [("a", _P * 3), ("nseg", _I), ("w", _P), ("bias", _P), ("res", _P), ("out_f32", _P), ("out_hi", _P), ("out_lo", _P),
                ("M", _I), ("N", _I), ("K", _I), ("act", _I), ("drop_p", _F), ("rng", _P), ("layer", C.c_uint64), ("mask_u", _P)]


class _AttnArgs(C.Structure):
    _fields_ = [("q", _P), ("k", _P), ("v", _P), ("q_bs", _I64), ("k_bs", _I64), ("v_bs", _I64), ("q_rs", _I), ("k_rs", _I),
                ("v_rs", _I), ("B", _I), ("Tq", _I), ("Tk", _I), ("H", _I), ("hd", _I), ("mode", _I), ("scale", _F), ("out", _P),
                ("out_rs", _I), ("out_hi", _P), ("out_lo", _P), ("split", _I)]


_sigs_done = False


def _lib():
    global _sigs_done
    lib = _unet_lib()
    if not _sigs_done:
        for name, argt in (("ctdd_hollow_embed", [_P, _P]), ("ctdd_hollow_layernorm", [_P, _P]),
                           ("ctdd_hollow_add", [_P, _I64, _P, _I64, _P, _P, _P, _I64, _I, _I64, _P]),
                           ("ctdd_hollow_put_rows", [_P, _P, _P, _P, _I64, _I, _I, _P]), ("ctdd_hollow_attention", [_P, _P]),
                           ("ctdd_hollow_attention_bf16", [_P, _P]), ("ctdd_gemm_bf16", [_P, _P]),
                           ("ctdd_hollow_small_linear", [_P, _P, _P, _I, _I, _I, _I, _P, _P])):
            fn = getattr(lib, name)
            fn.argtypes, fn.restype = argt, _I
        _sigs_done = True
    return lib


class PlanBuilder:
    """Launch list (`plan`) and the buffers it must keep alive (`keep`) of one plan of `engine` (its .net, .dev, .fast, .split,
    .single) for batch B.  fast: bf16 GEMM / attention operands; split: hi + lo bf16 pairs, three products per contraction."""

    def __init__(self, engine, B):
        self.lib, self.dev, self.m = _lib(), engine.dev, engine.net.config.model
        self.fast, self.split, self.single = engine.fast, engine.split, engine.single
        self.B, self.E, self.H = B, self.m.embed_dim, self.m.num_heads
        self.hd = self.E // self.H
        self.plan, self.keep = [], []

    def f32(self, *shape):
        return torch.empty(shape, dtype=torch.float32, device=self.dev)

    def hi(self, *shape):                           # bf16 GEMM operands
        return torch.empty(shape, dtype=torch.bfloat16, device=self.dev) if self.fast else None

    def lo(self, *shape):                           # their second terms
        return torch.empty(shape, dtype=torch.bfloat16, device=self.dev) if self.split else None

    P = staticmethod(ptr)

    def W(self, p):                                 # fp32 contiguous view of a parameter (kept alive)
        t = p.detach().float().contiguous()
        self.keep.append(t)
        return t

    def launch(self, fn, *args, label=None, flops=0):
        self.plan.append(bound_launch(fn, *args, label=label, flops=flops))

    def linear(self, x, rows, K, lin_w, lin_b, out, act=0, res=None, label="", x_hi=None, out_hi=None, x_lo=None, out_lo=None):
        """out[rows][N] = act(x[rows][K] @ W^T + b) (+ res) on the implicit-GEMM kernel: fp32 operands, or bf16
        operands (x_hi, bf16 weights) when x_hi is given; out (fp32) and/or out_hi (bf16) receive the result."""
        split, m, lib, keep, launch, P, W = self.split, self.m, self.lib, self.keep, self.launch, self.P, self.W
        w = W(lin_w)
        N = w.shape[0]
        assert w.shape[1] == K and K % 16 == 0
        if x_hi is None and res is None and rows <= 64 and K % 64 == 0 and K <= 1024 and x is not None and out is not None:
            # per-sample layers (time-embedding MLP, FiLM): a few MFLOP in fp32 -- one wave per output column
            bptr = P(W(lin_b)) if lin_b is not None else None
            launch(lib.ctdd_hollow_small_linear, P(x), P(w), bptr, rows, K, N, act, P(out), label=f"linear {label} {rows}x{K}->{N} rows",
                   flops=2 * rows * K * N)
            return
        a = _ConvArgs()
        a.nseg = 1
        a.seg[0].C, a.seg[0].kind = K, SEG_1x1
        use_bf16 = x_hi is not None
        if split and use_bf16 and (N % 8 != 0 or x_lo is None):
            assert x is not None, label                      # (a 3-column logits layer: the exact-fp32 kernel)
            use_bf16 = False
        if use_bf16 and split and label in self.single:
            wh = w.to(torch.bfloat16).contiguous()
            keep.append(wh)
            a.seg[0].hi, a.w_hi = P(x_hi), P(wh)
        elif use_bf16 and split:
            wh = w.to(torch.bfloat16)
            wl = (w - wh.float()).to(torch.bfloat16)
            wcat = torch.cat([wh, wh, wl], dim=1).contiguous()        # [N][3K] against the segments [x_hi | x_lo | x_hi]
            keep.append(wcat)
            a.nseg = 3
            for si, xs in enumerate((x_hi, x_lo, x_hi)):
                a.seg[si].C, a.seg[si].kind, a.seg[si].hi = K, SEG_1x1, P(xs)
            a.w_hi = P(wcat)
        elif use_bf16:
            wh = w.to(torch.bfloat16).contiguous()
            keep.append(wh)
            a.seg[0].hi, a.w_hi = P(x_hi), P(wh)
        else:
            a.seg[0].f32, a.w_f32 = P(x), P(w)
        a.B, a.H, a.W, a.Hin, a.Win, a.N, a.Ktot = 1, rows, 1, rows, 1, N, K * a.nseg
        a.bias = P(W(lin_b)) if lin_b is not None else None
        a.res_f32 = P(res)
        a.out_f32, a.out_hi, a.act = P(out), P(out_hi) if use_bf16 or not split else None, act
        a.out_lo = P(out_lo) if use_bf16 else None
        keep.append(a)
        if use_bf16:
            bk = 96 if K % 96 == 0 else 64 if K % 64 == 0 else 32 if K % 32 == 0 else 16
            bnt = 1 if bk == 16 else (3 if (N % 96 == 0 and bk in (96, 32)) else 4 if N % 128 == 0 else 2 if (N % 64 == 0 and bk == 64) else 1)
            if (bk, bnt) not in ((96, 3), (96, 4), (96, 1), (64, 4), (64, 2), (64, 1), (32, 1), (32, 3), (32, 4), (16, 1)):
                bnt = 1
        else:
            bk = 32 if K % 32 == 0 else 16
            bnt = 1 if bk == 16 else (3 if N % 96 == 0 else 4 if N % 128 == 0 else 1)
        if use_bf16 and N % 8 == 0 and K % 64 == 0 and getattr(m, "engine_linear", "gemm") == "gemm":
            # the plain GEMM kernel (csrc/gemm_kernels.hip); the hi / lo split product is three A segments against the
            # concatenated weight.  MNIST hollow forward, batch 64: linears 9.2 ms on the slab kernel below (model.engine_linear =
            # "patch") -> 7.7 ms; maze batch 128: forward 6.35 -> 5.52 ms
            ga = _GemmArgs()
            ga.nseg, ga.w, ga.bias, ga.res = a.nseg, a.w_hi, a.bias, a.res_f32
            for si in range(a.nseg):
                ga.a[si] = a.seg[si].hi
            ga.out_f32, ga.out_hi, ga.out_lo, ga.M, ga.N, ga.K, ga.act = a.out_f32, a.out_hi, a.out_lo, rows, N, K, act
            keep.append(ga)
            launch(lib.ctdd_gemm_bf16, C.byref(ga), label=f"linear {label} {rows}x{K}->{N} gemm", flops=2 * rows * K * N * a.nseg)
            return
        if use_bf16 and N % 8 == 0 and K % 16 == 0 and getattr(m, "engine_linear", "gemm") in ("gemm", "patch"):
            # the U-Net's slab kernel run as a plain GEMM (one 1x1 segment over a rows x 1 "image"): 16-byte row-major
            # epilogue, weights and activations staged per 128/256-row tile
            pbk, pbnt = patch_gemm_tiles(K, N)
            ext = act != 0 or a.out_lo                 # activation / hi + lo outputs: the EXT instantiations (wm = 32)
            wm = 64 if (not ext and rows >= 256 * 256 and (pbk, pbnt) in ((48, 3), (48, 4), (64, 4), (64, 2), (48, 2))) else 32
            launch(lib.ctdd_unet_conv_patch, C.byref(a), pbk, pbnt, wm, label=f"linear {label} {rows}x{K}->{N} patch",
                   flops=2 * rows * K * N * a.nseg)
            return
        launch(lib.ctdd_unet_conv, C.byref(a), bk, bnt, 0 if use_bf16 else 1, label=f"linear {label} {rows}x{K}->{N}",
               flops=2 * rows * K * N)

    def layernorm(self, x, x_bs, T, Ed, norm, out, out_bs, y=None, y_bs=0, film=None, film_stride=0, out_hi=None, out_hi_bs=0, out_lo=None, B=None):
        P, W = self.P, self.W
        B = self.B if B is None else B
        a = _LnArgs()
        a.x, a.y, a.x_bs, a.y_bs, a.out_bs = P(x), P(y), x_bs, y_bs, out_bs
        a.gamma, a.beta, a.eps = P(W(norm.weight)), P(W(norm.bias)), float(norm.eps)
        a.film, a.film_stride, a.B, a.T, a.E, a.out = P(film), film_stride, B, T, Ed, P(out)
        a.out_hi, a.out_hi_bs, a.out_lo = P(out_hi), out_hi_bs, P(out_lo)
        self.keep.append(a)
        self.launch(self.lib.ctdd_hollow_layernorm, C.byref(a))

    def attention(self, q, q_bs, q_rs, k, k_bs, k_rs, v, v_bs, v_rs, Tq, Tk, mode, out, out_hi=None, out_lo=None, B=None, fn=None):
        P, lib, m, E, H, hd, split, fast = self.P, self.lib, self.m, self.E, self.H, self.hd, self.split, self.fast
        B = self.B if B is None else B
        a = _AttnArgs()
        a.q, a.k, a.v, a.q_bs, a.k_bs, a.v_bs, a.q_rs, a.k_rs, a.v_rs = q, k, v, q_bs, k_bs, v_bs, q_rs, k_rs, v_rs
        a.B, a.Tq, a.Tk, a.H, a.hd, a.mode, a.scale, a.out, a.out_rs = B, Tq, Tk, H, hd, mode, 1.0 / math.sqrt(hd), P(out), E
        a.out_hi, a.out_lo, a.split = P(out_hi), P(out_lo), 1 if split else 0
        self.keep.append(a)
        if fn is None:                                  # (fn: another entry point with the same argument block)
            fn = lib.ctdd_hollow_attention_bf16 if (fast and hd in (16, 32) and getattr(m, "engine_attention", "mfma") == "mfma") else lib.ctdd_hollow_attention
        self.launch(fn, C.byref(a), label=f"attention mode {mode} {Tq}x{Tk}")

    def encoder_buffers(self, R):
        """The work buffers of encoder_blocks over R token rows (kept alive): LayerNorm output, packed qkv, attention context
        and MLP hidden rows in fp32, and the hi / lo bf16 operand twins of all but qkv."""
        E, mlp, fast, f32, hi, lo = self.E, self.m.mlp_dim, self.fast, self.f32, self.hi, self.lo
        b = types.SimpleNamespace(ln=None if fast else f32(R, E), qkv=f32(R, 3 * E), ctx=None if fast else f32(R, E),
                                  hid=None if fast else f32(R, mlp))
        b.ln_hi, b.ctx_hi, b.hid_hi = hi(R, E), hi(R, E), hi(R, mlp)
        b.ln_lo, b.ctx_lo, b.hid_lo = lo(R, E), lo(R, E), lo(R, mlp)
        self.keep.extend(vars(b).values())
        return b

    def encoder_blocks(self, x, layers, seqs, T, mode, bufs, attention_fn=None):
        """The prenorm transformer blocks `layers` over the residual stream x (seqs, T, E), in place: LayerNorm -> qkv linear ->
        attention `mode` over the T tokens of every sequence -> out-proj + x -> LayerNorm -> fc1 (ReLU) -> fc2 + x.
        bufs: encoder_buffers(seqs * T); attention_fn: another attention entry point (PlanBuilder.attention's fn)."""
        E, mlp, P, b, linear, layernorm = self.E, self.m.mlp_dim, self.P, bufs, self.linear, self.layernorm
        R = seqs * T
        for blk in layers:
            sa, ff = blk.self_attention_block, blk.feed_forward_block
            mha = sa.self_attention
            layernorm(x, T * E, T, E, sa.norm, b.ln, T * E, out_hi=b.ln_hi, out_hi_bs=T * E, out_lo=b.ln_lo, B=seqs)
            linear(b.ln, R, E, mha.in_proj_weight, mha.in_proj_bias, b.qkv, label="qkv", x_hi=b.ln_hi, x_lo=b.ln_lo)
            self.attention(P(b.qkv), T * 3 * E, 3 * E, P(b.qkv) + 4 * E, T * 3 * E, 3 * E, P(b.qkv) + 8 * E, T * 3 * E, 3 * E, T, T, mode, b.ctx,
                           out_hi=b.ctx_hi, out_lo=b.ctx_lo, B=seqs, fn=attention_fn)
            linear(b.ctx, R, E, mha.out_proj.weight, mha.out_proj.bias, x, res=x, label="attn out", x_hi=b.ctx_hi, x_lo=b.ctx_lo)   # in place: + inputs
            layernorm(x, T * E, T, E, ff.norm, b.ln, T * E, out_hi=b.ln_hi, out_hi_bs=T * E, out_lo=b.ln_lo, B=seqs)
            linear(b.ln, R, E, ff.mlp.fc1.weight, ff.mlp.fc1.bias, b.hid, act=1, label="fc1", x_hi=b.ln_hi, x_lo=b.ln_lo, out_hi=b.hid_hi,
                   out_lo=b.hid_lo)
            linear(b.hid, R, mlp, ff.mlp.fc2.weight, None, x, res=x, label="fc2", x_hi=b.hid_hi, x_lo=b.hid_lo)

    def film_readout(self, rr, xr, xr_hi, xr_lo, temb, B, Dp):
        """The FiLM residual readout `rr` (hollow_networks.py: ResidualReadout) over the B * Dp rows xr (fp32 and / or hi, lo) with
        the per-sample time embedding temb (B, E) -> the logits buffer (B, Dp, out_dim)."""
        E, mlp, fast, f32, hi, lo, keep, linear = self.E, self.m.mlp_dim, self.fast, self.f32, self.hi, self.lo, self.keep, self.linear
        R, E2 = B * Dp, 2 * E
        tm_h, tm = f32(B, mlp), f32(B, 4 * E)
        lin = [l for l in rr.mlp.layers if isinstance(l, torch.nn.Linear)]
        linear(temb, B, E, lin[0].weight, lin[0].bias, tm_h, act=2, label="temb mlp 1")
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
            fl = f32(B, 4 * E)                          # one per iteration: the plan keeps them alive across graph replay
            keep.append(fl)
            linear(tm, B, 4 * E, rr.film_layer[i].weight, rr.film_layer[i].bias, fl, label="film")          # per-sample path: fp32
            self.layernorm(h, Dp * E2, Dp, E2, ln_i, h, Dp * E2, y=r, y_bs=Dp * E2, film=fl, film_stride=4 * E, out_hi=h_hi, out_hi_bs=Dp * E2,
                           out_lo=h_lo, B=B)
        logits = f32(B, Dp, rr.out_dim)
        linear(h, R, E2, rr.logits_layer.weight, rr.logits_layer.bias, logits, label="logits", x_hi=h_hi, x_lo=h_lo)
        return logits


class PlanEngine:
    """The inference engine around a plan: subclasses give `_build(B, x_dtype)`, which returns a plan object with the input
    buffers x_in, t_in, the output buffer logits and -- for the default `_run` / `_capture` -- one launch list `plan` and
    `graph = None`.  One plan per (batch, state dtype), dropped when the weights move.

    precision "fp32": exact-fp32 matrix instructions and fp32 FMA attention; "bf16": bf16 operands (~1e-3 absolute on the logits);
    "bf16x3" (default): every GEMM / attention operand as a hi + lo bf16 pair, three bf16 products per contraction with fp32
    accumulation (x w ~ xh wh + xl wh + xh wl, dropped terms ~2^-17 relative): fp32-grade logits at bf16 matrix rates.
    model.engine_bf16_linears: names of linear layers (the labels given to PlanBuilder.linear: "qkv", "attn out", "fc1", "fc2", ...) that take ONE bf16 product
    in the bf16x3 mode (their inputs' hi parts against the weights' hi parts): a third of their matrix work for a measured logit
    error between the two pure modes (tests/test_gpu_hollow.py states it per setting)."""

    def __init__(self, model, precision=None):
        self.model, self.net = model, unwrap(model.net)
        self.precision = precision or getattr(self.net.config.model, "engine_precision", "bf16x3")
        if self.precision not in ("fp32", "bf16", "bf16x3"):
            raise ValueError(f"unknown engine precision {self.precision}")
        self.fast = self.precision in ("bf16", "bf16x3")
        self.split = self.precision == "bf16x3"
        self.single = set(getattr(self.net.config.model, "engine_bf16_linears", ()) or ())
        self.dev = next(self.net.parameters()).device
        if self.dev.type != "cuda":
            raise native.CtddError(f"{type(self).__name__} needs the model on a GPU")
        self._plans, self._wver = {}, None

    def _weights_version(self):
        return sum(p._version for p in self.net.parameters()) + 7919 * getattr(self.model, "_weights_version", 0)

    @staticmethod
    def _run(st):
        if st.graph is not None:
            st.graph.replay()
        else:
            for step in st.plan:
                step()

    @staticmethod
    def _capture(st):
        g = torch.cuda.CUDAGraph()
        with graph_capture(g):
            for step in st.plan:
                step()
        st.graph = g

    def __call__(self, x, times):
        key = (x.shape[0], x.dtype)
        ver = self._weights_version()
        if ver != self._wver:
            self._plans.clear()
            self._wver = ver
        st = self._plans.get(key)
        if st is None:
            # build (which refuses other than integer states) -> inputs -> eager warm run -> synchronize -> capture: in this
            # order, so that nothing of the warm run is in flight when the capture begins (plan_launch.graph_capture)
            st = self._plans[key] = self._build(*key)
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
