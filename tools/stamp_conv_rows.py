"""Phase durations of k_conv_rows (csrc/unet_rows_kernels.hip) and k_conv_rows_head (csrc/unet_head_kernels.hip) from the stamps build
(tools/build_conv_stamps.sh, -DCTDD_ROWS_STAMPS: thread 0 of every workgroup leaves s_memtime at the phase boundaries in the buffer
passed as out_stats; the statistics are off in that build).  Printed as raw s_memtime ticks (shader cycles), mean / min / max over
the workgroups of the third launch.

    bash tools/build_conv_stamps.sh && python tools/stamp_conv_rows.py [--batch 128] [--waves 8 4] [--head-waves 8 4]

--waves: the work splits of k_conv_rows to stamp (8: ctdd_unet_conv_rows, 4: ctdd_unet_conv_rows_w4; default both).  The stamps are
those of wave 0, which owns the band's upper 7 rows in the eight-wave kernel.  --head-waves: the same for k_conv_rows_head
(8: ctdd_unet_conv_rows_head, 4: ctdd_unet_conv_rows_head_w4; default both).
"""
import argparse
import ctypes as C
import os
import sys

_R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [_R, os.path.join(_R, "continuous-time-diffusion-models-for-discrete-data_amd")]
import torch  # noqa: E402

from ctdd import unet_engine as ue  # noqa: E402

ENTRY = {8: "ctdd_unet_conv_rows", 4: "ctdd_unet_conv_rows_w4"}
HEAD_ENTRY = {8: "ctdd_unet_conv_rows_head", 4: "ctdd_unet_conv_rows_head_w4"}
PHASES = ["prologue (zero fill, scale/shift)", "3x3 pieces (fill + K loop)", "1x1 segments", "epilogue to LDS", "store"]


def run(lib, waves, B, cs, rcs, res):
    H = W = 28
    M, N, Ct = B * H * W, 96, sum(cs)
    rn = lambda *s: torch.randn(s, device="cuda")
    xs, rs = [rn(M, c).to(torch.bfloat16) for c in cs], [rn(M, c).to(torch.bfloat16) for c in rcs]
    sts = []
    for x in xs:
        xd = x.double().view(B, H * W, -1)
        sts.append(torch.stack([xd.sum(1), (xd * xd).sum(1)], -1).contiguous())
    K = 9 * Ct + sum(rcs)
    w = ue.pack_conv_rows_weights((rn(N, K) / K ** 0.5).to(torch.bfloat16), cs, rcs)
    gamma, beta, bias = torch.ones(Ct, device="cuda"), torch.zeros(Ct, device="cuda"), torch.zeros(N, device="cuda")
    r = rn(M, N).to(torch.bfloat16) if res else None
    out = torch.empty((M, N), dtype=torch.bfloat16, device="cuda")
    nwg = B * 2
    buf = torch.zeros((nwg, 8), dtype=torch.int64, device="cuda")
    a = ue._ConvRowsArgs()
    for i, (x, st) in enumerate(zip(xs, sts)):
        setattr(a, f"s{i + 1}_bf16", x.data_ptr()); setattr(a, f"st{i + 1}", st.data_ptr()); setattr(a, f"C{i + 1}", x.shape[1])
    for i, x in enumerate(rs):
        setattr(a, f"r{i + 1}_bf16", x.data_ptr()); setattr(a, f"RC{i + 1}", x.shape[1])
    a.gamma, a.beta, a.G, a.eps, a.w, a.bias = gamma.data_ptr(), beta.data_ptr(), 32, 1e-5, w.data_ptr(), bias.data_ptr()
    if r is not None:
        a.res_bf16 = r.data_ptr()
    a.out_bf16, a.out_stats, a.B, a.H, a.W, a.N = out.data_ptr(), buf.data_ptr(), B, H, W, N
    st_ = torch.cuda.current_stream().cuda_stream
    for _ in range(3):
        assert getattr(lib, ENTRY[waves])(C.byref(a), 0, st_) == 0, lib.ctdd_last_error().decode()
    torch.cuda.synchronize()
    d = buf.cpu().double()
    dur = d[:, 1:6] - d[:, 0:5]
    print(f"{waves} waves B={B} 28x28 C={cs} raw={rcs} res={res}: {nwg} workgroups, per workgroup {float((d[:, 5] - d[:, 0]).mean()):.0f} cycles")
    for i, nm in enumerate(PHASES):
        print(f"   {nm:36s} mean {float(dur[:, i].mean()):8.0f}  min {float(dur[:, i].min()):8.0f}  max {float(dur[:, i].max()):8.0f}")


def run_head(lib, waves, B, C1, N):
    """k_conv_rows_head at 28x28: [workgroups][16] stamps: entry, prologue, fill, then per pass its K loop and its epilogue / store."""
    H = W = 28
    M, K, npass = B * H * W, 9 * C1, -(-N // 96)
    rn = lambda *s: torch.randn(s, device="cuda")
    x = rn(M, C1).to(torch.bfloat16)
    xd = x.double().view(B, H * W, -1)
    st = torch.stack([xd.sum(1), (xd * xd).sum(1)], -1).contiguous()
    w = ue.pack_conv_rows_head_weights((rn(N, K) / K ** 0.5).to(torch.bfloat16), C1)
    gamma, beta, bias = torch.ones(C1, device="cuda"), torch.zeros(C1, device="cuda"), torch.zeros(N, device="cuda")
    out = torch.empty((M, N), dtype=torch.bfloat16, device="cuda")
    nwg = B * 2
    buf = torch.zeros((nwg, 16), dtype=torch.int64, device="cuda")
    a = ue._ConvRowsArgs()
    a.s1_bf16, a.st1, a.C1 = x.data_ptr(), st.data_ptr(), C1
    a.gamma, a.beta, a.G, a.eps, a.w, a.bias = gamma.data_ptr(), beta.data_ptr(), 32, 1e-5, w.data_ptr(), bias.data_ptr()
    a.out_bf16, a.out_stats, a.B, a.H, a.W, a.N = out.data_ptr(), buf.data_ptr(), B, H, W, N
    st_ = torch.cuda.current_stream().cuda_stream
    for _ in range(3):
        assert getattr(lib, HEAD_ENTRY[waves])(C.byref(a), 0, st_) == 0, lib.ctdd_last_error().decode()
    torch.cuda.synchronize()
    d = buf.cpu().double()
    nst = 3 + 2 * npass
    dur = d[:, 1:nst] - d[:, 0:nst - 1]
    names = ["prologue (zero fill, scale/shift)", "fill"] + [f"pass {p} {what}" for p in range(npass) for what in ("K loop", "epilogue + store")]
    print(f"head {waves} waves B={B} 28x28 C1={C1} N={N}: {nwg} workgroups, per workgroup {float((d[:, nst - 1] - d[:, 0]).mean()):.0f} cycles")
    for i, nm in enumerate(names):
        print(f"   {nm:36s} mean {float(dur[:, i].mean()):8.0f}  min {float(dur[:, i].min()):8.0f}  max {float(dur[:, i].max()):8.0f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--waves", type=int, nargs="+", choices=(4, 8), default=[8, 4])
    ap.add_argument("--head-waves", type=int, nargs="+", choices=(4, 8), default=[8, 4])
    a = ap.parse_args()
    lib = C.CDLL(os.path.join(_R, "continuous-time-diffusion-models-for-discrete-data_amd", "librows_stamps.so"))
    for fn in (lib.ctdd_unet_conv_rows, lib.ctdd_unet_conv_rows_w4, lib.ctdd_unet_conv_rows_head, lib.ctdd_unet_conv_rows_head_w4):
        fn.argtypes, fn.restype = [C.c_void_p, C.c_int, C.c_void_p], C.c_int
    lib.ctdd_last_error.restype = C.c_char_p
    for cs, rcs, res in (([96], [], False), ([96], [], True), ([96, 96], [], False), ([192, 96], [], False), ([96], [96, 96], False)):
        for waves in a.waves:
            run(lib, waves, a.batch, cs, rcs, res)
    for C1, N in ((96, 256), (96, 96)):
        for waves in a.head_waves:
            run_head(lib, waves, a.batch, C1, N)


if __name__ == "__main__":
    main()
