"""What every engine and trainer shares (ctdd/unet_engine.py, ctdd/plan_common.py, ctdd/hollow_train.py and the modules built on
them): the pointer helpers, the network behind a DistributedDataParallel wrapper, the pre-bound launch a plan is a list of, graph
capture, and the tile pick of the patch kernel run as a plain GEMM."""
import contextlib
import gc

import torch

from . import native


def ptr(t):
    return None if t is None else t.data_ptr()


def unwrap(net):
    """cfg.distributed wraps the network in DistributedDataParallel (models.py:104-107); the engines read the module behind it."""
    return net.module if hasattr(net, "module") and net.__class__.__name__ == "DistributedDataParallel" else net


def set_state_ptr(args, x, who):
    """Point the x64 / x32 pair of an argument block at the integer states x; `who` names the caller in the error."""
    if x.dtype == torch.int64:
        args.x64 = x.data_ptr()
    elif x.dtype == torch.int32:
        args.x32 = x.data_ptr()
    else:
        raise native.CtddError(f"{who} expects integer states, got {x.dtype}")


def bound_launch(fn, *args, label=None, flops=0):
    """`fn(*args, stream)` on the stream that is current when the step runs; a non-zero return raises with the library's message."""
    def run():
        rc = fn(*args, torch.cuda.current_stream().cuda_stream)
        if rc != 0:
            raise native.CtddError(f"{fn.__name__} failed ({rc}): {native.load().ctdd_last_error().decode()}")
    run.label, run.flops = (fn.__name__, label), flops      # flops: matrix FLOPs of the launch (bench.py's network roofline)
    return run


@contextlib.contextmanager
def graph_capture(graph):
    """`torch.cuda.graph(graph)` with Python's cyclic collector held off.  The context no longer collects on entry
    (torch.compiler.config.force_cudagraph_gc, off by default), and a collection that happens to start between capture_begin and
    capture_end finalises whatever dead cycles hold -- device tensors, graphs, their pools -- from inside the capture, with runtime
    calls a capturing stream does not allow: the process aborts, and whether it does depends on how many objects the interpreter
    allocated before.  So: collect now, then no collection until the capture has ended."""
    gc.collect()
    was_enabled = gc.isenabled()
    gc.disable()
    try:
        with torch.cuda.graph(graph):
            yield
    finally:
        if was_enabled:
            gc.enable()


def patch_gemm_tiles(K, N):
    """(bk, bnt) of ctdd_unet_conv_patch for one 1x1 segment of K channels over a rows x 1 "image" with N outputs."""
    pbk = 64 if K % 64 == 0 else 48 if K % 48 == 0 else 32 if K % 32 == 0 else 16
    if pbk == 64:
        pbnt = 4 if N > 64 else 2 if N > 32 else 1
    elif pbk == 48:
        pbnt = 4 if N % 128 == 0 else 3 if N > 64 else 2 if N > 32 else 1
    elif pbk == 32:
        pbnt = 4 if N % 128 == 0 else 3 if N > 32 else 1
    else:
        pbnt = 1
    return pbk, pbnt
