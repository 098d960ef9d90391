"""Issuing a launch list -- what AIREngine and SceneSampler (and ImportanceEvaluator, through its engine) share: a plan is a list of
(fn, args, name) entries of libair_hip.so that run in order on one stream, eagerly (inside roctx ranges when AIR_ROCTX=1) or captured
into a hipGraph; and the stream discipline of an object that owns a stream."""
import ctypes
import os

import torch

from . import _lib

_ROCTX = [False, None]


def _roctx():
    """libroctx64 when AIR_ROCTX=1 (and the library is there), else None; resolved once per process"""
    if not _ROCTX[0]:
        _ROCTX[0] = True
        if os.environ.get("AIR_ROCTX", "0") == "1":
            for name in ("libroctx64.so", "/opt/rocm/lib/libroctx64.so", "librocprofiler-sdk-roctx.so"):
                try:
                    lib = ctypes.CDLL(name)
                    lib.roctxRangePushA.argtypes = [ctypes.c_char_p]; lib.roctxRangePushA.restype = ctypes.c_int
                    lib.roctxRangePop.restype = ctypes.c_int
                    _ROCTX[1] = lib
                    break
                except (OSError, AttributeError):
                    continue
    return _ROCTX[1]


def run_plan(plan, stream_ptr):
    """Issue a plan: entries (fn, args, name) on the stream, in order.  AIR_ROCTX=1: every entry inside a roctx range named
    "<position> <C-ABI entry>" (rocprofv3 --marker-trace shows the plan next to the kernel trace of an EAGER
    step -- `bench.py --no-graph`; a captured graph replays kernel nodes only, its positions are tools/probes/plan_dump.py's)."""
    rx = _roctx()
    for i, e in enumerate(plan):
        if rx is not None:
            rx.roctxRangePushA(("%02d %s" % (i, e[2])).encode())
        st = e[0](*e[1], stream_ptr)
        if rx is not None:
            rx.roctxRangePop()
        if st != 0:
            _lib.check(st, e[2])


def capture_plans(plans, stream_ptr):
    """Capture a list of plan entries into one hipGraph.  An entry is either a launch plan (list of (fn, args, name)) or
    a callable taking the stream pointer (collectives, stream forks / joins)."""
    L = _lib.load()
    _lib.check(L.air_graph_begin_capture(stream_ptr), "air_graph_begin_capture")
    try:
        for pl in plans:
            if callable(pl):
                pl(stream_ptr)
            else:
                run_plan(pl, stream_ptr)
    finally:
        exe = ctypes.c_void_p()
        st = L.air_graph_end_capture(stream_ptr, ctypes.byref(exe))
    _lib.check(st, "air_graph_end_capture")
    return exe


def destroy_graphs(graphs):
    L = _lib.load()
    for g in graphs:
        if g is not None:
            L.air_graph_destroy(g)


class LaunchMixin:
    """For an object with `stream` and `device`: it runs on its own stream.  Everything that enters its buffers from outside (a
    batch gathered on the default stream, checkpoint tensors, injected noise) is ordered explicitly: its stream first waits for the
    producer's stream, the copy runs ON its stream, and a device-side source is marked as in use by that stream so the caching
    allocator cannot hand its block to a later allocation while the copy is still pending."""

    def _sp(self):
        return ctypes.c_void_p(self.stream.cuda_stream)

    def _run(self, plan, stream_ptr):
        run_plan(plan, stream_ptr)

    def _capture_plans(self, plans):
        return capture_plans(plans, self._sp())

    def _replay_or_run(self, graph, plan):
        """replay `graph` if it was captured, else issue `plan`"""
        if graph is not None:
            _lib.check(_lib.load().air_graph_launch(graph, self._sp()), "air_graph_launch")
        else:
            self._run(plan, self._sp())

    def _copy_in(self, dst, src):
        src_t = src if torch.is_tensor(src) else torch.as_tensor(src)
        self.wait_for_caller()
        with torch.cuda.stream(self.stream):
            dst.copy_(src_t.reshape(dst.shape), non_blocking=True)
        if src_t.is_cuda:
            src_t.record_stream(self.stream)

    def _fill_in(self, dst, value):
        with torch.cuda.stream(self.stream):
            dst.fill_(value)

    def wait_for_caller(self):
        """Order the object's stream after the caller's current stream (after torch code on another stream touched buffers
        the next launch reads or overwrites)."""
        self.stream.wait_stream(torch.cuda.current_stream(self.device))

    def wait_for_stream(self):
        """Order the CALLER's current stream after everything queued on the object's stream (before torch code on another
        stream reads buffers it writes: the shared parameters, outputs)."""
        torch.cuda.current_stream(self.device).wait_stream(self.stream)

    def synchronize(self):
        self.stream.synchronize()
