"""The timing wrapper of tools/fsv_bench.py, tools/dlmfsv_bench.py and tools/dlmfsvsys_bench.py: an Engine whose method calls are
forwarded with the wall time taken around each (the engine's calls are synchronous), so that a tool can run the driver's own sweep and
still report the time of every call in it."""
import time

import numpy as np


class TimedEngine:
    def __init__(self, engine):
        self._engine = engine
        self.calls = []             # (method name, seconds) of every forwarded call since the last take()
        self.ffbs_variant = None    # Engine.last_variant after the last ffbs call

    def __getattr__(self, name):
        target = getattr(self._engine, name)
        if not callable(target):
            return target

        def timed(*args, **kwargs):
            t0 = time.perf_counter()
            out = target(*args, **kwargs)
            self.calls.append((name, time.perf_counter() - t0))
            if name == "ffbs":
                self.ffbs_variant = self._engine.last_variant
            return out
        return timed

    def take(self, names):
        """The seconds of the calls since the last take(), which must be the methods `names` in that order; forgets them."""
        got, self.calls = self.calls, []
        if [n for n, _ in got] != list(names):
            raise RuntimeError(f"the sweep made the calls {[n for n, _ in got]}, the tool names {list(names)}")
        return [s for _, s in got]


def time_sweeps(engine, sweep, methods, iters, warmup):
    """Runs sweep(timed engine, it) for it = 0 .. warmup + iters - 1, each after a device synchronisation.  Returns (med, variant, status):
    med[0] the median over the last `iters` iterations of the sum of the calls' wall times in ms (what lies between two calls on the host,
    the driver's status reads among it, is in none of them) and med[1:] the median of each call's, in the order of `methods`; the variant of
    the last ffbs call; and the statuses that sweep returns by name, or'ed over all calls and iterations into one int."""
    import torch
    timed = TimedEngine(engine)
    rows, status = [], 0
    for it in range(warmup + iters):
        torch.cuda.synchronize()
        st = sweep(timed, it)
        secs = timed.take(methods)
        for flags in st.values():
            status |= int(np.asarray(flags.cpu() if hasattr(flags, "cpu") else flags).max())
        if it >= warmup:
            rows.append([sum(secs)] + secs)
    return np.median(np.array(rows) * 1e3, axis=0), timed.ffbs_variant, status


def time_fill(engine, buffer, nbytes, iters, warmup):
    """The median wall time in ms of a dlm_buffer_fill of `nbytes` into the device tensor `buffer`: what plain device writes reach."""
    import torch
    fills = []
    for _ in range(warmup + iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        engine._check(engine.lib.dlm_buffer_fill(engine.h, buffer.data_ptr(), 0, 0, nbytes))
        engine.sync()
        fills.append(time.perf_counter() - t0)
    return float(np.median(fills[warmup:]) * 1e3)
