"""What the *_perf.py scripts share: HIP events around one call, the rounds in which all variants alternate, and the
summary of one variant's times."""
import numpy as np
import torch


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def alternate(runs, warm, rep):
    """runs: {name: callable}.  warm + rep rounds, every variant once a round in the dict's order, the warm-up rounds
    dropped: {name: [ms] * rep}"""
    t = {name: [] for name in runs}
    for it in range(warm + rep):
        for name, fn in runs.items():
            ms = timed(fn)
            if it >= warm:
                t[name].append(ms)
    return t


def stats(v, nbytes):
    v = np.array(v)
    return {"median_ms": float(np.median(v)), "min_ms": float(v.min()), "max_ms": float(v.max()),
            "GBps": nbytes / float(np.median(v)) / 1e6}
