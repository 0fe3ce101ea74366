"""Shared by profiles/bench_mesh_depth.py and profiles/bench_closest_points.py: device times of a cell-list build's two calls."""
import statistics

import torch


def build_phases(make, prefix, warmup=3, reps=10):
    """Median device ms of a build's two library calls, `prefix`_count (memset, count kernel, scan kernel) and `prefix`_fill:
    events around each call over `reps` builds after `warmup` (the host read of the pair total lies between the two)."""
    from gelslim_depth_amd._lib import lib
    spans = {}

    def wrap(name):
        fn = getattr(lib, name)

        def call(*args):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            rc = fn(*args)
            e1.record()
            spans.setdefault(name, []).append((e0, e1))
            return rc
        setattr(lib, name, call)
        return fn
    names = (prefix + "_count", prefix + "_fill")
    keep = [wrap(n) for n in names]
    try:
        for _ in range(warmup + reps):
            make()
        torch.cuda.synchronize()
    finally:
        for n, fn in zip(names, keep):
            setattr(lib, n, fn)
    return [statistics.median(e0.elapsed_time(e1) for e0, e1 in spans[n][warmup:]) for n in names]
