"""Host cost of one call through the Python binding, without a GPU: a Tracer whose `_lib` is a stub (every entry returns 0) runs
render_frame, read_accum (16 x 8), trace_rays on one ray and denoise() CALLS times each, REPEATS times over; prints the median and the
spread (max - min) of the per-call time over the repeats.

    python tools/bench_cabi_overhead.py [--against FILE]

--against: another _cabi.py to measure beside the tree's own (one from another commit: `git show REV:ray-tracing-extended_amd/_cabi.py
> FILE`).  The two take turns repeat by repeat in one process, so that a machine that speeds up or slows down does so for both.
profiles/cabi_refactor_overhead.txt holds the tables of the change that folded the binding's near-copies together."""
import argparse
import importlib.util
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS, REPEATS = 20000, 5


class Stub:
    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        entry = lambda *args: 0          # noqa: E731
        setattr(self, name, entry)
        return entry


def cases(path, label):
    spec = importlib.util.spec_from_file_location("cabi_" + label.replace(" ", "_"), path)
    c = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = c
    spec.loader.exec_module(c)
    t = object.__new__(c.Tracer)
    t._lib, t._ctx = Stub(), 0x1000
    p = np.zeros((), c.PARAMS)
    p["width"], p["height"], p["numRaysPerPixel"] = 16, 8, 1
    t.set_params(p)
    ray = np.zeros((1, 8), np.float32)
    return {"render_frame": lambda: t.render_frame(3), "read_accum": t.read_accum, "trace_rays, 1 ray": lambda: t.trace_rays(ray),
            "denoise()": t.denoise}


def per_call(fn):
    t0 = time.perf_counter()
    for _ in range(CALLS):
        fn()
    return (time.perf_counter() - t0) / CALLS * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--against")
    a = ap.parse_args()
    sides = {"this tree": cases(os.path.join(ROOT, "ray-tracing-extended_amd", "_cabi.py"), "this tree")}
    if a.against:
        sides = {"the other": cases(a.against, "the other"), **sides}
    times = {side: {name: [] for name in table} for side, table in sides.items()}
    for name in next(iter(sides.values())):
        for rep in range(REPEATS + 1):                  # the first repeat warms up and is dropped
            for side, table in sides.items():
                dt = per_call(table[name])
                if rep:
                    times[side][name].append(dt)
    for side in sides:
        print(f"{side}: {CALLS} calls x {REPEATS} repeats, microseconds per call")
        print(f"  {'method':<20}{'median':>9}{'min':>9}{'max':>9}{'spread':>9}")
        for name, v in times[side].items():
            print(f"  {name:<20}{statistics.median(v):9.3f}{min(v):9.3f}{max(v):9.3f}{max(v) - min(v):9.3f}")
    if a.against:
        print("median of this tree - median of the other, and the other's spread")
        for name in times["this tree"]:
            d = statistics.median(times["this tree"][name]) - statistics.median(times["the other"][name])
            v = times["the other"][name]
            print(f"  {name:<20}{d:+9.3f}{max(v) - min(v):9.3f}")


if __name__ == "__main__":
    main()
