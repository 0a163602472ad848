"""Child process of tests/test_gpu_query_fuzz.py: for every seed of the range, one family (seed % 4: ray queries, radiance, gather,
visibility) and one of the two later ones (even seeds: multi-hit queries in the seed's form and as the whole list; odd seeds:
closest-point queries on the seed's points) on its device entries — a torch tensor of the items, on torch's current stream, which the
context runs the call on — gives the host entries' bits at the seed's options, samples, seed and firstIndex.  torch is imported before the library is loaded (torch brings
its own HIP runtime; the library then uses it), so it runs in a fresh process: query_fuzz_torch_worker.py <first seed> <seeds>
[name=value ...].  It prints a line per seed as it starts it, then one JSON object, seed -> null or what differed."""
import json
import os
import sys

import torch  # noqa: F401  (first: see above)
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def one_seed(rtx, qf, seed, overrides):
    more, form = qf.point_knobs(seed)
    overrides = dict(overrides)
    form.update({k: int(overrides.pop(k)) for k in list(overrides) if k in form})
    scene, items, options, call = qf.fuzz_case(rtx, seed, overrides={**more, **overrides})
    side = torch.cuda.Stream()
    with rtx.Tracer(0) as t:
        qf.load_scene(t, scene, options)
        with torch.cuda.stream(side):
            dev = torch.from_numpy(items.view(np.float32).reshape(-1, 8).copy()).cuda()
            if seed % 4 == 0:
                runs = [("trace_rays", t.trace_rays(items).view(np.uint32).reshape(-1, 16), t.trace_rays(dev).cpu().numpy().view(np.uint32)),
                        ("occluded", t.occluded(items), t.occluded(dev).cpu().numpy())]
            else:
                family = ("radiance", "gather", "visibility")[seed % 4 - 1]
                runs = [(f"{family} mode {mode}", qf.run_family(t, items, call, family, mode).view(np.uint32),
                         qf.run_family(t, dev, call, family, mode).cpu().numpy().view(np.uint32)) for f, mode in qf.FAMILIES if f == family]
            if seed % 2 == 0:
                runs += [(f"trace_hits {f}", qf.run_hits(t, items, f).view(np.uint32).reshape(len(items), f["K"], 16),
                          qf.run_hits(t, dev, f).cpu().numpy().view(np.uint32)) for f in (form, qf.DEEP)]
            else:
                points = qf.fuzz_points(rtx, seed, scene, items)
                pdev = torch.from_numpy(points.view(np.float32).reshape(-1, 8).copy()).cuda()
                runs.append(("closest_points", t.closest_points(points).view(np.uint32).reshape(-1, 16), t.closest_points(pdev).cpu().numpy().view(np.uint32),
                             points))
        for what, host, device, *of in runs:
            given = of[0] if of else items
            if host.shape != device.shape:
                return f"{what}: host {host.shape}, device {device.shape}"
            bad = np.where((host != device).reshape(len(host), -1).any(1))[0]
            if len(bad):
                return (f"{what}, seed {seed}: the device entry differs from the host entry on {len(bad)} items, first {qf.describe(given, bad[0])}: "
                        f"host {host[bad[0]].tolist()} device {device[bad[0]].tolist()}; options {options} call {call}")
    return None


def main():
    import rtx_pkg
    import query_fuzz as qf
    rtx = rtx_pkg.load()
    first, count = int(sys.argv[1]), int(sys.argv[2])
    overrides = dict(a.split("=") for a in sys.argv[3:])
    report = {}
    for seed in range(first, first + count):
        print(f"QUERY_FUZZ_SEED {seed} {qf.fuzz_knobs(seed)}", flush=True)       # (the last of these lines names the seed a crash or a hang was in)
        try:
            report[seed] = one_seed(rtx, qf, seed, overrides)
        except Exception as e:                                                       # an error of the library: this seed's, not every seed's
            report[seed] = f"device entries, seed {seed}, {qf.fuzz_knobs(seed)}: {type(e).__name__}: {e}"
    print("QUERY_FUZZ_DEVICE " + json.dumps(report))


if __name__ == "__main__":
    main()
