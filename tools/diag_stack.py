#!/usr/bin/env python3
"""How deep k_stream's traversal stacks really go, and what its stack guard costs: the counting kernel of a build with -DRT_DIAG_STACK
(tools/build_variant.py stackdiag -DRT_DIAG_STACK; run with RTX_LIB=ab_libs/librt_stackdiag.so) re-uses phase counters 3 / 4
(csrc/rt_stream_body.hpp).  One JSON line per (config, LDS stack entries): 16 frames of the benchmark workload.
    RTX_LIB=ab_libs/librt_stackdiag.so python tools/diag_stack.py [entries ...]      (default 21 24)"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rtx_pkg
rtx = rtx_pkg.load()

caps = [int(a) for a in sys.argv[1:]] or [21, 24]
names = None
for cfg in (3, 5):
    mgr = {3: rtx.scenes.config3, 5: rtx.scenes.config5}[cfg]()
    params, spheres, tris, infos = mgr.build_buffers()
    for cap in caps:
        with rtx.Tracer(0) as t:
            t.set_params(params); t.upload(spheres=spheres, triangles=tris, meshinfo=infos)
            t.set_option("kernel", 1); t.set_option("stream_stack", cap)
            t.render(0, 4); t.reset_accum()
            t.render_counting(0, 16)
            st = t.stats()
        L, E, R = st["phaseLanes"], st["phaseExecs"], st["regionExecs"]
        if names is None:
            import re
            text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ray-tracing-extended_amd", "csrc", "rt_kernels.hpp")).read()
            names = re.findall(r"X\((\w+)\)", re.search(r"#define RT_REGION_LIST\(X\)(.*?)\n(?!\s*X\()", text, re.S).group(1))
        reg = dict(zip(names, R))
        steps = E[0]
        print(json.dumps({"config": cfg, "lds_entries": cap, "bvhMaxStack": st["bvhMaxStack"], "node_steps": steps, "node_loop_iterations": reg["nodeloop"],
                          "deepest_stack_of_any_lane": L[3],
                          "former_guard_trips": E[4], "former_guard_trip_share_of_node_steps": round(E[4] / max(steps, 1), 6),
                          "bound_tightened": E[3], "tightened_share_of_iterations": round(E[3] / max(reg["nodeloop"], 1), 6),
                          "second_ballot": L[4], "second_ballot_share_of_iterations": round(L[4] / max(reg["nodeloop"], 1), 6),
                          "checked_push_steps": reg["node_spill"], "checked_push_share_of_node_steps": round(reg["node_spill"] / max(steps, 1), 6)}), flush=True)
