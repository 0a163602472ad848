"""What the query fuzz shares (tests/test_query_fuzz_cpu.py, tests/test_gpu_query_fuzz.py, tools/query_fuzz_one.py): the items the four
query families are given on the renderer fuzz's scenes (test_gpu_fuzz.random_scene), the knob draw of a seed, and the checkers' answers.
Test infrastructure only; no tests in it.

An item is an rt_ray.  The ray families read it as origin / direction / tMax, the gather and visibility families as position / NORMAL /
first-cast bound or reach, so every item is given to every family.  Everything is a pure function of the seed.

The two per-lane families that came after those four draw from generators of their own (point_knobs, fuzz_points), so that what the
four are given never moves: rt_trace_hits takes the items as rays, rt_closest_points the points of fuzz_points, an rt_ray each with the
search radius in tMax."""
import numpy as np

import query_check as gc
import query_check as rc
import query_check as vc
from query_check import oracle_candidates, oracle_hits
from ray_query_helpers import load_shim, make_rays
from test_gpu_fuzz import draw_knobs, random_scene

N_ITEMS = 768
N_DEGENERATE = 8
SAMPLES = (1, 3, 4, 6, 16, 19)          # the three sample-lane layouts (1, 4, 16 lanes per item) and their ragged neighbours
FIRST_INDEX = (0, 11, 0xFFFFFF00)       # the last wraps inside a batch of 768
MAX_BOUNCES = 6                         # (CPU time of the checkers)
F32 = np.float32
INF = F32(np.inf)


def scene_shift(seed):
    """random_scene's shift of the whole scene (every eleventh seed)"""
    return F32([1e5, -2e5, 5e4]) if seed % 11 == 10 else F32([0, 0, 0])


def fuzz_scene(rtx, seed, intersect_mode=None):
    """random_scene(seed) with maxBounceCount capped and the intersectMode fuzz_knobs draws (or the one given): (params, spheres,
    triangles, meshinfo)"""
    p, sph, tris, infos = random_scene(rtx, seed)
    p["maxBounceCount"] = min(int(p["maxBounceCount"]), MAX_BOUNCES)
    p["intersectMode"] = fuzz_knobs(seed)[1]["intersectMode"] if intersect_mode is None else int(intersect_mode)
    return p, sph, tris, infos


def _unit(v):
    n = np.linalg.norm(v, axis=-1, keepdims=True)
    return (v / np.where(n > 0, n, 1)).astype(F32)


def _lattice_targets(pos, live):
    """Points that lie exactly on more than one triangle: corners and edge midpoints that two or more live axis-planar triangles share
    (the "grid" chunks' quads, the "stack" chunks' duplicates), taken from the float32 vertex data.  -> (targets (k, 3) float32, axis (k,)
    the planar axis of an owning triangle, side (k,) +-1: the side of the plane its front face looks to)"""
    targets, axes, sides = [], [], []
    seen = {}
    for ti in np.where(live)[0]:
        tri = pos[ti]
        planar = [a for a in range(3) if tri[0, a] == tri[1, a] == tri[2, a]]
        if not planar:
            continue
        n = np.cross((tri[1] - tri[0]).astype(np.float64), (tri[2] - tri[0]).astype(np.float64))
        if not n[planar[0]]:
            continue
        feats = [tri[k] for k in range(3)] + [((tri[k] + tri[(k + 1) % 3]) * F32(0.5)).astype(F32) for k in range(3)]
        for f in feats:
            key = f.tobytes()
            if key in seen:
                if seen[key] is not None:
                    targets.append(f); axes.append(planar[0]); sides.append(seen[key])
                    seen[key] = None                                  # listed once
            else:
                seen[key] = 1.0 if n[planar[0]] > 0 else -1.0
    if not targets:
        return np.zeros((0, 3), F32), np.zeros(0, np.int64), np.zeros(0)
    return np.array(targets, F32), np.array(axes), np.array(sides)


def _body(seed, scene):
    """The finite sources of a scene: its body is what lies within 1e4 units of its shift (the 3e37 triangle is finite, and not a place).
    -> (pos (nt, 3, 3) float32, live (nt,) the triangles of the body, the finite sphere centres, lo, hi, ext: the bounds of the body's
    vertices and centres and their extent, at least 1 per axis, diameter: |ext|)"""
    _, sph, tris, _ = scene
    shift = scene_shift(seed)
    pos = np.stack([tris["posA"], tris["posB"], tris["posC"]], 1).astype(F32)                       # (nt, 3, 3)
    with np.errstate(invalid="ignore"):
        live = (np.isfinite(pos) & (np.abs(pos - shift) < 1e4)).all((1, 2))
    centres = np.asarray(sph["position"], F32).reshape(-1, 3)
    centres = centres[np.isfinite(centres).all(1)]
    verts = pos[live].reshape(-1, 3)
    pool = np.concatenate([verts, centres]) if len(verts) + len(centres) else shift[None].copy()
    lo, hi = pool.min(0), pool.max(0)
    ext = np.maximum(hi - lo, F32(1))
    return pos, live, centres, lo, hi, ext, F32(np.linalg.norm(ext))


def item_split(n):
    """how n items divide: (aimed base rays — each is emitted four times, with tMax inf, dst, dst + 1 ulp and dst - 1 ulp, one third of the
    items —, surface points, special directions, the degenerate handful), in the order fuzz_items lays them out"""
    n_aim, n_surf = n // 12, n // 3
    return n_aim, n_surf, n - N_DEGENERATE - 4 * n_aim - n_surf, N_DEGENERATE


def fuzz_items(rtx, seed, n=N_ITEMS, scene=None, shim=None, parts=None):
    """RAY (n,): the items of seed `seed` for fuzz_scene(rtx, seed).  `parts` (a dict) receives the index ranges of the kinds."""
    p, sph, tris, infos = scene if scene is not None else fuzz_scene(rtx, seed)
    shim = shim or load_shim()
    mode = int(p["intersectMode"])
    rng = np.random.default_rng(5000 + seed)
    shift = scene_shift(seed)

    pos, live, centres, lo, hi, ext, diameter = _body(seed, (p, sph, tris, infos))
    live_tris = pos[live]

    def inside(k):
        return (lo - 0.25 * ext + rng.random((k, 3)) * 1.5 * ext).astype(F32)

    def targets(k):
        """points on live triangles (convex combinations of their vertices) and sphere centres"""
        out = np.empty((k, 3), F32)
        for i in range(k):
            if len(live_tris) and (not len(centres) or rng.random() < 0.85):
                w = rng.dirichlet((1, 1, 1)).astype(F32)
                out[i] = (live_tris[rng.integers(len(live_tris))] * w[:, None]).sum(0)
            elif len(centres):
                out[i] = centres[rng.integers(len(centres))]
            else:
                out[i] = inside(1)[0]
        return out

    n_aim, n_surf, n_spec, n_deg = item_split(n)

    # ---- aimed rays: lattice rays through shared edges and corners, then rays at points of triangles and at sphere centres
    lt, lax, lside = _lattice_targets(pos, live)
    n_lat = min(n_aim // 2, 4 * len(lt))
    o_lat, d_lat = np.zeros((n_lat, 3), F32), np.zeros((n_lat, 3), F32)
    for i in range(n_lat):
        k = i % len(lt) if i < len(lt) else int(rng.integers(len(lt)))
        off = rng.integers(-3, 4, 3).astype(np.float64)                      # a lattice vector, its planar component pointing to the front
        if i % 3 == 0:
            off[:] = 0                                                        # straight down the axis: u or v is exactly 0
        off[lax[k]] = lside[k] * float(rng.integers(1, 6))
        o_lat[i] = (lt[k] + off.astype(F32)).astype(F32)
        d_lat[i] = (lt[k] - o_lat[i]).astype(F32)
    n_rand = n_aim - n_lat
    tg = targets(n_rand)
    o_rand = inside(n_rand)
    aim = tg - o_rand
    half = n_rand // 2
    aim[:half] = _unit(aim[:half])                                            # (half normalised, half as they come: dst in units of |d|)
    base = make_rays(rtx, np.concatenate([o_lat, o_rand]), np.concatenate([d_lat, aim]).astype(F32))
    hit0 = oracle_hits(rtx, shim, sph, tris, infos, mode, base)
    dst = np.where(hit0["kind"] != 0, hit0["dst"], diameter).astype(F32)      # (a base ray that misses: the bound is just a bound)
    aimed = np.concatenate([base, base, base, base])
    aimed["tMax"][n_aim:2 * n_aim] = dst
    aimed["tMax"][2 * n_aim:3 * n_aim] = np.nextafter(dst, INF)
    aimed["tMax"][3 * n_aim:] = np.nextafter(dst, F32(0))

    # ---- surface points: where probe rays land, lifted off the surface along the normal, which goes in `direction`
    o = inside(n_surf)
    probe = make_rays(rtx, o, (targets(n_surf) - o).astype(F32))
    probe["origin"][: n_aim] = base["origin"]; probe["direction"][: n_aim] = base["direction"]       # ... the tie points among them
    ph = oracle_hits(rtx, shim, sph, tris, infos, mode, probe)
    surf = gc.surface_points(rtx, ph, offset=1e-3)
    miss = ph["kind"] == 0                                                    # a probe that missed: a free point with a random normal
    surf["origin"][miss] = inside(int(miss.sum()))
    surf["direction"][miss] = _unit(rng.standard_normal((int(miss.sum()), 3)))
    bad = ~np.isfinite(surf["origin"]).all(1)                                 # (a NaN normal lifts the point to NaN: keep the NaN normal only)
    surf["origin"][bad] = np.asarray(ph["hitPoint"])[bad]
    bad = ~np.isfinite(surf["origin"]).all(1)
    surf["origin"][bad] = inside(int(bad.sum()))
    surf["tMax"] = rng.choice([INF, diameter, F32(0.25) * diameter, F32(1.5)], n_surf).astype(F32)

    # ---- special directions and far origins
    o = inside(n_spec)
    d = rng.standard_normal((n_spec, 3)).astype(F32) * F32(10.0) ** rng.integers(-3, 4, (n_spec, 1)).astype(F32)   # not normalised
    q = n_spec // 6
    d[:q] = 0
    d[np.arange(q), rng.integers(0, 3, q)] = rng.choice([-1.0, 1.0, 2.5], q)                     # axis-aligned
    d[np.arange(q, 2 * q), rng.integers(0, 3, q)] = 0                                                           # one zero component
    d[np.arange(2 * q, 3 * q), rng.integers(0, 3, q)] = -0.0
    with np.errstate(all="ignore"):                                                              # ... each through a point of the geometry
        back = rng.uniform(0.5, 3.0, (3 * q, 1)) / np.linalg.norm(d[:3 * q], axis=1, keepdims=True)
        o[:3 * q] = (targets(3 * q) - d[:3 * q] * back).astype(F32)
    far = slice(3 * q, 5 * q)                                                                    # origins up to 1e3 outside the bounds, looking in
    out_dir = _unit(rng.standard_normal((2 * q, 3)))
    o[far] = (0.5 * (lo + hi) + out_dir * (0.5 * diameter + rng.uniform(1, 1e3, (2 * q, 1)))).astype(F32)
    d[far] = (targets(2 * q) - o[far]).astype(F32)
    d[5 * q:] = (targets(n_spec - 5 * q) - o[5 * q:]).astype(F32) * F32(0.37)                    # the rest: at the geometry, unnormalised
    spec = make_rays(rtx, o, d, rng.choice([INF, diameter], n_spec).astype(F32))

    # ---- the degenerate handful (fixed): not traced, or traced to nothing
    deg = make_rays(rtx, inside(n_deg), _unit(rng.standard_normal((n_deg, 3))))
    deg["origin"][0, 0] = np.nan
    deg["origin"][1, 2] = np.inf
    deg["direction"][2] = 0
    deg["tMax"][3] = 0.0
    deg["tMax"][4] = -0.0
    deg["tMax"][5] = -1.0
    deg["tMax"][6] = np.nan
    deg["direction"][7, 1] = np.nan

    items = np.concatenate([aimed, surf, spec, deg])
    assert len(items) == n
    if parts is not None:
        parts.update(aimed=(0, 4 * n_aim), base=(0, n_aim), lattice=(0, n_lat), surface=(4 * n_aim, 4 * n_aim + n_surf),
                     special=(4 * n_aim + n_surf, n - n_deg), degenerate=(n - n_deg, n))
    return items


def fuzz_knobs(seed):
    """(options, call): the context options of seed `seed` — the renderer fuzz's own draw (test_gpu_fuzz.draw_knobs on the same generator,
    so a seed builds the tree there and here with the same builder settings), of which the options queries read are kept, then the query
    options (one value in four of each leaves the context's own) — and the call's settings.  Nothing is restored: every seed gets a
    context of its own."""
    drawn = draw_knobs(np.random.default_rng(seed))
    read = ("max_leaf", "full_sort", "compact_nodes", "device_bvh", "bvh_collapse", "bvh_radius", "bvh_top", "bvh_treelets", "bvh_reinsert")
    options = {k: drawn[k] for k in read}
    rng = np.random.default_rng(9000 + seed)
    for name, values in (("lds_stack", (2, 3, 8, -1)), ("radiance_slice", (1, 7, 100, -1)), ("gather_slice", (1, 7, 100, -1)),
                         ("visibility_slice", (1, 7, 100, -1))):
        v = int(rng.choice(values))
        if v >= 0:
            options[name] = v
    call = {"samples": int(rng.choice(SAMPLES)), "first_index": int(rng.choice(FIRST_INDEX)), "seed": int(rng.integers(0, 1 << 32)),
            "intersectMode": int(rng.integers(0, 2))}
    return options, call


def fuzz_case(rtx, seed, shim=None, overrides=None):
    """Everything one seed is: (scene buffers with the drawn intersectMode and the capped maxBounceCount, items, options, call).
    `overrides`: name -> int, replacing options or call settings (tools/query_fuzz_one.py)."""
    options, call = fuzz_knobs(seed)
    for k, v in (overrides or {}).items():
        (call if k in call else options)[k] = int(v)
    p, sph, tris, infos = fuzz_scene(rtx, seed, call["intersectMode"])
    call["maxBounceCount"] = int(p["maxBounceCount"])
    scene = (p, sph, tris, infos)
    return scene, fuzz_items(rtx, seed, scene=scene, shim=shim), options, call


FAMILIES = (("radiance", None), ("gather", gc.COSINE), ("gather", gc.SH9), ("visibility", vc.COSINE), ("visibility", vc.SH9), ("visibility", vc.DISTANCE))


def checker(rtx, scene, items, call, family, mode, accel=True):
    """the CPU checker's answer for a sampled family"""
    p, sph, tris, infos = scene
    N, s, f = call["samples"], call["seed"], call["first_index"]
    if family == "radiance":
        return rc.oracle_radiance(rtx, p, sph, tris, infos, items, N, s, f, accel=accel)
    if family == "gather":
        return gc.oracle_gather(rtx, p, sph, tris, infos, items, N, s, f, mode, accel=accel)
    return vc.oracle_visibility(rtx, sph, tris, infos, items, N, s, f, mode, intersect=int(p["intersectMode"]), accel=accel)


def run_family(t, items, call, family, mode):
    """the same call on a Tracer or MultiTracer (items: a RAY array, or a tensor for the device entry)"""
    N, s, f = call["samples"], call["seed"], call["first_index"]
    if family == "radiance":
        return t.trace_radiance(items, N, s, f)
    if family == "gather":
        return t.gather(items, N, s, f, mode)
    return t.visibility(items, N, s, f, mode)


def load_scene(t, scene, options):
    """options, params and the world-space buffers into a fresh Tracer or MultiTracer — what test_gpu_ray_query.loaded_tracer does for a
    scene manager, here for random_scene's raw buffers and for both kinds of handle"""
    for k, v in options.items():
        t.set_option(k, v)
    p, sph, tris, infos = scene
    t.set_params(p)
    t.upload(spheres=sph, triangles=tris, meshinfo=infos)


def describe(items, i):
    r = items[int(i)]
    return f"item {int(i)}: origin {r['origin'].tolist()} direction {r['direction'].tolist()} tMax {float(r['tMax'])!r}"


def power_counts(rtx, scene, items, shim=None):
    """What the ray-query checker finds among the items: traced (tMax > 0), hits, misses, hits with a second candidate at the bit-identical
    dst (brute force over the scene under the checker's acceptance rule), and flips: aimed rays that miss at tMax = dst (and one ulp
    below it) and hit one ulp above it"""
    shim = shim or load_shim()
    p, sph, tris, infos = scene
    mode = int(p["intersectMode"])
    hits = oracle_hits(rtx, shim, sph, tris, infos, mode, items)
    cand = oracle_candidates(rtx, shim, sph, tris, infos, mode, items)
    with np.errstate(invalid="ignore"):
        traced = items["tMax"] > 0
    hit = hits["kind"] != 0
    k = item_split(len(items))[0]
    base, at, above, below = (hit[j * k:(j + 1) * k] for j in range(4))
    return {"traced": int(traced.sum()), "hits": int((hit & traced).sum()), "misses": int((~hit & traced).sum()),
            "ties": int((cand >= 2).sum()), "flips": int((base & ~at & above & ~below).sum())}


def inputs_table(rtx, seeds=range(24)):
    """the text of profiles/query_fuzz_inputs.txt: what power_counts finds per seed"""
    rows, total = [], {}
    for seed in seeds:
        scene, items, options, call = fuzz_case(rtx, seed)
        c = power_counts(rtx, scene, items)
        rows.append(f"{seed:4d} {len(scene[2]):5d} {len(scene[3]):6d} {len(scene[1]):7d} {int(scene[0]['intersectMode']):4d} {c['traced']:6d} {c['hits']:5d} {c['misses']:6d} "
                    f"{c['ties']:5d} {c['flips']:5d}")
        for k, v in c.items():
            total[k] = total.get(k, 0) + v
    head = "seed  tris chunks spheres mode traced  hits misses  ties flips"
    return "\n".join([head, *rows, f"sum  {'':25s} {total['traced']:6d} {total['hits']:5d} {total['misses']:6d} {total['ties']:5d} {total['flips']:5d}"]) + "\n"


# ---- the two per-lane families that came after the four: rt_trace_hits (the items as rays) and rt_closest_points (points of their own) ----
HIT_K = (1, 2, 3, 8)
POINT_RADII = (INF, None, None, F32(1.5), F32(3e20), F32(1e-30))     # None: the scene's diameter, a quarter of it; R * R is +inf for 3e20, 0 for 1e-30


def point_knobs(seed):
    """(options, form): the two families' slice options (one value in four of each leaves the context's own) and the multi-hit call's
    form, from a generator of their own: fuzz_knobs' draw stays what it was"""
    rng = np.random.default_rng(13000 + seed)
    options = {}
    for name in ("hits_slice", "closest_slice"):
        v = int(rng.choice((1, 7, 100, -1)))
        if v >= 0:
            options[name] = v
    return options, {"K": int(rng.choice(HIT_K)), "both_sides": int(rng.integers(0, 2)), "count_all": int(rng.integers(0, 2))}


def point_split(n):
    """how n points divide: (free points, points on the surface, radius-flip base points — each is emitted three times, with R = dst,
    dst + 1 ulp and dst - 1 ulp —, far points, the degenerate handful), in the order fuzz_points lays them out"""
    n_flip, n_surf, n_far = n // 12, n // 3, n // 12
    return n - n_surf - 3 * n_flip - n_far - N_DEGENERATE, n_surf, n_flip, n_far, N_DEGENERATE


def fuzz_points(rtx, seed, scene, items, shim=None, parts=None):
    """RAY (len(items),): the points of seed `seed` for rt_closest_points, the search radius in tMax (direction stays zero: it is not
    read).  `parts` (a dict) receives the index ranges of the kinds.  Points on the surface are float32 values taken from the data, so
    that their distance is exactly 0 and every primitive that owns them ties."""
    import closest_check as cc
    shim = shim or load_shim()
    p, sph, tris, infos = scene
    n = len(items)
    rng = np.random.default_rng(17000 + seed)
    pos, live, centres, lo, hi, ext, diameter = _body(seed, scene)
    n_free, n_surf, n_flip, n_far, n_deg = point_split(n)
    body = items[:n - n_deg]

    def radii(k, values):
        r = [values[j] for j in rng.integers(0, len(values), k)]
        return F32([diameter if v is None else v for v in r])

    def closest_dst(xyz):
        return cc.oracle_closest(rtx, sph, tris, infos, cc.points_of(rtx, xyz))["dst"]

    # ---- free points: origins of the items (one of each aimed base ray's four copies)
    n_aim = item_split(n)[0]
    pick = rng.permutation(np.concatenate([np.arange(n_aim), np.arange(4 * n_aim, n - n_deg)]))[:n_free]
    free_values = list(POINT_RADII)
    free_values[1], free_values[2] = diameter, F32(0.25) * diameter
    free = cc.points_of(rtx, body["origin"][pick], radii(n_free, free_values))

    # ---- points exactly on the surface
    verts = pos[live]                                                           # (k, 3, 3)
    seen, stacked = {}, []
    for tri in verts:                                                           # a triangle uploaded three times: a "stack" chunk's
        c = seen[tri.tobytes()] = seen.get(tri.tobytes(), 0) + 1
        if c == 3:
            stacked.append(tri)
    lt = _lattice_targets(pos, live)[0]
    # (where the items land as rays: the aimed base rays are the first probe rays of fuzz_items, the surface items sit 1e-3 above the rest)
    hit = oracle_hits(rtx, shim, sph, tris, infos, int(p["intersectMode"]), body)
    landed = np.asarray(hit["hitPoint"], F32)[(hit["kind"] != 0) & np.isfinite(hit["hitPoint"]).all(1)]
    zero = np.asarray(sph["position"], F32).reshape(-1, 3)[np.asarray(sph["radius"]) == 0]
    n_centres = len(centres) + len(zero)
    n_lat, n_stack = min(len(lt), n_surf // 4), min(3 * len(stacked), n_surf // 8)
    n_vert = (n_surf // 4 if len(verts) else 0)
    n_land = n_surf - n_centres - n_lat - n_stack - n_vert
    fill = verts.reshape(-1, 3) if len(verts) else scene_shift(seed)[None]
    some = [lt[:n_lat], np.array(stacked, F32).reshape(-1, 3)[:n_stack], fill[rng.integers(0, len(fill), n_vert)],
            landed[rng.permutation(len(landed))[:n_land]]]
    short = n_land - len(some[-1])                                               # (fewer probe hits than room: more vertices)
    some.append(fill[rng.integers(0, len(fill), short)])
    r_some = radii(n_surf - n_centres, (INF, INF, INF, diameter, F32(1.5), F32(1e-30)))
    surf = cc.points_of(rtx, np.concatenate([*some, centres, zero]).astype(F32),
                        np.concatenate([r_some, np.full(len(centres), INF), np.full(len(zero), F32(1.5))]).astype(F32))
    assert len(surf) == n_surf

    # ---- radius flips: the checker's dst of a point at R = inf, and the point with R = dst and one ulp either side of it
    base = body["origin"][rng.permutation(n - n_deg)[:n_flip]]
    dst = closest_dst(base)
    flips = cc.points_of(rtx, np.concatenate([base, base, base]), np.concatenate([dst, np.nextafter(dst, INF), np.nextafter(dst, F32(0))]))

    # ---- far points: up to 1e3 outside the bounds, unbounded and with a radius just short of the scene
    out_dir = _unit(rng.standard_normal((n_far, 3)))
    far_xyz = (0.5 * (lo + hi) + out_dir * (0.5 * diameter + rng.uniform(1, 1e3, (n_far, 1)))).astype(F32)
    r_far = np.full(n_far, INF)
    r_far[n_far // 2:] = closest_dst(far_xyz[n_far // 2:]) * F32(0.999)
    far = cc.points_of(rtx, far_xyz, r_far)

    # ---- the degenerate handful of the items, as it is: a NaN and an infinite coordinate, R of 0, -0, -1 and NaN
    deg = cc.points_of(rtx, items["origin"][n - n_deg:], items["tMax"][n - n_deg:])

    points = np.concatenate([free, surf, flips, far, deg])
    assert len(points) == n
    if parts is not None:
        a, b, c, d = n_free, n_free + n_surf, n_free + n_surf + 3 * n_flip, n - n_deg
        parts.update(free=(0, a), surface=(a, b), lattice=(a, a + n_lat), stacked=(a + n_lat, a + n_lat + n_stack), flips=(b, c),
                     flip_base=(b, b + n_flip), far=(c, d), degenerate=(d, n))
    return points


def run_hits(t, items, form):
    """rt_trace_hits in the drawn form on a Tracer or MultiTracer (items: a RAY array, or a tensor for the device entry)"""
    return t.trace_hits(items, form["K"], bool(form["both_sides"]), bool(form["count_all"]))


def check_hits(rtx, scene, items, form):
    """the multi-hit checker's answer for a form, at the scene's intersect mode"""
    import hits_check as hc
    p, sph, tris, infos = scene
    return hc.oracle_hits(rtx, sph, tris, infos, items, form["K"], hc.BOTH if form["both_sides"] else hc.FRONT, bool(form["count_all"]),
                          int(p["intersectMode"]))


DEEP = {"K": 8, "both_sides": 1, "count_all": 1}         # the form every seed also runs: the whole list, evictions included


def point_power_counts(rtx, scene, items, points, shim=None):
    """What the two checkers find.  Points: searched (R > 0), found, missed, tied (two or more candidates at the winner's key), at
    distance exactly 0, flips (a base point found at R = dst + 1 ulp and not at dst - 1 ulp), and the largest tie.  Rays (two-sided,
    countAll, the scene's intersect mode): rays with two or more hits, with more than eight, the largest count, and closest hits of the
    ray-query checker without a second candidate at their dst."""
    import closest_check as cc
    shim = shim or load_shim()
    p, sph, tris, infos = scene
    at_best = np.zeros(len(points), np.int32)
    got = cc.oracle_closest(rtx, sph, tris, infos, points, at_best=at_best)
    with np.errstate(invalid="ignore"):
        searched = points["tMax"] > 0
    found = got["kind"] != 0
    n_free, n_surf, n_flip = point_split(len(points))[:3]
    b = n_free + n_surf
    above, below = found[b + n_flip:b + 2 * n_flip], found[b + 2 * n_flip:b + 3 * n_flip]
    count = check_hits(rtx, scene, items, DEEP)[:, 0]["hitCount"]
    mode = int(p["intersectMode"])
    first, cand = oracle_hits(rtx, shim, sph, tris, infos, mode, items), oracle_candidates(rtx, shim, sph, tris, infos, mode, items)
    return {"searched": int(searched.sum()), "found": int(found.sum()), "missed": int((searched & ~found).sum()), "tied": int((at_best >= 2).sum()),
            "zero": int((found & (got["dst"] == 0)).sum()), "flips": int((above & ~below).sum()), "widest": int(at_best.max()),
            "two": int((count >= 2).sum()), "deep": int((count > 8).sum()), "most": int(count.max()),
            "untied": int(((first["kind"] != 0) & (cand < 2)).sum())}


POINT_COLUMNS = ("searched", "found", "missed", "tied", "zero", "flips", "widest", "two", "deep", "most", "untied")


def points_table(rtx, seeds=range(24)):
    """the text of profiles/query_fuzz_points.txt: what point_power_counts finds per seed"""
    rows = []
    for seed in seeds:
        scene, items, _, _ = fuzz_case(rtx, seed)
        c = point_power_counts(rtx, scene, items, fuzz_points(rtx, seed, scene, items))
        rows.append(f"{seed:4d} " + " ".join(f"{c[k]:8d}" for k in POINT_COLUMNS))
    return "\n".join(["seed " + " ".join(f"{k:>8s}" for k in POINT_COLUMNS), *rows]) + "\n"


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import rtx_pkg
    # `python tests/query_fuzz.py` prints profiles/query_fuzz_inputs.txt, `python tests/query_fuzz.py points` profiles/query_fuzz_points.txt
    print((points_table if sys.argv[1:] == ["points"] else inputs_table)(rtx_pkg.load()), end="")
