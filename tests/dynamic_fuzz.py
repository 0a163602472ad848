"""Scenes that change under a live context: one generator for tests/test_dynamic_fuzz_cpu.py, tests/test_gpu_dynamic_fuzz.py and
tools/dynamic_fuzz_one.py.  Test infrastructure only (numpy).

    case = dynamic_case(rtx, seed)         # (params, spheres, local_tris, chunks, n_meshes, steps), a function of the seed alone
    tris, infos = expected_world(case, k)  # the world-space scene after step k

The geometry is tests/test_gpu_fuzz.py random_scene's triangle buffer — slivers, stacks, NaN, infinite and 1e38-sized triangles — taken
as LOCAL triangles; each of its chunks is one local chunk of mesh `chunk % n_meshes`.  A step names one of the three doors a scene can
come through, or moves the camera:

    transforms  rt_upload_local_meshes + rt_set_mesh_transforms: a pose per mesh (POSE_CLASSES)
    deform      option device_geometry: the current world triangles are resident, then change in place (DEFORM_CLASSES; every class but
                the no-op is applied to the triangles the door was entered with, so a NaN corner or a 1e37 corner is gone the step after)
    reupload    rt_upload_triangles of the current world triangles from host memory, with a device_bvh of -1, 0 or 1 and 0, 1 or 20
                frames traced before the next step (the 16-frame rule of the automatic builder choice, both ways)
    camera      the camera 1e3 or 1e6 away for this step's frames and queries; the next step has it back

expected_world restates RayTracedMesh.cs:56-94 from the reference's text: rot * Scale(p, scale) + pos through host.quat_rotate, and the
chunk box as the loop the reference runs — start at the first world A, then A, B, C of every triangle through a < b ? a : b and
a > b ? a : b.  It is the one definition host.py, the compiled host and k_chunk_bounds are held to."""
import numpy as np

from device_geometry_helpers import displaced
from test_gpu_fuzz import draw_knobs, random_scene

f32 = np.float32
DOORS = ("transforms", "deform", "reupload")
POSE_CLASSES = ("random", "norm_half", "norm_sqrt2", "norm_3", "zero_quat", "nan", "scale_zero", "scale_negative", "scale_tiny_huge",
                "far_1e5", "far_1e30", "spread", "return")
DEFORM_CLASSES = ("displaced", "permuted", "nan_corner", "collapsed", "huge", "infinite", "normals_zero", "noop")
# what follows the first pose, by seed % 6: every third seed goes through all three doors, every seed through two, and twelve
# consecutive seeds take each of the six ordered door changes at least twice (tests/test_dynamic_fuzz_cpu.py counts them)
PLANS = (("deform", "deform", "reupload", "transforms", "transforms"),
         ("transforms", "deform", "deform", "transforms", "deform"),
         ("reupload", "transforms", "transforms", "reupload", "transforms"),
         ("reupload", "deform", "deform", "transforms", "transforms"),
         ("transforms", "reupload", "reupload", "deform", "deform"),
         ("deform", "transforms", "reupload", "reupload", "transforms"))
POSE_STRIDE, DEFORM_STRIDE = (1, 7, 7), (1, 2, 1)      # class of a seed's k-th step of the kind: (a * seed + b * k + c) % the number of classes


class Case(tuple):
    """(params, spheres, local_tris, chunks, n_meshes, steps) and, beside them, what a run of the seed draws: knobs (draw_knobs),
    kernel, seed, rtx"""


def _pose(rng, seed, i):
    """bvh_audit.random_pose's pose for mesh i"""
    q = rng.normal(size=4)
    q = q / np.linalg.norm(q) * (1.0001 if i == 1 else 1.0)
    s = 10.0 ** rng.uniform(-1.5, 0.8, 3) * rng.choice([1, 1, 1, -1], 3)
    if i == 2 and seed % 3 == 0:
        s[int(rng.integers(0, 3))] = 0.0
    big = 1e3 if seed % 4 == 3 else 6.0
    return rng.uniform(-big, big, 3), q, s


def _poses(rtx, rng, seed, n):
    xf = np.zeros(n, rtx._cabi.MESH_TRANSFORM)
    for i in range(n):
        xf[i]["position"], xf[i]["rotation"], xf[i]["lossyScale"] = _pose(rng, seed, i)
    return xf


def _classed_pose(rtx, rng, seed, kind, current, first):
    """the poses of a `transforms` step of class `kind`: one mesh (all of them for spread / return / random) leaves `current`"""
    n = len(current)
    xf = current.copy()
    j = int(rng.integers(0, n))
    if kind == "random":
        return _poses(rtx, rng, seed, n)
    if kind == "return":
        return first.copy()
    if kind == "spread":
        xf["position"] = (current["position"] * f32(50)).astype(f32)
        return xf
    q = xf[j]["rotation"].astype(np.float64)
    unit = q / np.linalg.norm(q) if np.isfinite(q).all() and np.linalg.norm(q) > 0 else np.array([0.0, 0.0, 0.0, 1.0])
    if kind in ("norm_half", "norm_sqrt2", "norm_3"):
        xf[j]["rotation"] = unit * {"norm_half": 0.5, "norm_sqrt2": np.sqrt(2.0), "norm_3": 3.0}[kind]
    elif kind == "zero_quat":
        xf[j]["rotation"] = 0.0
    elif kind == "nan":
        field = ("position", "rotation", "lossyScale")[int(rng.integers(0, 3))]
        v = xf[j][field].copy(); v[int(rng.integers(0, len(v)))] = np.nan; xf[j][field] = v
    elif kind == "scale_zero":
        s = xf[j]["lossyScale"].copy(); s[rng.permutation(3)[:int(rng.integers(1, 4))]] = 0.0; xf[j]["lossyScale"] = s
    elif kind == "scale_negative":
        xf[j]["lossyScale"] = -np.abs(xf[j]["lossyScale"]) * f32(rng.uniform(0.5, 2.0))
    elif kind == "scale_tiny_huge":
        xf[j]["lossyScale"] = rng.choice([1e-20, 1e18], 3)
    elif kind == "far_1e5":
        xf[j]["position"] = rng.choice([-1e5, 1e5], 3)
    elif kind == "far_1e30":
        xf[j]["position"] = rng.choice([-1e30, 1e30], 3)
    else:
        raise ValueError(kind)
    return xf


def dynamic_case(rtx, seed):
    params, spheres, tris, infos = random_scene(rtx, seed)
    params = params.copy()
    params["width"], params["height"] = min(int(params["width"]), 32), min(int(params["height"]), 24)
    params["numRaysPerPixel"] = min(int(params["numRaysPerPixel"]), 2)
    params["maxBounceCount"] = min(int(params["maxBounceCount"]), 3)
    rng = np.random.default_rng(7000 + seed)
    n_meshes = int(rng.integers(1, 5))
    # every fourth seed is a benign one: random_scene gives seed % 4 == 3 finite triangles only, and here it gets two meshes or more, finite
    # poses and the device builder, so that the tree's area and the padding are finite numbers the steps can cross: a spread of the
    # standing meshes (the local door's area rule), resident triangles that change places across them (the deform door's), and the camera 1e6
    # away while the scene stands in a world-space door (repad_boxes).  tests/test_gpu_dynamic_fuzz.py counts them.
    benign = seed % 4 == 3
    if benign:
        n_meshes = max(n_meshes, 2)
    # one local chunk per chunk of the scene, in list order; the local door refuses a triangle no chunk addresses, and random_scene's
    # chunks tile its buffer
    chunks = np.zeros(len(infos), rtx._cabi.LOCAL_CHUNK)
    chunks["firstTriangleIndex"], chunks["numTriangles"] = infos["firstTriangleIndex"], infos["numTriangles"]
    chunks["meshIndex"] = np.arange(len(infos)) % n_meshes
    chunks["material"] = infos["material"]
    assert int(chunks["numTriangles"].sum()) == len(tris)
    first = _poses(rtx, rng, seed, n_meshes)
    steps = [{"door": "transforms", "kind": "random", "xf": first}]
    doors = list(PLANS[seed % 6])
    for _ in range(int(rng.integers(0, 2))):                   # 6 or 7 steps: camera moves and further poses go in between
        doors.insert(int(rng.integers(0, len(doors) + 1)), str(rng.choice(["camera", "camera", "transforms"])))
    if benign:                                                 # (7 steps) the camera leaves right after the first world-space step
        doors = list(PLANS[seed % 6])
        doors.insert(1 + min(doors.index(d) for d in ("deform", "reupload") if d in doors), "camera")
    current, n_pose, n_deform, n_camera, stood = first, 0, 0, 0, "transforms"
    world = [d for d in doors if d != "camera"]
    standing_poses = [1 + i for i, d in enumerate(doors) if d == "transforms" and (["transforms"] + world)[len([x for x in doors[:i] if x != "camera"])] == "transforms"]
    spread_at = standing_poses[0] if benign and standing_poses else None     # the step index of the first pose on a standing local tree
    for door in doors:
        standing, stood = door == stood, stood if door == "camera" else door
        if door == "transforms":
            a, b, c = POSE_STRIDE
            kind = POSE_CLASSES[1 + (a * seed + b * n_pose + c) % (len(POSE_CLASSES) - 1)]       # ("random" is every first pose)
            if benign and spread_at is not None and len(steps) <= spread_at:     # finite poses until the spread has happened
                kind = "spread" if len(steps) == spread_at else "return"
            n_pose += 1
            current = _classed_pose(rtx, rng, seed, kind, current, first)
            steps.append({"door": door, "kind": kind, "xf": current})
        elif door == "deform":
            a, b, c = DEFORM_STRIDE
            kind = DEFORM_CLASSES[(a * seed + b * n_deform + c) % len(DEFORM_CLASSES)]
            if benign:
                # (permuted: triangles change places across meshes that stand far apart, so every leaf spans the scene; the area sum
                # leaves out boxes whose area is not finite, so 1e37 corners shrink it)
                kind = "displaced" if not standing else "huge" if "permuted" in [s["kind"] for s in steps] else "permuted"
            n_deform += 1
            steps.append({"door": door, "kind": kind, "draw": int(rng.integers(0, 1 << 30))})
        elif door == "reupload":
            again = steps[-1]["door"] == "reupload"              # the second of two re-uploads in a row leaves the builder to the 16-frame rule
            steps.append({"door": door, "kind": "reupload", "device_bvh": -1 if again else int(rng.choice([-1, -1, 0, 1])), "frames": int(rng.choice([0, 1, 20]))})
            if benign and steps[-1]["device_bvh"] == 0:        # (the option stays set: 0 would switch the local door's area rule off)
                steps[-1]["device_bvh"] = -1
        else:
            kind = "far_1e6" if benign else ("far_1e3", "far_1e6")[(seed + n_camera) % 2]; n_camera += 1
            steps.append({"door": door, "kind": kind, "axis": int(rng.integers(0, 3))})
    case = Case((params, spheres, tris, chunks, n_meshes, steps))
    case.rtx, case.seed, case.knobs, case.kernel = rtx, seed, draw_knobs(np.random.default_rng(seed)), (0, 1, 1, 0)[seed % 4]
    if benign:
        case.knobs["device_bvh"] = 1
    return case


# ---- the reference's marshal, from its text ----------------------------------------------------------------------------------------

def box_rule(points):
    """RayTracedMesh.cs:60-80 for the world points [A0, B0, C0, A1, ...] of one chunk (float32 [n, 3]) -> (boundsMin, boundsMax):
    boundsMin = boundsMax = the first A, then Vector3.Min / Max with every point in order — Mathf.Min(a, b) read as a < b ? a : b and
    Mathf.Max as a > b ? a : b, per component.  Literally the loop."""
    pts = np.asarray(points, f32).reshape(-1, 3)
    lo, hi = [pts[0, a] for a in range(3)], [pts[0, a] for a in range(3)]
    for p in pts:
        for a in range(3):
            lo[a] = lo[a] if lo[a] < p[a] else p[a]
            hi[a] = hi[a] if hi[a] > p[a] else p[a]
    return np.array(lo, f32), np.array(hi, f32)


def bounds_round_trip(lo, hi):
    """new Bounds((min + max) / 2, max - min) read back as MeshInfo does: bounds.min / max = centre -/+ size * 0.5 (:82, MeshInfo.cs:16-17)"""
    with np.errstate(all="ignore"):
        centre, size = ((lo + hi) / f32(2)).astype(f32), (hi - lo).astype(f32)
        return (centre - size * f32(0.5)).astype(f32), (centre + size * f32(0.5)).astype(f32)


def world_from_local(rtx, local_tris, chunks, xf):
    """UpdateWorldChunkFromLocal for every chunk -> (world triangles, meshinfo)"""
    quat_rotate = rtx.host.quat_rotate
    tris = np.zeros(len(local_tris), rtx.TRIANGLE)
    infos = np.zeros(len(chunks), rtx.MESHINFO)
    with np.errstate(all="ignore"):
        for m, ch in enumerate(chunks):
            a, n = int(ch["firstTriangleIndex"]), int(ch["numTriangles"])
            t = xf[int(ch["meshIndex"])]
            pos, rot, scale = np.asarray(t["position"], f32), np.asarray(t["rotation"], f32), np.asarray(t["lossyScale"], f32)
            lt, wt = local_tris[a:a + n], tris[a:a + n]
            for k in ("posA", "posB", "posC"):
                wt[k] = (quat_rotate(rot, (lt[k] * scale[None, :]).astype(f32)) + pos[None, :]).astype(f32)
            for k in ("normalA", "normalB", "normalC"):
                wt[k] = quat_rotate(rot, lt[k])
            infos[m]["firstTriangleIndex"], infos[m]["numTriangles"], infos[m]["material"] = a, n, ch["material"]
            if n:
                lo, hi = box_rule(np.stack([wt["posA"], wt["posB"], wt["posC"]], 1))
                infos[m]["boundsMin"], infos[m]["boundsMax"] = bounds_round_trip(lo, hi)
    return tris, infos


def deformed(base, current, kind, draw):
    """the resident triangles after a `deform` step of class `kind` (base: the triangles the door was entered with)"""
    rng = np.random.default_rng(draw)
    n = len(base)
    if kind == "noop":
        return current.copy()
    out = base.copy()
    if kind == "displaced":
        with np.errstate(all="ignore"):
            return displaced(base, 1 + draw % 5)
    if kind == "permuted":
        perm = rng.permutation(n)
        for k in ("posA", "posB", "posC"):
            out[k] = base[k][perm]
    elif kind == "nan_corner":
        v = out[("posA", "posB", "posC")[int(rng.integers(0, 3))]]
        v[int(rng.integers(0, n)), int(rng.integers(0, 3))] = np.nan
    elif kind == "collapsed":
        for k in ("posB", "posC"):
            out[k] = base["posA"]
    elif kind == "huge":
        i = rng.choice(n, min(n, 3), replace=False)
        out["posB"][i] = f32(1e37) * rng.choice([-1.0, 1.0], (len(i), 3)).astype(f32)
    elif kind == "infinite":
        i = rng.choice(n, min(n, 3), replace=False)
        out["posC"][i, int(rng.integers(0, 3))] = rng.choice([-np.inf, np.inf], len(i))
    elif kind == "normals_zero":
        for k in ("normalA", "normalB", "normalC"):
            out[k] = 0.0
    else:
        raise ValueError(kind)
    return out


def far_camera(params, kind, axis):
    """the step's params with the camera 1e3 / 1e6 further out along `axis`"""
    p = params.copy()
    pos = np.asarray(p["worldSpaceCameraPos"], f32).copy()
    pos[axis] += f32(1e3 if kind == "far_1e3" else 1e6)
    p["worldSpaceCameraPos"] = pos
    m = p["camLocalToWorld"].copy(); m[3], m[7], m[11] = pos; p["camLocalToWorld"] = m
    return p


def replay(case, upto=None):
    """the scene after each step 0..upto: a list of dicts — door (the door the scene stands in: a camera step keeps it), step, tris,
    infos, params (this step's), base (deform door: the triangles it was entered with), entered (the step came through another door
    than the scene stood in)"""
    params, spheres, local, chunks, n_meshes, steps = case
    rtx = case.rtx
    out, door, tris, infos, base = [], None, None, None, None
    for i, st in enumerate(steps[:None if upto is None else upto + 1]):
        p, entered = params, False
        if st["door"] == "camera":
            p = far_camera(params, st["kind"], st["axis"])
        else:
            entered, door = door != st["door"], st["door"]
            if door == "transforms":
                tris, infos = world_from_local(rtx, local, chunks, st["xf"])
            elif door == "deform":
                if entered:
                    base = tris.copy()
                tris = deformed(base, tris, st["kind"], st["draw"])
        out.append({"door": door, "step": st, "tris": tris.copy(), "infos": infos.copy(), "params": p, "base": None if base is None else base.copy(),
                    "entered": entered, "index": i})
    return out


def expected_world(case, upto):
    """the world (triangles, meshinfo) after step `upto`"""
    s = replay(case, upto)[-1]
    return s["tris"], s["infos"]


def manager_for(case, xf):
    """host.py's RayTracingManager holding the case's local chunks in the poses `xf` (its marshal is what expected_world is compared with)"""
    params, spheres, local, chunks, n_meshes, steps = case
    h = case.rtx.host
    cam = h.Camera(h.Transform())
    mgr = h.RayTracingManager(cam, width=int(params["width"]), height=int(params["height"]))
    by_mesh = {}
    for ch in chunks:                                  # (host.py lists a mesh's chunks together: compare per chunk, by range)
        by_mesh.setdefault(int(ch["meshIndex"]), []).append(ch)
    for m in range(n_meshes):
        lc = [h.MeshChunk(local[int(c["firstTriangleIndex"]):int(c["firstTriangleIndex"]) + int(c["numTriangles"])].copy(), h.Bounds(np.zeros(3, f32), np.zeros(3, f32)), 0)
              for c in by_mesh.get(m, [])]
        t = h.Transform(position=xf[m]["position"], rotation=xf[m]["rotation"], lossyScale=xf[m]["lossyScale"])
        mgr.meshes.append(h.RayTracedMesh(t, [h.RayTracingMaterial()], localChunks=lc, enforceTriangleLimit=False))
    return mgr, by_mesh


# ---- the static scene with NaN chunk boxes ----------------------------------------------------------------------------------------

def nan_box_scene(rtx):
    """the mesh-test scene's chunks with a NaN boundsMin component on one chunk, a NaN boundsMax component on another and an all-NaN box
    on a third: (params, spheres, triangles, meshinfo) at 32 x 24, FLAT_CHUNKS (RayBoundingBox :177-187 decides what a NaN face lets through)"""
    m = rtx.scenes.mesh_test_scene(32, 24)
    m.numRaysPerPixel, m.maxBounceCount = 2, 3
    params, spheres, tris, infos = m.build_buffers()
    infos = infos.copy()
    params = params.copy(); params["intersectMode"] = rtx._cabi.RT_INTERSECT_FLAT_CHUNKS
    big = np.argsort(-infos["numTriangles"])
    lo = infos["boundsMin"].copy(); hi = infos["boundsMax"].copy()
    lo[big[0], 1] = np.nan
    hi[big[1], 0] = np.nan
    lo[big[2]] = np.nan; hi[big[2]] = np.nan
    infos["boundsMin"], infos["boundsMax"] = lo, hi
    return params, spheres, tris, infos


# ---- a case on a context ------------------------------------------------------------------------------------------------------------

STAT_KEYS = ("bvhBuilds", "bvhRebuilds", "bvhRepads", "primaryListBuilds", "bvhBuiltOnDevice", "numBvhNodes", "refitAreaRatio", "bvhInternalArea", "bvhMaxStack")
REBUILD_PERCENT = 200      # rt_set_option("rebuild_percent")'s default, which the cases keep


def apply_step(t, mem, case, s, frame=0):
    """bring the context `t` (a Tracer or a MultiTracer) to the scene after step `s` (an entry of replay(case)); mem: a
    device_geometry_helpers.DeviceMemory for the resident triangles.  A door the scene did not stand in is entered first — the deform
    door by making the triangles it was entered with resident and tracing one frame of them, so that the step itself is an update."""
    params, spheres, local, chunks, n_meshes, steps = case
    st = s["step"]
    t.set_params(s["params"])
    if st["door"] == "transforms":
        if s["entered"]:
            t.upload(spheres=spheres)
            t.upload_local_meshes(local, chunks, n_meshes)
        t.set_mesh_transforms(st["xf"])
    elif st["door"] == "deform":
        if s["entered"]:
            t.upload(spheres=spheres, meshinfo=s["infos"])
            t.upload_triangles_device(*mem.put(s["base"]))
            t.render(frame, 1)
        t.upload_triangles_device(*mem.put(s["tris"]))
    elif st["door"] == "reupload":
        t.set_option("device_bvh", st["device_bvh"])
        t.upload(spheres=spheres, triangles=s["tris"], meshinfo=s["infos"])


def after_step(t, s, frame=0):
    """what a reupload step traces before the next step: 0, 1 or 20 frames"""
    if s["step"]["door"] == "reupload" and s["step"]["frames"]:
        t.render(frame, s["step"]["frames"])


def far_rays(rtx, s):
    """four rays from 1e5 away at the scene's finite middle (a camera step's queries: the padding has to follow the origins)"""
    from ray_query_helpers import make_rays
    p = np.concatenate([s["tris"]["posA"], s["tris"]["posB"], s["tris"]["posC"]]).astype(np.float64)
    with np.errstate(all="ignore"):
        p = p[np.isfinite(p).all(1) & (np.abs(p) < 1e4).all(1)]
    centre = (p.mean(0) if len(p) else np.zeros(3)).astype(f32)
    o = centre[None] + f32([[0, 1e5, 0], [1e5, 0, 0], [0, 0, -1e5], [3e4, 3e4, 3e4]])
    return make_rays(rtx, o, centre[None] - o)
