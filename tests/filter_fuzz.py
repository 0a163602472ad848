"""What the image-chain fuzz shares (tests/test_filter_fuzz_cpu.py, tests/test_gpu_filter_fuzz.py, tools/filter_fuzz_one.py): the renderer
fuzz's scenes (test_gpu_fuzz.random_scene) extended by elements that are hostile to the image filters, the camera poses of a temporal
sequence, the knob draw of a seed, the stages one seed runs on a context, and what the CPU checkers find in the inputs.  Test
infrastructure only; no tests in it.  Everything is a pure function of the seed.

The feature planes can only come out of a scene (there is no call that writes them), so the hostile guides are made by geometry:
vertex normals that normalise to NaN, to an infinity or to 0, a sphere 1e15 .. 4e18 units away, a sphere half a millimetre from the
camera, materials whose colour is 0, negative, 1e30, infinite or NaN, invisible lights in front of and coincident with ordinary
quads, a sliver a few hundredths of a pixel wide.

Two rules of the filters' arithmetic bound what a seed may hold if its output is to say anything (DESIGN.md "Image-chain fuzz"):
  - a pixel that is NaN in e_i makes every pixel whose tap reads it NaN in e_{i+1} (NaN + x = NaN in the exponent), so after k passes
    one NaN pixel has spread over reach(k) = 2 * (2^k - 1) pixels in each direction, the whole 64 x 48 image for k >= 5.  The elements
    that make a NaN (nan_ok) are therefore confined to the image's corner (0, 0) and drawn only on the seeds whose iteration counts
    leave more than half of the image out of reach; the other seeds get the finite extremes of the same elements.
  - a sigma of 1e-25 squares to 0, its constant is 1 / 0 = inf, and the centre tap's difference is exactly 0: 0 * inf = NaN on every
    pixel.  That call cannot leave a finite pixel, so a seed's first call draws its squared sigmas from the other four values and the
    seeds that draw 1e-25 make a second call with it ("underflow"), compared like every other call."""
import numpy as np

import aov_check
import denoise_check
import query_check
import temporal_check
import vdenoise_check
from test_gpu_fuzz import draw_knobs, random_scene

F32 = np.float32
NAN, INF = F32(np.nan), F32(np.inf)
SAMPLES = (1, 3, 4, 16, 20, 64)                  # the three sample-lane layouts (1, 4, 16 lanes per pixel) and their ragged neighbours
NORMALS = (NAN, INF, -INF, F32(1e30), F32(3e38), F32(1e-42), F32(0.0))      # vertex normals: normalize gives NaN, 0 (1e30: the dot overflows) or inf (1e-42: it underflows)
NORMALS_FINITE = (F32(1e30),)                    # ... the one that leaves a finite guide: the zero normal
ALBEDOS = (F32(0.0), F32(-1.0), F32(1e30), INF, NAN)
ALBEDOS_FINITE = ALBEDOS[:3]
SIGMA_UNDERFLOW, SIGMA_OVERFLOW = 1e-25, 1e25    # the square is 0: the constant is inf; the square is inf: the constant is 0
MAX_HISTORY = (1, 2, 32, 4096)
TOLERANCES = (1e-30, None, 1e30)                 # None: the header's default
ITERATIONS = (1, 2, 3, 1, 2, 3, 4, 5, 6)         # 1 .. 6, the short ones twice: they are the ones that leave a NaN confined
CORNER_U, CORNER_V = 0.10, 0.13                  # the hostile corner: this fraction of the image's width and height from pixel (0, 0)
FOCUS = 1.0                                      # the elements stand in the focal plane (viewParams.z = 1): defocus does not smear them


def reach(k):
    """pixels a NaN spreads in each direction over k a-trous passes: the taps of pass i lie at -2 .. 2 times 2^i"""
    return 2 * ((1 << k) - 1)


def corner_pixels(w, h):
    """the extent of the hostile corner in pixels: the patch, 2 pixels of ray jitter (divergeStrength <= 2: 1.6 pixels in the focal
    plane) and 2 of camera motion in the temporal sequence"""
    return int(np.ceil(CORNER_U * w)) + 4, int(np.ceil(CORNER_V * h)) + 4


def nan_ok(w, h, knobs):
    """may this seed hold elements that make a NaN?  Only if corner + reach covers at most 40 % of the image under both filters' drawn
    iteration counts (the variance filter's prefilter adds one pixel per pass)"""
    r = max(reach(knobs["denoise"]["iterations"]), reach(knobs["vdenoise"]["iterations"]) + knobs["vdenoise"]["iterations"])
    cw, ch = corner_pixels(w, h)
    return min(w, cw + r) * min(h, ch + r) <= 0.4 * w * h


def filter_knobs(seed):
    """{"options": the builder and traversal options the feature kernel sees (the renderer fuzz's own draw, test_gpu_fuzz.draw_knobs on the
    same generator, plus lds_stack), "frame": the first frame index, "denoise", "vdenoise", "temporal": the calls' parameters,
    "denoise_underflow", "vdenoise_underflow": None or the same parameters with one squared sigma at 1e-25}"""
    drawn = draw_knobs(np.random.default_rng(seed))
    read = ("max_leaf", "full_sort", "compact_nodes", "device_bvh", "bvh_collapse", "bvh_radius", "bvh_top", "bvh_treelets", "bvh_reinsert")
    options = {k: drawn[k] for k in read}
    rng = np.random.default_rng(29000 + seed)
    v = int(rng.choice((2, 3, 8, -1)))
    if v >= 0:
        options["lds_stack"] = v

    def sigmas(default, tight, wide, squared):
        out = {}
        for name in default:
            values = [default[name], tight[name], wide[name], SIGMA_OVERFLOW] + ([] if name in squared else [SIGMA_UNDERFLOW])
            out[name] = float(values[int(rng.integers(len(values)))])
        return out

    def underflow(params, squared):
        if rng.random() >= 1 / 3:
            return None
        return dict(params, **{squared[int(rng.integers(len(squared)))]: SIGMA_UNDERFLOW})

    d_names, v_names = ("sigmaColour", "sigmaNormal", "sigmaDepth"), ("sigmaLuminance", "sigmaNormal", "sigmaDepth")
    d_def = {k: denoise_check.DEFAULTS[k] for k in d_names}
    v_def = {k: vdenoise_check.DEFAULTS[k] for k in v_names}
    denoise = dict(iterations=int(rng.choice(ITERATIONS)), demodulate=int(rng.integers(0, 2)),
                   **sigmas(d_def, denoise_check.TIGHT, denoise_check.WIDE, d_names))
    vdenoise = dict(iterations=int(rng.choice(ITERATIONS)), demodulate=int(rng.integers(0, 2)),
                    **sigmas(v_def, vdenoise_check.TIGHT, vdenoise_check.WIDE, v_names[1:]))
    tol = [TOLERANCES[int(rng.integers(3))] for _ in range(2)]
    temporal = dict(maxHistory=int(rng.choice(MAX_HISTORY)),
                    depthTolerance=float(temporal_check.DEFAULTS["depthTolerance"] if tol[0] is None else tol[0]),
                    normalTolerance=float(temporal_check.DEFAULTS["normalTolerance"] if tol[1] is None else tol[1]))
    return {"options": options, "frame": int(rng.integers(0, 1000)), "denoise": denoise, "vdenoise": vdenoise, "temporal": temporal,
            "denoise_underflow": underflow(denoise, d_names), "vdenoise_underflow": underflow(vdenoise, v_names[1:])}


# ---- the scene ---------------------------------------------------------------------------------------------------------------------------
def _camera(p):
    M = np.asarray(p["camLocalToWorld"], np.float64).reshape(4, 4)
    return M[:3, :3].copy(), M[:3, 3].copy(), np.asarray(p["viewParams"], np.float64)


def _place(p, u, v, depth=FOCUS):
    """the float32 world point seen at image position (u, v) in -0.5 .. 0.5 (pixel x = (u + 0.5) * W - 0.5), `depth` focal distances from
    the camera: the far seeds' shift rides in the camera matrix"""
    R, pos, V = _camera(p)
    return (pos + R @ (np.array([u * V[0], v * V[1], V[2]]) * depth)).astype(F32)


def _quad(p, u0, v0, u1, v1, depth=FOCUS):
    """two triangles (2, 3, 3) over the image rectangle, their front faces to the camera"""
    a, b, c, d = (_place(p, *uv, depth) for uv in ((u0, v0), (u1, v0), (u1, v1), (u0, v1)))
    tri = np.array([[a, c, b], [a, d, c]], F32)
    fwd = _camera(p)[0][:, 2]
    n = np.cross((tri[:, 1] - tri[:, 0]).astype(np.float64), (tri[:, 2] - tri[:, 0]).astype(np.float64))
    flip = n @ fwd > 0
    tri[flip] = tri[flip][:, [0, 2, 1]]
    return tri


def _material(rng, **over):
    m = {"colour": (*rng.uniform(0.2, 1, 3), 1), "emissionColour": (*rng.uniform(0, 1, 3), 1), "specularColour": (1, 1, 1, 1),
         "emissionStrength": 0.0, "smoothness": 0.0, "specularProbability": 0.0, "flag": 0}
    m.update(over)
    return m


def _set_material(rec, m):
    for k, v in m.items():
        rec[k] = v


def fuzz_scene(rtx, seed):
    """(params, spheres, triangles, meshinfo): random_scene(seed) with numRaysPerPixel redrawn and the hostile elements appended, so
    that random_scene's own triangles, chunks and spheres are a prefix of the buffers.  On the seeds with a permuted chunk list
    (seed % 3 == 2) the appended chunks are permuted among themselves too."""
    p, sph, tris, infos = random_scene(rtx, seed)
    knobs = filter_knobs(seed)
    rng = np.random.default_rng(21000 + seed)
    p["numRaysPerPixel"] = int(rng.choice(SAMPLES))
    w, h = int(p["width"]), int(p["height"])
    hostile = nan_ok(w, h, knobs)
    far = seed % 11 == 10
    fwd = _camera(p)[0][:, 2]
    face = (-fwd / np.linalg.norm(fwd)).astype(F32)
    chunks, spheres = [], []                                        # (positions (n, 3, 3), normals (n, 3, 3), material), sphere records
    want = lambda: rng.random() < 0.75                              # every seed gets a subset
    U0, V0 = -0.5, -0.5

    def flat(pos):
        return np.broadcast_to(face, pos.shape).copy()

    # ---- hostile normals: two quads in the corner, in the focal plane; per triangle one value everywhere, one value per vertex, or one
    # component of an ordinary normal
    if want() or hostile:
        pos = np.concatenate([_quad(p, U0 - 0.02, V0 - 0.02, U0 + CORNER_U / 2, V0 + CORNER_V),
                              _quad(p, U0 + CORNER_U / 2, V0 - 0.02, U0 + CORNER_U, V0 + CORNER_V / 2)])
        values = NORMALS if hostile else NORMALS_FINITE
        nrm = flat(pos)
        for t in range(len(pos)):
            how = int(rng.integers(3))
            if how == 0:
                nrm[t] = values[int(rng.integers(len(values)))]
            elif how == 1:
                for k in range(3):
                    nrm[t, k] = values[int(rng.integers(len(values)))]
            else:
                nrm[t, int(rng.integers(3)), int(rng.integers(3))] = values[int(rng.integers(len(values)))]
        chunks.append((pos, nrm, _material(rng)))
    if hostile and knobs["denoise"]["iterations"] == 1:
        # an infinite normal (the dot of a denormal underflows: 1e-42 / 0) on a quad of its own, five pixels from the corner's NaNs: the one
        # hostile guide whose neighbours stay finite, its weight exp2_(-inf) = 0 — after one pass; from the second on the NaN of its own
        # pixel (inf - inf) travels in the colour
        pos = _quad(p, U0 + 0.20, V0 - 0.02, U0 + 0.27, V0 + 0.07)
        chunks.append((pos, np.full(pos.shape, F32(1e-42)), _material(rng)))
    # ---- albedo extremes: a quad in the corner whose colour, and a sphere half a millimetre from the camera (so that no bounce ray
    # finds it and the image's NaN stays in its pixels) whose checker colour, hold such values
    values = ALBEDOS if hostile else ALBEDOS_FINITE
    if want():
        pos = _quad(p, U0 + CORNER_U / 2, V0 + CORNER_V / 2, U0 + CORNER_U, V0 + CORNER_V, FOCUS * 0.99)
        colour = [values[int(rng.integers(len(values)))] for _ in range(3)]
        chunks.append((pos, flat(pos), _material(rng, colour=(*colour, 1))))
    if want() and not far:
        s = np.zeros((), rtx.SPHERE)
        D = 5e-4
        s["position"], s["radius"] = _place(p, U0 + 0.04, V0 + 0.05, D), D * 0.04
        emission = [values[int(rng.integers(len(values)))] for _ in range(3)]
        _set_material(s["material"], _material(rng, emissionColour=(*emission, 1), flag=1))
        spheres.append(s)
    # ---- depth extremes: a sphere far behind the scene, hit at 1e15 .. 4e18 (further, RaySphere's b * b overflows and the ray misses)
    if want():
        s = np.zeros((), rtx.SPHERE)
        D = 10.0 ** rng.uniform(15.3, 18.6)
        s["position"], s["radius"] = _place(p, 0.38, 0.36, D), D * 0.1
        _set_material(s["material"], _material(rng))
        spheres.append(s)
    # ---- tiny depths: a sphere so close to the camera that 1e-6 dominates zs (not where the scene stands 1e5 units out: float32 has no
    # such position there)
    if want() and not far:
        s = np.zeros((), rtx.SPHERE)
        D = 5e-4
        s["position"], s["radius"] = _place(p, 0.40, -0.38, D), D * 0.06
        _set_material(s["material"], _material(rng))
        spheres.append(s)
    # ---- invisible-light stack: an invisible quad before an ordinary one, and an invisible and an ordinary quad on the same vertices
    # (whichever comes first in the chunk list is hit) before a backdrop
    if want() or seed % 3 == 2:
        light = dict(flag=2, emissionStrength=1.0)
        front = _quad(p, 0.22, -0.10, 0.36, 0.16, FOCUS * 0.97)
        pair = _quad(p, 0.30, -0.06, 0.46, 0.12)
        back = _quad(p, 0.20, -0.12, 0.48, 0.18, FOCUS * 1.03)
        stack = [(front, flat(front), _material(rng, **light)), (pair, flat(pair), _material(rng)),
                 (pair.copy(), flat(pair), _material(rng, **light)), (back, flat(back), _material(rng))]
        if rng.random() < 0.5:
            stack[1], stack[2] = stack[2], stack[1]
        chunks += stack
    # ---- a sliver of coverage: a triangle 12 pixels long that tapers from a tenth of a pixel to nothing
    if want():
        a, b = _place(p, -0.45, 0.10), _place(p, -0.25, 0.13)
        c = _place(p, -0.45, 0.10 + 0.1 / max(h, 1))
        pos = np.array([[a, b, c]], F32)
        n = np.cross((b - a).astype(np.float64), (c - a).astype(np.float64))
        if n @ fwd > 0:
            pos = pos[:, [0, 2, 1]]
        chunks.append((pos, flat(pos), _material(rng)))

    n0, m0 = len(tris), len(infos)
    more_t = np.zeros(sum(len(c[0]) for c in chunks), rtx.TRIANGLE)
    more_m = np.zeros(len(chunks), rtx.MESHINFO)
    at = 0
    for ci, (pos, nrm, mat) in enumerate(chunks):
        t = more_t[at:at + len(pos)]
        t["posA"], t["posB"], t["posC"] = pos[:, 0], pos[:, 1], pos[:, 2]
        t["normalA"], t["normalB"], t["normalC"] = nrm[:, 0], nrm[:, 1], nrm[:, 2]
        mi = more_m[ci]
        mi["firstTriangleIndex"], mi["numTriangles"] = n0 + at, len(pos)
        _set_material(mi["material"], mat)
        mi["boundsMin"], mi["boundsMax"] = pos.reshape(-1, 3).min(0), pos.reshape(-1, 3).max(0)
        at += len(pos)
    if seed % 3 == 2 and len(more_m):
        more_m = more_m[rng.permutation(len(more_m))].copy()
    more_s = np.array(spheres, rtx.SPHERE) if spheres else np.zeros(0, rtx.SPHERE)
    return p, np.concatenate([sph, more_s]), np.concatenate([tris, more_t]), np.concatenate([infos, more_m])


# ---- the temporal sequence -----------------------------------------------------------------------------------------------------------------
def _posed(params, offset=(0.0, 0.0, 0.0), yaw=0.0, pitch=0.0, zoom=1.0):
    """a copy of `params` with the camera moved by `offset` (in its own axes), turned by `yaw` about its own up axis and by `pitch` about
    its own right axis, and its view plane scaled by `zoom`"""
    R, pos, V = _camera(params)
    cy, sy, cp, sp = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch)
    Rl = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @ np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]])
    M = np.eye(4)
    M[:3, :3], M[:3, 3] = R @ Rl, pos + R @ np.asarray(offset, np.float64)
    out = params.copy()
    out["camLocalToWorld"] = M.astype(F32).reshape(16)
    out["worldSpaceCameraPos"] = M[:3, 3].astype(F32)
    out["viewParams"] = (V * (zoom, zoom, 1.0)).astype(F32)
    return out


def poses(rtx, seed, params):
    """The cameras of the temporal sequence, call 0's (the scene's own) first: the same pose again; a small step that keeps most of the
    history — a tenth of a millimetre sideways and a yaw about the camera's own up axis that puts image column k of the new view at
    px = -0.995 - of the old one, so that on that column only the taps of weight fx < 0.01 lie inside (sw below 0.01) —; on one seed in
    three the same pose zoomed in; a jump that turns the camera away."""
    rng = np.random.default_rng(25000 + seed)
    W, V = int(params["width"]), np.asarray(params["viewParams"], np.float64)
    k = int(rng.integers(0, 3))
    lx = ((k + 0.5) / W - 0.5) * V[0]
    yaw = np.arctan(lx - (k + 0.995) * V[0] / W) - np.arctan(lx)
    small = _posed(params, offset=(*rng.uniform(-5e-5, 5e-5, 2), 0.0), yaw=yaw)
    out = [params.copy(), params.copy(), small]
    if seed % 3 == 1:
        out.append(_posed(small, zoom=float(rng.uniform(0.6, 0.9))))
    out.append(_posed(small, offset=rng.uniform(-2, 2, 3), yaw=float(rng.uniform(2.0, 4.0)), pitch=float(rng.uniform(-0.3, 0.3))))
    return out


# ---- one seed ------------------------------------------------------------------------------------------------------------------------------
def fuzz_case(rtx, seed):
    """{"seed", "scene", "knobs", "poses", "hostile", "inject", "planes"}: everything one seed is — `knobs` is filter_knobs(seed) with the
    iteration counts settled (below), `planes` the feature checker's (A, G) of the scene's own pose"""
    scene = fuzz_scene(rtx, seed)
    knobs = filter_knobs(seed)
    p = scene[0]
    w, h = int(p["width"]), int(p["height"])
    hostile = bool(nan_ok(w, h, knobs))
    rng = np.random.default_rng(31000 + seed)
    C = rng.uniform(0.0, 1e4, (h, w, 4)).astype(F32)
    if hostile:                                                     # a few non-finite entries, in the hostile corner
        cw, ch = min(w, int(np.ceil(CORNER_U * w))), min(h, int(np.ceil(CORNER_V * h)))
        for value in (NAN, INF, -INF, NAN):
            C[int(rng.integers(ch)), int(rng.integers(cw)), int(rng.integers(3))] = value
    # what is left to chance — random_scene's own zero vertex normals normalise to NaN wherever a sample meets them —: the iteration
    # counts come down until the pixels within reach of a non-finite guide or albedo are at most 40 % of the image
    f = knobs["frame"]
    A, G = aov_check.oracle_planes(rtx, *scene, [f, f + 1])
    ys, xs = np.nonzero(~(np.isfinite(A).all(-1) & np.isfinite(G).all(-1)))

    def within(r):
        m = np.zeros((h, w), bool)
        for y, x in zip(ys, xs):
            m[max(0, y - r):y + r + 1, max(0, x - r):x + r + 1] = True
        return m.mean() if m.size else 0.0
    for name, extra in (("denoise", 0), ("vdenoise", 1)):
        k = knobs[name]["iterations"]
        while k > 1 and within(reach(k) + extra * k) > 0.4:
            k -= 1
        for which in (name, name + "_underflow"):
            if knobs[which] is not None:
                knobs[which]["iterations"] = k
    return {"seed": seed, "scene": scene, "knobs": knobs, "poses": poses(rtx, seed, p), "hostile": hostile, "inject": C, "planes": (A, G)}


def load_scene(t, case):
    """options, params and buffers into a fresh Tracer or MultiTracer"""
    for k, v in case["knobs"]["options"].items():
        t.set_option(k, v)
    p, sph, tris, infos = case["scene"]
    t.set_params(p)
    t.upload(spheres=sph, triangles=tris, meshinfo=infos)


def _filter_calls(knobs):
    """(name, parameters) of the seed's rt_denoise and rt_denoise_variance calls"""
    d = [("drawn", knobs["denoise"])] + ([("underflow", knobs["denoise_underflow"])] if knobs["denoise_underflow"] else [])
    v = [("drawn", knobs["vdenoise"])] + ([("underflow", knobs["vdenoise_underflow"])] if knobs["vdenoise_underflow"] else [])
    return d, v


def stages(rtx, t, case, state=None):
    """The seed's calls on a loaded Tracer or MultiTracer, in order.  Yields (name, plane, want, inputs): every plane the calls leave,
    `want` a function that gives the CPU checker's answer from what the context's own readers returned (the colour, A and G in
    `inputs`), or None for a plane that must only be the same behind both kinds of handle.  `state`: a function (context, name) called
    before and after every group of filter calls (the state the header says stays)."""
    p, sph, tris, infos = case["scene"]
    knobs = case["knobs"]
    f = knobs["frame"]
    d_calls, v_calls = _filter_calls(knobs)
    mark = state or (lambda t, name: None)

    def var(plane):
        return plane[..., None]

    # 1. the feature planes
    t.render_aov(f, 2)
    A, G = t.read_aov(0), t.read_aov(1)
    want = {}

    def planes():
        if not want:
            want["A"], want["G"] = case.get("planes") or aov_check.oracle_planes(rtx, p, sph, tris, infos, [f, f + 1])
        return want
    yield "render_aov: albedo and coverage", A, lambda: planes()["A"], None
    yield "render_aov: normal and depth", G, lambda: planes()["G"], None
    # 2. rt_denoise on the rendered image, then on injected colours
    t.render(f, 1)
    for colour in ("rendered", "injected"):
        if colour == "injected":
            t.write_accum(case["inject"], 3)
        C = t.read_accum()
        mark(t, f"before the filters, {colour}")
        for name, kw in d_calls:
            t.denoise(**kw)
            yield f"denoise, {colour} image, {name} {kw}", t.read_denoised(), (lambda C=C, kw=kw: denoise_check.checker(C, A, G, **kw)), (C, A, G, kw)
        # 3. rt_denoise_variance on the image
        for name, kw in v_calls:
            t.denoise_variance(source=0, **kw)
            w = {}

            def both(C=C, kw=kw, w=w):
                if not w:
                    w["out"], w["var"] = vdenoise_check.checker(C, A, G, **kw)
                return w
            yield f"denoise_variance, {colour} image, {name} {kw}", t.read_denoised(), (lambda both=both: both()["out"]), (C, A, G, kw)
            yield f"denoise_variance var_0, {colour} image, {name} {kw}", var(t.read_variance()), (lambda both=both: var(both()["var"])), (C, A, G, kw)
        mark(t, f"after the filters, {colour}")
    # 4. the pose sequence
    chk = temporal_check.Checker()
    case["checker"] = chk
    last = len(case["poses"]) - 1
    for k, pose in enumerate(case["poses"]):
        t.set_params(pose)
        t.reset_accum()
        t.render(f + k, 1)
        t.reset_aov()
        t.render_aov(f + k, 2)
        C, A, G = t.read_accum(), t.read_aov(0), t.read_aov(1)
        mark(t, f"before rt_temporal, pose {k}")
        t.temporal(**knobs["temporal"])
        step = {}

        def stepped(C=C, A=A, G=G, pose=pose, step=step):
            if not step:
                step["T"], step["N"] = chk.step(C, A, G, pose, **knobs["temporal"])
            return step
        yield f"temporal pose {k}: T, {knobs['temporal']}", t.read_temporal(), (lambda s=stepped: s()["T"]), (C, A, G, pose)
        yield f"temporal pose {k}: N, {knobs['temporal']}", var(t.read_temporal_history()), (lambda s=stepped: var(s()["N"])), (C, A, G, pose)
        if k == last:
            T = t.read_temporal()
            for name, kw in d_calls:
                t.denoise_temporal(**kw)
                yield f"denoise_temporal, {name} {kw}", t.read_denoised(), (lambda T=T, A=A, G=G, kw=kw: denoise_check.checker(T, A, G, **kw)), (T, A, G, kw)
            for name, kw in v_calls:
                t.denoise_variance(source=1, **kw)
                w = {}

                def both1(T=T, A=A, G=G, kw=kw, w=w):
                    if not w:
                        w["out"], w["var"] = vdenoise_check.checker(T, A, G, **kw)
                    return w
                yield f"denoise_variance source 1, {name} {kw}", t.read_denoised(), (lambda b=both1: b()["out"]), (T, A, G, kw)
                yield f"denoise_variance source 1 var_0, {name} {kw}", var(t.read_variance()), (lambda b=both1: var(b()["var"])), (T, A, G, kw)
        mark(t, f"after rt_temporal, pose {k}")


# ---- what the checkers find in a seed's inputs ---------------------------------------------------------------------------------------------
class CpuContext:
    """The CPU checkers behind the calls `stages` makes: the oracle's frame for rt_render, aov_check for rt_render_aov, and the three
    filter checkers for the planes they leave, so that the stages run, and their inputs can be counted, without a GPU."""

    def __init__(self, rtx, oracle, case):
        self.rtx, self.oracle, self.case = rtx, oracle, case
        self.params = case["scene"][0]
        self.C = self.A = self.G = self.T = self.N = self.out = self.variance = None
        self.k = 0
        self.chk = temporal_check.Checker()

    def set_params(self, p):
        self.params = p

    def reset_accum(self):
        self.C = None

    def reset_aov(self):
        self.A, self.k = None, 0

    def render(self, frame, n):
        assert n == 1 and self.C is None
        _, sph, tris, infos = self.case["scene"]
        self.C = self.oracle.render_frame(self.params, sph, tris, infos, frame, accel=True)[0]

    def render_aov(self, frame, n):
        assert self.A is None
        _, sph, tris, infos = self.case["scene"]
        self.A, self.G = aov_check.oracle_planes(self.rtx, self.params, sph, tris, infos, range(frame, frame + n))

    def write_accum(self, C, frames):
        self.C = np.array(C, F32)

    def read_accum(self):
        return self.C.copy()

    def read_aov(self, which):
        return (self.G if which else self.A).copy()

    def denoise(self, **kw):
        self.out = denoise_check.checker(self.C, self.A, self.G, **kw)

    def denoise_temporal(self, **kw):
        self.out = denoise_check.checker(self.T, self.A, self.G, **kw)

    def denoise_variance(self, source=0, **kw):
        self.out, self.variance = vdenoise_check.checker(self.T if source else self.C, self.A, self.G, **kw)

    def temporal(self, **kw):
        self.T, self.N = self.chk.step(self.C, self.A, self.G, self.params, **kw)

    def read_denoised(self):
        return self.out.copy()

    def read_variance(self):
        return self.variance.copy()

    def read_temporal(self):
        return self.T.copy()

    def read_temporal_history(self):
        return self.N.copy()


def cpu_planes(rtx, oracle, case):
    """[(name, plane, inputs)] of a seed, every plane the checkers' own"""
    return [(name, plane, inputs) for name, plane, _, inputs in stages(rtx, CpuContext(rtx, oracle, case), case)]


def finite_fraction(plane):
    """the share of pixels that are finite in every channel"""
    return float(np.isfinite(plane).all(-1).mean()) if plane.size else 1.0


# the mutants of the three checkers (`variant` of denoise_oracle.c, vdenoise_oracle.c, temporal_oracle.c): one-line deviations from the
# definition that the comparison must be able to tell from it
DENOISE_MUTANTS = {1: "a tap outside the image clamped, not skipped", 2: "a colour sigma that does not halve",
                   3: "d = max(A.ch + cov1, 0.01) returning the NaN operand"}
VDENOISE_MUTANTS = {1: "a tap outside the image clamped, not skipped", 2: "the prefilter at spacing s", 3: "variance weighted by w, not w * w",
                    4: "d = max(A.ch + cov1, 0.01) returning the NaN operand", 5: "var_0 = max(v, 0) returning the NaN operand"}
TEMPORAL_MUTANTS = {1: "a tap outside the image clamped, not skipped", 2: "no depth test", 3: "the history length not capped",
                    4: "t <= maxHistory for t < maxHistory in the cap (the same n: only the decision code differs)",
                    5: "the depth test relative to G'.w, not ze", 6: "no normal test"}


def temporal_run(steps, knobs, variant=0):
    """the lock-step checker over a seed's recorded (C, A, G, pose) steps -> [(T, N, code)]"""
    chk, out = temporal_check.Checker(), []
    for C, A, G, pose in steps:
        T, N = chk.step(C, A, G, pose, variant=variant, **knobs["temporal"])
        out.append((T, N, chk.code.copy(), chk.G.copy()))
    return out


def _differ(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype == np.float32:
        return bool((~((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b)))).any())
    return bool((a != b).any())


def mutants_caught(recorded, knobs):
    """{(checker, variant): True if the mutant's output differs from the definition's on these recorded inputs}.  `recorded`: what
    cpu_planes returned.  Bits compared, NaN equal to NaN; the temporal mutants on T and N, mutant 4 on the decision code too (its T and N
    cannot differ: at t == maxHistory both forms give maxHistory)."""
    caught = {}
    steps = []
    for name, plane, inputs in recorded:
        if name.startswith("denoise,") or name.startswith("denoise_temporal"):
            C, A, G, kw = inputs
            for v in DENOISE_MUTANTS:
                caught["denoise", v] = caught.get(("denoise", v), False) or _differ(denoise_check.checker(C, A, G, variant=v, **kw), plane)
        elif name.startswith("denoise_variance") and "var_0" not in name:
            C, A, G, kw = inputs
            want = vdenoise_check.checker(C, A, G, **kw)
            for v in VDENOISE_MUTANTS:
                got = vdenoise_check.checker(C, A, G, variant=v, **kw)
                caught["vdenoise", v] = caught.get(("vdenoise", v), False) or _differ(got[0], want[0]) or _differ(got[1], want[1])
        elif name.startswith("temporal") and ": T" in name:
            steps.append(inputs)
    if steps:
        base = temporal_run(steps, knobs)
        for v in TEMPORAL_MUTANTS:
            run = temporal_run(steps, knobs, v)
            caught["temporal", v] = any(_differ(a[0], b[0]) or _differ(a[1], b[1]) or (v == 4 and _differ(a[2][..., 0], b[2][..., 0]))
                                        for a, b in zip(run, base))
    return caught


CLASSES = ("nan_normal", "far", "near", "albedo_nonfinite", "albedo_floor", "sliver", "pass_through", "tie_permuted", "tap_zero_weight",
           "tap_nan", "var_select", "t_accepted", "t_depth", "t_normal", "t_offscreen", "t_sky", "sw_above", "sw_below")
CLASS_NOTES = {
    "nan_normal": "a NaN normal in G", "far": "depth above 1e15", "near": "depth below 1e-3", "albedo_nonfinite": "a non-finite albedo",
    "albedo_floor": "an albedo channel <= 0 at coverage 1 (the 0.01 floor decides d)", "sliver": "coverage in (0, 1/16]",
    "pass_through": "sample 0's first hit is an invisible light and a second cast is made",
    "tie_permuted": "sample 0's first hit has a second candidate at its dst, under a permuted chunk list",
    "tap_zero_weight": "a denoised pixel finite although one of its 25 pass-0 taps is not",
    "tap_nan": "a denoised pixel not finite because of such a tap", "var_select": "var_0 = 0 by the select on a NaN",
    "t_accepted": "temporal taps that count", "t_depth": "taps the depth test alone rejects", "t_normal": "taps the normal test alone rejects",
    "t_offscreen": "pixels whose reprojection is not valid", "t_sky": "sky pixels with history", "sw_above": "sw >= 0.01",
    "sw_below": "0 < sw < 0.01"}


def _pass0_taps_nonfinite(C, A, G, kw):
    """per pixel: is any tap of pass 0 (spacing 1, inside the image, the centre included) non-finite in G or in e0?"""
    H, W = C.shape[:2]
    with np.errstate(all="ignore"):
        if kw["demodulate"]:
            t = A[..., :3] + (F32(1.0) - A[..., 3:4])
            e0 = C[..., :3] / np.where(t > F32(0.01), t, F32(0.01))
        else:
            e0 = C[..., :3]
    bad = ~(np.isfinite(G).all(-1) & np.isfinite(e0).all(-1))
    out = np.zeros((H, W), bool)
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            y0, y1, x0, x1 = max(0, -dy), min(H, H - dy), max(0, -dx), min(W, W - dx)
            if y0 < y1 and x0 < x1:
                out[y0:y1, x0:x1] |= bad[y0 + dy:y1 + dy, x0 + dx:x1 + dx]
    return out


def power_counts(rtx, case, recorded):
    """{class: pixels} of one seed, counted from the checkers' planes (`recorded`: what cpu_planes returned), and "finite": the share of
    finite pixels of the three outputs the floor is asserted on"""
    p, sph, tris, infos = case["scene"]
    knobs = case["knobs"]
    by = {name: (plane, inputs) for name, plane, inputs in recorded}
    A, G = recorded[0][1], recorded[1][1]
    c = dict.fromkeys(CLASSES, 0)
    with np.errstate(all="ignore"):
        cov = A[..., 3]
        zc = np.where(cov > 0, G[..., 3] / np.where(cov > 0, cov, 1), np.nan)
        c["nan_normal"] = int(np.isnan(G[..., :3]).any(-1).sum())
        c["far"], c["near"] = int((zc > 1e15).sum()), int((zc < 1e-3).sum())
        c["albedo_nonfinite"] = int((~np.isfinite(A[..., :3]).all(-1)).sum())
        c["albedo_floor"] = int(((cov == 1) & (A[..., :3] <= 0).any(-1)).sum())
        c["sliver"] = int(((cov > 0) & (cov <= F32(1 / 16))).sum())
    # sample 0's camera rays of the first feature frame are the rays frag draws in Philox mode
    rays = query_check.frame_camera_rays(rtx, p, knobs["frame"])
    shim, mode = query_check.lib(), int(p["intersectMode"])
    hits = query_check.oracle_hits(rtx, shim, sph, tris, infos, mode, rays)
    flag = np.zeros(len(rays), np.int64)
    tri, ball = hits["kind"] == 2, hits["kind"] == 1
    flag[tri] = infos["material"]["flag"][hits["chunk"][tri]]
    flag[ball] = sph["material"]["flag"][hits["primitive"][ball]]
    c["pass_through"] = int((flag == 2).sum()) if int(p["maxBounceCount"]) >= 1 else 0
    if case["seed"] % 3 == 2:
        c["tie_permuted"] = int((query_check.oracle_candidates(rtx, shim, sph, tris, infos, mode, rays) >= 2).sum())
    finite = {}
    for name, (plane, inputs) in by.items():
        if name.startswith("denoise, rendered image, drawn"):
            bad_tap = _pass0_taps_nonfinite(*inputs)
            ok = np.isfinite(plane).all(-1)
            c["tap_zero_weight"], c["tap_nan"] = int((bad_tap & ok).sum()), int((bad_tap & ~ok).sum())
            finite["denoise"] = finite_fraction(plane)
        elif name.startswith("denoise_variance, rendered image, drawn"):
            finite["vdenoise"] = finite_fraction(plane)
            C, Ain, Gin, kw = inputs
            kept = vdenoise_check.checker_variance(C, Ain, Gin, kw["demodulate"], kw["sigmaNormal"], kw["sigmaDepth"], variant=5)
            var0 = by[name.replace("denoise_variance,", "denoise_variance var_0,")][0][..., 0]
            c["var_select"] = int((np.isnan(kept) & (var0 == 0)).sum())
    steps = [inputs for name, plane, inputs in recorded if name.startswith("temporal") and ": T" in name]
    base, no_depth, no_normal = (temporal_run(steps, knobs, v) for v in (0, 2, 6))
    finite["temporal"] = finite_fraction(base[-1][0])
    for k in range(1, len(steps)):
        code, surf = base[k][2][..., 0], steps[k][1][..., 3] > 0
        taps = lambda code: sum(((code >> (1 + j)) & 1).astype(np.int64) for j in range(4))
        c["t_accepted"] += int(taps(code).sum())
        c["t_depth"] += int(np.maximum(taps(no_depth[k][2][..., 0]) - taps(code), 0).sum())
        c["t_normal"] += int(np.maximum(taps(no_normal[k][2][..., 0]) - taps(code), 0).sum())
        c["t_offscreen"] += int(((code & 1) == 0).sum())
        c["t_sky"] += int((~surf & ((code & 32) != 0)).sum())
        c["sw_above"] += int(((code & 32) != 0).sum())
        c["sw_below"] += int((((code & 32) == 0) & (taps(code) > 0)).sum())
    c["finite"] = finite
    return c


def benign_recorded(rtx, oracle):
    """what the image chain's GPU tests had before: mesh_test_scene at 70 x 45, two samples per pixel, the defaults and a tight set, a
    sideways step and a yaw — recorded as cpu_planes records a seed, for mutants_caught"""
    mgr = rtx.scenes.mesh_test_scene(70, 45)
    mgr.numRaysPerPixel = 2
    scene = mgr.build_buffers()
    p = scene[0]
    knobs = {"options": {}, "frame": 0, "denoise": dict(denoise_check.DEFAULTS, iterations=5, demodulate=1, **denoise_check.TIGHT),
             "vdenoise": dict(vdenoise_check.DEFAULTS), "temporal": dict(temporal_check.DEFAULTS, maxHistory=3),
             "denoise_underflow": None, "vdenoise_underflow": None}
    steps = [p.copy(), p.copy(), _posed(p, offset=(0.25, 0.0, 0.0)), _posed(p, offset=(0.25, 0.0, 0.0), yaw=0.35)]
    case = {"seed": -1, "scene": scene, "knobs": knobs, "poses": steps, "hostile": False,
            "inject": np.random.default_rng(7).uniform(0.0, 1e4, (45, 70, 4)).astype(F32)}
    return cpu_planes(rtx, oracle, case), knobs


def inputs_table(rtx, oracle, seeds=range(24)):
    """the text of profiles/filter_fuzz_inputs.txt"""
    head = ("seed    size   N it hostile  finite d / v / T   " + " ".join(f"{k[:9]:>9s}" for k in CLASSES))
    rows, reached, caught = [], dict.fromkeys(CLASSES, 0), {}
    for seed in seeds:
        case = fuzz_case(rtx, seed)
        rec = cpu_planes(rtx, oracle, case)
        c = power_counts(rtx, case, rec)
        for key, hit in mutants_caught(rec, case["knobs"]).items():
            caught.setdefault(key, []).extend([seed] if hit else [])
        p, f = case["scene"][0], c["finite"]
        it = f"{case['knobs']['denoise']['iterations']}{case['knobs']['vdenoise']['iterations']}"
        rows.append(f"{seed:4d} {int(p['width']):3d}x{int(p['height']):<3d} {int(p['numRaysPerPixel']):3d} {it} {'yes' if case['hostile'] else ' no':>7s}"
                    f"  {f['denoise']:5.3f} {f['vdenoise']:5.3f} {f['temporal']:5.3f}  " + " ".join(f"{c[k]:9d}" for k in CLASSES))
        for k in CLASSES:
            reached[k] += c[k] >= 4
    out = [head, *rows, "seeds with at least four pixels of the class:", f"{'':51s}" + " ".join(f"{reached[k]:9d}" for k in CLASSES), "", "the classes:"]
    out += [f"  {k:17s} {CLASS_NOTES[k]}" for k in CLASSES]
    out += ["", "not reachable through the feature definition:",
            "  an infinite depth, or a depth whose square overflows (above 1.8e19): RaySphere's b * b overflows from 9.2e18 on, the",
            "  discriminant is inf - inf = NaN and the ray misses; the farthest hit is near 4e18, where G.w * G.w = 1.6e37",
            "  a finite pixel in a call with a squared sigma of 1e-25: the constant is 1 / 0 = inf and the centre tap's difference is 0,",
            "  0 * inf = NaN on every pixel; the seeds that draw it make that call beside the drawn one (finite: the drawn one's share)",
            "", "mutants of the checkers (variant: the seeds whose inputs tell it from the definition; mesh_test_scene 70 x 45 as the GPU tests had it):"]
    benign = mutants_caught(*benign_recorded(rtx, oracle))
    names = {"denoise": DENOISE_MUTANTS, "vdenoise": VDENOISE_MUTANTS, "temporal": TEMPORAL_MUTANTS}
    for (which, v), where in sorted(caught.items()):
        out.append(f"  {which:8s} {v}  {names[which][v]}: seeds {' '.join(map(str, where)) or 'none'}; "
                   f"mesh_test_scene {'catches it' if benign[which, v] else 'DOES NOT catch it'}")
    return "\n".join(out) + "\n"


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import oracle_binding
    import rtx_pkg
    # `python tests/filter_fuzz.py` prints profiles/filter_fuzz_inputs.txt
    print(inputs_table(rtx_pkg.load(), oracle_binding.Oracle()), end="")
