"""A float64 twin of the reference's shader.  TEST INFRASTRUCTURE ONLY (like oracle/): nothing under the product imports it.

It restates Assets/Scripts/Shaders/RayTracing.shader and Accumulate.shader of the project this one was modelled on, function by
function, in plain NumPy, written from the shader's text and not from oracle/rt_oracle.c: IEEE double arithmetic, libm / NumPy
transcendentals, NumPy's own summation order, `fmin` / `fmax` for HLSL's min / max (Direct3D: "if one operand is NaN the other is
returned").  Its worth is that it is a second opinion: where the oracle misreads the shader and the kernels copy it, this file
disagrees.  Citations `:N` are line numbers of RayTracing.shader.

What is shared with the oracle on purpose, because it is exact: the input buffers (the float32 bytes of rtx.PARAMS / SPHERE / TRIANGLE /
MESHINFO, widened exactly), the integer PCG stream (:193-199, pinned by tests/golden/pcg_kat.json) and the Philox addressing of
DESIGN.md "Counter-based mode" (not a mode of the shader).  Because the random integers are the same, the twin walks the same light path
as the oracle sample by sample, and images are compared per pixel, not statistically.

Literals the shader writes as floats are float32 constants in HLSL; they are rounded to float32 first and then widened (`_lit`):
PI = 3.1415 (:35, RandomPointInCircle), 3.1415926 (:210), 4294967295.0 (:203; as a float32 this is 2^32, so RandomValue = r / 2^32),
1E-6 (:169), 0.001 (:320), 0.4 / 0.35 / -0.01 (:244-245).

The element type is a parameter (float64 by default).  With float32 the same text becomes one more float32 evaluation of the shader, with
its own rounding; comparing the two twins measures how far two honest evaluations may differ, and that (times 4) is where the
tolerances of the comparisons come from — never from the oracle or a kernel, which are the things under test.

DECISION MARGINS.  Every discrete decision of a sample (specular or diffuse, roulette, hit or miss and which primitive, checker cell,
sun gate, chunk-box cull) is recorded with a dimensionless margin; a sample's margin is the smallest of them and a sample is *fragile*
when it is under the case's threshold.  Per decision:
  isSpecularBounce (:325)   |specularProbability - r|
  roulette (:339)           |r - p|
  winning triangle (:169)   min(u, v, w), dst |dir| / |origin - posA|, (determinant - 1e-6) / (|dir| |normalVector|)
  winning sphere (:133,138) discriminant / b^2, dst |dir| / |origin - centre|
  runner-up                 (dst2 - dst) / dst for the second closest valid primitive
  near miss                 for every rejected primitive that would have been closer: the largest amount by which one of the conditions
                            above fails (a grazed sphere uses -b / 2a for its distance)
  chunk box (:186, mode 0)  min over axes i != j of (t2[j] - t1[i]) / max |t| (the i = j pairs cannot fail), as one more condition of
                            each triangle of the chunk
  tMax (ray queries)        |dst - tMax| / dst
  checker cell (:315)       distance of hitPoint.x and .z (the coordinates used) to the nearest integer
  environment (:244-249)    distance of both smoothstep arguments (x - e0) / (e1 - e0) to 0 and to 1; the sun gate groundToSkyT >= 1 is
                            the second one's distance to 1
The signature of a sample is, per bounce: kind, primitive, specular flag, checker parity, survived the roulette.

MEASURED NUMBERS.  `python tests/twin_cases.py` renders every case of the comparisons with the float32 and the float64 twin and prints,
per case: the largest error of the float32 twin where both twins took the same decisions, the largest margin at which they took
different ones, and the share of fragile samples under the derived threshold.  The table that run printed, the constants derived from
it (x 4) and the observed oracle-vs-twin and kernel-vs-twin maxima with their ratio to the tolerance are kept in tests/twin_cases.py next
to the cases themselves (MEASURED, OBSERVED_ORACLE, OBSERVED_KERNELS).
"""
import numpy as np

RT_HIT_NONE, RT_HIT_SPHERE, RT_HIT_TRIANGLE = 0, 1, 2
CHECKER_PATTERN, INVISIBLE_LIGHT_SOURCE = 1, 2                     # :57-58
MISREADINGS = ("swap_uv", "sun_ungated", "swap_pi", "checker_xy", "smooth_no_flag", "emit_after")


def _lit(text, dt):
    """a float literal of the shader: a float32 constant, widened"""
    return dt(np.float32(text))


# ---- integer RNG -----------------------------------------------------------------------------------------------------------------
M32 = 0xFFFFFFFF


def pcg_next(state):
    """NextRandom :193-199 on Python integers or uint64 arrays holding 32-bit values: (new state, result)"""
    state = (state * 747796405 + 2891336453) & M32
    result = (((state >> ((state >> 28) + 4)) ^ state) * 277803737) & M32
    result = ((result >> 22) ^ result) & M32
    return state, result


def philox4x32_10(ctr, key):
    """Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11) on Python integers or uint64 arrays holding
    32-bit values — independent of the oracle's C"""
    c0, c1, c2, c3 = ctr
    k0, k1 = key
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = ((p1 >> 32) ^ c1 ^ k0) & M32, p1 & M32, ((p0 >> 32) ^ c3 ^ k1) & M32, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


def philox_substreams(rays_per_pixel):
    return 16 if rays_per_pixel >= 16 else 4 if rays_per_pixel >= 4 else 1


class _Rng:
    """One stream per pixel.  PCG: the state chains through every draw of the pixel (:362, 374-385).  Philox: the draws of a scope are words
    0, 1, 2, ... of blocks `block`, `block` + 1, ... of philox(key = (pixelIndex, Frame), counter = (block, sample, 0, 0))."""

    def __init__(self, mode, pixel_index, frame, dt):
        self.mode, self.dt = mode, dt
        self.pixel = pixel_index.astype(np.uint64)
        self.frame = int(frame) & M32
        self.state = (self.pixel + ((int(frame) * 719393) & M32)) & M32                     # :362, uint arithmetic wraps
        n = len(pixel_index)
        self.sample, self.block, self.word = 0, np.zeros(n, np.uint64), np.zeros(n, np.uint64)

    def scope(self, lanes, block):
        self.block[lanes] = block
        self.word[lanes] = 0

    def value(self, lanes):
        """RandomValue :201-204 for the pixels `lanes`"""
        if self.mode == 0:
            self.state[lanes], r = pcg_next(self.state[lanes])
        else:
            n = self.word[lanes]
            out = philox4x32_10((self.block[lanes] + (n >> 2), np.full(len(lanes), self.sample, np.uint64), 0 * n, 0 * n),
                                (self.pixel[lanes], np.full(len(lanes), self.frame, np.uint64)))
            r = np.choose((n & 3).astype(np.int64), out)
            self.word[lanes] = n + 1
        # uint -> float conversion rounds to the element type; 4294967295.0 is the float32 constant 2^32
        return r.astype(self.dt) / _lit("4294967295.0", self.dt)


# ---- scene -----------------------------------------------------------------------------------------------------------------------
class Scene:
    """the reference's buffers, widened exactly to the element type"""

    def __init__(self, params, spheres, tris, infos, dtype=np.float64, mode=None, misread=()):
        dt = self.dt = np.dtype(dtype).type
        assert set(misread) <= set(MISREADINGS), misread
        self.misread = frozenset(misread)
        w = lambda a: np.asarray(a, np.float32).astype(dt)      # noqa: E731
        self.p = None
        if params is not None:
            p = np.asarray(params).reshape(())
            self.p = {k: (w(p[k]) if p[k].dtype.kind == "f" else int(p[k])) for k in p.dtype.names if not k.startswith("_")}
        self.mode = int(mode) if mode is not None else (self.p["intersectMode"] if self.p else 0)
        self.centre, self.radius = w(spheres["position"]).reshape(-1, 3), w(spheres["radius"]).reshape(-1)
        self.sphere_mat = self._materials(spheres["material"], w)
        # every triangle of every chunk, in the order the loops :276-294 visit them
        first, count = np.asarray(infos["firstTriangleIndex"], np.int64).reshape(-1), np.asarray(infos["numTriangles"], np.int64).reshape(-1)
        self.ref_tri = np.concatenate([np.arange(f, f + c) for f, c in zip(first, count)] + [np.zeros(0, np.int64)]).astype(np.int64)
        self.ref_chunk = np.repeat(np.arange(len(first)), count)
        t = np.asarray(tris)[self.ref_tri] if len(self.ref_tri) else np.asarray(tris)[:0]
        self.A, self.B, self.C = (w(t[k]).reshape(-1, 3) for k in ("posA", "posB", "posC"))
        self.nA, self.nB, self.nC = (w(t[k]).reshape(-1, 3) for k in ("normalA", "normalB", "normalC"))
        self.bmin, self.bmax = w(infos["boundsMin"]).reshape(-1, 3), w(infos["boundsMax"]).reshape(-1, 3)
        self.chunk_mat = self._materials(infos["material"], w)

    @staticmethod
    def _materials(m, w):
        out = {k: w(m[k]) for k in ("colour", "emissionColour", "specularColour", "emissionStrength", "smoothness", "specularProbability")}
        for k in ("colour", "emissionColour", "specularColour"):
            out[k] = out[k].reshape(-1, 4)[:, :3]
        for k in ("emissionStrength", "smoothness", "specularProbability"):
            out[k] = out[k].reshape(-1)
        out["flag"] = np.asarray(m["flag"], np.int64).reshape(-1)
        return out


# ---- HLSL intrinsics in the element type -------------------------------------------------------------------------------------------
def _dot(a, b):
    return np.sum(a * b, axis=-1)


def _cross(a, b):
    return np.cross(a, b)


def _normalize(v):
    return v / np.sqrt(_dot(v, v))[..., None]


def _lerp(a, b, t):
    return a + t * (b - a)


def _saturate(x):
    return np.fmin(np.fmax(x, x.dtype.type(0)), x.dtype.type(1))


def _neg_inf_for_nan(x):
    return np.where(np.isnan(x), -np.inf, x)


# ---- intersection ----------------------------------------------------------------------------------------------------------------
def _box_condition(sc, o, d):
    """RayBoundingBox :177-187 for every ray and chunk: (passes, margin of the decision; negative where it fails)"""
    inv = 1 / d[:, None, :]
    t_min, t_max = (sc.bmin[None] - o[:, None, :]) * inv, (sc.bmax[None] - o[:, None, :]) * inv
    t1, t2 = np.fmin(t_min, t_max), np.fmax(t_min, t_max)
    t_near, t_far = np.fmax(np.fmax(t1[..., 0], t1[..., 1]), t1[..., 2]), np.fmin(np.fmin(t2[..., 0], t2[..., 1]), t2[..., 2])
    passes = t_near <= t_far
    gap = np.full(passes.shape, np.inf)
    for i in range(3):
        for j in range(3):
            if i != j:
                gap = np.fmin(gap, (t2[..., j] - t1[..., i]).astype(np.float64))
    finite = np.where(np.isfinite(t1) | np.isfinite(t2), np.fmax(np.abs(t1), np.abs(t2)), 0)
    scale = np.max(np.where(np.isfinite(finite), finite, 0), axis=-1).astype(np.float64)
    rel = np.where(np.isfinite(gap) & (scale > 0), gap / np.where(scale > 0, scale, 1), np.where(passes, np.inf, -np.inf))
    rel = np.where(passes, np.abs(rel), -np.abs(rel))             # the sign follows the decision actually taken
    return passes, rel


def _collide_block(sc, o, d, t_max):
    dt = sc.dt
    n = len(o)
    len_d = np.sqrt(_dot(d, d)).astype(np.float64)
    cols_dst, cols_valid, cols_score, cols_order = [], [], [], []
    tri = None
    if len(sc.radius):
        # RaySphere :120-146
        oc = o[:, None, :] - sc.centre[None]
        a = _dot(d, d)[:, None]
        b = 2 * _dot(oc, d[:, None, :])
        c = _dot(oc, oc) - sc.radius[None] * sc.radius[None]
        disc = b * b - 4 * a * c
        dst = (-b - np.sqrt(disc)) / (2 * a)
        valid = (disc >= 0) & (dst >= 0)
        graze = (-b / (2 * a))
        order = np.where(disc >= 0, dst, graze)
        len_oc = np.sqrt(_dot(oc, oc)).astype(np.float64)
        rel = lambda t: t.astype(np.float64) * len_d[:, None] / len_oc          # noqa: E731
        score = np.fmin(_neg_inf_for_nan((disc / (b * b)).astype(np.float64)), _neg_inf_for_nan(rel(order)))
        cols_dst.append(dst); cols_valid.append(valid); cols_score.append(score); cols_order.append(order)
    if len(sc.ref_tri):
        # RayTriangle :150-174
        e_ab, e_ac = sc.B - sc.A, sc.C - sc.A
        nv = _cross(e_ab, e_ac)
        ao = o[:, None, :] - sc.A[None]
        dao = _cross(ao, d[:, None, :])
        det = -(d @ nv.T)
        inv_det = 1 / det
        dst = _dot(ao, nv[None]) * inv_det
        u = _dot(e_ac[None], dao) * inv_det
        v = -_dot(e_ab[None], dao) * inv_det
        w = 1 - u - v
        valid = (det >= _lit("1E-6", dt)) & (dst >= 0) & (u >= 0) & (v >= 0) & (w >= 0)
        len_n, len_ao = np.sqrt(_dot(nv, nv)).astype(np.float64), np.sqrt(_dot(ao, ao)).astype(np.float64)
        conds = [(det - _lit("1E-6", dt)).astype(np.float64) / (len_d[:, None] * len_n[None]), dst.astype(np.float64) * len_d[:, None] / len_ao,
                 u.astype(np.float64), v.astype(np.float64), w.astype(np.float64)]
        if sc.mode == 0:                                                         # the chunk cull :279
            passes, box_rel = _box_condition(sc, o, d)
            valid &= passes[:, sc.ref_chunk]
            conds.append(box_rel[:, sc.ref_chunk])
        score = conds[0]
        for cnd in conds:
            score = np.fmin(_neg_inf_for_nan(score), _neg_inf_for_nan(cnd))
        tri = (u, v, w)
        cols_dst.append(dst); cols_valid.append(valid); cols_score.append(score); cols_order.append(dst)
    out = {"hit": np.zeros(n, bool), "dst": np.full(n, np.inf, dt), "hitPoint": np.zeros((n, 3), dt), "normal": np.zeros((n, 3), dt),
           "kind": np.zeros(n, np.int32), "primitive": np.full(n, -1, np.int32), "chunk": np.full(n, -1, np.int32),
           "u": np.zeros(n, dt), "v": np.zeros(n, dt), "margin": np.full(n, np.inf)}
    if not cols_dst:
        return out
    dst, valid, score, order = (np.concatenate(c, axis=1) for c in (cols_dst, cols_valid, cols_score, cols_order))
    # CalculateRayCollision :256-297: strict '<' from +inf, so the first of equal distances wins and a valid dst of +inf or NaN never does
    cand = np.where(valid & (dst < np.inf), dst, np.inf)
    win = np.argmin(cand, axis=1)
    rows = np.arange(n)
    best = cand[rows, win]
    hit = best < np.inf
    hit &= best < t_max                                                         # ray queries: only hits with dst < tMax count
    best64 = best.astype(np.float64)
    margin = np.where(hit, score[rows, win], np.inf)
    with_t_max = np.isfinite(t_max) & (cand[rows, win] < np.inf)
    margin = np.where(with_t_max, np.fmin(margin, np.abs(best64 - t_max) / np.where(best64 > 0, best64, 1)), margin)
    others = cand.astype(np.float64)
    others[rows, win] = np.inf
    second = others.min(axis=1)
    margin = np.where(hit, np.fmin(margin, (second - best64) / np.where(best64 > 0, best64, 1)), margin)
    closer = ~valid & ~(order.astype(np.float64) >= np.where(hit, best64, np.inf)[:, None])
    margin = np.fmin(margin, np.where(closer, -score, np.inf).min(axis=1))
    ns = len(sc.radius)
    is_sphere = hit & (win < ns)
    is_tri = hit & (win >= ns)
    out["hit"], out["margin"] = hit, margin
    out["dst"] = np.where(hit, best, np.inf).astype(dt)
    point = o + d * np.where(hit, best, 0)[:, None]                              # :141, :170
    out["hitPoint"] = np.where(hit[:, None], point, 0)
    out["kind"] = np.where(is_sphere, RT_HIT_SPHERE, np.where(is_tri, RT_HIT_TRIANGLE, RT_HIT_NONE)).astype(np.int32)
    normal = np.zeros((n, 3), dt)
    if is_sphere.any():
        k = win[is_sphere]
        normal[is_sphere] = _normalize(point[is_sphere] - sc.centre[k])          # :142
        out["primitive"][is_sphere] = k
    if is_tri.any():
        r = np.nonzero(is_tri)[0]
        k = win[r] - ns
        uu, vv, ww = (x[r, k] for x in tri)
        if "swap_uv" in sc.misread:
            uu, vv = vv, uu
        normal[r] = _normalize(sc.nA[k] * ww[:, None] + sc.nB[k] * uu[:, None] + sc.nC[k] * vv[:, None])      # :171
        out["primitive"][r], out["chunk"][r] = sc.ref_tri[k], sc.ref_chunk[k]
        out["u"][r], out["v"][r] = tri[0][r, k], tri[1][r, k]
    out["normal"] = normal
    return out


def _collide(sc, o, d, t_max=None):
    """CalculateRayCollision :256-297 for the rays (o[n, 3], d[n, 3]): brute force over all spheres, then all triangles of all chunks"""
    n = len(o)
    t_max = np.full(n, np.inf) if t_max is None else np.asarray(t_max, np.float64)
    prims = max(1, len(sc.radius) + len(sc.ref_tri))
    step = max(1, 600_000 // prims)
    parts = []
    with np.errstate(all="ignore"):
        for i in range(0, max(n, 1), step):
            parts.append(_collide_block(sc, o[i:i + step], d[i:i + step], t_max[i:i + step]))
    return {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}


def closest_hit(scene, rays):
    """The fields of rt_hit (include/rt.h) for the rays (an rtx.RAY array), in the scene's element type, plus `margin`.  kind / primitive
    (a sphere's index, a triangle's index in the triangle buffer) / chunk as in rt_hit; a miss has dst = +inf and 0 elsewhere."""
    w = lambda a: np.asarray(a, np.float32).astype(scene.dt)      # noqa: E731
    return _collide(scene, w(rays["origin"]).reshape(-1, 3), w(rays["direction"]).reshape(-1, 3), np.asarray(rays["tMax"], np.float64).reshape(-1))


# ---- environment -----------------------------------------------------------------------------------------------------------------
def _smoothstep(e0, e1, x):
    """HLSL smoothstep: Hermite interpolation of saturate((x - e0) / (e1 - e0)); also returns the unclamped argument"""
    raw = (x - e0) / (e1 - e0)
    t = _saturate(raw)
    return t * t * (3 - 2 * t), raw


def _environment(sc, d):
    """GetEnvironmentLight :238-251 -> (light[n, 3], margin[n])"""
    dt, p = sc.dt, sc.p
    if not p["environmentEnabled"]:
        return np.zeros((len(d), 3), dt), np.full(len(d), np.inf)
    y = d[:, 1]
    sky_s, sky_raw = _smoothstep(dt(0), _lit("0.4", dt), y)
    sky_t = np.power(sky_s, _lit("0.35", dt))
    ground_to_sky, ground_raw = _smoothstep(_lit("-0.01", dt), dt(0), y)
    sky = _lerp(p["skyColourHorizon"][:3][None], p["skyColourZenith"][:3][None], sky_t[:, None])
    sun = np.power(np.fmax(dt(0), _dot(d, p["worldSpaceLightPos0"][None])), p["sunFocus"]) * p["sunIntensity"]
    gate = np.ones(len(d), dt) if "sun_ungated" in sc.misread else (ground_to_sky >= 1).astype(dt)
    light = _lerp(p["groundColour"][:3][None], sky, ground_to_sky[:, None]) + (sun * gate)[:, None]
    margin = np.inf
    for raw in (sky_raw, ground_raw):
        margin = np.fmin(margin, np.fmin(np.abs(raw), np.abs(raw - 1)).astype(np.float64))
    return light, margin


def environment_light(params, dirs, dtype=np.float64, misread=()):
    """GetEnvironmentLight for the directions dirs[n, 3] -> (light[n, 3], margin[n])"""
    empty = np.zeros(0, [("position", "<f4", 3), ("radius", "<f4"), ("material", _MAT)])
    info = np.zeros(0, [("firstTriangleIndex", "<u4"), ("numTriangles", "<u4"), ("material", _MAT), ("boundsMin", "<f4", 3), ("boundsMax", "<f4", 3)])
    sc = Scene(params, empty, np.zeros(0, [(k, "<f4", 3) for k in ("posA", "posB", "posC", "normalA", "normalB", "normalC")]), info, dtype, misread=misread)
    with np.errstate(all="ignore"):
        return _environment(sc, np.asarray(dirs, np.float32).astype(sc.dt).reshape(-1, 3))


_MAT = [("colour", "<f4", 4), ("emissionColour", "<f4", 4), ("specularColour", "<f4", 4), ("emissionStrength", "<f4"), ("smoothness", "<f4"),
        ("specularProbability", "<f4"), ("flag", "<i4")]


# ---- the path --------------------------------------------------------------------------------------------------------------------
def _random_normal(rng, lanes, sc):
    """RandomValueNormalDistribution :207-213"""
    pi = _lit("3.1415", sc.dt) if "swap_pi" in sc.misread else _lit("3.1415926", sc.dt)
    theta = 2 * pi * rng.value(lanes)
    rho = np.sqrt(-2 * np.log(rng.value(lanes)))
    return rho * np.cos(theta)


def _random_direction(rng, lanes, sc):
    """RandomDirection :216-223"""
    x = _random_normal(rng, lanes, sc)
    y = _random_normal(rng, lanes, sc)
    z = _random_normal(rng, lanes, sc)
    return _normalize(np.stack([x, y, z], axis=-1))


def _random_point_in_circle(rng, lanes, sc):
    """RandomPointInCircle :225-230, PI = 3.1415 (:35)"""
    pi = _lit("3.1415926", sc.dt) if "swap_pi" in sc.misread else _lit("3.1415", sc.dt)
    angle = rng.value(lanes) * 2 * pi
    on_circle = np.stack([np.cos(angle), np.sin(angle)], axis=-1)
    return on_circle * np.sqrt(rng.value(lanes))[:, None]


def _mod2(x, y):
    """mod2 :232-235"""
    return x - y * np.floor(x / y)


def _material_of(sc, kind, primitive, chunk):
    """the material of every hit: the sphere's own (:271) or the chunk's (:291); returns a lookup by field name"""
    sphere = kind == RT_HIT_SPHERE
    s_idx, c_idx = np.where(sphere, primitive, 0), np.where(kind == RT_HIT_TRIANGLE, chunk, 0)

    def table(k):
        a = sc.sphere_mat[k][s_idx] if len(sc.radius) else 0
        b = sc.chunk_mat[k][c_idx] if len(sc.bmin) else 0
        return np.where(sphere if sc.sphere_mat[k].ndim == 1 else sphere[:, None], a, b)
    return table


def _checker_colour(sc, point, flag, colour, emission_colour):
    """CheckerPattern :313-317 -> (colour, is a checker material, odd cell, distance of the coordinates used to the nearest integer)"""
    checker = flag == CHECKER_PATTERN
    cell = point[:, [0, 1]] if "checker_xy" in sc.misread else point[:, [0, 2]]
    c = _mod2(np.floor(cell), sc.dt(2))
    parity = checker & ~(c[:, 0] == c[:, 1])
    edge = np.min(np.abs(cell - np.round(cell)), axis=1).astype(np.float64)
    return np.where(parity[:, None], emission_colour, colour), checker, parity, edge


def _signature(kind, prim, specular, parity, survived):
    return ((prim.astype(np.int64) + 1) << 8) | (kind.astype(np.int64) << 4) | (specular.astype(np.int64) << 2) | (parity.astype(np.int64) << 1) | survived.astype(np.int64)


SIG_PASSED_LIGHT = 3 << 4                                              # an InvisibleLightSource passed through at bounce 0


def sig_fields(sig):
    """(kind, primitive, specular, checker parity, survived) of signature entries; kind 3 = an invisible light passed through, -1 = no event"""
    s = np.asarray(sig)
    none = s < 0
    return (np.where(none, -1, (s >> 4) & 3), np.where(none, -1, (s >> 8) - 1), np.where(none, 0, (s >> 2) & 1), np.where(none, 0, (s >> 1) & 1),
            np.where(none, 0, s & 1))


def _trace(sc, o, d, rng, sample_margin, sig, flags):
    """Trace :300-352 for one sample of every pixel; o, d are [n, 3].  Returns incomingLight[n, 3]; the margins, the signatures and the set
    of branches taken are updated in place."""
    dt, p = sc.dt, sc.p
    n = len(o)
    incoming = np.zeros((n, 3), dt)
    ray_colour = np.ones((n, 3), dt)
    o, d = o.copy(), d.copy()
    alive = np.arange(n)
    for bounce in range(p["maxBounceCount"] + 1):
        if not len(alive):
            break
        h = _collide(sc, o[alive], d[alive])
        sample_margin[alive] = np.fmin(sample_margin[alive], h["margin"])
        miss = ~h["hit"]
        if miss.any():                                                  # :346-347
            lanes = alive[miss]
            light, m = _environment(sc, d[lanes])
            incoming[lanes] += light * ray_colour[lanes]
            sample_margin[lanes] = np.fmin(sample_margin[lanes], m)
            sig[lanes, bounce] = 0
            flags.add("miss")
        keep = h["hit"]
        lanes = alive[keep]
        if not len(lanes):
            break
        sphere = h["kind"][keep] == RT_HIT_SPHERE
        table = _material_of(sc, h["kind"][keep], h["primitive"][keep], h["chunk"][keep])
        flag = table("flag")
        emission_colour, specular_colour = table("emissionColour"), table("specularColour")
        point, normal = h["hitPoint"][keep], h["normal"][keep]
        colour, checker, parity, edge = _checker_colour(sc, point, flag, table("colour"), emission_colour)
        if checker.any():
            sample_margin[lanes] = np.fmin(sample_margin[lanes], np.where(checker, edge, np.inf))
            flags.add("checker")
        passed = (flag == INVISIBLE_LIGHT_SOURCE) & (bounce == 0)       # :318-322
        if passed.any():
            o[lanes[passed]] = point[passed] + d[lanes[passed]] * _lit("0.001", dt)
            sig[lanes[passed], bounce] = SIG_PASSED_LIGHT | ((h["primitive"][keep][passed].astype(np.int64) + 1) << 8)
            flags.add("passed_light")
        if ((flag == INVISIBLE_LIGHT_SOURCE) & ~passed).any():
            flags.add("light_hit_after_bounce_0")
        s = ~passed                                                     # the lanes that scatter
        lanes_s = lanes[s]
        if len(lanes_s):
            rng.scope(lanes_s, 1 + 2 * bounce)
            r = rng.value(lanes_s)
            probability = table("specularProbability")[s]
            is_specular = probability >= r                              # :325
            sample_margin[lanes_s] = np.fmin(sample_margin[lanes_s], np.abs(probability - r).astype(np.float64))
            spec = is_specular.astype(dt)
            o[lanes_s] = point[s]                                       # :327
            diffuse_dir = _normalize(normal[s] + _random_direction(rng, lanes_s, sc))
            incident = d[lanes_s]
            specular_dir = incident - 2 * _dot(normal[s], incident)[:, None] * normal[s]            # reflect(i, n) = i - 2 dot(n, i) n
            smooth = table("smoothness")[s] * (dt(1) if "smooth_no_flag" in sc.misread else spec)
            d[lanes_s] = _normalize(_lerp(diffuse_dir, specular_dir, smooth[:, None]))              # :330
            emitted = emission_colour[s] * table("emissionStrength")[s][:, None]                    # :333
            tint = _lerp(colour[s], specular_colour[s], spec[:, None])
            if "emit_after" in sc.misread:
                ray_colour[lanes_s] *= tint
                incoming[lanes_s] += emitted * ray_colour[lanes_s]
            else:
                incoming[lanes_s] += emitted * ray_colour[lanes_s]
                ray_colour[lanes_s] *= tint
            rc = ray_colour[lanes_s]
            pr = np.fmax(rc[:, 0], np.fmax(rc[:, 1], rc[:, 2]))         # :338
            r = rng.value(lanes_s)
            stop = r >= pr                                              # :339
            sample_margin[lanes_s] = np.fmin(sample_margin[lanes_s], np.abs(r - pr).astype(np.float64))
            ray_colour[lanes_s] = np.where(stop[:, None], rc, rc * (dt(1) / pr)[:, None])           # :342
            sig[lanes_s, bounce] = _signature(h["kind"][keep][s], h["primitive"][keep][s], is_specular, parity[s], ~stop)
            for name, cond in (("specular", is_specular), ("diffuse", ~is_specular), ("roulette_stop", stop), ("emissive", (emitted > 0).any(1)),
                               ("smooth_specular", is_specular & (table("smoothness")[s] > 0)), ("sphere", sphere[s]), ("triangle", ~sphere[s]),
                               ("checker_odd", parity[s]), ("checker_even", checker[s] & ~parity[s])):
                if cond.any():
                    flags.add(name)
            alive_next = np.concatenate([lanes[passed], lanes_s[~stop]])
        else:
            alive_next = lanes[passed]
        alive = np.sort(alive_next)
    return incoming


def render_frame(scene, frame, rect=None):
    """frag :356-389 for the pixel rectangle (x0, y0, x1, y1) of the full image, row 0 at the bottom (Unity's uv origin), pixel centres at
    ((x + 0.5) / W, (y + 0.5) / H).  Returns a dict: image[h, w, 4] in the element type, margin[h, w, rays] (the smallest decision margin of
    every sample), signature[h, w, rays, maxBounceCount + 1] and branches (the set of branches of Trace that were taken)."""
    sc, dt, p = scene, scene.dt, scene.p
    W, H = p["width"], p["height"]
    x0, y0, x1, y1 = rect if rect is not None else (0, 0, W, H)
    ys, xs = np.mgrid[y0:y1, x0:x1]
    xs, ys = xs.ravel(), ys.ravel()
    n, rays = len(xs), p["numRaysPerPixel"]
    with np.errstate(all="ignore"):
        uv = np.stack([(xs.astype(dt) + dt(0.5)) / dt(W), (ys.astype(dt) + dt(0.5)) / dt(H)], axis=-1)     # i.uv at the pixel's centre
        pixel_index = (ys * W + xs) & M32                                                                   # :359-361
        rng = _Rng(p["rngMode"], pixel_index, frame, dt)
        M = p["camLocalToWorld"].reshape(4, 4)
        local = np.concatenate([uv - dt(0.5), np.ones((n, 1), dt)], axis=1) * p["viewParams"][None]         # :365
        focus = (np.concatenate([local, np.ones((n, 1), dt)], axis=1) @ M.T)[:, :3]                         # :366
        cam_right, cam_up = M[:3, 0], M[:3, 1]                                                              # :367-368
        margin = np.full((n, rays), np.inf)
        sig = np.full((n, rays, p["maxBounceCount"] + 1), -1, np.int64)
        branches = set()
        philox = p["rngMode"] != 0
        S = philox_substreams(rays) if philox else 1
        part = np.zeros((S, n, 3), dt)
        lanes = np.arange(n)
        for ray_index in range(rays):
            rng.sample = ray_index
            rng.scope(lanes, 0)
            jitter = _random_point_in_circle(rng, lanes, sc) * p["defocusStrength"] / dt(W)                 # :377
            origin = p["worldSpaceCameraPos"][None] + cam_right[None] * jitter[:, :1] + cam_up[None] * jitter[:, 1:]
            jitter = _random_point_in_circle(rng, lanes, sc) * p["divergeStrength"] / dt(W)                 # :380
            target = focus + cam_right[None] * jitter[:, :1] + cam_up[None] * jitter[:, 1:]
            direction = _normalize(target - origin)
            m, s = margin[:, ray_index].copy(), sig[:, ray_index].copy()
            part[ray_index % S] += _trace(sc, origin, direction, rng, m, s, branches)                       # :384
            margin[:, ray_index], sig[:, ray_index] = m, s
        step = 1
        while step < S:                                      # the Philox mode's fixed tree: pairs (k, k + 1), then (k, k + 2), ...
            for k in range(0, S, 2 * step):
                part[k] += part[k + step]
            step *= 2
        colour = part[0] / dt(rays)                                                                         # :387
    h, w = y1 - y0, x1 - x0
    image = np.concatenate([colour, np.ones((n, 1), dt)], axis=1).reshape(h, w, 4)
    return {"image": image, "margin": margin.reshape(h, w, rays), "signature": sig.reshape(h, w, rays, -1), "branches": branches}


def camera_rays(scene, frame, sample=0, rect=None):
    """the camera ray (origin[n, 3], direction[n, 3]) of sample `sample` of every pixel in Philox mode, where a sample's draws do not depend
    on the samples before it (block 0 of the stream): what rt_render_aov's samples are"""
    sc, dt, p = scene, scene.dt, scene.p
    W, H = p["width"], p["height"]
    x0, y0, x1, y1 = rect if rect is not None else (0, 0, W, H)
    ys, xs = np.mgrid[y0:y1, x0:x1]
    xs, ys = xs.ravel(), ys.ravel()
    n = len(xs)
    with np.errstate(all="ignore"):
        uv = np.stack([(xs.astype(dt) + dt(0.5)) / dt(W), (ys.astype(dt) + dt(0.5)) / dt(H)], axis=-1)
        rng = _Rng(1, (ys * W + xs) & M32, frame, dt)
        M = p["camLocalToWorld"].reshape(4, 4)
        local = np.concatenate([uv - dt(0.5), np.ones((n, 1), dt)], axis=1) * p["viewParams"][None]
        focus = (np.concatenate([local, np.ones((n, 1), dt)], axis=1) @ M.T)[:, :3]
        lanes = np.arange(n)
        rng.sample = sample
        rng.scope(lanes, 0)
        jitter = _random_point_in_circle(rng, lanes, sc) * p["defocusStrength"] / dt(W)
        origin = p["worldSpaceCameraPos"][None] + M[:3, 0][None] * jitter[:, :1] + M[:3, 1][None] * jitter[:, 1:]
        jitter = _random_point_in_circle(rng, lanes, sc) * p["divergeStrength"] / dt(W)
        target = focus + M[:3, 0][None] * jitter[:, :1] + M[:3, 1][None] * jitter[:, 1:]
        return origin, _normalize(target - origin)


def first_surface(scene, origin, direction):
    """The first surface at which Trace scatters along each ray: the first hit, an InvisibleLightSource passed through once as at bounce 0
    (:318-322; only with a bounce left).  Returns a dict: surface (bool), albedo (the colour after the checker rule), normal, hitPoint,
    kind, primitive, margin (the smallest decision margin on the way)."""
    sc, dt = scene, scene.dt
    n = len(origin)
    out = {"surface": np.zeros(n, bool), "albedo": np.zeros((n, 3), dt), "normal": np.zeros((n, 3), dt), "hitPoint": np.zeros((n, 3), dt),
           "kind": np.zeros(n, np.int32), "primitive": np.full(n, -1, np.int32), "margin": np.full(n, np.inf)}
    o, live = origin.copy(), np.arange(n)
    with np.errstate(all="ignore"):
        for bounce in range(min(sc.p["maxBounceCount"] + 1, 2)):
            if not len(live):
                break
            h = _collide(sc, o[live], direction[live])
            out["margin"][live] = np.fmin(out["margin"][live], h["margin"])
            table = _material_of(sc, h["kind"], h["primitive"], h["chunk"])
            flag = table("flag")
            colour, checker, _, edge = _checker_colour(sc, h["hitPoint"], flag, table("colour"), table("emissionColour"))
            passed = h["hit"] & (flag == INVISIBLE_LIGHT_SOURCE) & (bounce == 0)
            surface = h["hit"] & ~passed
            lanes = live[surface]
            out["margin"][lanes] = np.fmin(out["margin"][lanes], np.where(checker[surface], edge[surface], np.inf))
            out["surface"][lanes] = True
            for k, v in (("albedo", colour), ("normal", h["normal"]), ("hitPoint", h["hitPoint"]), ("kind", h["kind"]), ("primitive", h["primitive"])):
                out[k][lanes] = v[surface]
            o[live[passed]] = h["hitPoint"][passed] + direction[live[passed]] * _lit("0.001", dt)
            live = live[passed]
    return out


def feature_frame(scene, frame):
    """One feature frame of rt_render_aov (include/rt.h; not part of the shader): per sample the first scattering surface along the sample's
    own camera ray (Philox block 0, whatever rngMode is), albedo.rgb and coverage 1, the shading normal and depth = |hitPoint - the camera
    ray's origin|, 0 on a miss; summed over the samples and divided by their number.  Returns (planes[h, w, 8], margin[h, w, rays],
    signature[h, w, rays])."""
    sc, p = scene, scene.p
    H, W, n = p["height"], p["width"], p["numRaysPerPixel"]
    total = np.zeros((H * W, 8), sc.dt)
    margin, sig = np.full((H * W, n), np.inf), np.zeros((H * W, n), np.int64)
    for sample in range(n):
        origin, d = camera_rays(sc, frame, sample)
        s = first_surface(sc, origin, d)
        q = s["hitPoint"] - origin
        row = np.concatenate([s["albedo"], np.ones((H * W, 1), sc.dt), s["normal"], np.sqrt(_dot(q, q))[:, None]], axis=1)
        total += np.where(s["surface"][:, None], row, 0)
        margin[:, sample] = s["margin"]
        sig[:, sample] = (s["primitive"].astype(np.int64) + 1) * 4 + s["kind"]
    return (total / sc.dt(n)).reshape(H, W, 8), margin.reshape(H, W, n), sig.reshape(H, W, n)


def accumulate(accum, cur, frame, dtype=np.float64):
    """Accumulate.shader:43-54: weight = 1 / (_Frame + 1); saturate(prev * (1 - weight) + cur * weight).  saturate of NaN is 0 (Direct3D's
    max(NaN, 0) = 0).  Returns the new accumulation in the element type."""
    dt = np.dtype(dtype).type
    prev, cur = np.asarray(accum, np.float32).astype(dt), np.asarray(cur, np.float32).astype(dt)
    weight = dt(1.0) / dt(frame + 1)
    with np.errstate(all="ignore"):
        return _saturate(prev * (1 - weight) + cur * weight)
