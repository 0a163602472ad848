"""What the Python binding looks like from outside, and what it says to the C side — both written as plain JSON-able data.

  surface(rtx)      restype / argtypes of every C entry, the public names of the two binding modules, the public attributes and
                    signatures of Tracer, MultiTracer and CppScene, and the record dtypes
  transcript(rtx)   every public method of the three classes driven once on handles that were never created: `_lib` is a Recorder
                    whose entries log their arguments and return 0, the handle is a dummy integer

tests/golden/make_fixtures.py wrote both down from the binding as it was before its near-copies were folded together
(cabi_surface.json, cabi_transcript.json); tests/test_cabi_surface_cpu.py holds the binding to them.  No GPU is touched: surface()
only dlopens the libraries, transcript() loads nothing.
"""
import ctypes
import hashlib
import inspect

import numpy as np

CTX, MULTI, SCENE = 0x1000, 0x2000, 0x3000          # the dummy handles
W, H, N_RAYS = 16, 8, 3

# the entries of librt_host.so that host_cpp_binding declares
HOST_SYMBOLS = ["rth_load_unity", "rth_last_error", "rth_free", "rth_build", "rth_copy", "rth_render", "rth_render_multi",
                "rth_render_animated", "rth_trace_radiance", "rth_gather", "rth_visibility", "rth_closest_points", "rth_raycast_all",
                "rth_split_mesh", "rth_split_info", "rth_split_triangles"]

# ---- surface -------------------------------------------------------------------------------------------------------


def _ctype_name(t):
    return None if t is None else t.__name__


def _signatures(lib, names):
    out = {}
    for n in names:
        f = getattr(lib, n)
        out[n] = {"restype": _ctype_name(f.restype),
                  "argtypes": "none set" if f.argtypes is None else [_ctype_name(a) for a in f.argtypes]}
    return out


def _public(obj):
    return sorted(n for n in dir(obj) if not n.startswith("_"))


def _class_surface(cls):
    out = {}
    for n in _public(cls) + [d for d in ("__init__", "__enter__", "__exit__", "__del__") if getattr(cls, d, None) is not getattr(object, d, None)]:
        a = inspect.getattr_static(cls, n)
        f = getattr(cls, n)
        if callable(f):
            doc = inspect.getdoc(f)
            out[n] = {"signature": str(inspect.signature(f)), "kind": type(a).__name__,
                      "doc_sha1": None if doc is None else hashlib.sha1(doc.encode()).hexdigest()}
        else:
            out[n] = {"attribute": type(a).__name__}
    return out


def _jsonable(x):
    if isinstance(x, (list, tuple)):
        return [_jsonable(v) for v in x]
    return x


def surface(rtx):
    cabi, hcb = rtx._cabi, rtx.host_cpp_binding
    return {
        "symbols": sorted(cabi.SYMBOLS),                # (a set with a count: nothing reads their order)
        "signatures": _signatures(cabi.load_library(), cabi.SYMBOLS),
        "host_signatures": _signatures(hcb.load_host_library(), HOST_SYMBOLS),
        "module_names": {"_cabi": _public(cabi), "host_cpp_binding": _public(hcb)},
        "classes": {"Tracer": _class_surface(cabi.Tracer), "MultiTracer": _class_surface(cabi.MultiTracer),
                    "CppScene": _class_surface(hcb.CppScene)},
        "dtypes": {n: _jsonable(getattr(cabi, n).descr) for n in _public(cabi) if isinstance(getattr(cabi, n), np.dtype)},
    }


# ---- transcript ----------------------------------------------------------------------------------------------------

_QUERIES = {"trace_rays": None, "occluded": None, "closest_points": None, "trace_radiance": 3, "gather": 3, "visibility": 3, "trace_hits": 3}
# records behind a pointer argument that the log shows as bytes: entry -> (argument, record size, argument holding the count or None)
_SHOWN = {}
for _stem, _at in _QUERIES.items():
    for _name in ("rt_" + _stem, "rt_multi_" + _stem):
        _SHOWN[_name] = [(1, 32, 2)] + ([(_at, 32, None)] if _at else [])
for _stem in ("denoise", "temporal", "denoise_temporal", "denoise_variance"):
    for _name in ("rt_" + _stem, "rt_multi_" + _stem):
        _SHOWN[_name] = [(1, 32, None)]
for _stem, _at in {"trace_radiance": 5, "gather": 5, "visibility": 5}.items():
    _SHOWN["rth_" + _stem] = [(3, 32, 4), (_at, 32, None)]
_SHOWN["rth_closest_points"] = [(3, 32, 4)]


class Recorder:
    """stands where a loaded library would: every attribute is an entry that logs its call and returns 0 (or what `returns` says)"""

    def __init__(self, params_size, returns=None, fail=None):
        self.log, self.returns, self.fail = [], dict(returns or {}), dict(fail or {})
        self._shown = dict(_SHOWN)
        for n in ("rt_set_params", "rt_multi_set_params"):
            self._shown[n] = [(1, params_size, None)]
        self._shown["rt_submit_frame_params"] = [(2, params_size, None)]
        for n in ("rt_render_params", "rt_multi_render_params"):
            self._shown[n] = [(3, params_size, 2)]

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)

        def entry(*args):
            shown = {at: (size, count) for at, size, count in self._shown.get(name, ())}
            row = []
            for i, a in enumerate(args):
                if a is None or isinstance(a, (int, float)):
                    row.append(a)
                elif isinstance(a, bytes):
                    row.append("bytes:" + a.decode())
                elif i in shown:
                    size, count = shown[i]
                    row.append("record:" + ctypes.string_at(ctypes.cast(a, ctypes.c_void_p), size * (args[count] if count is not None else 1)).hex())
                elif isinstance(a, ctypes.Array):
                    row.append("array:" + ",".join(str(v) for v in a))
                else:
                    row.append("pointer")
            self.log.append({"call": name, "nargs": len(args), "args": row})
            if name in self.fail:
                return self.fail[name]
            r = self.returns.get(name, 0)
            return r(*args) if callable(r) else r
        entry.__name__ = name
        setattr(self, name, entry)
        return entry


def _describe(r):
    if isinstance(r, np.ndarray):
        return {"type": "ndarray", "dtype": str(r.dtype) if r.dtype.names is None else _jsonable(r.dtype.descr), "shape": list(r.shape)}
    if isinstance(r, dict):
        return {"type": "dict", "items": {k: _describe(v) for k, v in r.items()}, "order": list(r)}
    if isinstance(r, (list, tuple)):
        return {"type": type(r).__name__, "items": [_describe(v) for v in r]}
    return {"type": type(r).__name__}


def _names_of(fn):
    """the public names under which the class of a bound method holds the function that is about to run (an alias is the same function)"""
    if not inspect.ismethod(fn):
        return []
    cls = type(fn.__self__)
    return sorted(n for n in dir(cls) if not n.startswith("_") and inspect.getattr_static(cls, n) is fn.__func__)


class _Driver:
    def __init__(self, lib):
        self.lib, self.out = lib, []

    def __call__(self, label, fn, *args, zeroed=False, **kw):
        at = len(self.lib.log)
        step = {"step": label, "methods": _names_of(fn)}
        try:
            r = fn(*args, **kw)
            step["result"] = _describe(r)
            if zeroed:
                step["zeroed"] = not np.ascontiguousarray(r).view(np.uint8).any()
        except Exception as e:                                                  # the text of every refusal is part of the surface
            step["raised"] = [type(e).__name__, str(e)]
        step["calls"] = self.lib.log[at:]
        self.out.append(step)


def _inputs(rtx):
    c = rtx._cabi
    p = np.zeros((), c.PARAMS)
    p["width"], p["height"], p["maxBounceCount"], p["numRaysPerPixel"] = W, H, 2, 5
    run = np.zeros(2, c.PARAMS)
    run[:] = p
    run["numRaysPerPixel"] = (6, 7)
    rays = np.arange(N_RAYS * 8, dtype=np.float32).reshape(N_RAYS, 8)
    return p, run, rays


def _queries(d, o, rtx, multi):
    c = rtx._cabi
    _, _, rays = _inputs(rtx)
    d("trace_rays", o.trace_rays, rays, zeroed=True)
    d("trace_rays(RAY array)", o.trace_rays, rays.view(c.RAY).reshape(-1), zeroed=True)
    d("trace_rays(bad shape)", o.trace_rays, np.zeros((3, 7), np.float32))
    d("occluded", o.occluded, rays, zeroed=True)
    d("trace_radiance", o.trace_radiance, rays, zeroed=True)
    d("trace_radiance(samples)", o.trace_radiance, rays, samples=4, seed=9, first_index=2, zeroed=True)
    d("trace_radiance(seed alone)", o.trace_radiance, rays, seed=9)
    d("gather", o.gather, rays, zeroed=True)
    d("gather(samples, cosine)", o.gather, rays, samples=4, seed=1, mode=c.GATHER_COSINE, zeroed=True)
    d("gather(samples, sh9)", o.gather, rays, samples=4, first_index=3, mode=c.GATHER_SH9, zeroed=True)
    d("gather(sh9, samples of the params)", o.gather, rays, mode=c.GATHER_SH9, zeroed=True)
    d("visibility", o.visibility, rays, zeroed=True)
    d("visibility(samples, cosine)", o.visibility, rays, samples=4, seed=1, mode=c.VIS_COSINE, zeroed=True)
    d("visibility(sh9)", o.visibility, rays, mode=c.VIS_SH9, zeroed=True)
    d("visibility(samples, distance)", o.visibility, rays, samples=4, mode=c.VIS_DISTANCE, zeroed=True)
    d("closest_points", o.closest_points, rays, zeroed=True)
    d("trace_hits", o.trace_hits, rays, max_hits=2, zeroed=True)
    d("trace_hits(defaults)", o.trace_hits, rays, zeroed=True)
    d("trace_hits(both sides, count all)", o.trace_hits, rays, 2, both_sides=True, count_all=True, zeroed=True)
    d("trace_hits(max_hits 0)", o.trace_hits, rays, max_hits=0)
    d("trace_hits(max_hits 9)", o.trace_hits, rays, max_hits=9)
    if not multi:           # arrays through the aliases take the host entries
        d("visibility_device", o.visibility_device, rays, samples=4, zeroed=True)
        d("closest_points_device", o.closest_points_device, rays, zeroed=True)
        d("trace_hits_device", o.trace_hits_device, rays, max_hits=2, zeroed=True)
        d("trace_hits_device(max_hits 9)", o.trace_hits_device, rays, max_hits=9)


def _filters(d, o):
    d("denoise", o.denoise)
    d("denoise(iterations)", o.denoise, iterations=2)
    d("denoise(unknown)", o.denoise, sigma=1.0)
    d("denoise_info", o.denoise_info)
    d("temporal", o.temporal)
    d("temporal(maxHistory)", o.temporal, maxHistory=8)
    d("temporal(unknown)", o.temporal, iterations=2)
    d("temporal_info", o.temporal_info)
    d("denoise_temporal", o.denoise_temporal)
    d("denoise_temporal(sigmaDepth)", o.denoise_temporal, sigmaDepth=0.25)
    d("denoise_temporal(unknown)", o.denoise_temporal, source=1)
    d("denoise_info after denoise_temporal", o.denoise_info)
    d("denoise_variance", o.denoise_variance)
    d("denoise_variance(source)", o.denoise_variance, source=1)
    d("denoise_variance(unknown)", o.denoise_variance, sigmaColour=1.0)
    d("reset_temporal", o.reset_temporal)
    d("temporal_info after reset", o.temporal_info)
    for name in ("read_denoised", "read_denoised_display", "read_temporal", "read_temporal_history", "read_temporal_display", "read_variance"):
        d(name, getattr(o, name))


def _geometry(d, o, rtx):
    c = rtx._cabi
    d("upload(all)", o.upload, spheres=np.zeros(2, c.SPHERE), triangles=np.zeros(3, c.TRIANGLE), meshinfo=np.zeros(1, c.MESHINFO))
    d("upload(triangles)", o.upload, triangles=np.zeros(4, c.TRIANGLE))
    d("upload()", o.upload)
    d("upload_triangles_device(pointer)", o.upload_triangles_device, 0x7F0000001000, 3)
    d("set_option", o.set_option, "sort", 1)
    d("set_option(device_geometry 0)", o.set_option, "device_geometry", 0)
    d("upload_triangles_device(refused)", o.upload_triangles_device, 0x7F0000001000, 3)
    d("upload_local_meshes", o.upload_local_meshes, np.zeros(3, c.TRIANGLE), np.zeros(2, c.LOCAL_CHUNK), 1)
    d("set_mesh_transforms", o.set_mesh_transforms, np.zeros(1, c.MESH_TRANSFORM))


def _drive_tracer(rtx):
    c = rtx._cabi
    p, run, rays = _inputs(rtx)
    lib = Recorder(c.PARAMS.itemsize)
    t = object.__new__(c.Tracer)
    t._lib, t._ctx = lib, CTX
    d = _Driver(lib)
    d("set_params", t.set_params, p)
    _geometry(d, t, rtx)
    d("read_world_geometry", t.read_world_geometry)
    d("read_accum", t.read_accum)
    d("set_rows", t.set_rows, 2, 4)
    d("read_accum after set_rows", t.read_accum)
    d("read_display after set_rows", t.read_display)
    d("read_denoised after set_rows", t.read_denoised)
    d("set_bands", t.set_bands, 0, 2)
    d("read_last_frame after set_bands", t.read_last_frame)
    d("set_bands(height)", t.set_bands, 1, 2, 20)
    d("read_aov after set_bands", t.read_aov, c.RT_AOV_NORMAL_DEPTH)
    d("set_rows(whole)", t.set_rows, 0, H)
    d("set_stream", t.set_stream, 0x5000)
    _queries(d, t, rtx, False)
    for name in ("radiance_info", "gather_info", "visibility_info", "closest_info", "hits_info", "aov_info", "vdenoise_info", "stats"):
        d(name, getattr(t, name))
    d("render_frame", t.render_frame, 3)
    d("render", t.render, 0, 2)
    d("render_counting", t.render_counting, 1, 2)
    d("render_frame_flat", t.render_frame_flat, 4)
    d("reset_accum", t.reset_accum)
    d("submit_frame", t.submit_frame, 5)
    d("wait", t.wait)
    d("write_accum", t.write_accum, np.zeros((H, W, 4), np.float32), 7)
    d("read_last_frame", t.read_last_frame)
    d("read_display", t.read_display)
    d("copy_accum_to_device", t.copy_accum_to_device, 0x6000, 512)
    d("read_bvh", t.read_bvh)
    d("read_bvh_order", t.read_bvh_order)
    d("render_aov", t.render_aov, 0, 2)
    d("read_aov", t.read_aov, c.RT_AOV_ALBEDO)
    d("copy_aov_to_device", t.copy_aov_to_device, 1, 0x6000, 512)
    d("reset_aov", t.reset_aov)
    _filters(d, t)
    for name in ("copy_denoised_to_device", "copy_temporal_to_device", "copy_variance_to_device"):
        d(name, getattr(t, name), 0x6000, 512)
    d("render_params", t.render_params, 3, run)
    d("gather(sh9) after render_params", t.gather, rays, mode=c.GATHER_SH9, zeroed=True)
    run[1]["numRaysPerPixel"], run[1]["width"] = 9, 24
    d("submit_frame_params", t.submit_frame_params, 6, run[1])
    d("gather(sh9) after submit_frame_params", t.gather, rays, mode=c.GATHER_SH9, zeroed=True)
    d("read_accum after submit_frame_params", t.read_accum)
    d("render_params(empty)", t.render_params, 0, np.zeros(0, c.PARAMS))
    d("with", lambda: t.__enter__() is t)
    lib.fail.update(rt_render=-2, rt_set_option=-3, rt_trace_hits=-4, rt_get_stats=-5, rt_read_accum=-6, rt_denoise=-7)
    lib.returns["rt_last_error"] = b"said the library"
    d("render failing", t.render, 0, 1)
    d("set_option failing", t.set_option, "sort", 2)
    d("trace_hits failing", t.trace_hits, rays, 2)
    d("stats failing", t.stats)
    d("read_accum failing", t.read_accum)
    d("denoise failing", t.denoise)
    d("close", t.close)
    d("close again", t.close)
    d("handle after close", lambda: t._ctx)
    return d.out


def _drive_multi(rtx):
    c = rtx._cabi
    p, run, rays = _inputs(rtx)
    lib = Recorder(c.PARAMS.itemsize, returns={"rt_multi_count": 2, "rt_multi_context": lambda m, i: 0x4000 + i})
    m = object.__new__(c.MultiTracer)
    m._lib, m._m, m._shape = lib, MULTI, None           # (_shape: as __init__ leaves it before set_params)
    d = _Driver(lib)
    d("gather(sh9) before set_params", m.gather, rays, mode=c.GATHER_SH9)
    for name in ("read_accum", "read_display", "read_denoised", "read_denoised_display", "read_temporal", "read_temporal_history",
                 "read_temporal_display", "read_variance", "temporal_info"):
        d(name + " before set_params", getattr(m, name))
    d("read_aov before set_params", m.read_aov, c.RT_AOV_ALBEDO)
    d("set_params", m.set_params, p)
    d("count", m.count)
    _geometry(d, m, rtx)
    _queries(d, m, rtx, True)
    d("render", m.render, 0, 2)
    d("reset_accum", m.reset_accum)
    d("read_accum", m.read_accum)
    d("read_display", m.read_display)
    d("write_accum", m.write_accum, np.zeros((H, W, 4), np.float32), 7)
    d("render_aov", m.render_aov, 0, 2)
    d("read_aov", m.read_aov, c.RT_AOV_NORMAL_DEPTH)
    d("reset_aov", m.reset_aov)
    d("aov_info", m.aov_info)
    d("denoise_info before denoise", m.denoise_info)
    _filters(d, m)
    d("stats", m.stats)
    d("info", m.info)
    run["height"] = 12
    d("render_params", m.render_params, 3, run)
    d("gather(sh9) after render_params", m.gather, rays, mode=c.GATHER_SH9, zeroed=True)
    d("read_accum after render_params", m.read_accum)
    d("render_params(empty)", m.render_params, 0, np.zeros(0, c.PARAMS))
    d("with", lambda: m.__enter__() is m)
    lib.fail.update(rt_multi_render=-2, rt_multi_set_option=-3, rt_multi_trace_hits=-4, rt_multi_get_stats=-5, rt_get_aov_info=-6,
                    rt_multi_temporal=-7)
    lib.returns["rt_multi_last_error"] = b"said the handle"
    d("render failing", m.render, 0, 1)
    d("set_option failing", m.set_option, "sort", 2)
    d("trace_hits failing", m.trace_hits, rays, 2)
    d("stats failing", m.stats)
    d("aov_info failing", m.aov_info)
    d("temporal failing", m.temporal)
    d("temporal_info after a failed call", m.temporal_info)
    d("close", m.__exit__, None, None, None)
    d("close again", m.close)
    d("handle after close", lambda: m._m)
    return d.out


def _drive_scene(rtx):
    hcb = rtx.host_cpp_binding
    _, _, rays = _inputs(rtx)
    lib = Recorder(rtx._cabi.PARAMS.itemsize, returns={"rth_last_error": b"said the host", "rth_raycast_all": 2})
    s = object.__new__(hcb.CppScene)
    s._L, s._h, s.width, s.height = lib, SCENE, W, H
    d = _Driver(lib)
    q, shift = (0.0, 0.0, 0.0, 1.0), (0.5, 0.0, 0.25)
    for devices in ((), (1, 0)):
        kw = {"devices": devices} if devices else {"device": 2}
        d(f"trace_radiance {kw}", s.trace_radiance, rays, **kw, zeroed=True)
        d(f"trace_radiance(samples) {kw}", s.trace_radiance, rays, samples=4, seed=9, first_index=2, **kw, zeroed=True)
        d(f"gather {kw}", s.gather, rays, **kw, zeroed=True)
        d(f"gather(sh9) {kw}", s.gather, rays, samples=4, mode=1, **kw, zeroed=True)
        d(f"gather(sh9, no samples) {kw}", s.gather, rays, mode=1, **kw)
        d(f"visibility {kw}", s.visibility, rays, **kw, zeroed=True)
        d(f"visibility(sh9) {kw}", s.visibility, rays, mode=1, **kw, zeroed=True)
        d(f"visibility(samples, distance) {kw}", s.visibility, rays, samples=4, mode=2, **kw, zeroed=True)
        d(f"closest_points {kw}", s.closest_points, rays, **kw, zeroed=True)
        d(f"raycast_all {kw}", s.raycast_all, (0, 1, 2), (0, 0, 1), 50.0, 3, True, **kw)
        d(f"raycast_all(max_hits 0) {kw}", s.raycast_all, (0, 1, 2), (0, 0, 1), max_hits=0, **kw)
        d(f"render_animated {kw}", s.render_animated, 2, 3, q, shift, device_geometry=bool(devices), **kw)
    bad = np.zeros((3, 7), np.float32)                  # wrong in two ways: the rays are refused first
    d("trace_radiance(bad rays, seed alone)", s.trace_radiance, bad, seed=9)
    d("gather(bad rays, sh9 without samples)", s.gather, bad, mode=1)
    d("visibility(bad rays)", s.visibility, bad, mode=1)
    d("closest_points(bad rays)", s.closest_points, bad)
    d("render", s.render, 2)
    d("render(device)", s.render, 2, 1)
    d("render_multi", s.render_multi, 2, [0, 1, 0])
    d("build_buffers", s.build_buffers)
    d("counts", lambda: dict(s.counts))
    for name in ("rth_build", "rth_render", "rth_render_multi", "rth_render_animated", "rth_trace_radiance", "rth_gather", "rth_visibility",
                 "rth_closest_points"):
        lib.fail[name] = 1
    lib.fail["rth_raycast_all"] = -1
    d("build_buffers failing", s.build_buffers)
    d("render failing", s.render, 2)
    d("render_multi failing", s.render_multi, 2, [0, 1])
    d("render_animated failing", s.render_animated, 2, 3, q, shift)
    d("trace_radiance failing", s.trace_radiance, rays)
    d("gather failing", s.gather, rays)
    d("visibility failing", s.visibility, rays)
    d("closest_points failing", s.closest_points, rays)
    d("raycast_all failing", s.raycast_all, (0, 1, 2), (0, 0, 1))
    d("close", s.close)
    d("close again", s.close)
    return d.out


def transcript(rtx):
    return {"Tracer": _drive_tracer(rtx), "MultiTracer": _drive_multi(rtx), "CppScene": _drive_scene(rtx)}


# every public method the transcript does not drive, and why (at most five; anything else missing fails the test)
NOT_DRIVEN = {}


def driven(transcript_):
    """class -> the public methods its steps ran"""
    return {cls: {n for s in steps for n in s["methods"]} for cls, steps in transcript_.items()}
