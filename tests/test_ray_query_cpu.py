"""Ray queries without a GPU: the six entry points are declared in include/rt.h, bound in _cabi.py and exported by the library; rt_ray and
rt_hit have the same fields at the same offsets in the C header, the numpy dtypes, the library's rt_sizeof and the C# structs of
host_cs/RtQuery.cs; the query kernels are in the built code object with no scratch and no spills."""
import os
import re

from test_camera_batch_cpu import built_library
from test_csharp_binding_cpu import CS, _cs_structs, _layout
from test_kernarg_layout_cpu import ROOT, code_objects, kernel_metadata

EXPORTS = ("rt_trace_rays", "rt_occluded", "rt_trace_rays_device", "rt_occluded_device", "rt_multi_trace_rays", "rt_multi_occluded")


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rt.h")).read(), flags=re.S)


def test_entry_points_are_declared_exported_and_bound(rtx):
    header = _header()
    lib = rtx.load_library()
    for name in EXPORTS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in rtx._cabi.SYMBOLS
        assert getattr(lib, name).argtypes is not None, name
    for cls in (rtx.Tracer, rtx.MultiTracer):
        assert hasattr(cls, "trace_rays") and hasattr(cls, "occluded")
    assert hasattr(rtx.RayTracingManager, "Raycast")
    assert lib.rt_abi_version() == 1


def test_struct_sizes_and_header_field_order(rtx):
    lib = rtx.load_library()
    assert lib.rt_sizeof(b"rt_ray") == 32 == rtx.RAY.itemsize
    assert lib.rt_sizeof(b"rt_hit") == 64 == rtx.HIT.itemsize
    header = _header()
    for name, dt in (("rt_ray", rtx.RAY), ("rt_hit", rtx.HIT)):
        body = re.search(r"typedef struct " + name + r"\s*\{(.*?)\}\s*" + name + ";", header, re.S).group(1)
        names = []
        for decl in body.split(";"):
            decl = decl.strip()
            if decl:
                decl = re.sub(r"^\w+\s+", "", decl)
                names += [re.sub(r"\[.*?\]", "", d).strip() for d in decl.split(",")]
        assert names == list(dt.names), (name, names, dt.names)


def test_csharp_query_structs_match_the_c_abi(rtx):
    structs = _cs_structs(open(os.path.join(CS, "RtQuery.cs")).read())
    lib = rtx.load_library()
    pairs = {"RtRay": ("rt_ray", rtx.RAY), "RtHit": ("rt_hit", rtx.HIT)}
    assert set(structs) == set(pairs)
    for cs_name, (c_name, dt) in pairs.items():
        rows, size, _ = _layout(structs, cs_name)
        assert size == lib.rt_sizeof(c_name.encode()) == dt.itemsize, (cs_name, size)
        assert [r[0] for r in rows] == list(dt.names), (cs_name, rows)
        for field, off, nbytes in rows:
            assert off == dt.fields[field][1] and nbytes == dt.fields[field][0].itemsize, (cs_name, field, off, nbytes)


def test_csharp_backend_queries_use_declared_imports():
    text = open(os.path.join(CS, "RtBackend.cs")).read()
    native = open(os.path.join(CS, "RtNative.cs")).read()
    available = set(re.findall(r"static\s+(?:extern\s+)?[\w<>\[\]]+\s+(\w+)\s*[<(]", native))
    used = set(re.findall(r"RtNative\.(\w+)", text)) - {"cs"}
    assert used <= available | {"UploadCall"}, used - available
    for name in ("rt_trace_rays", "rt_occluded", "rt_multi_trace_rays", "rt_multi_occluded"):
        assert name in used, name
    assert re.search(r"public\s+bool\s+Raycast\s*\(\s*Vector3\s+origin,\s*Vector3\s+direction,\s*float\s+maxDistance,\s*out\s+RtHit\s+hit\s*\)", text)
    assert re.search(r"public\s+bool\s+Occluded\s*\(", text)


def test_query_kernels_are_built_without_scratch_or_spills():
    blob = built_library()
    names = set()
    for elf in code_objects(blob):
        for k in kernel_metadata(elf):
            if "k_ray_query" not in k[".name"] and "k_query_origin_bound" not in k[".name"]:
                continue
            assert not any(s in k[".name"] for s in ("k_trace", "k_stream", "k_cam_stream")), k[".name"]
            names.add(k[".name"])
            assert k[".sgpr_spill_count"] == 0 and k[".vgpr_spill_count"] == 0, k[".name"]
            assert k[".private_segment_fixed_size"] == 0, (k[".name"], "scratch")
    assert len([n for n in names if "k_ray_query" in n]) == 4, sorted(names)      # closest / any x f16 / f32 nodes
    assert any("k_query_origin_bound" in n for n in names), sorted(names)
