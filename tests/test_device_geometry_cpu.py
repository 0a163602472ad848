"""Triangles from device memory without a GPU: the boundary.  Option "device_geometry" is documented where the options are, the Python
layer has the upload on both handles and refuses before any C call where it must, the feature adds no export, and the update kernel
k_deform_update is in the gfx950 code object without scratch."""
import os
import re

import pytest

from test_camera_batch_cpu import built_library
from test_kernarg_layout_cpu import ROOT, code_objects, kernel_metadata


def header():
    return open(os.path.join(ROOT, "include", "rt.h")).read()


def test_the_option_is_documented_in_the_option_list():
    h = header()
    options = h[h.index("/* Tuning knobs"):h.index("int rt_set_option(")]
    assert re.search(r'^ \*   "device_geometry"', options, re.M), "device_geometry is not in rt_set_option's list"
    entry = options[options.index('"device_geometry"'):]
    for word in ("rt_upload_triangles", "stream", "boundsMin"):          # what the entry has to say: who reads it, ordering, whose boxes
        assert word in entry, word
    bvh = options[options.index('"device_bvh"'):options.index('"bvh_treelets"')]
    assert "device_geometry" in bvh                                       # resident triangles always take the device builder


def test_methods_exist_and_no_export_was_added(rtx):
    for cls in (rtx.Tracer, rtx.MultiTracer):
        assert callable(getattr(cls, "upload_triangles_device"))
    assert len(rtx._cabi.SYMBOLS) == 115
    assert not [s for s in rtx._cabi.SYMBOLS if "device_geometry" in s or "deform" in s]


class _NoLibrary:
    """stands where the loaded library would: any C call is a failure of the test"""
    def __getattr__(self, name):
        raise AssertionError(f"the C function {name} was reached")


def _bare(cls, **state):
    t = cls.__new__(cls)
    t._lib, t._ctx, t._m = _NoLibrary(), None, None
    for k, v in state.items():
        setattr(t, k, v)
    return t


@pytest.mark.parametrize("cls_name", ["Tracer", "MultiTracer"])
def test_python_refuses_before_any_c_call(rtx, cls_name):
    cls = getattr(rtx, cls_name)
    with pytest.raises(rtx.RtError, match="device_geometry is 0"):
        _bare(cls, _device_geometry=0).upload_triangles_device(0x7F0000001000, 4)        # the option was set to 0: never passed down
    for bad, n in ((0x7F0000001000, None), ("a string", 3), (1.5, 3), (True, 1)):
        with pytest.raises(ValueError):
            _bare(cls, _device_geometry=1).upload_triangles_device(bad, n)
    import numpy as np
    with pytest.raises(ValueError):
        _bare(cls, _device_geometry=1).upload_triangles_device(np.zeros((3, 18), np.float32))   # host memory has its own door: upload()


def test_manager_hook_skips_the_cpu_transform(rtx):
    """RayTracingManager.deviceTriangles: the chunks go up once, every frame hands the caller's tensor over, and CreateMeshes — the CPU
    transform of every triangle — runs for the first frame only"""
    calls = []

    class Backend:
        def set_params(self, p): calls.append("params")
        def upload(self, **kw): calls.append(("upload", sorted(k for k, v in kw.items() if v is not None)))
        def upload_triangles_device(self, t): calls.append(("device", t))

    mgr = rtx.scenes.mesh_test_scene(16, 8)
    mgr.backend = Backend()
    frames = iter(["pose 0", "pose 1", "pose 2"])
    mgr.deviceTriangles = lambda: next(frames)
    transforms = []
    create = mgr.CreateMeshes
    mgr.CreateMeshes = lambda: (transforms.append(1), create())[1]
    for _ in range(3):
        mgr.InitFrame()
    assert len(transforms) == 1
    assert [c for c in calls if c != "params"] == [("upload", ["meshinfo", "spheres"]), ("device", "pose 0"), ("device", "pose 1"), ("device", "pose 2")]


def test_update_kernel_is_built_without_scratch():
    found = {}
    for elf in code_objects(built_library()):
        for k in kernel_metadata(elf):
            if "k_deform_update" not in k[".name"]:
                continue
            found[k[".name"]] = (k[".vgpr_count"], k[".sgpr_count"])
            assert k[".private_segment_fixed_size"] == 0 and k[".vgpr_spill_count"] == 0 and k[".sgpr_spill_count"] == 0, (k[".name"], "scratch")
            assert k[".max_flat_workgroup_size"] == 256
            assert k[".vgpr_count"] <= 64, k[".vgpr_count"]                 # a streaming kernel: eight waves per SIMD
    print("k_deform_update (VGPRs, SGPRs):", found)
    assert len(found) == 1, sorted(found)
