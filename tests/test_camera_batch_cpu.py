"""Per-frame cameras without a GPU: the kernel with a camera table (k_cam_stream) is in the built code object, its kernarg segment is laid
out like its struct view (csrc/rt_stream.hpp StreamCamKernArgs = {DeviceScene, FrameArgs, StreamArgs, const CamRecord*}) and it needs no
scratch; the three entry points are declared in include/rt.h, exported by the library and bound in _cabi.py."""
import os
import re
import shutil

import pytest

from test_kernarg_layout_cpu import LIB, ROOT, code_objects, kernel_metadata

EXPORTS = ("rt_render_params", "rt_submit_frame_params", "rt_multi_render_params")


def built_library():
    if not os.path.exists(LIB):
        if shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc"):
            pytest.fail("librt_mi355x.so is not built although hipcc is present: run __graft_entry__.build()")
        pytest.skip("library not built and no hipcc to build it with")
    return open(LIB, "rb").read()


def test_camera_table_kernel_is_built_and_laid_out_like_its_struct_view():
    blob = built_library()
    names = set()
    for elf in code_objects(blob):
        for k in kernel_metadata(elf):
            if "k_cam_stream" not in k[".name"]:
                continue
            assert "k_stream" not in k[".name"]
            names.add(k[".name"])
            args = k[".args"]
            by_value = [a for a in args if a[".value_kind"] == "by_value"]
            table = [a for a in args if a[".value_kind"] == "global_buffer"]
            assert len(by_value) == 3 and len(table) == 1, (k[".name"], args)
            pos = 0
            for a in by_value + table:                    # struct rule: members in order, each aligned to 8
                pos = (pos + 7) & ~7
                assert a[".offset"] == pos, (k[".name"], a)
                pos += a[".size"]
            assert table[0][".size"] == 8
            assert k[".sgpr_spill_count"] == 0 and k[".vgpr_spill_count"] == 0, k[".name"]
            assert k[".private_segment_fixed_size"] == 0, (k[".name"], "scratch")
    assert len(names) == 6, sorted(names)                 # PHILOX x f16 / f32 nodes with triangles, PHILOX without triangles


def test_entry_points_are_declared_exported_and_bound(rtx):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rt.h")).read(), flags=re.S)
    lib = rtx.load_library()
    for name in EXPORTS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in rtx._cabi.SYMBOLS
        assert getattr(lib, name).argtypes is not None, name
    assert hasattr(rtx.Tracer, "render_params") and hasattr(rtx.Tracer, "submit_frame_params")
    assert hasattr(rtx.MultiTracer, "render_params")
