"""What the compiled host (host_cpp/) sends to the C ABI, seen without a GPU: host_transcript.cpp drives every rth_* entry and every
device-facing RayTracingManager method with handles of both kinds against a recording stub (host_stub.c), and its output is compared
line for line with tests/golden/host_cpp_transcript.txt — recorded from the host as it was when every method had one copy per handle
kind, with this driver and this stub.  The properties a reader should not have to dig out of the recording are asserted one by one."""
import os
import re
import subprocess

import pytest

from test_kernarg_layout_cpu import ROOT

HOST = os.path.join(ROOT, "ray-tracing-extended_amd", "host_cpp")
GOLDEN = os.path.join(ROOT, "tests", "golden", "host_cpp_transcript.txt")


@pytest.fixture(scope="module")
def transcript(rtx, tmp_path_factory):
    from rtx_amd import unity_scene
    tmp = tmp_path_factory.mktemp("host_transcript")
    scene, stub, program = str(tmp / "scene.unity"), str(tmp / "host_stub.o"), str(tmp / "host_transcript")
    unity_scene.save_unity_scene(rtx.scenes.mesh_test_scene(32, 24), scene)
    subprocess.run(["gcc", "-O0", "-std=c11", "-c", os.path.join(ROOT, "tests", "host_stub.c"), "-o", stub], check=True)
    subprocess.run(["g++", "-O0", "-std=c++17", "-ffp-contract=off", os.path.join(ROOT, "tests", "host_transcript.cpp")] +
                   [os.path.join(HOST, f) for f in ("rt_host.cpp", "unity_loader.cpp", "rt_host_c.cpp")] + [stub, "-o", program], check=True)
    return subprocess.run([program, scene], check=True, capture_output=True, text=True).stdout.splitlines()


def sections(lines):
    """{(title, kind): lines}, in the driver's order: a section starts at '== title [kind]'"""
    found, current = {}, None
    for line in lines:
        m = re.fullmatch(r"== (.*) \[(\w*)\]", line)
        if m:
            current = found.setdefault((m.group(1), m.group(2)), [])
        else:
            current.append(line)
    return found


def kind_free(lines):
    """a section with what tells the handle kinds apart taken out: the entry prefix, the handle tag (numbered by first appearance in the
    section) and what the two create entries are given"""
    seen, out = {}, []
    for line in lines:
        line = line.replace("rt_multi_", "rt_")
        line = re.sub(r"^(rt_create null) .* ->", r"\1 ->", line)
        out.append(re.sub(r"\b(?:ctx|multi)#\d+", lambda m: "handle#%d" % seen.setdefault(m.group(0), len(seen) + 1), line))
    return out


def test_the_host_sends_what_it_sent_before_its_handle_kinds_shared_a_body(transcript):
    want = open(GOLDEN).read().splitlines()
    for i, (g, w) in enumerate(zip(transcript, want)):
        assert g == w, f"line {i + 1}"
    assert len(transcript) == len(want)


def test_both_handle_kinds_get_the_same_calls(transcript):
    found = sections(transcript)
    paired = [title for title, kind in found if kind == "ctx" and (title, "multi") in found]
    for stem in ("Denoise", "DenoiseVariance", "Temporal", "OnRenderImage, nothing changed", "rth_overlap_sphere", "rth_render_animated, device geometry",
                 "fail OverlapSphere at set_option call 2", "fail Start at reset_accum call 1", "rth entries that fail"):
        assert stem in paired, stem
    for title in paired:
        assert all(l.startswith("rt_multi_") for l in found[title, "multi"] if l.startswith("rt_")), title
        assert not any(l.startswith("rt_multi_") for l in found[title, "ctx"]), title
        assert kind_free(found[title, "ctx"]) == kind_free(found[title, "multi"]), title


def test_overlap_sphere_always_puts_both_options_back(transcript):
    seen = 0
    for (title, kind), lines in sections(transcript).items():
        # one run of option calls per OverlapSphere: it ends where another entry's line, or the driver's, follows an option call
        runs, run = [], []
        for line in lines:
            m = re.match(r"rt_(?:multi_)?set_option \w+#\d+ name=(\w+) value=(-?\d+) -> (-?\d+)", line)
            if m:
                run.append(m.groups())
            elif run and not line.startswith(("rt_closest_points", "rt_multi_closest_points", "rt_last_error", "rt_multi_last_error")):
                runs.append(run)
                run = []
        runs += [run] if run else []
        for run in runs:
            assert [(name, value) for name, value, _ in run[-2:]] == [("closest_k", "1"), ("closest_all", "0")], (title, kind, run)
            seen += 1
    assert seen == 2 * (2 + 1 + 2 + 3)          # per kind: two in the C window and one failing there, two direct, three that throw


def test_a_bad_max_results_reaches_no_entry(transcript):
    found = sections(transcript)
    for kind in ("ctx", "multi"):
        for title in ("OverlapSphere, maxResults 0", "OverlapSphere, maxResults 9"):
            assert found[title, kind] == ['OverlapSphere threw "OverlapSphere: maxResults outside 1..RT_HITS_MAX"'], (title, kind)
        lines = found["rth_overlap_sphere", kind]
        bad = lines.index('bad -> -1 error "rth_overlap_sphere: bad arguments"')
        assert lines[bad - 1].startswith("out ") and lines[bad + 1] == 'no handle -> -1 error "rth_overlap_sphere: bad arguments"'
