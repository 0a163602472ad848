"""tests/dynamic_fuzz.py without a GPU: the generator is a function of the seed and reaches every class it names; expected_world — the
reference's marshal as a literal loop — is what host.py and the compiled host marshal, byte for byte, NaN, infinite and zero-scaled
vertices included; it lies within a float64 twin where the inputs are finite; the box rule is pinned by hand cases; and the oracle's
search tree returns its loop's image on every world the steps make, chunk boxes with NaN faces among them."""
import os

import numpy as np
import pytest

import dynamic_fuzz as df
from dynamic_fuzz import nan_box_scene           # noqa: F401 (tests/test_gpu_geometry.py takes it from here)
from test_gpu_fuzz import random_scene

SEEDS = range(12)                        # the default seeds of tests/test_gpu_dynamic_fuzz.py
NAN = np.float32(np.nan)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def cases(rtx):
    return {seed: df.dynamic_case(rtx, seed) for seed in SEEDS}


@pytest.fixture(scope="module")
def replays(cases):
    return {seed: df.replay(case) for seed, case in cases.items()}


def _bytes(x):
    if isinstance(x, dict):
        return b"".join(_bytes(x[k]) for k in sorted(x))
    if isinstance(x, (list, tuple)):
        return b"".join(_bytes(v) for v in x)
    return np.asarray(x).tobytes() if not isinstance(x, str) else x.encode()


def test_the_generator_is_a_function_of_the_seed_alone(rtx, cases):
    for seed in (0, 5, 10):
        before = _bytes(list(random_scene(rtx, seed)))
        again = df.dynamic_case(rtx, seed)
        assert _bytes(list(again)) == _bytes(list(cases[seed])) and again.knobs == cases[seed].knobs and again.kernel == cases[seed].kernel
        df.replay(again)
        assert _bytes(list(random_scene(rtx, seed))) == before, "random_scene's buffers changed"
        params, spheres, tris, chunks, n_meshes, steps = again
        assert int(params["width"]) <= 32 and int(params["height"]) <= 24 and int(params["numRaysPerPixel"]) <= 2 and int(params["maxBounceCount"]) <= 3
        assert 3 <= len(chunks) <= 8 and 1 <= n_meshes <= 4 and 5 <= len(steps) <= 7
        assert (chunks["meshIndex"] == np.arange(len(chunks)) % n_meshes).all()
        covered = np.zeros(len(tris), int)
        for c in chunks:
            covered[int(c["firstTriangleIndex"]):int(c["firstTriangleIndex"]) + int(c["numTriangles"])] += 1
        assert (covered == 1).all()                               # every triangle in exactly one chunk


def test_reach_of_the_default_seeds(cases):
    """every pose class, every deformation class and each of the six ordered door changes at least twice; every seed goes through two
    doors, every third through all three"""
    pose, deform, pairs = {}, {}, {}
    for seed, case in cases.items():
        doors = [s["door"] for s in case[5] if s["door"] != "camera"]
        assert len(set(doors)) >= 2 and (seed % 3 or len(set(doors)) == 3), (seed, doors)
        for a, b in zip(doors, doors[1:]):
            if a != b:
                pairs[(a, b)] = pairs.get((a, b), 0) + 1
        for s in case[5]:
            book = pose if s["door"] == "transforms" else deform if s["door"] == "deform" else None
            if book is not None:
                book[s["kind"]] = book.get(s["kind"], 0) + 1
    assert all(pose.get(k, 0) >= 2 for k in df.POSE_CLASSES), pose
    assert all(deform.get(k, 0) >= 2 for k in df.DEFORM_CLASSES), deform
    assert all(pairs.get((a, b), 0) >= 2 for a in df.DOORS for b in df.DOORS if a != b), pairs
    assert any(s["door"] == "camera" for case in cases.values() for s in case[5])
    assert {s["frames"] for case in cases.values() for s in case[5] if s["door"] == "reupload"} == {0, 1, 20}


# ---- the box rule by hand ------------------------------------------------------------------------------------------------------------

# (what, the coordinates a chunk's vertices take on one axis in buffer order, min, max after the loop) — dyadic numbers throughout
HAND = [("NaN first", [NAN, 1.0, 2.0], 1.0, 2.0),                     # the start is NaN; 1 replaces it; 2 is no smaller
        ("NaN in the middle", [1.0, NAN, 2.0], 2.0, 2.0),             # the NaN replaces 1, 2 replaces the NaN: the 1 is forgotten
        ("NaN last", [1.0, 2.0, NAN], NAN, NAN),
        ("all NaN", [NAN, NAN, NAN], NAN, NAN),
        ("NaN in the middle of two triangles", [4.0, 0.5, NAN, 3.0, 8.0, 2.0], 2.0, 8.0),
        ("one triangle", [3.0, 1.0, 2.0], 1.0, 3.0),
        ("one triangle, negative", [-0.5, -4.0, 0.25], -4.0, 0.25)]


def _same(got, want):
    return np.asarray(got, np.float32).tobytes() == np.asarray(want, np.float32).tobytes() or (np.isnan(got).all() and np.isnan(want).all())


@pytest.mark.parametrize("what,seq,lo,hi", HAND, ids=[h[0] for h in HAND])
def test_box_rule_hand_cases(rtx, what, seq, lo, hi):
    """the literal loop, host.py's closed form of it and host.py's marshal (identity pose: the rotation multiplies the other coordinates
    by zero, so a NaN vertex is NaN on every axis and the sequence goes on all three)"""
    pts = np.repeat(np.asarray(seq, np.float32)[:, None], 3, 1)
    got = df.box_rule(pts)
    assert _same(got[0], [lo] * 3) and _same(got[1], [hi] * 3), (what, got)
    assert _same(rtx.host._running_extreme(pts[:, 0], np.less), lo) and _same(rtx.host._running_extreme(pts[:, 0], np.greater), hi)
    tris = np.zeros(len(seq) // 3, rtx.TRIANGLE)
    tris["posA"], tris["posB"], tris["posC"] = pts[0::3], pts[1::3], pts[2::3]
    h = rtx.host
    wc = h.RayTracedMesh._UpdateWorldChunkFromLocal(h.MeshChunk(tris, None), np.zeros(3, np.float32), np.float32([0, 0, 0, 1]), np.ones(3, np.float32))
    want = df.bounds_round_trip(np.float32([lo] * 3), np.float32([hi] * 3))
    assert _same(wc.bounds.min, want[0]) and _same(wc.bounds.max, want[1]), (what, wc.bounds)


def test_box_rule_signed_zeros(rtx):
    """equal values: the later one stays (a < b and a > b are both false), so the zero's sign is the last zero's"""
    for seq, lo, hi in (([0.0, -0.0, 0.0], 0.0, 0.0), ([0.0, 0.0, -0.0], -0.0, -0.0), ([-0.0, 1.0, 0.0], 0.0, 1.0), ([0.0, -1.0, -0.0], -1.0, -0.0)):
        pts = np.repeat(np.asarray(seq, np.float32)[:, None], 3, 1)
        got = df.box_rule(pts)
        assert got[0].tobytes() == np.float32([lo] * 3).tobytes() and got[1].tobytes() == np.float32([hi] * 3).tobytes(), (seq, got)
        assert np.float32(rtx.host._running_extreme(pts[:, 0], np.less)).tobytes() == np.float32(lo).tobytes()
        assert np.float32(rtx.host._running_extreme(pts[:, 0], np.greater)).tobytes() == np.float32(hi).tobytes()


@pytest.mark.parametrize("scene", ["mesh_test", "Knight", "config3"])
def test_finite_scenes_keep_their_boxes(rtx, scene):
    """the rule the marshal had before (numpy's min / max over the chunk) gives the same bytes wherever no vertex is NaN"""
    from rtx_amd import unity_scene
    mgr = rtx.scenes.mesh_test_scene(16, 8) if scene == "mesh_test" else rtx.scenes.config3(16, 9) if scene == "config3" \
        else unity_scene.load_scene_npz(os.path.join(GOLDEN, "scenes", "Knight.npz"), 16, 9)
    _, _, tris, infos = mgr.build_buffers()
    for mi in infos:
        t = tris[int(mi["firstTriangleIndex"]):int(mi["firstTriangleIndex"]) + int(mi["numTriangles"])]
        p = np.concatenate([t["posA"], t["posB"], t["posC"]])
        lo, hi = df.bounds_round_trip(p.min(0), p.max(0))
        assert lo.tobytes() == mi["boundsMin"].tobytes() and hi.tobytes() == mi["boundsMax"].tobytes()


# ---- expected_world against the hosts ------------------------------------------------------------------------------------------------

def _pose_steps(case):
    return [(i, s) for i, s in enumerate(case[5]) if s["door"] == "transforms"]


def test_expected_world_is_host_py_byte_for_byte(cases, replays):
    for seed, case in cases.items():
        for i, step in _pose_steps(case):
            want_tris, want_infos = replays[seed][i]["tris"], replays[seed][i]["infos"]
            assert df.expected_world(case, i)[0].tobytes() == want_tris.tobytes()
            mgr, by_mesh = df.manager_for(case, step["xf"])
            with np.errstate(all="ignore"):
                for m, mesh in enumerate(mgr.meshes):
                    for ch, wc in zip(by_mesh.get(m, []), mesh.GetSubMeshes()):
                        a, n = int(ch["firstTriangleIndex"]), int(ch["numTriangles"])
                        k = int(np.flatnonzero(case[3]["firstTriangleIndex"] == a)[0])
                        what = f"seed {seed} step {i} ({step['kind']}) chunk {k}"
                        assert wc.triangles.tobytes() == want_tris[a:a + n].tobytes(), what + ": triangles"
                        assert wc.bounds.min.tobytes() == want_infos[k]["boundsMin"].tobytes(), what + f": boundsMin {wc.bounds.min} {want_infos[k]['boundsMin']}"
                        assert wc.bounds.max.tobytes() == want_infos[k]["boundsMax"].tobytes(), what + f": boundsMax {wc.bounds.max} {want_infos[k]['boundsMax']}"


def test_expected_world_is_the_compiled_host_byte_for_byte(rtx, cases, replays, tmp_path):
    """the compiled host reads its scenes from Unity YAML: the case's local chunks and poses are written as one (NaN and infinite
    coordinates included), and its marshal compared chunk by chunk"""
    from rtx_amd import unity_scene
    from rtx_amd.host_cpp_binding import CppScene
    checked = 0
    for seed in (0, 1, 4, 6):
        case = cases[seed]
        for i, step in _pose_steps(case):
            mgr, by_mesh = df.manager_for(case, step["xf"])
            path = str(tmp_path / f"s{seed}_{i}.unity")
            unity_scene.save_unity_scene(mgr, path)
            cpp = CppScene(path, mgr.width, mgr.height)
            _, _, tris, infos = cpp.build_buffers()
            cpp.close()
            want_tris, want_infos = replays[seed][i]["tris"], replays[seed][i]["infos"]
            at = 0
            for m in range(case[4]):
                for ch in by_mesh.get(m, []):
                    a, n = int(ch["firstTriangleIndex"]), int(ch["numTriangles"])
                    k = int(np.flatnonzero(case[3]["firstTriangleIndex"] == a)[0])
                    what = f"seed {seed} step {i} ({step['kind']}) chunk {k}"
                    assert int(infos[at]["numTriangles"]) == n
                    f = int(infos[at]["firstTriangleIndex"])
                    assert tris[f:f + n].tobytes() == want_tris[a:a + n].tobytes(), what + ": triangles"
                    assert infos[at]["boundsMin"].tobytes() == want_infos[k]["boundsMin"].tobytes(), what + f": boundsMin {infos[at]['boundsMin']} {want_infos[k]['boundsMin']}"
                    assert infos[at]["boundsMax"].tobytes() == want_infos[k]["boundsMax"].tobytes(), what + f": boundsMax {infos[at]['boundsMax']} {want_infos[k]['boundsMax']}"
                    at += 1
                    checked += 1
    assert checked > 20


def test_expected_world_lies_within_a_float64_twin(cases, replays):
    """world = R(q) (s o p) + pos.  In float32 the marshal rounds: s o p once; an entry of R three times (x * x2, a sum or difference, 1 - it)
    with every entry and every intermediate bounded by E = 1 + 2 |q|^2, so an entry is off by at most 3 u E (u = 2^-24); a row of
    R (s o p) takes three products and two sums; the translation one more sum.  Nine roundings on the way to a coordinate, each relative to
    a partial result no larger than E |s o p|_1 + |pos_a|:  |error| <= 10 u (E |s o p|_1 + |pos_a|)  (10 for 9 and the second-order
    terms), plus 2^-126 per operation where a result is denormal.  Checked wherever the twin's bound is below 1e30 (no overflow on
    the way)."""
    u = 2.0 ** -24
    n_checked = 0
    for seed, case in cases.items():
        local, chunks = case[2], case[3]
        for i, step in _pose_steps(case):
            got = replays[seed][i]["tris"]
            for ch in chunks:
                a, n = int(ch["firstTriangleIndex"]), int(ch["numTriangles"])
                t = step["xf"][int(ch["meshIndex"])]
                q, s, pos = (np.asarray(t[k], np.float64) for k in ("rotation", "lossyScale", "position"))
                if not (np.isfinite(q).all() and np.isfinite(s).all() and np.isfinite(pos).all()):
                    continue
                x, y, z, w = q
                R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                              [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                              [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
                E = 1 + 2 * float(q @ q)
                for k in ("posA", "posB", "posC"):
                    p = np.asarray(local[k][a:a + n], np.float64)
                    with np.errstate(all="ignore"):
                        sp = p * s[None]
                        want = sp @ R.T + pos[None]
                        bound = E * np.abs(sp).sum(1, keepdims=True) + np.abs(pos)[None]
                        ok = np.isfinite(p).all(1, keepdims=True) & (bound < 1e30)
                        err = np.abs(np.asarray(got[k][a:a + n], np.float64) - want)
                        bad = ok & ~(err <= 10 * u * bound + 10 * 2.0 ** -126)
                    assert not bad.any(), f"seed {seed} step {i} ({step['kind']}): {k} of triangle {a + int(np.argwhere(bad)[0][0])} is {err[bad][0]:.3g} off, bound {(10 * u * bound)[bad.any(1)][0]}"
                    n_checked += int(np.broadcast_to(ok, err.shape).sum())
    assert n_checked > 10000


# ---- the oracle on the worlds the steps make ----------------------------------------------------------------------------------------

def test_oracle_tree_equals_its_loop_on_a_nan_chunk_box(rtx, oracle):
    b = nan_box_scene(rtx)
    for first in (0, 3):
        loop, loop_last, lc = oracle.render(*b, first, 2)
        tree, tree_last, tc = oracle.render(*b, first, 2, accel=True)
        assert loop.tobytes() == tree.tobytes() and loop_last.tobytes() == tree_last.tobytes() and lc["rays"] == tc["rays"]


def test_oracle_tree_equals_its_loop_after_every_step(cases, replays, oracle):
    for seed, case in cases.items():
        for s in replays[seed]:
            b = (s["params"], case[1], s["tris"], s["infos"])
            loop, _, lc = oracle.render(*b, s["index"], 1)
            tree, _, tc = oracle.render(*b, s["index"], 1, accel=True)
            same = (loop.view(np.uint32) == tree.view(np.uint32)) | (np.isnan(loop) & np.isnan(tree))
            assert same.all() and lc["rays"] == tc["rays"], f"seed {seed} step {s['index']} ({s['step']['door']} {s['step']['kind']}): {int((~same).any(-1).sum())} pixels differ"
