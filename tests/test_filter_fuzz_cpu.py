"""The image-chain fuzz on the CPU (tests/filter_fuzz.py): on the extended scenes the feature checker gives the same bits through the
oracle's search tree and through its literal loop; scene, poses and knobs are functions of the seed and keep random_scene's buffers as
a prefix; the inputs have what the GPU test (tests/test_gpu_filter_fuzz.py) relies on — every class of hostile guide, albedo, coverage and
temporal decision on at least three seeds with at least four pixels, and more than half of every seed's output finite, so that the
comparison is not NaN against NaN —; and every mutant of the three filter checkers gives other bits than the definition on some seed.
The checkers alone: nothing here touches a GPU."""
import os

import numpy as np
import pytest

import aov_check
import filter_fuzz as ff
from test_gpu_fuzz import random_scene

SEEDS = range(24)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the mutants mesh_test_scene at 70 x 45 (what the image chain's GPU tests had) cannot tell from the definition: both rules for a NaN
# operand give the same bits where no guide, albedo or moment is ever NaN
ONLY_THE_FUZZ_CATCHES = {("denoise", 3), ("vdenoise", 4), ("vdenoise", 5)}


@pytest.fixture(scope="module")
def cases(rtx):
    return {seed: ff.fuzz_case(rtx, seed) for seed in SEEDS}


@pytest.fixture(scope="module")
def recorded(rtx, oracle, cases):
    """seed -> every plane of the seed's stages, from the checkers alone"""
    return {seed: ff.cpu_planes(rtx, oracle, cases[seed]) for seed in SEEDS}


@pytest.fixture(scope="module")
def counts(rtx, cases, recorded):
    return {seed: ff.power_counts(rtx, cases[seed], recorded[seed]) for seed in SEEDS}


@pytest.mark.parametrize("seed", SEEDS)
def test_tree_against_loop(rtx, cases, seed):
    p, sph, tris, infos = cases[seed]["scene"]
    for frame in (cases[seed]["knobs"]["frame"], cases[seed]["knobs"]["frame"] + 1):
        tree = aov_check.oracle_frame(rtx, p, sph, tris, infos, frame, accel=True)
        loop = aov_check.oracle_frame(rtx, p, sph, tris, infos, frame, accel=False)
        for a, b, what in zip(tree, loop, ("albedo", "normal_depth")):
            aov_check.assert_same_bits(a, b, f"seed {seed}, frame {frame}, {what}: tree vs loop")


def test_everything_is_a_function_of_the_seed_and_keeps_random_scene_as_a_prefix(rtx, cases):
    for seed in (0, 5, 8, 10, 14):
        again = ff.fuzz_case(rtx, seed)
        for a, b in zip(again["scene"], cases[seed]["scene"]):
            assert a.tobytes() == b.tobytes(), seed
        assert again["knobs"] == cases[seed]["knobs"] and ff.filter_knobs(seed) == ff.filter_knobs(seed)
        assert [q.tobytes() for q in again["poses"]] == [q.tobytes() for q in cases[seed]["poses"]]
        assert again["inject"].tobytes() == cases[seed]["inject"].tobytes()
        # the settled knobs are the drawn ones, the iteration counts at most the drawn
        drawn = ff.filter_knobs(seed)
        for name in ("denoise", "vdenoise"):
            assert cases[seed]["knobs"][name]["iterations"] <= drawn[name]["iterations"]
            assert {k: v for k, v in cases[seed]["knobs"][name].items() if k != "iterations"} == {k: v for k, v in drawn[name].items() if k != "iterations"}
        assert cases[seed]["knobs"]["options"] == drawn["options"] and cases[seed]["knobs"]["temporal"] == drawn["temporal"]
    for seed in SEEDS:
        p0, sph0, tris0, infos0 = random_scene(rtx, seed)
        p, sph, tris, infos = cases[seed]["scene"]
        assert sph[:len(sph0)].tobytes() == sph0.tobytes() and tris[:len(tris0)].tobytes() == tris0.tobytes(), seed
        assert infos[:len(infos0)].tobytes() == infos0.tobytes() and len(tris) > len(tris0), seed
        q = p.copy()
        q["numRaysPerPixel"] = p0["numRaysPerPixel"]
        assert q.tobytes() == p0.tobytes(), seed                                      # (only the sample count was redrawn)
        # every added chunk addresses added triangles only, and is finite and near the camera
        for m in infos[len(infos0):]:
            first, n = int(m["firstTriangleIndex"]), int(m["numTriangles"])
            assert len(tris0) <= first and first + n <= len(tris), seed
            pos = np.stack([tris[k][first:first + n] for k in ("posA", "posB", "posC")])
            near = 1.1 * float(np.linalg.norm(np.append(0.5 * p["viewParams"][:2], 1.0))) + 0.1      # the focal plane's corner, 3 % behind it
            assert np.isfinite(pos).all() and np.linalg.norm(pos - p["worldSpaceCameraPos"], axis=-1).max() < near, seed
        assert 4 <= len(cases[seed]["poses"]) <= 5


def test_the_draws_cover_every_value(cases):
    knobs = [ff.filter_knobs(s) for s in range(200)]
    assert {k["denoise"]["iterations"] for k in knobs} == {k["vdenoise"]["iterations"] for k in knobs} == set(range(1, 7))
    for name, sig in (("denoise", ("sigmaColour", "sigmaNormal", "sigmaDepth")), ("vdenoise", ("sigmaNormal", "sigmaDepth"))):
        for s in sig:
            assert {k[name][s] for k in knobs} >= {ff.SIGMA_OVERFLOW} and ff.SIGMA_UNDERFLOW not in {k[name][s] for k in knobs}
            assert any(k[name + "_underflow"] and k[name + "_underflow"][s] == ff.SIGMA_UNDERFLOW for k in knobs), (name, s)
    assert {k["vdenoise"]["sigmaLuminance"] for k in knobs} >= {ff.SIGMA_UNDERFLOW, ff.SIGMA_OVERFLOW}
    assert {k["temporal"]["maxHistory"] for k in knobs} == set(ff.MAX_HISTORY)
    for tol in ("depthTolerance", "normalTolerance"):
        assert {k["temporal"][tol] for k in knobs} >= {1e-30, 1e30}
    assert {int(c["scene"][0]["numRaysPerPixel"]) for c in cases.values()} == set(ff.SAMPLES)
    assert {k["denoise"]["demodulate"] for k in knobs} == {k["vdenoise"]["demodulate"] for k in knobs} == {0, 1}
    assert any(c["knobs"]["denoise_underflow"] for c in cases.values()) and any(c["knobs"]["vdenoise_underflow"] for c in cases.values())


@pytest.mark.parametrize("seed", SEEDS)
def test_more_than_half_of_every_output_is_finite(counts, seed):
    """the drawn rt_denoise and rt_denoise_variance calls on the rendered image, and T after the last pose"""
    f = counts[seed]["finite"]
    assert set(f) == {"denoise", "vdenoise", "temporal"}
    for which, share in f.items():
        assert share >= 0.5, f"seed {seed}: {share:.3f} of the pixels of the {which} output are finite in every channel"


def test_a_squared_sigma_of_1e_25_leaves_no_finite_pixel(recorded):
    """why that value has a call of its own: 1 / (s * s) = inf, and the centre tap's 0 * inf is NaN on every pixel"""
    seen = 0
    for seed in SEEDS:
        for name, plane, _ in recorded[seed]:
            if "underflow" in name and "var_0" not in name:
                assert np.isnan(plane[..., :3]).all(), (seed, name)
                seen += 1
    assert seen >= 8


@pytest.mark.parametrize("cls", ff.CLASSES)
def test_every_class_occurs_on_three_seeds_with_four_pixels(counts, cls):
    seeds = [s for s in SEEDS if counts[s][cls] >= 4]
    assert len(seeds) >= 3, f"{cls} ({ff.CLASS_NOTES[cls]}): seeds {seeds}"


def test_every_mutant_differs_on_some_seed_and_three_only_there(rtx, oracle, cases, recorded):
    caught = {}
    for seed in SEEDS:
        for key, hit in ff.mutants_caught(recorded[seed], cases[seed]["knobs"]).items():
            caught[key] = caught.get(key, 0) + bool(hit)
    want = {("denoise", v) for v in ff.DENOISE_MUTANTS} | {("vdenoise", v) for v in ff.VDENOISE_MUTANTS} | {("temporal", v) for v in ff.TEMPORAL_MUTANTS}
    assert set(caught) == want
    assert all(caught.values()), {k: n for k, n in caught.items() if not n}
    benign = ff.mutants_caught(*ff.benign_recorded(rtx, oracle))
    assert {k for k, hit in benign.items() if not hit} == ONLY_THE_FUZZ_CATCHES


def test_the_recorded_table_is_this(rtx, cases, counts):
    """profiles/filter_fuzz_inputs.txt holds what `python tests/filter_fuzz.py` prints"""
    rows = {}
    for line in open(os.path.join(ROOT, "profiles", "filter_fuzz_inputs.txt")):
        w = line.split()
        if len(w) == 8 + len(ff.CLASSES) and w[0].isdigit():
            rows[int(w[0])] = [int(x) for x in w[8:]]
    assert sorted(rows) == list(SEEDS)
    for seed, c in counts.items():
        assert rows[seed] == [c[k] for k in ff.CLASSES], seed
