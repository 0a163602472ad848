#!/usr/bin/env python3
"""The answers of the tests' point and sweep checkers in two trees of this repository, byte by byte (CPU only): the check a refactor of
the checkers owes.

    python tools/checker_diff.py <parent tree> <branch tree>      (e.g. a `git worktree add --detach` of the parent, and `.`)

From each tree tests/closest_oracle.c, nearest_oracle.c, overlap_oracle.c, capsule_oracle.c and sweep_oracle.c are compiled with the
CFLAGS of THAT tree's oracle/Makefile (as tests/checker_build.py does it) into a directory of their own, and both builds are called on
the same inputs, which the branch tree's test modules make: the scenes of test_gpu_closest.NAMES and the capsule tests' cube, beside and
around, each with the family's own batch_of, every (K, all) of its FORMS and every variant number, mutants included, with totals and
kth_ties asked for; ov_touches, cp_keys and cp_origin_bound on the same batches; sw_cast on test_sweep_cpu's scenes and batches.  One
line per (entry, scene, form, variant): the number of bytes that differ over all the arrays the entry writes."""
import argparse
import ctypes
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

SOURCES = ("closest_oracle.c", "nearest_oracle.c", "overlap_oracle.c", "capsule_oracle.c", "sweep_oracle.c")


def build(tree, work, side):
    """source name -> the tree's checker, loaded"""
    mk = open(os.path.join(tree, "oracle", "Makefile")).read()
    cflags = re.search(r"^CFLAGS\s*\?=\s*(.*)$", mk, re.M).group(1).split()
    libs = {}
    for src in SOURCES:
        so = os.path.join(work, side, "lib" + src[:-2] + ".so")
        os.makedirs(os.path.dirname(so), exist_ok=True)
        subprocess.check_call(["gcc", *cflags, "-shared", "-o", so, os.path.join(tree, "tests", src), "-lm"])
        libs[src] = ctypes.CDLL(so)
    return libs


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("parent"); ap.add_argument("branch")
    a = ap.parse_args()
    branch = os.path.abspath(a.branch)
    sys.path[:0] = [branch, os.path.join(branch, "tests")]
    import rtx_pkg
    rtx = rtx_pkg.load()
    import capsule_check as kc
    import nearest_check as nc
    import overlap_check as oc
    import sweep_check as sc
    import test_gpu_capsule
    import test_gpu_closest
    import test_sweep_cpu
    from listed_check import _p, bind_listed, oracle_listed

    vp, ci = ctypes.c_void_p, ctypes.c_int
    work = tempfile.TemporaryDirectory(prefix="checker_diff_")
    sides = [build(os.path.abspath(a.parent), work.name, "parent"), build(branch, work.name, "branch")]
    lines = differing = 0

    def report(what, answers):
        """answers: per side, the arrays an entry wrote"""
        nonlocal lines, differing
        (old, new) = ([np.ascontiguousarray(x).view(np.uint8).reshape(-1) for x in side] for side in answers)
        assert [len(x) for x in old] == [len(x) for x in new]
        d = sum(int((x != y).sum()) for x, y in zip(old, new))
        print(f"{what}: {d} of {sum(len(x) for x in old)} bytes differ")
        lines += 1
        differing += d != 0

    def closest(lib, s, t, m, p):
        lib.cp_closest.argtypes, lib.cp_closest.restype = [vp, ci, vp, ci, vp, ci, vp, vp, ci, vp, vp, vp], ci
        out, tests, at_best = np.zeros(len(p), rtx.CLOSEST), np.zeros(1, np.uint64), np.zeros(len(p), np.int32)
        assert lib.cp_closest(_p(s), len(s), _p(t), len(t), _p(m), len(m), None, _p(p), len(p), _p(out), _p(tests), _p(at_best)) == 0
        return out, tests, at_best

    def listed(fn, s, t, m, p, form, variant):
        totals, ties = np.zeros(len(p), np.int32), np.zeros(len(p), np.int32)
        return oracle_listed(bind_listed(fn), rtx, s, t, m, p, *form, variant=variant, totals=totals, kth_ties=ties), totals, ties

    def touches(lib, s, t, p, variant):
        lib.ov_touches.argtypes, lib.ov_touches.restype = [vp, ci, vp, ci, vp, ci, ci, vp], ci
        out = np.zeros((len(p), len(s) + len(t)), np.uint8)
        assert lib.ov_touches(_p(s), len(s), _p(t), len(t), _p(p), len(p), variant, _p(out)) == 0
        return (out,)

    def keys(lib, s, t, p, variant):
        lib.cp_keys.argtypes, lib.cp_keys.restype = [vp, ci, vp, ci, vp, ci, ci, vp, vp], ci
        lib.cp_origin_bound.argtypes, lib.cp_origin_bound.restype = [vp, ci, ci], ctypes.c_float
        k, par = np.zeros((len(p), len(s) + len(t)), np.float32), np.zeros((len(p), len(s) + len(t)), np.float32)
        assert lib.cp_keys(_p(s), len(s), _p(t), len(t), _p(p), len(p), variant, _p(k), _p(par)) == 0
        return k, par, np.float32([lib.cp_origin_bound(_p(p), len(p), variant)])

    def cast(lib, s, t, m, rays):
        lib.sw_cast.argtypes, lib.sw_cast.restype = [vp, ci, vp, ci, vp, ci, vp, vp, ci, vp, vp, vp], ci
        out, occ, sec = np.zeros(len(rays), rtx.HIT), np.zeros(len(rays), np.uint8), np.zeros(len(rays), np.float32)
        assert lib.sw_cast(_p(s), len(s), _p(t), len(t), _p(m), len(m), None, _p(rays), len(rays), _p(out), _p(occ), _p(sec)) == 0
        return out, occ, sec

    families = (("np_nearest", "nearest_oracle.c", nc, sorted({nc.DEFINITION, *nc.MUTANTS.values()})),
                ("ov_overlap", "overlap_oracle.c", oc, sorted({oc.DEFINITION, *oc.MUTANTS.values()})),
                ("cp_capsule", "capsule_oracle.c", kc, sorted({kc.DEFINITION, kc.BOUND_FROM_P0, *kc.MUTANTS.values()})))
    for name in (*test_gpu_closest.NAMES, "cube", "beside", "around"):
        s, t, m = (np.ascontiguousarray(x) for x in test_gpu_capsule.scene(rtx, name))
        base = test_gpu_closest.batch_of(rtx, s, t, m)
        report(f"cp_closest {name}", [closest(side["closest_oracle.c"], s, t, m, base) for side in sides])
        for entry, src, mod, variants in families:
            p = np.ascontiguousarray(mod.batch_of(rtx, s, t, m, base))
            for form in mod.FORMS:
                for variant in variants:
                    report(f"{entry} {name} (K, all) = {form} variant {variant}",
                           [listed(getattr(side[src], entry), s, t, m, p, form, variant) for side in sides])
            for variant in variants:
                if mod is oc:
                    report(f"ov_touches {name} variant {variant}", [touches(side[src], s, t, p, variant) for side in sides])
                if mod is kc:
                    report(f"cp_keys, cp_origin_bound {name} variant {variant}", [keys(side[src], s, t, p, variant) for side in sides])
    for name in test_sweep_cpu.NAMES:
        s, t, m = (np.ascontiguousarray(x) for x in test_gpu_closest.buffers_of(rtx, name))
        rays = np.ascontiguousarray(sc.batch_of(rtx, s, t, m)[0])
        report(f"sw_cast {name}", [cast(side["sweep_oracle.c"], s, t, m, rays) for side in sides])
    print(f"{lines} lines, {differing} with differing bytes")
    return 1 if differing else 0


if __name__ == "__main__":
    sys.exit(main())
