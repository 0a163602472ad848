#!/usr/bin/env python3
"""Generated code of two trees of this repository, kernel by kernel (gfx950, no GPU needed): the check a refactor of the kernels owes.

    python tools/isa_diff.py <parent tree> <branch tree> [--keep DIR]      (e.g. a `git worktree add --detach` of the parent, and `.`)

Each tree's .hip units — those its own __graft_entry__.hip_sources() lists — are assembled as tools/static_valu.py assemble() does
it, with the flags of THAT tree's __graft_entry__, and the kernels are matched by mangled name across all units of a tree: a kernel may
move between units from one tree to the other, and one that a tree holds twice is reported.  Per kernel (its label to its
.Lfunc_end): comments dropped, the function's ordinal taken out of the block labels (.LBB<ordinal>_<n>: the ordinal is the function's
position in the file), then the lines compared one by one.  VGPRs, SGPRs, scratch, occupancy and spills come from the summary lines
the compiler prints after each kernel.  One line per kernel: identical, or the instruction delta with those figures.  Text is
compared; no instruction is interpreted."""
import argparse
import os
import re
import runpy
import shutil
import subprocess
import tempfile

FIGURES = (("VGPRs", "NumVgprs"), ("SGPRs", "TotalNumSgprs"), ("scratch", "ScratchSize"), ("occupancy", "Occupancy"),
           ("SGPR spills", "SGPRSpillCount"), ("VGPR spills", "VGPRSpillCount"))       # (the spill counts only where the compiler prints them)


def tree_kernels(tree, side, work):
    """mangled name -> kernels() entry over all .hip units of `tree`, and the names it holds more than once"""
    g = runpy.run_path(os.path.join(tree, "__graft_entry__.py"), run_name="isa_diff")
    flags = [f for f in g["HIPCC_FLAGS"] if f not in ("-shared", "-fPIC")]
    units = [s for s in g["hip_sources"]()[0] if s.endswith(".hip")]
    outs, procs = [], []
    for src in units:                       # side by side, as build() compiles them
        extra = g["STREAM_TU_FLAGS"] if src.endswith("rt_stream_kernels.hip") else []
        outs.append(os.path.join(work, side + "_" + os.path.basename(src)[:-4] + ".s"))
        procs.append(subprocess.Popen([shutil.which("hipcc") or "/opt/rocm/bin/hipcc", *flags, *extra, "--offload-device-only", "-S",
                                       src, "-o", outs[-1]], stderr=subprocess.DEVNULL))
    if any(p.wait() != 0 for p in procs):
        raise SystemExit(f"hipcc failed on a unit of {tree}")
    found, twice = {}, []
    for src, out in zip(units, outs):
        ks = kernels(open(out).read())
        print(f"== {side} {os.path.basename(src)}: {len(ks)} kernels")
        twice += [n for n in ks if n in found]
        found.update(ks)
    return found, twice


def kernels(text):
    """mangled name -> (the body's lines without comments and ordinals, the figures of its summary)"""
    names = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M)
    out = {}
    for name in names:
        start = text.index("\n" + name + ":") + len(name) + 2
        end = text.index(".Lfunc_end", start)
        body = []
        for ln in text[start:end].split("\n"):
            ln = re.sub(r"\.LBB\d+_", ".LBB_", ln.split(";")[0]).strip()
            if ln:
                body.append(ln)
        summary = text[end:text.index(".amdhsa_kernel", end) if ".amdhsa_kernel" in text[end:] else len(text)]
        summary = summary[:summary.index(".end_amdhsa_kernel")] if ".end_amdhsa_kernel" in summary else summary
        fig = {}
        for word, key in FIGURES:
            m = re.search(r"^\s*; %s: (\d+)" % key, summary, re.M)
            if m:
                fig[word] = int(m.group(1))
        out[name] = ([b for b in body if not b.startswith(".") and not b.endswith(":")], body, fig)
    return out


def demangle(names):
    filt = shutil.which("llvm-cxxfilt") or shutil.which("c++filt") or "/opt/rocm/llvm/bin/llvm-cxxfilt"
    try:
        out = subprocess.run([filt], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
        return {n: d[5:] if d.startswith("void ") else d for n, d in zip(names, out)}
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("parent"); ap.add_argument("branch")
    ap.add_argument("--keep", help="keep the assembly files in this directory")
    a = ap.parse_args()
    work = a.keep or tempfile.mkdtemp()
    os.makedirs(work, exist_ok=True)
    differing = 0
    (kp, twice_p), (kb, twice_b) = tree_kernels(a.parent, "parent", work), tree_kernels(a.branch, "branch", work)
    print(f"== {len(kp)} kernels at the parent, {len(kb)} at the branch")
    pretty = demangle(sorted(set(kp) | set(kb)))
    for side, twice in (("parent", twice_p), ("branch", twice_b)):
        for n in twice:
            print(f"{pretty[n]}: more than once at the {side}"); differing += 1
    library = [n for n in pretty if pretty[n].startswith("rocprim::")]
    if library:             # the device BVH build's sort / scan templates, which the project does not write: one line
        same = sum(1 for n in library if n in kp and n in kb and kp[n][1] == kb[n][1])
        print(f"rocprim::* ({len(library)} instantiations of the library's templates): {same} identical, {len(library) - same} not")
        differing += len(library) - same
    for n in sorted(set(pretty) - set(library), key=lambda n: pretty[n]):
        if n not in kp or n not in kb:
            print(f"{pretty[n]}: only at the {'parent' if n in kp else 'branch'}"); differing += 1
            continue
        (ip, bp, fp), (ib, bb, fb) = kp[n], kb[n]
        if bp == bb and fp == fb:
            print(f"{pretty[n]}: identical ({len(ip)} instructions, {fp.get('VGPRs')} VGPRs)")
            continue
        differing += 1
        moved = sum(1 for x, y in zip(ip, ib) if x != y) + abs(len(ip) - len(ib))
        figs = ", ".join(f"{w} {fp.get(w)} -> {fb.get(w)}" for w, _ in FIGURES if w in fp or w in fb)
        print(f"{pretty[n]}: DIFFERS instructions {len(ip)} -> {len(ib)} ({len(ib) - len(ip):+d}; {moved} positions differ), {figs}")
    print(f"{differing} kernels differ")
    if not a.keep:
        shutil.rmtree(work)


if __name__ == "__main__":
    main()
