"""Structural audit of a BVH4 as the tracer holds it (rt_read_bvh + rt_read_bvh_order), node by node against its triangles, in
numpy / float64 and without a GPU.  A hierarchy only prunes, so an image shows a wrong box only to the few rays that graze it; the
audit looks at every box instead.  Test infrastructure only.

    report = audit(f32_nodes, f16_nodes, order, tris, live=None, max_stack=None)
    assert_clean(report, "what was audited")

Categories of the report (each a counter and a few example messages):

  topology     child references are empty, a leaf or a node index < len(nodes); every node but the root is referenced exactly once
               and reachable from the root (the walk keeps a visited set, so a cycle ends and is reported); meta[0] == k with slots
               [0, k) used and [k, 4) empty (k_stack_need and the traversal rely on it)
  empty        empty slots are (+inf, -inf) in both node forms
  leaves       leaf ranges [first, first + count) tile [0, len(order)) without gap or overlap, count is 1..4, `order` is a
               permutation of `live` (default: every triangle)
  containment  every finite vertex coordinate (not NaN, |p| < 1e30: tests/bvh_check.cpp) of a triangle lies inside its leaf slot's
               f32 box and inside every slot box on the way down from the root — THE invariant: a ray that hits the triangle
               passes every one of these boxes
  padding      a leaf slot's box reaches at least 0.99 * (3e-5 * m + 2e-6 * G_low) beyond the exact bounds lo / hi of its triangles'
               finite coordinates, per axis, m = max(|lo|, |hi|), G_low = the largest finite |coordinate| of the tree's triangles
               (bvh.cpp pad_box with its G >= the scene's extent; the device builder's k_collapse_level and k_refit_level take the
               same expression with G >= that extent as well).  0.99 is derived: the float32 evaluation of e = 3e-5f * m + 2e-6f * G
               is off by a few ulps of e (relative 1e-7: 3e-5f and 2e-6f are within 3e-8 of the decimals), and the subtraction
               lo - e rounds by at most 2^-24 * (m + e) = 0.2 % of the 3e-5 * m that e contains.  A face at +-inf or beyond +-FLT_MAX
               counts as met.
  nesting      each internal slot's f32 box contains the four slot boxes of its child node; with refitted=True (after k_refit_level)
               it equals their union.  Both builders pad the *unpadded* boxes of their binary trees with one monotone expression
               (a box inside another has the smaller m), so built trees nest as well; the host builder's trees were found to nest
               for every collapse mode and with the insertion passes on (tests/test_bvh_audit_cpu.py), so nesting is asserted for
               every tree.
  f16          child references equal the f32 form's, every used f16 box contains its f32 box, no f16 denormal, the plane sets of
               a node agree, and the widening stays within (node extent) / 2 * 2^-9 + 2^-13 per axis — the bound of
               test_f16_boxes_contain_the_f32_boxes — wherever the offset from the node's origin fits the f16 range (|offset| <
               65503; larger offsets become +-inf by design, bvh.hpp)
  stack        the worst-case traversal stack, recomputed as (k - 1) + max over the internal children (floor 1), is <= max_stack;
               == max_stack with exact_stack=True (a device build computes it exactly; so does the host builder)
"""
import numpy as np

EMPTY = 0xFFFFFFFF
LEAF = 0x80000000
FLT_MAX = float(np.finfo(np.float32).max)
CATEGORIES = ("topology", "empty", "leaves", "containment", "padding", "nesting", "f16", "stack")
AXES = "xyz"


def decode_f16_nodes(h):
    """Node4h words [n, 32] -> (mins [n, 3, 4], maxs [n, 3, 4]) as float64 = origin + offset, checking that the plane sets agree."""
    n = h.shape[0]
    halves = h[:, :24].copy().view(np.float16).astype(np.float64).reshape(n, 6, 8)          # six 16-byte sets of 8 halves
    org = h[:, 28:31].copy().view(np.float32).astype(np.float64)                             # [n, 3]
    sets = halves[:, :4].reshape(n, 4, 2, 4)                                                 # set c: (x planes, y planes)
    minx, maxx, miny, maxy = sets[:, 0, 0], sets[:, 1, 0], sets[:, 0, 1], sets[:, 2, 1]
    assert np.array_equal(sets[:, 2, 0], minx) and np.array_equal(sets[:, 3, 0], maxx)       # bit 0 of c picks the x planes
    assert np.array_equal(sets[:, 1, 1], miny) and np.array_equal(sets[:, 3, 1], maxy)       # bit 1 the y planes
    minz, maxz = halves[:, 4, :4], halves[:, 4, 4:]
    assert np.array_equal(halves[:, 5, :4], maxz) and np.array_equal(halves[:, 5, 4:], minz)
    mins = np.stack([minx, miny, minz], 1) + org[:, :, None]
    maxs = np.stack([maxx, maxy, maxz], 1) + org[:, :, None]
    return mins, maxs


def decode_f32_nodes(f32):
    """Node4 words [n, 32] -> (mins [n, 3, 4], maxs [n, 3, 4]) float64, child [n, 4] uint32, meta0 [n]"""
    w = np.ascontiguousarray(f32).view(np.uint32).reshape(-1, 32)
    planes = w[:, :24].copy().view(np.float32).astype(np.float64).reshape(-1, 6, 4)
    return planes[:, :3], planes[:, 3:], w[:, 24:28].copy(), w[:, 28].copy()


def triangle_positions(tris):
    """[n, 3 vertices, 3 axes] float64 of a TRIANGLE record array, an (n, 9) or an (n, 3, 3) float array"""
    if getattr(tris, "dtype", None) is not None and tris.dtype.names:
        return np.stack([tris["posA"], tris["posB"], tris["posC"]], 1).astype(np.float64).reshape(-1, 3, 3)
    return np.asarray(tris, np.float64).reshape(-1, 3, 3)


class Report:
    def __init__(self):
        self.counts = {c: 0 for c in CATEGORIES}
        self.examples = {c: [] for c in CATEGORIES}
        self.n_nodes = self.n_triangles = self.levels = self.stack_need = 0

    def add(self, category, count, message):
        count = int(count)
        if count <= 0:
            return
        self.counts[category] += count
        if len(self.examples[category]) < 4:
            self.examples[category].append(message() if callable(message) else message)

    @property
    def clean(self):
        return not any(self.counts.values())

    def failed(self):
        return {c for c, n in self.counts.items() if n}

    def __str__(self):
        lines = [f"{self.n_nodes} nodes, {self.n_triangles} triangles, {self.levels} levels, stack {self.stack_need}"]
        for c in CATEGORIES:
            if self.counts[c]:
                lines.append(f"  {c}: {self.counts[c]}")
                lines += [f"    {m}" for m in self.examples[c]]
        return "\n".join(lines)


def assert_clean(report, what):
    assert report.clean, f"{what}: BVH audit failed: {report}"


def _first(mask):
    return tuple(int(i) for i in np.argwhere(mask)[0])


def audit(f32_nodes, f16_nodes, order, tris, live=None, max_stack=None, refitted=False, exact_stack=False):
    rep = Report()
    mins, maxs, child, meta0 = decode_f32_nodes(f32_nodes)
    n = len(child)
    order = np.asarray(order).astype(np.int64).ravel()
    P = triangle_positions(tris)
    nt = len(P)
    expected = np.arange(nt, dtype=np.int64) if live is None else np.asarray(live).astype(np.int64).ravel()
    rep.n_nodes, rep.n_triangles = n, len(order)
    finiteP = ~np.isnan(P) & (np.abs(P) < 1e30)

    # ---- order: a permutation of the expected triangles
    if not np.array_equal(np.sort(order), np.sort(expected)):
        cnt = np.bincount(order[(order >= 0) & (order < nt)], minlength=nt) - np.bincount(expected, minlength=nt)
        rep.add("leaves", max(1, int((cnt != 0).sum()) + int(((order < 0) | (order >= nt)).sum())),
                lambda: f"order is no permutation of the {len(expected)} expected triangles: {len(order)} entries, "
                        f"twice / unexpected {np.where(cnt > 0)[0][:4].tolist()}, missing {np.where(cnt < 0)[0][:4].tolist()}")
    if n == 0:
        rep.add("leaves", len(order), f"no nodes, but {len(order)} order entries")
        return rep
    order_ok = (order >= 0) & (order < nt)
    G_low = float(np.abs(P[order[order_ok]])[finiteP[order[order_ok]]].max(initial=0.0))

    used = child != EMPTY
    is_leaf = used & ((child & LEAF) != 0)
    is_node = used & ~is_leaf

    # ---- topology over the whole array
    bad_ref = is_node & (child >= n)
    rep.add("topology", bad_ref.sum(), lambda: "node %d slot %d refers to node %d of %d" % (*_first(bad_ref), child[bad_ref][0], n))
    is_node &= ~bad_ref
    refs = np.bincount(child[is_node].astype(np.int64), minlength=n)
    rep.add("topology", refs[0] != 0, f"the root is referenced {refs[0]} times")
    wrong = refs[1:] != 1
    rep.add("topology", wrong.sum(), lambda: f"node {1 + int(np.argmax(wrong))} is referenced {refs[1 + int(np.argmax(wrong))]} times")
    k_used = used.sum(1)
    bad_meta = (meta0 != k_used) | (used != (np.arange(4)[None, :] < k_used[:, None])).any(1)
    rep.add("topology", bad_meta.sum(), lambda: f"node {int(np.argmax(bad_meta))}: meta[0] = {meta0[np.argmax(bad_meta)]}, used slots "
                                                f"{used[np.argmax(bad_meta)].astype(int).tolist()}")

    # ---- empty slots, f32 form
    e3 = np.broadcast_to(~used[:, None, :], mins.shape)
    bad_empty = e3 & ~(np.isposinf(mins) & np.isneginf(maxs))
    rep.add("empty", bad_empty.any(1).sum(), lambda: "node %d axis %d slot %d: an empty slot's f32 box is not (+inf, -inf)" % _first(bad_empty))

    # ---- the walk from the root, one tree level at a time
    visited = np.zeros(n, bool)
    frontier = np.array([0], np.int64)
    visited[0] = True
    path_lo = np.full((1, 3), -np.inf); path_hi = np.full((1, 3), np.inf)
    own_lo = np.full((1, 3), -1, np.int64); own_hi = np.full((1, 3), -1, np.int64)     # node * 4 + slot of the binding ancestor face
    levels = []
    leaf_first, leaf_count = [], []
    while len(frontier):
        levels.append(frontier)
        lo = mins[frontier]; hi = maxs[frontier]                                       # [m, 3, 4]
        slot_id = frontier[:, None] * 4 + np.arange(4)[None, :]                        # [m, 4]
        # the intersection of the boxes on the way down (a NaN face poisons it: no coordinate is inside a NaN box)
        with np.errstate(invalid="ignore"):
            tighter_lo = ~(lo <= path_lo[:, :, None]) & ~np.isnan(path_lo[:, :, None]); tighter_hi = ~(hi >= path_hi[:, :, None]) & ~np.isnan(path_hi[:, :, None])
        cur_lo = np.where(tighter_lo, lo, path_lo[:, :, None]); cur_hi = np.where(tighter_hi, hi, path_hi[:, :, None])
        cur_own_lo = np.where(tighter_lo, slot_id[:, None, :], own_lo[:, :, None]); cur_own_hi = np.where(tighter_hi, slot_id[:, None, :], own_hi[:, :, None])

        # -- leaves of this level
        lf = is_leaf[frontier]
        li, ls = np.nonzero(lf)
        if len(li):
            c = child[frontier[li], ls].astype(np.int64)
            first, count = (c & 0x7FFFFFFF) >> 2, (c & 3) + 1
            leaf_first.append(first); leaf_count.append(count)
            idx = first[:, None] + np.arange(4)[None, :]
            valid = (np.arange(4)[None, :] < count[:, None]) & (idx < len(order))
            t = order[np.where(valid, idx, 0)] if len(order) else np.zeros_like(idx)
            valid &= (t >= 0) & (t < nt)
            V = P[np.where(valid, t, 0)] if nt else np.zeros(idx.shape + (3, 3))      # [L, 4, vertex, axis]
            fin = (finiteP[np.where(valid, t, 0)] if nt else np.zeros(V.shape, bool)) & valid[:, :, None, None]
            blo = cur_lo[li, :, ls][:, None, None, :]; bhi = cur_hi[li, :, ls][:, None, None, :]
            with np.errstate(invalid="ignore"):
                out_lo = fin & ~(V >= blo); out_hi = fin & ~(V <= bhi)
            out = out_lo | out_hi
            if out.any():
                def msg(out=out, out_lo=out_lo, V=V, t=t, li=li, ls=ls, frontier=frontier, cur_own_lo=cur_own_lo, cur_own_hi=cur_own_hi, cur_lo=cur_lo, cur_hi=cur_hi):
                    L, j, v, a = _first(out)
                    low = bool(out_lo[L, j, v, a])
                    owner = int((cur_own_lo if low else cur_own_hi)[li[L], a, ls[L]])
                    face = (cur_lo if low else cur_hi)[li[L], a, ls[L]]
                    return (f"triangle {int(t[L, j])} vertex {v} {AXES[a]} = {V[L, j, v, a]:.9g} is {'below' if low else 'above'} the {'min' if low else 'max'} "
                            f"face {face:.9g} of node {owner // 4} slot {owner % 4} (leaf: node {int(frontier[li[L]])} slot {int(ls[L])})")
                rep.add("containment", out.sum(), msg)
            # padding against the leaf slot's own box
            Vlo = np.where(fin, V, np.inf).min(axis=(1, 2)); Vhi = np.where(fin, V, -np.inf).max(axis=(1, 2))     # [L, axis]
            has = Vlo <= Vhi
            m = np.maximum(np.abs(Vlo), np.abs(Vhi))
            with np.errstate(invalid="ignore", over="ignore"):
                e = 0.99 * (3e-5 * m + 2e-6 * G_low)
                slo = lo[li, :, ls]; shi = hi[li, :, ls]
                thin_lo = has & ~((slo <= Vlo - e) | (slo <= -FLT_MAX)); thin_hi = has & ~((shi >= Vhi + e) | (shi >= FLT_MAX))
            thin = thin_lo | thin_hi
            if thin.any():
                def msg(thin=thin, thin_lo=thin_lo, li=li, ls=ls, frontier=frontier, slo=slo, shi=shi, Vlo=Vlo, Vhi=Vhi, e=e, t=t):
                    L, a = _first(thin)
                    low = bool(thin_lo[L, a])
                    return (f"node {int(frontier[li[L]])} slot {int(ls[L])} {AXES[a]}: {'min' if low else 'max'} face {(slo if low else shi)[L, a]:.9g} is "
                            f"{abs((slo - Vlo if low else shi - Vhi)[L, a]):.9g} beyond the triangles' {(Vlo if low else Vhi)[L, a]:.9g} (triangle {int(t[L, 0])} ...), "
                            f"at least {e[L, a]:.9g} wanted (G_low {G_low:.9g})")
                rep.add("padding", thin_lo.sum() + thin_hi.sum(), msg)

        # -- internal slots: nesting, and the next level
        ni, ns = np.nonzero(is_node[frontier])
        c = child[frontier[ni], ns].astype(np.int64)
        if len(c):
            with np.errstate(invalid="ignore"):
                cmin = np.fmin.reduce(mins[c], axis=2, initial=np.inf); cmax = np.fmax.reduce(maxs[c], axis=2, initial=-np.inf)    # [q, 3]
                plo = lo[ni, :, ns]; phi = hi[ni, :, ns]
                if refitted:
                    bad = (plo != cmin) | (phi != cmax)
                else:
                    bad = ((cmin <= cmax) | np.isfinite(cmin) | np.isfinite(cmax)) & ~((plo <= cmin) & (phi >= cmax))
            if bad.any():
                def msg(bad=bad, frontier=frontier, ni=ni, ns=ns, c=c, plo=plo, phi=phi, cmin=cmin, cmax=cmax):
                    q, a = _first(bad)
                    return (f"node {int(frontier[ni[q]])} slot {int(ns[q])} {AXES[a]}: [{plo[q, a]:.9g}, {phi[q, a]:.9g}] "
                            f"{'is not the union' if refitted else 'does not contain the boxes'} of its child node {int(c[q])}: [{cmin[q, a]:.9g}, {cmax[q, a]:.9g}]")
                rep.add("nesting", bad.sum(), msg)
        # first reference wins; a node met again (a cycle, a shared child) is reported and not entered twice
        uniq, pos = np.unique(c, return_index=True)
        fresh = ~visited[uniq]
        again = len(c) - int(fresh.sum())
        rep.add("topology", again, lambda: f"level {len(levels)}: {again} references to nodes already visited (first: node "
                                           f"{int(c[np.setdiff1d(np.arange(len(c)), pos[fresh])[0]])}): a cycle or a shared child")
        pos = np.sort(pos[fresh])
        frontier = c[pos]
        visited[frontier] = True
        path_lo = cur_lo[ni[pos], :, ns[pos]]; path_hi = cur_hi[ni[pos], :, ns[pos]]
        own_lo = cur_own_lo[ni[pos], :, ns[pos]]; own_hi = cur_own_hi[ni[pos], :, ns[pos]]
    rep.levels = len(levels)
    rep.add("topology", (~visited).sum(), lambda: f"node {int(np.argmin(visited))} cannot be reached from the root")

    # ---- leaves tile the order
    first = np.concatenate(leaf_first) if leaf_first else np.zeros(0, np.int64)
    count = np.concatenate(leaf_count) if leaf_count else np.zeros(0, np.int64)
    rep.add("leaves", ((count < 1) | (count > 4)).sum(), "a leaf count outside 1..4")
    o = np.argsort(first, kind="stable")
    first, count = first[o], count[o]
    ends = np.concatenate([[0], first + count])
    starts = np.concatenate([first, [len(order)]])
    seam = ends != starts
    rep.add("leaves", seam.sum(), lambda: f"leaf ranges do not tile [0, {len(order)}): after position {int(ends[np.argmax(seam)])} the next leaf "
                                          f"(or the end) starts at {int(starts[np.argmax(seam)])}")

    # ---- the f16 form
    h = np.ascontiguousarray(f16_nodes).view(np.uint32).reshape(-1, 32)
    if len(h) != n:
        rep.add("f16", 1, f"{len(h)} f16 nodes for {n} f32 nodes")
    else:
        diff = h[:, 24:28] != child
        rep.add("f16", diff.sum(), lambda: "node %d slot %d: child reference %#x in the f16 form, %#x in the f32 form" % (*_first(diff), h[:, 24:28][diff][0], child[diff][0]))
        halves = h[:, :24].copy().view(np.uint16)
        den = ((halves & 0x7C00) == 0) & ((halves & 0x03FF) != 0)
        rep.add("f16", den.sum(), lambda: "node %d half %d is an f16 denormal" % _first(den))
        try:
            mins16, maxs16 = decode_f16_nodes(h)
        except AssertionError:
            rep.add("f16", 1, "the plane sets of a node disagree")
            mins16 = None
        if mins16 is not None:
            u3 = np.broadcast_to(used[:, None, :], mins.shape)
            bad = ~u3 & ~(np.isposinf(mins16) & np.isneginf(maxs16))
            rep.add("empty", bad.any(1).sum(), lambda: "node %d axis %d slot %d: an empty slot's f16 box is not (+inf, -inf)" % _first(bad))
            with np.errstate(invalid="ignore"):
                cut_lo = u3 & ~np.isnan(mins) & ~(mins16 <= mins); cut_hi = u3 & ~np.isnan(maxs) & ~(maxs16 >= maxs)
            cut = cut_lo | cut_hi
            if cut.any():
                def msg():
                    i, a, s = _first(cut)
                    return (f"node {i} slot {s} {AXES[a]}: f16 box [{mins16[i, a, s]:.9g}, {maxs16[i, a, s]:.9g}] does not contain the f32 box "
                            f"[{mins[i, a, s]:.9g}, {maxs[i, a, s]:.9g}]")
                rep.add("f16", cut.sum(), msg)
            org = h[:, 28:31].copy().view(np.float32).astype(np.float64)[:, :, None]
            with np.errstate(invalid="ignore"):
                fl = u3 & np.isfinite(mins); fh = u3 & np.isfinite(maxs)
                nlo = np.where(fl, mins, np.inf).min(axis=2, keepdims=True); nhi = np.where(fh, maxs, -np.inf).max(axis=2, keepdims=True)
                slack = np.broadcast_to(np.where(nhi >= nlo, nhi - nlo, 0.0) * 0.5 * 2.0 ** -9 + 2.0 ** -13, mins.shape)
                wide_lo = fl & (np.abs(mins - org) < 65503.0) & ~(mins - mins16 <= slack)
                wide_hi = fh & (np.abs(maxs - org) < 65503.0) & ~(maxs16 - maxs <= slack)
            wide = wide_lo | wide_hi
            if wide.any():
                def msg():
                    i, a, s = _first(wide)
                    return (f"node {i} slot {s} {AXES[a]}: f16 box [{mins16[i, a, s]:.9g}, {maxs16[i, a, s]:.9g}] is more than {slack[i, a, s]:.9g} wider than "
                            f"[{mins[i, a, s]:.9g}, {maxs[i, a, s]:.9g}]")
                rep.add("f16", wide.sum(), msg)

    # ---- worst-case traversal stack, bottom-up over the levels of the walk
    need = np.zeros(n, np.int64)
    level_of = np.full(n, -1, np.int64)
    for L, nodes_L in enumerate(levels):
        level_of[nodes_L] = L
    for L in range(len(levels) - 1, -1, -1):
        nodes_L = levels[L]
        c = np.where(is_node[nodes_L], child[nodes_L], 0).astype(np.int64)
        below = is_node[nodes_L] & (level_of[c] > L)                       # (a reference back up the tree was reported above)
        deepest = np.where(below, need[c], 0).max(axis=1)
        need[nodes_L] = k_used[nodes_L] - 1 + deepest
    rep.stack_need = max(1, int(need[0]))
    if max_stack is not None:
        rep.add("stack", max_stack < rep.stack_need or (exact_stack and max_stack != rep.stack_need),
                f"the traversal needs a stack of {rep.stack_need}, bvhMaxStack says {max_stack}")
    return rep


# ---- helpers the audit's tests share ---------------------------------------------------------------------------------------------

def _f32_below(x):
    """bvh.hpp f32_below: the next float32 below x; +-inf and NaN stay"""
    x = np.asarray(x, np.float32)
    with np.errstate(invalid="ignore"):
        return np.where(np.isfinite(x), np.nextafter(x, np.float32(-np.inf)), x).astype(np.float32)


def _f16_round_down(x):
    """bvh.hpp f16_round_down as bits: the largest f16 <= x that is no denormal; NaN -> -inf"""
    x = np.asarray(x, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        h = x.astype(np.float16)
        h = np.where(h.astype(np.float32) > x, np.nextafter(h, np.float16(-np.inf)), h).astype(np.float16)
        hf = h.astype(np.float32)
        tiny = (np.abs(hf) < np.float32(2.0 ** -14)) & ((hf != 0) | (x < 0))
        h = np.where(tiny, np.where(x > 0, np.float16(0.0), np.float16(-2.0 ** -14)), h).astype(np.float16)
        h = np.where(np.isnan(x), np.float16(-np.inf), h).astype(np.float16)
    return h.view(np.uint16)


def pack_f16_nodes(f32_nodes):
    """Node4 words [n, 32] -> Node4h words [n, 32] the way bvh.hpp describes Node4h and k_compact_nodes makes it: offsets from the
    node's origin (the centre of its finite faces), min offsets rounded down and max offsets rounded up, no denormals."""
    w = np.ascontiguousarray(f32_nodes).view(np.uint32).reshape(-1, 32)
    n = len(w)
    planes = w[:, :24].copy().view(np.float32).reshape(n, 6, 4)
    mins, maxs = planes[:, :3], planes[:, 3:]                                     # [n, 3, 4] float32
    with np.errstate(invalid="ignore", over="ignore"):
        lo = np.where(np.isfinite(mins), mins, np.float32(np.inf)).min(axis=2)
        hi = np.where(np.isfinite(maxs), maxs, np.float32(-np.inf)).max(axis=2)
        o = (np.float32(0.5) * lo + np.float32(0.5) * hi).astype(np.float32)
        o = np.where(np.isfinite(o), o, np.where(lo < np.inf, lo, np.where(hi > -np.inf, hi, np.float32(0)))).astype(np.float32)
        hmin = _f16_round_down(_f32_below((mins - o[:, :, None]).astype(np.float32)))
        hmax = _f16_round_down(_f32_below((-(maxs - o[:, :, None])).astype(np.float32))) ^ np.uint16(0x8000)
    halves = np.zeros((n, 64), np.uint16)
    for c in range(4):
        halves[:, 8 * c:8 * c + 4] = (hmax if c & 1 else hmin)[:, 0]
        halves[:, 8 * c + 4:8 * c + 8] = (hmax if c & 2 else hmin)[:, 1]
    halves[:, 32:36], halves[:, 36:40], halves[:, 40:44], halves[:, 44:48] = hmin[:, 2], hmax[:, 2], hmax[:, 2], hmin[:, 2]
    out = halves.view(np.uint32).reshape(n, 32).copy()
    out[:, 24:28] = w[:, 24:28]
    out[:, 28:31] = o.view(np.uint32)
    out[:, 31] = 0
    return out


def awkward_triangles(rtx, n):
    """n random triangles with an exact duplicate and a NaN coordinate among them (n >= 5), as one chunk: (triangles, meshinfo)"""
    rng = np.random.default_rng(n)
    tris = np.zeros(n, rtx.TRIANGLE)
    c = rng.uniform([-3, 0, -2], [3, 3, 4], (n, 1, 3)).astype(np.float32)
    p = c + rng.uniform(-0.6, 0.6, (n, 3, 3)).astype(np.float32)
    if n >= 5:
        p[3] = p[2]                               # an exact duplicate
        p[4, 1, 0] = np.nan
    tris["posA"], tris["posB"], tris["posC"] = p[:, 0], p[:, 1], p[:, 2]
    nrm = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]).astype(np.float32)
    for f in ("normalA", "normalB", "normalC"):
        tris[f] = nrm
    infos = np.zeros(1, rtx.MESHINFO)
    infos["numTriangles"] = n
    infos["material"]["colour"] = (0.8, 0.7, 0.6, 1); infos["material"]["emissionColour"] = (1, 1, 1, 1); infos["material"]["emissionStrength"] = 0.5
    with np.errstate(invalid="ignore"):
        infos["boundsMin"], infos["boundsMax"] = np.nanmin(p.reshape(-1, 3), 0) - 1, np.nanmax(p.reshape(-1, 3), 0) + 1
    return tris, infos


STAND_OFF = 0.01


def aimed_rays(rtx, tris, live=None):
    """Rays at the box faces: for every live triangle and each of its vertices the point 0.2 % of the way from the vertex to the
    centroid, and through it one ray along each axis, against the triangle's front (RayTriangle culls back faces), from STAND_OFF in
    front of the point.  A triangle attains each of its six bounding extremes at a vertex, so a box face that cuts a triangle — in
    either node form — culls one of these rays.  -> (rays, the triangle each ray is aimed at)"""
    P = triangle_positions(tris)
    ids = np.arange(len(P)) if live is None else np.asarray(live)
    T = P[ids]                                                             # [n, 3, 3]
    centroid = T.mean(axis=1, keepdims=True)
    q = (T + 0.002 * (centroid - T)).astype(np.float32)                    # [n, vertex, 3]
    nrm = np.cross(T[:, 1] - T[:, 0], T[:, 2] - T[:, 0])                   # front = the side cross(AB, AC) points to
    d = np.zeros((len(T), 3, 3, 3), np.float32)                            # [n, vertex, ray axis, xyz]
    for a in range(3):
        d[:, :, a, a] = np.where(nrm[:, a] > 0, -1.0, 1.0)[:, None]
    o = (q[:, :, None, :] - np.float32(STAND_OFF) * d).astype(np.float32)
    rays = np.zeros(len(T) * 9, rtx.RAY)
    rays["origin"], rays["direction"], rays["tMax"] = o.reshape(-1, 3), d.reshape(-1, 3), np.inf
    return rays, np.repeat(ids, 9)


def aimed_ray_shares(rtx, hits, target, tris, live=None):
    """(share of the rays whose closest hit is the triangle they were aimed at, triangles with a non-zero normal none of whose
    rays reports them) of the oracle's answers `hits`"""
    on = (hits["kind"] == rtx._cabi.RT_HIT_TRIANGLE) & (hits["primitive"] == target)
    P = triangle_positions(tris)
    ids = np.arange(len(P)) if live is None else np.asarray(live)
    nrm = np.cross(P[ids, 1] - P[ids, 0], P[ids, 2] - P[ids, 0])
    with np.errstate(invalid="ignore"):
        solid = (np.abs(nrm) > 0).any(1)
    reported = np.zeros(len(P), bool)
    reported[target[on]] = True
    return float(on.mean()) if len(on) else 1.0, ids[solid & ~reported[ids]]


def ragged_chunk_scene(rtx, width=64, height=40):
    """The mesh-test scene with a chunk of numTriangles = 0 and three triangles no chunk refers to (the shader can never reach
    them): (params, spheres, triangles, meshinfo)"""
    params, spheres, tris, infos = rtx.scenes.mesh_test_scene(width, height).build_buffers()
    infos = infos.copy()
    empty = infos[:1].copy()
    empty["numTriangles"] = 0
    infos = np.concatenate([infos[:3], empty, infos[3:]])
    infos["numTriangles"][5] -= 3                      # the last 3 triangles of that chunk become unreachable
    return params, spheres, tris, infos


def live_triangles(infos, n_tris):
    """the triangles some chunk addresses, in buffer order"""
    live = np.zeros(n_tris, bool)
    for first, count in zip(infos["firstTriangleIndex"].tolist(), infos["numTriangles"].tolist()):
        live[first:first + count] = True
    return np.nonzero(live)[0]


def random_pose(rtx, mgr, rng, seed):
    """A random pose per mesh of `mgr`: arbitrary unit quaternions (and a slightly non-unit one), non-uniform, negative and (seed % 3
    == 0) zero scales, translations up to 6, or 1e3 when seed % 4 == 3"""
    for i, me in enumerate(mgr.meshes):
        q = rng.normal(size=4)
        q = q / np.linalg.norm(q) * (1.0001 if i == 1 else 1.0)
        s = 10.0 ** rng.uniform(-1.5, 0.8, 3) * rng.choice([1, 1, 1, -1], 3)
        if i == 2 and seed % 3 == 0:
            s[int(rng.integers(0, 3))] = 0.0
        big = 1e3 if seed % 4 == 3 else 6.0
        me.transform = rtx.host.Transform(position=tuple(rng.uniform(-big, big, 3)), rotation=tuple(q), lossyScale=tuple(s))
