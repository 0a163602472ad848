/*
 * overlap_oracle.c — box overlap queries (include/rt.h "box overlap queries": rt_closest_points with the option "closest_box" = 1)
 * restated in plain C: a brute-force loop over every sphere and every triangle a chunk addresses, the touch predicates expression for
 * expression, the closest-point key of the box's centre for every candidate that touches, a FULL sort by (k, kind, primitive) and the
 * count rule.  The checker of tests/test_gpu_overlap.py, itself pinned by tests/test_overlap_cpu.py (an exact rational clip, a float64
 * twin, closest_oracle.c, and the mutants below).  TEST INFRASTRUCTURE: compiled by the tests with the oracle's own CFLAGS
 * (tests/checker_build.py: -ffp-contract=off, so every product and sum rounds on its own, as the header demands).  It includes nothing
 * but the public header, through point_oracle.h: the vectors, the closest-point keys, the records, the order of the list and the list's
 * driver (the argument check, the sort, the count rule, the K writes) live there, shared with the other point checkers.  Here: the touch
 * predicates, `searched`, and the loop.
 *
 * variant: 0 the definition;
 *          1 a triangle test that stops after the bounds condition (no plane, no edge axes);
 *          2 no plane axis;
 *          3 no edge axes;
 *          4 open sets: every <= and >= of the touch predicates strict;
 *          5 a NaN key counts.
 */
#include "point_oracle.h"

/* a <= b, or a < b for the open-set mutant; false for a NaN either way */
static int le(float a, float b, int variant) { return variant == 4 ? a < b : a <= b; }

/* ---- the touch predicates ---- */
static int sphere_touches(v3 lo, v3 hi, const rt_sphere* s, int variant)
{
    const float ex = fmaxf(fmaxf(lo.x - s->position[0], s->position[0] - hi.x), 0.0f);
    const float ey = fmaxf(fmaxf(lo.y - s->position[1], s->position[1] - hi.y), 0.0f);
    const float ez = fmaxf(fmaxf(lo.z - s->position[2], s->position[2] - hi.z), 0.0f);
    const float d2 = (ex * ex + ey * ey) + ez * ez;
    return le(d2, s->radius * s->radius, variant);
}

static int axis_ok(float p0, float p1, float p2, float r, int variant)
{
    return le(fminf(fminf(p0, p1), p2), r, variant) && le(-r, fmaxf(fmaxf(p0, p1), p2), variant);
}

static int edge_ok(v3 f, v3 v0, v3 v1, v3 v2, v3 h, int variant)
{
    if (!axis_ok(v0.z * f.y - v0.y * f.z, v1.z * f.y - v1.y * f.z, v2.z * f.y - v2.y * f.z, h.y * fabsf(f.z) + h.z * fabsf(f.y), variant)) return 0;
    if (!axis_ok(v0.x * f.z - v0.z * f.x, v1.x * f.z - v1.z * f.x, v2.x * f.z - v2.z * f.x, h.x * fabsf(f.z) + h.z * fabsf(f.x), variant)) return 0;
    if (!axis_ok(v0.y * f.x - v0.x * f.y, v1.y * f.x - v1.x * f.y, v2.y * f.x - v2.x * f.y, h.x * fabsf(f.y) + h.y * fabsf(f.x), variant)) return 0;
    return 1;
}

static int triangle_touches(v3 c, v3 h, v3 lo, v3 hi, const rt_triangle* t, int variant)
{
    const v3 A = ld(t->posA), eAB = sub(ld(t->posB), A), eAC = sub(ld(t->posC), A);
    const v3 B = add(A, eAB), C = add(A, eAC);
    /* 1: finite */
    const float co[9] = { A.x, A.y, A.z, B.x, B.y, B.z, C.x, C.y, C.z };
    for (int i = 0; i < 9; i++) if (!(fabsf(co[i]) < 1e30f)) return 0;
    /* 2: bounds */
    if (!(le(fminf(fminf(A.x, B.x), C.x), hi.x, variant) && le(lo.x, fmaxf(fmaxf(A.x, B.x), C.x), variant))) return 0;
    if (!(le(fminf(fminf(A.y, B.y), C.y), hi.y, variant) && le(lo.y, fmaxf(fmaxf(A.y, B.y), C.y), variant))) return 0;
    if (!(le(fminf(fminf(A.z, B.z), C.z), hi.z, variant) && le(lo.z, fmaxf(fmaxf(A.z, B.z), C.z), variant))) return 0;
    if (variant == 1) return 1;
    /* 3: plane */
    const v3 v0 = sub(A, c), v1 = sub(B, c), v2 = sub(C, c);
    if (variant != 2) {
        const v3 n = cross(eAB, eAC);
        const float d = dot(n, v0);
        const float rr = (h.x * fabsf(n.x) + h.y * fabsf(n.y)) + h.z * fabsf(n.z);
        if (!le(fabsf(d), rr, variant)) return 0;
    }
    /* 4: nine edge axes */
    if (variant != 3) {
        if (!edge_ok(eAB, v0, v1, v2, h, variant)) return 0;
        if (!edge_ok(sub(eAC, eAB), v0, v1, v2, h, variant)) return 0;
        if (!edge_ok(eAC, v0, v1, v2, h, variant)) return 0;
    }
    return 1;
}

static int searched(const rt_ray* b)
{
    if (!(b->tMax > 0.0f)) return 0;
    for (int a = 0; a < 3; a++) {
        if (!(fabsf(b->origin[a]) <= 3.4028235e38f)) return 0;
        if (!(b->direction[a] >= 0.0f && b->direction[a] <= 3.4028235e38f)) return 0;
    }
    return 1;
}

/* The touch decisions alone, for the twins of tests/test_overlap_cpu.py: touch[i * (ns + nt) + j] = 1 when primitive j (the spheres,
 * then ALL nt triangles in uploaded order) touches box i; a box that is not searched touches nothing. */
int ov_touches(const rt_sphere* spheres, int ns, const rt_triangle* tris, int nt, const rt_ray* boxes, int n, int variant, uint8_t* touch)
{
    for (int i = 0; i < n; i++) {
        uint8_t* o = touch + (size_t)i * ((size_t)ns + nt);
        memset(o, 0, (size_t)ns + nt);
        if (!searched(&boxes[i])) continue;
        const v3 c = ld(boxes[i].origin), h = ld(boxes[i].direction);
        const v3 lo = sub(c, h), hi = add(c, h);
        for (int s = 0; s < ns; s++) o[s] = (uint8_t)sphere_touches(lo, hi, &spheres[s], variant);
        for (int t = 0; t < nt; t++) o[ns + t] = (uint8_t)triangle_touches(c, h, lo, hi, &tris[t], variant);
    }
    return 0;
}

/* the record of a candidate is the closest-point queries', from the box's centre */
static void record(rt_closest* o, const void* c, const cand* e, const list_scene* sc, int count)
{
    record_point(o, *(const v3*)c, e, sc->spheres, sc->tris, sc->chunk_mesh, count);
}

/* out[i * K + j] = record j of boxes[i].  chunk_mesh: per chunk its mesh index (a local-mesh scene), or NULL (mesh = -1).  totals (may be
 * NULL): per box, the number of ALL candidates that count, whatever K and all are.  kth_ties (may be NULL): per box, 1 when the K-th and
 * the (K+1)-th key of the full sort are bit-equal.  -3: a chunk's range leaves the triangle buffer; -4: K or all out of range; -5: out of
 * memory. */
int ov_overlap(const rt_sphere* spheres, int ns, const rt_triangle* tris, int nt, const rt_meshinfo* mi, int nm, const int32_t* chunk_mesh,
               const rt_ray* boxes, int n, int K, int all, int variant, rt_closest* out, int32_t* totals, int32_t* kth_ties)
{
    size_t addressed;
    const int bad = list_check(mi, nm, nt, K, all, &addressed);
    if (bad) return bad;
    const list_scene scene = { spheres, tris, chunk_mesh, variant };
    int failed = 0;
#pragma omp parallel for schedule(dynamic, 16)
    for (int i = 0; i < n; i++) {
        rt_closest* o = &out[(size_t)i * K];
        list_clear(o, K, totals, kth_ties, i);
        if (!searched(&boxes[i])) continue;
        const v3 c = ld(boxes[i].origin), h = ld(boxes[i].direction);
        const v3 lo = sub(c, h), hi = add(c, h);
        cand* cd = (cand*)malloc(sizeof(cand) * ((size_t)ns + addressed + 1));
        if (!cd) { failed = 1; continue; }
        int total = 0;
        /* a candidate touches the box; its key is the closest-point queries' key of the centre, and a NaN key does not count */
        for (int s = 0; s < ns; s++) {
            if (!sphere_touches(lo, hi, &spheres[s], variant)) continue;
            const float k = sphere_key(c, &spheres[s]);
            if (k != k && variant != 5) continue;
            const cand e = { .k = k, .kind = RT_HIT_SPHERE, .prim = (uint32_t)s, .chunk = -1 };
            cd[total++] = e;
        }
        for (int m = 0; m < nm; m++)
            for (uint32_t j = 0; j < mi[m].numTriangles; j++) {
                const uint32_t t = mi[m].firstTriangleIndex + j;
                if (!triangle_touches(c, h, lo, hi, &tris[t], variant)) continue;
                const v3 A = ld(tris[t].posA), eAB = sub(ld(tris[t].posB), A), eAC = sub(ld(tris[t].posC), A);
                float u, v;
                const float k = triangle_key(c, A, eAB, eAC, &u, &v);
                if (k != k && variant != 5) continue;
                const cand e = { .k = k, .u = u, .v = v, .kind = RT_HIT_TRIANGLE, .prim = t, .chunk = m };
                cd[total++] = e;
            }
        list_finish(o, cd, total, K, all, COUNT_RULE, record, &c, &scene, totals, kth_ties, i);
        free(cd);
    }
    return failed ? -5 : 0;
}

