/*
 * overlap_oracle.c — box overlap queries (include/rt.h "box overlap queries": rt_closest_points with the option "closest_box" = 1)
 * restated in plain C: a brute-force loop over every sphere and every triangle a chunk addresses, the touch predicates expression for
 * expression, the closest-point key of the box's centre for every candidate that touches, a FULL sort by (k, kind, primitive) and the
 * count rule.  The checker of tests/test_gpu_overlap.py, itself pinned by tests/test_overlap_cpu.py (an exact rational clip, a float64
 * twin, closest_oracle.c, and the mutants below).  TEST INFRASTRUCTURE: compiled by the tests with the oracle's own CFLAGS
 * (tests/checker_build.py: -ffp-contract=off, so every product and sum rounds on its own, as the header demands).  It includes nothing
 * but the public header.
 *
 * variant: 0 the definition;
 *          1 a triangle test that stops after the bounds condition (no plane, no edge axes);
 *          2 no plane axis;
 *          3 no edge axes;
 *          4 open sets: every <= and >= of the touch predicates strict;
 *          5 a NaN key counts.
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include "../include/rt.h"

typedef struct { float x, y, z; } v3;
static v3 V(float x, float y, float z) { v3 r = { x, y, z }; return r; }
static v3 ld(const float* p) { return V(p[0], p[1], p[2]); }
static v3 add(v3 a, v3 b) { return V(a.x + b.x, a.y + b.y, a.z + b.z); }
static v3 sub(v3 a, v3 b) { return V(a.x - b.x, a.y - b.y, a.z - b.z); }
static v3 scale(v3 a, float s) { return V(a.x * s, a.y * s, a.z * s); }
static float dot(v3 a, v3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
static v3 cross(v3 a, v3 b) { return V(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); }
static v3 normalize(v3 a) { const float len = sqrtf(dot(a, a)); return V(a.x / len, a.y / len, a.z / len); }

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

/* ---- the keys: the closest-point queries', operation for operation (closest_oracle.c, nearest_oracle.c) ---- */
static float sphere_key(v3 p, const rt_sphere* s)
{
    const v3 m = sub(p, ld(s->position));
    const float len = sqrtf(dot(m, m));
    const float ds = fabsf(len - s->radius);
    return ds * ds;
}

static float triangle_key(v3 p, const rt_triangle* t, float* pu, float* pv)
{
    const v3 A = ld(t->posA), eAB = sub(ld(t->posB), A), eAC = sub(ld(t->posC), A);
    const v3 ap = sub(p, A);
    const float d1 = dot(eAB, ap), d2 = dot(eAC, ap);
    const v3 bp = sub(ap, eAB);
    const float d3 = dot(eAB, bp), d4 = dot(eAC, bp);
    const v3 cp = sub(ap, eAC);
    const float d5 = dot(eAB, cp), d6 = dot(eAC, cp);
    const float vc = d1 * d4 - d3 * d2;
    const float vb = d5 * d2 - d1 * d6;
    const float va = d3 * d6 - d5 * d4;
    const float d43 = d4 - d3, d56 = d5 - d6;
    float u, v;
    if (d1 <= 0.0f && d2 <= 0.0f) { u = 0.0f; v = 0.0f; }
    else if (d3 >= 0.0f && d4 <= d3) { u = 1.0f; v = 0.0f; }
    else if (vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f) { u = d1 / (d1 - d3); v = 0.0f; }
    else if (d6 >= 0.0f && d5 <= d6) { u = 0.0f; v = 1.0f; }
    else if (vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f) { u = 0.0f; v = d2 / (d2 - d6); }
    else if (va <= 0.0f && d43 >= 0.0f && d56 >= 0.0f) { v = d43 / (d43 + d56); u = 1.0f - v; }
    else {
        const float den = (va + vb) + vc;
        u = vb / den; v = vc / den;
        u = u < 0.0f ? 0.0f : u;
        u = u > 1.0f ? 1.0f : u;
        v = v < 0.0f ? 0.0f : v;
        const float room = 1.0f - u;
        v = v > room ? room : v;
    }
    const v3 q = add(add(A, scale(eAB, u)), scale(eAC, v));
    const v3 e = sub(p, q);
    *pu = u; *pv = v;
    return dot(e, e);
}

static void miss(rt_closest* o, int count)
{
    memset(o, 0, sizeof *o);
    o->dst = INFINITY;
    o->kind = RT_HIT_NONE;
    o->primitive = o->chunk = o->mesh = -1;
    o->_reserved[0] = count;
}

typedef struct { float k, u, v; int kind; uint32_t prim; int chunk; } cand;

/* ascending (k, kind, primitive): a sphere (RT_HIT_SPHERE = 1) before a triangle (RT_HIT_TRIANGLE = 2), then the lower uploaded index */
static int before(const cand* a, const cand* b)
{
    if (a->k != b->k) return a->k < b->k;
    if (a->kind != b->kind) return a->kind < b->kind;
    return a->prim < b->prim;
}
static int by_key(const void* a, const void* b)
{
    return before((const cand*)a, (const cand*)b) ? -1 : before((const cand*)b, (const cand*)a) ? 1 : 0;
}

static void record(rt_closest* o, v3 p, const cand* c, const rt_sphere* spheres, const rt_triangle* tris, const int32_t* chunk_mesh, int count)
{
    miss(o, count);
    o->kind = c->kind;
    o->primitive = (int32_t)c->prim;
    if (c->kind == RT_HIT_SPHERE) {
        const rt_sphere* s = &spheres[c->prim];
        const v3 ce = ld(s->position), m = sub(p, ce);
        const float len = sqrtf(dot(m, m));
        const v3 q = add(ce, scale(m, s->radius / len));
        const v3 nn = normalize(sub(q, ce));
        o->dst = fabsf(len - s->radius);
        o->point[0] = q.x; o->point[1] = q.y; o->point[2] = q.z;
        o->normal[0] = nn.x; o->normal[1] = nn.y; o->normal[2] = nn.z;
        o->side = len >= s->radius ? 1 : -1;
    } else {
        const rt_triangle* t = &tris[c->prim];
        const v3 A = ld(t->posA), eAB = sub(ld(t->posB), A), eAC = sub(ld(t->posC), A);
        const v3 q = add(add(A, scale(eAB, c->u)), scale(eAC, c->v));
        const v3 e = sub(p, q);
        const float sd = dot(e, cross(eAB, eAC));
        const float w = 1.0f - c->u - c->v;
        const v3 nn = normalize(add(add(scale(ld(t->normalA), w), scale(ld(t->normalB), c->u)), scale(ld(t->normalC), c->v)));
        o->dst = sqrtf(c->k);
        o->point[0] = q.x; o->point[1] = q.y; o->point[2] = q.z;
        o->normal[0] = nn.x; o->normal[1] = nn.y; o->normal[2] = nn.z;
        o->chunk = c->chunk;
        o->mesh = chunk_mesh ? chunk_mesh[c->chunk] : -1;
        o->u = c->u; o->v = c->v;
        o->side = sd > 0.0f ? 1 : sd < 0.0f ? -1 : 0;
    }
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

/* out[i * K + j] = record j of boxes[i].  chunk_mesh: per chunk its mesh index (a local-mesh scene), or NULL (mesh = -1).  totals (may be
 * NULL): per box, the number of ALL candidates that count, whatever K and all are.  kth_ties (may be NULL): per box, 1 when the K-th and
 * the (K+1)-th key of the full sort are bit-equal.  -3: a chunk's range leaves the triangle buffer; -4: K or all out of range; -5: out of
 * memory. */
int ov_overlap(const rt_sphere* spheres, int ns, const rt_triangle* tris, int nt, const rt_meshinfo* mi, int nm, const int32_t* chunk_mesh,
               const rt_ray* boxes, int n, int K, int all, int variant, rt_closest* out, int32_t* totals, int32_t* kth_ties)
{
    if (K < 1 || K > RT_HITS_MAX || (all != 0 && all != 1)) return -4;
    size_t addressed = 0;
    for (int m = 0; m < nm; m++) {
        if ((uint64_t)mi[m].firstTriangleIndex + mi[m].numTriangles > (uint64_t)nt) return -3;
        addressed += mi[m].numTriangles;
    }
    int failed = 0;
#pragma omp parallel for schedule(dynamic, 16)
    for (int i = 0; i < n; i++) {
        rt_closest* o = &out[(size_t)i * K];
        for (int j = 0; j < K; j++) miss(&o[j], 0);
        if (totals) totals[i] = 0;
        if (kth_ties) kth_ties[i] = 0;
        if (!searched(&boxes[i])) continue;
        const v3 c = ld(boxes[i].origin), h = ld(boxes[i].direction);
        const v3 lo = sub(c, h), hi = add(c, h);
        cand* cd = (cand*)malloc(sizeof(cand) * ((size_t)ns + addressed + 1));
        if (!cd) { failed = 1; continue; }
        int total = 0;
        for (int s = 0; s < ns; s++) {
            if (!sphere_touches(lo, hi, &spheres[s], variant)) continue;
            const float k = sphere_key(c, &spheres[s]);
            if (k != k && variant != 5) continue;
            cand e = { k, 0.0f, 0.0f, RT_HIT_SPHERE, (uint32_t)s, -1 };
            cd[total++] = e;
        }
        for (int m = 0; m < nm; m++)
            for (uint32_t j = 0; j < mi[m].numTriangles; j++) {
                const uint32_t t = mi[m].firstTriangleIndex + j;
                if (!triangle_touches(c, h, lo, hi, &tris[t], variant)) continue;
                float u, v;
                const float k = triangle_key(c, &tris[t], &u, &v);
                if (k != k && variant != 5) continue;
                cand e = { k, u, v, RT_HIT_TRIANGLE, t, m };
                cd[total++] = e;
            }
        qsort(cd, (size_t)total, sizeof(cand), by_key);
        const int listed = total < K ? total : K;
        if (kth_ties && total > K && cd[K - 1].k == cd[K].k) kth_ties[i] = 1;
        if (totals) totals[i] = total;
        const int count = all ? total : listed;
        for (int j = 0; j < K; j++) {
            if (j < listed) record(&o[j], c, &cd[j], spheres, tris, chunk_mesh, count);
            else miss(&o[j], count);
        }
        free(cd);
    }
    return failed ? -5 : 0;
}
