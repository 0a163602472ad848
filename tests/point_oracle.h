/*
 * point_oracle.h — what the checkers of the point-query family share, once: closest_oracle.c, nearest_oracle.c, overlap_oracle.c and
 * capsule_oracle.c (sweep_oracle.c takes the vectors and the triangle key).  The vectors; the closest-point keys of a sphere and of a
 * triangle, operation for operation as include/rt.h "closest-point queries" writes them; the miss record; the record of a candidate seen
 * from a point; the candidate of a sorted list, its order, and the list's driver: the argument check, the sort, the count rule and the K
 * writes.  Each checker's own file keeps its brute-force loop with the predicate that decides what counts.  TEST INFRASTRUCTURE: like
 * the checkers it includes nothing but the public header, and every product and sum rounds on its own (tests/checker_build.py:
 * -ffp-contract=off).  Everything is static; a checker uses what it needs.
 */
#ifndef POINT_ORACLE_H
#define POINT_ORACLE_H
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include "../include/rt.h"

#pragma GCC diagnostic push
#pragma GCC diagnostic ignored "-Wunused-function"

typedef struct { float x, y, z; } v3;
static v3 V(float x, float y, float z) { v3 r = { x, y, z }; return r; }
static v3 ld(const float* p) { return V(p[0], p[1], p[2]); }
static v3 add(v3 a, v3 b) { return V(a.x + b.x, a.y + b.y, a.z + b.z); }
static v3 sub(v3 a, v3 b) { return V(a.x - b.x, a.y - b.y, a.z - b.z); }
static v3 scale(v3 a, float s) { return V(a.x * s, a.y * s, a.z * s); }
static float dot(v3 a, v3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
static v3 cross(v3 a, v3 b) { return V(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); }
static v3 normalize(v3 a) { const float len = sqrtf(dot(a, a)); return V(a.x / len, a.y / len, a.z / len); }

/* ---- the keys ---- */
static float sphere_key(v3 p, const rt_sphere* s)
{
    const v3 m = sub(p, ld(s->position));
    const float len = sqrtf(dot(m, m));
    const float ds = fabsf(len - s->radius);
    return ds * ds;
}

/* the triangle A, A + eAB, A + eAC: the seven regions in the header's order, first match decides; returns the key, (u, v) through the
 * pointers */
static float triangle_key(v3 p, v3 A, v3 eAB, v3 eAC, float* pu, float* pv)
{
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

/* ---- the records ---- */
static void miss(rt_closest* o, int count)
{
    memset(o, 0, sizeof *o);
    o->dst = INFINITY;
    o->kind = RT_HIT_NONE;
    o->primitive = o->chunk = o->mesh = -1;
    o->_reserved[0] = count;
}

/* how `before` breaks a tie: nearest_oracle.c's ordering mutants, apart from every checker's `variant` numbers */
typedef enum { ORDER_DEFINITION, ORDER_TIE_BY_POSITION, ORDER_TRIANGLE_FIRST } tie_order;

/* a candidate: its key and where it was taken (s and pierced: the capsule's), what it is, and its position in the enumeration */
typedef struct { float k, s, u, v; int pierced, kind; uint32_t prim; int chunk; uint32_t seq; tie_order order; } cand;

/* ascending (k, kind, primitive): a sphere (RT_HIT_SPHERE = 1) before a triangle (RT_HIT_TRIANGLE = 2), then the lower uploaded index */
static int before(const cand* a, const cand* b)
{
    if (a->k != b->k) return a->k < b->k;
    if (a->kind != b->kind) return a->order == ORDER_TRIANGLE_FIRST ? a->kind > b->kind : a->kind < b->kind;
    if (a->order == ORDER_TIE_BY_POSITION && a->kind == RT_HIT_TRIANGLE) return a->seq < b->seq;
    return a->prim < b->prim;
}
static int by_key(const void* a, const void* b)
{
    return before((const cand*)a, (const cand*)b) ? -1 : before((const cand*)b, (const cand*)a) ? 1 : 0;
}

/* the fields of a triangle candidate at (c->u, c->v) with key c->k, seen from p */
static void record_triangle(rt_closest* o, v3 p, const cand* c, const rt_triangle* tris, const int32_t* chunk_mesh)
{
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

/* the record of candidate c for the point p: a sphere's shell, or the triangle */
static void record_point(rt_closest* o, v3 p, const cand* c, const rt_sphere* spheres, const rt_triangle* tris, const int32_t* chunk_mesh, int count)
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
    } else record_triangle(o, p, c, tris, chunk_mesh);
}

/* ---- the list's driver ---- */
/* -4: K or all out of range; -3: a chunk's range leaves the triangle buffer; else 0 and the number of addressed triangles */
static int list_check(const rt_meshinfo* mi, int nm, int nt, int K, int all, size_t* addressed)
{
    if (K < 1 || K > RT_HITS_MAX || (all != 0 && all != 1)) return -4;
    *addressed = 0;
    for (int m = 0; m < nm; m++) {
        if ((uint64_t)mi[m].firstTriangleIndex + mi[m].numTriangles > (uint64_t)nt) return -3;
        *addressed += mi[m].numTriangles;
    }
    return 0;
}

/* input i before it is searched: K misses, no candidates, no tie */
static void list_clear(rt_closest* o, int K, int32_t* totals, int32_t* kth_ties, int i)
{
    for (int j = 0; j < K; j++) miss(&o[j], 0);
    if (totals) totals[i] = 0;
    if (kth_ties) kth_ties[i] = 0;
}

/* what the records and, per checker, its record function see of the scene */
typedef struct { const rt_sphere* spheres; const rt_triangle* tris; const int32_t* chunk_mesh; int variant; } list_scene;
typedef void (*record_fn)(rt_closest* o, const void* input, const cand* c, const list_scene* scene, int count);

/* _reserved[0]: all ? every candidate : the listed ones; the listed ones whatever all is; 0 (the defaults leave _reserved 0) */
typedef enum { COUNT_RULE, COUNT_CAPPED, COUNT_ZERO } count_rule;

/* the first `listed` of c are the list: records for those, misses up to K, the count in each, totals[i] */
static void list_write(rt_closest* o, const cand* c, int listed, int total, int K, int all, count_rule rule, record_fn record, const void* input,
                       const list_scene* scene, int32_t* totals, int i)
{
    if (totals) totals[i] = total;
    const int capped = total < K ? total : K;
    const int count = rule == COUNT_ZERO ? 0 : (all && rule != COUNT_CAPPED) ? total : capped;
    for (int j = 0; j < K; j++) {
        if (j < listed) record(&o[j], input, &c[j], scene, count);
        else miss(&o[j], count);
    }
}

/* the FULL sort of the candidates, kth_ties[i], then list_write */
static void list_finish(rt_closest* o, cand* c, int total, int K, int all, count_rule rule, record_fn record, const void* input,
                        const list_scene* scene, int32_t* totals, int32_t* kth_ties, int i)
{
    qsort(c, (size_t)total, sizeof(cand), by_key);
    if (kth_ties && total > K && c[K - 1].k == c[K].k) kth_ties[i] = 1;
    list_write(o, c, total < K ? total : K, total, K, all, rule, record, input, scene, totals, i);
}

#pragma GCC diagnostic pop
#endif
