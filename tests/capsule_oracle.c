/*
 * capsule_oracle.c — capsule overlap queries (include/rt.h "capsule overlap queries": rt_closest_points with the option
 * "closest_capsule" = 1) restated in plain C: a brute-force loop over every sphere and every triangle a chunk addresses, the six
 * sub-candidates of a triangle's key one after the other, the solid sphere's key, a FULL sort by (k, kind, primitive) and the count rule.
 * The checker of tests/test_gpu_capsule.py, itself pinned by tests/test_capsule_cpu.py (hand cases, nearest_oracle.c at d = 0, a float64
 * twin by golden section, and the mutants below).  TEST INFRASTRUCTURE: compiled by the tests with the oracle's own CFLAGS
 * (tests/checker_build.py: -ffp-contract=off, so every product and sum rounds on its own, as the header demands).  It includes nothing
 * but the public header.
 *
 * variant: 0 the definition;
 *          1 `<=` for `<` in the replacement rule of the sub-candidates;
 *          2 an edge sub-candidate's s is not clamped;
 *          3 a shell instead of a solid sphere (ds = |len - r|);
 *          4 the origin bound from P0 only (cp_origin_bound);
 *          12 .. 16: sub-candidate 2 .. 6 (endpoint P1, edge AB, edge AC, edge BC, piercing) is dropped.
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

static float clamp01(float x)
{
    x = x < 0.0f ? 0.0f : x;
    return x > 1.0f ? 1.0f : x;
}

typedef struct { v3 p0, d, p1; float R, dd; } seg;

/* ---- the closest-point queries' triangle key from a point, operation for operation (closest_oracle.c, nearest_oracle.c) ---- */
static float point_triangle(v3 p, v3 A, v3 eAB, v3 eAC, float* pu, float* pv)
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

/* ---- the clamped closest pair of the segment and the edge E0 + e t (Ericson 5.1.9), the header's operation order ---- */
static void segment_edge(const seg* g, v3 E0, v3 e, int variant, float* ps, float* pt)
{
    const v3 r = sub(g->p0, E0);
    const float ee = dot(e, e), f = dot(e, r), c = dot(g->d, r), b = dot(g->d, e);
    const float den = g->dd * ee - b * b;
    float s0 = 0.0f;
    if (den > 0.0f) { s0 = (b * f - c * ee) / den; if (variant != 2) s0 = clamp01(s0); }
    const float t0 = (b * s0 + f) / ee;
    if (ee == 0.0f || t0 < 0.0f) { *pt = 0.0f; *ps = -c / g->dd; if (variant != 2) *ps = clamp01(*ps); }
    else if (t0 > 1.0f) { *pt = 1.0f; *ps = (b - c) / g->dd; if (variant != 2) *ps = clamp01(*ps); }
    else { *pt = t0; *ps = s0; }
}

/* ---- the two-sided RayTriangle of the multi-hit queries (hits_oracle.c): nonzero when |det| >= 1e-6f and dst, u, v, w >= 0 ---- */
static int ray_triangle_both(v3 o, v3 d, v3 A, v3 eAB, v3 eAC, float* dst, float* u, float* v)
{
    const v3 n = cross(eAB, eAC);
    const v3 ao = sub(o, A);
    const v3 dao = cross(ao, d);
    const float det = -dot(d, n);
    const float inv = copysignf(1.0f / fabsf(det), det);
    *dst = dot(ao, n) * inv;
    *u = dot(eAC, dao) * inv;
    *v = -dot(eAB, dao) * inv;
    const float w = 1.0f - *u - *v;
    if (!(*dst >= 0.0f && *u >= 0.0f && *v >= 0.0f && w >= 0.0f)) return 0;
    return det >= 1e-6f ? 1 : det <= -1e-6f ? -1 : 0;
}

typedef struct { float k, s, u, v; int pierced; } tkey;

static int replaces(float ck, float k, int variant) { return variant == 1 ? ck <= k : ck < k; }

/* x = P0 + d s, q = (A + eAB u) + eAC v, k = dot(x - q, x - q): the key of every sub-candidate but the endpoints' */
static void pair(const seg* g, v3 A, v3 eAB, v3 eAC, float s, float u, float v, int pierced, int variant, tkey* best)
{
    const v3 x = add(g->p0, scale(g->d, s));
    const v3 q = add(add(A, scale(eAB, u)), scale(eAC, v));
    const v3 e = sub(x, q);
    const float ck = dot(e, e);
    if (replaces(ck, best->k, variant)) { best->k = ck; best->s = s; best->u = u; best->v = v; best->pierced = pierced; }
}

static tkey segment_triangle(const seg* g, const rt_triangle* t, int variant)
{
    const v3 A = ld(t->posA), eAB = sub(ld(t->posB), A), eAC = sub(ld(t->posC), A);
    tkey best;
    best.k = point_triangle(g->p0, A, eAB, eAC, &best.u, &best.v);
    best.s = 0.0f; best.pierced = 0;
    if (g->dd == 0.0f) return best;
    if (variant != 12) {
        float u, v;
        const float k = point_triangle(g->p1, A, eAB, eAC, &u, &v);
        if (replaces(k, best.k, variant)) { best.k = k; best.s = 1.0f; best.u = u; best.v = v; }
    }
    float s, e;
    if (variant != 13) { segment_edge(g, A, eAB, variant, &s, &e); pair(g, A, eAB, eAC, s, e, 0.0f, 0, variant, &best); }
    if (variant != 14) { segment_edge(g, A, eAC, variant, &s, &e); pair(g, A, eAB, eAC, s, 0.0f, e, 0, variant, &best); }
    if (variant != 15) { segment_edge(g, add(A, eAB), sub(eAC, eAB), variant, &s, &e); pair(g, A, eAB, eAC, s, 1.0f - e, e, 0, variant, &best); }
    if (variant != 16) {
        float pt, pu, pv;
        if (ray_triangle_both(g->p0, g->d, A, eAB, eAC, &pt, &pu, &pv) != 0 && pt <= 1.0f) pair(g, A, eAB, eAC, pt, pu, pv, 1, variant, &best);
    }
    return best;
}

typedef struct { float s, len, ds; v3 m; } skey;

static float segment_sphere(const seg* g, const rt_sphere* sp, int variant, skey* o)
{
    const v3 c = ld(sp->position);
    const float t = clamp01(dot(sub(c, g->p0), g->d) / g->dd);
    o->s = g->dd == 0.0f ? 0.0f : t;
    const v3 x = add(g->p0, scale(g->d, o->s));
    o->m = sub(x, c);
    o->len = sqrtf(dot(o->m, o->m));
    float ds = o->len - sp->radius;
    if (variant == 3) ds = fabsf(ds);
    else ds = ds < 0.0f ? 0.0f : ds;
    o->ds = ds;
    return ds * ds;
}

static void miss(rt_closest* o, int count)
{
    memset(o, 0, sizeof *o);
    o->dst = INFINITY;
    o->kind = RT_HIT_NONE;
    o->primitive = o->chunk = o->mesh = -1;
    o->_reserved[0] = count;
}

typedef struct { float k, s, u, v; int pierced, kind; uint32_t prim; int chunk; } cand;

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

static void record(rt_closest* o, const seg* g, const cand* c, const rt_sphere* spheres, const rt_triangle* tris, const int32_t* chunk_mesh,
                   int count, int variant)
{
    miss(o, count);
    o->kind = c->kind;
    o->primitive = (int32_t)c->prim;
    memcpy(&o->_reserved[1], &c->s, sizeof(float));
    if (c->kind == RT_HIT_SPHERE) {
        const rt_sphere* s = &spheres[c->prim];
        skey k;
        segment_sphere(g, s, variant, &k);
        const v3 ce = ld(s->position);
        const v3 q = add(ce, scale(k.m, s->radius / k.len));
        const v3 nn = normalize(sub(q, ce));
        o->dst = k.ds;
        o->point[0] = q.x; o->point[1] = q.y; o->point[2] = q.z;
        o->normal[0] = nn.x; o->normal[1] = nn.y; o->normal[2] = nn.z;
        o->side = k.len >= s->radius ? 1 : -1;
    } else {
        const rt_triangle* t = &tris[c->prim];
        const v3 A = ld(t->posA), eAB = sub(ld(t->posB), A), eAC = sub(ld(t->posC), A);
        const v3 x = add(g->p0, scale(g->d, c->s));
        const v3 q = add(add(A, scale(eAB, c->u)), scale(eAC, c->v));
        const v3 e = sub(x, q);
        const float sd = dot(e, cross(eAB, eAC));
        const float w = 1.0f - c->u - c->v;
        const v3 nn = normalize(add(add(scale(ld(t->normalA), w), scale(ld(t->normalB), c->u)), scale(ld(t->normalC), c->v)));
        o->dst = sqrtf(c->k);
        o->point[0] = q.x; o->point[1] = q.y; o->point[2] = q.z;
        o->normal[0] = nn.x; o->normal[1] = nn.y; o->normal[2] = nn.z;
        o->chunk = c->chunk;
        o->mesh = chunk_mesh ? chunk_mesh[c->chunk] : -1;
        o->u = c->u; o->v = c->v;
        o->side = c->pierced ? 0 : sd > 0.0f ? 1 : sd < 0.0f ? -1 : 0;
    }
}

static int searched(const rt_ray* b, seg* g)
{
    g->p0 = ld(b->origin); g->d = ld(b->direction); g->p1 = add(g->p0, g->d);
    g->R = b->tMax; g->dd = dot(g->d, g->d);
    if (!(b->tMax > 0.0f)) return 0;
    const float co[9] = { g->p0.x, g->p0.y, g->p0.z, g->d.x, g->d.y, g->d.z, g->p1.x, g->p1.y, g->p1.z };
    for (int a = 0; a < 9; a++) if (!(fabsf(co[a]) <= 3.4028235e38f)) return 0;
    return 1;
}

/* The origin bound of a batch: the largest finite |coordinate| of P0 and of P0 + d over the inputs with tMax > 0 */
float cp_origin_bound(const rt_ray* segs, int n, int variant)
{
    float m = 0.0f;
    for (int i = 0; i < n; i++) {
        if (!(segs[i].tMax > 0.0f)) continue;
        for (int a = 0; a < 3; a++) {
            const float v = fabsf(segs[i].origin[a]), w = fabsf(segs[i].origin[a] + segs[i].direction[a]);
            if (v > m && v <= 3.4028235e38f) m = v;
            if (variant != 4 && w > m && w <= 3.4028235e38f) m = w;
        }
    }
    return m;
}

/* keys[i * (ns + nt) + j] = the key of primitive j (the spheres, then ALL nt triangles in uploaded order) for segment i, and params[..] its
 * s; NaN for a segment that is not searched.  For the twins of tests/test_capsule_cpu.py. */
int cp_keys(const rt_sphere* spheres, int ns, const rt_triangle* tris, int nt, const rt_ray* segs, int n, int variant, float* keys, float* params)
{
    for (int i = 0; i < n; i++) {
        float* ko = keys + (size_t)i * ((size_t)ns + nt);
        float* po = params + (size_t)i * ((size_t)ns + nt);
        seg g;
        const int ok = searched(&segs[i], &g);
        for (int s = 0; s < ns; s++) { skey k; ko[s] = ok ? segment_sphere(&g, &spheres[s], variant, &k) : NAN; po[s] = ok ? k.s : NAN; }
        for (int t = 0; t < nt; t++) {
            if (!ok) { ko[ns + t] = po[ns + t] = NAN; continue; }
            const tkey k = segment_triangle(&g, &tris[t], variant);
            ko[ns + t] = k.k; po[ns + t] = k.s;
        }
    }
    return 0;
}

/* out[i * K + j] = record j of segs[i].  chunk_mesh: per chunk its mesh index (a local-mesh scene), or NULL (mesh = -1).  totals (may be
 * NULL): per segment, the number of ALL candidates below R * R, whatever K and all are.  kth_ties (may be NULL): per segment, 1 when the
 * K-th and the (K+1)-th key of the full sort are bit-equal.  -3: a chunk's range leaves the triangle buffer; -4: K or all out of range;
 * -5: out of memory. */
int cp_capsule(const rt_sphere* spheres, int ns, const rt_triangle* tris, int nt, const rt_meshinfo* mi, int nm, const int32_t* chunk_mesh,
               const rt_ray* segs, int n, int K, int all, int variant, rt_closest* out, int32_t* totals, int32_t* kth_ties)
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
        seg g;
        if (!searched(&segs[i], &g)) continue;
        const float r2 = g.R * g.R;
        cand* cd = (cand*)malloc(sizeof(cand) * ((size_t)ns + addressed + 1));
        if (!cd) { failed = 1; continue; }
        int total = 0;
        for (int s = 0; s < ns; s++) {
            skey sk;
            const float k = segment_sphere(&g, &spheres[s], variant, &sk);
            if (!(k < r2)) continue;
            cand e = { k, sk.s, 0.0f, 0.0f, 0, RT_HIT_SPHERE, (uint32_t)s, -1 };
            cd[total++] = e;
        }
        for (int m = 0; m < nm; m++)
            for (uint32_t j = 0; j < mi[m].numTriangles; j++) {
                const uint32_t t = mi[m].firstTriangleIndex + j;
                const tkey tk = segment_triangle(&g, &tris[t], variant);
                if (!(tk.k < r2)) continue;
                cand e = { tk.k, tk.s, tk.u, tk.v, tk.pierced, RT_HIT_TRIANGLE, t, m };
                cd[total++] = e;
            }
        qsort(cd, (size_t)total, sizeof(cand), by_key);
        const int listed = total < K ? total : K;
        if (kth_ties && total > K && cd[K - 1].k == cd[K].k) kth_ties[i] = 1;
        if (totals) totals[i] = total;
        const int count = all ? total : listed;
        for (int j = 0; j < K; j++) {
            if (j < listed) record(&o[j], &g, &cd[j], spheres, tris, chunk_mesh, count, variant);
            else miss(&o[j], count);
        }
        free(cd);
    }
    return failed ? -5 : 0;
}
