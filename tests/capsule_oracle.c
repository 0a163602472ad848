/*
 * capsule_oracle.c — capsule overlap queries (include/rt.h "capsule overlap queries": rt_closest_points with the option
 * "closest_capsule" = 1) restated in plain C: a brute-force loop over every sphere and every triangle a chunk addresses, the six
 * sub-candidates of a triangle's key one after the other, the solid sphere's key, a FULL sort by (k, kind, primitive) and the count rule.
 * The checker of tests/test_gpu_capsule.py, itself pinned by tests/test_capsule_cpu.py (hand cases, nearest_oracle.c at d = 0, a float64
 * twin by golden section, and the mutants below).  TEST INFRASTRUCTURE: compiled by the tests with the oracle's own CFLAGS
 * (tests/checker_build.py: -ffp-contract=off, so every product and sum rounds on its own, as the header demands).  It includes nothing
 * but the public header, through point_oracle.h: the vectors, the point's triangle key (sub-candidates 1 and 2), the miss record, a
 * triangle's record, the order of the list and the list's driver (the argument check, the sort, the count rule, the K writes) live there,
 * shared with the other point checkers.  Here: the segment's keys, its record, `searched`, the origin bound, and the loop.
 *
 * variant: 0 the definition;
 *          1 `<=` for `<` in the replacement rule of the sub-candidates;
 *          2 an edge sub-candidate's s is not clamped;
 *          3 a shell instead of a solid sphere (ds = |len - r|);
 *          4 the origin bound from P0 only (cp_origin_bound);
 *          12 .. 16: sub-candidate 2 .. 6 (endpoint P1, edge AB, edge AC, edge BC, piercing) is dropped.
 */
#include "point_oracle.h"

static float clamp01(float x)
{
    x = x < 0.0f ? 0.0f : x;
    return x > 1.0f ? 1.0f : x;
}

typedef struct { v3 p0, d, p1; float R, dd; } seg;

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
    best.k = triangle_key(g->p0, A, eAB, eAC, &best.u, &best.v);
    best.s = 0.0f; best.pierced = 0;
    if (g->dd == 0.0f) return best;
    if (variant != 12) {
        float u, v;
        const float k = triangle_key(g->p1, A, eAB, eAC, &u, &v);
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

/* the capsule's own record: s in _reserved[1]; a SOLID sphere; the triangle's fields seen from x = P0 + d s (point_oracle.h's, operation
 * for operation), and side 0 where the segment pierces it */
static void record(rt_closest* o, const void* input, const cand* c, const list_scene* sc, int count)
{
    const seg* g = (const seg*)input;
    miss(o, count);
    o->kind = c->kind;
    o->primitive = (int32_t)c->prim;
    memcpy(&o->_reserved[1], &c->s, sizeof(float));
    if (c->kind == RT_HIT_SPHERE) {
        const rt_sphere* s = &sc->spheres[c->prim];
        skey k;
        segment_sphere(g, s, sc->variant, &k);
        const v3 ce = ld(s->position);
        const v3 q = add(ce, scale(k.m, s->radius / k.len));
        const v3 nn = normalize(sub(q, ce));
        o->dst = k.ds;
        o->point[0] = q.x; o->point[1] = q.y; o->point[2] = q.z;
        o->normal[0] = nn.x; o->normal[1] = nn.y; o->normal[2] = nn.z;
        o->side = k.len >= s->radius ? 1 : -1;
    } else {
        record_triangle(o, add(g->p0, scale(g->d, c->s)), c, sc->tris, sc->chunk_mesh);
        if (c->pierced) o->side = 0;
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
    size_t addressed;
    const int bad = list_check(mi, nm, nt, K, all, &addressed);
    if (bad) return bad;
    const list_scene scene = { spheres, tris, chunk_mesh, variant };
    int failed = 0;
#pragma omp parallel for schedule(dynamic, 16)
    for (int i = 0; i < n; i++) {
        rt_closest* o = &out[(size_t)i * K];
        list_clear(o, K, totals, kth_ties, i);
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
            const cand e = { .k = k, .s = sk.s, .kind = RT_HIT_SPHERE, .prim = (uint32_t)s, .chunk = -1 };
            cd[total++] = e;
        }
        for (int m = 0; m < nm; m++)
            for (uint32_t j = 0; j < mi[m].numTriangles; j++) {
                const uint32_t t = mi[m].firstTriangleIndex + j;
                const tkey tk = segment_triangle(&g, &tris[t], variant);
                if (!(tk.k < r2)) continue;
                const cand e = { .k = tk.k, .s = tk.s, .u = tk.u, .v = tk.v, .pierced = tk.pierced, .kind = RT_HIT_TRIANGLE, .prim = t, .chunk = m };
                cd[total++] = e;
            }
        list_finish(o, cd, total, K, all, COUNT_RULE, record, &g, &scene, totals, kth_ties, i);
        free(cd);
    }
    return failed ? -5 : 0;
}
