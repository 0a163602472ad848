/*
 * sweep_oracle.c — sphere casts (include/rt.h "sphere casts": option "sweep" = 1 on rt_trace_rays / rt_occluded) restated in plain C as a
 * brute-force loop over every sphere and every triangle a chunk addresses: the checker of tests/test_gpu_sweep.py, itself pinned by
 * tests/test_sweep_cpu.py (analytic cases, a float64 twin).  TEST INFRASTRUCTURE: compiled by the tests with the oracle's own CFLAGS
 * (oracle/Makefile, tests/checker_build.py: -ffp-contract=off, so every product and sum below rounds on its own, as the header demands).
 * It includes nothing but the public header, through point_oracle.h, from which it takes the vectors and the closest-point queries'
 * triangle key: the definition is the library's own.
 */
#include "point_oracle.h"

/* RaySphere (RayTracing.shader:120-146): 1 and the near root when it is accepted */
static int ray_sphere(v3 o, v3 d, v3 centre, float radius, float* dst)
{
    const v3 oc = sub(o, centre);
    const float a = dot(d, d);
    const float b = 2.0f * dot(oc, d);
    const float c = dot(oc, oc) - radius * radius;
    const float disc = b * b - 4.0f * a * c;
    if (disc >= 0.0f) {
        *dst = (-b - sqrtf(disc)) / (2.0f * a);
        return *dst >= 0.0f;
    }
    return 0;
}

/* RayTriangle with both faces (the multi-hit queries' test): +1 front, -1 back, 0 none */
static int ray_triangle_sided(v3 o, v3 d, v3 A, v3 eAB, v3 eAC, v3 n, float* dst, float* u, float* v)
{
    const v3 ao = sub(o, A);
    const v3 dao = cross(ao, d);
    const float det = -dot(d, n);
    const float inv = 1.0f / det;
    *dst = dot(ao, n) * inv;
    *u = dot(eAC, dao) * inv;
    *v = -dot(eAB, dao) * inv;
    const float w = 1.0f - *u - *v;
    if (!(*dst >= 0.0f && *u >= 0.0f && *v >= 0.0f && w >= 0.0f)) return 0;
    return det >= 1e-6f ? 1 : det <= -1e-6f ? -1 : 0;
}

/* One feature of a triangle: 1 when it answers, with its time, contact point and (u, v).  code 1..8 as in the header. */
static int feature(int code, v3 o, v3 d, float r, v3 A, v3 eAB, v3 eAC, float* t, v3* point, float* u, float* v)
{
    const v3 B = add(A, eAB), C = add(A, eAC);
    *u = 0.0f; *v = 0.0f;
    if (code <= 2) {
        const v3 n = cross(eAB, eAC);
        const v3 N = scale(n, 1.0f / sqrtf(dot(n, n)));
        const v3 o2 = code == 1 ? sub(o, scale(N, r)) : add(o, scale(N, r));
        if (ray_triangle_sided(o2, d, A, eAB, eAC, n, t, u, v) != (code == 1 ? 1 : -1)) return 0;
        *point = add(o2, scale(d, *t));
        return 1;
    }
    if (code <= 5) {
        const v3 P = code == 5 ? B : A;
        const v3 e = code == 3 ? eAB : code == 4 ? eAC : sub(eAC, eAB);
        const v3 m = sub(o, P);
        const float ee = dot(e, e), md = dot(m, e), nd = dot(d, e), dd = dot(d, d);
        const float qa = ee * dd - nd * nd;
        const float qb = ee * dot(m, d) - nd * md;
        const float qc = ee * (dot(m, m) - r * r) - md * md;
        const float disc = qb * qb - qa * qc;
        if (!(qa > 0.0f && disc >= 0.0f)) return 0;
        *t = (-qb - sqrtf(disc)) / qa;
        const float s = md + *t * nd;
        if (!(*t >= 0.0f && s > 0.0f && s < ee)) return 0;
        const float q = s / ee;
        *point = add(P, scale(e, q));
        if (code == 3) *u = q;
        else if (code == 4) *v = q;
        else { *v = q; *u = 1.0f - q; }
        return 1;
    }
    *point = code == 6 ? A : code == 7 ? B : C;
    *u = code == 7 ? 1.0f : 0.0f;
    *v = code == 8 ? 1.0f : 0.0f;
    return ray_sphere(o, d, *point, r, t);
}

static void no_hit(rt_hit* o)
{
    memset(o, 0, sizeof *o);
    o->dst = INFINITY;
    o->kind = RT_HIT_NONE;
    o->primitive = o->chunk = o->mesh = -1;
}

/* out[i] = the sphere-cast record of rays[i]; occluded (may be NULL) [i] = 1 when it is a hit.  chunk_mesh: per chunk its mesh index (a
 * local-mesh scene), or NULL (mesh = -1).  second (may be NULL): per ray the time of the best candidate of ANOTHER primitive (+inf:
 * none) — how close the runner-up came.  -3: a chunk's range leaves the triangle buffer. */
int sw_cast(const rt_sphere* spheres, int ns, const rt_triangle* tris, int nt, const rt_meshinfo* mi, int nm, const int32_t* chunk_mesh,
            const rt_ray* rays, int n, rt_hit* out, uint8_t* occluded, float* second)
{
    for (int m = 0; m < nm; m++)
        if ((uint64_t)mi[m].firstTriangleIndex + mi[m].numTriangles > (uint64_t)nt) return -3;
#pragma omp parallel for schedule(dynamic, 16)
    for (int i = 0; i < n; i++) {
        rt_hit* h = &out[i];
        no_hit(h);
        if (occluded) occluded[i] = 0;
        if (second) second[i] = INFINITY;
        const v3 o = ld(rays[i].origin), d = ld(rays[i].direction);
        const float t_max = rays[i].tMax;
        float r;
        memcpy(&r, &rays[i]._reserved, sizeof r);
        if (!(t_max > 0.0f) || !(r > 0.0f) || !(r <= 3.4028235e38f)) continue;     /* not traced */
        const float g = r * (1.0f + 0x1p-6f), g2 = g * g;
        /* the smallest (t, kind, primitive, feature) with t < tMax */
        int have = 0, kind = 0, chunk = -1, feat = 0;
        uint32_t prim = 0;
        float best = 0.0f, bu = 0.0f, bv = 0.0f, runner = INFINITY;
        v3 bp = V(0, 0, 0);
        for (int s = 0; s < ns; s++) {
            float t;
            if (!ray_sphere(o, d, ld(spheres[s].position), spheres[s].radius + r, &t) || !(t < t_max)) continue;
            if (!have || t < best) {
                if (have) runner = best;
                have = 1; kind = RT_HIT_SPHERE; prim = (uint32_t)s; best = t;
            } else if (t < runner) runner = t;
        }
        for (int m = 0; m < nm; m++)
            for (uint32_t j = 0; j < mi[m].numTriangles; j++) {
                const uint32_t ti = mi[m].firstTriangleIndex + j;
                const v3 A = ld(tris[ti].posA), eAB = sub(ld(tris[ti].posB), A), eAC = sub(ld(tris[ti].posC), A);
                /* the triangle's own best: codes in ascending order, strict '<' keeps the lower code at a tie */
                int thave = 0, tfeat = 0;
                float tt = 0.0f, tu = 0.0f, tv = 0.0f;
                v3 tp = V(0, 0, 0);
                for (int code = 1; code <= 8; code++) {
                    float t, u, v, ku, kv;
                    v3 point;
                    if (!feature(code, o, d, r, A, eAB, eAC, &t, &point, &u, &v) || !(t < t_max)) continue;
                    /* the guard: the closest-point queries' key of the centre at t (point_oracle.h, include/rt.h "closest-point queries") */
                    if (!(triangle_key(add(o, scale(d, t)), A, eAB, eAC, &ku, &kv) <= g2)) continue;
                    if (!thave || t < tt) { thave = 1; tfeat = code; tt = t; tu = u; tv = v; tp = point; }
                }
                if (!thave) continue;
                if (!have || tt < best || (tt == best && kind == RT_HIT_TRIANGLE && ti < prim)) {
                    if (have) runner = best;
                    have = 1; kind = RT_HIT_TRIANGLE; prim = ti; best = tt; bu = tu; bv = tv; bp = tp; chunk = m; feat = tfeat;
                } else if (tt < runner) runner = tt;
            }
        if (!have) continue;
        if (occluded) occluded[i] = 1;
        if (second) second[i] = runner;
        const v3 centre = add(o, scale(d, best));
        v3 nn;
        h->kind = kind;
        h->primitive = (int32_t)prim;
        h->dst = best;
        if (kind == RT_HIT_SPHERE) {
            nn = normalize(sub(centre, ld(spheres[prim].position)));
            bp = sub(centre, scale(nn, r));
        } else {
            nn = normalize(sub(centre, bp));
            h->chunk = chunk;
            h->mesh = chunk_mesh ? chunk_mesh[chunk] : -1;
            h->u = bu; h->v = bv;
            h->_reserved[0] = feat;
        }
        h->hitPoint[0] = bp.x; h->hitPoint[1] = bp.y; h->hitPoint[2] = bp.z;
        h->normal[0] = nn.x; h->normal[1] = nn.y; h->normal[2] = nn.z;
    }
    return 0;
}
