/*
 * sweep_all_oracle.c — sphere-cast-all (include/rt.h "sphere-cast-all": option "hits_sweep" = 1 on rt_trace_hits) restated in plain C as a
 * brute-force loop over every sphere and every triangle a chunk addresses, and a sort: the checker of tests/test_gpu_sweep_all.py, itself
 * pinned by tests/test_sweep_all_cpu.py (against sw_cast on one-primitive scenes, hand cases).  TEST INFRASTRUCTURE: compiled by the tests
 * with the oracle's own CFLAGS (tests/checker_build.py).  It includes the sphere casts' checker unchanged and forms every primitive's
 * candidate with that file's own ray_sphere, feature and triangle_key: the definition of a contact is the sphere casts' own.
 */
#include "sweep_oracle.c"

typedef struct swa_cand {
    float t, u, v;
    int32_t kind, chunk, feat;
    uint32_t prim;
    v3 point;
} swa_cand;

/* ascending (t, kind, primitive); t compares as a float: -0.0f == 0.0f */
static int swa_less(const void* pa, const void* pb)
{
    const swa_cand* a = (const swa_cand*)pa;
    const swa_cand* b = (const swa_cand*)pb;
    if (a->t < b->t) return -1;
    if (a->t > b->t) return 1;
    if (a->kind != b->kind) return a->kind < b->kind ? -1 : 1;
    if (a->prim != b->prim) return a->prim < b->prim ? -1 : 1;
    return 0;
}

static void swa_empty(rt_multihit* o, int count)
{
    memset(o, 0, sizeof *o);
    o->dst = INFINITY;
    o->kind = RT_HIT_NONE;
    o->primitive = o->chunk = o->mesh = -1;
    o->hitCount = count;
}

/* out[i * K + j] = record j of rays[i]: the first K candidates in order, then empty records; hitCount = min(total, K), or total when
 * count_all.  chunk_mesh: per chunk its mesh index (a local-mesh scene), or NULL (mesh = -1).  -3: a chunk's range leaves the triangle
 * buffer; -4: out of memory. */
int swa_cast(const rt_sphere* spheres, int ns, const rt_triangle* tris, int nt, const rt_meshinfo* mi, int nm, const int32_t* chunk_mesh,
             const rt_ray* rays, int n, int K, int count_all, rt_multihit* out)
{
    size_t cap = (size_t)ns + 1;
    for (int m = 0; m < nm; m++) {
        if ((uint64_t)mi[m].firstTriangleIndex + mi[m].numTriangles > (uint64_t)nt) return -3;
        cap += mi[m].numTriangles;
    }
    int failed = 0;
#pragma omp parallel for schedule(dynamic, 16)
    for (int i = 0; i < n; i++) {
        rt_multihit* rec = out + (size_t)i * (size_t)K;
        for (int j = 0; j < K; j++) swa_empty(&rec[j], 0);
        const v3 o = ld(rays[i].origin), d = ld(rays[i].direction);
        const float t_max = rays[i].tMax;
        float r;
        memcpy(&r, &rays[i]._reserved, sizeof r);
        if (!(t_max > 0.0f) || !(r > 0.0f) || !(r <= 3.4028235e38f)) continue;     /* not traced */
        swa_cand* c = (swa_cand*)malloc(cap * sizeof *c);
        if (!c) { failed = 1; continue; }
        const float g = r * (1.0f + 0x1p-6f), g2 = g * g;
        int total = 0;
        for (int s = 0; s < ns; s++) {
            float t;
            if (!ray_sphere(o, d, ld(spheres[s].position), spheres[s].radius + r, &t) || !(t < t_max)) continue;
            swa_cand* k = &c[total++];
            memset(k, 0, sizeof *k);
            k->t = t; k->kind = RT_HIT_SPHERE; k->prim = (uint32_t)s; k->chunk = -1;
        }
        for (int m = 0; m < nm; m++)
            for (uint32_t j = 0; j < mi[m].numTriangles; j++) {
                const uint32_t ti = mi[m].firstTriangleIndex + j;
                const v3 A = ld(tris[ti].posA), eAB = sub(ld(tris[ti].posB), A), eAC = sub(ld(tris[ti].posC), A);
                /* the triangle's candidate: codes in ascending order, strict '<' keeps the lower code at a tie (as sw_cast) */
                swa_cand best;
                int have = 0;
                for (int code = 1; code <= 8; code++) {
                    float t, u, v, ku, kv;
                    v3 point;
                    if (!feature(code, o, d, r, A, eAB, eAC, &t, &point, &u, &v) || !(t < t_max)) continue;
                    if (!(triangle_key(add(o, scale(d, t)), A, eAB, eAC, &ku, &kv) <= g2)) continue;
                    if (!have || t < best.t) {
                        have = 1;
                        best.t = t; best.u = u; best.v = v; best.kind = RT_HIT_TRIANGLE; best.chunk = m; best.feat = code; best.prim = ti; best.point = point;
                    }
                }
                if (have) c[total++] = best;
            }
        qsort(c, (size_t)total, sizeof *c, swa_less);
        const int count = count_all ? total : (total < K ? total : K);
        for (int j = 0; j < K; j++) {
            rt_multihit* h = &rec[j];
            h->hitCount = count;
            if (j >= total) continue;
            const swa_cand* k = &c[j];
            const v3 centre = add(o, scale(d, k->t));
            v3 nn, bp;
            h->dst = k->t;
            h->kind = k->kind;
            h->primitive = (int32_t)k->prim;
            if (k->kind == RT_HIT_SPHERE) {
                nn = normalize(sub(centre, ld(spheres[k->prim].position)));
                bp = sub(centre, scale(nn, r));
                h->side = 1;
            } else {
                const uint32_t ti = k->prim;
                const v3 A = ld(tris[ti].posA), eAB = sub(ld(tris[ti].posB), A), eAC = sub(ld(tris[ti].posC), A);
                bp = k->point;
                nn = normalize(sub(centre, bp));
                h->chunk = k->chunk;
                h->mesh = chunk_mesh ? chunk_mesh[k->chunk] : -1;
                h->u = k->u; h->v = k->v;
                const float sd = dot(sub(centre, bp), cross(eAB, eAC));
                h->side = sd > 0.0f ? 1 : sd < 0.0f ? -1 : 0;
                h->_reserved = k->feat;
            }
            h->hitPoint[0] = bp.x; h->hitPoint[1] = bp.y; h->hitPoint[2] = bp.z;
            h->normal[0] = nn.x; h->normal[1] = nn.y; h->normal[2] = nn.z;
        }
        free(c);
    }
    return failed ? -4 : 0;
}
