/*
 * gather_oracle.c — gather queries (include/rt.h rt_gather) on the CPU oracle: the checker of tests/test_gpu_gather.py, itself pinned by
 * tests/test_gather_cpu.py.  TEST INFRASTRUCTURE: it includes the oracle unchanged and is compiled by the tests with the oracle's own
 * CFLAGS (oracle/Makefile).
 *
 * For point i of a call (origin o, normal n, tMax t), K = firstIndex + i:
 *   1. t <= 0 or NaN: every output float 0, nothing is drawn or cast;
 *   2. sample s draws R with the oracle's own random_direction() from rng.mode = RT_RNG_PHILOX, key (K, seed), rng.sample = s,
 *      rng_scope(&rng, 0xFFFFFFFE): words 0..3 of block 0xFFFFFFFE, words 0, 1 of block 0xFFFFFFFF;
 *      mode 0: d = v_normalize(n + R) (trace()'s own diffuse-lobe expression); mode 1: d = R;
 *   3. L_s = the radiance checker's per-sample rule for the ray (o, d, t) (tests/radiance_oracle.c, restated here): the oracle's own
 *      trace(o, d) with the same key and sample — trace() scopes its hits to blocks 1 + 2b, 2 + 2b itself — unless the hit of the cast at
 *      loop index 0 fails dst < t: then trace()'s miss branch at loop index 0 is all that runs, 0 + environment_light(d) * 1;
 *   4. mode 0: the channels are L_s.rgb; mode 1: L_s.c * Y_k(d), 27 channels; the Philox mode's fixed tree over the N samples,
 *      root / N; mode 1: * 12.566371f; alpha 1 (mode 1: for k = 0 only).
 */
#include "../oracle/rt_oracle.c"

enum { GTH_COSINE = 0, GTH_SH9 = 1 };

static orng gth_rng(uint32_t K, uint32_t seed, uint32_t s)
{
    orng rng; memset(&rng, 0, sizeof rng);
    rng.mode = RT_RNG_PHILOX;
    rng.key[0] = K; rng.key[1] = seed;
    rng.sample = s;
    return rng;
}

/* step 2 */
static v3 gth_dir(v3 n, int mode, uint32_t K, uint32_t seed, uint32_t s)
{
    orng rng = gth_rng(K, seed, s);
    rng_scope(&rng, 0xFFFFFFFEu);
    const v3 R = random_direction(&rng);
    return mode == GTH_SH9 ? R : v_normalize(v_add(n, R));
}

/* step 3 */
static v3 gth_one(const scene_t* sc, v3 o, v3 d, float t, uint32_t K, uint32_t seed, uint32_t s, orc_counts* cnt)
{
    if (sc->p->maxBounceCount >= 0) {                            /* (else trace() casts nothing) */
        orc_counts pre; memset(&pre, 0, sizeof pre);
        const hit_t h = calculate_ray_collision(sc, o, d, &pre);
        if (h.didHit && !(h.dst < t)) {                          /* the bounded miss */
            cnt->rays++;
            return v_add(V(0, 0, 0), v_mul(environment_light(sc->p, d), V(1, 1, 1)));
        }
    }
    orng rng = gth_rng(K, seed, s);
    return trace(sc, o, d, &rng, cnt);
}

static int gth_scene(scene_t* sc, const rt_params* params, const rt_sphere* spheres, int ns, const rt_triangle* tris, int nt,
                     const rt_meshinfo* mi, int nm)
{
    for (int m = 0; m < nm; m++)
        if ((uint64_t)mi[m].firstTriangleIndex + mi[m].numTriangles > (uint64_t)nt) return -3;
    scene_t s = { params, spheres, ns, tris, nt, mi, nm, params->intersectMode, NULL };
    *sc = s;
    return 0;
}

/* the nine basis values on d, as include/rt.h writes them (the oracle is compiled with -ffp-contract=off: every product rounds) */
static void gth_basis(v3 d, float Y[9])
{
    const float x = d.x, y = d.y, z = d.z;
    Y[0] = 0.28209479f;
    Y[1] = 0.48860251f * y;
    Y[2] = 0.48860251f * z;
    Y[3] = 0.48860251f * x;
    Y[4] = 1.09254843f * (x * y);
    Y[5] = 1.09254843f * (y * z);
    Y[6] = 0.31539157f * (3.0f * (z * z) - 1.0f);
    Y[7] = 1.09254843f * (x * z);
    Y[8] = 0.54627421f * (x * x - y * y);
}

/* out[i] = the gather query of points[i]: 4 floats (mode 0) or 36 (mode 1); accel != 0: triangles are found through the oracle's own
 * search tree; casts (may be NULL) = the calls of CalculateRayCollision the samples made (the pre-cast of step 3 not counted) */
int gth_gather(const rt_params* params, const rt_sphere* spheres, int ns, const rt_triangle* tris, int nt, const rt_meshinfo* mi, int nm,
               const rt_ray* points, int n, int samples, uint32_t seed, uint32_t firstIndex, int mode, int accel, float* out, uint64_t* casts)
{
    if (!params || n < 0 || (n > 0 && (!points || !out)) || samples < 1 || samples > 65536 || (mode != GTH_COSINE && mode != GTH_SH9)) return -1;
    scene_t sc;
    { int r = gth_scene(&sc, params, spheres, ns, tris, nt, mi, nm); if (r) return r; }
    oaccel* tree = accel ? accel_build(&sc) : NULL;
    sc.accel = tree;
    const int S = orc_philox_substreams(samples);
    const int NC = mode == GTH_SH9 ? 9 : 1;
    uint64_t total_casts = 0;
#pragma omp parallel for schedule(dynamic, 16) reduction(+ : total_casts)
    for (int i = 0; i < n; i++) {
        orc_counts cnt; memset(&cnt, 0, sizeof cnt);
        const rt_ray* r = &points[i];
        float* o4 = out + 4 * (size_t)NC * (size_t)i;
        if (!(r->tMax > 0.0f)) { for (int k = 0; k < 4 * NC; k++) o4[k] = 0.0f; continue; }
        const v3 o = v_load(r->origin), nrm = v_load(r->direction);
        const uint32_t K = firstIndex + (uint32_t)i;
        v3 part[9][16];
        for (int c = 0; c < NC; c++) for (int k = 0; k < 16; k++) part[c][k] = V(0, 0, 0);
        for (int s = 0; s < samples; s++) {
            const v3 d = gth_dir(nrm, mode, K, seed, (uint32_t)s);
            const v3 L = gth_one(&sc, o, d, r->tMax, K, seed, (uint32_t)s, &cnt);
            if (mode == GTH_SH9) {
                float Y[9];
                gth_basis(d, Y);
                for (int c = 0; c < 9; c++) part[c][s % S] = v_add(part[c][s % S], V(L.x * Y[c], L.y * Y[c], L.z * Y[c]));
            } else part[0][s % S] = v_add(part[0][s % S], L);
        }
        const float nf = (float)samples;
        for (int c = 0; c < NC; c++) {
            for (int step = 1; step < S; step <<= 1)
                for (int k = 0; k < S; k += 2 * step) part[c][k] = v_add(part[c][k], part[c][k + step]);
            const v3 m = V(part[c][0].x / nf, part[c][0].y / nf, part[c][0].z / nf);
            float* q = o4 + 4 * c;
            if (mode == GTH_SH9) { q[0] = m.x * 12.566371f; q[1] = m.y * 12.566371f; q[2] = m.z * 12.566371f; q[3] = c == 0 ? 1.0f : 0.0f; }
            else { q[0] = m.x; q[1] = m.y; q[2] = m.z; q[3] = 1.0f; }
        }
        total_casts += cnt.rays;
    }
    accel_free(tree);
    if (casts) *casts = total_casts;
    return 0;
}

/* rgb[0..2] = L of sample `sample` alone of one point with stream index `index` (what gth_gather feeds its tree, before the basis) */
int gth_sample(const rt_params* params, const rt_sphere* spheres, int ns, const rt_triangle* tris, int nt, const rt_meshinfo* mi, int nm,
               const rt_ray* point, uint32_t sample, uint32_t seed, uint32_t index, int mode, int accel, float* rgb)
{
    if (!params || !point || !rgb) return -1;
    scene_t sc;
    { int r = gth_scene(&sc, params, spheres, ns, tris, nt, mi, nm); if (r) return r; }
    oaccel* tree = accel ? accel_build(&sc) : NULL;
    sc.accel = tree;
    orc_counts cnt; memset(&cnt, 0, sizeof cnt);
    v3 c = V(0, 0, 0);
    if (point->tMax > 0.0f) {
        const v3 d = gth_dir(v_load(point->direction), mode, index, seed, sample);
        c = gth_one(&sc, v_load(point->origin), d, point->tMax, index, seed, sample, &cnt);
    }
    rgb[0] = c.x; rgb[1] = c.y; rgb[2] = c.z;
    accel_free(tree);
    return 0;
}

/* d[0..2] = the direction of sample `sample` of a point with normal `normal` and stream index `index` */
int gth_direction(const float* normal, uint32_t sample, uint32_t seed, uint32_t index, int mode, float* d)
{
    if (!normal || !d) return -1;
    const v3 v = gth_dir(v_load(normal), mode, index, seed, sample);
    d[0] = v.x; d[1] = v.y; d[2] = v.z;
    return 0;
}
