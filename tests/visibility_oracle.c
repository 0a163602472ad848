/*
 * visibility_oracle.c — visibility gathers (include/rt.h rt_visibility) on the CPU oracle: the checker of tests/test_gpu_visibility.py,
 * itself pinned by tests/test_visibility_cpu.py.  TEST INFRASTRUCTURE: it includes the oracle unchanged and is compiled by the tests
 * with the oracle's own CFLAGS (oracle/Makefile).
 *
 * For point i of a call (origin o, normal n, reach t), K = firstIndex + i:
 *   1. t <= 0 or NaN: every output float 0, nothing is drawn or cast;
 *   2. sample s draws R with the oracle's own random_direction() from rng.mode = RT_RNG_PHILOX, key (K, seed), rng.sample = s,
 *      rng_scope(&rng, 0xFFFFFFFE): words 0..3 of block 0xFFFFFFFE, words 0, 1 of block 0xFFFFFFFF (the gather checker's draw);
 *      modes 0, 2: d = v_normalize(n + R); mode 1: d = R;
 *   3. h = the oracle's calculate_ray_collision(o, d); it is a hit when h.didHit and h.dst < t — the rule tests/ray_query_oracle.c
 *      states for rt_trace_rays and rt_occluded.  Modes 0, 1: v = hit ? 0 : 1.  Mode 2: r = hit ? h.dst : t, hit = 1 / 0;
 *   4. channels: mode 0 (v ? d : 0, v); mode 1 (v ? Y_k(d) : 0, k = 0..8, then v); mode 2 (r, r * r, hit); the Philox mode's fixed
 *      tree over the N samples per channel, root / N; mode 1: coefficients 0..8 * 12.566371f after the division, floats 10, 11 = 0;
 *      mode 2: the fourth float is 1.
 */
#include "../oracle/rt_oracle.c"

enum { VIS_COSINE = 0, VIS_SH9 = 1, VIS_DISTANCE = 2 };

/* step 2 */
static v3 vis_dir(v3 n, int mode, uint32_t K, uint32_t seed, uint32_t s)
{
    orng rng; memset(&rng, 0, sizeof rng);
    rng.mode = RT_RNG_PHILOX;
    rng.key[0] = K; rng.key[1] = seed;
    rng.sample = s;
    rng_scope(&rng, 0xFFFFFFFEu);
    const v3 R = random_direction(&rng);
    return mode == VIS_SH9 ? R : v_normalize(v_add(n, R));
}

/* step 3: returns hit (1 / 0); *r = the distance mode 2 sums */
static int vis_cast(const scene_t* sc, v3 o, v3 d, float t, float* r)
{
    orc_counts cnt; memset(&cnt, 0, sizeof cnt);
    const hit_t h = calculate_ray_collision(sc, o, d, &cnt);
    const int hit = h.didHit && h.dst < t;
    *r = hit ? h.dst : t;
    return hit;
}

static int vis_scene(scene_t* sc, rt_params* p, int intersect, const rt_sphere* spheres, int ns, const rt_triangle* tris, int nt,
                     const rt_meshinfo* mi, int nm)
{
    for (int m = 0; m < nm; m++)
        if ((uint64_t)mi[m].firstTriangleIndex + mi[m].numTriangles > (uint64_t)nt) return -3;
    memset(p, 0, sizeof *p);
    p->intersectMode = intersect;
    scene_t s = { p, spheres, ns, tris, nt, mi, nm, intersect, NULL };
    *sc = s;
    return 0;
}

/* the nine basis values on d, as include/rt.h writes them (the oracle is compiled with -ffp-contract=off: every product rounds) */
static void vis_basis(v3 d, float Y[9])
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

/* the channels of one sample (step 4, before the tree); returns their number: 4, 10 or 3 */
static int vis_channels(const scene_t* sc, const rt_ray* pt, int mode, uint32_t K, uint32_t seed, uint32_t s, float ch[10])
{
    const v3 d = vis_dir(v_load(pt->direction), mode, K, seed, s);
    float r;
    const int hit = vis_cast(sc, v_load(pt->origin), d, pt->tMax, &r);
    if (mode == VIS_DISTANCE) { ch[0] = r; ch[1] = r * r; ch[2] = hit ? 1.0f : 0.0f; return 3; }
    const int v = !hit;
    if (mode == VIS_SH9) {
        float Y[9];
        vis_basis(d, Y);
        for (int k = 0; k < 9; k++) ch[k] = v ? Y[k] : 0.0f;
        ch[9] = v ? 1.0f : 0.0f;
        return 10;
    }
    ch[0] = v ? d.x : 0.0f; ch[1] = v ? d.y : 0.0f; ch[2] = v ? d.z : 0.0f; ch[3] = v ? 1.0f : 0.0f;
    return 4;
}

/* out[i] = the visibility gather of points[i]: 4 floats (modes 0, 2) or 12 (mode 1); intersect = the intersectMode that applies;
 * accel != 0: triangles are found through the oracle's own search tree */
int vis_gather(const rt_sphere* spheres, int ns, const rt_triangle* tris, int nt, const rt_meshinfo* mi, int nm, int intersect,
               const rt_ray* points, int n, int samples, uint32_t seed, uint32_t firstIndex, int mode, int accel, float* out)
{
    if (n < 0 || (n > 0 && (!points || !out)) || samples < 1 || samples > 65536 || mode < VIS_COSINE || mode > VIS_DISTANCE) return -1;
    scene_t sc; rt_params p;
    { int r = vis_scene(&sc, &p, intersect, spheres, ns, tris, nt, mi, nm); if (r) return r; }
    oaccel* tree = accel ? accel_build(&sc) : NULL;
    sc.accel = tree;
    const int S = orc_philox_substreams(samples);
    const int NF = mode == VIS_SH9 ? 12 : 4;
#pragma omp parallel for schedule(dynamic, 16)
    for (int i = 0; i < n; i++) {
        const rt_ray* r = &points[i];
        float* o = out + (size_t)NF * (size_t)i;
        for (int k = 0; k < NF; k++) o[k] = 0.0f;
        if (!(r->tMax > 0.0f)) continue;
        const uint32_t K = firstIndex + (uint32_t)i;
        float part[10][16];
        for (int c = 0; c < 10; c++) for (int k = 0; k < 16; k++) part[c][k] = 0.0f;
        int NC = 0;
        for (int s = 0; s < samples; s++) {
            float ch[10];
            NC = vis_channels(&sc, r, mode, K, seed, (uint32_t)s, ch);
            for (int c = 0; c < NC; c++) part[c][s % S] = part[c][s % S] + ch[c];
        }
        const float nf = (float)samples;
        for (int c = 0; c < NC; c++) {
            for (int step = 1; step < S; step <<= 1)
                for (int k = 0; k < S; k += 2 * step) part[c][k] = part[c][k] + part[c][k + step];
            const float m = part[c][0] / nf;
            o[c] = (mode == VIS_SH9 && c < 9) ? m * 12.566371f : m;
        }
        if (mode == VIS_DISTANCE) o[3] = 1.0f;
    }
    accel_free(tree);
    return 0;
}

/* ch[0..] = the channels of sample `sample` alone of one point with stream index `index` (what vis_gather feeds its tree): 4, 10 or 3
 * floats; returns their number, or a negative error.  A point that is not traced has no samples: -2 */
int vis_sample(const rt_sphere* spheres, int ns, const rt_triangle* tris, int nt, const rt_meshinfo* mi, int nm, int intersect,
               const rt_ray* point, uint32_t sample, uint32_t seed, uint32_t index, int mode, int accel, float* ch)
{
    if (!point || !ch || mode < VIS_COSINE || mode > VIS_DISTANCE) return -1;
    if (!(point->tMax > 0.0f)) return -2;
    scene_t sc; rt_params p;
    { int r = vis_scene(&sc, &p, intersect, spheres, ns, tris, nt, mi, nm); if (r) return r; }
    oaccel* tree = accel ? accel_build(&sc) : NULL;
    sc.accel = tree;
    const int NC = vis_channels(&sc, point, mode, index, seed, sample, ch);
    accel_free(tree);
    return NC;
}

/* d[0..2] = the direction of sample `sample` of a point with normal `normal` and stream index `index` */
int vis_direction(const float* normal, uint32_t sample, uint32_t seed, uint32_t index, int mode, float* d)
{
    if (!normal || !d) return -1;
    const v3 v = vis_dir(v_load(normal), mode, index, seed, sample);
    d[0] = v.x; d[1] = v.y; d[2] = v.z;
    return 0;
}
