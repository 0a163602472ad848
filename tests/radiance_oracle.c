/*
 * radiance_oracle.c — radiance queries (include/rt.h rt_trace_radiance) on the CPU oracle: the checker of tests/test_gpu_radiance.py,
 * itself pinned by tests/test_radiance_cpu.py.  TEST INFRASTRUCTURE: it includes the oracle unchanged and is compiled by the tests
 * with the oracle's own CFLAGS (oracle/Makefile).
 *
 * For ray i of a call (origin o, direction d, tMax t), K = firstIndex + i:
 *   1. t <= 0 or NaN: (0, 0, 0, 0), nothing is cast;
 *   2. sample s is the oracle's own trace(o, d) with rng.mode = RT_RNG_PHILOX, key (K, seed), rng.sample = s — trace() scopes the draws
 *      of the hit at loop index b to blocks 1 + 2b, 2 + 2b itself; block 0 stays unused;
 *   3. the first-cast bound, applied as ray_query_oracle.c applies it: calculate_ray_collision, then the comparison.  When the hit of the
 *      cast at loop index 0 fails dst < t that cast is a miss, and trace()'s miss branch at loop index 0 is all that runs:
 *      incomingLight (0) + environment_light(d) * rayColour (1).  It draws nothing, so every sample of the ray has that value;
 *   4. the N samples are summed by the Philox mode's fixed tree (frag's), root / N, alpha 1.
 */
#include "../oracle/rt_oracle.c"

/* one sample of one ray (step 2 and 3); `bounded_miss`: step 3 applies */
static v3 rad_one(const scene_t* sc, v3 o, v3 d, int bounded_miss, uint32_t K, uint32_t seed, uint32_t s, orc_counts* cnt)
{
    if (bounded_miss) {
        cnt->rays++;
        return v_add(V(0, 0, 0), v_mul(environment_light(sc->p, d), V(1, 1, 1)));
    }
    orng rng; memset(&rng, 0, sizeof rng);
    rng.mode = RT_RNG_PHILOX;
    rng.key[0] = K; rng.key[1] = seed;
    rng.sample = s;
    return trace(sc, o, d, &rng, cnt);
}

/* does the cast at loop index 0 hit something that the bound t rejects? */
static int rad_bounded_miss(const scene_t* sc, v3 o, v3 d, float t)
{
    if (sc->p->maxBounceCount < 0) return 0;                    /* trace() casts nothing */
    orc_counts cnt; memset(&cnt, 0, sizeof cnt);
    const hit_t h = calculate_ray_collision(sc, o, d, &cnt);
    return h.didHit && !(h.dst < t);
}

static int rad_scene(scene_t* sc, const rt_params* params, const rt_sphere* spheres, int ns, const rt_triangle* tris, int nt,
                     const rt_meshinfo* mi, int nm)
{
    for (int m = 0; m < nm; m++)
        if ((uint64_t)mi[m].firstTriangleIndex + mi[m].numTriangles > (uint64_t)nt) return -3;
    scene_t s = { params, spheres, ns, tris, nt, mi, nm, params->intersectMode, NULL };
    *sc = s;
    return 0;
}

/* rgba[i] = the radiance query of rays[i]; accel != 0: triangles are found through the oracle's own search tree (the same hits,
 * tests/test_oracle_cpu.py); casts (may be NULL) = the calls of CalculateRayCollision the samples made (the pre-cast of step 3 not
 * counted: a sample's own first cast is) */
int rad_trace(const rt_params* params, const rt_sphere* spheres, int ns, const rt_triangle* tris, int nt, const rt_meshinfo* mi, int nm,
              const rt_ray* rays, int n, int samples, uint32_t seed, uint32_t firstIndex, int accel, float* rgba, uint64_t* casts)
{
    if (!params || n < 0 || (n > 0 && (!rays || !rgba)) || samples < 1 || samples > 65536) return -1;
    scene_t sc;
    { int r = rad_scene(&sc, params, spheres, ns, tris, nt, mi, nm); if (r) return r; }
    oaccel* tree = accel ? accel_build(&sc) : NULL;
    sc.accel = tree;
    const int S = orc_philox_substreams(samples);
    uint64_t total_casts = 0;
#pragma omp parallel for schedule(dynamic, 16) reduction(+ : total_casts)
    for (int i = 0; i < n; i++) {
        orc_counts cnt; memset(&cnt, 0, sizeof cnt);
        const rt_ray* r = &rays[i];
        float* out = rgba + 4 * (size_t)i;
        if (!(r->tMax > 0.0f)) { out[0] = out[1] = out[2] = out[3] = 0.0f; continue; }
        const v3 o = v_load(r->origin), d = v_load(r->direction);
        const int bounded_miss = rad_bounded_miss(&sc, o, d, r->tMax);
        v3 part[16];
        for (int k = 0; k < 16; k++) part[k] = V(0, 0, 0);
        for (int s = 0; s < samples; s++)
            part[s % S] = v_add(part[s % S], rad_one(&sc, o, d, bounded_miss, firstIndex + (uint32_t)i, seed, (uint32_t)s, &cnt));
        for (int step = 1; step < S; step <<= 1)
            for (int k = 0; k < S; k += 2 * step) part[k] = v_add(part[k], part[k + step]);
        const float nf = (float)samples;
        out[0] = part[0].x / nf; out[1] = part[0].y / nf; out[2] = part[0].z / nf; out[3] = 1.0f;
        total_casts += cnt.rays;
    }
    accel_free(tree);
    if (casts) *casts = total_casts;
    return 0;
}

/* rgb[0..2] = sample `sample` alone of one ray with stream index `index` (what rad_trace feeds its tree) */
int rad_sample(const rt_params* params, const rt_sphere* spheres, int ns, const rt_triangle* tris, int nt, const rt_meshinfo* mi, int nm,
               const rt_ray* ray, uint32_t sample, uint32_t seed, uint32_t index, int accel, float* rgb)
{
    if (!params || !ray || !rgb) return -1;
    scene_t sc;
    { int r = rad_scene(&sc, params, spheres, ns, tris, nt, mi, nm); if (r) return r; }
    oaccel* tree = accel ? accel_build(&sc) : NULL;
    sc.accel = tree;
    orc_counts cnt; memset(&cnt, 0, sizeof cnt);
    v3 c = V(0, 0, 0);
    if (ray->tMax > 0.0f) {
        const v3 o = v_load(ray->origin), d = v_load(ray->direction);
        c = rad_one(&sc, o, d, rad_bounded_miss(&sc, o, d, ray->tMax), index, seed, sample, &cnt);
    }
    rgb[0] = c.x; rgb[1] = c.y; rgb[2] = c.z;
    accel_free(tree);
    return 0;
}

/* rays[pixelIndex] = sample 0's camera ray of every pixel of frame `frame` as frag draws it in Philox mode (key (pixelIndex, frame),
 * counter (block 0, sample 0)), tMax = +inf: width * height rays */
int rad_camera_rays(const rt_params* p, int frame, rt_ray* rays)
{
    if (!p || !rays) return -1;
    const float* M = p->camLocalToWorld;
    const uint32_t W = (uint32_t)p->width, H = (uint32_t)p->height;
    const float Wf = (float)W, Hf = (float)H;
    const v3 camRight = V(M[0], M[4], M[8]), camUp = V(M[1], M[5], M[9]), camPos = v_load(p->worldSpaceCameraPos);
    for (uint32_t y = 0; y < H; y++)
        for (uint32_t x = 0; x < W; x++) {
            const uint32_t pixelIndex = y * W + x;
            const float uvx = ((float)x + 0.5f) / Wf, uvy = ((float)y + 0.5f) / Hf;
            const float lx = (uvx - 0.5f) * p->viewParams[0], ly = (uvy - 0.5f) * p->viewParams[1], lz = 1.0f * p->viewParams[2];
            const v3 focusPoint = V(((M[0] * lx + M[1] * ly) + M[2]  * lz) + M[3]  * 1.0f,
                                    ((M[4] * lx + M[5] * ly) + M[6]  * lz) + M[7]  * 1.0f,
                                    ((M[8] * lx + M[9] * ly) + M[10] * lz) + M[11] * 1.0f);
            orng rng; memset(&rng, 0, sizeof rng);
            rng.mode = RT_RNG_PHILOX;
            rng.key[0] = pixelIndex; rng.key[1] = (uint32_t)frame;
            rng.sample = 0u; rng_scope(&rng, 0u);
            float jx, jy;
            random_point_in_circle(&rng, &jx, &jy);
            jx = jx * p->defocusStrength / Wf;  jy = jy * p->defocusStrength / Wf;
            const v3 origin = v_add(v_add(camPos, v_scale(camRight, jx)), v_scale(camUp, jy));
            random_point_in_circle(&rng, &jx, &jy);
            jx = jx * p->divergeStrength / Wf;  jy = jy * p->divergeStrength / Wf;
            const v3 jfp = v_add(v_add(focusPoint, v_scale(camRight, jx)), v_scale(camUp, jy));
            const v3 dir = v_normalize(v_sub(jfp, origin));
            rt_ray* r = &rays[pixelIndex];
            memset(r, 0, sizeof *r);
            r->origin[0] = origin.x; r->origin[1] = origin.y; r->origin[2] = origin.z;
            r->direction[0] = dir.x; r->direction[1] = dir.y; r->direction[2] = dir.z;
            r->tMax = INFINITY;
        }
    return 0;
}
