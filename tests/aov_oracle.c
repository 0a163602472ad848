/*
 * aov_oracle.c — the first-hit feature buffers (include/rt.h rt_render_aov) restated serially per pixel on the CPU oracle: the checker of
 * tests/test_gpu_aov.py, itself pinned by tests/test_aov_cpu.py.  TEST INFRASTRUCTURE: it includes the oracle unchanged and is compiled
 * by the tests with the oracle's own CFLAGS (oracle/Makefile).
 *
 * For pixel (x, y) of feature frame f, N = numRaysPerPixel:
 *   1. sample s draws its camera ray as frag does (rt_oracle.c frag), always from the Philox stream key (pixelIndex, f), counter
 *      (block 0, sample s);
 *   2. its surface is the hit at which trace() first scatters: the first hit, an InvisibleLight (flag 2) passed through once as trace()
 *      does at bounce 0 (only if maxBounceCount >= 1; with no bounce left there is no surface);
 *   3. a hit gives albedo (colour, checker rule), normal, depth = sqrtf(v_dot(q, q)), q = hitPoint - the camera ray's origin, coverage 1;
 *      a miss gives 0 in all eight channels;
 *   4. the eight channels are summed by the Philox mode's fixed tree (sample s to sub-stream s mod S, pairwise), root / N;
 *   5. frames accumulate as acc = acc * (1 - w) + cur * w, w = 1 / (k + 1), no saturate.
 */
#include "../oracle/rt_oracle.c"

static void aov_pixel(const scene_t* sc, int x, int y, int frame, float* out_a, float* out_n, orc_counts* cnt)
{
    const rt_params* p = sc->p;
    const float* M = p->camLocalToWorld;
    uint32_t W = (uint32_t)p->width, H = (uint32_t)p->height;
    float Wf = (float)W, Hf = (float)H;
    float uvx = ((float)x + 0.5f) / Wf, uvy = ((float)y + 0.5f) / Hf;
    uint32_t pixelIndex = (uint32_t)y * W + (uint32_t)x;
    orng rng; memset(&rng, 0, sizeof rng);
    rng.mode = RT_RNG_PHILOX;                                       /* whatever p->rngMode is */
    rng.key[0] = pixelIndex; rng.key[1] = (uint32_t)frame;

    float lx = (uvx - 0.5f) * p->viewParams[0];
    float ly = (uvy - 0.5f) * p->viewParams[1];
    float lz = 1.0f * p->viewParams[2];
    v3 focusPoint = V(((M[0] * lx + M[1] * ly) + M[2]  * lz) + M[3]  * 1.0f,
                      ((M[4] * lx + M[5] * ly) + M[6]  * lz) + M[7]  * 1.0f,
                      ((M[8] * lx + M[9] * ly) + M[10] * lz) + M[11] * 1.0f);
    v3 camRight = V(M[0], M[4], M[8]);
    v3 camUp    = V(M[1], M[5], M[9]);
    v3 camPos   = v_load(p->worldSpaceCameraPos);

    float part[16][8];
    const int S = orc_philox_substreams(p->numRaysPerPixel);
    for (int k = 0; k < 16; k++) for (int c = 0; c < 8; c++) part[k][c] = 0.0f;
    for (int s = 0; s < p->numRaysPerPixel; s++) {
        float jx, jy;
        rng.sample = (uint32_t)s; rng_scope(&rng, 0u);
        random_point_in_circle(&rng, &jx, &jy);
        jx = jx * p->defocusStrength / Wf;  jy = jy * p->defocusStrength / Wf;
        v3 origin = v_add(v_add(camPos, v_scale(camRight, jx)), v_scale(camUp, jy));
        random_point_in_circle(&rng, &jx, &jy);
        jx = jx * p->divergeStrength / Wf;  jy = jy * p->divergeStrength / Wf;
        v3 jfp = v_add(v_add(focusPoint, v_scale(camRight, jx)), v_scale(camUp, jy));
        v3 d = v_normalize(v_sub(jfp, origin));

        float v[8] = { 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f };
        v3 o = origin;
        for (int bounce = 0; bounce <= p->maxBounceCount && bounce < 2; bounce++) {
            hit_t h = calculate_ray_collision(sc, o, d, cnt);
            if (!h.didHit) break;
            const rt_material* m = h.material;
            v3 colour = v_load(m->colour);
            if (m->flag == 1) {
                float cx = mod2(floorf(h.hitPoint.x)), cz = mod2(floorf(h.hitPoint.z));
                if (!(cx == cz)) colour = v_load(m->emissionColour);
            } else if (m->flag == 2 && bounce == 0) {
                o = v_add(h.hitPoint, v_scale(d, 0.001f));
                continue;
            }
            v3 q = v_sub(h.hitPoint, origin);
            v[0] = colour.x; v[1] = colour.y; v[2] = colour.z; v[3] = 1.0f;
            v[4] = h.normal.x; v[5] = h.normal.y; v[6] = h.normal.z; v[7] = sqrtf(v_dot(q, q));
            break;
        }
        for (int c = 0; c < 8; c++) part[s % S][c] = part[s % S][c] + v[c];
    }
    for (int step = 1; step < S; step <<= 1)
        for (int k = 0; k < S; k += 2 * step)
            for (int c = 0; c < 8; c++) part[k][c] = part[k][c] + part[k + step][c];
    float n = (float)p->numRaysPerPixel;
    for (int c = 0; c < 4; c++) { out_a[c] = part[0][c] / n; out_n[c] = part[0][4 + c] / n; }
}

/* One feature frame of the pixel rectangle [x0, x1) x [y0, y1) of the full image: albedo and normal_depth, (y1 - y0) * (x1 - x0) * 4
 * floats each.  accel != 0: triangles are found through the oracle's own search tree (the same hits, tests/test_oracle_cpu.py). */
int aov_frame(const rt_params* params, const rt_sphere* spheres, int ns, const rt_triangle* tris, int nt,
              const rt_meshinfo* meshinfo, int nm, int frame, int x0, int y0, int x1, int y1, int accel,
              float* albedo, float* normal_depth)
{
    if (!params || !albedo || !normal_depth) return -1;
    if (x0 < 0 || y0 < 0 || x1 > params->width || y1 > params->height || x0 > x1 || y0 > y1) return -2;
    for (int m = 0; m < nm; m++)
        if ((uint64_t)meshinfo[m].firstTriangleIndex + meshinfo[m].numTriangles > (uint64_t)nt) return -3;
    scene_t sc = { params, spheres, ns, tris, nt, meshinfo, nm, params->intersectMode, NULL };
    oaccel* tree = accel ? accel_build(&sc) : NULL;
    sc.accel = tree;
    int cw = x1 - x0;
#pragma omp parallel for schedule(dynamic, 1)
    for (int y = y0; y < y1; y++) {
        orc_counts cnt; memset(&cnt, 0, sizeof cnt);
        for (int x = x0; x < x1; x++) {
            size_t i = ((size_t)(y - y0) * cw + (x - x0)) * 4;
            aov_pixel(&sc, x, y, frame, albedo + i, normal_depth + i, &cnt);
        }
    }
    accel_free(tree);
    return 0;
}

/* step 5: feature frame number k (0-based count of frames already in acc) */
void aov_accumulate(float* acc, const float* cur, size_t n_floats, int k)
{
    float w = 1.0f / (float)(k + 1);
    float omw = 1.0f - w;
    for (size_t i = 0; i < n_floats; i++) acc[i] = acc[i] * omw + cur[i] * w;
}
