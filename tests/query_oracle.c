/*
 * query_oracle.c — the four query families (include/rt.h: rt_trace_rays / rt_occluded, rt_trace_radiance, rt_gather, rt_visibility) on
 * the CPU oracle: the checker of tests/test_gpu_ray_query.py, test_gpu_radiance.py, test_gpu_gather.py and test_gpu_visibility.py, itself
 * pinned by their *_cpu.py counterparts.  TEST INFRASTRUCTURE: it includes the oracle unchanged and is compiled by the tests with the
 * oracle's own CFLAGS (oracle/Makefile, tests/checker_build.py).
 *
 * The families share rules on purpose, and each rule is written once, in "shared rules" below: the scene of a call, the Philox stream
 * of an item's sample, the direction a gather draws, the bound a hit has to meet, the radiance of one sample, the SH9 basis and the
 * estimator's fixed tree.  The sections after it are the families' definitions, each headed by its numbered steps.
 */
#include "../oracle/rt_oracle.c"

enum { Q_COSINE = 0, Q_SH9 = 1, Q_DISTANCE = 2 };           /* the gather modes (0, 1) and the visibility modes (0, 1, 2) */

/* ---------------------------------------------------------------- shared rules ---------------------------------------------------------------- */

/* The scene of a call: the caller's rt_params, or (params == NULL) a zeroed one that carries only `intersect` as its intersectMode;
 * accel != 0: triangles are found through the oracle's own search tree instead of its literal loop (the same hits,
 * tests/test_oracle_cpu.py).  -3: a chunk's triangle range leaves the triangle buffer.  A scene that opened is closed once. */
typedef struct { scene_t sc; rt_params own; oaccel* tree; } qscene;

static int scene_open(qscene* q, const rt_params* params, int intersect, const rt_sphere* spheres, int ns, const rt_triangle* tris, int nt,
                      const rt_meshinfo* mi, int nm, int accel)
{
    for (int m = 0; m < nm; m++)
        if ((uint64_t)mi[m].firstTriangleIndex + mi[m].numTriangles > (uint64_t)nt) return -3;
    if (!params) {
        memset(&q->own, 0, sizeof q->own);
        q->own.intersectMode = intersect;
        params = &q->own;
    }
    const scene_t s = { params, spheres, ns, tris, nt, mi, nm, params->intersectMode, NULL };
    q->sc = s;
    q->tree = accel ? accel_build(&q->sc) : NULL;
    q->sc.accel = q->tree;
    return 0;
}

static void scene_close(qscene* q) { accel_free(q->tree); }

/* The Philox stream of sample s of the item with stream index K: key (K, seed), counter (block, s); the user scopes it to a block */
static orng stream_of(uint32_t K, uint32_t seed, uint32_t s)
{
    orng rng; memset(&rng, 0, sizeof rng);
    rng.mode = RT_RNG_PHILOX;
    rng.key[0] = K; rng.key[1] = seed;
    rng.sample = s;
    return rng;
}

/* The direction a gather or visibility sample looks in: R = the oracle's own random_direction() on the sample's stream scoped to block
 * 0xFFFFFFFE (words 0..3 of block 0xFFFFFFFE, words 0, 1 of block 0xFFFFFFFF); mode 1: d = R; modes 0, 2: d = v_normalize(n + R)
 * (trace()'s own diffuse-lobe expression) */
static v3 sample_direction(v3 n, int mode, uint32_t K, uint32_t seed, uint32_t s)
{
    orng rng = stream_of(K, seed, s);
    rng_scope(&rng, 0xFFFFFFFEu);
    const v3 R = random_direction(&rng);
    return mode == Q_SH9 ? R : v_normalize(v_add(n, R));
}

/* The bound rule: what CalculateRayCollision found counts as a hit of a ray with bound t when it lies strictly before t */
static int hit_within(hit_t h, float t) { return h.didHit && h.dst < t; }

/* The radiance of one sample of the ray (o, d) with bound t, in two parts.
 * bounded_miss: does the cast at trace()'s loop index 0 hit something that the bound rejects?  (It is a pre-cast: not counted.)
 * radiance_sample: when it does, that cast is a miss and trace()'s miss branch at loop index 0 is all that runs: incomingLight (0) +
 * environment_light(d) * rayColour (1), one ray counted, nothing drawn; else the oracle's own trace(o, d) on the sample's stream — trace()
 * scopes the draws of the hit at loop index b to blocks 1 + 2b, 2 + 2b itself; block 0 stays unused. */
static int bounded_miss(const scene_t* sc, v3 o, v3 d, float t)
{
    if (sc->p->maxBounceCount < 0) return 0;                    /* trace() casts nothing */
    orc_counts pre; memset(&pre, 0, sizeof pre);
    const hit_t h = calculate_ray_collision(sc, o, d, &pre);
    return h.didHit && !hit_within(h, t);
}

static v3 radiance_sample(const scene_t* sc, v3 o, v3 d, int missed, uint32_t K, uint32_t seed, uint32_t s, orc_counts* cnt)
{
    if (missed) {
        cnt->rays++;
        return v_add(V(0, 0, 0), v_mul(environment_light(sc->p, d), V(1, 1, 1)));
    }
    orng rng = stream_of(K, seed, s);
    return trace(sc, o, d, &rng, cnt);
}

/* The nine SH basis values on d, as include/rt.h writes them (the oracle is compiled with -ffp-contract=off: every product rounds) */
static void sh9_basis(v3 d, float Y[9])
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

/* The Philox mode's fixed tree (frag's) over the N samples of an item, per float channel: sample s is added to sub-stream s % S in
 * increasing s from 0.0f, the sub-sums pairwise, the root / (float)N.  A v3 is three channels. */
enum { TREE_CHANNELS = 27 };
typedef struct { int C, N, S; float part[TREE_CHANNELS][16]; } qtree;

static void tree_open(qtree* t, int C, int N)
{
    t->C = C; t->N = N; t->S = orc_philox_substreams(N);
    for (int c = 0; c < C; c++) for (int k = 0; k < 16; k++) t->part[c][k] = 0.0f;
}

static void tree_add(qtree* t, int s, const float* ch)
{
    for (int c = 0; c < t->C; c++) t->part[c][s % t->S] = t->part[c][s % t->S] + ch[c];
}

static void tree_root(qtree* t, float* root)
{
    for (int c = 0; c < t->C; c++) {
        for (int step = 1; step < t->S; step <<= 1)
            for (int k = 0; k < t->S; k += 2 * step) t->part[c][k] = t->part[c][k] + t->part[c][k + step];
        root[c] = t->part[c][0] / (float)t->N;
    }
}

static int traced(const rt_ray* r) { return r->tMax > 0.0f; }      /* an item with tMax <= 0 or NaN is not traced: its outputs are 0 */

/* ---------------------------------------------------------------- ray queries -----------------------------------------------------------------
 * The CPU oracle's CalculateRayCollision (RayTracing.shader:256-297) for caller-supplied rays, as rt_hit records.
 *
 * The oracle returns dst, hitPoint, normal and a material pointer.  What was hit is recovered from that pointer: a sphere's own material
 * (the sphere's index), or a chunk's (the chunk's index).  The triangle of a chunk hit is the first of that chunk, in the reference's
 * visiting order, whose RayTriangle accepts the ray at exactly that dst — the one the reference's strict '<' kept (overlapping chunk
 * ranges are refused by the library's upload, so the chunk owns it alone).
 */

/* hits[i] = CalculateRayCollision(rays[i]) when its dst < rays[i].tMax (the bound rule), else a miss (dst = +inf, indices -1, the rest 0) */
int rq_trace(const rt_sphere* spheres, int ns, const rt_triangle* tris, int nt, const rt_meshinfo* mi, int nm, int mode,
             const rt_ray* rays, int n, int accel, rt_hit* hits)
{
    qscene q;
    { int r = scene_open(&q, NULL, mode, spheres, ns, tris, nt, mi, nm, accel); if (r) return r; }
#pragma omp parallel for schedule(dynamic, 64)
    for (int i = 0; i < n; i++) {
        orc_counts cnt;
        memset(&cnt, 0, sizeof cnt);
        const rt_ray* r = &rays[i];
        const v3 o = v_load(r->origin), d = v_load(r->direction);
        const hit_t h = calculate_ray_collision(&q.sc, o, d, &cnt);
        rt_hit* out = &hits[i];
        memset(out, 0, sizeof *out);
        out->dst = INFINITY;
        out->primitive = out->chunk = out->mesh = -1;
        if (!hit_within(h, r->tMax)) continue;
        out->dst = h.dst;
        out->hitPoint[0] = h.hitPoint.x; out->hitPoint[1] = h.hitPoint.y; out->hitPoint[2] = h.hitPoint.z;
        out->normal[0] = h.normal.x; out->normal[1] = h.normal.y; out->normal[2] = h.normal.z;
        const char* mat = (const char*)h.material;
        if (ns > 0 && mat >= (const char*)spheres && mat < (const char*)(spheres + ns)) {
            out->kind = RT_HIT_SPHERE;
            out->primitive = (int32_t)((mat - (const char*)spheres) / (ptrdiff_t)sizeof(rt_sphere));
            continue;
        }
        const int m = (int)((mat - (const char*)&mi[0].material) / (ptrdiff_t)sizeof(rt_meshinfo));
        out->kind = RT_HIT_TRIANGLE;
        out->chunk = m;
        for (uint32_t k = 0; k < mi[m].numTriangles; k++) {
            const uint32_t ti = mi[m].firstTriangleIndex + k;
            float dst, u, v, w;
            if (ray_triangle(o, d, &tris[ti], &dst, &u, &v, &w) && dst == h.dst) {
                out->primitive = (int32_t)ti; out->u = u; out->v = v;
                break;
            }
        }
    }
    scene_close(&q);
    return 0;
}

/* count[i] = how many candidates the literal loop could take at the bit-identical dst of rays[i]'s closest hit, the winner included: every
 * sphere RaySphere accepts and every triangle RayTriangle accepts at that dst (in FLAT_CHUNKS mode only those of chunks whose box test
 * passes) — brute force, no tree.  0 for a miss (tMax applied as rq_trace applies it).  2 or more: the tie-break decided the hit. */
int rq_candidates(const rt_sphere* spheres, int ns, const rt_triangle* tris, int nt, const rt_meshinfo* mi, int nm, int mode,
                  const rt_ray* rays, int n, int32_t* count)
{
    qscene q;
    { int r = scene_open(&q, NULL, mode, spheres, ns, tris, nt, mi, nm, 0); if (r) return r; }
#pragma omp parallel for schedule(dynamic, 64)
    for (int i = 0; i < n; i++) {
        orc_counts cnt;
        memset(&cnt, 0, sizeof cnt);
        const rt_ray* r = &rays[i];
        const v3 o = v_load(r->origin), d = v_load(r->direction);
        const hit_t h = calculate_ray_collision(&q.sc, o, d, &cnt);
        count[i] = 0;
        if (!hit_within(h, r->tMax)) continue;
        int32_t c = 0;
        for (int s = 0; s < ns; s++) {
            float dst;
            if (ray_sphere(o, d, v_load(spheres[s].position), spheres[s].radius, &dst) && dst == h.dst) c++;
        }
        for (int m = 0; m < nm; m++) {
            if (mode == RT_INTERSECT_FLAT_CHUNKS && !ray_bounding_box(o, d, mi[m].boundsMin, mi[m].boundsMax)) continue;
            for (uint32_t k = 0; k < mi[m].numTriangles; k++) {
                float dst, u, v, w;
                if (ray_triangle(o, d, &tris[mi[m].firstTriangleIndex + k], &dst, &u, &v, &w) && dst == h.dst) c++;
            }
        }
        count[i] = c;
    }
    scene_close(&q);
    return 0;
}

/* -------------------------------------------------------------- radiance queries --------------------------------------------------------------
 * For ray i of a call (origin o, direction d, tMax t), K = firstIndex + i:
 *   1. t <= 0 or NaN: (0, 0, 0, 0), nothing is cast;
 *   2. sample s is the oracle's own trace(o, d) with rng.mode = RT_RNG_PHILOX, key (K, seed), rng.sample = s — trace() scopes the draws
 *      of the hit at loop index b to blocks 1 + 2b, 2 + 2b itself; block 0 stays unused;
 *   3. the first-cast bound, applied as the ray queries apply it: calculate_ray_collision, then the comparison.  When the hit of the
 *      cast at loop index 0 fails dst < t that cast is a miss, and trace()'s miss branch at loop index 0 is all that runs:
 *      incomingLight (0) + environment_light(d) * rayColour (1).  It draws nothing, so every sample of the ray has that value;
 *   4. the N samples are summed by the Philox mode's fixed tree (frag's), root / N, alpha 1.
 */

/* rgba[i] = the radiance query of rays[i]; casts (may be NULL) = the calls of CalculateRayCollision the samples made (the pre-cast of
 * step 3 not counted: a sample's own first cast is) */
int rad_trace(const rt_params* params, const rt_sphere* spheres, int ns, const rt_triangle* tris, int nt, const rt_meshinfo* mi, int nm,
              const rt_ray* rays, int n, int samples, uint32_t seed, uint32_t firstIndex, int accel, float* rgba, uint64_t* casts)
{
    if (!params || n < 0 || (n > 0 && (!rays || !rgba)) || samples < 1 || samples > 65536) return -1;
    qscene q;
    { int r = scene_open(&q, params, 0, spheres, ns, tris, nt, mi, nm, accel); if (r) return r; }
    uint64_t total_casts = 0;
#pragma omp parallel for schedule(dynamic, 16) reduction(+ : total_casts)
    for (int i = 0; i < n; i++) {
        orc_counts cnt; memset(&cnt, 0, sizeof cnt);
        const rt_ray* r = &rays[i];
        float* out = rgba + 4 * (size_t)i;
        if (!traced(r)) { out[0] = out[1] = out[2] = out[3] = 0.0f; continue; }
        const v3 o = v_load(r->origin), d = v_load(r->direction);
        const int missed = bounded_miss(&q.sc, o, d, r->tMax);        /* (the same for every sample of the ray: asked once) */
        qtree t;
        tree_open(&t, 3, samples);
        for (int s = 0; s < samples; s++) {
            const v3 L = radiance_sample(&q.sc, o, d, missed, firstIndex + (uint32_t)i, seed, (uint32_t)s, &cnt);
            const float ch[3] = { L.x, L.y, L.z };
            tree_add(&t, s, ch);
        }
        tree_root(&t, out);
        out[3] = 1.0f;
        total_casts += cnt.rays;
    }
    scene_close(&q);
    if (casts) *casts = total_casts;
    return 0;
}

/* rgb[0..2] = sample `sample` alone of one ray with stream index `index` (what rad_trace feeds its tree) */
int rad_sample(const rt_params* params, const rt_sphere* spheres, int ns, const rt_triangle* tris, int nt, const rt_meshinfo* mi, int nm,
               const rt_ray* ray, uint32_t sample, uint32_t seed, uint32_t index, int accel, float* rgb)
{
    if (!params || !ray || !rgb) return -1;
    qscene q;
    { int r = scene_open(&q, params, 0, spheres, ns, tris, nt, mi, nm, accel); if (r) return r; }
    orc_counts cnt; memset(&cnt, 0, sizeof cnt);
    v3 c = V(0, 0, 0);
    if (traced(ray)) {
        const v3 o = v_load(ray->origin), d = v_load(ray->direction);
        c = radiance_sample(&q.sc, o, d, bounded_miss(&q.sc, o, d, ray->tMax), index, seed, sample, &cnt);
    }
    rgb[0] = c.x; rgb[1] = c.y; rgb[2] = c.z;
    scene_close(&q);
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
            orng rng = stream_of(pixelIndex, (uint32_t)frame, 0u);
            rng_scope(&rng, 0u);
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

/* --------------------------------------------------------------- gather queries ---------------------------------------------------------------
 * For point i of a call (origin o, normal n, tMax t), K = firstIndex + i:
 *   1. t <= 0 or NaN: every output float 0, nothing is drawn or cast;
 *   2. sample s draws R with the oracle's own random_direction() from rng.mode = RT_RNG_PHILOX, key (K, seed), rng.sample = s,
 *      rng_scope(&rng, 0xFFFFFFFE): words 0..3 of block 0xFFFFFFFE, words 0, 1 of block 0xFFFFFFFF;
 *      mode 0: d = v_normalize(n + R) (trace()'s own diffuse-lobe expression); mode 1: d = R;
 *   3. L_s = the radiance queries' per-sample rule for the ray (o, d, t) (radiance_sample above, called, not restated): the oracle's own
 *      trace(o, d) with the same key and sample — trace() scopes its hits to blocks 1 + 2b, 2 + 2b itself — unless the hit of the cast at
 *      loop index 0 fails dst < t: then trace()'s miss branch at loop index 0 is all that runs, 0 + environment_light(d) * 1;
 *   4. mode 0: the channels are L_s.rgb; mode 1: L_s.c * Y_k(d), 27 channels; the Philox mode's fixed tree over the N samples,
 *      root / N; mode 1: * 12.566371f; alpha 1 (mode 1: for k = 0 only).
 */

/* steps 2 and 3 for one sample; *d = its direction */
static v3 gather_sample(const scene_t* sc, const rt_ray* pt, int mode, uint32_t K, uint32_t seed, uint32_t s, v3* d, orc_counts* cnt)
{
    const v3 o = v_load(pt->origin);
    *d = sample_direction(v_load(pt->direction), mode, K, seed, s);
    return radiance_sample(sc, o, *d, bounded_miss(sc, o, *d, pt->tMax), K, seed, s, cnt);
}

/* out[i] = the gather query of points[i]: 4 floats (mode 0) or 36 (mode 1); casts (may be NULL) = the calls of CalculateRayCollision
 * the samples made (the pre-cast of step 3 not counted) */
int gth_gather(const rt_params* params, const rt_sphere* spheres, int ns, const rt_triangle* tris, int nt, const rt_meshinfo* mi, int nm,
               const rt_ray* points, int n, int samples, uint32_t seed, uint32_t firstIndex, int mode, int accel, float* out, uint64_t* casts)
{
    if (!params || n < 0 || (n > 0 && (!points || !out)) || samples < 1 || samples > 65536 || (mode != Q_COSINE && mode != Q_SH9)) return -1;
    qscene q;
    { int r = scene_open(&q, params, 0, spheres, ns, tris, nt, mi, nm, accel); if (r) return r; }
    const int NC = mode == Q_SH9 ? 9 : 1;
    uint64_t total_casts = 0;
#pragma omp parallel for schedule(dynamic, 16) reduction(+ : total_casts)
    for (int i = 0; i < n; i++) {
        orc_counts cnt; memset(&cnt, 0, sizeof cnt);
        const rt_ray* r = &points[i];
        float* o4 = out + 4 * (size_t)NC * (size_t)i;
        if (!traced(r)) { for (int k = 0; k < 4 * NC; k++) o4[k] = 0.0f; continue; }
        qtree t;
        tree_open(&t, 3 * NC, samples);
        for (int s = 0; s < samples; s++) {
            v3 d;
            const v3 L = gather_sample(&q.sc, r, mode, firstIndex + (uint32_t)i, seed, (uint32_t)s, &d, &cnt);
            float ch[27] = { L.x, L.y, L.z };
            if (mode == Q_SH9) {
                float Y[9];
                sh9_basis(d, Y);
                for (int c = 0; c < 9; c++) { ch[3 * c] = L.x * Y[c]; ch[3 * c + 1] = L.y * Y[c]; ch[3 * c + 2] = L.z * Y[c]; }
            }
            tree_add(&t, s, ch);
        }
        float root[27];
        tree_root(&t, root);
        for (int c = 0; c < NC; c++) {
            float* o = o4 + 4 * c;
            for (int k = 0; k < 3; k++) o[k] = mode == Q_SH9 ? root[3 * c + k] * 12.566371f : root[3 * c + k];
            o[3] = c == 0 ? 1.0f : 0.0f;
        }
        total_casts += cnt.rays;
    }
    scene_close(&q);
    if (casts) *casts = total_casts;
    return 0;
}

/* rgb[0..2] = L of sample `sample` alone of one point with stream index `index` (what gth_gather feeds its tree, before the basis) */
int gth_sample(const rt_params* params, const rt_sphere* spheres, int ns, const rt_triangle* tris, int nt, const rt_meshinfo* mi, int nm,
               const rt_ray* point, uint32_t sample, uint32_t seed, uint32_t index, int mode, int accel, float* rgb)
{
    if (!params || !point || !rgb) return -1;
    qscene q;
    { int r = scene_open(&q, params, 0, spheres, ns, tris, nt, mi, nm, accel); if (r) return r; }
    orc_counts cnt; memset(&cnt, 0, sizeof cnt);
    v3 c = V(0, 0, 0), d;
    if (traced(point)) c = gather_sample(&q.sc, point, mode, index, seed, sample, &d, &cnt);
    rgb[0] = c.x; rgb[1] = c.y; rgb[2] = c.z;
    scene_close(&q);
    return 0;
}

/* d[0..2] = the direction of sample `sample` of a gather or visibility point with normal `normal` and stream index `index` */
int query_direction(const float* normal, uint32_t sample, uint32_t seed, uint32_t index, int mode, float* d)
{
    if (!normal || !d) return -1;
    const v3 v = sample_direction(v_load(normal), mode, index, seed, sample);
    d[0] = v.x; d[1] = v.y; d[2] = v.z;
    return 0;
}

/* ------------------------------------------------------------- visibility gathers -------------------------------------------------------------
 * For point i of a call (origin o, normal n, reach t), K = firstIndex + i:
 *   1. t <= 0 or NaN: every output float 0, nothing is drawn or cast;
 *   2. sample s draws R with the oracle's own random_direction() from rng.mode = RT_RNG_PHILOX, key (K, seed), rng.sample = s,
 *      rng_scope(&rng, 0xFFFFFFFE): words 0..3 of block 0xFFFFFFFE, words 0, 1 of block 0xFFFFFFFF (the gather queries' draw);
 *      modes 0, 2: d = v_normalize(n + R); mode 1: d = R;
 *   3. h = the oracle's calculate_ray_collision(o, d); it is a hit when h.didHit and h.dst < t — the bound rule of rt_trace_rays and
 *      rt_occluded.  Modes 0, 1: v = hit ? 0 : 1.  Mode 2: r = hit ? h.dst : t, hit = 1 / 0;
 *   4. channels: mode 0 (v ? d : 0, v); mode 1 (v ? Y_k(d) : 0, k = 0..8, then v); mode 2 (r, r * r, hit); the Philox mode's fixed
 *      tree over the N samples per channel, root / N; mode 1: coefficients 0..8 * 12.566371f after the division, floats 10, 11 = 0;
 *      mode 2: the fourth float is 1.
 */

static int vis_valid_mode(int mode) { return mode >= Q_COSINE && mode <= Q_DISTANCE; }
static int vis_channel_count(int mode) { return mode == Q_SH9 ? 10 : mode == Q_DISTANCE ? 3 : 4; }

/* the channels of one sample (steps 2 to 4, before the tree) */
static void vis_channels(const scene_t* sc, const rt_ray* pt, int mode, uint32_t K, uint32_t seed, uint32_t s, float ch[10])
{
    const v3 d = sample_direction(v_load(pt->direction), mode, K, seed, s);
    orc_counts cnt; memset(&cnt, 0, sizeof cnt);
    const hit_t h = calculate_ray_collision(sc, v_load(pt->origin), d, &cnt);
    const int hit = hit_within(h, pt->tMax);
    if (mode == Q_DISTANCE) {
        const float r = hit ? h.dst : pt->tMax;
        ch[0] = r; ch[1] = r * r; ch[2] = hit ? 1.0f : 0.0f;
        return;
    }
    const int v = !hit;
    if (mode == Q_SH9) {
        float Y[9];
        sh9_basis(d, Y);
        for (int k = 0; k < 9; k++) ch[k] = v ? Y[k] : 0.0f;
        ch[9] = v ? 1.0f : 0.0f;
        return;
    }
    ch[0] = v ? d.x : 0.0f; ch[1] = v ? d.y : 0.0f; ch[2] = v ? d.z : 0.0f; ch[3] = v ? 1.0f : 0.0f;
}

/* out[i] = the visibility gather of points[i]: 4 floats (modes 0, 2) or 12 (mode 1); intersect = the intersectMode that applies */
int vis_gather(const rt_sphere* spheres, int ns, const rt_triangle* tris, int nt, const rt_meshinfo* mi, int nm, int intersect,
               const rt_ray* points, int n, int samples, uint32_t seed, uint32_t firstIndex, int mode, int accel, float* out)
{
    if (n < 0 || (n > 0 && (!points || !out)) || samples < 1 || samples > 65536 || !vis_valid_mode(mode)) return -1;
    qscene q;
    { int r = scene_open(&q, NULL, intersect, spheres, ns, tris, nt, mi, nm, accel); if (r) return r; }
    const int NF = mode == Q_SH9 ? 12 : 4, NC = vis_channel_count(mode);
#pragma omp parallel for schedule(dynamic, 16)
    for (int i = 0; i < n; i++) {
        const rt_ray* r = &points[i];
        float* o = out + (size_t)NF * (size_t)i;
        for (int k = 0; k < NF; k++) o[k] = 0.0f;
        if (!traced(r)) continue;
        qtree t;
        tree_open(&t, NC, samples);
        for (int s = 0; s < samples; s++) {
            float ch[10];
            vis_channels(&q.sc, r, mode, firstIndex + (uint32_t)i, seed, (uint32_t)s, ch);
            tree_add(&t, s, ch);
        }
        tree_root(&t, o);
        if (mode == Q_SH9) for (int c = 0; c < 9; c++) o[c] = o[c] * 12.566371f;
        if (mode == Q_DISTANCE) o[3] = 1.0f;
    }
    scene_close(&q);
    return 0;
}

/* ch[0..] = the channels of sample `sample` alone of one point with stream index `index` (what vis_gather feeds its tree): 4, 10 or 3
 * floats; returns their number, or a negative error.  A point that is not traced has no samples: -2 */
int vis_sample(const rt_sphere* spheres, int ns, const rt_triangle* tris, int nt, const rt_meshinfo* mi, int nm, int intersect,
               const rt_ray* point, uint32_t sample, uint32_t seed, uint32_t index, int mode, int accel, float* ch)
{
    if (!point || !ch || !vis_valid_mode(mode)) return -1;
    if (!traced(point)) return -2;
    qscene q;
    { int r = scene_open(&q, NULL, intersect, spheres, ns, tris, nt, mi, nm, accel); if (r) return r; }
    vis_channels(&q.sc, point, mode, index, seed, sample, ch);
    scene_close(&q);
    return vis_channel_count(mode);
}
