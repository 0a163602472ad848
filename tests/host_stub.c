/* host_stub.c — a recording stand-in for every C-ABI entry the compiled host (host_cpp/) links, for both handle kinds.  No GPU: every
   call prints one line (entry, handle, scalar arguments, count and FNV-1a hash of every input buffer, return code) and fills its output
   deterministically, so that a program linked with it (host_transcript.cpp) shows what the host sends and how it trims what comes back.
   stub_fail(entry, nth) makes the nth call of that entry from now return -2 and the matching last-error getter say "stub: <entry>". */
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../include/rt.h"

struct handle { int number; const char* kind; int closest_k; };
struct rt_ctx { struct handle h; };
struct rt_multi { struct handle h; };

static int g_created[2];                        /* handles are numbered by creation order, per kind */
static char g_error[2][96];                     /* what rt_last_error / rt_multi_last_error return */
static char g_fail_entry[64];
static int g_fail_countdown;

static char g_line[1024];
static size_t g_len;

static void put(const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    if (g_len < sizeof g_line) g_len += (size_t)vsnprintf(g_line + g_len, sizeof g_line - g_len, fmt, ap);
    va_end(ap);
}

static void put_handle(const struct handle* h)
{
    if (h) put(" %s#%d", h->kind, h->number); else put(" null");
}

static void open_line(const char* entry, const struct handle* h)
{
    g_len = 0;
    put("%s", entry);
    put_handle(h);
}

/* an input buffer: count:hash of its bytes, "null" for a null pointer with a count, "0:-" for an empty one */
static void put_buffer(const char* name, const void* p, size_t count, size_t size)
{
    if (count == 0) { put(" %s=0:-", name); return; }
    if (!p) { put(" %s=null", name); return; }
    uint32_t hash = 2166136261u;
    const unsigned char* b = (const unsigned char*)p;
    for (size_t i = 0; i < count * size; ++i) { hash ^= b[i]; hash *= 16777619u; }
    put(" %s=%zu:%08x", name, count, hash);
}

static void put_params(const void* p, size_t size)
{
    if (p) put_buffer("params", p, 1, size); else put(" params=null");
}

static int is_multi(const char* entry) { return strncmp(entry, "rt_multi_", 9) == 0; }

/* the return code of this call: -2 when the stub refuses it or stub_fail armed it, else 0; ends the line */
static int close_refusing(const char* entry, int refused)
{
    int rc = refused ? -2 : 0;
    if (g_fail_countdown > 0 && strcmp(entry, g_fail_entry) == 0 && --g_fail_countdown == 0) rc = -2;
    if (rc != 0) snprintf(g_error[is_multi(entry)], sizeof g_error[0], "stub: %s", entry);
    printf("%s -> %d\n", g_line, rc);
    return rc;
}
static int close_line(const char* entry) { return close_refusing(entry, 0); }

void stub_fail(const char* entry, int nth)
{
    snprintf(g_fail_entry, sizeof g_fail_entry, "%s", entry);
    g_fail_countdown = nth;
}

static void fill_floats(float* out, size_t n, float step)
{
    for (size_t i = 0; out && i < n; ++i) out[i] = (float)i * step;
}

/* ---- the handles ---------------------------------------------------------------------------------------------------------------- */

static struct handle* create(const char* entry, int multi, size_t size, int refused)
{
    if (close_refusing(entry, refused) != 0) return NULL;
    struct handle* h = (struct handle*)calloc(1, size);
    h->number = ++g_created[multi]; h->kind = multi ? "multi" : "ctx"; h->closest_k = 1;
    return h;
}

rt_ctx* rt_create(int device)
{
    open_line("rt_create", NULL);
    put(" device=%d", device);
    return (rt_ctx*)create("rt_create", 0, sizeof(rt_ctx), 0);
}

rt_multi* rt_multi_create(const int* devices, int n_devices)
{
    open_line("rt_multi_create", NULL);
    put_buffer("devices", devices, n_devices > 0 ? (size_t)n_devices : 0, sizeof(int));
    put(" n_devices=%d", n_devices);
    return (rt_multi*)create("rt_multi_create", 1, sizeof(rt_multi), !devices || n_devices <= 0);
}

void rt_destroy(rt_ctx* c) { open_line("rt_destroy", c ? &c->h : NULL); printf("%s\n", g_line); free(c); }
void rt_multi_destroy(rt_multi* m) { open_line("rt_multi_destroy", m ? &m->h : NULL); printf("%s\n", g_line); free(m); }

static const char* last_error(const char* entry, const struct handle* h)
{
    open_line(entry, h);
    printf("%s -> \"%s\"\n", g_line, g_error[is_multi(entry)]);
    return g_error[is_multi(entry)];
}
const char* rt_last_error(const rt_ctx* c) { return last_error("rt_last_error", c ? &c->h : NULL); }
const char* rt_multi_last_error(const rt_multi* m) { return last_error("rt_multi_last_error", m ? &m->h : NULL); }

/* ---- the entries, one body per pair --------------------------------------------------------------------------------------------- */

static int set_params(const char* e, struct handle* h, const rt_params* p)
{
    open_line(e, h); put_params(p, sizeof *p);
    return close_line(e);
}
int rt_set_params(rt_ctx* c, const rt_params* p) { return set_params("rt_set_params", &c->h, p); }
int rt_multi_set_params(rt_multi* m, const rt_params* p) { return set_params("rt_multi_set_params", &m->h, p); }

static int upload(const char* e, struct handle* h, const char* what, const void* p, int n, size_t size)
{
    open_line(e, h); put_buffer(what, p, n > 0 ? (size_t)n : 0, size); put(" n=%d", n);
    return close_line(e);
}
int rt_upload_spheres(rt_ctx* c, const rt_sphere* s, int n) { return upload("rt_upload_spheres", &c->h, "spheres", s, n, sizeof *s); }
int rt_multi_upload_spheres(rt_multi* m, const rt_sphere* s, int n) { return upload("rt_multi_upload_spheres", &m->h, "spheres", s, n, sizeof *s); }
int rt_upload_triangles(rt_ctx* c, const rt_triangle* t, int n) { return upload("rt_upload_triangles", &c->h, "tris", t, n, sizeof *t); }
int rt_multi_upload_triangles(rt_multi* m, const rt_triangle* t, int n) { return upload("rt_multi_upload_triangles", &m->h, "tris", t, n, sizeof *t); }
int rt_upload_meshinfo(rt_ctx* c, const rt_meshinfo* i, int n) { return upload("rt_upload_meshinfo", &c->h, "meshinfo", i, n, sizeof *i); }
int rt_multi_upload_meshinfo(rt_multi* m, const rt_meshinfo* i, int n) { return upload("rt_multi_upload_meshinfo", &m->h, "meshinfo", i, n, sizeof *i); }
int rt_set_mesh_transforms(rt_ctx* c, const rt_mesh_transform* x, int n) { return upload("rt_set_mesh_transforms", &c->h, "transforms", x, n, sizeof *x); }
int rt_multi_set_mesh_transforms(rt_multi* m, const rt_mesh_transform* x, int n) { return upload("rt_multi_set_mesh_transforms", &m->h, "transforms", x, n, sizeof *x); }

static int upload_local(const char* e, struct handle* h, const rt_triangle* t, int nt, const rt_local_chunk* ch, int nc, int nm)
{
    open_line(e, h);
    put_buffer("local_tris", t, nt > 0 ? (size_t)nt : 0, sizeof *t); put(" n_tris=%d", nt);
    put_buffer("chunks", ch, nc > 0 ? (size_t)nc : 0, sizeof *ch); put(" n_chunks=%d n_meshes=%d", nc, nm);
    return close_line(e);
}
int rt_upload_local_meshes(rt_ctx* c, const rt_triangle* t, int nt, const rt_local_chunk* ch, int nc, int nm)
{
    return upload_local("rt_upload_local_meshes", &c->h, t, nt, ch, nc, nm);
}
int rt_multi_upload_local_meshes(rt_multi* m, const rt_triangle* t, int nt, const rt_local_chunk* ch, int nc, int nm)
{
    return upload_local("rt_multi_upload_local_meshes", &m->h, t, nt, ch, nc, nm);
}

static int set_option(const char* e, struct handle* h, const char* name, int value)
{
    open_line(e, h); put(" name=%s value=%d", name, value);
    const int rc = close_line(e);
    if (rc == 0 && strcmp(name, "closest_k") == 0) h->closest_k = value;
    return rc;
}
int rt_set_option(rt_ctx* c, const char* name, int value) { return set_option("rt_set_option", &c->h, name, value); }
int rt_multi_set_option(rt_multi* m, const char* name, int value) { return set_option("rt_multi_set_option", &m->h, name, value); }

static int reset_accum(const char* e, struct handle* h) { open_line(e, h); return close_line(e); }
int rt_reset_accum(rt_ctx* c) { return reset_accum("rt_reset_accum", &c->h); }
int rt_multi_reset_accum(rt_multi* m) { return reset_accum("rt_multi_reset_accum", &m->h); }

static int render(const char* e, struct handle* h, int first_frame, int n_frames)
{
    open_line(e, h); put(" first_frame=%d n_frames=%d", first_frame, n_frames);
    return close_line(e);
}
int rt_render(rt_ctx* c, int f, int n) { return render("rt_render", &c->h, f, n); }
int rt_multi_render(rt_multi* m, int f, int n) { return render("rt_multi_render", &m->h, f, n); }
int rt_render_aov(rt_ctx* c, int f, int n) { return render("rt_render_aov", &c->h, f, n); }

int rt_get_aov_info(rt_ctx* c, rt_aov_info* out)
{
    open_line("rt_get_aov_info", &c->h);
    const int rc = close_line("rt_get_aov_info");
    if (rc == 0) { memset(out, 0, sizeof *out); out->framesAccumulated = 7; out->lastSampleLanes = 16; }
    return rc;
}

/* the image and plane reads: out[i] = i * 0.5f */
static int read_plane(const char* e, struct handle* h, float* out, size_t n_floats)
{
    open_line(e, h); put(" n_floats=%zu", n_floats);
    const int rc = close_line(e);
    if (rc == 0) fill_floats(out, n_floats, 0.5f);
    return rc;
}
int rt_read_accum(rt_ctx* c, float* o, size_t n) { return read_plane("rt_read_accum", &c->h, o, n); }
int rt_multi_read_accum(rt_multi* m, float* o, size_t n) { return read_plane("rt_multi_read_accum", &m->h, o, n); }
int rt_read_denoised(rt_ctx* c, float* o, size_t n) { return read_plane("rt_read_denoised", &c->h, o, n); }
int rt_multi_read_denoised(rt_multi* m, float* o, size_t n) { return read_plane("rt_multi_read_denoised", &m->h, o, n); }
int rt_read_variance(rt_ctx* c, float* o, size_t n) { return read_plane("rt_read_variance", &c->h, o, n); }
int rt_multi_read_variance(rt_multi* m, float* o, size_t n) { return read_plane("rt_multi_read_variance", &m->h, o, n); }
int rt_read_temporal(rt_ctx* c, float* o, size_t n) { return read_plane("rt_read_temporal", &c->h, o, n); }
int rt_multi_read_temporal(rt_multi* m, float* o, size_t n) { return read_plane("rt_multi_read_temporal", &m->h, o, n); }
int rt_read_aov(rt_ctx* c, int which, float* o, size_t n)
{
    open_line("rt_read_aov", &c->h); put(" which=%d n_floats=%zu", which, n);
    const int rc = close_line("rt_read_aov");
    if (rc == 0) fill_floats(o, n, 0.5f);
    return rc;
}

static int filter(const char* e, struct handle* h, const void* params, size_t size)
{
    open_line(e, h); put_params(params, size);
    return close_line(e);
}
int rt_denoise(rt_ctx* c, const rt_denoise_params* p) { return filter("rt_denoise", &c->h, p, sizeof *p); }
int rt_multi_denoise(rt_multi* m, const rt_denoise_params* p) { return filter("rt_multi_denoise", &m->h, p, sizeof *p); }
int rt_denoise_variance(rt_ctx* c, const rt_vdenoise_params* p) { return filter("rt_denoise_variance", &c->h, p, sizeof *p); }
int rt_multi_denoise_variance(rt_multi* m, const rt_vdenoise_params* p) { return filter("rt_multi_denoise_variance", &m->h, p, sizeof *p); }
int rt_temporal(rt_ctx* c, const rt_temporal_params* p) { return filter("rt_temporal", &c->h, p, sizeof *p); }
int rt_multi_temporal(rt_multi* m, const rt_temporal_params* p) { return filter("rt_multi_temporal", &m->h, p, sizeof *p); }

/* the float queries: floats_per_item results per ray or point, out[i] = i * 0.25f */
static int query(const char* e, struct handle* h, const rt_ray* items, int n, const void* params, size_t size, float* out, size_t floats_per_item)
{
    open_line(e, h); put_buffer("items", items, n > 0 ? (size_t)n : 0, sizeof *items); put(" n=%d", n); put_params(params, size);
    const int rc = close_line(e);
    if (rc == 0 && n > 0) fill_floats(out, (size_t)n * floats_per_item, 0.25f);
    return rc;
}
int rt_trace_radiance(rt_ctx* c, const rt_ray* r, int n, const rt_radiance_params* p, float* o)
{
    return query("rt_trace_radiance", &c->h, r, n, p, sizeof *p, o, 4);
}
int rt_multi_trace_radiance(rt_multi* m, const rt_ray* r, int n, const rt_radiance_params* p, float* o)
{
    return query("rt_multi_trace_radiance", &m->h, r, n, p, sizeof *p, o, 4);
}
static size_t gather_floats(const rt_gather_params* p) { return p && p->mode == RT_GATHER_SH9 ? 36 : 4; }
int rt_gather(rt_ctx* c, const rt_ray* r, int n, const rt_gather_params* p, float* o)
{
    return query("rt_gather", &c->h, r, n, p, sizeof *p, o, gather_floats(p));
}
int rt_multi_gather(rt_multi* m, const rt_ray* r, int n, const rt_gather_params* p, float* o)
{
    return query("rt_multi_gather", &m->h, r, n, p, sizeof *p, o, gather_floats(p));
}
static size_t visibility_floats(const rt_visibility_params* p) { return p && p->mode == RT_VIS_SH9 ? 12 : 4; }
int rt_visibility(rt_ctx* c, const rt_ray* r, int n, const rt_visibility_params* p, float* o)
{
    return query("rt_visibility", &c->h, r, n, p, sizeof *p, o, visibility_floats(p));
}
int rt_multi_visibility(rt_multi* m, const rt_ray* r, int n, const rt_visibility_params* p, float* o)
{
    return query("rt_multi_visibility", &m->h, r, n, p, sizeof *p, o, visibility_floats(p));
}

/* per point, K = the remembered "closest_k" records: min(K, 3) non-empty ones, then empty ones, _reserved[0] = 5 in all K */
static int closest_points(const char* e, struct handle* h, const rt_ray* points, int n, rt_closest* out)
{
    open_line(e, h); put_buffer("points", points, n > 0 ? (size_t)n : 0, sizeof *points); put(" n=%d closest_k=%d", n, h->closest_k);
    const int rc = close_line(e);
    for (int i = 0; rc == 0 && i < n; ++i)
        for (int k = 0; k < h->closest_k; ++k) {
            rt_closest* r = &out[(size_t)i * (size_t)h->closest_k + (size_t)k];
            memset(r, 0, sizeof *r);
            r->kind = k < 3 ? RT_HIT_TRIANGLE : RT_HIT_NONE;
            r->dst = (float)(i * 8 + k) * 0.125f; r->primitive = k < 3 ? i * 8 + k : -1; r->chunk = r->mesh = k < 3 ? 0 : -1;
            r->side = k < 3 ? 1 : 0;
            r->_reserved[0] = 5;
        }
    return rc;
}
int rt_closest_points(rt_ctx* c, const rt_ray* p, int n, rt_closest* o) { return closest_points("rt_closest_points", &c->h, p, n, o); }
int rt_multi_closest_points(rt_multi* m, const rt_ray* p, int n, rt_closest* o) { return closest_points("rt_multi_closest_points", &m->h, p, n, o); }

/* per ray, maxHits records: two non-empty ones, then empty ones (maxHits outside 1..RT_HITS_MAX is refused as the library refuses it) */
static int trace_hits(const char* e, struct handle* h, const rt_ray* rays, int n, const rt_hits_params* p, rt_multihit* out)
{
    const int K = p ? p->maxHits : RT_HITS_DEFAULT_MAX;
    open_line(e, h); put_buffer("rays", rays, n > 0 ? (size_t)n : 0, sizeof *rays); put(" n=%d", n); put_params(p, sizeof *p);
    const int rc = close_refusing(e, K < 1 || K > RT_HITS_MAX);
    for (int i = 0; rc == 0 && i < n; ++i)
        for (int k = 0; k < K; ++k) {
            rt_multihit* r = &out[(size_t)i * (size_t)K + (size_t)k];
            memset(r, 0, sizeof *r);
            r->kind = k < 2 ? RT_HIT_SPHERE : RT_HIT_NONE;
            r->dst = (float)(i * 8 + k) * 0.125f; r->primitive = k < 2 ? i * 8 + k : -1; r->chunk = r->mesh = -1;
            r->side = k < 2 ? 1 : 0;
            r->hitCount = K < 2 ? K : 2;
        }
    return rc;
}
int rt_trace_hits(rt_ctx* c, const rt_ray* r, int n, const rt_hits_params* p, rt_multihit* o) { return trace_hits("rt_trace_hits", &c->h, r, n, p, o); }
int rt_multi_trace_hits(rt_multi* m, const rt_ray* r, int n, const rt_hits_params* p, rt_multihit* o)
{
    return trace_hits("rt_multi_trace_hits", &m->h, r, n, p, o);
}
