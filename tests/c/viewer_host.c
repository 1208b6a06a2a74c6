/* viewer_host.c -- TEST: a plain C11 host of include/sdfviewer.h (no C++), checked against the oracle's loop (liboracle.so,
 * or_viewer_update_fn / or_viewer_update) stepped by max_iterations to the visited counts the viewer reports.
 *   (a) a host-callback gyroid (tests/c/gyroid_provider.c's function as callbacks) loads progressively under a 30 ms budget,
 *       on 1 and on 8 threads: every intermediate tex0 / tex1 equals the oracle's;
 *   (b) the demo given as device_params equals sdfv_fill_grid;
 *   (c) the demo given as sample_batch_device (calling sdfv_sample_points) goes through every intermediate state of the
 *       oracle's loop: 64^3 over 3 passes in both volume layouts, and a grid with an odd height;
 *   (d) a changed() box after the load gives the oracle's 3-pass reload, through the host and the device route;
 *   (e) a callback that fails mid-load returns SDFV_ERR_CALLBACK, leaves the textures as they were, and a later update
 *       finishes the load to the same bits.
 * Prints "viewer_host ok" or the first failed check. */
#include <hip/hip_runtime_api.h>

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "sdf_oracle.h"
#include "sdfviewer.h"

#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) {                                                           \
            printf("FAILED line %d: %s\n", __LINE__, #cond);                     \
            exit(1);                                                             \
        }                                                                        \
    } while (0)
#define OK(call)                                                                 \
    do {                                                                         \
        int rc_ = (call);                                                        \
        if (rc_ != 0) {                                                          \
            printf("FAILED line %d: %s = %d\n", __LINE__, #call, rc_);          \
            exit(1);                                                             \
        }                                                                        \
    } while (0)

/* ---- the gyroid of tests/c/gyroid_provider.c ---- */
static float g_thickness = 0.15f;
static const float k_bounds[6] = {-1.0f, -0.5f, -0.75f, 1.0f, 0.5f, 0.75f};

static void gyroid(const float p[3], int distance_only, float out[7]) {
    const float k = 6.0f;
    const float x = p[0] * k, y = p[1] * k, z = p[2] * k;
    float g = sinf(x) * cosf(y) + sinf(y) * cosf(z) + sinf(z) * cosf(x);
    float d = fabsf(g) / k - g_thickness * 0.5f;
    d = d * 2.5f;
    if (p[0] == k_bounds[0] && p[1] == k_bounds[1] && p[2] == k_bounds[2]) d = NAN;
    memset(out, 0, 7 * sizeof(float));
    out[0] = d;
    if (distance_only) return;
    const float band = floorf((p[0] + 1.0f) * 4.0f);
    if (fmodf(band, 3.0f) != 0.0f) {
        out[1] = 0.5f + 0.6f * sinf(y);
        out[2] = fabsf(cosf(z));
        out[3] = (p[2] > 0.0f) ? 1.0f : 0.25f;
    }
    out[4] = 0.5f + 0.5f * cosf(x);
    out[5] = p[1] > 0.0f ? 0.3f : 0.0f;
    out[6] = p[0] > 0.25f ? 0.0f : (p[0] < -0.25f ? -1.0f : 0.6f);
}

typedef struct {
    int changed;     /* report edit_box once */
    float edit_box[6];
    int threads;
} Gyroid;

static void gy_bb(void *user, float out[6]) {
    (void)user;
    memcpy(out, k_bounds, sizeof k_bounds);
}
static int gy_sample(void *user, const float p[3], int distance_only, sdfv_sample *out) {
    (void)user;
    gyroid(p, distance_only, (float *)out);
    return 0;
}
static uint32_t gy_concurrency(void *user) { return (uint32_t)((Gyroid *)user)->threads; }
static int gy_changed(void *user, float out[6]) {
    Gyroid *g = (Gyroid *)user;
    if (!g->changed) return 0;
    g->changed = 0;
    memcpy(out, g->edit_box, sizeof g->edit_box);
    return 1;
}
static void gy_oracle(void *user, const float p[3], int distance_only, OrSample *out) {
    (void)user;
    gyroid(p, distance_only, (float *)out);
}

/* ---- the demo through the device route ---- */
typedef struct {
    sdfv_demo_params prm;
    long fail_after;  /* calls before one fails (< 0: never) */
    long calls;       /* sampling calls so far */
} DeviceDemo;

static void demo_bb(void *user, float out[6]) {
    (void)user;
    const float bb[6] = {-1, -1, -1, 1, 1, 1};
    memcpy(out, bb, sizeof bb);
}
static int demo_device(void *user, const float *points_dev, size_t n, sdfv_sample *out_dev, void *stream) {
    DeviceDemo *d = (DeviceDemo *)user;
    const long call = d->calls++;
    if (d->fail_after >= 0 && call == d->fail_after) return 7;
    return sdfv_sample_points(&d->prm, SDFV_SDF_DEMO, points_dev, n, 0, out_dev, stream);
}

/* ---- the comparison ---- */
typedef struct {
    uint32_t dims[3];
    float bb[6];
    size_t n;
    float *r0, *r1, *t0, *t1;  /* oracle, viewer */
    OrLoadingManager lm;
} Ref;

static void ref_new(Ref *r, const uint32_t dims[3], const float bb[6], int passes) {
    memcpy(r->dims, dims, sizeof r->dims);
    memcpy(r->bb, bb, sizeof r->bb);
    r->n = (size_t)dims[0] * dims[1] * dims[2];
    r->r0 = malloc(r->n * 16);
    r->r1 = malloc(r->n * 16);
    r->t0 = malloc(r->n * 16);
    r->t1 = malloc(r->n * 16);
    CHECK(r->r0 && r->r1 && r->t0 && r->t1);
    or_grid_init(r->r0, r->r1, r->n);
    const uint64_t lim[3] = {dims[0], dims[1], dims[2]};
    or_lm_new(&r->lm, lim, (uint64_t)passes);
}
static void ref_reload(Ref *r) {
    const uint64_t lim[3] = {r->dims[0], r->dims[1], r->dims[2]};
    or_lm_new(&r->lm, lim, 3);
}
static void ref_free(Ref *r) {
    free(r->r0);
    free(r->r1);
    free(r->t0);
    free(r->t1);
}
static void ref_compare(Ref *r, sdfv_viewer *v) {
    OK(sdfv_viewer_download(v, r->t0, r->t1));
    CHECK(memcmp(r->t0, r->r0, r->n * 16) == 0);
    CHECK(memcmp(r->t1, r->r1, r->n * 16) == 0);
}
/* one update of the viewer, the same number of iterations of the oracle's loop, and the textures compared */
static size_t step(Ref *r, sdfv_viewer *v, const sdfv_surface *s, uint64_t budget_ns, or_sample_fn fn, void *fn_user,
                   const OrDemoParams *demo, const float *box) {
    size_t visited = 0;
    const int rc = sdfv_viewer_update(v, s, budget_ns, &visited);
    if (rc != 0) printf("update: %s\n", sdfv_viewer_last_error(v));
    CHECK(rc == 0);
    uint64_t did = demo ? or_viewer_update(demo, OR_SDF_DEMO, r->dims, r->bb, r->bb + 3, &r->lm, box, visited, r->r0, r->r1)
                        : or_viewer_update_fn(fn, fn_user, r->dims, r->bb, r->bb + 3, &r->lm, box, visited, r->r0, r->r1);
    CHECK(did == visited);
    ref_compare(r, v);
    return visited;
}
static uint64_t remaining(const sdfv_viewer *v) {
    sdfv_load_state st;
    OK(sdfv_viewer_state(v, &st));
    return st.remaining;
}

/* (a) + (d), host route */
static void host_gyroid(int threads) {
    Gyroid gy = {0, {-1.0f, -0.3f, -0.75f, 0.1f, 0.5f, 0.75f}, threads};
    sdfv_surface s;
    memset(&s, 0, sizeof s);
    s.user = &gy;
    s.bounding_box = gy_bb;
    s.sample = gy_sample;
    s.sample_concurrency = gy_concurrency;
    s.changed = gy_changed;
    sdfv_viewer *v = NULL;
    OK(sdfv_viewer_from_bb(k_bounds, 160, 3, &v));  /* 160 x 80 x 120: more than one 30 ms call on one thread */
    OK(sdfv_viewer_set_ingest(v, (uint32_t)threads, 4096));
    sdfv_load_state st;
    OK(sdfv_viewer_state(v, &st));
    Ref r;
    ref_new(&r, st.dims, k_bounds, 3);
    g_thickness = 0.15f;
    int steps = 0;
    while (remaining(v)) {
        step(&r, v, &s, 30000000ull, gy_oracle, NULL, NULL, NULL);
        ++steps;
    }
    CHECK(steps >= (threads == 1 ? 2 : 1));  /* progressive: intermediate states were compared */
    /* (d): an edit reports a box */
    g_thickness = 0.3f;
    gy.changed = 1;
    ref_reload(&r);
    step(&r, v, &s, 0, gy_oracle, NULL, NULL, gy.edit_box);
    while (remaining(v)) step(&r, v, &s, 30000000ull, gy_oracle, NULL, NULL, gy.edit_box);
    g_thickness = 0.15f;
    ref_free(&r);
    sdfv_viewer_free(v);
    printf("(a)+(d) host gyroid, %d thread(s): %d steps\n", threads, steps);
}

/* (b) */
static void demo_device_params(void) {
    sdfv_demo_params prm;
    sdfv_demo_params_default(&prm);
    sdfv_surface s;
    memset(&s, 0, sizeof s);
    s.bounding_box = demo_bb;
    s.device_params = &prm;
    const uint32_t dims[3] = {64, 64, 64};
    const float bb[6] = {-1, -1, -1, 1, 1, 1};
    sdfv_viewer *v = NULL;
    OK(sdfv_viewer_new_voxels(dims, bb, 3, SDFV_LAYOUT_AUTO, &v));
    size_t visited = 0;
    OK(sdfv_viewer_update(v, &s, 1000000000ull, &visited));
    CHECK(visited == 64 * 64 * 64 + 32 * 32 * 32 + 16 * 16 * 16 && remaining(v) == 0);
    Ref r;
    ref_new(&r, dims, bb, 3);
    sdfv_grid g;
    float *t0 = NULL, *t1 = NULL;
    OK(sdfv_viewer_textures(v, &t0, &t1, &g));
    CHECK(t0 && t1 && g.dims[0] == 64);
    float *d0 = NULL, *d1 = NULL;
    CHECK(hipMalloc((void **)&d0, r.n * 16) == hipSuccess && hipMalloc((void **)&d1, r.n * 16) == hipSuccess);
    OK(sdfv_fill_grid(&prm, SDFV_SDF_DEMO, &g, d0, d1, NULL));
    CHECK(hipDeviceSynchronize() == hipSuccess);
    CHECK(hipMemcpy(r.r0, d0, r.n * 16, hipMemcpyDeviceToHost) == hipSuccess);
    CHECK(hipMemcpy(r.r1, d1, r.n * 16, hipMemcpyDeviceToHost) == hipSuccess);
    ref_compare(&r, v);
    (void)hipFree(d0);
    (void)hipFree(d1);
    ref_free(&r);
    sdfv_viewer_free(v);
    printf("(b) demo as device_params == sdfv_fill_grid\n");
}

static float g_pending_box[6] = {-1, -1, -1, 0.2f, 1, 1};
static int g_pending = 1;
static int changed_once(void *user, float out[6]) {
    (void)user;
    if (!g_pending) return 0;
    g_pending = 0;
    memcpy(out, g_pending_box, sizeof g_pending_box);
    return 1;
}

/* (c) + (d) + (e), device route */
static void demo_device_callback(const uint32_t dims[3], sdfv_volume_layout layout, int with_edit) {
    DeviceDemo dd;
    sdfv_demo_params_default(&dd.prm);
    dd.fail_after = -1;
    dd.calls = 0;
    const float *box = g_pending_box;
    sdfv_surface s;
    memset(&s, 0, sizeof s);
    s.user = &dd;
    s.bounding_box = demo_bb;
    s.sample_batch_device = demo_device;
    const float bb[6] = {-1, -1, -1, 1, 1, 1};
    sdfv_viewer *v = NULL;
    OK(sdfv_viewer_new_voxels(dims, bb, 3, layout, &v));
    hipStream_t stream = NULL;
    CHECK(hipStreamCreate(&stream) == hipSuccess);
    OK(sdfv_viewer_set_stream(v, stream));
    Ref r;
    ref_new(&r, dims, bb, 3);
    OrDemoParams op;
    memcpy(&op, &dd.prm, sizeof op);
    int steps = 0;
    while (remaining(v)) {
        step(&r, v, &s, 0, NULL, NULL, &op, NULL);
        ++steps;
    }
    CHECK(steps >= 4);
    if (with_edit) {
        /* (d): new parameters, reported as a box that covers part of the grid */
        dd.prm.sphere_radius = 0.8f;
        memcpy(&op, &dd.prm, sizeof op);
        sdfv_surface se = s;
        se.changed = changed_once;  /* reports g_pending_box once */
        ref_reload(&r);
        /* (e): the third sampling of the reload fails */
        dd.fail_after = 2;
        dd.calls = 0;
        int failed = 0;
        while (remaining(v) || g_pending) {
            OK(sdfv_viewer_download(v, r.t0, r.t1));
            size_t visited = 0;
            const int rc = sdfv_viewer_update(v, &se, 0, &visited);
            if (rc == SDFV_ERR_CALLBACK) {
                CHECK(!failed && visited == 0 && strstr(sdfv_viewer_last_error(v), "sample_batch_device") != NULL);
                failed = 1;
                ref_compare(&r, v);  /* as the last complete run left them */
                continue;
            }
            CHECK(rc == 0);
            CHECK(or_viewer_update(&op, OR_SDF_DEMO, r.dims, r.bb, r.bb + 3, &r.lm, box, visited, r.r0, r.r1) == visited);
            ref_compare(&r, v);
        }
        CHECK(failed);
    }
    ref_free(&r);
    sdfv_viewer_free(v);
    (void)hipStreamDestroy(stream);
    printf("(c)%s device callback %ux%ux%u layout %d: %d steps\n", with_edit ? "+(d)+(e)" : "", dims[0], dims[1], dims[2],
           (int)layout, steps);
}

/* (c), several runs in one call: the device route with runs of at most 5000 points and a budget that lets one update load
 * the whole grid -- every pass boundary inside one call -- then the changed-box reload the same way */
static void demo_device_one_call(const uint32_t dims[3], sdfv_volume_layout layout) {
    DeviceDemo dd;
    sdfv_demo_params_default(&dd.prm);
    dd.fail_after = -1;
    dd.calls = 0;
    sdfv_surface s;
    memset(&s, 0, sizeof s);
    s.user = &dd;
    s.bounding_box = demo_bb;
    s.sample_batch_device = demo_device;
    const float bb[6] = {-1, -1, -1, 1, 1, 1};
    sdfv_viewer *v = NULL;
    OK(sdfv_viewer_new_voxels(dims, bb, 3, layout, &v));
    OK(sdfv_viewer_set_ingest(v, 0, 5000));
    Ref r;
    ref_new(&r, dims, bb, 3);
    OrDemoParams op;
    memcpy(&op, &dd.prm, sizeof op);
    const size_t visited = step(&r, v, &s, 60000000000ull, NULL, NULL, &op, NULL);
    CHECK(remaining(v) == 0 && visited == r.n + (size_t)((dims[0] + 1) / 2) * ((dims[1] + 1) / 2) * ((dims[2] + 1) / 2) +
                                                (size_t)((dims[0] + 3) / 4) * ((dims[1] + 3) / 4) * ((dims[2] + 3) / 4));
    CHECK(dd.calls > 3);  /* (more than one run) */
    dd.prm.sphere_radius = 0.8f;
    memcpy(&op, &dd.prm, sizeof op);
    sdfv_surface se = s;
    se.changed = changed_once;
    g_pending = 1;
    ref_reload(&r);
    step(&r, v, &se, 60000000000ull, NULL, NULL, &op, g_pending_box);
    CHECK(remaining(v) == 0);
    ref_free(&r);
    sdfv_viewer_free(v);
    printf("(c) device callback, one call over every run: %ux%ux%u layout %d, %ld sampling calls\n", dims[0], dims[1], dims[2],
           (int)layout, dd.calls);
}

int main(void) {
    CHECK(sdfv_viewer_abi_version() == SDFV_VIEWER_ABI_VERSION);
    host_gyroid(1);
    host_gyroid(8);
    demo_device_params();
    const uint32_t cube[3] = {64, 64, 64}, odd[3] = {40, 27, 33};
    demo_device_callback(cube, SDFV_LAYOUT_PLAIN, 1);
    g_pending = 1;
    demo_device_callback(cube, SDFV_LAYOUT_INTERLEAVED, 1);
    g_pending = 1;
    demo_device_callback(odd, SDFV_LAYOUT_PLAIN, 1);
    demo_device_one_call(cube, SDFV_LAYOUT_INTERLEAVED);
    demo_device_one_call(odd, SDFV_LAYOUT_PLAIN);
    printf("viewer_host ok\n");
    return 0;
}
