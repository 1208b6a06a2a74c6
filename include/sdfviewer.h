/*
 * sdfviewer.h -- C ABI of the viewer: SDFViewer and SDFViewerAppScene over any SDF the caller describes with callbacks.
 * Exported by libsdfviewer_host.so (which links libsdfgrid.so).
 *
 * This is the reference's controller, flat (paths relative to the reference root):
 *   sdfv_viewer_*  SDFViewer::{from_bb, new_voxels, update, commit}   src/app/scene/sdf/mod.rs:46,75,128,220
 *   sdfv_scene_*   SDFViewerAppScene::{new, set_sdf, render, load_progress}   src/app/scene/mod.rs:80-247
 *   sdfv_surface   `impl SDFSurface`   src/sdf/mod.rs:33-43
 * The library owns all load state: the LoadingManager, changed_box, what each pass may assume about the grid.  A caller of
 * this header never passes pass flags (those are sdfgrid.h's, for callers that drive the kernels themselves).
 *
 * Conventions
 *   - every call returns an sdfv_status (sdfgrid.h): 0 on success, negative on failure.  Each handle keeps the message of its
 *     last failure (sdfv_viewer_last_error / sdfv_scene_last_error; "" after a call that went through).  A constructor that
 *     fails returns its status alone (SDFV_ERR_NO_DEVICE without a GPU, SDFV_ERR_INVALID_ARGUMENT, SDFV_ERR_INTERNAL).
 *   - nothing crosses the C boundary: a callback that reports a failure, or an error inside the library, ends the call with an
 *     error.  The run it happened in is dropped -- the textures keep what the last complete run left, the LoadingManager is
 *     not advanced past what was packed -- and a later update samples that run again.
 *   - a handle is single-owner: one thread at a time.  Device pointers are HIP device memory; `stream` is a hipStream_t.
 */
#ifndef SDFVIEWER_H
#define SDFVIEWER_H

#include <stddef.h>
#include <stdint.h>

#include "sdfgrid.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 1: the first version. */
#define SDFV_VIEWER_ABI_VERSION 1

/* status codes beyond sdfgrid.h's sdfv_status */
#define SDFV_ERR_CALLBACK (-6) /* a callback of the surface reported a failure (the message names it) */
#define SDFV_ERR_INTERNAL (-7) /* the library could not complete the call (out of memory, ...) */

/* ---- the surface: `impl SDFSurface` as a struct of callbacks ----
 * The library copies the struct; `user` must outlive every call that uses it.  update() picks its route in this order:
 * device_params (the demo: the device path of sdfgrid.h), then sample_batch_device, then the host routes. */
typedef struct sdfv_surface {
    void *user;
    /* REQUIRED: [min.xyz, max.xyz] (src/sdf/mod.rs:35) */
    void (*bounding_box)(void *user, float out[6]);
    /* SDFSurface::sample (src/sdf/mod.rs:43); non-zero = failure.  Required unless a batch form is given. */
    int (*sample)(void *user, const float p[3], int distance_only, sdfv_sample *out);
    /* optional: out[i] = sample(p[3 i .. 3 i + 2]) for i < n, HOST memory; non-zero = failure */
    int (*sample_batch)(void *user, const float *p, size_t n, int distance_only, sdfv_sample *out);
    /* optional (default 1): how many host threads may call sample / sample_batch at once */
    uint32_t (*sample_concurrency)(void *user);
    /* optional: 1 = Some(box) written to out, 0 = None.  Called once at the start of every update (scene/sdf/mod.rs:130). */
    int (*changed)(void *user, float out[6]);
    /* optional, the device route: enqueue out_dev[i] = sample(points_dev[3 i .. 3 i + 2], false) for i < n on `stream` and
     * return without synchronising the device; DEVICE memory; non-zero = failure */
    int (*sample_batch_device)(void *user, const float *points_dev, size_t n, sdfv_sample *out_dev, void *stream);
    /* optional: when set, the surface IS the demo with these parameters (the library copies them per update) */
    const sdfv_demo_params *device_params;
    uint32_t device_sdf_id;
} sdfv_surface;

typedef struct sdfv_viewer sdfv_viewer;
typedef struct sdfv_scene sdfv_scene;

/* how the 4 B/voxel distance volume next to the textures is laid out (SDFViewer::VolumeLayout) */
typedef enum sdfv_volume_layout {
    SDFV_LAYOUT_AUTO = 0,       /* what the march reads fastest for this grid */
    SDFV_LAYOUT_PLAIN = 1,      /* texture order */
    SDFV_LAYOUT_INTERLEAVED = 2 /* y-interleaved (needs an even height) */
} sdfv_volume_layout;

/* a perspective camera (three-d Camera::new_perspective, scene/mod.rs:82-95) */
typedef struct sdfv_view {
    float position[3];
    float target[3];
    float up[3];
    float fovy_degrees;
    float z_near;
    float z_far;
} sdfv_view;

typedef struct sdfv_load_state {
    uint64_t remaining;        /* LoadingManager::len() */
    uint64_t total_iterations; /* LoadingManager::total_iterations() */
    uint32_t passes_left;      /* 0 = loaded */
    uint32_t has_changed_box;
    float lod_dist_between_samples; /* the shader's LOD uniform, 2^passes_left */
    uint32_t dims[3];
} sdfv_load_state;

uint32_t sdfv_viewer_abi_version(void);

/* ---- the viewer ---- */
/* SDFViewer::from_bb: voxels from the box and max_voxels_side (scene/sdf/mod.rs:46-72) */
int sdfv_viewer_from_bb(const float bb[6], uint32_t max_voxels_side, uint32_t loading_passes, sdfv_viewer **out);
/* SDFViewer::new_voxels (scene/sdf/mod.rs:75-101) */
int sdfv_viewer_new_voxels(const uint32_t dims[3], const float bb[6], uint32_t loading_passes, sdfv_volume_layout layout,
                           sdfv_viewer **out);
/* SDFViewer::update(sdf, max_delta_time): *visited = the LoadingManager iterations consumed (the reference's return value) --
 * on an error too: then the iterations of the runs that were packed before the one that failed (budget_ns: a run is timed to
 * its end, so a call returns with nothing of it left in flight) */
int sdfv_viewer_update(sdfv_viewer *v, const sdfv_surface *surface, uint64_t budget_ns, size_t *visited);
int sdfv_viewer_commit(sdfv_viewer *v);
int sdfv_viewer_state(const sdfv_viewer *v, sdfv_load_state *out);
/* the device textures (W*H*D RGBA32F each, see sdfgrid.h) and the grid they hold, for interop */
int sdfv_viewer_textures(const sdfv_viewer *v, float **tex0, float **tex1, sdfv_grid *grid);
/* both textures to HOST memory (W*H*D*4 floats each); synchronises the viewer's stream */
int sdfv_viewer_download(sdfv_viewer *v, float *tex0_host, float *tex1_host);
/* SDFViewerMaterial::render: one ray per pixel into rgba_device (width*height*4 floats, DEVICE); view NULL = the scene's
 * default camera.  The march runs on the CALLING thread, so that thread's options hold: while the grid is still loading,
 * sdfv_set_option(SDFV_OPT_RAYMARCH_LOD_FILTER, 1) (sdfgrid.h) on it makes this frame -- and sdfv_scene_render's -- interpolate
 * between the loaded lattice points instead of snapping to the nearest.  Nothing is exported here for it */
int sdfv_viewer_render(sdfv_viewer *v, const sdfv_view *view, uint32_t width, uint32_t height, float *rgba_device);
/* the hipStream_t every later call of this viewer enqueues on (NULL = the default stream) */
int sdfv_viewer_set_stream(sdfv_viewer *v, void *stream);
/* host routes: sampling threads (0 = what the surface allows) and records per run (0 = automatic) */
int sdfv_viewer_set_ingest(sdfv_viewer *v, uint32_t host_threads, size_t capacity);
const char *sdfv_viewer_last_error(const sdfv_viewer *v); /* never NULL */
void sdfv_viewer_free(sdfv_viewer *v);

/* ---- the scene ---- */
typedef struct sdfv_render_report { /* what the reference logs per frame (scene/mod.rs:180-197) */
    uint64_t cpu_updates;
    uint32_t committed;
    uint32_t last_chunk;
    uint32_t request_repaint;
} sdfv_render_report;

/* the scene's clock in nanoseconds (any epoch); NULL = the steady clock */
typedef uint64_t (*sdfv_clock_fn)(void *user);

/* SDFViewerAppScene::new: the default camera, a 32^3 / 2-pass viewer (scene/mod.rs:80-136) */
int sdfv_scene_new(const sdfv_surface *surface, sdfv_clock_fn clock, void *clock_user, sdfv_scene **out);
/* set_sdf: a new viewer for this surface; 0 keeps the previous max_voxels_side / loading_passes (scene/mod.rs:139-156) */
int sdfv_scene_set_surface(sdfv_scene *s, const sdfv_surface *surface, uint32_t max_voxels_side, uint32_t loading_passes);
int sdfv_scene_set_camera(sdfv_scene *s, const sdfv_view *view);
/* the per-frame load budget (30 ms) and the least time between commits while loading (500 ms), scene/mod.rs:168-174 */
int sdfv_scene_set_budget(sdfv_scene *s, uint32_t load_budget_ms, uint32_t commit_interval_ms);
/* one frame: load within the budget, commit sparingly, draw into rgba_device (width*height*4 floats, DEVICE; NULL = no drawing) */
int sdfv_scene_render(sdfv_scene *s, uint32_t width, uint32_t height, float *rgba_device, sdfv_render_report *out);
/* *loading = 0: None.  Else the progress in [0, 1] and its text (scene/mod.rs:228-247), cut to text_len bytes with its NUL */
int sdfv_scene_load_progress(const sdfv_scene *s, int *loading, float *progress, char *text, size_t text_len);
/* the scene's current viewer (owned by the scene, valid until the next set_surface or free) */
sdfv_viewer *sdfv_scene_viewer(sdfv_scene *s);
const char *sdfv_scene_last_error(const sdfv_scene *s); /* never NULL */
void sdfv_scene_free(sdfv_scene *s);

#ifdef __cplusplus
}
#endif
#endif
