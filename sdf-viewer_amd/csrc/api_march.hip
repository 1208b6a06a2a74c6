// api_march.hip -- the grid march: what its kernels are told, the launch policy, tile bands, and the rounds of the sharded march.
#include <cmath>
#include <cstddef>
#include <cstring>

#include "api_internal.h"
#include "march_plan.h"
#include "raymarch_kernels.h"

using namespace sdfv;

namespace {

// A batch of more than kMaxCamerasPerLaunch cameras is several launches (the cameras ride in the kernel-argument block).  When
// each is small -- low-resolution views, a rank's share of a split batch -- it is as long as its longest waves, not as its
// work, and running them one after the other multiplies that: such launches go to side streams forked from and joined back
// into the caller's stream (events only: capturable), where they overlap.  Created on first use, per thread and device.
struct BatchStreams {
    static constexpr int kSide = 3;
    hipStream_t side[kSide] = {};
    hipEvent_t fork = nullptr, join[kSide] = {};
    int device = -1;
    void release() {
        for (int i = 0; i < kSide; ++i) {
            if (side[i]) (void)hipStreamDestroy(side[i]);
            if (join[i]) (void)hipEventDestroy(join[i]);
        }
        if (fork) (void)hipEventDestroy(fork);
        *this = BatchStreams{};
    }
    hipError_t ensure(int device_now) {
        if (device == device_now && fork) return hipSuccess;
        release();
        hipError_t e = hipEventCreateWithFlags(&fork, hipEventDisableTiming);
        for (int i = 0; i < kSide && e == hipSuccess; ++i) {
            e = hipStreamCreateWithFlags(&side[i], hipStreamNonBlocking);
            if (e == hipSuccess) e = hipEventCreateWithFlags(&join[i], hipEventDisableTiming);
        }
        if (e != hipSuccess) release();
        else device = device_now;
        return e;
    }
};
thread_local BatchStreams g_batch_streams;  // released by sdfv_mesh_trim(); a thread that exits without it leaks three streams

// Cameras of a launch of more than kInlineCameras that arrive as a HOST array (the kernel-argument block carries 16): the
// launch reads them from a slot of this per-thread ring of device memory, written on the launch's own stream by small
// kernels that carry 32 cameras each as THEIR arguments -- no copy engine, no allocation per call, nothing the host waits
// for.  A slot is reused every kSlots launches; the event recorded behind its last reader orders the rewrite after it,
// whatever stream that reader ran on.  Allocated on first use (122 KB), released by sdfv_mesh_trim().
struct CameraRing {
    static constexpr uint32_t kSlots = 16;
    sdfv_camera* base = nullptr;  // kSlots x kMaxCamerasPerLaunch
    hipEvent_t read[kSlots] = {};
    bool recorded[kSlots] = {};
    uint32_t next = 0;
    int device = -1;
    void release() {
        for (uint32_t i = 0; i < kSlots; ++i)
            if (read[i]) (void)hipEventDestroy(read[i]);
        if (base) (void)hipFree(base);
        *this = CameraRing{};
    }
    hipError_t ensure(int device_now) {
        if (device == device_now && base) return hipSuccess;
        release();
        hipError_t e = hipMalloc(reinterpret_cast<void**>(&base), (size_t)kSlots * sdfv::kMaxCamerasPerLaunch * sizeof(sdfv_camera));
        for (uint32_t i = 0; i < kSlots && e == hipSuccess; ++i) e = hipEventCreateWithFlags(&read[i], hipEventDisableTiming);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            release();
        } else {
            device = device_now;
        }
        return e;
    }
};
thread_local CameraRing g_camera_ring;

}  // namespace

namespace sdfv {
void release_march_caches() {
    g_batch_streams.release();
    g_camera_ring.release();
}

// The light list: the scene's ambient light (rp->ambient) plus rp->lights.  Only ambient entries can be rendered.
int check_lights(const sdfv_render_params* rp) {
    if (rp->n_lights > SDFV_MAX_LIGHTS)
        return set_error(SDFV_ERR_INVALID_ARGUMENT, "n_lights %u exceeds SDFV_MAX_LIGHTS", rp->n_lights);
    for (uint32_t i = 0; i < rp->n_lights; ++i) {
        if (rp->lights[i].kind == SDFV_LIGHT_DIRECTIONAL)
            return set_error(SDFV_ERR_INVALID_ARGUMENT,
                        "lights[%u] is directional: three-d 0.18.2 shader source not available (scene/mod.rs:107-112 keeps "
                        "its directional lights commented out; their BRDF is not restated from memory)", i);
        if (rp->lights[i].kind != SDFV_LIGHT_AMBIENT)
            return set_error(SDFV_ERR_INVALID_ARGUMENT, "lights[%u] has unknown kind %u", i, rp->lights[i].kind);
    }
    return SDFV_OK;
}
}  // namespace sdfv

namespace {

// What every march launch is told besides the render parameters: the two textures and the rows of the image.
void set_march_frame(sdfv::RaymarchArgs& a, const float* tex0, const float* tex1, uint32_t width, uint32_t height, uint32_t y0, uint32_t y1) {
    a.tex0 = reinterpret_cast<const float4*>(tex0);
    a.tex1 = reinterpret_cast<const float4*>(tex1);
    a.width = width;
    a.height = height;
    a.y0 = y0;
    a.y1 = y1;
}

// The argument checks of a march call, then the device.
int check_march_call(const sdfv_march_desc& d, uint32_t y0, uint32_t y1, uint32_t lod_filter) {
    const sdfv_render_params* rp = d.rp;
    if (!rp || !d.tex0 || !d.tex1) return set_error(SDFV_ERR_INVALID_ARGUMENT, "NULL argument");
    if (!d.rgba && !d.rgba8) return set_error(SDFV_ERR_INVALID_ARGUMENT, "no colour output: rgba and rgba8 are both NULL");
    if (int rc = check_lights(rp)) return rc;
    if (int rc = check_texel_alignment(d.tex0, d.tex1, d.rgba)) return rc;
    if (int rc = check_word_aligned("dist, depth, aux and rgba8", d.dist, d.depth, d.aux, d.rgba8)) return rc;
    if (((uintptr_t)d.pairs | (uintptr_t)d.ilv) & 7) return set_error(SDFV_ERR_INVALID_ARGUMENT, "pairs and ilv must be 8-byte aligned");
    if (d.n_cameras && !d.cameras) return set_error(SDFV_ERR_INVALID_ARGUMENT, "cameras is NULL");
    if (y0 > y1 || y1 > d.height) return set_error(SDFV_ERR_INVALID_ARGUMENT, "rows [%u,%u) outside height %u", y0, y1, d.height);
    if (rp->tex_size[0] == 0 || rp->tex_size[1] == 0 || rp->tex_size[2] == 0)
        return set_error(SDFV_ERR_INVALID_ARGUMENT, "empty texture");
    if (!(rp->lod_dist_between_samples >= 1.0f)) return set_error(SDFV_ERR_INVALID_ARGUMENT, "lod_dist_between_samples < 1");
    if (lod_filter == 1 && rp->lod_dist_between_samples != 1.0f) {  // the lattice filter: L a power of two (what LoadingManager publishes)
        int e = 0;
        const float lod = rp->lod_dist_between_samples;
        if (!(lod >= 2.0f && lod <= 32768.0f) || frexpf(lod, &e) != 0.5f)
            return set_error(SDFV_ERR_INVALID_ARGUMENT,
                             "SDFV_OPT_RAYMARCH_LOD_FILTER 1: lod_dist_between_samples %g is not a power of two in [2, 32768]", (double)lod);
    }
    if ((uint64_t)rp->tex_size[0] * rp->tex_size[1] * rp->tex_size[2] >= (1ull << 32))
        return set_error(SDFV_ERR_INVALID_ARGUMENT, "texture too large for 32-bit texel indexing");
    return need_device();
}

// What the device and the calling thread's options contribute to a launch (march_plan.h: apply_march_policy).
sdfv::MarchPolicy march_policy() {
    const DeviceFacts& dev = device_facts();
    return {dev.gfx950, dev.cus, dev.xcds, dev.last_level_cache_bytes, g_options.raymarch_tile_group, g_options.raymarch_waves_per_simd,
            g_options.raymarch_box_first};
}

// Everything the launches of a call are told, cameras and output planes apart: rows [y0, y1) of the image (band_step 1), or the
// bands of band_height rows y0 / band_height, y0 / band_height + band_step, ... below y1 == height.
void fill_march_args(const sdfv_march_desc& d, uint32_t y0, uint32_t y1, uint32_t band_step, uint32_t band_height, sdfv::RaymarchArgs& a) {
    derive_raymarch_args(d.rp, g_options.raymarch_disable, a);
    a.dist = d.dist;
    a.pairs = d.pairs;
    a.ilv = d.ilv;
    set_march_frame(a, d.tex0, d.tex1, d.width, d.height, y0, y1);
    a.band_skip = band_height * (band_step - 1u);
    a.band_shift = band_height == 8u ? 3u : 4u;
    a.rows_out = band_step > 1 ? sdfv_band_rows_ex(d.height, y0 / band_height, band_step, band_height) : y1 - y0;
    // sdfNormal's result only feeds calculate_lighting (material.frag:155,163), and the one AmbientLight the scene
    // configures (scene/mod.rs:106-112) does not read it: dead code a GLSL compiler removes.  It is evaluated when the
    // aux record asks for it; SDFV_OPT_RAYMARCH_KEEP_NORMAL evaluates it per hit regardless (what it would cost once a
    // directional light uses it).
    a.compute_normal = g_options.raymarch_keep_normal ? 1u : 0u;
    apply_march_policy(a, march_policy(), d.n_cameras);
#ifdef SDFV_TUNING
    a.wave_timing = reinterpret_cast<unsigned long long*>(g_options.wave_timing);  // 32 B per wave, or 0
    a.priority_map = reinterpret_cast<const unsigned char*>(g_options.priority_map);
    a.tile_order = d.n_cameras == 1 ? reinterpret_cast<const uint32_t*>(g_options.tile_order) : nullptr;
#endif
}

// Where the launches of a call read their cameras (march_plan.h: camera_source).  kStaged means a slot of the camera ring per
// launch (CameraRing); if the ring cannot be had the batch goes out as launches of kInlineCameras instead (same pixels).
sdfv::CameraSource cameras_of_call(const sdfv_camera* cameras, uint32_t n_cameras, hipStream_t main) {
    // (asked for ANY count -- ADVICE r04: a device array of <= kInlineCameras cameras, e.g. a rank's share of a resident batch,
    // used to be memcpy'd from on the host; the kernel reads camera_list for any count)
    hipPointerAttribute_t attr;
    const bool on_device = hipPointerGetAttributes(&attr, cameras) == hipSuccess && (attr.type == hipMemoryTypeDevice || attr.type == hipMemoryTypeManaged);
    hipStreamCaptureStatus capturing = hipStreamCaptureStatusNone;
    if (!on_device) {
        (void)hipGetLastError();
        if (n_cameras > sdfv::kInlineCameras && hipStreamIsCapturing(main, &capturing) != hipSuccess) (void)hipGetLastError();
    }
    sdfv::CameraSource src = sdfv::camera_source(n_cameras, on_device, capturing != hipStreamCaptureStatusNone, g_options.raymarch_camera_staging != 0);
    if (src == sdfv::CameraSource::kStaged && g_camera_ring.ensure(current_device()) != hipSuccess) src = sdfv::CameraSource::kInline;
    return src;
}

// The launches of one call: kMaxCamerasPerLaunch or kInlineCameras cameras each, small ones overlapping on side streams.
int launch_march_batch(const sdfv_march_desc& d, sdfv::RaymarchArgs& a, uint32_t lod_filter, hipStream_t main) {
    const uint32_t n_cameras = d.n_cameras;
    const sdfv_camera* cameras = d.cameras;
    const uint64_t pixels_per_cam = (uint64_t)a.rows_out * d.width;
    const sdfv::CameraSource source = cameras_of_call(cameras, n_cameras, main);
    const bool ring = source == sdfv::CameraSource::kStaged;
    const uint32_t per_launch = sdfv::cameras_per_launch(source);
    const uint64_t groups_per_launch = (uint64_t)((d.width + 15) / 16) * ((a.rows_out + 15) / 16) * per_launch;
    const bool overlap = sdfv::launches_overlap(n_cameras, per_launch, groups_per_launch) && g_options.raymarch_batch_streams;  // see BatchStreams
    uint32_t used = 0;  // side streams that carry a launch of this call
    int rc = SDFV_OK;
    auto hip_ok = [&](hipError_t e, const char* what) {
        if (e != hipSuccess && rc == SDFV_OK) rc = hip_fail(e, what);
        return e == hipSuccess;
    };
    if (overlap) hip_ok(g_batch_streams.ensure(current_device()), "batch streams") && hip_ok(hipEventRecord(g_batch_streams.fork, main), "hipEventRecord");
    uint32_t launch = 0;
    for (uint32_t c0 = 0; c0 < n_cameras && rc == SDFV_OK; c0 += per_launch, ++launch) {
        const uint32_t nc = n_cameras - c0 < per_launch ? n_cameras - c0 : per_launch;
        a.n_cameras = nc;
        if (source == sdfv::CameraSource::kInPlace) a.camera_list = cameras + c0;
        else if (!ring) memcpy(a.cameras, cameras + c0, nc * sizeof(sdfv_camera));
        point_outputs_at(a, pixels_per_cam, c0, d.rgba, d.rgba8, d.aux, d.depth);
        hipStream_t on = main;
        const uint32_t lane = launch % (BatchStreams::kSide + 1);  // 0 = the caller's stream
        if (overlap && lane != 0) {
            on = g_batch_streams.side[lane - 1];
            if (lane > used) {
                if (!hip_ok(hipStreamWaitEvent(on, g_batch_streams.fork, 0), "hipStreamWaitEvent")) break;
                used = lane;
            }
        }
        if (ring) {
            CameraRing& r = g_camera_ring;
            const uint32_t slot = r.next++ % CameraRing::kSlots;
            sdfv_camera* at = r.base + (size_t)slot * sdfv::kMaxCamerasPerLaunch;
            if (r.recorded[slot] && !hip_ok(hipStreamWaitEvent(on, r.read[slot], 0), "hipStreamWaitEvent")) break;
            if (!hip_ok(sdfv::launch_store_cameras(cameras + c0, nc, at, on), "store_cameras")) break;
            a.camera_list = at;
            hip_ok(sdfv::launch_raymarch(a, on, lod_filter), "launch_raymarch") && hip_ok(hipEventRecord(r.read[slot], on), "hipEventRecord");
            r.recorded[slot] = true;  // (a failed record leaves the event as it was: waiting on it is harmless)
            continue;
        }
        hip_ok(sdfv::launch_raymarch(a, on, lod_filter), "launch_raymarch");
    }
    for (uint32_t i = 0; i < used; ++i)  // (joined even after an error: the side streams must not run on behind the caller's)
        hip_ok(hipEventRecord(g_batch_streams.join[i], g_batch_streams.side[i]), "hipEventRecord") &&
            hip_ok(hipStreamWaitEvent(main, g_batch_streams.join[i], 0), "hipStreamWaitEvent");
    return rc;
}

// Rows [y0, y1) of the image (band_step 1), or the 16-row bands y0 / 16, y0 / 16 + band_step, ... below y1 == height.
int raymarch_rows(const sdfv_march_desc& d, uint32_t y0, uint32_t y1, uint32_t band_step, uint32_t band_height, void* stream) {
    const uint32_t lod_filter = g_options.raymarch_lod_filter;
    if (int rc = check_march_call(d, y0, y1, lod_filter)) return rc;
    sdfv::RaymarchArgs a;
    fill_march_args(d, y0, y1, band_step, band_height, a);
    return launch_march_batch(d, a, lod_filter, (hipStream_t)stream);
}

// Argument checks and RaymarchArgs / SlabMarchArgs shared by the two forms of a round of the sharded march.
int slab_round_args(const sdfv_render_params* rp, const sdfv_grid* slab, uint32_t ghost_lo, uint32_t ghost_hi,
                           const float* tex0, const float* tex1, const sdfv_camera* camera, uint32_t width, uint32_t height,
                           float* rgba, sdfv_march_aux* aux, sdfv::RaymarchArgs& a, sdfv::SlabMarchArgs& s) {
    if (!rp || !slab || !tex0 || !tex1 || !camera || !rgba) return set_error(SDFV_ERR_INVALID_ARGUMENT, "NULL argument");
    if (int rc = check_grid(slab)) return rc;
    if (int rc = check_lights(rp)) return rc;
    if (int rc = check_texel_alignment(tex0, tex1, rgba)) return rc;
    for (int i = 0; i < 3; ++i)
        if (rp->tex_size[i] != slab->dims[i])
            return set_error(SDFV_ERR_INVALID_ARGUMENT, "render parameters describe a %ux%ux%u grid, the slab a %ux%ux%u one",
                        rp->tex_size[0], rp->tex_size[1], rp->tex_size[2], slab->dims[0], slab->dims[1], slab->dims[2]);
    if (slab->z_begin >= slab->z_end) return set_error(SDFV_ERR_INVALID_ARGUMENT, "empty slab");
    if (ghost_lo > slab->z_begin || slab->z_end + ghost_hi > slab->dims[2])
        return set_error(SDFV_ERR_INVALID_ARGUMENT, "ghost slices reach outside the grid");
    if (ghost_lo > 1 || ghost_hi > 2) return set_error(SDFV_ERR_INVALID_ARGUMENT, "at most 1 lower and 2 upper ghost slices");
    if (slab->z_end < slab->dims[2] && ghost_hi == 0)
        return set_error(SDFV_ERR_INVALID_ARGUMENT, "an interior slab needs its upper ghost slice (run the halo exchange)");
    if (rp->lod_dist_between_samples != 1.0f)
        return set_error(SDFV_ERR_INVALID_ARGUMENT, "the sharded march renders loaded grids only (lod_dist_between_samples == 1)");
    if ((uint64_t)width * height >= (1ull << 32)) return set_error(SDFV_ERR_INVALID_ARGUMENT, "image too large");
    const uint64_t resident = (uint64_t)slab->dims[0] * slab->dims[1] * (ghost_lo + (slab->z_end - slab->z_begin) + ghost_hi);
    if (resident >= (1ull << 32)) return set_error(SDFV_ERR_INVALID_ARGUMENT, "slab too large for 32-bit texel indexing");
    if (int rc = need_device()) return rc;
    derive_raymarch_args(rp, g_options.raymarch_disable, a);
    if (!a.fast_index)
        return set_error(SDFV_ERR_INVALID_ARGUMENT, "box too small for the sharded march: 1e-4 * N / size must be <= 0.25");
    set_march_frame(a, tex0, tex1, width, height, 0, height);
    a.rows_out = height;
    a.band_shift = 4;
    a.n_cameras = 1;
    a.cameras[0] = *camera;
    a.rgba = reinterpret_cast<float4*>(rgba);
    a.aux = aux;
    s = sdfv::SlabMarchArgs{};
    s.z_lo = slab->z_begin - ghost_lo;
    s.z_count = ghost_lo + (slab->z_end - slab->z_begin) + ghost_hi;
    s.own_begin = slab->z_begin;
    s.own_end = slab->z_end;
    return SDFV_OK;
}

}  // namespace

#pragma GCC visibility push(default)
extern "C" {

int sdfv_march_volume_advice(const sdfv_grid* grid, uint32_t* kind) {
    if (int rc = check_grid(grid)) return rc;
    if (!kind) return set_error(SDFV_ERR_INVALID_ARGUMENT, "kind is NULL");
    if (int rc = need_device()) return rc;
    // only the hand-written gfx950 loop reads these volumes -- on another device, or with that loop switched off, a
    // host would allocate 4-8 B/voxel and re-run the commit after every fill for a volume no march ever touches.  ADVICE r04:
    // and the loop's OTHER conditions (power-of-two extents, symmetric box, clamp-for-mirror, its addressing limits) are
    // asked of the launcher itself, over the render parameters a march of this grid would carry (sdfv_render_params_default).
    sdfv_render_params rp;
    sdfv_render_params_default(&rp, grid);
    sdfv::RaymarchArgs a;
    derive_raymarch_args(&rp, g_options.raymarch_disable, a);
    apply_march_policy(a, march_policy(), 1);
    // the launcher's own choice with all three volumes at hand (a grid that is not cubic marches fastest over its distance volume)
    const int mode = sdfv::march_volume_choice(a, true, true, true);
    *kind = mode == sdfv::kMarchIlv ? SDFV_MARCH_VOLUME_INTERLEAVED : mode == sdfv::kMarchPairs ? SDFV_MARCH_VOLUME_PAIRS : SDFV_MARCH_VOLUME_NONE;
    return SDFV_OK;
}

int sdfv_raymarch_ex(const sdfv_march_desc* desc, void* stream) {
    sdfv_march_desc d;
    if (int rc = read_sized_desc(desc, offsetof(sdfv_march_desc, depth), "sdfv_march_desc", d)) return rc;
    if (d.reserved != 0) return set_error(SDFV_ERR_INVALID_ARGUMENT, "sdfv_march_desc: reserved fields must be 0");
    if (d.band_step == 0 && d.band_height != 0)
        return set_error(SDFV_ERR_INVALID_ARGUMENT, "band_height %u with band_step 0: a band set needs band_step >= 1 (0 = rows [y0, y1))", d.band_height);
    if (d.band_step == 0)
        return raymarch_rows(d, d.y0, d.y1, 1, 16, stream);
    const uint32_t B = d.band_height ? d.band_height : 16u;
    if (B != 8u && B != 16u) return set_error(SDFV_ERR_INVALID_ARGUMENT, "band_height %u: 8 or 16 (0 = 16)", d.band_height);
    if (sdfv_band_rows_ex(d.height, d.band_first, d.band_step, B) == 0) return SDFV_OK;  // a band set below the image: nothing to render
    return raymarch_rows(d, d.band_first * B, d.height, d.band_step, B, stream);
}

uint32_t sdfv_band_rows_ex(uint32_t height, uint32_t band_first, uint32_t band_step, uint32_t band_height) {
    const uint32_t B = band_height ? band_height : 16u;
    if (B != 8u && B != 16u) return 0;
    const uint32_t bands = (height + B - 1) / B;
    if (band_step == 0 || band_first >= bands) return 0;
    const uint32_t n = (bands - band_first + band_step - 1) / band_step, last = band_first + (n - 1) * band_step;
    return (n - 1) * B + (height - last * B < B ? height - last * B : B);
}
uint32_t sdfv_band_rows(uint32_t height, uint32_t band_first, uint32_t band_step) {
    return sdfv_band_rows_ex(height, band_first, band_step, 16u);
}

int sdfv_raymarch_slab(const sdfv_render_params* rp, const sdfv_grid* slab, uint32_t ghost_lo, uint32_t ghost_hi,
                       const float* tex0, const float* tex1, const sdfv_camera* camera, uint32_t width, uint32_t height,
                       const sdfv_ray_state* in_states, uint32_t n_in, float* rgba, sdfv_march_aux* aux,
                       sdfv_ray_state* out_down, sdfv_ray_state* out_up, uint32_t capacity, uint32_t* counters,
                       void* stream) {
    if (!out_down || !out_up || !counters) return set_error(SDFV_ERR_INVALID_ARGUMENT, "NULL argument");
    if (in_states == nullptr && n_in != 0) return set_error(SDFV_ERR_INVALID_ARGUMENT, "n_in without in_states");
    sdfv::RaymarchArgs a;
    sdfv::SlabMarchArgs s;
    if (int rc = slab_round_args(rp, slab, ghost_lo, ghost_hi, tex0, tex1, camera, width, height, rgba, aux, a, s)) return rc;
    s.in = in_states;
    s.n_in = n_in;
    s.out_down = out_down;
    s.out_up = out_up;
    s.count_down = counters;
    s.count_up = counters + 1;
    s.capacity = capacity;
    if (in_states && n_in == 0) return SDFV_OK;  // nothing arrived this round
    SDFV_HIP_RETURN(sdfv::launch_raymarch_slab(a, s, (hipStream_t)stream));
}

size_t sdfv_ray_buffer_bytes(uint32_t capacity) { return SDFV_RAY_BUFFER_HEADER_BYTES + (size_t)capacity * sizeof(sdfv_ray_state); }

int sdfv_raymarch_slab_round(const sdfv_render_params* rp, const sdfv_grid* slab, uint32_t ghost_lo, uint32_t ghost_hi,
                             const float* tex0, const float* tex1, const sdfv_camera* camera, uint32_t width, uint32_t height,
                             const void* in_lo, const void* in_hi, int first_round, float* rgba, sdfv_march_aux* aux,
                             void* out_down, void* out_up, uint32_t capacity, uint32_t* overflow, void* stream) {
    return sdfv_internal_raymarch_slab_round(rp, slab, ghost_lo, ghost_hi, tex0, tex1, camera, width, height, in_lo, in_hi,
                                             first_round, rgba, aux, out_down, out_up, capacity, overflow, nullptr, stream);
}

__attribute__((visibility("hidden"))) int sdfv_internal_raymarch_slab_round(
    const sdfv_render_params* rp, const sdfv_grid* slab, uint32_t ghost_lo, uint32_t ghost_hi, const float* tex0, const float* tex1,
    const sdfv_camera* camera, uint32_t width, uint32_t height, const void* in_lo, const void* in_hi, int first_round, float* rgba,
    sdfv_march_aux* aux, void* out_down, void* out_up, uint32_t capacity, uint32_t* overflow, uint32_t* leftover, void* stream) {
    if (!out_down || !out_up) return set_error(SDFV_ERR_INVALID_ARGUMENT, "NULL ray buffer");
    if (int rc = check_word_aligned("ray buffers", in_lo, in_hi, out_down, out_up, overflow)) return rc;
    if (first_round && (in_lo || in_hi)) return set_error(SDFV_ERR_INVALID_ARGUMENT, "the first round takes no incoming rays");
    sdfv::RaymarchArgs a;
    sdfv::SlabMarchArgs s;
    if (int rc = slab_round_args(rp, slab, ghost_lo, ghost_hi, tex0, tex1, camera, width, height, rgba, aux, a, s)) return rc;
    auto count_of = [](const void* b) { return reinterpret_cast<const uint32_t*>(b); };
    auto rays_of = [](const void* b) {
        return reinterpret_cast<const sdfv_ray_state*>(static_cast<const char*>(b) + SDFV_RAY_BUFFER_HEADER_BYTES);
    };
    // this round's outgoing lists start empty: their headers are cleared on the stream, ahead of the kernel
    SDFV_HIP(hipMemsetAsync(out_down, 0, SDFV_RAY_BUFFER_HEADER_BYTES, (hipStream_t)stream));
    SDFV_HIP(hipMemsetAsync(out_up, 0, SDFV_RAY_BUFFER_HEADER_BYTES, (hipStream_t)stream));
    if (!first_round) {
        if (!in_lo && !in_hi) return SDFV_OK;  // a rank without neighbours has nothing to continue
        s.in_count[0] = in_lo ? count_of(in_lo) : nullptr;
        s.in_rays[0] = in_lo ? rays_of(in_lo) : nullptr;
        s.in_count[1] = in_hi ? count_of(in_hi) : nullptr;
        s.in_rays[1] = in_hi ? rays_of(in_hi) : nullptr;
        // every pixel's ray is in exactly one place, so the two lists together hold at most width * height rays
        const uint64_t most = (uint64_t)capacity * ((in_lo ? 1u : 0u) + (in_hi ? 1u : 0u));
        const uint64_t pixels = (uint64_t)width * height;
        s.max_in = (uint32_t)(most < pixels ? most : pixels);
        if (s.max_in == 0) return SDFV_OK;
    }
    s.out_down = const_cast<sdfv_ray_state*>(rays_of(out_down));
    s.out_up = const_cast<sdfv_ray_state*>(rays_of(out_up));
    s.count_down = reinterpret_cast<uint32_t*>(out_down);
    s.count_up = reinterpret_cast<uint32_t*>(out_up);
    s.overflow = overflow;
    s.leftover = leftover;
    s.capacity = capacity;
    SDFV_HIP_RETURN(sdfv::launch_raymarch_slab(a, s, (hipStream_t)stream));
}

}  // extern "C"
#pragma GCC visibility pop
