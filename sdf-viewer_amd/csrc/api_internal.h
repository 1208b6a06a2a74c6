// api_internal.h -- shared by the translation units behind include/sdfgrid.h (not part of the ABI).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <string>

#include "../../include/sdfgrid.h"

namespace sdfv {
// The calling thread's options (sdfv_set_option); every entry point copies what it needs once per call.
struct Options {
    uint32_t fill_nontemporal = 0;   // 0 auto (nt when the launch also writes the distance volume), 1 always, 2 never
    uint32_t fill_form = 0;          // 0 auto, 1 rows, 2 flat
    uint32_t raymarch_disable = 0;   // SDFV_RM_NO_*
    uint32_t raymarch_keep_normal = 0;
    uint32_t raymarch_lod_filter = 0;  // 0 sdfSampleRawNearest, 1 the lattice filter (launches with lod_dist_between_samples != 1 only)
    uint32_t raymarch_batch_streams = 1;  // batches of several SMALL launches overlap on side streams
    uint32_t raymarch_camera_staging = 1;  // host arrays of more than kInlineCameras cameras are copied to stream-ordered device memory
    uint32_t raymarch_box_first = 1;   // single frames: groups under the projected bounding box are launched first
    uint32_t raymarch_waves_per_simd = 0;  // 0 = no cap
    uint32_t raymarch_tile_group = 0;  // 0 auto, 1 launch order, v >= 2: XCD-aware order over groups of 2^(v-1) x 2^(v-1) tiles
    uint32_t slab_step_form = 0;     // 0 auto, SDFV_STEP_* otherwise
    uint32_t ext_srgb_quant = 0;     // Srgba::from(Vec3): 0 truncate (default), 1 round
    uint32_t pass_form = 0;          // 0 auto, 1 = unflagged passes take the per-voxel kernels only
    uint32_t pass_loads = 0;         // 0 auto (SDFV_PASS_EXPECT_NOOP decides), 1 cached loads, 2 nontemporal loads for update_required
    unsigned long long pass_index_limit = 0;  // 0 = 2^32: voxels per piece of a pass over a slab too large for 32-bit indices
    unsigned long long wave_timing = 0;  // tuning build only
    unsigned long long priority_map = 0;  // tuning build only
    unsigned long long tile_order = 0;    // tuning build only
};
// One definition each (api_common.hip), hidden like everything that is not the ABI: the calling thread's last message and options.
extern thread_local char g_err[512];
extern thread_local Options g_options;
inline const Options& options() { return g_options; }
// SDFV_OPT_RCCL_LIBRARY: process-wide path of the RCCL-ABI library the communicator loads (empty = librccl.so.1 by name)
// (claim_rccl_library_path: the path, and from that moment on SDFV_OPT_RCCL_LIBRARY is refused -- one RCCL per process)
std::string rccl_library_path_copy();
const char* claim_rccl_library_path();
// SDFV_OPT_HIPRTC_LIBRARY, by the same rules: the run-time compiler library sdfv_program_compile loads (empty = libhiprtc.so by name)
std::string hiprtc_library_path_copy();
const char* claim_hiprtc_library_path();
// Formats the thread-local message sdfv_last_error() returns and hands `code` back.
int set_error(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
int hip_fail(hipError_t e, const char* what);  // SDFV_ERR_NO_DEVICE or SDFV_ERR_HIP, with HIP's text
#define SDFV_HIP(call)                                          \
    do {                                                        \
        hipError_t e_ = (call);                                 \
        if (e_ != hipSuccess) return sdfv::hip_fail(e_, #call); \
    } while (0)
#define SDFV_HIP_RETURN(call) return sdfv::hip_status((call), #call)  // the entry point's last call: its status is the answer
inline int hip_status(hipError_t e, const char* what) { return e == hipSuccess ? SDFV_OK : hip_fail(e, what); }

// ---- the check vocabulary: one body and one message per rule; tests/golden/api_errors.json pins each entry point's order.
int check_params(const sdfv_demo_params* p, uint32_t sdf_id);
int check_grid(const sdfv_grid* g);
int check_lights(const sdfv_render_params* rp);  // only ambient entries can be rendered
int need_device();
inline int need_textures(const void* tex0, const void* tex1) {
    return tex0 && tex1 ? SDFV_OK : set_error(SDFV_ERR_INVALID_ARGUMENT, "texture pointer is NULL");
}
// Every entry point that reinterprets a float* as float4* (dwordx4 loads and stores) checks this first: a misaligned
// caller buffer is an argument error, not a GPU fault.
template <typename... P>
int check_texel_alignment(const P*... p) {
    return ((... | (uintptr_t)p) & 15) ? set_error(SDFV_ERR_INVALID_ARGUMENT, "texel buffers (tex0, tex1, rgba) must be 16-byte aligned") : SDFV_OK;
}
inline int check_textures(const void* tex0, const void* tex1) {
    const int rc = need_textures(tex0, tex1);
    return rc ? rc : check_texel_alignment(tex0, tex1);
}
// `names` is how the message calls the pointers: "dist", "points and out", ...
template <typename... P>
int check_word_aligned(const char* names, const P*... p) {
    return ((... | (uintptr_t)p) & 3) ? set_error(SDFV_ERR_INVALID_ARGUMENT, "%s must be 4-byte aligned", names) : SDFV_OK;
}
// SDFV_PASS_VOLUME_INTERLEAVED: the flag needs a volume whose rows pair up.
inline int check_interleaved_volume(const sdfv_grid* grid, const float* dist, uint32_t flags) {
    if (!(flags & SDFV_PASS_VOLUME_INTERLEAVED)) return SDFV_OK;
    if (!dist) return set_error(SDFV_ERR_INVALID_ARGUMENT, "SDFV_PASS_VOLUME_INTERLEAVED without a volume");
    if ((grid->dims[1] & 1u) || ((uintptr_t)dist & 7))
        return set_error(SDFV_ERR_INVALID_ARGUMENT, "the interleaved volume pairs rows: H = %u must be even and the volume 8-byte aligned", grid->dims[1]);
    return SDFV_OK;
}
// A dense fill's argument block (FillArgs, ProgramFillArgs): rows and row length fit the launch's 31-bit indices.
template <typename Args>
int check_one_launch(const Args& a) {
    if ((uint64_t)a.H * a.slab_d > 0x7fffffffull || a.W > 0x7fffffffu)
        return set_error(SDFV_ERR_INVALID_ARGUMENT, "slab of %u x %u rows is too large for one launch", a.H, a.slab_d);
    return SDFV_OK;
}
inline int check_point_buffers(const void* points, const void* out, size_t n) {
    return n && (!points || !out) ? set_error(SDFV_ERR_INVALID_ARGUMENT, "NULL buffer") : SDFV_OK;
}
inline int check_mesher(uint32_t algorithm, uint32_t max_voxels_per_axis) {
    if (algorithm != SDFV_MESHER_MARCHING_CUBES && algorithm != SDFV_MESHER_DUAL_CONTOURING_PARTICLE)
        return set_error(SDFV_ERR_INVALID_ARGUMENT, "Unsupported algorithm %u", algorithm);  // isosurface.rs:49
    if (max_voxels_per_axis < 1 || max_voxels_per_axis > 1024)
        return set_error(SDFV_ERR_INVALID_ARGUMENT, "max_voxels_per_axis %u is outside [1, 1024]", max_voxels_per_axis);
    return SDFV_OK;
}
inline uint64_t slab_voxels(const sdfv_grid* g) { return (uint64_t)g->dims[0] * g->dims[1] * (g->z_end - g->z_begin); }
// A size-prefixed descriptor: read what the caller's header knew, take the rest as 0 / NULL (a binder built against an older
// header).  A NEWER caller's descriptor: fields this library does not know may only be zero (0 / NULL = "not used" by the
// descriptors' rule); anything else would be dropped silently.  The caller checks `reserved` next.
template <typename Desc>
int read_sized_desc(const Desc* desc, size_t first_version_bytes, const char* type, Desc& d) {
    if (!desc) return set_error(SDFV_ERR_INVALID_ARGUMENT, "desc is NULL");
    if (desc->size < first_version_bytes)
        return set_error(SDFV_ERR_INVALID_ARGUMENT, "%s.size = %u is smaller than the descriptor's first version (%zu)", type, desc->size,
                    first_version_bytes);
    memset(&d, 0, sizeof(d));
    memcpy(&d, desc, desc->size < sizeof(d) ? desc->size : sizeof(d));
    for (uint32_t i = (uint32_t)sizeof(d); i < desc->size; ++i)
        if (reinterpret_cast<const unsigned char*>(desc)[i] != 0)
            return set_error(SDFV_ERR_INVALID_ARGUMENT, "%s.size = %u: this library knows %zu bytes and byte %u beyond them is not 0", type,
                        desc->size, sizeof(d), i);
    return SDFV_OK;
}

// The four output planes of an argument block (RaymarchArgs, ProgramMarchArgs) at camera c0 of the caller's.
template <typename Args>
void point_outputs_at(Args& a, uint64_t pixels_per_cam, uint32_t c0, float* rgba, uint32_t* rgba8, sdfv_march_aux* aux, float* depth) {
    a.rgba = rgba ? reinterpret_cast<float4*>(rgba) + c0 * pixels_per_cam : nullptr;
    a.rgba8 = rgba8 ? rgba8 + c0 * pixels_per_cam : nullptr;
    a.aux = aux ? aux + c0 * pixels_per_cam : nullptr;
    a.depth = depth ? depth + c0 * pixels_per_cam : nullptr;
}
inline float air_dist() {
    volatile float a = 1e-1f, b = 0.001234f;  // scene/sdf/mod.rs:42, f32 const evaluation
    return a + b;
}

// The per-thread device caches (mesh scratch, batch streams, camera ring, staging block) belong to the HIP device that was
// current when they were made: each records its owner and is released and re-made when the thread calls in with another.
int current_device();  // -1: none
void release_march_caches();  // the batch streams and the camera ring of the calling thread (sdfv_mesh_trim)
// What the raymarch launcher needs to know about the device it launches on (cached per host thread and device): the
// hand-written march loop is gfx950 machine code, the XCD-aware tile order assumes workgroup L -> XCD L % xcds, and the
// occupancy rule counts wave slots.
struct DeviceFacts {
    int device = -2;
    bool gfx950 = false;
    uint32_t cus = 0, xcds = 0;
    uint64_t last_level_cache_bytes = 0;
};
const DeviceFacts& device_facts();
// An SDF program's instructions on the current device (copied there on the first use), their count and, if asked for, its box.
int program_on_device(const sdfv_program* p, const sdfv_prog_op** ops, uint32_t* n_ops, const float** bb = nullptr);
// The specialised kernels a handle has for `route` (one SDFV_COMPILE_* bit) on the current device, for the launchers of
// program_kernels.h / program_march_kernels.h: *k stays empty for a plain handle and for a route that was not compiled (the
// launcher then interprets).  A compiled route on a device of another architecture is SDFV_ERR_INVALID_ARGUMENT, decided
// before anything is loaded; the first use on a device loads the code object (synchronously).  Needs a current device.
struct ProgramKernels;
int program_compiled_kernels(const sdfv_program* p, uint32_t route, ProgramKernels* k);
void program_release_compiled(sdfv_program* p);  // sdfv_program_free's share: the modules and the code
// Dense fill of `slab` in boundary-first workgroup order (fill_kernels.h): the `lead` first slices and the last one come
// first, optionally copied into the packed staging buffers.
struct OrderedFill {
    uint32_t lead = 1;
    bool stage_only = false;  // write the packed copies only (the textures are another launch's)
    float* dist = nullptr;    // compact distance volume of the owned slices (fused commit), or nullptr
    float* stage_lo = nullptr;
    float* stage_hi = nullptr;
};
// Workgroups per slice and in total of that order for this slab; per_slice = 0: the shape does not allow it.
int ordered_fill_blocks(const sdfv_grid* slab, uint32_t* per_slice, uint32_t* total);
// Logical workgroups [block_begin, block_end) of the ordered fill; o0/o1 address the first owned slice.
int fill_slab_ordered(const sdfv_demo_params* params, uint32_t sdf_id, const sdfv_grid* slab, float* o0, float* o1,
                      const OrderedFill& of, uint32_t block_begin, uint32_t block_end, void* stream);
// dst[i] = src[i] over up to four segments of `n` 16-byte texels (ghost slices out of the packed receive buffers).
// r_out (or its entries) may be NULL; r_out[i] receives the first component of segment i's texels as a compact array
int copy_texel_segments(const float* const src[4], float* const dst[4], const size_t n[4], float* const r_out[4],
                        void* stream);
// sdfv_fill_grid whose first workgroup stores `value` to `signal` (signal memory) as soon as the launch starts.
int fill_grid_signalling_start(const sdfv_demo_params* params, uint32_t sdf_id, const sdfv_grid* grid, float* tex0,
                               float* tex1, float* dist, uint32_t* signal, uint32_t value, void* stream);
// dist[i] = tex0[i].r over n texels (the ghost slices' share of the compact distance volume)
int extract_distance(const float* tex0, float* dist, size_t n, void* stream);
}  // namespace sdfv

// sdfv_raymarch_slab_round with a counter of the rays the round hands on (`leftover`, DEVICE or NULL): sdfv_slab_march passes
// it in its last round, after which no ray may be in flight.  Not part of the ABI (hidden).
extern "C" __attribute__((visibility("hidden"))) int sdfv_internal_raymarch_slab_round(
    const sdfv_render_params* rp, const sdfv_grid* slab, uint32_t ghost_lo, uint32_t ghost_hi, const float* tex0, const float* tex1,
    const sdfv_camera* camera, uint32_t width, uint32_t height, const void* in_lo, const void* in_hi, int first_round, float* rgba,
    sdfv_march_aux* aux, void* out_down, void* out_up, uint32_t capacity, uint32_t* overflow, uint32_t* leftover, void* stream);
