// api_common.hip -- what every entry point of include/sdfgrid.h rests on: the error state, the options, the device.
#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>

#include "api_internal.h"

namespace sdfv {
thread_local char g_err[512] = "";
thread_local Options g_options;

int set_error(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

int hip_fail(hipError_t e, const char* what) {
    if (e == hipErrorNoDevice || e == hipErrorInvalidDevice)
        return set_error(SDFV_ERR_NO_DEVICE, "%s: no HIP device (%s)", what, hipGetErrorString(e));
    return set_error(SDFV_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
}

int check_params(const sdfv_demo_params* p, uint32_t sdf_id) {
    if (!p) return set_error(SDFV_ERR_INVALID_ARGUMENT, "params is NULL");
    if (sdf_id > SDFV_SDF_SPHERE) {
        fprintf(stderr, "Failed to find SDF with ID %u\n", sdf_id);  // ffi.rs:47
        return set_error(SDFV_ERR_UNKNOWN_SDF, "Failed to find SDF with ID %u", sdf_id);
    }
    if (p->cube_material > SDFV_MATERIAL_NORMAL || p->sphere_material > SDFV_MATERIAL_NORMAL)
        return set_error(SDFV_ERR_INVALID_ARGUMENT, "Invalid cube material");  // cube.rs:33
    return SDFV_OK;
}

int check_grid(const sdfv_grid* g) {
    if (!g) return set_error(SDFV_ERR_INVALID_ARGUMENT, "grid is NULL");
    if (g->z_begin > g->z_end || g->z_end > g->dims[2])
        return set_error(SDFV_ERR_INVALID_ARGUMENT, "slab [%u,%u) outside depth %u", g->z_begin, g->z_end, g->dims[2]);
    return SDFV_OK;
}

int need_device() {
    static int cached = 0;  // only a positive answer is cached
    if (cached > 0 || (cached = sdfv_device_count()) > 0) return SDFV_OK;
    return set_error(SDFV_ERR_NO_DEVICE, "no HIP device visible: libsdfgrid has no CPU path");
}

int current_device() {
    int d = -1;
    if (hipGetDevice(&d) != hipSuccess) {
        (void)hipGetLastError();
        return -1;
    }
    return d;
}

const DeviceFacts& device_facts() {
    thread_local DeviceFacts f;
    const int now = current_device();
    if (f.device == now) return f;
    f = DeviceFacts();
    f.device = now;
    hipDeviceProp_t prop;
    if (now >= 0 && hipGetDeviceProperties(&prop, now) == hipSuccess) {
        f.gfx950 = strncmp(prop.gcnArchName, "gfx950", 6) == 0;
        f.cus = prop.multiProcessorCount > 0 ? (uint32_t)prop.multiProcessorCount : 0u;
        int x = 0;
        if (hipDeviceGetAttribute(&x, hipDeviceAttributeNumberOfXccs, now) == hipSuccess && x > 0) f.xcds = (uint32_t)x;
        // MI355X: 256 MB of Infinity Cache behind the eight 4 MB L2s (MI355X_MICROARCH.md); HIP reports the L2 only
        f.last_level_cache_bytes = f.gfx950 ? (256ull << 20) : (uint64_t)(prop.l2CacheSize > 0 ? prop.l2CacheSize : 0);
    } else {
        (void)hipGetLastError();
    }
    return f;
}

namespace {
std::mutex g_rccl_path_mutex;
std::string g_rccl_path;         // SDFV_OPT_RCCL_LIBRARY (process-wide: RCCL is loaded once per process)
std::atomic<bool> g_rccl_loaded{false};
}  // namespace
std::string rccl_library_path_copy() {
    std::lock_guard<std::mutex> lock(g_rccl_path_mutex);
    return g_rccl_path;
}
const char* claim_rccl_library_path() {
    std::lock_guard<std::mutex> lock(g_rccl_path_mutex);
    g_rccl_loaded.store(true);
    return g_rccl_path.c_str();
}
static bool set_rccl_library_path(const char* path) {
    std::lock_guard<std::mutex> lock(g_rccl_path_mutex);
    if (g_rccl_loaded.load()) return false;  // (decided under the same lock the loader claims the path under)
    g_rccl_path = path ? path : "";
    return true;
}
namespace {
std::mutex g_hiprtc_path_mutex;
std::string g_hiprtc_path;  // SDFV_OPT_HIPRTC_LIBRARY (process-wide: the run-time compiler is loaded once per process)
bool g_hiprtc_loaded = false;
}  // namespace
std::string hiprtc_library_path_copy() {
    std::lock_guard<std::mutex> lock(g_hiprtc_path_mutex);
    return g_hiprtc_path;
}
const char* claim_hiprtc_library_path() {
    std::lock_guard<std::mutex> lock(g_hiprtc_path_mutex);
    g_hiprtc_loaded = true;
    return g_hiprtc_path.c_str();
}
static bool set_hiprtc_library_path(const char* path) {
    std::lock_guard<std::mutex> lock(g_hiprtc_path_mutex);
    if (g_hiprtc_loaded) return false;
    g_hiprtc_path = path ? path : "";
    return true;
}
}  // namespace sdfv

using namespace sdfv;
#pragma GCC visibility push(default)
extern "C" {

uint32_t sdfv_abi_version(void) { return SDFV_ABI_VERSION; }

const char* sdfv_last_error(void) { return g_err; }

#ifndef SDFV_BUILD_ID
#define SDFV_BUILD_ID "unknown"
#endif
const char* sdfv_build_id(void) { return SDFV_BUILD_ID; }

int sdfv_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return n;
}

float sdfv_air_dist(void) { return air_dist(); }

// The options that are a number up to a largest value; the others have rules of their own below.
static const struct { uint32_t option; uint32_t Options::*member; uint32_t max; } kPlainOptions[] = {
    {SDFV_OPT_FILL_NONTEMPORAL, &Options::fill_nontemporal, 2},   {SDFV_OPT_FILL_FORM, &Options::fill_form, 4},
    {SDFV_OPT_RAYMARCH_TILE_GROUP, &Options::raymarch_tile_group, 5}, {SDFV_OPT_RAYMARCH_BOX_FIRST, &Options::raymarch_box_first, 1},
    {SDFV_OPT_RAYMARCH_BATCH_STREAMS, &Options::raymarch_batch_streams, 1},
    {SDFV_OPT_RAYMARCH_CAMERA_STAGING, &Options::raymarch_camera_staging, 1},
    {SDFV_OPT_EXT_SRGB_QUANT, &Options::ext_srgb_quant, 1},       {SDFV_OPT_PASS_FORM, &Options::pass_form, 1},
    {SDFV_OPT_PASS_LOADS, &Options::pass_loads, 2},                {SDFV_OPT_RAYMARCH_KEEP_NORMAL, &Options::raymarch_keep_normal, 1},
    {SDFV_OPT_RAYMARCH_LOD_FILTER, &Options::raymarch_lod_filter, 1},
    {SDFV_OPT_RAYMARCH_DISABLE, &Options::raymarch_disable,  // a mask: the six flags are bits 0..5, so no other bit = at most their sum
     SDFV_RM_NO_FAST_INDEX | SDFV_RM_NO_POW2_EXTENT | SDFV_RM_NO_POW2_SIZE | SDFV_RM_NO_SYMMETRIC | SDFV_RM_NO_ASM_LOOP | SDFV_RM_NO_INTERIOR_FETCH},
};

int sdfv_set_option(uint32_t option, uint64_t value) {
    auto out_of_range = [&] {
        return set_error(SDFV_ERR_INVALID_ARGUMENT, "value %llu is out of range for option %u", (unsigned long long)value, option);
    };
    for (const auto& o : kPlainOptions) {
        if (o.option != option) continue;
        if (value > o.max) return out_of_range();
        g_options.*o.member = (uint32_t)value;
        return SDFV_OK;
    }
    switch (option) {
        case SDFV_OPT_SLAB_STEP_FORM: {
            const uint64_t form = value & ~(uint64_t)(SDFV_STEP_UNPACKED | SDFV_STEP_START_EVENT | SDFV_STEP_DEFER_JOIN);
            if (form != 0 && form != SDFV_STEP_SIDE_BOUNDARY) break;
            g_options.slab_step_form = (uint32_t)value;
            return SDFV_OK;
        }
        case SDFV_OPT_PASS_INDEX_LIMIT:
            if (value != 0 && (value < 2 || value > (1ull << 32))) break;
            g_options.pass_index_limit = value;
            return SDFV_OK;
        case SDFV_OPT_RCCL_LIBRARY: {
            // value = address of a NUL-terminated path (copied), or 0 = librccl.so.1 by name; process-wide, before the first
            // communicator -- RCCL is loaded once
            const char* path = reinterpret_cast<const char*>((uintptr_t)value);
            if (path && strnlen(path, 4096) >= 4096) break;
            if (!sdfv::set_rccl_library_path(path))
                return set_error(SDFV_ERR_INVALID_ARGUMENT, "SDFV_OPT_RCCL_LIBRARY: RCCL has already been loaded in this process");
            return SDFV_OK;
        }
        case SDFV_OPT_HIPRTC_LIBRARY: {  // the same rules for the run-time compiler library of sdfv_program_compile
            const char* path = reinterpret_cast<const char*>((uintptr_t)value);
            if (path && strnlen(path, 4096) >= 4096) break;
            if (!sdfv::set_hiprtc_library_path(path))
                return set_error(SDFV_ERR_INVALID_ARGUMENT, "SDFV_OPT_HIPRTC_LIBRARY: the run-time compiler has already been loaded in this process");
            return SDFV_OK;
        }
        case SDFV_OPT_RAYMARCH_WAVES_PER_SIMD:
            if (value == 1 || value > 7) break;  // 0 auto (the launcher's rule) | 2..6 cap | 7 never cap
            g_options.raymarch_waves_per_simd = (uint32_t)value;
            return SDFV_OK;
        case SDFV_OPT_TUNING_TILE_ORDER: case SDFV_OPT_TUNING_PRIORITY_MAP: case SDFV_OPT_TUNING_WAVE_TIMING: {
#ifdef SDFV_TUNING
            (option == SDFV_OPT_TUNING_TILE_ORDER ? g_options.tile_order
             : option == SDFV_OPT_TUNING_PRIORITY_MAP ? g_options.priority_map : g_options.wave_timing) = value;
            return SDFV_OK;
#else
            const char* name = option == SDFV_OPT_TUNING_TILE_ORDER ? "TILE_ORDER" : option == SDFV_OPT_TUNING_PRIORITY_MAP ? "PRIORITY_MAP" : "WAVE_TIMING";
            return set_error(SDFV_ERR_INVALID_ARGUMENT, "SDFV_OPT_TUNING_%s needs the tuning build (make tuning)", name);
#endif
        }
        default:
            return set_error(SDFV_ERR_INVALID_ARGUMENT, "unknown option %u", option);
    }
    return out_of_range();
}

int sdfv_get_option(uint32_t option, uint64_t* value) {
    if (!value) return set_error(SDFV_ERR_INVALID_ARGUMENT, "value is NULL");
    for (const auto& o : kPlainOptions)
        if (o.option == option) {
            *value = g_options.*o.member;
            return SDFV_OK;
        }
    switch (option) {
        case SDFV_OPT_SLAB_STEP_FORM: *value = g_options.slab_step_form; return SDFV_OK;
        case SDFV_OPT_TUNING_WAVE_TIMING: *value = g_options.wave_timing; return SDFV_OK;
        case SDFV_OPT_TUNING_PRIORITY_MAP: *value = g_options.priority_map; return SDFV_OK;
        case SDFV_OPT_TUNING_TILE_ORDER: *value = g_options.tile_order; return SDFV_OK;
        case SDFV_OPT_RAYMARCH_WAVES_PER_SIMD: *value = g_options.raymarch_waves_per_simd; return SDFV_OK;
        case SDFV_OPT_PASS_INDEX_LIMIT: *value = g_options.pass_index_limit; return SDFV_OK;
        case SDFV_OPT_RCCL_LIBRARY: {  // address of a copy that belongs to the CALLING THREAD ("" = by name): valid until this
            thread_local std::string copy;  // thread asks again, whatever another thread sets meanwhile
            copy = sdfv::rccl_library_path_copy();
            *value = (uint64_t)(uintptr_t)copy.c_str();
            return SDFV_OK;
        }
        case SDFV_OPT_HIPRTC_LIBRARY: {  // likewise
            thread_local std::string copy;
            copy = sdfv::hiprtc_library_path_copy();
            *value = (uint64_t)(uintptr_t)copy.c_str();
            return SDFV_OK;
        }
        default: return set_error(SDFV_ERR_INVALID_ARGUMENT, "unknown option %u", option);
    }
}

void sdfv_demo_params_default(sdfv_demo_params* p) {
    if (!p) return;
    p->cube_half_side = 0.95f;                // cube.rs:17
    p->cube_material = SDFV_MATERIAL_BRICK;   // cube.rs:15
    p->sphere_radius = 1.05f;                 // sphere.rs:13
    p->sphere_material = SDFV_MATERIAL_NORMAL;  // sphere.rs:11
    p->max_distance_custom_material = 0.05f;  // demo/mod.rs:26
    p->disable_sphere = 0;                    // demo/mod.rs:28
}

int sdfv_grid_from_bb(const float bb_min[3], const float bb_max[3], uint32_t max_voxels_side, sdfv_grid* out) {
    if (!bb_min || !bb_max || !out) return set_error(SDFV_ERR_INVALID_ARGUMENT, "NULL argument");
    // scene/sdf/mod.rs:46-72: the longest axis gets max_voxels_side (ties: the LAST longest axis, as
    // Iterator::max_by), the others (N as f32 * size_i / size_max) as usize.
    float size[3] = {bb_max[0] - bb_min[0], bb_max[1] - bb_min[1], bb_max[2] - bb_min[2]};
    int max_dim = 0;
    for (int i = 1; i < 3; ++i)
        if (size[i] >= size[max_dim]) max_dim = i;
    for (int i = 0; i < 3; ++i) {
        if (i == max_dim) {
            out->dims[i] = max_voxels_side;
        } else {
            float v = (float)max_voxels_side * size[i] / size[max_dim];
            out->dims[i] = v > 0.0f ? (uint32_t)v : 0u;
        }
        out->bb_min[i] = bb_min[i];
        out->bb_max[i] = bb_max[i];
    }
    out->z_begin = 0;
    out->z_end = out->dims[2];
    return SDFV_OK;
}

int sdfv_camera_look_at(sdfv_camera* cam, const float eye[3], const float target[3], const float up[3],
                        float fovy_degrees, float aspect, float z_near, float z_far) {
    if (!cam || !eye || !target || !up) return set_error(SDFV_ERR_INVALID_ARGUMENT, "NULL argument");
    // cgmath look_at_rh: f = normalize(target - eye), s = normalize(f x up), u = s x f
    float f[3] = {target[0] - eye[0], target[1] - eye[1], target[2] - eye[2]};
    float fl = 1.0f / sqrtf(f[0] * f[0] + f[1] * f[1] + f[2] * f[2]);
    for (float& c : f) c *= fl;
    float s[3] = {f[1] * up[2] - f[2] * up[1], f[2] * up[0] - f[0] * up[2], f[0] * up[1] - f[1] * up[0]};
    float sl = 1.0f / sqrtf(s[0] * s[0] + s[1] * s[1] + s[2] * s[2]);
    for (float& c : s) c *= sl;
    float u[3] = {s[1] * f[2] - s[2] * f[1], s[2] * f[0] - s[0] * f[2], s[0] * f[1] - s[1] * f[0]};
    for (int i = 0; i < 3; ++i) {
        cam->eye[i] = eye[i];
        cam->right[i] = s[i];
        cam->up[i] = u[i];
        cam->forward[i] = f[i];
    }
    cam->tan_half_fovy = tanf(fovy_degrees * (3.14159265358979323846f / 180.0f) / 2.0f);
    cam->aspect = aspect;
    const float view[16] = {s[0], u[0], -f[0], 0.0f, s[1], u[1], -f[1], 0.0f, s[2], u[2], -f[2], 0.0f,
                            -(eye[0] * s[0] + eye[1] * s[1] + eye[2] * s[2]),
                            -(eye[0] * u[0] + eye[1] * u[1] + eye[2] * u[2]),
                            (eye[0] * f[0] + eye[1] * f[1] + eye[2] * f[2]), 1.0f};
    const float ct = 1.0f / cam->tan_half_fovy;
    const float proj[16] = {ct / aspect, 0, 0, 0, 0, ct, 0, 0,
                            0, 0, (z_far + z_near) / (z_near - z_far), -1.0f,
                            0, 0, (2.0f * z_far * z_near) / (z_near - z_far), 0};
    const float bias[16] = {0.5f, 0, 0, 0, 0, 0.5f, 0, 0, 0, 0, 0.5f, 0, 0.5f, 0.5f, 0.5f, 1.0f};  // material.rs:90-95
    auto multiply = [](const float* a, const float* b, float* out) {  // out = a * b, column-major
        for (int c = 0; c < 4; ++c)
            for (int r = 0; r < 4; ++r) {
                float acc = 0.0f;
                for (int k = 0; k < 4; ++k) acc += a[k * 4 + r] * b[c * 4 + k];
                out[c * 4 + r] = acc;
            }
    };
    float pv[16];
    multiply(proj, view, pv);
    multiply(bias, pv, cam->bvp);
    return SDFV_OK;
}

}  // extern "C"
#pragma GCC visibility pop
