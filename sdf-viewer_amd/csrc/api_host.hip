// api_host.hip -- the *_host conveniences: host buffers up, the stream form on the null stream, results down.
#include <cstring>

#include "api_internal.h"

using namespace sdfv;

namespace {

// Per-point callers (the reference's ffi.rs ABI: one sample() per call) would otherwise pay two hipMalloc/hipFree per
// point.  Small requests of the *_host conveniences run through a per-thread staging area instead: a device block
// and a pinned host block allocated once, asynchronous copies on the null stream, one synchronisation.
struct SmallStage {
    static constexpr size_t kBytes = 64 << 10;  // in + out of up to 1024 points
    char* dev = nullptr;
    char* host = nullptr;
    int device = -1;
    bool ensure() {
        const int now = current_device();
        if (dev && device != now) {  // the staging block lives on another GPU than the one this call runs on
            (void)hipFree(dev);
            dev = nullptr;
        }
        device = now;
        if (dev && host) return true;
        if (!dev && hipMalloc((void**)&dev, kBytes) != hipSuccess) dev = nullptr;
        if (!host && hipHostMalloc((void**)&host, kBytes, hipHostMallocDefault) != hipSuccess) host = nullptr;
        return dev && host;
    }
};
thread_local SmallStage g_stage;  // never freed: lives as long as the thread's device context

struct DeviceBuf {
    void* p = nullptr;
    ~DeviceBuf() {
        if (p) (void)hipFree(p);
    }
};

// One host buffer of a round trip: copied up before the work, down after it, or both; host == NULL: left out, the work sees NULL.
enum : uint32_t { kUp = 1, kDown = 2 };
struct HostBuf {
    const void* host;
    size_t bytes;
    uint32_t dir;
};

// Runs `enqueue(dev)` over device copies dev[i] of the host buffers b[i].  Temporary device buffers and synchronous copies; with
// `may_stage`, requests that fit the per-thread staging area (every buffer on a 256-byte boundary of it) go through that instead.
template <size_t N, typename Enqueue>
int run_over_host_buffers(const HostBuf (&b)[N], bool may_stage, Enqueue enqueue) {
    void* dev[N] = {};
    size_t at[N], end = 0;
    for (size_t i = 0; i < N; ++i) {
        at[i] = (end + 255) & ~(size_t)255;
        end = at[i] + b[i].bytes;
    }
    if (may_stage && end <= SmallStage::kBytes && g_stage.ensure()) {
        for (size_t i = 0; i < N; ++i) {
            dev[i] = g_stage.dev + at[i];
            if (!(b[i].dir & kUp)) continue;
            memcpy(g_stage.host + at[i], b[i].host, b[i].bytes);
            SDFV_HIP(hipMemcpyAsync(dev[i], g_stage.host + at[i], b[i].bytes, hipMemcpyHostToDevice, nullptr));
        }
        if (int rc = enqueue(dev)) return rc;
        for (size_t i = 0; i < N; ++i)
            if (b[i].dir & kDown) SDFV_HIP(hipMemcpyAsync(g_stage.host + at[i], dev[i], b[i].bytes, hipMemcpyDeviceToHost, nullptr));
        SDFV_HIP(hipStreamSynchronize(nullptr));
        for (size_t i = 0; i < N; ++i)
            if (b[i].dir & kDown) memcpy(const_cast<void*>(b[i].host), g_stage.host + at[i], b[i].bytes);
        return SDFV_OK;
    }
    DeviceBuf own[N];
    for (size_t i = 0; i < N; ++i) {
        if (!b[i].host) continue;
        SDFV_HIP(hipMalloc(&own[i].p, b[i].bytes));
        dev[i] = own[i].p;
    }
    for (size_t i = 0; i < N; ++i)
        if (dev[i] && (b[i].dir & kUp)) SDFV_HIP(hipMemcpy(dev[i], b[i].host, b[i].bytes, hipMemcpyHostToDevice));
    if (int rc = enqueue(dev)) return rc;
    for (size_t i = 0; i < N; ++i)
        if (dev[i] && (b[i].dir & kDown)) SDFV_HIP(hipMemcpy(const_cast<void*>(b[i].host), dev[i], b[i].bytes, hipMemcpyDeviceToHost));
    return SDFV_OK;
}

}  // namespace

#pragma GCC visibility push(default)
extern "C" {

int sdfv_fill_grid_host(const sdfv_demo_params* params, uint32_t sdf_id, const sdfv_grid* grid, float* tex0_host,
                        float* tex1_host) {
    if (int rc = check_grid(grid)) return rc;
    if (int rc = need_textures(tex0_host, tex1_host)) return rc;
    if (int rc = need_device()) return rc;
    const size_t bytes = (size_t)slab_voxels(grid) * 16;
    if (bytes == 0) return SDFV_OK;
    const HostBuf b[] = {{tex0_host, bytes, kDown}, {tex1_host, bytes, kDown}};
    return run_over_host_buffers(b, false, [&](void* const* d) {
        return sdfv_fill_grid(params, sdf_id, grid, (float*)d[0], (float*)d[1], nullptr);
    });
}

int sdfv_sample_points_host(const sdfv_demo_params* params, uint32_t sdf_id, const float* points_host, size_t n,
                            int distance_only, sdfv_sample* out_host) {
    if (int rc = check_point_buffers(points_host, out_host, n)) return rc;
    if (int rc = check_params(params, sdf_id)) return rc;
    if (int rc = need_device()) return rc;
    if (n == 0) return SDFV_OK;
    const HostBuf b[] = {{points_host, n * 12, kUp}, {out_host, n * sizeof(sdfv_sample), kDown}};
    return run_over_host_buffers(b, true, [&](void* const* d) {
        return sdfv_sample_points(params, sdf_id, (const float*)d[0], n, distance_only, (sdfv_sample*)d[1], nullptr);
    });
}

int sdfv_normal_points_host(const sdfv_demo_params* params, uint32_t sdf_id, const float* points_host, size_t n,
                            float eps, int use_default, float* out_host) {
    if (int rc = check_point_buffers(points_host, out_host, n)) return rc;
    if (int rc = check_params(params, sdf_id)) return rc;
    if (int rc = need_device()) return rc;
    if (n == 0) return SDFV_OK;
    const HostBuf b[] = {{points_host, n * 12, kUp}, {out_host, n * 12, kDown}};
    return run_over_host_buffers(b, true, [&](void* const* d) {
        return sdfv_normal_points(params, sdf_id, (const float*)d[0], n, eps, use_default, (float*)d[1], nullptr);
    });
}

int sdfv_mesh_postproc_host(const sdfv_demo_params* params, uint32_t sdf_id, sdfv_vertex* vertices_host, size_t n) {
    if (int rc = check_point_buffers(vertices_host, vertices_host, n)) return rc;
    if (int rc = check_params(params, sdf_id)) return rc;
    if (int rc = need_device()) return rc;
    if (n == 0) return SDFV_OK;
    const HostBuf b[] = {{vertices_host, n * sizeof(sdfv_vertex), kUp | kDown}};
    return run_over_host_buffers(b, false, [&](void* const* d) {
        return sdfv_mesh_postproc(params, sdf_id, (sdfv_vertex*)d[0], n, nullptr);
    });
}

int sdfv_raymarch_host(const sdfv_render_params* rp, const float* tex0_host, const float* tex1_host,
                       const sdfv_camera* cameras, uint32_t n_cameras, uint32_t width, uint32_t height,
                       float* rgba_host, sdfv_march_aux* aux_host) {
    if (!rp || !tex0_host || !tex1_host || !rgba_host) return set_error(SDFV_ERR_INVALID_ARGUMENT, "NULL argument");
    if (int rc = need_device()) return rc;
    const size_t tex_bytes = (size_t)rp->tex_size[0] * rp->tex_size[1] * rp->tex_size[2] * 16;
    const size_t px = (size_t)n_cameras * width * height;
    if (tex_bytes == 0 || px == 0) return SDFV_OK;
    const HostBuf b[] = {{tex0_host, tex_bytes, kUp}, {tex1_host, tex_bytes, kUp}, {rgba_host, px * 16, kDown},
                         {aux_host, px * sizeof(sdfv_march_aux), kDown}};
    return run_over_host_buffers(b, false, [&](void* const* d) {
        return sdfv_raymarch(rp, (const float*)d[0], (const float*)d[1], cameras, n_cameras, width, height, 0, height, (float*)d[2],
                             (sdfv_march_aux*)d[3], nullptr);
    });
}

int sdfv_program_sample_points_host(const sdfv_program* p, const float* points_host, size_t n, int distance_only,
                                    sdfv_sample* out_host) {
    if (!p) return set_error(SDFV_ERR_INVALID_ARGUMENT, "program is NULL");
    if (int rc = check_point_buffers(points_host, out_host, n)) return rc;
    if (int rc = need_device()) return rc;
    if (n == 0) return SDFV_OK;
    const HostBuf b[] = {{points_host, n * 12, kUp}, {out_host, n * sizeof(sdfv_sample), kDown}};
    return run_over_host_buffers(b, true, [&](void* const* d) {
        return sdfv_program_sample_points(p, (const float*)d[0], n, distance_only, (sdfv_sample*)d[1], nullptr);
    });
}

int sdfv_program_mesh_postproc_host(const sdfv_program* p, sdfv_vertex* vertices_host, size_t n) {
    if (!p) return set_error(SDFV_ERR_INVALID_ARGUMENT, "program is NULL");
    if (int rc = check_point_buffers(vertices_host, vertices_host, n)) return rc;
    if (int rc = need_device()) return rc;
    if (n == 0) return SDFV_OK;
    const HostBuf b[] = {{vertices_host, n * sizeof(sdfv_vertex), kUp | kDown}};
    return run_over_host_buffers(b, false, [&](void* const* d) {
        return sdfv_program_mesh_postproc(p, (sdfv_vertex*)d[0], n, nullptr);
    });
}

}  // extern "C"
#pragma GCC visibility pop
