// viewer_kernels.hip -- the update_required scan of SDFViewer::update for an SDF that the CALLER samples on the device
// (sdfv_surface.sample_batch_device, include/sdfviewer.h), and its two entry points of include/sdfgrid.h.
//
// The reference's loop (src/app/scene/sdf/mod.rs:173-215) takes the next LoadingManager index, computes the voxel's position,
// decides update_required and samples.  For a run [cursor, cursor + n) of one pass this file does the first three for every
// point of the run at once and writes out the points that need a sample, in LoadingManager order: their positions (what the
// caller's kernel samples) and their flat indices (what sdfv_pack_samples stores the samples through).
//   1. an ordered select (rocPRIM, decoupled look-back) over k in [0, n): the predicate decodes the lattice point from the
//      LoadingManager's closed form, reads the voxel's entry of the 4 B/voxel distance volume (texture order or
//      y-interleaved) and, with a changed box, computes its position with the reference's three roundings; the offsets k
//      it keeps go to `indices`;
//   2. one thread per kept point turns its k into the flat index and the position, in place.
// Traffic: 4 B read per visited voxel, 4 + 4 + 16 B moved per kept one -- a streaming scan.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_select.hpp>
#include <rocprim/iterator/counting_iterator.hpp>

#include <cstring>

#include "../../include/sdfgrid.h"
#include "api_internal.h"
#include "kernel_common.h"

namespace sdfv {

namespace {

struct EmitArgs {
    uint32_t W, H;       // grid dims (x, y): flat = (z * H + y) * W + x
    uint32_t step;       // lattice spacing of the pass
    uint32_t nx, ny;     // points per axis of the pass's walk (x fastest, then y, then z)
    uint32_t cursor;     // first point of the run within the pass
    uint32_t n;          // points of the run
    float dm1[3];        // (float)dim - 1.0f
    float bb_size[3];    // bb_max - bb_min
    float bb_min[3];
    uint32_t has_box;
    float box[6];        // changed_box: min.xyz, max.xyz
    const float* dist;   // the distance volume (tex0.r), texture order or y-interleaved
    uint32_t dist_ilv;
    float air_dist;
};

struct Lattice {
    uint32_t x, y, z;
};

// LoadingManager::lattice_point (host/loading_manager.hpp): x fastest, then y, then z
__device__ __forceinline__ Lattice lattice_point(const EmitArgs& a, uint32_t k) {
    const uint32_t c = a.cursor + k;
    const uint32_t kx = c % a.nx, r = c / a.nx;
    return {kx * a.step, (r % a.ny) * a.step, (r / a.ny) * a.step};
}

__device__ __forceinline__ uint32_t flat_index(const EmitArgs& a, Lattice p) { return (p.z * a.H + p.y) * a.W + p.x; }  // :177

struct UpdateRequired {
    EmitArgs a;
    __device__ bool operator()(uint32_t k) const {
        const Lattice p = lattice_point(a, k);
        uint32_t at = flat_index(a, p);
        if (a.dist_ilv) at = vol_index(1u, p.z * a.H + p.y, p.x, a.W);  // (32-bit: the grid holds at most 2^32 voxels)
        // Check if the update is required: was AIR on initial load, or has changed since.  (scene/sdf/mod.rs:184-190)
        bool required = a.dist[at] == a.air_dist;
        if (!required && a.has_box) {
            const float px = voxel_coord(p.x, a.dm1[0], a.bb_size[0], a.bb_min[0]);
            const float py = voxel_coord(p.y, a.dm1[1], a.bb_size[1], a.bb_min[1]);
            const float pz = voxel_coord(p.z, a.dm1[2], a.bb_size[2], a.bb_min[2]);
            required = px >= a.box[0] && px <= a.box[3] && py >= a.box[1] && py <= a.box[4] && pz >= a.box[2] && pz <= a.box[5];
        }
        return required;
    }
};

__global__ __launch_bounds__(kBlock) void emit_positions_kernel(EmitArgs a, float* points, uint32_t* indices, const uint32_t* count) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= a.n || i >= *count) return;
    const Lattice p = lattice_point(a, indices[i]);
    indices[i] = flat_index(a, p);
    points[3 * (size_t)i + 0] = voxel_coord(p.x, a.dm1[0], a.bb_size[0], a.bb_min[0]);  // :179-182
    points[3 * (size_t)i + 1] = voxel_coord(p.y, a.dm1[1], a.bb_size[1], a.bb_min[1]);
    points[3 * (size_t)i + 2] = voxel_coord(p.z, a.dm1[2], a.bb_size[2], a.bb_min[2]);
}

size_t select_scratch_bytes(uint32_t n) {
    size_t bytes = 0;
    if (rocprim::select(nullptr, bytes, rocprim::counting_iterator<uint32_t>(0), (uint32_t*)nullptr, (uint32_t*)nullptr,
                        (size_t)(n ? n : 1), UpdateRequired{}, (hipStream_t)0) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return bytes;
}

}  // namespace

}  // namespace sdfv

#pragma GCC visibility push(default)
extern "C" {

size_t sdfv_emit_update_points_scratch_bytes(uint64_t n) {
    return n > 0xffffffffull ? 0 : sdfv::select_scratch_bytes((uint32_t)n);
}

int sdfv_emit_update_points(const sdfv_grid* grid, uint32_t step, uint64_t cursor, uint64_t n, const float* changed_box,
                            const float* dist, uint32_t flags, float* points, uint32_t* indices, uint32_t* count, void* scratch,
                            size_t scratch_bytes, void* stream) {
    using sdfv::set_error;
    if (!grid) return set_error(SDFV_ERR_INVALID_ARGUMENT, "grid is NULL");
    const uint64_t W = grid->dims[0], H = grid->dims[1], D = grid->dims[2];
    if (grid->z_begin != 0 || grid->z_end != D) return set_error(SDFV_ERR_INVALID_ARGUMENT, "the scan runs over a whole grid, not a slab");
    if (W * H * D == 0 || W * H * D > 0x100000000ull)
        return set_error(SDFV_ERR_INVALID_ARGUMENT, "grid of %llu voxels: between 1 and 2^32 (32-bit flat indices)",
                         (unsigned long long)(W * H * D));
    if (step == 0 || (step & (step - 1))) return set_error(SDFV_ERR_INVALID_ARGUMENT, "step %u is not a power of two", step);
    const uint64_t nx = (W + step - 1) / step, ny = (H + step - 1) / step, nz = (D + step - 1) / step;
    if (cursor > nx * ny * nz || n > nx * ny * nz - cursor)
        return set_error(SDFV_ERR_INVALID_ARGUMENT, "run [%llu, %llu) beyond the pass's %llu points", (unsigned long long)cursor,
                         (unsigned long long)(cursor + n), (unsigned long long)(nx * ny * nz));
    if (n > 0xffffffffull)  // (the count, the offsets the select keeps and the launch are 32-bit)
        return set_error(SDFV_ERR_INVALID_ARGUMENT, "a run of %llu points: at most 2^32 - 1", (unsigned long long)n);
    if (flags & ~SDFV_PASS_VOLUME_INTERLEAVED) return set_error(SDFV_ERR_INVALID_ARGUMENT, "unknown flags 0x%x", flags);
    if (!count) return set_error(SDFV_ERR_INVALID_ARGUMENT, "count is NULL");
    if (n && (!dist || !points || !indices)) return set_error(SDFV_ERR_INVALID_ARGUMENT, "NULL buffer");
    if (((uintptr_t)dist | (uintptr_t)points | (uintptr_t)indices | (uintptr_t)count) & 3)
        return set_error(SDFV_ERR_INVALID_ARGUMENT, "dist, points, indices and count must be 4-byte aligned");
    if ((flags & SDFV_PASS_VOLUME_INTERLEAVED) && ((H & 1) || ((uintptr_t)dist & 7)))
        return set_error(SDFV_ERR_INVALID_ARGUMENT, "the interleaved volume pairs rows: H = %u must be even and the volume 8-byte aligned",
                         grid->dims[1]);
    const size_t need = sdfv::select_scratch_bytes((uint32_t)n);
    if (n && (!scratch || scratch_bytes < need))
        return set_error(SDFV_ERR_INVALID_ARGUMENT, "scratch of %zu bytes: the run needs %zu (sdfv_emit_update_points_scratch_bytes)",
                         scratch_bytes, need);
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev == 0) {
        (void)hipGetLastError();
        return set_error(SDFV_ERR_NO_DEVICE, "no HIP device visible: libsdfgrid has no CPU path");
    }
    const hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipSuccess;
    if (n == 0) {
        e = hipMemsetAsync(count, 0, sizeof(uint32_t), st);
    } else {
        sdfv::EmitArgs a;
        memset(&a, 0, sizeof(a));
        a.W = (uint32_t)W;
        a.H = (uint32_t)H;
        a.step = step;
        a.nx = (uint32_t)nx;
        a.ny = (uint32_t)ny;
        a.cursor = (uint32_t)cursor;
        a.n = (uint32_t)n;
        sdfv::set_voxel_coords(a, *grid);
        a.has_box = changed_box ? 1u : 0u;
        if (changed_box) memcpy(a.box, changed_box, sizeof(a.box));
        a.dist = dist;
        a.dist_ilv = (flags & SDFV_PASS_VOLUME_INTERLEAVED) ? 1u : 0u;
        a.air_dist = sdfv_air_dist();
        size_t bytes = scratch_bytes;
        e = rocprim::select(scratch, bytes, rocprim::counting_iterator<uint32_t>(0), indices, count, (size_t)n,
                            sdfv::UpdateRequired{a}, st);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(sdfv::emit_positions_kernel, dim3((uint32_t)(((uint64_t)a.n + sdfv::kBlock - 1) / sdfv::kBlock)), dim3(sdfv::kBlock), 0, st,
                               a, points, indices, count);
            e = hipGetLastError();
        }
    }
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return set_error(SDFV_ERR_HIP, "sdfv_emit_update_points: %s", hipGetErrorString(e));
    }
    return SDFV_OK;
}

}  // extern "C"
#pragma GCC visibility pop
