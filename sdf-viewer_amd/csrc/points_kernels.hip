// points_kernels.hip -- the "Batched sampling" the reference leaves as a TODO (src/sdf/mod.rs:39):
// SDFSurface::sample(p, distance_only) and SDFSurface::normal(p, eps) for n arbitrary points, one
// thread per point.  Gather-style front end for the meshers (src/sdf/meshers/isosurface.rs:78-92,
// src/sdf/meshers/mesh.rs:22-33) and the per-point C ABI (src/sdf/ffi.rs:57-65,322-332).
// Every kernel has a scalar form (any alignment, any n) and a staged form for whole workgroups (tile_load / tile_store);
// the sample kernels' bodies are sample_points / sample_points_staged of kernel_common.h, shared with program_kernels.hip.
#include "points_kernels.h"

#include "kernel_common.h"

namespace sdfv {
namespace {

// The demo tree as the samplers' evaluator (sample_points / sample_points_staged, kernel_common.h).
struct DemoSampleEval {
    const sdfv_demo_params& prm;
    uint32_t sdf_id;
    bool distance_only;
    __device__ __forceinline__ Sample operator()(float px, float py, float pz) const {
        return demo_sample(prm, sdf_id, px, py, pz, distance_only);
    }
};

__global__ __launch_bounds__(kBlock) void sample_points_kernel(sdfv_demo_params prm, uint32_t sdf_id,
                                                               const float* __restrict__ points, size_t first,
                                                               size_t n, bool distance_only, float* __restrict__ out) {
    sample_points(DemoSampleEval{prm, sdf_id, distance_only}, points, first, n, out);
}

__global__ __launch_bounds__(kBlock) void sample_points_staged_kernel(sdfv_demo_params prm, uint32_t sdf_id,
                                                                      const float4* __restrict__ points,
                                                                      bool distance_only, float4* __restrict__ out) {
    sample_points_staged(DemoSampleEval{prm, sdf_id, distance_only}, points, out);
}

__global__ __launch_bounds__(kBlock) void normal_points_kernel(sdfv_demo_params prm, uint32_t sdf_id, SourceBox box,
                                                               const float* __restrict__ points, size_t first, size_t n,
                                                               float eps, bool use_default,
                                                               float* __restrict__ out) {
    const size_t i = first + (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    float px = points[i * 3 + 0], py = points[i * 3 + 1], pz = points[i * 3 + 2];
    box.to_world(px, py, pz);
    float nx, ny, nz;
    demo_normal(prm, sdf_id, px, py, pz, eps, use_default, nx, ny, nz);
    out[i * 3 + 0] = nx; out[i * 3 + 1] = ny; out[i * 3 + 2] = nz;
}

// The same for whole workgroups of 256 points, staged like sample_points_staged: 3 KiB in, 3 KiB out (tile_load / tile_store).
__global__ __launch_bounds__(kBlock) void normal_points_staged_kernel(sdfv_demo_params prm, uint32_t sdf_id, SourceBox box,
                                                                      const float4* __restrict__ points, float eps,
                                                                      bool use_default, float4* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) float s_io[kBlock * 3];
    const uint32_t t = threadIdx.x;
    tile_load<3>(s_io, points);
    __syncthreads();
    float px = s_io[t * 3 + 0], py = s_io[t * 3 + 1], pz = s_io[t * 3 + 2];
    box.to_world(px, py, pz);
    float nx, ny, nz;
    demo_normal(prm, sdf_id, px, py, pz, eps, use_default, nx, ny, nz);
    s_io[t * 3 + 0] = nx; s_io[t * 3 + 1] = ny; s_io[t * 3 + 2] = nz;  // a thread's own three words: no barrier in between
    __syncthreads();
    tile_store<3>(out, s_io);
}

// ScalarSource::sample_scalar, meshers/isosurface.rs:78-84: distance only, 12 B in, 4 B out per point.
__global__ __launch_bounds__(kBlock) void source_scalar_kernel(sdfv_demo_params prm, uint32_t sdf_id, SourceBox box,
                                                               const float* __restrict__ points, size_t first, size_t n,
                                                               float* __restrict__ out) {
    const size_t i = first + (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    float px = points[i * 3 + 0], py = points[i * 3 + 1], pz = points[i * 3 + 2];
    box.to_world(px, py, pz);
    out[i] = demo_sample(prm, sdf_id, px, py, pz, true).distance;
}

// Whole workgroups: the 12-byte points through LDS as streamed dwordx4; the 4-byte results are coalesced as they are.
__global__ __launch_bounds__(kBlock) void source_scalar_staged_kernel(sdfv_demo_params prm, uint32_t sdf_id, SourceBox box,
                                                                      const float4* __restrict__ points,
                                                                      float* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) float s_in[kBlock * 3];
    const uint32_t t = threadIdx.x;
    tile_load<3>(s_in, points);
    __syncthreads();
    float px = s_in[t * 3 + 0], py = s_in[t * 3 + 1], pz = s_in[t * 3 + 2];
    box.to_world(px, py, pz);
    __builtin_nontemporal_store(demo_sample(prm, sdf_id, px, py, pz, true).distance, out + (size_t)blockIdx.x * kBlock + t);
}

// Mesh::postproc, meshers/mesh.rs:22-33, in place over #[repr(Rust)]-free 48-byte vertices (sdfv_vertex):
// material from sample(position, false); normal from sdf.normal(position, None) where the mesher left |n|^2 < 1e-4.
__device__ __forceinline__ void postproc_vertex(const sdfv_demo_params& prm, uint32_t sdf_id, float* v) {
    const float px = v[0], py = v[1], pz = v[2];
    Sample s = demo_sample(prm, sdf_id, px, py, pz, false);
    const float dx = v[3] - 0.0f, dy = v[4] - 0.0f, dz = v[5] - 0.0f;  // distance2(Vector3::zero())
    if (dx * dx + dy * dy + dz * dz < 0.0001f) {
        float nx, ny, nz;
        demo_normal(prm, sdf_id, px, py, pz, 0.0f, false, nx, ny, nz);
        v[3] = nx; v[4] = ny; v[5] = nz;
    }
    v[6] = s.m.r; v[7] = s.m.g; v[8] = s.m.b;
    v[9] = s.m.metallic; v[10] = s.m.roughness; v[11] = s.m.occlusion;
}

__global__ __launch_bounds__(kBlock) void mesh_postproc_kernel(sdfv_demo_params prm, uint32_t sdf_id,
                                                               float* __restrict__ vertices, size_t first, size_t n) {
    const size_t i = first + (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    float v[12];
    for (int k = 0; k < 12; ++k) v[k] = vertices[i * 12 + k];
    postproc_vertex(prm, sdf_id, v);
    for (int k = 3; k < 12; ++k) vertices[i * 12 + k] = v[k];
}

// Whole workgroups: 256 vertices = 12 KiB contiguous, through LDS (tile_load / tile_store).
__global__ __launch_bounds__(kBlock) void mesh_postproc_staged_kernel(sdfv_demo_params prm, uint32_t sdf_id,
                                                                      float4* __restrict__ vertices) {
    __shared__ __attribute__((aligned(16))) float s_v[kBlock * 12];
    const uint32_t t = threadIdx.x;
    tile_load<12>(s_v, vertices);
    __syncthreads();
    float v[12];
    for (int k = 0; k < 12; ++k) v[k] = s_v[t * 12 + k];
    postproc_vertex(prm, sdf_id, v);
    for (int k = 3; k < 12; ++k) s_v[t * 12 + k] = v[k];
    __syncthreads();
    tile_store<12>(vertices, s_v);
}

}  // namespace

hipError_t launch_sample_points(const sdfv_demo_params& prm, uint32_t sdf_id, const float* points, size_t n,
                                bool distance_only, sdfv_sample* out, hipStream_t stream) {
    float* o = reinterpret_cast<float*>(out);
    return launch_staged_then_tail(
        n, (((uintptr_t)points | (uintptr_t)out) & 15) == 0,
        [&](uint32_t whole) {
            hipLaunchKernelGGL(sample_points_staged_kernel, dim3(whole), dim3(kBlock), 0, stream, prm, sdf_id,
                               reinterpret_cast<const float4*>(points), distance_only, reinterpret_cast<float4*>(o));
        },
        [&](uint32_t blocks, size_t done) {
            hipLaunchKernelGGL(sample_points_kernel, dim3(blocks), dim3(kBlock), 0, stream, prm, sdf_id, points, done, n,
                               distance_only, o);
        });
}

namespace {
SourceBox make_box(const float* bb_min, const float* bb_max) {
    SourceBox b{};
    b.unit_cube = bb_min != nullptr && bb_max != nullptr;
    for (int i = 0; i < 3 && b.unit_cube; ++i) {
        b.bb_min[i] = bb_min[i];
        b.bb_size[i] = bb_max[i] - bb_min[i];
    }
    return b;
}
}  // namespace

// (These two refuse ceil(n / 256) workgroups beyond 2^31 - 1 whatever the alignment.)
hipError_t launch_normal_points(const sdfv_demo_params& prm, uint32_t sdf_id, const float* bb_min,
                                const float* bb_max, const float* points, size_t n, float eps, bool use_default,
                                float* out, hipStream_t stream) {
    if ((n + kBlock - 1) / kBlock > 0x7fffffffull) return hipErrorInvalidValue;
    const SourceBox box = make_box(bb_min, bb_max);
    return launch_staged_then_tail(
        n, (((uintptr_t)points | (uintptr_t)out) & 15) == 0,
        [&](uint32_t whole) {
            hipLaunchKernelGGL(normal_points_staged_kernel, dim3(whole), dim3(kBlock), 0, stream, prm, sdf_id, box,
                               reinterpret_cast<const float4*>(points), eps, use_default, reinterpret_cast<float4*>(out));
        },
        [&](uint32_t blocks, size_t done) {
            hipLaunchKernelGGL(normal_points_kernel, dim3(blocks), dim3(kBlock), 0, stream, prm, sdf_id, box, points, done, n,
                               eps, use_default, out);
        });
}

hipError_t launch_source_scalar(const sdfv_demo_params& prm, uint32_t sdf_id, const float* bb_min,
                                const float* bb_max, const float* points, size_t n, float* out, hipStream_t stream) {
    if ((n + kBlock - 1) / kBlock > 0x7fffffffull) return hipErrorInvalidValue;
    const SourceBox box = make_box(bb_min, bb_max);
    return launch_staged_then_tail(
        n, (((uintptr_t)points & 15) | ((uintptr_t)out & 3)) == 0,
        [&](uint32_t whole) {
            hipLaunchKernelGGL(source_scalar_staged_kernel, dim3(whole), dim3(kBlock), 0, stream, prm, sdf_id, box,
                               reinterpret_cast<const float4*>(points), out);
        },
        [&](uint32_t blocks, size_t done) {
            hipLaunchKernelGGL(source_scalar_kernel, dim3(blocks), dim3(kBlock), 0, stream, prm, sdf_id, box, points, done, n, out);
        });
}

hipError_t launch_mesh_postproc(const sdfv_demo_params& prm, uint32_t sdf_id, sdfv_vertex* vertices, size_t n,
                                hipStream_t stream) {
    float* v = reinterpret_cast<float*>(vertices);
    return launch_staged_then_tail(
        n, ((uintptr_t)vertices & 15) == 0,
        [&](uint32_t whole) {
            hipLaunchKernelGGL(mesh_postproc_staged_kernel, dim3(whole), dim3(kBlock), 0, stream, prm, sdf_id,
                               reinterpret_cast<float4*>(v));
        },
        [&](uint32_t blocks, size_t done) {
            hipLaunchKernelGGL(mesh_postproc_kernel, dim3(blocks), dim3(kBlock), 0, stream, prm, sdf_id, v, done, n);
        });
}

}  // namespace sdfv
