// points_kernels.hip -- the "Batched sampling" the reference leaves as a TODO (src/sdf/mod.rs:39):
// SDFSurface::sample(p, distance_only) and SDFSurface::normal(p, eps) for n arbitrary points, one
// thread per point.  Gather-style front end for the meshers (src/sdf/meshers/isosurface.rs:78-92,
// src/sdf/meshers/mesh.rs:22-33) and the per-point C ABI (src/sdf/ffi.rs:57-65,322-332).
// Every kernel is the element map of kernel_common.h around an evaluator: map_elements, the scalar form (any alignment, any n),
// and map_elements_staged for whole workgroups (tile_load / tile_store); program_kernels.hip and program_mesh_kernels.hip build
// the program's on the same two.
#include "points_kernels.h"

#include "kernel_common.h"

namespace sdfv {
namespace {

// The demo tree as the element map's evaluators; all of them leave the lanes beyond n at once.
// SDFSurface::sample: a point in, its 28-byte record out.
struct DemoSampleEval {
    const sdfv_demo_params& prm;
    uint32_t sdf_id;
    bool distance_only;
    __device__ __forceinline__ void operator()(float* v, bool live) const {
        if (live) write_record(v, demo_sample(prm, sdf_id, v[0], v[1], v[2], distance_only));
    }
};

// SDFSurface::normal: a point in, the normal there out.
struct DemoNormalEval {
    const sdfv_demo_params& prm;
    uint32_t sdf_id;
    const SourceBox& box;
    float eps;
    bool use_default;
    __device__ __forceinline__ void operator()(float* v, bool live) const {
        if (!live) return;
        float px = v[0], py = v[1], pz = v[2];
        box.to_world(px, py, pz);
        float nx, ny, nz;
        demo_normal(prm, sdf_id, px, py, pz, eps, use_default, nx, ny, nz);
        v[0] = nx; v[1] = ny; v[2] = nz;
    }
};

// ScalarSource::sample_scalar, meshers/isosurface.rs:78-84: distance only, 12 B in, 4 B out per point.
struct DemoScalarEval {
    const sdfv_demo_params& prm;
    uint32_t sdf_id;
    const SourceBox& box;
    __device__ __forceinline__ void operator()(float* v, bool live) const {
        if (!live) return;
        float px = v[0], py = v[1], pz = v[2];
        box.to_world(px, py, pz);
        v[0] = demo_sample(prm, sdf_id, px, py, pz, true).distance;
    }
};

// Mesh::postproc, meshers/mesh.rs:22-33, in place over #[repr(Rust)]-free 48-byte vertices (sdfv_vertex):
// material from sample(position, false); normal from sdf.normal(position, None) where the mesher left it unset.
struct DemoPostprocEval {
    const sdfv_demo_params& prm;
    uint32_t sdf_id;
    __device__ __forceinline__ void operator()(float* v, bool live) const {
        if (!live) return;
        const float px = v[0], py = v[1], pz = v[2];
        const Sample s = demo_sample(prm, sdf_id, px, py, pz, false);
        if (normal_unset(v[3], v[4], v[5])) {
            float nx, ny, nz;
            demo_normal(prm, sdf_id, px, py, pz, 0.0f, false, nx, ny, nz);
            v[3] = nx; v[4] = ny; v[5] = nz;
        }
        v[6] = s.m.r; v[7] = s.m.g; v[8] = s.m.b;
        v[9] = s.m.metallic; v[10] = s.m.roughness; v[11] = s.m.occlusion;
    }
};

__global__ __launch_bounds__(kBlock) void sample_points_kernel(sdfv_demo_params prm, uint32_t sdf_id,
                                                               const float* __restrict__ points, size_t first,
                                                               size_t n, bool distance_only, float* __restrict__ out) {
    map_elements<3, 7>(DemoSampleEval{prm, sdf_id, distance_only}, points, first, n, out);
}

__global__ __launch_bounds__(kBlock) void sample_points_staged_kernel(sdfv_demo_params prm, uint32_t sdf_id,
                                                                      const float4* __restrict__ points,
                                                                      bool distance_only, float4* __restrict__ out) {
    map_elements_staged<3, 7>(DemoSampleEval{prm, sdf_id, distance_only}, points, out);
}

__global__ __launch_bounds__(kBlock) void normal_points_kernel(sdfv_demo_params prm, uint32_t sdf_id, SourceBox box,
                                                               const float* __restrict__ points, size_t first, size_t n,
                                                               float eps, bool use_default,
                                                               float* __restrict__ out) {
    map_elements<3, 3>(DemoNormalEval{prm, sdf_id, box, eps, use_default}, points, first, n, out);
}

__global__ __launch_bounds__(kBlock) void normal_points_staged_kernel(sdfv_demo_params prm, uint32_t sdf_id, SourceBox box,
                                                                      const float4* __restrict__ points, float eps,
                                                                      bool use_default, float4* __restrict__ out) {
    map_elements_staged<3, 3>(DemoNormalEval{prm, sdf_id, box, eps, use_default}, points, out);
}

__global__ __launch_bounds__(kBlock) void source_scalar_kernel(sdfv_demo_params prm, uint32_t sdf_id, SourceBox box,
                                                               const float* __restrict__ points, size_t first, size_t n,
                                                               float* __restrict__ out) {
    map_elements<3, 1>(DemoScalarEval{prm, sdf_id, box}, points, first, n, out);
}

__global__ __launch_bounds__(kBlock) void source_scalar_staged_kernel(sdfv_demo_params prm, uint32_t sdf_id, SourceBox box,
                                                                      const float4* __restrict__ points,
                                                                      float* __restrict__ out) {
    map_elements_staged<3, 1>(DemoScalarEval{prm, sdf_id, box}, points, out);
}

// The scalar form leaves the three position words unwritten (SKIP = 3); the staged form stores its tile whole, as loaded.
__global__ __launch_bounds__(kBlock) void mesh_postproc_kernel(sdfv_demo_params prm, uint32_t sdf_id,
                                                               float* __restrict__ vertices, size_t first, size_t n) {
    map_elements<12, 12, 3>(DemoPostprocEval{prm, sdf_id}, vertices, first, n, vertices);
}

__global__ __launch_bounds__(kBlock) void mesh_postproc_staged_kernel(sdfv_demo_params prm, uint32_t sdf_id,
                                                                      float4* __restrict__ vertices) {
    map_elements_staged<12, 12, 3>(DemoPostprocEval{prm, sdf_id}, vertices, vertices);
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

hipError_t launch_normal_points(const sdfv_demo_params& prm, uint32_t sdf_id, const float* bb_min,
                                const float* bb_max, const float* points, size_t n, float eps, bool use_default,
                                float* out, hipStream_t stream) {
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
