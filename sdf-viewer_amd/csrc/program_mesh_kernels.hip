// program_mesh_kernels.hip -- the mesh pipeline over SDF programs on gfx950 (include/sdfgrid.h, "SDF programs: meshing"): the two
// steps of an extraction that evaluate the SDF, the batched normal and Mesh::postproc, with the interpreter of program_eval.h as
// the evaluator.  The SDF-independent steps (edge masks, the two scans, the vertex positions, the triangles) are
// mesh_kernels.hip's, shared with the demo tree.
//
// Shape.  The interpreter costs one whole program run per WAVE, however few of its lanes are live, so nothing here evaluates the
// program under a sparse mask:
//  * sdfprog_mesh_lattice: one lattice point per thread, x fastest, distance only (no resolve(), no material traffic);
//  * sdfprog_mesh_vertices[_mat]: one thread per VERTEX of the compacted list the scan produced, whose positions
//    mesh_edge_positions (mesh_kernels.hip, SDF-free) or dual contouring's solve has written -- dense waves.  Reads the
//    position, runs the four taps of normal_default_impl through ONE copy of the interpreter in a loop (tap_normal; _mat adds a
//    fifth, full run at the position itself + resolve(): material_at), writes the 48-byte record as three 16-byte stores;
//  * sdfprog_normal_points[_staged] (the element map of kernel_common.h), sdfprog_mesh_postproc[_unaligned]: the same per-lane
//    function over caller arrays.
// Every live lane runs the whole program, so the instruction stream stays wave-uniform: scalar loads, as in program_kernels.hip.
// The kernels carry C names: tests and profiles find them under the same symbol whatever the toolchain mangles.
#include "program_mesh_kernels.h"

#include "kernel_common.h"
#include "mesh_lattice.h"
#include "program_eval.h"
#include "program_resolve.h"

namespace sdfv {

namespace {

__device__ __forceinline__ bool wave_any(bool b) { return __ballot(b) != 0ull; }

// normal_default_impl (defaults.rs:49-56) of the program at p -> (nx, ny, nz), per lane, written for a WAVE: under the lanes
// with `taps`, left alone under the others, skipped by the wave when no lane wants it.  The operation sequence is
// demo_normal(..., use_default = true) of demo_sdf_device.h with the program's distance in the demo's place:
// e = eps > 0 ? eps : 0.001; taps at p + (e, -e, -e), (-e, e, -e), (-e, -e, e), (e, e, e), a coordinate being p + k * e with
// k = 1.0f or -1.0f (k * e is exact); sums left to right in tap order, the first term standing alone (d1 + -d2 + -d3 + d4 for
// x; a term is k * d, exact); normalize3.
// The four runs go through ONE copy of the interpreter: a loop that is not unrolled, as program_march.h does for its taps.  Only
// the distance of a run is used, so this copy carries no material indices (the compiler drops them: 56 VGPRs for a bare run, as
// in sdfprog_mesh_lattice, against 72 with them).
__device__ __forceinline__ void tap_normal(const sdfv_prog_op* __restrict__ ops, uint32_t n_ops, float px, float py, float pz,
                                           float eps, bool taps, float& nx, float& ny, float& nz) {
    if (!wave_any(taps)) return;
    const float e = eps > 0.0f ? eps : 0.001f;
    float ax = 0.0f, ay = 0.0f, az = 0.0f;
#pragma unroll 1
    for (int t = 0; t < 4; ++t) {
        if (taps) {
            const float kx = (t == 0 || t == 3) ? 1.0f : -1.0f;
            const float ky = (t == 1 || t == 3) ? 1.0f : -1.0f;
            const float kz = (t == 2 || t == 3) ? 1.0f : -1.0f;
            const float d = prog::run(ops, n_ops, px + kx * e, py + ky * e, pz + kz * e).d;
            ax = t == 0 ? kx * d : ax + kx * d;
            ay = t == 0 ? ky * d : ay + ky * d;
            az = t == 0 ? kz * d : az + kz * d;
        }
    }
    if (taps) normalize3(ax, ay, az, nx, ny, nz);
}

// The material fields of sample(p, false) under the lanes with `live`: a fifth, full run (this one does carry the material
// index) + resolve() -- raw fields, not packed, not clamped.  It comes BEFORE the taps in every kernel below: a run with material
// indices needs 72 VGPRs by itself, and after it only the six fields (or the two that share a store with the normal) stay live
// across the cheaper taps -- the other way round the normal and the point would have to survive the expensive run.
__device__ __forceinline__ Mat material_at(const sdfv_prog_op* __restrict__ ops, uint32_t n_ops, float px, float py, float pz,
                                           bool live) {
    prog::Value v;
    v.d = 0.0f;
    v.m = prog::kNoMaterial;
    if (live) v = prog::run(ops, n_ops, px, py, pz);
    return resolve(ops, v, false).m;
}

template <bool MAT>
__device__ __forceinline__ void mesh_vertices(const sdfv_prog_op* __restrict__ ops, uint32_t n_ops, float4* __restrict__ vertices,
                                              uint32_t n) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    const bool live = i < n;
    float4* v = vertices + (size_t)(live ? i : 0) * 3;
    float4 p = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (live) p = v[0];  // the position (w: not yet written, not used)
    // the 48-byte record leaves as three 16-byte stores: {b, metallic, roughness, occlusion} as soon as it is known
    Mat m = zero_mat();  // without MAT: Vertex::default()'s zero material
    if (MAT) m = material_at(ops, n_ops, p.x, p.y, p.z, live);
    if (live) v[2] = make_float4(m.b, m.metallic, m.roughness, m.occlusion);
    float nx = 0.0f, ny = 0.0f, nz = 0.0f;
    tap_normal(ops, n_ops, p.x, p.y, p.z, 0.0f, live, nx, ny, nz);
    if (live) {
        v[0] = make_float4(p.x, p.y, p.z, nx);
        v[1] = make_float4(ny, nz, m.r, m.g);
    }
}

// The batched normal as the element map's evaluator (kernel_common.h): a point in, the normal there out.  EVERY lane goes into
// tap_normal, the lanes beyond n (whose point is zero) under its mask: the interpreter's loop is the wave's.
struct ProgramNormalEval {
    const sdfv_prog_op* ops;
    uint32_t n_ops;
    float eps;
    __device__ __forceinline__ void operator()(float* v, bool live) const {
        float nx = 0.0f, ny = 0.0f, nz = 0.0f;
        tap_normal(ops, n_ops, v[0], v[1], v[2], eps, live, nx, ny, nz);
        v[0] = nx; v[1] = ny; v[2] = nz;
    }
};

}  // namespace

extern "C" {

__global__ __launch_bounds__(kBlock) void sdfprog_mesh_lattice(const sdfv_prog_op* __restrict__ ops, uint32_t n_ops, MeshGrid g,
                                                               float* __restrict__ dist) {
    const Lattice L(g);
    const uint32_t v = blockIdx.x * kBlock + threadIdx.x;
    if (v >= L.points()) return;
    uint32_t i, j, k;
    L.unflat(v, i, j, k);
    float px, py, pz;
    lattice_position(g, i, j, k, px, py, pz);
    dist[v] = prog::run(ops, n_ops, px, py, pz).d;
}

__global__ __launch_bounds__(kBlock) void sdfprog_mesh_vertices(const sdfv_prog_op* __restrict__ ops, uint32_t n_ops,
                                                                float4* __restrict__ vertices, uint32_t n) {
    mesh_vertices<false>(ops, n_ops, vertices, n);
}

__global__ __launch_bounds__(kBlock) void sdfprog_mesh_vertices_mat(const sdfv_prog_op* __restrict__ ops, uint32_t n_ops,
                                                                    float4* __restrict__ vertices, uint32_t n) {
    mesh_vertices<true>(ops, n_ops, vertices, n);
}

__global__ __launch_bounds__(kBlock) void sdfprog_normal_points(const sdfv_prog_op* __restrict__ ops, uint32_t n_ops,
                                                                const float* __restrict__ points, size_t first, size_t n,
                                                                float eps, float* __restrict__ out) {
    map_elements<3, 3>(ProgramNormalEval{ops, n_ops, eps}, points, first, n, out);
}

__global__ __launch_bounds__(kBlock) void sdfprog_normal_points_staged(const sdfv_prog_op* __restrict__ ops, uint32_t n_ops,
                                                                       const float4* __restrict__ points, float eps,
                                                                       float4* __restrict__ out) {
    map_elements_staged<3, 3>(ProgramNormalEval{ops, n_ops, eps}, points, out);
}

// 16-byte aligned vertices: 16-byte accesses.  A kept normal goes back as it was read.
__global__ __launch_bounds__(kBlock) void sdfprog_mesh_postproc(const sdfv_prog_op* __restrict__ ops, uint32_t n_ops,
                                                                float4* __restrict__ vertices, size_t n) {
    const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    const bool live = i < n;
    float4* v = vertices + (live ? i : 0) * 3;
    float4 a = make_float4(0.0f, 0.0f, 0.0f, 1.0f), b = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (live) {
        a = v[0];
        b = v[1];
    }
    const Mat m = material_at(ops, n_ops, a.x, a.y, a.z, live);
    if (live) v[2] = make_float4(m.b, m.metallic, m.roughness, m.occlusion);
    float nx = a.w, ny = b.x, nz = b.y;
    const bool taps = live && normal_unset(nx, ny, nz);
    tap_normal(ops, n_ops, a.x, a.y, a.z, 0.0f, taps, nx, ny, nz);
    if (taps) v[0] = make_float4(a.x, a.y, a.z, nx);
    if (live) v[1] = make_float4(ny, nz, m.r, m.g);
}

// Any 4-byte aligned vertex array: dword accesses; position and a kept normal are not written.
__global__ __launch_bounds__(kBlock) void sdfprog_mesh_postproc_unaligned(const sdfv_prog_op* __restrict__ ops, uint32_t n_ops,
                                                                          float* __restrict__ vertices, size_t n) {
    const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    const bool live = i < n;
    float* v = vertices + (live ? i : 0) * 12;
    float px = 0.0f, py = 0.0f, pz = 0.0f, nx = 1.0f, ny = 0.0f, nz = 0.0f;
    if (live) {
        px = v[0]; py = v[1]; pz = v[2];
        nx = v[3]; ny = v[4]; nz = v[5];
    }
    const Mat m = material_at(ops, n_ops, px, py, pz, live);
    if (live) {
        v[6] = m.r; v[7] = m.g; v[8] = m.b;
        v[9] = m.metallic; v[10] = m.roughness; v[11] = m.occlusion;
    }
    const bool taps = live && normal_unset(nx, ny, nz);
    tap_normal(ops, n_ops, px, py, pz, 0.0f, taps, nx, ny, nz);
    if (taps) {
        v[3] = nx; v[4] = ny; v[5] = nz;
    }
}

}  // extern "C"

hipError_t launch_program_mesh_lattice(const sdfv_prog_op* ops, uint32_t n_ops, const MeshGrid& g, const MeshWork& w,
                                       hipStream_t stream) {
    if (!g.launchable()) return hipErrorInvalidValue;
    hipLaunchKernelGGL(sdfprog_mesh_lattice, dim3(blocks_for(g.n_points())), dim3(kBlock), 0, stream, ops, n_ops, g, w.dist);
    return hipGetLastError();
}

hipError_t launch_program_vertex_normals(const sdfv_prog_op* ops, uint32_t n_ops, sdfv_vertex* vertices, size_t n_vertices,
                                         bool materials, hipStream_t stream) {
    if (!vertices || n_vertices == 0) return hipSuccess;
    if (n_vertices > 0xffffffffull || ((uintptr_t)vertices & 15)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(materials ? sdfprog_mesh_vertices_mat : sdfprog_mesh_vertices, dim3(blocks_for(n_vertices)), dim3(kBlock), 0,
                       stream, ops, n_ops, reinterpret_cast<float4*>(vertices), (uint32_t)n_vertices);
    return hipGetLastError();
}

hipError_t launch_program_normal_points(const sdfv_prog_op* ops, uint32_t n_ops, const float* points, size_t n, float eps,
                                        float* out, hipStream_t stream) {
    return launch_staged_then_tail(
        n, (((uintptr_t)points | (uintptr_t)out) & 15) == 0,
        [&](uint32_t whole) {
            hipLaunchKernelGGL(sdfprog_normal_points_staged, dim3(whole), dim3(kBlock), 0, stream, ops, n_ops,
                               reinterpret_cast<const float4*>(points), eps, reinterpret_cast<float4*>(out));
        },
        [&](uint32_t blocks, size_t done) {
            hipLaunchKernelGGL(sdfprog_normal_points, dim3(blocks), dim3(kBlock), 0, stream, ops, n_ops, points, done, n, eps, out);
        });
}

hipError_t launch_program_mesh_postproc(const sdfv_prog_op* ops, uint32_t n_ops, sdfv_vertex* vertices, size_t n,
                                        hipStream_t stream) {
    if (n == 0) return hipSuccess;
    const uint32_t blocks = blocks_for(n);
    if (!blocks) return hipErrorInvalidValue;
    if (((uintptr_t)vertices & 15) == 0)
        hipLaunchKernelGGL(sdfprog_mesh_postproc, dim3(blocks), dim3(kBlock), 0, stream, ops, n_ops,
                           reinterpret_cast<float4*>(vertices), n);
    else
        hipLaunchKernelGGL(sdfprog_mesh_postproc_unaligned, dim3(blocks), dim3(kBlock), 0, stream, ops, n_ops,
                           reinterpret_cast<float*>(vertices), n);
    return hipGetLastError();
}

}  // namespace sdfv
