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
//    position, runs the four taps of normal_default_impl through ONE copy of the interpreter in a loop (tap_normal of
//    program_mesh_device.h; _mat adds a fifth, full run at the position itself + resolve(): material_at), writes the 48-byte
//    record as three 16-byte stores;
//  * sdfprog_normal_points[_staged] (the element map of kernel_common.h), sdfprog_mesh_postproc[_unaligned]: the same per-lane
//    function over caller arrays.
// Every live lane runs the whole program, so the instruction stream stays wave-uniform: scalar loads, as in program_kernels.hip.
// The kernels carry C names: tests and profiles find them under the same symbol whatever the toolchain mangles.
#include "program_mesh_kernels.h"

#include "program_kernels.h"
#include "program_mesh_device.h"

namespace sdfv {

// The bodies are program_mesh_device.h's, over an evaluator: here the interpreter, in the kernels a handle compiled with
// SDFV_COMPILE_MESH brings (program_compile.hip) that program's own.  Each launcher below tries the handle's kernel first
// (ProgramKernels::launch) over ONE argument array -- the two kernels of a pair have the same parameter list -- and launches the
// interpreter's otherwise, with the same grid, block and stream.
namespace {
using Interp = prog::Interpreter;
}  // namespace

extern "C" {

__global__ __launch_bounds__(kBlock) void sdfprog_mesh_lattice(const sdfv_prog_op* __restrict__ ops, uint32_t n_ops, MeshGrid g,
                                                               float* __restrict__ dist) {
    mesh_lattice_points(Interp{ops, n_ops}, g, dist);
}

__global__ __launch_bounds__(kBlock) void sdfprog_mesh_vertices(const sdfv_prog_op* __restrict__ ops, uint32_t n_ops,
                                                                float4* __restrict__ vertices, uint32_t n) {
    mesh_vertices<false>(Interp{ops, n_ops}, Interp{ops, n_ops}, ops, vertices, n);
}

__global__ __launch_bounds__(kBlock) void sdfprog_mesh_vertices_mat(const sdfv_prog_op* __restrict__ ops, uint32_t n_ops,
                                                                    float4* __restrict__ vertices, uint32_t n) {
    mesh_vertices<true>(Interp{ops, n_ops}, Interp{ops, n_ops}, ops, vertices, n);
}

__global__ __launch_bounds__(kBlock) void sdfprog_normal_points(const sdfv_prog_op* __restrict__ ops, uint32_t n_ops,
                                                                const float* __restrict__ points, size_t first, size_t n,
                                                                float eps, float* __restrict__ out) {
    map_elements<3, 3>(ProgramNormalEval<Interp>{Interp{ops, n_ops}, eps}, points, first, n, out);
}

__global__ __launch_bounds__(kBlock) void sdfprog_normal_points_staged(const sdfv_prog_op* __restrict__ ops, uint32_t n_ops,
                                                                       const float4* __restrict__ points, float eps,
                                                                       float4* __restrict__ out) {
    map_elements_staged<3, 3>(ProgramNormalEval<Interp>{Interp{ops, n_ops}, eps}, points, out);
}

__global__ __launch_bounds__(kBlock) void sdfprog_mesh_postproc(const sdfv_prog_op* __restrict__ ops, uint32_t n_ops,
                                                                float4* __restrict__ vertices, size_t n) {
    mesh_postproc_aligned(Interp{ops, n_ops}, Interp{ops, n_ops}, ops, vertices, n);
}

__global__ __launch_bounds__(kBlock) void sdfprog_mesh_postproc_unaligned(const sdfv_prog_op* __restrict__ ops, uint32_t n_ops,
                                                                          float* __restrict__ vertices, size_t n) {
    mesh_postproc_words(Interp{ops, n_ops}, Interp{ops, n_ops}, ops, vertices, n);
}

}  // extern "C"

hipError_t launch_program_mesh_lattice(const sdfv_prog_op* ops, uint32_t n_ops, const MeshGrid& g, const MeshWork& w,
                                       const ProgramKernels& k, hipStream_t stream) {
    if (!g.launchable()) return hipErrorInvalidValue;
    MeshGrid grid = g;
    float* dist = w.dist;
    void* params[] = {&ops, &n_ops, &grid, &dist};
    bool mine = false;
    const hipError_t e = k.launch(kKernelMeshLattice, dim3(blocks_for(g.n_points())), dim3(kBlock), params, stream, &mine);
    if (mine) return e;
    hipLaunchKernelGGL(sdfprog_mesh_lattice, dim3(blocks_for(g.n_points())), dim3(kBlock), 0, stream, ops, n_ops, g, w.dist);
    return hipGetLastError();
}

hipError_t launch_program_vertex_normals(const sdfv_prog_op* ops, uint32_t n_ops, sdfv_vertex* vertices, size_t n_vertices,
                                         bool materials, const ProgramKernels& k, hipStream_t stream) {
    if (!vertices || n_vertices == 0) return hipSuccess;
    if (n_vertices > 0xffffffffull || ((uintptr_t)vertices & 15)) return hipErrorInvalidValue;
    float4* v4 = reinterpret_cast<float4*>(vertices);
    uint32_t n = (uint32_t)n_vertices;
    void* params[] = {&ops, &n_ops, &v4, &n};
    bool mine = false;
    const hipError_t e = k.launch(materials ? kKernelMeshVerticesMat : kKernelMeshVertices, dim3(blocks_for(n_vertices)), dim3(kBlock),
                                  params, stream, &mine);
    if (mine) return e;
    hipLaunchKernelGGL(materials ? sdfprog_mesh_vertices_mat : sdfprog_mesh_vertices, dim3(blocks_for(n_vertices)), dim3(kBlock), 0,
                       stream, ops, n_ops, v4, n);
    return hipGetLastError();
}

hipError_t launch_program_normal_points(const sdfv_prog_op* ops, uint32_t n_ops, const float* points, size_t n, float eps,
                                        float* out, const ProgramKernels& k, hipStream_t stream) {
    hipError_t first = hipSuccess;  // of the specialised launches (the interpreter's report through hipGetLastError)
    bool mine = false;
    const hipError_t e = launch_staged_then_tail(
        n, (((uintptr_t)points | (uintptr_t)out) & 15) == 0,
        [&](uint32_t whole) {
            const float4* in4 = reinterpret_cast<const float4*>(points);
            float4* out4 = reinterpret_cast<float4*>(out);
            void* params[] = {&ops, &n_ops, &in4, &eps, &out4};
            const hipError_t es = k.launch(kKernelNormalPointsStaged, dim3(whole), dim3(kBlock), params, stream, &mine);
            if (first == hipSuccess) first = es;
            if (mine) return;
            hipLaunchKernelGGL(sdfprog_normal_points_staged, dim3(whole), dim3(kBlock), 0, stream, ops, n_ops, in4, eps, out4);
        },
        [&](uint32_t blocks, size_t done) {
            void* params[] = {&ops, &n_ops, &points, &done, &n, &eps, &out};
            const hipError_t es = k.launch(kKernelNormalPoints, dim3(blocks), dim3(kBlock), params, stream, &mine);
            if (first == hipSuccess) first = es;
            if (mine) return;
            hipLaunchKernelGGL(sdfprog_normal_points, dim3(blocks), dim3(kBlock), 0, stream, ops, n_ops, points, done, n, eps, out);
        });
    return first != hipSuccess ? first : e;
}

hipError_t launch_program_mesh_postproc(const sdfv_prog_op* ops, uint32_t n_ops, sdfv_vertex* vertices, size_t n,
                                        const ProgramKernels& k, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    const uint32_t blocks = blocks_for(n);
    if (!blocks) return hipErrorInvalidValue;
    const bool aligned = ((uintptr_t)vertices & 15) == 0;
    void* params[] = {&ops, &n_ops, &vertices, &n};  // (float4* or float*: a pointer either way)
    bool mine = false;
    const hipError_t e = k.launch(aligned ? kKernelMeshPostproc : kKernelMeshPostprocUnaligned, dim3(blocks), dim3(kBlock), params,
                                  stream, &mine);
    if (mine) return e;
    if (aligned)
        hipLaunchKernelGGL(sdfprog_mesh_postproc, dim3(blocks), dim3(kBlock), 0, stream, ops, n_ops,
                           reinterpret_cast<float4*>(vertices), n);
    else
        hipLaunchKernelGGL(sdfprog_mesh_postproc_unaligned, dim3(blocks), dim3(kBlock), 0, stream, ops, n_ops,
                           reinterpret_cast<float*>(vertices), n);
    return hipGetLastError();
}

}  // namespace sdfv
