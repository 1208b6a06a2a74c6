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

// The kernels are program_mesh_device.h's definitions with the interpreter as both evaluators; a handle compiled with
// SDFV_COMPILE_MESH brings the same definitions over that program's own (program_compile.hip).  Each launcher below builds ONE
// argument array and ProgramKernels::launch hands it to the handle's kernel or to the interpreter's, with the same grid, block
// and stream.
#define SDFV_EVAL_ONCE(ops, n_ops) prog::Interpreter{ops, n_ops}
#define SDFV_EVAL_LOOPED(ops, n_ops) prog::Interpreter{ops, n_ops}

SDFV_PROGRAM_KERNEL_mesh_lattice(sdfprog_mesh_lattice)
SDFV_PROGRAM_KERNEL_mesh_vertices(sdfprog_mesh_vertices)
SDFV_PROGRAM_KERNEL_mesh_vertices_mat(sdfprog_mesh_vertices_mat)
SDFV_PROGRAM_KERNEL_normal_points(sdfprog_normal_points)
SDFV_PROGRAM_KERNEL_normal_points_staged(sdfprog_normal_points_staged)
SDFV_PROGRAM_KERNEL_mesh_postproc(sdfprog_mesh_postproc)
SDFV_PROGRAM_KERNEL_mesh_postproc_unaligned(sdfprog_mesh_postproc_unaligned)

hipError_t launch_program_mesh_lattice(const sdfv_prog_op* ops, uint32_t n_ops, const MeshGrid& g, const MeshWork& w,
                                       const ProgramKernels& k, hipStream_t stream) {
    if (!g.launchable()) return hipErrorInvalidValue;
    MeshGrid grid = g;
    float* dist = w.dist;
    void* params[] = {&ops, &n_ops, &grid, &dist};
    return k.launch(kKernelMeshLattice, (const void*)sdfprog_mesh_lattice, dim3(blocks_for(g.n_points())), dim3(kBlock), params, stream);
}

hipError_t launch_program_vertex_normals(const sdfv_prog_op* ops, uint32_t n_ops, sdfv_vertex* vertices, size_t n_vertices,
                                         bool materials, const ProgramKernels& k, hipStream_t stream) {
    if (!vertices || n_vertices == 0) return hipSuccess;
    if (n_vertices > 0xffffffffull || ((uintptr_t)vertices & 15)) return hipErrorInvalidValue;
    float4* v4 = reinterpret_cast<float4*>(vertices);
    uint32_t n = (uint32_t)n_vertices;
    void* params[] = {&ops, &n_ops, &v4, &n};
    return k.launch(materials ? kKernelMeshVerticesMat : kKernelMeshVertices,
                    materials ? (const void*)sdfprog_mesh_vertices_mat : (const void*)sdfprog_mesh_vertices,
                    dim3(blocks_for(n_vertices)), dim3(kBlock), params, stream);
}

hipError_t launch_program_normal_points(const sdfv_prog_op* ops, uint32_t n_ops, const float* points, size_t n, float eps,
                                        float* out, const ProgramKernels& k, hipStream_t stream) {
    hipError_t first = hipSuccess;  // of the launches
    const hipError_t e = launch_staged_then_tail(
        n, (((uintptr_t)points | (uintptr_t)out) & 15) == 0,
        [&](uint32_t whole) {
            const float4* in4 = reinterpret_cast<const float4*>(points);
            float4* out4 = reinterpret_cast<float4*>(out);
            void* params[] = {&ops, &n_ops, &in4, &eps, &out4};
            const hipError_t es = k.launch(kKernelNormalPointsStaged, (const void*)sdfprog_normal_points_staged, dim3(whole), dim3(kBlock), params, stream);
            if (first == hipSuccess) first = es;
        },
        [&](uint32_t blocks, size_t done) {
            void* params[] = {&ops, &n_ops, &points, &done, &n, &eps, &out};
            const hipError_t es = k.launch(kKernelNormalPoints, (const void*)sdfprog_normal_points, dim3(blocks), dim3(kBlock), params, stream);
            if (first == hipSuccess) first = es;
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
    return k.launch(aligned ? kKernelMeshPostproc : kKernelMeshPostprocUnaligned,
                    aligned ? (const void*)sdfprog_mesh_postproc : (const void*)sdfprog_mesh_postproc_unaligned, dim3(blocks),
                    dim3(kBlock), params, stream);
}

}  // namespace sdfv
