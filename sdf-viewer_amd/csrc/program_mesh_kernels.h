// program_mesh_kernels.h -- launch interface of the mesh pipeline's SDF-program kernels (see program_mesh_kernels.hip): the two
// steps of an extraction that evaluate the SDF (mesh_kernels.h has the others), the batched normal and Mesh::postproc.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/sdfgrid.h"
#include "mesh_kernels.h"

namespace sdfv {

struct ProgramKernels;  // program_kernels.h
// ops: the DEVICE copy of the validated program.  k: the kernels of a handle compiled with SDFV_COMPILE_MESH, launched in the
// interpreter's place with the same grid, block and stream -- or none (a plain handle, a handle without the route).
// step 1 of an extraction: the program's distance at every lattice point into w.dist.  Checks the grid (MeshGrid::launchable).
hipError_t launch_program_mesh_lattice(const sdfv_prog_op* ops, uint32_t n_ops, const MeshGrid& g, const MeshWork& w,
                                       const ProgramKernels& k, hipStream_t stream);
// step 5: one thread per vertex of n_vertices whose positions are written (16-byte aligned) for the normal and, with `materials`,
// the material fields Mesh::postproc would write (zero otherwise).  Marching cubes runs it over the vertices of step 4, dual
// contouring over its Hermite records and again over its solved vertices -- the same kernels
hipError_t launch_program_vertex_normals(const sdfv_prog_op* ops, uint32_t n_ops, sdfv_vertex* vertices, size_t n_vertices,
                                         bool materials, const ProgramKernels& k, hipStream_t stream);
// normal_default_impl of the program at n points: 12 bytes in, 12 bytes out
hipError_t launch_program_normal_points(const sdfv_prog_op* ops, uint32_t n_ops, const float* points, size_t n, float eps,
                                        float* out, const ProgramKernels& k, hipStream_t stream);
// Mesh::postproc in place
hipError_t launch_program_mesh_postproc(const sdfv_prog_op* ops, uint32_t n_ops, sdfv_vertex* vertices, size_t n,
                                        const ProgramKernels& k, hipStream_t stream);

}  // namespace sdfv
