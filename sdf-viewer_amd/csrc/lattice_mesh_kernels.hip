// lattice_mesh_kernels.hip -- meshing a lattice of distances the caller sampled (include/sdfgrid.h, "Meshing a sampled lattice"),
// on gfx950: the positions of lattice points (so that a surface sampled on the device can be fed), the distances out of sample
// records, and the per-vertex normal from the lattice itself.  Nothing here evaluates an SDF.
//
// Shape.
//  * lattice_points, lattice_from_samples: one element per thread, memory order.
//  * lattice_normals[_zero_mat]: one thread per VERTEX of the compacted list, dense waves, as sdfprog_mesh_vertices: the vertex
//    pass of lattice_vertex.h (shared with grid_mesh_kernels.hip), 48 distances per vertex in four rounds of 12 loads.  The
//    lanes of a wave are neighbours on the surface (the vertex list is in lattice order), so their taps share cache lines.
// Every float step is one rounded f32 operation (the translation unit is built with -ffp-contract=off).
// The kernels carry C names: tests and profiles find them under the same symbol whatever the toolchain mangles.
#include "lattice_mesh_kernels.h"

#include "kernel_common.h"
#include "lattice_vertex.h"
#include "mesh_lattice.h"

namespace sdfv {

extern "C" {

__global__ __launch_bounds__(kBlock) void lattice_points(MeshGrid g, uint32_t first, uint32_t n, float* __restrict__ out) {
    const Lattice L(g);
    const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
    if (t >= n) return;
    uint32_t i, j, k;
    L.unflat(first + t, i, j, k);
    float px, py, pz;
    lattice_position(g, i, j, k, px, py, pz);
    float* o = out + (size_t)t * 3;
    o[0] = px;
    o[1] = py;
    o[2] = pz;
}

__global__ __launch_bounds__(kBlock) void lattice_from_samples(const float* __restrict__ samples, size_t n, float* __restrict__ dist) {
    const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < n) dist[i] = samples[i * 7];
}

__global__ __launch_bounds__(kBlock) void lattice_normals(const float* __restrict__ dist, MeshGrid g, float* __restrict__ vertices,
                                                          uint32_t n) {
    vertex_normal(dist, g, vertices, n, KeepMaterial{});
}

__global__ __launch_bounds__(kBlock) void lattice_normals_zero_mat(const float* __restrict__ dist, MeshGrid g,
                                                                   float* __restrict__ vertices, uint32_t n) {
    vertex_normal(dist, g, vertices, n, ZeroMaterial{});
}

}  // extern "C"

hipError_t launch_lattice_points(const MeshGrid& g, uint32_t first, uint32_t n, float* out, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    if (!g.launchable() || (uint64_t)first + n > g.n_points()) return hipErrorInvalidValue;
    hipLaunchKernelGGL(lattice_points, dim3(blocks_for(n)), dim3(kBlock), 0, stream, g, first, n, out);
    return hipGetLastError();
}

hipError_t launch_lattice_from_samples(const sdfv_sample* samples, size_t n, float* dist, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    const uint32_t blocks = blocks_for(n);
    if (!blocks) return hipErrorInvalidValue;
    hipLaunchKernelGGL(lattice_from_samples, dim3(blocks), dim3(kBlock), 0, stream, reinterpret_cast<const float*>(samples),
                       n, dist);
    return hipGetLastError();
}

hipError_t launch_lattice_normals(const float* dist, const MeshGrid& g, sdfv_vertex* vertices, size_t n, bool zero_materials,
                                  hipStream_t stream) {
    if (!vertices || n == 0) return hipSuccess;
    if (!g.launchable() || n > 0xffffffffull || (zero_materials && ((uintptr_t)vertices & 7))) return hipErrorInvalidValue;
    hipLaunchKernelGGL(zero_materials ? lattice_normals_zero_mat : lattice_normals, dim3(blocks_for(n)), dim3(kBlock), 0, stream,
                       dist, g, reinterpret_cast<float*>(vertices), (uint32_t)n);
    return hipGetLastError();
}

}  // namespace sdfv
