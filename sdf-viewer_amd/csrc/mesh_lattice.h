// mesh_lattice.h -- the lattice arithmetic the mesh kernels share on the device (mesh_kernels.hip for the demo tree,
// program_mesh_kernels.hip for SDF programs): where a lattice point lies and where the vertex of a crossing edge lies.  One
// statement of each, so that the two extractors cannot drift apart: both translation units are built with
// -ffp-contract=off, every step below is one rounded f32 operation.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mesh_kernels.h"

namespace sdfv {

struct Lattice {
    uint32_t nx, ny, nz;  // points per axis
    __device__ __forceinline__ explicit Lattice(const MeshGrid& g) : nx(g.cells[0] + 1), ny(g.cells[1] + 1), nz(g.cells[2] + 1) {}
    __device__ __forceinline__ uint32_t points() const { return nx * ny * nz; }  // < 2^32: the API caps cells per axis at 1024
    __device__ __forceinline__ size_t flat(uint32_t i, uint32_t j, uint32_t k) const {
        return ((size_t)k * ny + j) * nx + i;
    }
    // flat index -> (i, j, k), x fastest (32-bit divisions: a handful of instructions, unlike 64-bit ones)
    __device__ __forceinline__ void unflat(uint32_t v, uint32_t& i, uint32_t& j, uint32_t& k) const {
        const uint32_t r = v / nx;
        i = v - r * nx;
        k = r / ny;
        j = r - k * ny;
    }
};

__device__ __forceinline__ float unit_coord(uint32_t i, uint32_t cells) { return (float)i / (float)cells; }

// vert_pos_to of lattice point (i, j, k): unit * size + min per axis
__device__ __forceinline__ void lattice_position(const MeshGrid& g, uint32_t i, uint32_t j, uint32_t k, float& px, float& py,
                                                 float& pz) {
    px = unit_coord(i, g.cells[0]) * g.bb_size[0] + g.bb_min[0];
    py = unit_coord(j, g.cells[1]) * g.bb_size[1] + g.bb_min[1];
    pz = unit_coord(k, g.cells[2]) * g.bb_size[2] + g.bb_min[2];
}

// The vertex on the edge from lattice point idx towards +axis a, whose ends have the distances d0 and d1 of different sign (so
// the denominator is never 0): linear interpolation in unit-cube coordinates, then vert_pos_to.
__device__ __forceinline__ void edge_position(const MeshGrid& g, const uint32_t idx[3], int a, float d0, float d1, float& px,
                                              float& py, float& pz) {
    const float t = d0 / (d0 - d1);
    float u[3];
    for (int b = 0; b < 3; ++b) u[b] = unit_coord(idx[b], g.cells[b]);
    const float u1 = unit_coord(idx[a] + 1, g.cells[a]);
    u[a] = u[a] + t * (u1 - u[a]);
    px = u[0] * g.bb_size[0] + g.bb_min[0];
    py = u[1] * g.bb_size[1] + g.bb_min[1];
    pz = u[2] * g.bb_size[2] + g.bb_min[2];
}

}  // namespace sdfv
