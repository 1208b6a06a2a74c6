// mesh_lattice.h -- the lattice arithmetic the mesh kernels share on the device (mesh_kernels.hip: the demo tree and every SDF-free
// step; program_mesh_kernels.hip: SDF programs; dual_contour_kernels.hip; sparse_mesh_kernels.hip: bricks): which point or cell a
// thread has, where a lattice point lies, which side of the surface a distance is on, the cube case of a cell, which corner of a
// cell owns a table edge, where the vertex of a crossing edge lies and which vertex record it is.  One statement of each, so that
// the extractors cannot drift apart (the steps built from these, over either point layout, are mesh_steps.h's): the translation
// units are built with -ffp-contract=off, every float step below is one rounded f32 operation, every division is a 32-bit one.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mesh_kernels.h"

namespace sdfv {

struct Lattice {
    uint32_t nx, ny, nz;  // points per axis
    uint32_t cx, cy, cz;  // cells per axis
    __device__ __forceinline__ explicit Lattice(const MeshGrid& g)
        : nx(g.cells[0] + 1), ny(g.cells[1] + 1), nz(g.cells[2] + 1), cx(g.cells[0]), cy(g.cells[1]), cz(g.cells[2]) {}
    __device__ __forceinline__ uint32_t points() const { return nx * ny * nz; }  // < 2^32: MeshGrid::launchable()
    __device__ __forceinline__ uint32_t cells() const { return cx * cy * cz; }
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
    // the same for a cell: c -> the (i, j, k) of the cell, which are those of its lowest corner
    __device__ __forceinline__ void uncell(uint32_t c, uint32_t& i, uint32_t& j, uint32_t& k) const {
        const uint32_t r = c / cx;
        i = c - r * cx;
        k = r / cy;
        j = r - k * cy;
    }
};

__device__ __forceinline__ bool inside(float d) { return d < 0.0f; }  // Signed: negative inside

// The cube case of the cell whose lowest corner's distance is *corner, in an array with the strides sy and sz towards +y and +z
// (1 towards +x): corner bit = x | y << 1 | z << 2.
template <typename Stride>
__device__ __forceinline__ uint32_t cube_case(const float* __restrict__ corner, Stride sy, Stride sz) {
    uint32_t c = 0;
    for (uint32_t q = 0; q < 8; ++q)
        if (inside(corner[(q & 1) + ((q >> 1) & 1) * sy + ((q >> 2) & 1) * sz])) c |= 1u << q;
    return c;
}

// Edge e of a cell, e = 4 * axis + u + 2 * v (the marching-cubes table's numbering): the edge along `axis` that starts at the
// corner offset by u along the lower (o0) and v along the higher (o1) of the two other axes.  That corner owns the edge.
// dx, dy, dz: the same offset per axis, each 0 or 1.  (Scalars: e is a run-time value in the triangle kernels, and an array
// indexed by it would live in scratch.)
struct CellEdge {
    uint32_t axis, u, v, dx, dy, dz;
};
__device__ __forceinline__ CellEdge cell_edge(int e) {
    const uint32_t a = (uint32_t)e >> 2, u = (uint32_t)e & 1u, v = ((uint32_t)e >> 1) & 1u;
    // axis 0: (u, v) along (y, z); axis 1: along (x, z); axis 2: along (x, y)
    return CellEdge{a, u, v, a != 0u ? u : 0u, a == 0u ? u : (a == 2u ? v : 0u), a != 2u ? v : 0u};
}
// the two other axes of an axis, increasing
__device__ __forceinline__ int lower_other(uint32_t axis) { return axis == 0u ? 1 : 0; }
__device__ __forceinline__ int higher_other(uint32_t axis) { return axis == 2u ? 1 : 2; }

// The vertex record of the edge towards +axis of the point in slot `owner`: a point's records come in axis order from
// point_first[owner] on.
__device__ __forceinline__ uint32_t owner_record(size_t owner, uint32_t axis, const uint8_t* __restrict__ mask,
                                                 const uint32_t* __restrict__ point_first) {
    return point_first[owner] + __popc((uint32_t)mask[owner] & ((1u << axis) - 1u));
}

// The vertex record of edge e of the cell whose lowest corner is lattice point `origin` of the dense lattice.
__device__ __forceinline__ uint32_t edge_record(const Lattice& L, size_t origin, int e, const uint8_t* __restrict__ mask,
                                                const uint32_t* __restrict__ point_first) {
    const size_t stride[3] = {1, L.nx, (size_t)L.nx * L.ny};
    const CellEdge c = cell_edge(e);
    const size_t owner = origin + c.u * stride[lower_other(c.axis)] + c.v * stride[higher_other(c.axis)];
    return owner_record(owner, c.axis, mask, point_first);
}

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
