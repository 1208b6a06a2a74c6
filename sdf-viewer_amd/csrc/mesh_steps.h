// mesh_steps.h -- the steps of marching cubes that do not depend on the SDF, stated once for both ways the lattice points of an
// extraction are laid out in memory: the whole box, x fastest (DenseLayout here; mesh_kernels.hip, dual_contour_kernels.hip), and
// 125 points per brick (BrickLayout of sparse_mesh_kernels.hip).  The layout is a template parameter; a kernel is index, bounds
// and a call.
//
// A layout says what thread t's point is.  Its slot in dist / mask / first is t in both.
//  * point(t): a LatticePoint -- the lattice index in the whole box (what edge_position takes) and, per axis, whether the point
//    has (owns) the edge towards +axis;
//  * stride[3]: from a slot to the slot of the +axis neighbour, where the point has that edge.
// Which point owns an edge, in which order a point's vertices come and which way `inside` cuts at 0 are rules the tests pin bit
// for bit: they are here and in mesh_lattice.h, and nowhere else.
#pragma once

#include "mesh_lattice.h"

namespace sdfv {

namespace {
#define SDFV_MC_TABLE __constant__ const
#include "mc_table.inc"
#undef SDFV_MC_TABLE
}  // namespace

struct LatticePoint {
    uint32_t idx[3];
    uint32_t edges;  // bit a: the point has the edge towards +axis a
};

// Every point of the box; a point has the edges that stay inside it.  32-bit divisions, size_t strides.
struct DenseLayout {
    Lattice L;
    size_t stride[3];
    __device__ __forceinline__ explicit DenseLayout(const MeshGrid& g) : L(g), stride{1, L.nx, (size_t)L.nx * L.ny} {}
    __device__ __forceinline__ LatticePoint point(uint32_t v) const {
        LatticePoint p;
        L.unflat(v, p.idx[0], p.idx[1], p.idx[2]);
        p.edges = (p.idx[0] + 1 < L.nx ? 1u : 0u) | (p.idx[1] + 1 < L.ny ? 2u : 0u) | (p.idx[2] + 1 < L.nz ? 4u : 0u);
        return p;
    }
};

// Which of the point's +axis edges cross the surface -> mask[t], and their number -> count[t], the scan's input.
template <typename Layout>
__device__ __forceinline__ void edge_mask_step(const Layout& lay, uint32_t t, const float* __restrict__ dist,
                                               uint8_t* __restrict__ mask, uint32_t* __restrict__ count) {
    const LatticePoint p = lay.point(t);
    const bool in0 = inside(dist[t]);
    uint32_t m = 0;
    for (int a = 0; a < 3; ++a)
        if ((p.edges >> a & 1u) && inside(dist[t + lay.stride[a]]) != in0) m |= 1u << a;
    mask[t] = (uint8_t)m;
    count[t] = __popc(m);
}

// One vertex per crossing edge of point t, in axis order: vertex(id, px, py, pz) with the position on the edge by linear
// interpolation of the two distances and the record id, which starts at first[t].
template <typename Layout, typename VertexFn>
__device__ __forceinline__ void edge_vertex_step(const MeshGrid& g, const Layout& lay, uint32_t t, const float* __restrict__ dist,
                                                 const uint8_t* __restrict__ mask, const uint32_t* __restrict__ first,
                                                 VertexFn&& vertex) {
    const uint32_t m = mask[t];
    if (m == 0) return;
    const LatticePoint p = lay.point(t);
    const float d0 = dist[t];
    uint32_t id = first[t];
    for (int a = 0; a < 3; ++a) {
        if (!(m & (1u << a))) continue;
        float px, py, pz;
        edge_position(g, p.idx, a, d0, dist[t + lay.stride[a]], px, py, pz);
        vertex(id, px, py, pz);
        ++id;
    }
}

// ... whose position alone is stored, into record id of `vertices`
struct StorePosition {
    float* __restrict__ vertices;
    __device__ __forceinline__ void operator()(uint32_t id, float px, float py, float pz) const {
        float* o = vertices + (size_t)id * 12;
        o[0] = px; o[1] = py; o[2] = pz;
    }
};

// The n_tri triangles of a cell with cube case cs: record_of(e) is the vertex record of the cell's edge e.
template <typename RecordFn>
__device__ __forceinline__ void triangle_step(uint32_t cs, uint32_t n_tri, uint32_t* __restrict__ out, RecordFn&& record_of) {
    for (uint32_t q = 0; q < n_tri * 3; ++q) out[q] = record_of(kMcTriEdges[cs][q]);
}

}  // namespace sdfv
