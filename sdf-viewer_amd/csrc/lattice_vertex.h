// lattice_vertex.h -- the per-vertex pass over a lattice of distances (include/sdfgrid.h, "Meshing a sampled lattice", normal(p)),
// shared by the kernels that run it: lattice_mesh_kernels.hip (a caller's lattice: the normal, or the normal and the zero
// material) and grid_mesh_kernels.hip (a loaded grid's lattice: the normal and the grid's material, or the material alone).
// One statement of the cell a position falls into, so that "the nearest lattice point" of the material gather and the cell of
// the normal cannot drift apart.  Every float step is one rounded f32 operation (the translation units are built with
// -ffp-contract=off).  The central difference's division by 1.0f or 2.0f is written as a multiplication by 1.0f or 0.5f: both
// are exact scalings, bit for bit the same.
#pragma once

#include "kernel_common.h"
#include "mesh_lattice.h"

namespace sdfv {

namespace {

// Steps 1-2 of normal(p) along axis a: u = (p - bb_min) / bb_size * cells clamped to [0, cells], the cell c = min(floor(u),
// cells - 1) and the place f = u - c within it, f in [0, 1].  (Per axis and by value: called from the unrolled loop of the caller
// it compiles to the kernel that spelled the steps out.)
__device__ __forceinline__ uint32_t lattice_cell(const MeshGrid& g, int a, float p, float& f) {
    const float cells = (float)g.cells[a];
    float u = (p - g.bb_min[a]) / g.bb_size[a] * cells;
    u = u > 0.0f ? u : 0.0f;  // also a NaN and -0
    u = u < cells ? u : cells;
    const uint32_t c = min((uint32_t)floorf(u), g.cells[a] - 1u);
    f = u - (float)c;
    return c;
}

// Component `a` of the lattice gradient at the lattice point with flat index `at` and index q along that axis: the central
// difference, one-sided at the border.  `cells` >= 1, so hi - lo is 1 or 2 and both taps are lattice points.
__device__ __forceinline__ float lattice_gradient(const float* __restrict__ dist, uint32_t at, uint32_t q, uint32_t cells,
                                                  uint32_t stride) {
    const uint32_t hi = min(q + 1u, cells), lo = max(q, 1u) - 1u;
    const float d = dist[at + (hi - q) * stride] - dist[at - (q - lo) * stride];
    return d * (hi - lo == 2u ? 0.5f : 1.0f);
}

__device__ __forceinline__ float lerp(float a, float b, float t) { return a + t * (b - a); }

// What a vertex pass does with the six material words of a record once the normal is stored: nothing, or Vertex::default()'s
// zeros (the record's second half then starts 8-byte aligned: the extractor's own vertices).  grid_mesh_kernels.hip has a
// third.  `v` is the record, c and f the cell of its position and the place within it.
struct KeepMaterial {
    __device__ __forceinline__ void operator()(float*, const uint32_t*, const float*) const {}
};
struct ZeroMaterial {
    __device__ __forceinline__ void operator()(float* v, const uint32_t*, const float*) const {
        float2* m = reinterpret_cast<float2*>(v + 6);
        m[0] = m[1] = m[2] = make_float2(0.0f, 0.0f);
    }
};

// One thread per vertex of a list whose positions are written: the normal of the header's definition from `dist` over g's
// lattice, then `material`.  A vertex reads 48 distances: two per axis at each of the 8 corners of its cell.  The corners are
// visited in a loop over the four (y, z) corner pairs that is not unrolled -- 12 loads in flight, the x interpolation done in the
// round -- and the y and z interpolations fold in as the rounds complete, so that no more than three partial triples are live.
template <typename Material>
__device__ __forceinline__ void vertex_normal(const float* __restrict__ dist, const MeshGrid& g, float* __restrict__ vertices,
                                              uint32_t n, const Material& material) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    float* v = vertices + (size_t)i * 12;
    const float p[3] = {v[0], v[1], v[2]};
    const Lattice L(g);
    uint32_t c[3];
    float f[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) c[a] = lattice_cell(g, a, p[a], f[a]);
    const uint32_t sy = L.nx, sz = L.nx * L.ny;  // points() < 2^32: MeshGrid::launchable()
    float ey[3] = {0.0f, 0.0f, 0.0f}, ez[3] = {0.0f, 0.0f, 0.0f}, G[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll 1
    for (uint32_t t = 0; t < 4u; ++t) {  // the corner pairs (y, z) = (0,0), (1,0), (0,1), (1,1); t is wave-uniform
        const uint32_t qy = c[1] + (t & 1u), qz = c[2] + (t >> 1);
        const uint32_t at = (qz * L.ny + qy) * L.nx + c[0];
        float e[3];
        {
            const float x0 = lattice_gradient(dist, at, c[0], L.cx, 1u), x1 = lattice_gradient(dist, at + 1u, c[0] + 1u, L.cx, 1u);
            const float y0 = lattice_gradient(dist, at, qy, L.cy, sy), y1 = lattice_gradient(dist, at + 1u, qy, L.cy, sy);
            const float z0 = lattice_gradient(dist, at, qz, L.cz, sz), z1 = lattice_gradient(dist, at + 1u, qz, L.cz, sz);
            e[0] = lerp(x0, x1, f[0]);
            e[1] = lerp(y0, y1, f[0]);
            e[2] = lerp(z0, z1, f[0]);
        }
        if ((t & 1u) == 0u) {
#pragma unroll
            for (int a = 0; a < 3; ++a) ey[a] = e[a];
        } else if ((t & 2u) == 0u) {
#pragma unroll
            for (int a = 0; a < 3; ++a) ez[a] = lerp(ey[a], e[a], f[1]);
        } else {
#pragma unroll
            for (int a = 0; a < 3; ++a) G[a] = lerp(ez[a], lerp(ey[a], e[a], f[1]), f[2]);
        }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) G[a] = G[a] * ((float)g.cells[a] / g.bb_size[a]);
    const float s = (G[0] * G[0] + G[1] * G[1]) + G[2] * G[2];
    float nx = 0.0f, ny = 0.0f, nz = 0.0f;  // !(s > 0): the mesher's "unset" normal (meshers/mesh.rs:25-27)
    if (s > 0.0f) {
        const float inv = 1.0f / sqrtf(s);
        nx = G[0] * inv;
        ny = G[1] * inv;
        nz = G[2] * inv;
    }
    v[3] = nx;
    v[4] = ny;
    v[5] = nz;
    material(v, c, f);
}

}  // namespace

}  // namespace sdfv
