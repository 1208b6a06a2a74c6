// lattice_mesh_kernels.hip -- meshing a lattice of distances the caller sampled (include/sdfgrid.h, "Meshing a sampled lattice"),
// on gfx950: the positions of lattice points (so that a surface sampled on the device can be fed), the distances out of sample
// records, and the per-vertex normal from the lattice itself.  Nothing here evaluates an SDF.
//
// Shape.
//  * lattice_points, lattice_from_samples: one element per thread, memory order.
//  * lattice_normals[_zero_mat]: one thread per VERTEX of the compacted list, dense waves, as sdfprog_mesh_vertices.  A vertex
//    reads 48 distances: two per axis at each of the 8 corners of its cell.  The corners are visited in a loop over the four
//    (y, z) corner pairs that is not unrolled -- 12 loads in flight, the x interpolation done in the round -- and the y and z
//    interpolations fold in as the rounds complete, so that no more than three partial triples are live.  The lanes of a wave
//    are neighbours on the surface (the vertex list is in lattice order), so their taps share cache lines.
// Every float step is one rounded f32 operation (the translation unit is built with -ffp-contract=off).  The central
// difference's division by 1.0f or 2.0f is written as a multiplication by 1.0f or 0.5f: both are exact scalings, bit for bit
// the same.
// The kernels carry C names: tests and profiles find them under the same symbol whatever the toolchain mangles.
#include "lattice_mesh_kernels.h"

#include "kernel_common.h"
#include "mesh_lattice.h"

namespace sdfv {

namespace {

// Component `a` of the lattice gradient at the lattice point with flat index `at` and index q along that axis: the central
// difference, one-sided at the border.  `cells` >= 1, so hi - lo is 1 or 2 and both taps are lattice points.
__device__ __forceinline__ float lattice_gradient(const float* __restrict__ dist, uint32_t at, uint32_t q, uint32_t cells,
                                                  uint32_t stride) {
    const uint32_t hi = min(q + 1u, cells), lo = max(q, 1u) - 1u;
    const float d = dist[at + (hi - q) * stride] - dist[at - (q - lo) * stride];
    return d * (hi - lo == 2u ? 0.5f : 1.0f);
}

__device__ __forceinline__ float lerp(float a, float b, float t) { return a + t * (b - a); }

template <bool ZERO_MAT>
__device__ __forceinline__ void vertex_normal(const float* __restrict__ dist, const MeshGrid& g, float* __restrict__ vertices,
                                              uint32_t n) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    float* v = vertices + (size_t)i * 12;
    const float p[3] = {v[0], v[1], v[2]};
    const Lattice L(g);
    uint32_t c[3];
    float f[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float cells = (float)g.cells[a];
        float u = (p[a] - g.bb_min[a]) / g.bb_size[a] * cells;
        u = u > 0.0f ? u : 0.0f;  // also a NaN and -0
        u = u < cells ? u : cells;
        c[a] = min((uint32_t)floorf(u), g.cells[a] - 1u);
        f[a] = u - (float)c[a];
    }
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
    if (ZERO_MAT) {  // Vertex::default()'s material; the record's second half starts 8-byte aligned
        float2* m = reinterpret_cast<float2*>(v + 6);
        m[0] = m[1] = m[2] = make_float2(0.0f, 0.0f);
    }
}

}  // namespace

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
    vertex_normal<false>(dist, g, vertices, n);
}

__global__ __launch_bounds__(kBlock) void lattice_normals_zero_mat(const float* __restrict__ dist, MeshGrid g,
                                                                   float* __restrict__ vertices, uint32_t n) {
    vertex_normal<true>(dist, g, vertices, n);
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
