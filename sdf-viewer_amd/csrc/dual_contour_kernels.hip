// dual_contour_kernels.hip -- Meshers::DualContouringParticleBasedMinimization on gfx950 (include/sdfgrid.h, "Dual contouring"):
// one vertex per lattice CELL the surface passes through, placed where the tangent planes of the cell's crossing edges meet, and
// one quad per crossing edge between the four cells around it.  Nothing here evaluates an SDF: the lattice distances, the edge
// masks, the point scan and the Hermite records (position + normal per crossing edge) are the marching-cubes extractor's, for the
// demo tree and for SDF programs alike, and the normals at the solved vertices come from the SDF's own vertex-list kernel.
//
// Shape.  Under 1 % of the cells are active at 256 cells per axis, so the solve does not run under a sparse mask over all cells:
//  * dc_cell_count / dc_edge_count: one cell / one lattice point per thread, a 0/1 and a 0..3 for the two scans;
//  * dc_cell_list: one cell per thread, the active ones write their id to their scanned slot -- the compacted list;
//  * dc_solve: one thread per ENTRY of that list, dense waves.  The <= 12 Hermite records are gathered twice through
//    edge_record of mesh_lattice.h (once for the mass point, once for the normal equations: the second pass hits the cache) and
//    accumulated as they arrive -- nine sums, no per-thread array; then 24 steps on nine floats of state;
//  * dc_quads: one lattice point per thread, those with an interior crossing edge look up four vertex ids in the cell scan.
// The kernels carry C names: tests and profiles find them under the same symbol whatever the toolchain mangles.
#include "dual_contour_kernels.h"

#include "kernel_common.h"
#include "mesh_lattice.h"

namespace sdfv {

namespace {

// The cell's crossing edges as 12 bits, bit e = 4 * axis + u + 2 * v (the marching-cubes table's numbering): the edge along
// `axis` that starts at the corner offset by u along the lower and v along the higher of the two other axes.  Seven of the cell's
// eight corners own one of its edges; their masks are read once each.
__device__ __forceinline__ uint32_t cell_edges(const Lattice& L, const uint8_t* __restrict__ mask, size_t origin) {
    const size_t sy = L.nx, sz = (size_t)L.nx * L.ny;
    const uint32_t m000 = mask[origin], m100 = mask[origin + 1], m010 = mask[origin + sy], m110 = mask[origin + sy + 1];
    const uint32_t m001 = mask[origin + sz], m101 = mask[origin + sz + 1], m011 = mask[origin + sz + sy];
    return (m000 & 1u) | (m010 & 1u) << 1 | (m001 & 1u) << 2 | (m011 & 1u) << 3 |                          // along x: u = y, v = z
           (m000 >> 1 & 1u) << 4 | (m100 >> 1 & 1u) << 5 | (m001 >> 1 & 1u) << 6 | (m101 >> 1 & 1u) << 7 |  // along y: u = x, v = z
           (m000 >> 2 & 1u) << 8 | (m100 >> 2 & 1u) << 9 | (m010 >> 2 & 1u) << 10 | (m110 >> 2 & 1u) << 11; // along z: u = x, v = y
}

// Those of the point's crossing +axis edges (bits of m) that have all four cells around them
__device__ __forceinline__ uint32_t interior_edges(const MeshGrid& g, uint32_t m, uint32_t i, uint32_t j, uint32_t k) {
    const bool x = i >= 1 && i < g.cells[0], y = j >= 1 && j < g.cells[1], z = k >= 1 && k < g.cells[2];
    return m & ((y && z ? 1u : 0u) | (x && z ? 2u : 0u) | (x && y ? 4u : 0u));
}

__device__ __forceinline__ float min_f(float a, float b) { return b < a ? b : a; }  // the program table's min and max
__device__ __forceinline__ float max_f(float a, float b) { return a < b ? b : a; }

// f(record id) for every crossing edge of the cell, e = 0..11 ascending
template <typename F>
__device__ __forceinline__ void for_each_record(const Lattice& L, uint32_t edges, size_t origin, const uint8_t* __restrict__ mask,
                                                const uint32_t* __restrict__ point_first, F&& f) {
#pragma unroll
    for (int e = 0; e < 12; ++e)
        if (edges >> e & 1u) f(edge_record(L, origin, e, mask, point_first));
}

}  // namespace

extern "C" {

__global__ __launch_bounds__(kBlock) void dc_cell_count(MeshGrid g, const uint8_t* __restrict__ mask,
                                                        uint32_t* __restrict__ count) {
    const Lattice L(g);
    const uint32_t c = blockIdx.x * kBlock + threadIdx.x;
    if (c >= L.cells()) return;
    uint32_t i, j, k;
    L.uncell(c, i, j, k);
    count[c] = cell_edges(L, mask, L.flat(i, j, k)) != 0u ? 1u : 0u;
}

__global__ __launch_bounds__(kBlock) void dc_edge_count(MeshGrid g, const uint8_t* __restrict__ mask,
                                                        uint32_t* __restrict__ count) {
    const Lattice L(g);
    const uint32_t v = blockIdx.x * kBlock + threadIdx.x;
    if (v >= L.points()) return;
    uint32_t i, j, k;
    L.unflat(v, i, j, k);
    count[v] = __popc(interior_edges(g, mask[v], i, j, k));
}

// The last element's offset + count = the total; one thread, so the host needs a single 12-byte read-back.
__global__ void dc_totals(MeshGrid g, const uint8_t* mask, const uint32_t* point_first, const uint32_t* cell_first,
                          const uint32_t* quad_first, uint32_t* totals) {
    const Lattice L(g);
    const uint32_t last = L.points() - 1;
    totals[0] = point_first[last] + __popc((uint32_t)mask[last]);
    totals[1] = cell_first[L.cells() - 1] + (cell_edges(L, mask, L.flat(L.cx - 1, L.cy - 1, L.cz - 1)) != 0u ? 1u : 0u);
    totals[2] = quad_first[last] + __popc(interior_edges(g, mask[last], L.nx - 1, L.ny - 1, L.nz - 1));
}

// cell_first[c + 1] != cell_first[c] would do as well, but the last cell has no successor: the mask test is the count's own.
__global__ __launch_bounds__(kBlock) void dc_cell_list(MeshGrid g, const uint8_t* __restrict__ mask,
                                                       const uint32_t* __restrict__ cell_first, uint32_t* __restrict__ list) {
    const Lattice L(g);
    const uint32_t c = blockIdx.x * kBlock + threadIdx.x;
    if (c >= L.cells()) return;
    uint32_t i, j, k;
    L.uncell(c, i, j, k);
    if (cell_edges(L, mask, L.flat(i, j, k)) != 0u) list[cell_first[c]] = c;
}

// The vertex of one active cell (sdfgrid.h, "Dual contouring", vertices): mass point of the crossing edges' positions, gradient
// descent on the sum of squared plane distances from there, clamped to the cell.
__global__ __launch_bounds__(kBlock) void dc_solve(MeshGrid g, const float4* __restrict__ hermite, const uint8_t* __restrict__ mask,
                                                   const uint32_t* __restrict__ point_first, const uint32_t* __restrict__ list,
                                                   uint32_t n, float* __restrict__ vertices) {
    const Lattice L(g);
    const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
    if (t >= n) return;
    uint32_t i, j, k;
    L.uncell(list[t], i, j, k);
    const size_t origin = L.flat(i, j, k);
    const uint32_t edges = cell_edges(L, mask, origin);
    // mass point
    float cx = 0.0f, cy = 0.0f, cz = 0.0f;
    for_each_record(L, edges, origin, mask, point_first, [&](uint32_t id) {
        const float4 p = hermite[(size_t)id * 3];
        cx += p.x; cy += p.y; cz += p.z;
    });
    const float m = (float)__popc(edges);
    cx = cx / m; cy = cy / m; cz = cz / m;
    // normal equations of sum (n . (x - p))^2 about the mass point, over the edges with a usable normal
    float mxx = 0.0f, mxy = 0.0f, mxz = 0.0f, myy = 0.0f, myz = 0.0f, mzz = 0.0f, gx = 0.0f, gy = 0.0f, gz = 0.0f;
    uint32_t used = 0;
    for_each_record(L, edges, origin, mask, point_first, [&](uint32_t id) {
        const float4 p = hermite[(size_t)id * 3], q = hermite[(size_t)id * 3 + 1];
        const float nx = p.w, ny = q.x, nz = q.y;
        const float w = nx * nx + ny * ny + nz * nz;
        if (w > 0.5f && w < 2.0f) {  // leaves NaN and zero normals out
            const float rx = p.x - cx, ry = p.y - cy, rz = p.z - cz;
            const float b = (nx * rx + ny * ry) + nz * rz;
            mxx += nx * nx; mxy += nx * ny; mxz += nx * nz;
            myy += ny * ny; myz += ny * nz; mzz += nz * nz;
            gx += nx * b; gy += ny * b; gz += nz * b;
            ++used;
        }
    });
    float yx = 0.0f, yy = 0.0f, yz = 0.0f;
    if (used != 0) {
        const float s = 1.0f / (float)used;
#pragma unroll 1
        for (int step = 0; step < 24; ++step) {
            const float tx = gx - ((mxx * yx + mxy * yy) + mxz * yz);
            const float ty = gy - ((mxy * yx + myy * yy) + myz * yz);
            const float tz = gz - ((mxz * yx + myz * yy) + mzz * yz);
            yx = yx + s * tx; yy = yy + s * ty; yz = yz + s * tz;
        }
    }
    float lx, ly, lz, hx, hy, hz;
    lattice_position(g, i, j, k, lx, ly, lz);
    lattice_position(g, i + 1, j + 1, k + 1, hx, hy, hz);
    float* o = vertices + (size_t)t * 12;
    o[0] = max_f(lx, min_f(cx + yx, hx));
    o[1] = max_f(ly, min_f(cy + yy, hy));
    o[2] = max_f(lz, min_f(cz + yz, hz));
}

// Two triangles per interior crossing edge: the vertices of the four cells around it, counter-clockwise seen from outside.
__global__ __launch_bounds__(kBlock) void dc_quads(MeshGrid g, const float* __restrict__ dist, const uint8_t* __restrict__ mask,
                                                   const uint32_t* __restrict__ quad_first, const uint32_t* __restrict__ cell_first,
                                                   uint32_t* __restrict__ indices) {
    const Lattice L(g);
    const uint32_t v = blockIdx.x * kBlock + threadIdx.x;
    if (v >= L.points()) return;
    uint32_t idx[3];
    L.unflat(v, idx[0], idx[1], idx[2]);
    const uint32_t m = interior_edges(g, mask[v], idx[0], idx[1], idx[2]);
    if (m == 0) return;
    const bool outside0 = dist[v] >= 0.0f;
    const uint32_t cell_stride[3] = {1, L.cx, L.cx * L.cy};
    const uint32_t here = (idx[2] * L.cy + idx[1]) * L.cx + idx[0];  // the cell whose lowest corner is this point
    uint2* out = reinterpret_cast<uint2*>(indices) + (size_t)quad_first[v] * 3;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        if (!(m & (1u << a))) continue;
        const int o0 = a == 0 ? 1 : 0, o1 = a == 2 ? 1 : 2;  // the two other axes, increasing
        const uint32_t q0 = cell_first[here - cell_stride[o0] - cell_stride[o1]], q1 = cell_first[here - cell_stride[o1]],
                       q2 = cell_first[here], q3 = cell_first[here - cell_stride[o0]];
        const bool flip = (a == 1) != outside0;
        out[0] = make_uint2(q0, flip ? q2 : q1);
        out[1] = make_uint2(flip ? q1 : q2, q0);
        out[2] = flip ? make_uint2(q3, q2) : make_uint2(q2, q3);
        out += 3;
    }
}

}  // extern "C"

hipError_t launch_dc_count(const MeshGrid& g, const MeshWork& w, uint32_t* totals_dev, hipStream_t stream) {
    if (!w.quad_first) return hipErrorInvalidValue;
    if (hipError_t e = launch_mesh_edge_masks(g, w, stream); e != hipSuccess) return e;  // also checks the grid
    const size_t n_points = g.n_points(), n_cells = g.n_cells();
    hipLaunchKernelGGL(dc_cell_count, dim3(blocks_for(n_cells)), dim3(kBlock), 0, stream, g, w.point_mask, w.cell_first);
    if (hipError_t e = mesh_exclusive_scan(w, w.cell_first, n_cells, stream); e != hipSuccess) return e;
    hipLaunchKernelGGL(dc_edge_count, dim3(blocks_for(n_points)), dim3(kBlock), 0, stream, g, w.point_mask, w.quad_first);
    if (hipError_t e = mesh_exclusive_scan(w, w.quad_first, n_points, stream); e != hipSuccess) return e;
    hipLaunchKernelGGL(dc_totals, dim3(1), dim3(1), 0, stream, g, w.point_mask, w.point_first, w.cell_first, w.quad_first,
                       totals_dev);
    return hipGetLastError();
}

hipError_t launch_dc_vertices(const MeshGrid& g, const MeshWork& w, const sdfv_vertex* hermite, uint32_t* cell_list,
                              sdfv_vertex* vertices, size_t n_vertices, hipStream_t stream) {
    if (n_vertices == 0) return hipSuccess;
    if (!hermite || !cell_list || !vertices || n_vertices > 0xffffffffull || ((uintptr_t)hermite & 15)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(dc_cell_list, dim3(blocks_for(g.n_cells())), dim3(kBlock), 0, stream, g, w.point_mask, w.cell_first, cell_list);
    hipLaunchKernelGGL(dc_solve, dim3(blocks_for(n_vertices)), dim3(kBlock), 0, stream, g, reinterpret_cast<const float4*>(hermite),
                       w.point_mask, w.point_first, cell_list, (uint32_t)n_vertices, reinterpret_cast<float*>(vertices));
    return hipGetLastError();
}

hipError_t launch_dc_quads(const MeshGrid& g, const MeshWork& w, uint32_t* indices, hipStream_t stream) {
    if (indices)
        hipLaunchKernelGGL(dc_quads, dim3(blocks_for(g.n_points())), dim3(kBlock), 0, stream, g, w.dist, w.point_mask, w.quad_first,
                           w.cell_first, indices);
    return hipGetLastError();
}

}  // namespace sdfv
