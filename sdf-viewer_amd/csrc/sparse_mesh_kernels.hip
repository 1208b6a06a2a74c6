// sparse_mesh_kernels.hip -- sparse marching cubes over SDF programs on gfx950 (include/sdfgrid.h, "SDF programs: sparse
// meshing"): the program is evaluated only where a 1-Lipschitz distance cannot rule the surface out.
//
// Shape.  As in program_mesh_kernels.hip the interpreter costs one program run per WAVE, so nothing evaluates under a sparse
// mask: both evaluating kernels run over compact lists, one element per thread, every lane but the last wave's tail live.
//  * sdfprog_sparse_refine: one CHILD block per thread (8 per block of the list), distance only at its centre lattice point,
//    kept iff !(|d| > threshold); sparse_compact moves the survivors up behind an exclusive scan -- no atomics, the order is the
//    header's.  One launch per level; the host reads one count per level.
//  * sdfprog_sparse_bricks: thread t has lattice point t % 125 of brick t / 125: all 5^3 points of a brick, its upper faces
//    included, because a pruned neighbour would leave them unknown.  Distances brick-major.
//  * sparse_brick_edges, sparse_brick_positions, sparse_brick_triangles: the SDF-free steps of mesh_steps.h (edge_mask_step,
//    edge_vertex_step, triangle_step: the very code mesh_kernels.hip runs) over BrickLayout, which says what thread t's point
//    is in the brick-major arrays and which edges it owns.  sparse_brick_neighbours, sparse_brick_cells: the brick route's own.
//    A brick owns the points with local index < 4 per axis (<= 4 where it is
//    the box's last brick), and the edges that start there; a cell on a brick's upper faces reads the records of up to seven
//    neighbours, which sparse_brick_neighbours has looked up once per brick by binary search in the brick list (sorted by Morton
//    key; a directory of (cells / 4)^3 words would be 4 GiB at 4096 cells).  A cell whose crossing edge has no owner among the
//    bricks (the program broke its Lipschitz promise) emits nothing: no index is ever out of range.
// The two evaluating kernels are program_mesh_device.h's definitions (SDFV_PROGRAM_KERNEL_sparse_refine, _sparse_bricks) with the
// interpreter as the evaluator; a handle compiled with SDFV_COMPILE_MESH brings the same definitions over that program's own, and
// ProgramKernels::launch hands either the one argument array its launcher builds.
// A block is its Morton key in units of its own side, x the lowest bit; keys are below 2^30 (1024 bricks per axis at the most).
// The kernels carry C names: tests and profiles find them under the same symbol whatever the toolchain mangles.
#include "sparse_mesh_kernels.h"

#include "kernel_common.h"
#include "mesh_steps.h"
#include "program_kernels.h"
#include "program_mesh_device.h"

namespace sdfv {

namespace {

constexpr uint32_t kNoBrick = 0xffffffffu;

// a 10-bit coordinate -> every third bit of a Morton key (gather3 of program_mesh_device.h back)
__device__ __forceinline__ uint32_t spread3(uint32_t x) {
    x &= 0x000003ffu;
    x = (x ^ (x << 16)) & 0x030000ffu;
    x = (x ^ (x << 8)) & 0x0300f00fu;
    x = (x ^ (x << 4)) & 0x030c30c3u;
    x = (x ^ (x << 2)) & 0x09249249u;
    return x;
}

// index of the brick with this key, or kNoBrick: the list is sorted
__device__ __forceinline__ uint32_t find_brick(const uint32_t* __restrict__ bricks, uint32_t n, uint32_t key) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (bricks[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo < n && bricks[lo] == key ? lo : kNoBrick;
}

// Thread t's point of the brick-major arrays (mesh_steps.h).  A brick owns the points with local index < 4 per axis (<= 4 where
// it is the box's last brick on that axis), and of an owned point the edges towards a local index <= 4: the +axis neighbour of
// such a point is one of the brick's own 125.  last = bricks per axis - 1.
struct BrickLayout {
    const uint32_t* __restrict__ bricks;
    uint32_t last;
    uint32_t stride[3] = {1u, 5u, 25u};
    __device__ __forceinline__ LatticePoint point(uint32_t t) const {
        uint32_t b, lx, ly, lz;
        unbrick(t, b, lx, ly, lz);
        const uint32_t key = bricks[b];
        const bool owned = (lx < 4u || gather3(key) == last) && (ly < 4u || gather3(key >> 1) == last) &&
                           (lz < 4u || gather3(key >> 2) == last);
        LatticePoint p;
        p.idx[0] = gather3(key) * 4u + lx;
        p.idx[1] = gather3(key >> 1) * 4u + ly;
        p.idx[2] = gather3(key >> 2) * 4u + lz;
        p.edges = owned ? (lx < 4u ? 1u : 0u) | (ly < 4u ? 2u : 0u) | (lz < 4u ? 4u : 0u) : 0u;
        return p;
    }
};

// The cube case of cell (cx, cy, cz) of a brick whose distances start at d.
__device__ __forceinline__ uint32_t brick_cell_case(const float* __restrict__ d, uint32_t cx, uint32_t cy, uint32_t cz) {
    return cube_case(d + (cz * 5u + cy) * 5u + cx, 5u, 25u);
}

// Does edge e of a cell with cube case cs cross?  From the corners' sides, not from the edge masks as cell_edges of
// dual_contour_kernels.hip has it: a brick's masks hold its OWN edges only, and those of an upper-face cell are other bricks'.
__device__ __forceinline__ bool edge_crosses(uint32_t cs, int e) {
    const CellEdge c = cell_edge(e);
    const uint32_t start = c.dx | c.dy << 1 | c.dz << 2;
    return (((cs >> start) ^ (cs >> (start | (1u << c.axis)))) & 1u) != 0;
}

// Where the record of edge e of cell (cx, cy, cz) of brick `self` (whose key the caller has loaded) is kept: the slot
// of its owning point in the brick-major arrays, or kNoBrick when the owner is no brick.  The edge starts at the cell's corner
// cell_edge(e) names; a local index of 4 belongs to the next brick on that axis unless this one is the box's last.
__device__ __forceinline__ bool next_brick(uint32_t& l, uint32_t& b, uint32_t last) {
    if (l != 4u || b >= last) return false;
    l = 0;
    b += 1;
    return true;
}
__device__ __forceinline__ uint32_t edge_owner_slot(const uint32_t* __restrict__ neighbours, uint32_t last, uint32_t self,
                                                    uint32_t key, uint32_t cx, uint32_t cy, uint32_t cz, int e) {
    const CellEdge c = cell_edge(e);
    uint32_t lx = cx + c.dx, ly = cy + c.dy, lz = cz + c.dz;
    uint32_t bx = gather3(key), by = gather3(key >> 1), bz = gather3(key >> 2);
    const bool fx = next_brick(lx, bx, last), fy = next_brick(ly, by, last), fz = next_brick(lz, bz, last);
    uint32_t owner = self;
    if (fx || fy || fz) {
        owner = neighbours[self * 8u + ((fx ? 1u : 0u) | (fy ? 2u : 0u) | (fz ? 4u : 0u))];
        if (owner == kNoBrick) return kNoBrick;
    }
    return owner * kBrickPoints + (lz * 5u + ly) * 5u + lx;
}

}  // namespace

// the two evaluating kernels: program_mesh_device.h's definitions with the interpreter as the evaluator
#define SDFV_EVAL_ONCE(ops, n_ops) prog::Interpreter{ops, n_ops}
SDFV_PROGRAM_KERNEL_sparse_refine(sdfprog_sparse_refine)
SDFV_PROGRAM_KERNEL_sparse_bricks(sdfprog_sparse_bricks)

extern "C" {

// survivors up, in order; the last thread leaves their number
__global__ __launch_bounds__(kBlock) void sparse_compact(const uint32_t* __restrict__ cand, const uint32_t* __restrict__ pos,
                                                         uint32_t n, uint32_t* __restrict__ list, uint32_t* __restrict__ kept) {
    const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
    if (t >= n) return;
    const uint32_t c = cand[t], at = pos[t];
    if (c & kSparseKept) list[at] = c & ~kSparseKept;
    if (t == n - 1) *kept = at + (c >> 31);
}

// Which of the point's three +axis edges the brick owns and cross; count -> scan input.  n = 125 * bricks; thread n writes the
// scan's extra entry.  last = bricks per axis - 1.
__global__ __launch_bounds__(kBlock) void sparse_brick_edges(uint32_t last, const uint32_t* __restrict__ bricks, uint32_t n,
                                                             const float* __restrict__ dist, uint8_t* __restrict__ mask,
                                                             uint32_t* __restrict__ count) {
    const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
    if (t > n) return;
    if (t == n) {
        count[n] = 0;
        return;
    }
    edge_mask_step(BrickLayout{bricks, last}, t, dist, mask, count);
}

// The up to seven bricks whose points a brick's upper-face cells refer to: neighbours[8 * b + dir] = index of the brick at
// offset (dir & 1, dir >> 1 & 1, dir >> 2) from brick b, or kNoBrick; entry 0 is b itself.  One binary search per entry, in the
// brick list, which the refinement leaves sorted by key.  n = 8 * bricks.
__global__ __launch_bounds__(kBlock) void sparse_brick_neighbours(uint32_t last, const uint32_t* __restrict__ bricks,
                                                                  uint32_t n_bricks, uint32_t* __restrict__ neighbours) {
    const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
    if (t >= n_bricks * 8u) return;
    const uint32_t b = t >> 3, key = bricks[b];
    const uint32_t bx = gather3(key) + (t & 1u), by = gather3(key >> 1) + ((t >> 1) & 1u), bz = gather3(key >> 2) + ((t >> 2) & 1u);
    uint32_t at = b;
    if (t & 7u)
        at = bx > last || by > last || bz > last ? kNoBrick
                                                 : find_brick(bricks, n_bricks, spread3(bx) | (spread3(by) << 1) | (spread3(bz) << 2));
    neighbours[t] = at;
}

// Triangles per cell: the table's, or none where a crossing edge of the cell has no owner among the bricks.  n = 64 * bricks.
__global__ __launch_bounds__(kBlock) void sparse_brick_cells(uint32_t last, const uint32_t* __restrict__ bricks, uint32_t n_bricks,
                                                             const uint32_t* __restrict__ neighbours,
                                                             const float* __restrict__ dist, uint32_t* __restrict__ count) {
    const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
    const uint32_t n = n_bricks * kBrickCells;
    if (t > n) return;
    if (t == n) {
        count[n] = 0;
        return;
    }
    const uint32_t b = t >> 6;
    const uint32_t cx = t & 3u, cy = (t >> 2) & 3u, cz = (t >> 4) & 3u;
    const uint32_t cs = brick_cell_case(dist + (size_t)b * kBrickPoints, cx, cy, cz);
    uint32_t n_tri = kMcTriCount[cs];
    if (n_tri != 0 && (cx == 3u || cy == 3u || cz == 3u)) {  // only an upper-face cell has edges of other owners
        const uint32_t key = bricks[b];
#pragma unroll
        for (int e = 0; e < 12; ++e)
            if (edge_crosses(cs, e) && edge_owner_slot(neighbours, last, b, key, cx, cy, cz, e) == kNoBrick) n_tri = 0;
    }
    count[t] = n_tri;
}

// One vertex per owned crossing edge, bricks in list order, points in local order, then axis order: edge_position with the
// point's lattice index in the whole box.  n = 125 * bricks.
__global__ __launch_bounds__(kBlock) void sparse_brick_positions(MeshGrid g, const uint32_t* __restrict__ bricks, uint32_t n,
                                                                 const float* __restrict__ dist, const uint8_t* __restrict__ mask,
                                                                 const uint32_t* __restrict__ first, float* __restrict__ vertices) {
    const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
    if (t >= n) return;
    edge_vertex_step(g, BrickLayout{bricks, g.cells[0] / 4u - 1u}, t, dist, mask, first, StorePosition{vertices});
}

__global__ __launch_bounds__(kBlock) void sparse_brick_triangles(uint32_t last, const uint32_t* __restrict__ bricks,
                                                                 uint32_t n_bricks, const uint32_t* __restrict__ neighbours,
                                                                 const float* __restrict__ dist,
                                                                 const uint8_t* __restrict__ mask,
                                                                 const uint32_t* __restrict__ point_first,
                                                                 const uint32_t* __restrict__ cell_first,
                                                                 uint32_t* __restrict__ indices) {
    const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
    if (t >= n_bricks * kBrickCells) return;
    const uint32_t begin = cell_first[t], n_tri = cell_first[t + 1] - begin;  // 0 too where sparse_brick_cells refused the cell
    if (n_tri == 0) return;
    const uint32_t b = t >> 6;
    const uint32_t cx = t & 3u, cy = (t >> 2) & 3u, cz = (t >> 4) & 3u;
    const uint32_t cs = brick_cell_case(dist + (size_t)b * kBrickPoints, cx, cy, cz);
    const uint32_t key = bricks[b];
    triangle_step(cs, n_tri, indices + (size_t)begin * 3, [&](int e) {
        const uint32_t slot = edge_owner_slot(neighbours, last, b, key, cx, cy, cz, e);  // a brick's: sparse_brick_cells has looked
        return slot == kNoBrick ? 0u : owner_record(slot, (uint32_t)e >> 2, mask, point_first);
    });
}

}  // extern "C"

namespace {
bool sparse_grid(const MeshGrid& g) {  // one power of two, 4 .. 4096, on every axis
    const uint32_t n = g.cells[0];
    return n >= 4 && n <= 4096 && (n & (n - 1)) == 0 && g.cells[1] == n && g.cells[2] == n;
}
}  // namespace

hipError_t launch_sparse_refine(const sdfv_prog_op* ops, uint32_t n_ops, const MeshGrid& g, uint32_t shift, float threshold,
                                const SparseWork& w, uint32_t n_parents, uint32_t* kept_dev, const ProgramKernels& k,
                                hipStream_t stream) {
    if (!sparse_grid(g) || n_parents == 0 || n_parents > 0x10000000u || shift < 2 || (2u << shift) > g.cells[0])
        return hipErrorInvalidValue;  // children of 4 .. cells / 2 cells, and 8 of them per parent in 32 bits
    uint32_t n = n_parents * 8u;
    MeshGrid grid = g;
    const uint32_t* parents = w.list;
    uint32_t *cand = w.cand, *pos = w.pos;
    void* params[] = {&ops, &n_ops, &grid, &parents, &n, &shift, &threshold, &cand, &pos};
    if (hipError_t e = k.launch(kKernelSparseRefine, (const void*)sdfprog_sparse_refine, dim3(blocks_for(n)), dim3(kBlock), params, stream);
        e != hipSuccess)
        return e;
    if (hipError_t e = mesh_exclusive_scan(w.mesh, w.pos, n, stream); e != hipSuccess) return e;
    hipLaunchKernelGGL(sparse_compact, dim3(blocks_for(n)), dim3(kBlock), 0, stream, w.cand, w.pos, n, w.list, kept_dev);
    return hipGetLastError();
}

hipError_t launch_sparse_brick_lattice(const sdfv_prog_op* ops, uint32_t n_ops, const MeshGrid& g, const SparseWork& w,
                                       uint32_t n_bricks, const ProgramKernels& k, hipStream_t stream) {
    if (!sparse_grid(g) || n_bricks == 0 || (uint64_t)n_bricks * kBrickPoints >= 0xffffffffull) return hipErrorInvalidValue;
    uint32_t n = n_bricks * kBrickPoints;
    MeshGrid grid = g;
    const uint32_t* bricks = w.list;
    float* dist = w.mesh.dist;
    void* params[] = {&ops, &n_ops, &grid, &bricks, &n, &dist};
    return k.launch(kKernelSparseBricks, (const void*)sdfprog_sparse_bricks, dim3(blocks_for(n)), dim3(kBlock), params, stream);
}

hipError_t launch_sparse_count(const MeshGrid& g, const SparseWork& w, uint32_t n_bricks, hipStream_t stream) {
    if (!sparse_grid(g) || n_bricks == 0 || (uint64_t)n_bricks * kBrickPoints >= 0xffffffffull) return hipErrorInvalidValue;
    const uint32_t last = g.cells[0] / 4u - 1u, n_points = n_bricks * kBrickPoints, n_cells = n_bricks * kBrickCells;
    hipLaunchKernelGGL(sparse_brick_edges, dim3(blocks_for((uint64_t)n_points + 1)), dim3(kBlock), 0, stream, last, w.list, n_points,
                       w.mesh.dist, w.mesh.point_mask, w.mesh.point_first);
    if (hipError_t e = mesh_exclusive_scan(w.mesh, w.mesh.point_first, (size_t)n_points + 1, stream); e != hipSuccess) return e;
    hipLaunchKernelGGL(sparse_brick_neighbours, dim3(blocks_for((uint64_t)n_bricks * 8)), dim3(kBlock), 0, stream, last, w.list,
                       n_bricks, w.neighbours);
    hipLaunchKernelGGL(sparse_brick_cells, dim3(blocks_for((uint64_t)n_cells + 1)), dim3(kBlock), 0, stream, last, w.list, n_bricks,
                       w.neighbours, w.mesh.dist, w.mesh.cell_first);
    return mesh_exclusive_scan(w.mesh, w.mesh.cell_first, (size_t)n_cells + 1, stream);
}

hipError_t launch_sparse_positions(const MeshGrid& g, const SparseWork& w, uint32_t n_bricks, sdfv_vertex* vertices, size_t n,
                                   hipStream_t stream) {
    if (n == 0) return hipSuccess;
    if (!vertices || n_bricks == 0) return hipErrorInvalidValue;
    const uint32_t n_points = n_bricks * kBrickPoints;
    hipLaunchKernelGGL(sparse_brick_positions, dim3(blocks_for(n_points)), dim3(kBlock), 0, stream, g, w.list, n_points, w.mesh.dist,
                       w.mesh.point_mask, w.mesh.point_first, reinterpret_cast<float*>(vertices));
    return hipGetLastError();
}

hipError_t launch_sparse_triangles(const MeshGrid& g, const SparseWork& w, uint32_t n_bricks, uint32_t* indices,
                                   hipStream_t stream) {
    if (indices && n_bricks)
        hipLaunchKernelGGL(sparse_brick_triangles, dim3(blocks_for((uint64_t)n_bricks * kBrickCells)), dim3(kBlock), 0, stream,
                           g.cells[0] / 4u - 1u, w.list, n_bricks, w.neighbours, w.mesh.dist, w.mesh.point_mask, w.mesh.point_first, w.mesh.cell_first,
                           indices);
    return hipGetLastError();
}

}  // namespace sdfv
