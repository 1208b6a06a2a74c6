// sparse_mesh_kernels.h -- launch interface of sparse marching cubes over SDF programs (see sparse_mesh_kernels.hip;
// include/sdfgrid.h, "SDF programs: sparse meshing"): the block refinement, the brick lattice, and counting, positions and
// triangles over bricks.  The vertex attributes are program_mesh_kernels.h's launch_program_vertex_normals, the scans
// mesh_kernels.h's mesh_exclusive_scan over the MeshWork a SparseWork holds.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#if defined(__HIPCC_RTC__)  // the run-time compiler is handed the headers by name (program_compile.hip)
#include "sdfgrid.h"
#else
#include "../../include/sdfgrid.h"
#endif
#include "mesh_kernels.h"

namespace sdfv {

constexpr uint32_t kBrickPoints = 125;  // 5^3 lattice points of a leaf block of 4^3 cells
constexpr uint32_t kBrickCells = 64;

// Device scratch of one sparse extraction.  A block is its Morton key in units of its own side (x the lowest bit): the child
// order of the refinement is then key * 8 + child, and the surviving list stays sorted by key at every level.
struct SparseWork {
    uint32_t* list;         // the blocks of the current level, [n]; after the last level: the bricks
    uint32_t* cand;         // refinement: [8 * n] children, key | kept << 31
    uint32_t* pos;          // refinement: [8 * n] kept (0 / 1), then its exclusive scan
    uint32_t* neighbours;   // [8 * bricks] index of the brick at offset (dir & 1, dir >> 1 & 1, dir >> 2), or 0xffffffff
    // What the brick phase has in common with a dense extraction, brick-major (x fastest within a brick):
    //   dist [125 * bricks]; point_mask [125 * bricks], bit a: the brick owns the edge towards +axis a and it crosses;
    //   point_first [125 * bricks + 1] and cell_first [64 * bricks + 1], the last entry of each the total.
    // scan_tmp serves both phases; totals is one word, the survivors of a refinement level; quad_first stays NULL.
    MeshWork mesh;
};

#if !defined(__HIPCC_RTC__)  // (host only: the run-time compiler reads this header for the brick constants)
struct ProgramKernels;  // program_kernels.h
// g: `cells` on every axis, a power of two; ops: the DEVICE copy of the validated program; k: the kernels of a handle compiled
// with SDFV_COMPILE_MESH, or none (the interpreter's are launched, with the same grid, block and stream).
// One level: the 8 * n_parents children of w.list, blocks of 2^shift cells, are tested at their centre lattice point
// (kept iff !(|d| > threshold)) and the survivors replace w.list in order; *kept_dev receives their number.
hipError_t launch_sparse_refine(const sdfv_prog_op* ops, uint32_t n_ops, const MeshGrid& g, uint32_t shift, float threshold,
                                const SparseWork& w, uint32_t n_parents, uint32_t* kept_dev, const ProgramKernels& k,
                                hipStream_t stream);
// The program's distance at the 125 lattice points of every brick into w.dist.
hipError_t launch_sparse_brick_lattice(const sdfv_prog_op* ops, uint32_t n_ops, const MeshGrid& g, const SparseWork& w,
                                       uint32_t n_bricks, const ProgramKernels& k, hipStream_t stream);
// Edge masks of the owned points, the neighbour table, triangle counts of the cells, both scans (each over one entry more: the
// total).
hipError_t launch_sparse_count(const MeshGrid& g, const SparseWork& w, uint32_t n_bricks, hipStream_t stream);
// vertices[id].position of the n vertices launch_sparse_count counted.
hipError_t launch_sparse_positions(const MeshGrid& g, const SparseWork& w, uint32_t n_bricks, sdfv_vertex* vertices, size_t n,
                                   hipStream_t stream);
hipError_t launch_sparse_triangles(const MeshGrid& g, const SparseWork& w, uint32_t n_bricks, uint32_t* indices,
                                   hipStream_t stream);
#endif

}  // namespace sdfv
