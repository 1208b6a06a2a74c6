// mesh_kernels.h -- cube-by-cube isosurface extraction over the unit-cube lattice the reference's meshers sample
// (src/sdf/meshers/isosurface.rs:16-66: MarchingCubes::<Signed>::new(max_voxels_per_axis) over ScalarSource /
// HermiteSource).  The extractor itself lives in the un-vendored `isosurface` crate; this is the build's own.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#if defined(__HIPCC_RTC__)  // the run-time compiler is handed the headers by name (program_compile.hip)
#include "sdfgrid.h"
#else
#include "../../include/sdfgrid.h"
#endif

namespace sdfv {

struct MeshGrid {
    uint32_t cells[3];     // cells per axis; lattice points = cells + 1
    float bb_min[3], bb_size[3];
    // host side (the kernels have mesh_lattice.h's Lattice): the sizes every launcher and the scratch layout go by
    size_t n_points() const { return (size_t)(cells[0] + 1) * (cells[1] + 1) * (cells[2] + 1); }
    size_t n_cells() const { return (size_t)cells[0] * cells[1] * cells[2]; }
    // what every launch of an extraction may assume, checked by its first launcher: cells on every axis, and lattice points a
    // kernel can index with 32 bits (their workgroups then fit one launch)
    bool launchable() const { return n_cells() != 0 && n_points() <= 0xffffffffull; }
};

struct MeshWork {           // device scratch of one extraction: sub-blocks of the calling thread's block (api_points_mesh.hip)
    float* dist;            // [points] ScalarSource at every lattice point
    uint32_t* point_first;  // [points] first vertex id of the point's edges (exclusive scan of the edge counts)
    uint8_t* point_mask;    // [points] bit a: the edge towards +axis a crosses the surface
    uint32_t* cell_first;   // [cells] first triangle of the cell (exclusive scan of the triangle counts); dual contouring: the
                            //         cell's vertex id (exclusive scan of a 0/1 per active cell)
    uint32_t* quad_first;   // [points] dual contouring only (NULL otherwise): first quad of the point's interior crossing edges
    void* scan_tmp;
    size_t scan_tmp_bytes;
    uint32_t* totals;       // [3] the counts the host reads back to allocate the output
};

#if !defined(__HIPCC_RTC__)  // (host only: the run-time compiler reads this header for MeshGrid)
size_t mesh_scan_tmp_bytes(size_t n);
// An extraction is six steps on one stream (five for the demo tree's marching cubes: see the end); the first and the fifth evaluate the SDF, the others do not and serve every kind of
// SDF (the demo tree here, SDF programs in program_mesh_kernels.hip) and both meshers (dual_contour_kernels.h has algorithm 4's
// own counting, solve and quads):
// 1. lattice distances into w.dist (the demo tree's).  Checks the grid (MeshGrid::launchable).
hipError_t launch_mesh_lattice(const sdfv_demo_params& prm, uint32_t sdf_id, const MeshGrid& g, const MeshWork& w,
                               hipStream_t stream);
// 2. edge masks, triangle counts, both scans.  Leaves the totals in totals_dev[0] (vertices), [1] (triangles).
hipError_t launch_mesh_count(const MeshGrid& g, const MeshWork& w, uint32_t* totals_dev, hipStream_t stream);
//    Its two parts, for an extractor that counts something else per cell (dual_contour_kernels.hip): edge masks + the point scan
//    (checks the grid too), and the in-place exclusive scan of n counts through w.scan_tmp (the brick route's scans too).
hipError_t launch_mesh_edge_masks(const MeshGrid& g, const MeshWork& w, hipStream_t stream);
hipError_t mesh_exclusive_scan(const MeshWork& w, uint32_t* counts, size_t n, hipStream_t stream);
// 3. (the host reads the totals and allocates)
// 4. positions: vertices[id].position of the n vertices step 2 counted, one per crossing edge in lattice then axis order, on the
//    edge by linear interpolation of its two distances.  Nothing else of a record is written.  The output vertices of marching
//    cubes, the Hermite records of dual contouring.
hipError_t launch_mesh_edge_positions(const MeshGrid& g, const MeshWork& w, sdfv_vertex* vertices, size_t n, hipStream_t stream);
// 5. attributes: one thread per vertex of a list whose positions are written -- the rest of the record.  The demo tree's: the
//    HermiteSource normal at the position, a zero material.  Dual contouring runs it over its Hermite records and again over its
//    solved vertices.
hipError_t launch_mesh_vertex_normals(const sdfv_demo_params& prm, uint32_t sdf_id, sdfv_vertex* vertices, size_t n,
                                      hipStream_t stream);
// 4 + 5 in one kernel, for the demo tree's marching cubes alone: the same records, written under the sparse mask of step 4
hipError_t launch_mesh_fused_vertices(const sdfv_demo_params& prm, uint32_t sdf_id, const MeshGrid& g, const MeshWork& w,
                                      sdfv_vertex* vertices, size_t n, hipStream_t stream);
// 6. triangle indices
hipError_t launch_mesh_triangles(const MeshGrid& g, const MeshWork& w, uint32_t* indices, hipStream_t stream);
#endif

}  // namespace sdfv
