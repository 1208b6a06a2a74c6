// dual_contour_kernels.h -- launch interface of the dual-contouring steps that do not depend on the SDF (see
// dual_contour_kernels.hip; include/sdfgrid.h, "Dual contouring", states the arithmetic): counting, the per-cell solve and the
// quads.  The steps that evaluate an SDF stay where they are: the lattice distances and the Hermite records are the marching-cubes
// extractor's (mesh_kernels.h, program_mesh_kernels.h), the normals at the solved vertices are the SDF's vertex-list kernel.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/sdfgrid.h"
#include "mesh_kernels.h"

namespace sdfv {

// step 2 of a dual-contouring extraction: edge masks + the point scan (mesh_kernels.hip's), one 0/1 per ACTIVE cell into
// w.cell_first + scan, interior crossing edges per lattice point into w.quad_first + scan.  Leaves three totals:
// totals_dev[0] Hermite records (crossing edges), [1] vertices (active cells), [2] quads (interior crossing edges).
hipError_t launch_dc_count(const MeshGrid& g, const MeshWork& w, uint32_t* totals_dev, hipStream_t stream);
// step 4b: the compacted list of the n_vertices active cells into cell_list, then one thread per entry: the position of the
// cell's vertex from the Hermite records `hermite` (the marching-cubes vertex records of step 4a) into vertices[].position.
// Nothing else of the record is written: the SDF's vertex-list kernel follows.
hipError_t launch_dc_vertices(const MeshGrid& g, const MeshWork& w, const sdfv_vertex* hermite, uint32_t* cell_list,
                              sdfv_vertex* vertices, size_t n_vertices, hipStream_t stream);
// step 5: six indices per interior crossing edge, in the Hermite order
hipError_t launch_dc_quads(const MeshGrid& g, const MeshWork& w, uint32_t* indices, hipStream_t stream);

}  // namespace sdfv
