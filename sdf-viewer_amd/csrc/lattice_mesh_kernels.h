// lattice_mesh_kernels.h -- the third kind of SDF the extractor serves (include/sdfgrid.h, "Meshing a sampled lattice"): one the
// library cannot evaluate at all.  Its distances are a lattice the caller filled, and its normals come from that same lattice.
// Every SDF-free step of an extraction is mesh_kernels.h's and dual_contour_kernels.h's; this adds what feeds them and the
// attributes.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mesh_kernels.h"

namespace sdfv {

// out[3 * t ..] = lattice_position of flat lattice point first + t, t in [0, n).  The caller has checked first + n <= points.
hipError_t launch_lattice_points(const MeshGrid& g, uint32_t first, uint32_t n, float* out, hipStream_t stream);
// dist[i] = samples[i].distance
hipError_t launch_lattice_from_samples(const sdfv_sample* samples, size_t n, float* dist, hipStream_t stream);
// The attributes of n vertices whose positions are written: the normal of the header's definition, from `dist` over g's lattice.
// zero_materials: the six material fields are written too, as 0 (the vertices are then 8-byte aligned: the extractor's own);
// otherwise the three dwords of the normal are all that is stored.
hipError_t launch_lattice_normals(const float* dist, const MeshGrid& g, sdfv_vertex* vertices, size_t n, bool zero_materials,
                                  hipStream_t stream);

}  // namespace sdfv
