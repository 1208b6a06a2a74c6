// grid_mesh_kernels.h -- the fourth kind of SDF the extractor serves (include/sdfgrid.h, "Meshing a loaded grid"): the one a
// viewer has loaded.  Its samples are on the device already: tex0.r (or the compact distance volume) holds the distance at
// exactly the points of a mesher's lattice, tex0.gba and tex1.rgb the material the shader shows.  Every SDF-free step of an
// extraction is mesh_kernels.h's and dual_contour_kernels.h's, the normals are lattice_mesh_kernels.h's over the unpacked
// lattice; this adds the unpack and the materials.
//
// The lattice.  Point (i, j, k) is voxel (i, j, k) * lod: n_a = (dims_a - 1) / lod + 1 points per axis, the points a load has
// published at that step.  It takes the stored distance s of its voxel and d = s - 0.1f, one rounded f32 operation; 0.1f is the
// float the fill adds (scene/sdf/mod.rs:196).  So
//  * inside (d < 0) is s < 0.1f, up to the rounding of 0.1f + d in the fill;
//  * a voxel still at AIR_DIST (0.1f + 0.001234f) is outside;
//  * the distances are the clamped ones, d in [-0.1, 0.9]: this is the surface as the viewer renders it;
//  * a vertex moves off the SDF's own crossing only on an edge one of whose ends was clamped, which needs an edge longer
//    than 0.1.
//
// The material of a vertex at p, from the grid (the shader's own values: its nearest filter while a grid loads):
//  1. the cell c and the place f of p per axis: steps 1-2 of the header's lattice normal(p) (lattice_vertex.h: lattice_cell)
//  2. the nearest lattice point q_a = c_a + (f_a > 0.5f ? 1 : 0); its voxel is q * lod
//  3. that voxel's tex0 and tex1 texels, 16 bytes each
//  4. per colour channel x = tex0.g / .b / .a: idx = the number of entries of the 256-entry sRGB -> linear table (srgb_lut.inc)
//     that are < x, at the most 255, 0 for a NaN; colour = (float)idx / 255.0f.  The table is strictly increasing, so for a
//     texel the fill wrote this is the 8-bit colour the fill quantised to, exactly.
//  5. metallic, roughness, occlusion = tex1.r, .g, .b as stored.
// What differs from Mesh::postproc on the SDF itself: colours are the 8-bit ones; a black sample arrives as the grid's 0.5
// grey; occlusion <= 0 arrives as 1; the material is the nearest voxel's, not the vertex point's.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mesh_kernels.h"

namespace sdfv {

// Where the grid's samples are.  vol: the compact distance volume (one float per voxel; ilv != 0: the y-interleaved layout) or
// nullptr, then tex0.r is read.  W, H: the grid's dims[0], dims[1].
struct GridTexels {
    const float4* tex0;
    const float4* tex1;  // the material gathers only
    const float* vol;
    uint32_t ilv;
    uint32_t W, H;
    uint32_t lod;
};

// lattice[point] = stored distance of the point's voxel - 0.1f over g's lattice (g.cells[a] * lod <= dims[a] - 1).  One thread
// per lattice point, x fastest.  Checks the grid (MeshGrid::launchable).
hipError_t launch_grid_lattice(const GridTexels& t, const MeshGrid& g, float* lattice, hipStream_t stream);
// The six material words of n vertices whose positions are written, rule above, and nothing else of a record (vertices: 4-byte
// aligned).
hipError_t launch_grid_vertex_materials(const GridTexels& t, const MeshGrid& g, sdfv_vertex* vertices, size_t n,
                                        hipStream_t stream);
// launch_lattice_normals over `lattice` and launch_grid_vertex_materials in one pass over the extractor's own vertices (8-byte
// aligned), the way lattice_normals_zero_mat writes the zero material.
hipError_t launch_grid_normals_materials(const float* lattice, const GridTexels& t, const MeshGrid& g, sdfv_vertex* vertices,
                                         size_t n, hipStream_t stream);

}  // namespace sdfv
