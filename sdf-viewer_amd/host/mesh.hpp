// mesh.hpp -- host mirror of the reference's mesh export (src/sdf/meshers/):
//   struct Mesh / Vertex            meshers/mesh.rs:8-17,133-155
//   Mesh::postproc                  meshers/mesh.rs:22-33     -> sdfv_mesh_postproc / sdfv_program_mesh_postproc (device)
//   Mesh::serialize_ply             meshers/mesh.rs:37-129    (ASCII PLY through the un-vendored ply-rs crate)
//   Config, Meshers, Mesher::mesh   meshers/mod.rs:92-149     -> sdfv_mesh_extract / sdfv_program_mesh_extract (device)
// mesh_sdf / Mesh::postproc serve the SDFs with a device form (SDFSurface::device_sdf, or SDFSurface::device_program: an SDF
// program); mesh_any_sdf / postproc_any serve every SDFSurface: one without a device form is SAMPLED -- on the host, or by its own
// kernel -- into a lattice that the device meshes (include/sdfgrid.h, "Meshing a sampled lattice").  The extraction itself has no
// CPU path.
#pragma once

#include <cstdint>
#include <optional>
#include <ostream>
#include <string>
#include <vector>

#include "sdf_surface.hpp"

namespace sdfviewer {

// meshers/mesh.rs:133-143 -- layout-compatible with sdfv_vertex (48 bytes)
struct Vertex {
    Vec3 position, normal, color;
    float metallic = 0.0f, roughness = 0.0f, occlusion = 0.0f;
};
static_assert(sizeof(Vertex) == sizeof(sdfv_vertex), "Vertex must stay layout-compatible with sdfv_vertex");

// meshers/mod.rs:92-107: `-v, --max-voxels-per-axis`, default 64
struct MesherConfig {
    size_t max_voxels_per_axis = 64;
};

// meshers/mod.rs:114-134; the clap subcommand names are the kebab-case variants
enum class Meshers { MarchingCubes, LinearHashedMarchingCubes, DualContouringMinimizeQEF, DualContouringParticleBasedMinimization };
std::optional<Meshers> mesher_from_name(const std::string& kebab);

struct Mesh {
    std::vector<Vertex> vertices;
    std::vector<uint32_t> indices;

    // Retrieves the materials for each vertex from the SDF; fills the normals the mesher left unset (mesh.rs:20-33).
    // Returns 0 or the sdfv status (sdfv_last_error() has the text).
    int postproc(const SDFSurface& sdf);
    // ASCII PLY with the reference's element/property list (mesh.rs:47-96); returns the bytes written.
    size_t serialize_ply(std::ostream& out, const std::string& version_info) const;
};

// Mesher::mesh (meshers/mod.rs:136-149).  MarchingCubes and DualContouringParticleBasedMinimization have a device
// implementation; the other two report "Unsupported algorithm" (isosurface.rs:49).  nullopt on error, text in *err.
std::optional<Mesh> mesh_sdf(Meshers mesher, const SDFSurface& sdf, const MesherConfig& cfg, std::string* err);

// Mesher::mesh for ANY SDFSurface.  One with a device form goes through mesh_sdf unchanged.  Any other is sampled at the
// (max_voxels_per_axis + 1)^3 lattice points -- has_device_sampler(): by sample_batch_device, chunk after chunk on one stream;
// otherwise on the host by sample_batch(..., distance_only = true) on sample_concurrency() threads, z-plane by z-plane, checked
// with check_samples() and uploaded while the next chunk is sampled -- and the lattice is meshed by sdfv_lattice_mesh_extract:
// positions and indices as the SDF's own distances give them, normals from the lattice, material fields zero until postproc_any.
// A sample() that throws ends the call with its text in *err.
std::optional<Mesh> mesh_any_sdf(Meshers mesher, const SDFSurface& sdf, const MesherConfig& cfg, std::string* err);
// Mesh::postproc for ANY SDFSurface: the device forms through Mesh::postproc, any other on the host (mesh.rs:22-33), sampled
// with one sample_batch(..., false); normal(p, nullopt) is asked only where the mesher left |n|^2 < 1e-4.  Whatever the SDF
// throws passes through.  Returns 0 or the sdfv status.
int postproc_any(Mesh& mesh, const SDFSurface& sdf);

// What every route to a host Mesh shares (SDFViewer::mesh, sdf_viewer.cpp, is the fourth): the device extractor's number of a
// mesher, nullopt for the two without a device implementation ("Unsupported algorithm", isosurface.rs:49), and the device mesh
// an extraction has just returned -> a host Mesh; the library's copy is freed either way.
std::optional<uint32_t> device_algorithm(Meshers mesher);
std::optional<Mesh> take_mesh(sdfv_mesh& m, std::string* err);

// f32 Display as Rust prints it (shortest digits that round-trip, never an exponent): what ply-rs writes for floats.
std::string format_f32(float v);
// (c * 255.9999) as u8, mesh.rs:106-108
uint8_t ply_color_u8(float c);

}  // namespace sdfviewer
