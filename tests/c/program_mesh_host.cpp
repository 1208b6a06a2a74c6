// program_mesh_host.cpp -- the C++ host's mesh route over an SDF program: ProgramSDF -> mesh_sdf -> Mesh::postproc ->
// serialize_ply, as `sdf-viewer-gpu mesh` does for the demo.  Reads a program (a file of sdfv_prog_op records), writes the
// vertices and indices as raw files for tests/test_gpu_program_mesh.py to compare with the Python route, and checks that a
// surface with neither device form is still refused.
//   program_mesh_host <ops.bin> <cells> <vertices.bin> <indices.bin> <mesh.ply>
#include <cstdio>
#include <fstream>
#include <sstream>
#include <vector>

#include "mesh.hpp"
#include "program_sdf.hpp"

using namespace sdfviewer;

namespace {
struct HostOnly final : SDFSurface {  // an application's own surface: no device form of either kind
    BoundingBox bounding_box() const override { return {Vec3{-1, -1, -1}, Vec3{1, 1, 1}}; }
    SDFSample sample(Vec3, bool) const override { return SDFSample{}; }
};
}  // namespace

int main(int argc, char** argv) {
    if (argc != 6) return 2;
    std::ifstream in(argv[1], std::ios::binary);
    std::vector<char> raw((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    if (raw.empty() || raw.size() % sizeof(sdfv_prog_op)) return 2;
    const float bb[6] = {-1.0f, -0.9f, -0.8f, 1.0f, 0.9f, 0.8f};
    sdfv_program* program = nullptr;
    if (sdfv_program_create(reinterpret_cast<const sdfv_prog_op*>(raw.data()), raw.size() / sizeof(sdfv_prog_op), bb, &program)) {
        std::fprintf(stderr, "create: %s\n", sdfv_last_error());
        return 1;
    }
    {
        ProgramSDF sdf(program);
        if (sdf.device_sdf() || sdf.device_program() != program) return 1;
        MesherConfig cfg;
        cfg.max_voxels_per_axis = (size_t)std::atoi(argv[2]);
        std::string err;
        auto mesh = mesh_sdf(Meshers::MarchingCubes, sdf, cfg, &err);
        if (!mesh) {
            std::fprintf(stderr, "mesh_sdf: %s\n", err.c_str());
            return 1;
        }
        if (mesh_sdf(Meshers::DualContouringMinimizeQEF, sdf, cfg, &err) || err != "Unsupported algorithm") return 1;
        if (int rc = mesh->postproc(sdf)) {
            std::fprintf(stderr, "postproc: %d %s\n", rc, sdfv_last_error());
            return 1;
        }
        std::ofstream(argv[3], std::ios::binary).write(reinterpret_cast<const char*>(mesh->vertices.data()),
                                                       (std::streamsize)(mesh->vertices.size() * sizeof(Vertex)));
        std::ofstream(argv[4], std::ios::binary).write(reinterpret_cast<const char*>(mesh->indices.data()),
                                                       (std::streamsize)(mesh->indices.size() * 4));
        std::ofstream ply(argv[5], std::ios::binary);
        const size_t bytes = mesh->serialize_ply(ply, "program_mesh_host");
        HostOnly other;
        Mesh none;
        if (mesh_sdf(Meshers::MarchingCubes, other, cfg, &err) || err.find("no device form") == std::string::npos) return 1;
        if (none.postproc(other) != SDFV_ERR_INVALID_ARGUMENT) return 1;
        std::printf("program_mesh_host ok vertices=%zu indices=%zu ply_bytes=%zu\n", mesh->vertices.size(), mesh->indices.size(),
                    bytes);
    }
    sdfv_program_free(program);
    return 0;
}
