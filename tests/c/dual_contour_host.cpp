// dual_contour_host.cpp -- the C++ host's mesh route with Meshers::DualContouringParticleBasedMinimization.
//   dual_contour_host host-only
//       no device needed: a surface with neither device form is refused with "no device form" whatever the mesher, and the two
//       meshers without a device implementation are still "Unsupported algorithm" for a surface that has one.
//   dual_contour_host <ops.bin> <cells> <vertices.bin> <indices.bin> <mesh.ply>
//       ProgramSDF -> mesh_sdf (dual contouring) -> Mesh::postproc -> serialize_ply; the arrays go to raw files for
//       tests/test_gpu_dual_contour.py to compare with the Python route.  The program's box is -1..1.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <vector>

#include "mesh.hpp"
#include "program_sdf.hpp"

using namespace sdfviewer;

namespace {
struct HostOnly final : SDFSurface {  // an application's own surface: no device form of either kind
    BoundingBox bounding_box() const override { return {Vec3{-1, -1, -1}, Vec3{1, 1, 1}}; }
    SDFSample sample(Vec3, bool) const override { return SDFSample{}; }
};
constexpr Meshers kDual = Meshers::DualContouringParticleBasedMinimization;
const float kBox[6] = {-1.0f, -1.0f, -1.0f, 1.0f, 1.0f, 1.0f};

int host_only() {
    if (mesher_from_name("dual-contouring-particle-based-minimization") != kDual) return 1;
    MesherConfig cfg;
    cfg.max_voxels_per_axis = 8;
    std::string err;
    HostOnly other;
    if (mesh_sdf(kDual, other, cfg, &err) || err.find("no device form") == std::string::npos) return 1;
    sdfv_prog_op op;
    std::memset(&op, 0, sizeof(op));
    op.op = SDFV_OP_SPHERE;
    op.a[0] = 0.6f;
    sdfv_program* program = nullptr;
    if (sdfv_program_create(&op, 1, kBox, &program)) return 1;
    int rc = 0;
    {
        ProgramSDF sdf(program);
        for (Meshers m : {Meshers::LinearHashedMarchingCubes, Meshers::DualContouringMinimizeQEF}) {
            err.clear();
            if (mesh_sdf(m, sdf, cfg, &err) || err != "Unsupported algorithm") rc = 1;
        }
    }
    sdfv_program_free(program);
    if (rc == 0) std::printf("dual_contour_host host-only ok\n");
    return rc;
}
}  // namespace

int main(int argc, char** argv) {
    if (argc == 2 && std::strcmp(argv[1], "host-only") == 0) return host_only();
    if (argc != 6) return 2;
    std::ifstream in(argv[1], std::ios::binary);
    std::vector<char> raw((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    if (raw.empty() || raw.size() % sizeof(sdfv_prog_op)) return 2;
    sdfv_program* program = nullptr;
    if (sdfv_program_create(reinterpret_cast<const sdfv_prog_op*>(raw.data()), raw.size() / sizeof(sdfv_prog_op), kBox, &program)) {
        std::fprintf(stderr, "create: %s\n", sdfv_last_error());
        return 1;
    }
    {
        ProgramSDF sdf(program);
        MesherConfig cfg;
        cfg.max_voxels_per_axis = (size_t)std::atoi(argv[2]);
        std::string err;
        auto mesh = mesh_sdf(kDual, sdf, cfg, &err);
        if (!mesh) {
            std::fprintf(stderr, "mesh_sdf: %s\n", err.c_str());
            return 1;
        }
        if (int rc = mesh->postproc(sdf)) {
            std::fprintf(stderr, "postproc: %d %s\n", rc, sdfv_last_error());
            return 1;
        }
        std::ofstream(argv[3], std::ios::binary).write(reinterpret_cast<const char*>(mesh->vertices.data()),
                                                       (std::streamsize)(mesh->vertices.size() * sizeof(Vertex)));
        std::ofstream(argv[4], std::ios::binary).write(reinterpret_cast<const char*>(mesh->indices.data()),
                                                       (std::streamsize)(mesh->indices.size() * 4));
        std::ofstream ply(argv[5], std::ios::binary);
        const size_t bytes = mesh->serialize_ply(ply, "dual_contour_host");
        std::printf("dual_contour_host ok vertices=%zu indices=%zu ply_bytes=%zu\n", mesh->vertices.size(), mesh->indices.size(),
                    bytes);
    }
    sdfv_program_free(program);
    return 0;
}
