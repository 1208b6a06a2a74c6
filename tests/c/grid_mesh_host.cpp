// grid_mesh_host.cpp -- the C++ host's route to the mesh of the grid a viewer has loaded: SDFViewer::mesh.
//   grid_mesh_host <provider library> <out-prefix>
// The SDF is a provider library behind the per-point ABI (tests/c/gyroid_provider.c): host-only, the case the route exists for.
// Every case runs twice: on 17^3 with the plain distance volume and on 17 x 18 x 17 with the y-interleaved one (an even height;
// the layout is pinned, Auto picks the plain volume for grids this small), and holds that the viewer keeps that volume -- so
// that what SDFViewer::mesh reads, the volume and layout LoadState names, is the interleaved one in the second round.
// * After a full load, SDFViewer::mesh with both meshers, with and without materials, equals, byte for byte, the call
//   sdfv_grid_mesh_extract made by hand on the viewer's texture pointers and grid (what sdfv_viewer_textures hands out), lod 1,
//   from tex0 alone.
// * After a load stopped while the last pass runs (lod_dist_between_samples == 2) it equals the call with lod = 2; the rows no
//   pass has reached were virgin and are materialised by the call.
// * The demo, loaded by whole passes into a virgin grid and stopped at lod 2 likewise: the virgin rows are materialised first;
//   and the demo loaded to the end.
// * A viewer nothing was loaded into gives an empty mesh and success; the meshers without a device implementation are refused.
// The marching-cubes mesh with materials of the full load goes to <out-prefix>.{v,i}.bin for the test's CLI comparison.
#include <hip/hip_runtime_api.h>

#include <array>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <vector>

#include "provider_sdf.hpp"
#include "sdf_demo.hpp"
#include "sdf_viewer.hpp"

using namespace sdfviewer;

namespace {

bool fail(const char* what) {
    std::fprintf(stderr, "grid_mesh_host: %s\n", what);
    return false;
}

// sdfv_grid_mesh_extract by hand, from tex0 alone -> host Mesh
bool by_hand(SDFViewer& v, uint32_t lod, uint32_t algorithm, uint32_t flags, Mesh& out) {
    const sdfv_grid g = v.grid();
    sdfv_mesh m{};
    if (sdfv_grid_mesh_extract(&g, v.tex0_device(), v.tex1_device(), nullptr, 0, lod, algorithm, flags, &m, v.stream) != SDFV_OK)
        return fail(sdfv_last_error());
    out.vertices.resize(m.n_vertices);
    out.indices.resize(m.n_indices);
    bool ok = true;
    if (m.n_vertices) ok = hipMemcpy(out.vertices.data(), m.vertices, m.n_vertices * sizeof(Vertex), hipMemcpyDeviceToHost) == hipSuccess;
    if (ok && m.n_indices) ok = hipMemcpy(out.indices.data(), m.indices, m.n_indices * 4, hipMemcpyDeviceToHost) == hipSuccess;
    sdfv_mesh_free(&m);
    return ok || fail("copying a mesh back");
}

bool same(const Mesh& a, const Mesh& b) {
    return a.vertices.size() == b.vertices.size() && a.indices.size() == b.indices.size() && !a.vertices.empty() && !a.indices.empty() &&
           std::memcmp(a.vertices.data(), b.vertices.data(), a.vertices.size() * sizeof(Vertex)) == 0 &&
           std::memcmp(a.indices.data(), b.indices.data(), a.indices.size() * 4) == 0;
}

template <typename T>
void dump(const std::string& path, const std::vector<T>& v) {
    std::ofstream(path, std::ios::binary).write(reinterpret_cast<const char*>(v.data()), (std::streamsize)(v.size() * sizeof(T)));
}

constexpr Meshers kMeshers[2] = {Meshers::MarchingCubes, Meshers::DualContouringParticleBasedMinimization};
constexpr uint32_t kAlgorithms[2] = {SDFV_MESHER_MARCHING_CUBES, SDFV_MESHER_DUAL_CONTOURING_PARTICLE};

// SDFViewer::mesh against the call by hand at `lod`, both meshers, with and without materials
bool compare(SDFViewer& v, uint32_t lod, const char* what, const std::string* dump_prefix) {
    for (int k = 0; k < 2; ++k)
        for (int materials = 0; materials < 2; ++materials) {
            Mesh got, want;
            std::string err;
            if (!v.mesh(kMeshers[k], materials != 0, &got, &err)) return fail(err.c_str());
            if (v.material.undefined_rows) return fail("SDFViewer::mesh left virgin rows");
            if (!by_hand(v, lod, kAlgorithms[k], materials ? SDFV_MESH_WITH_MATERIALS : 0u, want)) return false;
            if (!same(got, want)) {
                std::fprintf(stderr, "grid_mesh_host: %s: SDFViewer::mesh (mesher %d, materials %d: %zu vertices, %zu indices) differs from the call "
                             "by hand (%zu, %zu)\n", what, k, materials, got.vertices.size(), got.indices.size(), want.vertices.size(),
                             want.indices.size());
                return false;
            }
            bool coloured = false;
            for (const Vertex& x : got.vertices) coloured = coloured || x.color.x != 0.0f || x.color.y != 0.0f || x.color.z != 0.0f;
            if (coloured != (materials != 0)) return fail("the material fields do not follow with_materials");
            if (dump_prefix && k == 0 && materials) {
                dump(*dump_prefix + ".v.bin", got.vertices);
                dump(*dump_prefix + ".i.bin", got.indices);
            }
        }
    return true;
}

// The two volumes a viewer can keep: texture order on 17^3, and y-interleaved, which pairs rows and so needs the even height
// of 17 x 18 x 17.  (Auto would pick the plain one for grids this small: sdfv_march_volume_advice.)
struct Shape {
    std::array<size_t, 3> dims;
    SDFViewer::VolumeLayout layout;
    const char* name;
};
const Shape kShapes[2] = {{{17, 17, 17}, SDFViewer::VolumeLayout::Plain, "plain 17x17x17"},
                          {{17, 18, 17}, SDFViewer::VolumeLayout::Interleaved, "interleaved 17x18x17"}};

// The viewer reads the volume it keeps, in the layout it keeps it in: LoadState::mesh_source's answer is what is under test.
bool keeps(const SDFViewer& v, const Shape& s) {
    const bool interleaved = s.layout == SDFViewer::VolumeLayout::Interleaved;
    if (!v.material.dist || v.material.dist_interleaved != interleaved) {
        std::fprintf(stderr, "grid_mesh_host: %s: the viewer does not keep the volume this case is about\n", s.name);
        return false;
    }
    return true;
}

bool run(const std::string& library, const std::string& prefix) {
    std::string err;
    auto sdf = ProviderSDF::load(library, &err);
    if (!sdf) return fail(err.c_str());
    auto demo = SDFDemo::from_args({}, &err);
    if (!demo) return fail(err.c_str());
    const BoundingBox bb = sdf->bounding_box();
    const auto budget = std::chrono::milliseconds(30);
    for (const Shape& shape : kShapes) {
        const bool first = &shape == &kShapes[0];
        // a full load of the provider
        {
            auto v = SDFViewer::new_voxels(shape.dims, bb, 3, shape.layout);
            if (!v) return fail("cannot create the viewer");
            if (!keeps(*v, shape)) return false;
            Mesh empty;
            if (!v->mesh(Meshers::MarchingCubes, true, &empty, &err)) return fail(err.c_str());  // nothing loaded: AIR everywhere
            if (!empty.vertices.empty() || !empty.indices.empty()) return fail("a viewer nothing was loaded into gave a mesh");
            while (v->update(*sdf, budget) != 0) v->commit();
            if (*v->last_error()) return fail(v->last_error());
            v->commit();
            if (v->material.lod_dist_between_samples != 1.0f) return fail("the load did not finish");
            if (!compare(*v, 1, shape.name, first ? &prefix : nullptr)) return false;
            Mesh m;
            if (v->mesh(Meshers::LinearHashedMarchingCubes, true, &m, &err) || err != "Unsupported algorithm") return fail("linear-hashed was not refused");
            if (v->mesh(Meshers::DualContouringMinimizeQEF, true, &m, &err) || err != "Unsupported algorithm") return fail("QEF was not refused");
        }
        // a load of the provider stopped while its last pass runs: the voxels at step 2 are published
        {
            auto v = SDFViewer::new_voxels(shape.dims, bb, 3, shape.layout);
            if (!v) return fail("cannot create the viewer");
            v->host_threads = 1;
            v->ingest_capacity = 64;  // short runs: the load stops soon after the step-2 pass ends
            while (v->loading_mgr.step_size() > 1) {
                if (v->update(*sdf, std::chrono::nanoseconds(1)) == 0) return fail("the load ended before its last pass");
                if (*v->last_error()) return fail(v->last_error());
            }
            if (v->material.lod_dist_between_samples != 2.0f || v->loading_mgr.len() == 0) return fail("the load is not at lod 2");
            if (!keeps(*v, shape) || !compare(*v, 2, shape.name, nullptr)) return false;
        }
        // the same with the demo, which loads by whole passes into a virgin grid: after the step-2 pass the rows with an odd y or
        // z hold undefined bytes, and SDFViewer::mesh writes their initial state before anything reads the grid
        {
            auto v = SDFViewer::new_voxels(shape.dims, demo->bounding_box(), 3, shape.layout);
            if (!v) return fail("cannot create the viewer");
            while (v->loading_mgr.step_size() > 1) {
                if (v->update(*demo, std::chrono::nanoseconds(1)) == 0) return fail("the demo's load ended before its last pass");
                if (*v->last_error()) return fail(v->last_error());
            }
            if (v->material.lod_dist_between_samples != 2.0f) return fail("the demo's load is not at lod 2");
            if (!v->material.undefined_rows) return fail("the demo's passes left no virgin rows: this case shows nothing");
            if (!keeps(*v, shape) || !compare(*v, 2, shape.name, nullptr)) return false;
        }
        // ... and the demo loaded to the end (one dense fill, which writes the interleaved volume itself)
        {
            auto v = SDFViewer::new_voxels(shape.dims, demo->bounding_box(), 3, shape.layout);
            if (!v) return fail("cannot create the viewer");
            while (v->update(*demo, budget) != 0) v->commit();
            if (*v->last_error()) return fail(v->last_error());
            if (v->material.lod_dist_between_samples != 1.0f) return fail("the demo's load did not finish");
            if (!keeps(*v, shape) || !compare(*v, 1, shape.name, nullptr)) return false;
        }
    }
    return true;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    if (sdfv_device_count() == 0) return fail("no device"), 1;
    if (!run(argv[1], argv[2])) return 1;
    sdfv_mesh_trim();
    std::printf("grid_mesh_host ok\n");
    return 0;
}
