// lattice_mesh_host.cpp -- the C++ host's mesh route for surfaces WITHOUT a device form: mesh_any_sdf and postproc_any.
//   lattice_mesh_host <out-prefix>
// * HostOnly, an application's own surface with sample_concurrency() 4, is meshed by mesh_any_sdf with both meshers at 12 cells
//   (one chunk) and at 104 cells (105^3 points: more than one upload); each result equals, byte for byte, the mesh of a lattice
//   this program samples itself in a plain single-thread loop and hands to sdfv_lattice_mesh_extract.  The 12-cell lattice and
//   meshes go to <out-prefix>.{dist,v0,i0,v4,i4}.bin for tests/test_gpu_lattice_mesh.py to hold against its restatement.
// * DeviceSampled, a surface that fills device records itself (here with the library's demo sampler standing for the
//   application's kernel), goes through the device route, one chunk and two: the same bytes as the lattice calls made by hand,
//   and the indices (marching cubes: the positions too) of sdfv_mesh_extract over the same demo.
// * A surface whose sample() throws on its worker threads yields an error with its text, and the process ends cleanly.
// * postproc_any equals a plain restatement of meshers/mesh.rs:22-33.
// * mesh_sdf and Mesh::postproc still refuse HostOnly; the meshers without a device implementation are still unsupported.
#include <hip/hip_runtime_api.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <stdexcept>
#include <vector>

#include "mesh.hpp"

using namespace sdfviewer;

namespace {

struct HostOnly : SDFSurface {  // two spheres in a box that is no cube; colour and material vary with the point
    BoundingBox bounding_box() const override { return {Vec3{-1.0f, -0.9f, -0.8f}, Vec3{1.0f, 0.9f, 0.8f}}; }
    SDFSample sample(Vec3 p, bool distance_only) const override {
        const float a = std::sqrt(p.x * p.x + p.y * p.y + p.z * p.z) - 0.55f;
        const float qx = p.x - 0.4f, qy = p.y - 0.3f, qz = p.z - 0.2f;
        const float b = std::sqrt(qx * qx + qy * qy + qz * qz) - 0.3f;
        SDFSample s = SDFSample::make(b < a ? b : a, Vec3{});
        if (distance_only) return s;
        s.color = Vec3{0.5f + 0.5f * p.x, 0.25f, b < a ? 1.0f : 0.0f};
        s.metallic = 0.5f * p.y;
        s.roughness = 0.125f;
        s.occlusion = p.z;
        return s;
    }
    unsigned sample_concurrency() const override { return 4; }
};

struct Throwing final : HostOnly {
    SDFSample sample(Vec3 p, bool distance_only) const override {
        if (p.z > 0.3f) throw std::runtime_error("no sample above z = 0.3");
        return HostOnly::sample(p, distance_only);
    }
};

struct DeviceSampled final : SDFSurface {  // sampled by "the application's kernel" only: no device form, no host samples
    sdfv_demo_params params;
    DeviceSampled() { sdfv_demo_params_default(&params); }
    BoundingBox bounding_box() const override { return {Vec3{-1, -1, -1}, Vec3{1, 1, 1}}; }
    SDFSample sample(Vec3, bool) const override { throw std::logic_error("DeviceSampled is never sampled on the host"); }
    bool has_device_sampler() const override { return true; }
    void sample_batch_device(const float* points_dev, size_t n, sdfv_sample* out_dev, void* stream) const override {
        if (sdfv_sample_points(&params, 0, points_dev, n, 0, out_dev, stream) != SDFV_OK) throw std::runtime_error(sdfv_last_error());
    }
};

bool fail(const char* what) {
    std::fprintf(stderr, "lattice_mesh_host: %s\n", what);
    return false;
}

void box_of(const SDFSurface& sdf, float lo[3], float hi[3]) {
    const BoundingBox bb = sdf.bounding_box();
    lo[0] = bb[0].x; lo[1] = bb[0].y; lo[2] = bb[0].z;
    hi[0] = bb[1].x; hi[1] = bb[1].y; hi[2] = bb[1].z;
}

// the lattice of the header, sampled point by point on this thread
std::vector<float> plain_lattice(const SDFSurface& sdf, uint32_t cells) {
    float lo[3], hi[3];
    box_of(sdf, lo, hi);
    const uint32_t np1 = cells + 1;
    std::vector<float> d((size_t)np1 * np1 * np1);
    size_t at = 0;
    for (uint32_t k = 0; k < np1; ++k)
        for (uint32_t j = 0; j < np1; ++j)
            for (uint32_t i = 0; i < np1; ++i) {
                const Vec3 p{(float)i / (float)cells * (hi[0] - lo[0]) + lo[0], (float)j / (float)cells * (hi[1] - lo[1]) + lo[1],
                             (float)k / (float)cells * (hi[2] - lo[2]) + lo[2]};
                d[at++] = sdf.sample(p, true).distance;
            }
    return d;
}

// sdfv_lattice_mesh_extract over a device lattice -> host Mesh
bool extract(const float* dist_dev, const SDFSurface& sdf, uint32_t cells, uint32_t algorithm, Mesh& out) {
    float lo[3], hi[3];
    box_of(sdf, lo, hi);
    sdfv_mesh m{};
    if (sdfv_lattice_mesh_extract(dist_dev, lo, hi, cells, algorithm, 0, &m, nullptr) != SDFV_OK) return fail(sdfv_last_error());
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

bool host_route(const std::string& prefix) {
    HostOnly sdf;
    for (uint32_t cells : {12u, 104u}) {
        const std::vector<float> d = plain_lattice(sdf, cells);
        float* dev = nullptr;
        if (hipMalloc(reinterpret_cast<void**>(&dev), d.size() * 4) != hipSuccess ||
            hipMemcpy(dev, d.data(), d.size() * 4, hipMemcpyHostToDevice) != hipSuccess)
            return fail("uploading the plain lattice");
        if (cells == 12) dump(prefix + ".dist.bin", d);
        for (int k = 0; k < 2; ++k) {
            Mesh want;
            if (!extract(dev, sdf, cells, kAlgorithms[k], want)) return false;
            MesherConfig cfg;
            cfg.max_voxels_per_axis = cells;
            std::string err;
            auto got = mesh_any_sdf(kMeshers[k], sdf, cfg, &err);
            if (!got) return fail(err.c_str());
            if (!same(*got, want)) return fail("mesh_any_sdf (host route) differs from the plain lattice's mesh");
            if (cells == 12) {
                dump(prefix + (k ? ".v4.bin" : ".v0.bin"), got->vertices);
                dump(prefix + (k ? ".i4.bin" : ".i0.bin"), got->indices);
            }
        }
        (void)hipFree(dev);
    }
    return true;
}

bool device_route() {
    DeviceSampled sdf;
    float lo[3], hi[3];
    box_of(sdf, lo, hi);
    for (uint32_t cells : {12u, 104u}) {
        const size_t n = (size_t)(cells + 1) * (cells + 1) * (cells + 1);
        float *points = nullptr, *dist = nullptr;
        sdfv_sample* samples = nullptr;
        if (hipMalloc(reinterpret_cast<void**>(&points), n * 12) != hipSuccess || hipMalloc(reinterpret_cast<void**>(&dist), n * 4) != hipSuccess ||
            hipMalloc(reinterpret_cast<void**>(&samples), n * sizeof(sdfv_sample)) != hipSuccess)
            return fail("device buffers");
        if (sdfv_lattice_points(lo, hi, cells, 0, n, points, nullptr) != SDFV_OK) return fail(sdfv_last_error());
        sdf.sample_batch_device(points, n, samples, nullptr);
        if (sdfv_lattice_from_samples(samples, n, dist, nullptr) != SDFV_OK) return fail(sdfv_last_error());
        for (int k = 0; k < 2; ++k) {
            Mesh want;
            if (!extract(dist, sdf, cells, kAlgorithms[k], want)) return false;
            MesherConfig cfg;
            cfg.max_voxels_per_axis = cells;
            std::string err;
            auto got = mesh_any_sdf(kMeshers[k], sdf, cfg, &err);
            if (!got) return fail(err.c_str());
            if (!same(*got, want)) return fail("mesh_any_sdf (device route) differs from the lattice calls made by hand");
            // the demo's own extraction: the same distances, so the same positions and indices
            sdfv_mesh m{};
            if (sdfv_mesh_extract(&sdf.params, 0, lo, hi, cells, kAlgorithms[k], &m, nullptr) != SDFV_OK) return fail(sdfv_last_error());
            std::vector<Vertex> v(m.n_vertices);
            std::vector<uint32_t> idx(m.n_indices);
            bool ok = m.n_vertices == got->vertices.size() && m.n_indices == got->indices.size() &&
                      hipMemcpy(v.data(), m.vertices, v.size() * sizeof(Vertex), hipMemcpyDeviceToHost) == hipSuccess &&
                      hipMemcpy(idx.data(), m.indices, idx.size() * 4, hipMemcpyDeviceToHost) == hipSuccess;
            sdfv_mesh_free(&m);
            if (!ok) return fail("the device route's counts differ from sdfv_mesh_extract's");
            if (std::memcmp(idx.data(), got->indices.data(), idx.size() * 4) != 0)
                return fail("the device route's indices differ from sdfv_mesh_extract's");
            // (dual contouring solves its positions from each route's own normals: only marching cubes' are comparable)
            for (size_t i = 0; k == 0 && i < v.size(); ++i)
                if (std::memcmp(&v[i].position, &got->vertices[i].position, 12) != 0)
                    return fail("the device route's positions differ from sdfv_mesh_extract's");
        }
        (void)hipFree(points);
        (void)hipFree(dist);
        (void)hipFree(samples);
    }
    return true;
}

bool throwing_surface() {
    Throwing sdf;
    MesherConfig cfg;
    cfg.max_voxels_per_axis = 12;
    std::string err;
    if (mesh_any_sdf(Meshers::MarchingCubes, sdf, cfg, &err)) return fail("a throwing surface was meshed");
    if (err.find("no sample above z = 0.3") == std::string::npos) return fail(("the error lacks the exception's text: " + err).c_str());
    return true;
}

bool postproc_restated() {
    HostOnly sdf;
    MesherConfig cfg;
    cfg.max_voxels_per_axis = 12;
    std::string err;
    auto mesh = mesh_any_sdf(Meshers::MarchingCubes, sdf, cfg, &err);
    if (!mesh || mesh->vertices.size() < 8) return fail("no mesh to post-process");
    for (size_t i = 0; i < mesh->vertices.size(); i += 3) mesh->vertices[i].normal = Vec3{0.0f, i % 2 ? 0.009f : 0.0f, 0.0f};  // unset
    mesh->vertices[1].normal = Vec3{0.0f, 0.0101f, 0.0f};  // |n|^2 = 1.02e-4: kept
    Mesh want = *mesh;
    for (Vertex& v : want.vertices) {  // meshers/mesh.rs:22-33
        const SDFSample s = sdf.sample(v.position, false);
        const float dx = v.normal.x - 0.0f, dy = v.normal.y - 0.0f, dz = v.normal.z - 0.0f;
        if (dx * dx + dy * dy + dz * dz < 0.0001f) v.normal = sdf.normal(v.position, std::nullopt);
        v.color = s.color;
        v.metallic = s.metallic;
        v.roughness = s.roughness;
        v.occlusion = s.occlusion;
    }
    if (postproc_any(*mesh, sdf) != SDFV_OK) return fail("postproc_any failed");
    if (!same(*mesh, want)) return fail("postproc_any differs from meshers/mesh.rs:22-33");
    const Vec3 kept{0.0f, 0.0101f, 0.0f};
    if (std::memcmp(&want.vertices[1].normal, &kept, 12) != 0) return fail("a set normal was recomputed");
    if (want.vertices[0].normal.x == 0.0f && want.vertices[0].normal.y == 0.0f && want.vertices[0].normal.z == 0.0f)
        return fail("an unset normal was kept");
    return true;
}

bool refusals() {
    HostOnly sdf;
    MesherConfig cfg;
    cfg.max_voxels_per_axis = 12;
    std::string err;
    Mesh none;
    if (mesh_sdf(Meshers::MarchingCubes, sdf, cfg, &err) || err.find("no device form") == std::string::npos) return fail("mesh_sdf took HostOnly");
    if (none.postproc(sdf) != SDFV_ERR_INVALID_ARGUMENT) return fail("Mesh::postproc took HostOnly");
    for (Meshers m : {Meshers::LinearHashedMarchingCubes, Meshers::DualContouringMinimizeQEF}) {
        err.clear();
        if (mesh_any_sdf(m, sdf, cfg, &err) || err != "Unsupported algorithm") return fail("an unsupported mesher was not refused");
    }
    for (size_t cells : {(size_t)0, (size_t)1025}) {
        cfg.max_voxels_per_axis = cells;
        err.clear();
        if (mesh_any_sdf(Meshers::MarchingCubes, sdf, cfg, &err) || err.find("outside [1, 1024]") == std::string::npos)
            return fail("a lattice size out of range was not refused");
    }
    return true;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    if (!refusals() || !host_route(argv[1]) || !device_route() || !throwing_surface() || !postproc_restated()) return 1;
    (void)sdfv_mesh_trim();
    std::printf("lattice_mesh_host ok\n");
    return 0;
}
