// mesh.cpp -- see mesh.hpp.  The PLY text follows what ply-rs 0.1.3 (un-vendored, Cargo.lock) emits for the header
// the reference builds in meshers/mesh.rs:41-96: parity of the byte stream is UNPINNED, the element and property
// lists, their order and types are the reference's.
#include "mesh.hpp"

#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <charconv>
#include <cmath>
#include <cstring>
#include <exception>

#include "worker_pool.hpp"

namespace sdfviewer {

std::optional<Meshers> mesher_from_name(const std::string& k) {
    if (k == "marching-cubes") return Meshers::MarchingCubes;
    if (k == "linear-hashed-marching-cubes") return Meshers::LinearHashedMarchingCubes;
    if (k == "dual-contouring-minimize-qef") return Meshers::DualContouringMinimizeQEF;
    if (k == "dual-contouring-particle-based-minimization") return Meshers::DualContouringParticleBasedMinimization;
    return std::nullopt;
}

// The device mesh an extraction has just returned -> a host Mesh; the library's copy is freed either way.
std::optional<Mesh> take_mesh(sdfv_mesh& m, std::string* err) {
    Mesh out;
    out.vertices.resize(m.n_vertices);
    out.indices.resize(m.n_indices);
    hipError_t e = hipSuccess;
    if (m.n_vertices) e = hipMemcpy(out.vertices.data(), m.vertices, m.n_vertices * sizeof(Vertex), hipMemcpyDeviceToHost);
    if (e == hipSuccess && m.n_indices) e = hipMemcpy(out.indices.data(), m.indices, m.n_indices * 4, hipMemcpyDeviceToHost);
    sdfv_mesh_free(&m);
    if (e != hipSuccess) {
        if (err) *err = std::string("copying the mesh to the host: ") + hipGetErrorString(e);
        return std::nullopt;
    }
    return out;
}

std::optional<uint32_t> device_algorithm(Meshers mesher) {
    if (mesher == Meshers::MarchingCubes) return SDFV_MESHER_MARCHING_CUBES;
    if (mesher == Meshers::DualContouringParticleBasedMinimization) return SDFV_MESHER_DUAL_CONTOURING_PARTICLE;
    return std::nullopt;  // isosurface.rs:49
}

namespace {

std::string describe(std::exception_ptr e) {
    try {
        std::rethrow_exception(e);
    } catch (const std::exception& ex) {
        return ex.what();
    } catch (...) {
        return "unknown exception";
    }
}

// What mesh_any_sdf holds on the device and in pinned memory while it fills a lattice; everything goes when it returns.
struct LatticeFill {
    hipStream_t stream = nullptr;
    float* dist = nullptr;               // (cells + 1)^3
    float* pinned[2] = {nullptr, nullptr};  // host route: one chunk of distances each
    hipEvent_t copied[2] = {nullptr, nullptr};
    float* points = nullptr;             // device route: one chunk of positions and of records
    sdfv_sample* samples = nullptr;
    ~LatticeFill() {
        if (stream) (void)hipStreamSynchronize(stream);
        for (int b = 0; b < 2; ++b) {
            if (pinned[b]) (void)hipHostFree(pinned[b]);
            if (copied[b]) (void)hipEventDestroy(copied[b]);
        }
        if (points) (void)hipFree(points);
        if (samples) (void)hipFree(samples);
        if (dist) (void)hipFree(dist);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

constexpr size_t kChunkPoints = (size_t)1 << 20;  // 4 MiB of distances per upload, 40 MiB of device records per batch

// The surface's own kernel fills the lattice: positions, the caller's samples, their distances, chunk after chunk on one stream.
bool fill_on_device(const SDFSurface& sdf, const float lo[3], const float hi[3], uint32_t cells, size_t n_points, LatticeFill& f,
                    std::string& why) {
    const size_t chunk = std::min(n_points, kChunkPoints);
    if (hipMalloc(reinterpret_cast<void**>(&f.points), chunk * 12) != hipSuccess ||
        hipMalloc(reinterpret_cast<void**>(&f.samples), chunk * sizeof(sdfv_sample)) != hipSuccess) {
        why = "cannot allocate the sampling buffers on the device";
        return false;
    }
    for (size_t first = 0; first < n_points; first += chunk) {
        const size_t n = std::min(chunk, n_points - first);
        if (sdfv_lattice_points(lo, hi, cells, first, n, f.points, f.stream) != SDFV_OK) {
            why = sdfv_last_error();
            return false;
        }
        try {
            sdf.sample_batch_device(f.points, n, f.samples, f.stream);
        } catch (...) {
            why = "the SDF's sample_batch_device() threw: " + describe(std::current_exception());
            return false;
        }
        if (sdfv_lattice_from_samples(f.samples, n, f.dist + first, f.stream) != SDFV_OK) {
            why = sdfv_last_error();
            return false;
        }
    }
    return true;
}

// The host samples the lattice: chunks of whole z-planes, the planes of a chunk dealt to the workers, distance only; a chunk's
// upload (pinned, asynchronous) runs while the next one is sampled into the other buffer.
bool fill_on_host(const SDFSurface& sdf, const float lo[3], const float hi[3], uint32_t cells, LatticeFill& f, std::string& why) {
    const size_t np1 = (size_t)cells + 1, plane = np1 * np1;
    const size_t chunk_planes = std::max<size_t>(1, std::min(np1, kChunkPoints / plane));
    for (int b = 0; b < 2; ++b) {
        if (hipHostMalloc(reinterpret_cast<void**>(&f.pinned[b]), chunk_planes * plane * 4, hipHostMallocDefault) != hipSuccess ||
            hipEventCreateWithFlags(&f.copied[b], hipEventDisableTiming) != hipSuccess) {
            why = "cannot allocate the pinned upload buffers";
            return false;
        }
    }
    std::vector<float> coord[3];  // the header's arithmetic: (float)i / (float)cells * size + min
    for (int a = 0; a < 3; ++a) {
        coord[a].resize(np1);
        const float size = hi[a] - lo[a];
        for (size_t i = 0; i < np1; ++i) coord[a][i] = (float)i / (float)cells * size + lo[a];
    }
    const unsigned threads = std::max(1u, std::min({sdf.sample_concurrency(), WorkerPool::usable_cpus(), 0xffffu}));
    std::vector<std::exception_ptr> thrown(threads);
    WorkerPool pool;
    pool.begin(threads);
    struct EndSession {
        WorkerPool& pool;
        ~EndSession() { pool.end(); }
    } end_session{pool};
    bool in_flight[2] = {false, false};
    int b = 0;
    for (size_t z0 = 0; z0 < np1; z0 += chunk_planes, b ^= 1) {
        const size_t planes = std::min(chunk_planes, np1 - z0);
        if (in_flight[b]) {  // the copy that read this buffer two chunks ago
            (void)hipEventSynchronize(f.copied[b]);
            in_flight[b] = false;
        }
        float* out = f.pinned[b];
        const unsigned workers = (unsigned)std::min<size_t>(threads, planes);
        auto sample_planes = [&](unsigned t) {
            // a worker thread has nobody to throw to: what sample() throws is kept for the calling thread
            try {
                std::vector<Vec3> p(np1);
                std::vector<SDFSample> s(np1);
                for (size_t z = t; z < planes; z += workers) {
                    for (size_t y = 0; y < np1; ++y) {
                        for (size_t x = 0; x < np1; ++x) p[x] = Vec3{coord[0][x], coord[1][y], coord[2][z0 + z]};
                        sdf.sample_batch(p.data(), np1, true, s.data());
                        float* row = out + (z * np1 + y) * np1;
                        for (size_t x = 0; x < np1; ++x) row[x] = s[x].distance;
                    }
                }
            } catch (...) {
                thrown[t] = std::current_exception();
            }
        };
        pool.run(workers, sample_planes);
        for (unsigned t = 0; t < workers; ++t) {
            if (thrown[t]) {
                why = "the SDF's sample() threw: " + describe(thrown[t]);
                return false;
            }
        }
        try {
            sdf.check_samples();
        } catch (...) {
            why = "the SDF's sample() failed: " + describe(std::current_exception());
            return false;
        }
        if (hipMemcpyAsync(f.dist + z0 * plane, out, planes * plane * 4, hipMemcpyHostToDevice, f.stream) != hipSuccess ||
            hipEventRecord(f.copied[b], f.stream) != hipSuccess) {
            why = "uploading the lattice failed";
            return false;
        }
        in_flight[b] = true;
    }
    return true;
}

}  // namespace

std::optional<Mesh> mesh_sdf(Meshers mesher, const SDFSurface& sdf, const MesherConfig& cfg, std::string* err) {
    auto fail = [&](const std::string& m) -> std::optional<Mesh> {
        if (err) *err = m;
        return std::nullopt;
    };
    const auto dev = sdf.device_sdf();
    const sdfv_program* program = dev ? nullptr : sdf.device_program();
    if (!dev && !program) return fail("this SDF has no device form: it cannot be meshed on the GPU");
    const auto algorithm = device_algorithm(mesher);
    if (!algorithm) return fail("Unsupported algorithm");
    const BoundingBox bb = sdf.bounding_box();
    const float lo[3] = {bb[0].x, bb[0].y, bb[0].z}, hi[3] = {bb[1].x, bb[1].y, bb[1].z};
    sdfv_mesh m{};
    const int rc = dev ? sdfv_mesh_extract(&dev->params, dev->sdf_id, lo, hi, (uint32_t)cfg.max_voxels_per_axis, *algorithm, &m,
                                           nullptr)
                       : sdfv_program_mesh_extract(program, lo, hi, (uint32_t)cfg.max_voxels_per_axis, *algorithm, 0, &m, nullptr);
    if (rc != SDFV_OK) return fail(sdfv_last_error());
    return take_mesh(m, err);
}

std::optional<Mesh> mesh_any_sdf(Meshers mesher, const SDFSurface& sdf, const MesherConfig& cfg, std::string* err) {
    if (sdf.device_sdf() || sdf.device_program()) return mesh_sdf(mesher, sdf, cfg, err);
    auto fail = [&](const std::string& m) -> std::optional<Mesh> {
        if (err) *err = m;
        return std::nullopt;
    };
    const auto algorithm = device_algorithm(mesher);
    if (!algorithm) return fail("Unsupported algorithm");
    if (cfg.max_voxels_per_axis < 1 || cfg.max_voxels_per_axis > 1024)  // before a single sample is taken
        return fail("max_voxels_per_axis " + std::to_string(cfg.max_voxels_per_axis) + " is outside [1, 1024]");
    const uint32_t cells = (uint32_t)cfg.max_voxels_per_axis;
    const size_t n_points = ((size_t)cells + 1) * (cells + 1) * (cells + 1);
    const BoundingBox bb = sdf.bounding_box();
    const float lo[3] = {bb[0].x, bb[0].y, bb[0].z}, hi[3] = {bb[1].x, bb[1].y, bb[1].z};
    LatticeFill f;
    if (hipStreamCreateWithFlags(&f.stream, hipStreamNonBlocking) != hipSuccess ||
        hipMalloc(reinterpret_cast<void**>(&f.dist), n_points * 4) != hipSuccess)
        return fail("cannot allocate the lattice on the device");
    std::string why;
    const bool filled = sdf.has_device_sampler() ? fill_on_device(sdf, lo, hi, cells, n_points, f, why)
                                                 : fill_on_host(sdf, lo, hi, cells, f, why);
    if (!filled) return fail(why);
    sdfv_mesh m{};
    if (sdfv_lattice_mesh_extract(f.dist, lo, hi, cells, *algorithm, 0, &m, f.stream) != SDFV_OK) return fail(sdfv_last_error());
    return take_mesh(m, err);
}

int postproc_any(Mesh& mesh, const SDFSurface& sdf) {
    if (sdf.device_sdf() || sdf.device_program()) return mesh.postproc(sdf);
    const size_t n = mesh.vertices.size();
    std::vector<Vec3> p(n);
    std::vector<SDFSample> s(n);
    for (size_t i = 0; i < n; ++i) p[i] = mesh.vertices[i].position;
    sdf.sample_batch(p.data(), n, false, s.data());
    for (size_t i = 0; i < n; ++i) {
        Vertex& v = mesh.vertices[i];
        const float dx = v.normal.x - 0.0f, dy = v.normal.y - 0.0f, dz = v.normal.z - 0.0f;  // distance2(zero), mesh.rs:25
        if (dx * dx + dy * dy + dz * dz < 0.0001f) v.normal = sdf.normal(v.position, std::nullopt);
        v.color = s[i].color;
        v.metallic = s[i].metallic;
        v.roughness = s[i].roughness;
        v.occlusion = s[i].occlusion;
    }
    return SDFV_OK;
}

int Mesh::postproc(const SDFSurface& sdf) {
    sdfv_vertex* v = reinterpret_cast<sdfv_vertex*>(vertices.data());
    if (const auto dev = sdf.device_sdf()) return sdfv_mesh_postproc_host(&dev->params, dev->sdf_id, v, vertices.size());
    if (const sdfv_program* program = sdf.device_program()) return sdfv_program_mesh_postproc_host(program, v, vertices.size());
    return SDFV_ERR_INVALID_ARGUMENT;
}

std::string format_f32(float v) {
    if (std::isnan(v)) return "NaN";
    if (std::isinf(v)) return v < 0 ? "-inf" : "inf";
    // shortest round-trip digits (scientific form), then laid out positionally with zero padding like Rust's Display
    char buf[64];
    auto r = std::to_chars(buf, buf + sizeof(buf), std::fabs(v), std::chars_format::scientific);
    std::string sci(buf, r.ptr);  // d[.ddd]e[+-]xx
    const size_t e = sci.find('e');
    std::string digits;
    for (char c : sci.substr(0, e))
        if (c != '.') digits += c;
    const int exp10 = std::stoi(sci.substr(e + 1));
    std::string out = std::signbit(v) ? "-" : "";
    const int n = (int)digits.size();
    if (exp10 >= n - 1) {
        out += digits + std::string((size_t)(exp10 - (n - 1)), '0');
    } else if (exp10 >= 0) {
        out += digits.substr(0, (size_t)exp10 + 1) + "." + digits.substr((size_t)exp10 + 1);
    } else {
        out += "0." + std::string((size_t)(-exp10 - 1), '0') + digits;
    }
    return out;
}

uint8_t ply_color_u8(float c) {
    const float v = c * 255.9999f;
    if (!(v > 0.0f)) return 0;  // negatives and NaN: Rust's saturating `as u8`
    if (v >= 255.0f) return 255;
    return (uint8_t)v;
}

size_t Mesh::serialize_ply(std::ostream& out, const std::string& version_info) const {
    std::string s;
    s.reserve(96 * vertices.size() + 16 * indices.size() + 512);
    s += "ply\nformat ascii 1.0\n";
    s += "comment Created with " + version_info + "\n";  // mesh.rs:45
    s += "element vertex " + std::to_string(vertices.size()) + "\n";
    for (const char* p : {"x", "y", "z", "nx", "ny", "nz"}) s += std::string("property float ") + p + "\n";
    for (const char* p : {"red", "green", "blue"}) s += std::string("property uchar ") + p + "\n";
    for (const char* p : {"metallic", "roughness", "occlusion"}) s += std::string("property float ") + p + "\n";
    s += "element face " + std::to_string(indices.size() / 3) + "\n";
    s += "property list uchar int vertex_index\nend_header\n";
    for (const Vertex& v : vertices) {
        const float f6[6] = {v.position.x, v.position.y, v.position.z, v.normal.x, v.normal.y, v.normal.z};
        for (float f : f6) s += format_f32(f) + " ";
        s += std::to_string(ply_color_u8(v.color.x)) + " " + std::to_string(ply_color_u8(v.color.y)) + " " +
             std::to_string(ply_color_u8(v.color.z)) + " ";
        s += format_f32(v.metallic) + " " + format_f32(v.roughness) + " " + format_f32(v.occlusion) + "\n";
    }
    for (size_t t = 0; t + 2 < indices.size(); t += 3) {  // chunks_exact(3), mesh.rs:116
        s += "3 " + std::to_string((int32_t)indices[t]) + " " + std::to_string((int32_t)indices[t + 1]) + " " +
             std::to_string((int32_t)indices[t + 2]) + "\n";
    }
    out.write(s.data(), (std::streamsize)s.size());
    return s.size();
}

}  // namespace sdfviewer
