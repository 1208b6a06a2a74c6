// ingest_throw.cpp -- TEST: an application's own SDFSurface (host-only: no device_sdf()) whose sample() throws, loaded through
// SDFViewer::update's ingest path (libsdfviewer_host.so, linked the way sdf-viewer-host-bench links it).
// Viewer A loads the plain surface; viewer B loads the same surface armed to throw std::runtime_error once, at the K-th sample()
// made on the calling thread (after the first gather of a run), catches the exception from update() and keeps calling update()
// until the load is done.  The same again for a parameter edit that reports a changed box.  A and B must end with byte-identical
// tex0, tex1 and distance volume.  Usage: ingest_throw <host_threads>; prints "ingest_throw ok threads=<t> exceptions=<n>".
#include <hip/hip_runtime_api.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "sdf_viewer.hpp"

using namespace sdfviewer;

namespace {

constexpr long kThrowAt = 50000;

// A wobbly sphere with a procedural colour.  Only the thread that constructed it counts its sample() calls and may throw.
class Blob : public SDFSurface {
   public:
    BoundingBox bounding_box() const override { return {Vec3{-1.0f, -0.75f, -1.0f}, Vec3{1.0f, 0.75f, 1.0f}}; }
    SDFSample sample(Vec3 p, bool /*distance_only*/) const override {
        if (std::this_thread::get_id() == caller_ && armed_ && ++caller_calls_ == kThrowAt) {
            armed_ = false;
            throw std::runtime_error("sample() refused this point");
        }
        const float r = std::sqrt(p.x * p.x + p.y * p.y + p.z * p.z);
        const float d = r - radius_ + 0.05f * std::sin(9.0f * p.x) * std::cos(7.0f * p.z);
        SDFSample s = SDFSample::make(d, Vec3{0.5f + 0.5f * std::sin(5.0f * p.y), std::fabs(p.z), p.x > 0.0f ? 0.9f : 0.0f});
        s.metallic = 0.25f;
        s.roughness = p.y > 0.0f ? 0.7f : 0.1f;
        return s;
    }
    unsigned sample_concurrency() const override { return 64; }
    std::optional<BoundingBox> changed() override {
        auto b = pending_;
        pending_.reset();
        return b;
    }
    // an edit: a new radius, reported as a box that covers part of the grid
    void edit(float radius) {
        radius_ = radius;
        pending_ = BoundingBox{Vec3{-1.0f, -0.75f, -1.0f}, Vec3{0.2f, 0.75f, 1.0f}};
    }
    void arm() {
        armed_ = true;
        caller_calls_ = 0;
    }

   private:
    std::thread::id caller_ = std::this_thread::get_id();
    mutable bool armed_ = false;
    mutable long caller_calls_ = 0;
    float radius_ = 0.6f;
    std::optional<BoundingBox> pending_;
};

// update() until the load (and any changed box) is worked off; counts the exceptions update() let through, and those after
// which last_error() did not describe them
bool work_off(SDFViewer& v, Blob& sdf, int& exceptions, int& unreported) {
    for (int calls = 0; calls < 100000; ++calls) {
        size_t n = 0;
        try {
            n = v.update(sdf, std::chrono::milliseconds(500));
        } catch (const std::runtime_error& e) {
            ++exceptions;
            if (std::strstr(v.last_error(), e.what()) == nullptr) {
                fprintf(stderr, "last_error() after the throw: '%s'\n", v.last_error());
                ++unreported;
            }
            continue;
        }
        if (*v.last_error()) {
            fprintf(stderr, "update failed: %s\n", v.last_error());
            return false;
        }
        if (n == 0 && v.loading_mgr.len() == 0 && !v.changed_box) return true;
    }
    fprintf(stderr, "the load never finished\n");
    return false;
}

bool download(const SDFViewer& v, std::vector<float>& t0, std::vector<float>& t1, std::vector<float>& dist) {
    const size_t voxels = (size_t)v.material.tex_size[0] * v.material.tex_size[1] * v.material.tex_size[2];
    t0.resize(voxels * 4);
    t1.resize(voxels * 4);
    if (v.download(t0.data(), t1.data()) != 0) return false;
    dist.clear();
    if (v.material.dist) {
        dist.resize(v.material.dist->bytes() / sizeof(float));
        if (hipStreamSynchronize((hipStream_t)v.stream) != hipSuccess ||
            hipMemcpy(dist.data(), v.material.dist->get(), v.material.dist->bytes(), hipMemcpyDeviceToHost) != hipSuccess)
            return false;
    }
    return true;
}

bool same_bytes(const std::vector<float>& a, const std::vector<float>& b) {
    return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(float)) == 0;
}

bool compare(const SDFViewer& a, const SDFViewer& b, const char* phase) {
    std::vector<float> a0, a1, ad, b0, b1, bd;
    if (!download(a, a0, a1, ad) || !download(b, b0, b1, bd)) {
        fprintf(stderr, "%s: download failed\n", phase);
        return false;
    }
    const bool ok0 = same_bytes(a0, b0), ok1 = same_bytes(a1, b1), okd = same_bytes(ad, bd);
    if (!(ok0 && ok1 && okd)) {
        size_t differing = 0;
        for (size_t i = 0; i < a0.size() && i < b0.size(); ++i) differing += std::memcmp(&a0[i], &b0[i], sizeof(float)) != 0;
        fprintf(stderr, "%s: tex0 %s (%zu floats differ), tex1 %s, distance volume %s\n", phase, ok0 ? "same" : "DIFFERS", differing,
                ok1 ? "same" : "DIFFERS", okd ? "same" : "DIFFERS");
        return false;
    }
    return true;
}

}  // namespace

int main(int argc, char** argv) {
    const unsigned threads = argc > 1 ? (unsigned)atoi(argv[1]) : 1;
    const std::array<size_t, 3> dims{96, 72, 96};
    Blob plain, throwing;
    auto a = SDFViewer::new_voxels(dims, plain.bounding_box(), 3);
    auto b = SDFViewer::new_voxels(dims, throwing.bounding_box(), 3);
    if (!a || !b) {
        fprintf(stderr, "cannot create the viewers\n");
        return 1;
    }
    a->host_threads = b->host_threads = threads;
    int unexpected = 0, exceptions = 0, unreported = 0;
    throwing.arm();
    if (!work_off(*a, plain, unexpected, unreported) || !work_off(*b, throwing, exceptions, unreported)) return 1;
    if (unexpected != 0 || exceptions != 1) {
        fprintf(stderr, "load: %d exception(s) from the throwing viewer (want 1), %d from the plain one\n", exceptions, unexpected);
        return 1;
    }
    if (!compare(*a, *b, "load")) return 1;
    plain.edit(0.45f);
    throwing.edit(0.45f);
    throwing.arm();
    if (!work_off(*a, plain, unexpected, unreported) || !work_off(*b, throwing, exceptions, unreported)) return 1;
    if (unexpected != 0 || exceptions != 2) {
        fprintf(stderr, "edit: %d exception(s) in all from the throwing viewer (want 2), %d from the plain one\n", exceptions, unexpected);
        return 1;
    }
    if (!compare(*a, *b, "edit")) return 1;
    if (unreported != 0) return 1;
    printf("ingest_throw ok threads=%u exceptions=%d\n", threads, exceptions);
    return 0;
}
