// program_sdf.cpp -- ProgramSDF and sdfv_program_as_surface (include/sdfprogram.h): SDF programs on the host.
// Built with -ffp-contract=off like the kernels: csrc/program_eval.h then rounds every step as the device does.
#include "program_sdf.hpp"

#include <atomic>
#include <cstring>
#include <stdexcept>

#include "../../include/sdfprogram.h"
#include "../csrc/program_cast.h"
#include "../csrc/program_eval.h"
#include "../csrc/program_march.h"
#include "worker_pool.hpp"

namespace sdfviewer {
namespace {

// The result of the stack machine as a record: the material index resolved against the program's own instructions.
void evaluate(const sdfv_prog_op* ops, size_t n_ops, const float* p, bool distance_only, sdfv_sample* out) {
    const sdfv::prog::Value v = sdfv::prog::run(ops, (uint32_t)n_ops, p[0], p[1], p[2]);
    out->distance = v.d;
    const bool has = !distance_only && v.m != sdfv::prog::kNoMaterial;
    const float* a = has ? ops[v.m].a : nullptr;
    for (int k = 0; k < 3; ++k) out->color[k] = has ? a[k] : 0.0f;
    out->metallic = has ? a[3] : 0.0f;
    out->roughness = has ? a[4] : 0.0f;
    out->occlusion = has ? a[5] : 0.0f;
}

// ---- the callbacks of sdfv_program_as_surface ----
// `user` is the program (the surface has no destructor, so it cannot own an object): every callback makes the ProgramSDF over it
// -- a view, three words read from the handle -- and goes through the class, so that the C surface and a C++ host's ProgramSDF
// are one code path.  Nothing crosses the C boundary: an exception becomes a non-zero status.
template <class F>
int through_program_sdf(void* user, F&& body) {
    try {
        const ProgramSDF sdf(static_cast<const sdfv_program*>(user));
        body(sdf);
        return 0;
    } catch (...) {
        return 1;
    }
}
void cb_bounding_box(void* user, float out[6]) {
    through_program_sdf(user, [&](const ProgramSDF& sdf) {
        box_floats(sdf.bounding_box(), out);
    });
}
int cb_sample_batch(void* user, const float* p, size_t n, int distance_only, sdfv_sample* out) {
    static_assert(sizeof(Vec3) == 12, "points are handed over as 3 floats each");
    return through_program_sdf(user, [&](const ProgramSDF& sdf) {
        sdf.sample_batch(reinterpret_cast<const Vec3*>(p), n, distance_only != 0, reinterpret_cast<SDFSample*>(out));
    });
}
int cb_sample(void* user, const float p[3], int distance_only, sdfv_sample* out) {
    return through_program_sdf(user, [&](const ProgramSDF& sdf) {
        const SDFSample s = sdf.sample(Vec3{p[0], p[1], p[2]}, distance_only != 0);
        memcpy(out, &s, sizeof(s));
    });
}
uint32_t cb_sample_concurrency(void* user) {
    uint32_t n = 1;
    through_program_sdf(user, [&](const ProgramSDF& sdf) { n = sdf.sample_concurrency(); });
    return n;
}
int cb_sample_batch_device(void* user, const float* points_dev, size_t n, sdfv_sample* out_dev, void* stream) {
    return through_program_sdf(user, [&](const ProgramSDF& sdf) { sdf.sample_batch_device(points_dev, n, out_dev, stream); });
}

}  // namespace

ProgramSDF::ProgramSDF(const sdfv_program* program) : program_(program) {
    if (sdfv_program_ops(program, &ops_, &n_ops_, bb_) != SDFV_OK) throw std::invalid_argument(sdfv_last_error());
}

BoundingBox ProgramSDF::bounding_box() const { return {Vec3{bb_[0], bb_[1], bb_[2]}, Vec3{bb_[3], bb_[4], bb_[5]}}; }

SDFSample ProgramSDF::sample(Vec3 p, bool distance_only) const {
    SDFSample out;
    evaluate(ops_, n_ops_, &p.x, distance_only, reinterpret_cast<sdfv_sample*>(&out));
    return out;
}

void ProgramSDF::sample_batch(const Vec3* p, size_t n, bool distance_only, SDFSample* out) const {
    for (size_t i = 0; i < n; ++i) evaluate(ops_, n_ops_, &p[i].x, distance_only, reinterpret_cast<sdfv_sample*>(out + i));
}

bool ProgramSDF::has_device_sampler() const { return sdfv_device_count() > 0; }

void ProgramSDF::sample_batch_device(const float* points_dev, size_t n, sdfv_sample* out_dev, void* stream) const {
    if (sdfv_program_sample_points(program_, points_dev, n, 0, out_dev, stream) != SDFV_OK)
        throw std::runtime_error(sdfv_last_error());
}

void ProgramSDF::raymarch(const sdfv_program_march_desc& d, float normal_h, bool srgb_round, int n_threads) const {
    sdfv::pmarch::Frame f;
    f.ops = ops_;
    f.n_ops = (uint32_t)n_ops_;
    f.width = d.width;
    f.height = d.height;
    f.normal_h = normal_h;
    f.air_dist = sdfv_air_dist();
    f.srgb_round = srgb_round ? 1u : 0u;
    f.rp = *d.rp;
    const uint32_t rows = d.y1 - d.y0;
    const uint64_t n_rows = (uint64_t)rows * d.n_cameras;
    if (n_rows == 0 || d.width == 0) return;
    // rows are dealt out one at a time: a row across the object costs many times a row of background
    std::atomic<uint64_t> next{0};
    const auto work = [&](unsigned) {
        for (uint64_t r = next.fetch_add(1, std::memory_order_relaxed); r < n_rows; r = next.fetch_add(1, std::memory_order_relaxed)) {
            const uint32_t c = (uint32_t)(r / rows), row = (uint32_t)(r % rows);
            for (uint32_t x = 0; x < d.width; ++x) {
                const uint64_t o = ((uint64_t)c * rows + row) * d.width + x;
                float4 rgba;
                sdfv_march_aux aux;
                sdfv::pmarch::march_pixel_program(f, d.cameras[c], x, d.y0 + row, true, sdfv::kSrgbToLinear, rgba, aux);
                if (d.rgba) {
                    float* out = d.rgba + o * 4;
                    out[0] = rgba.x; out[1] = rgba.y; out[2] = rgba.z; out[3] = rgba.w;
                }
                if (d.rgba8) d.rgba8[o] = sdfv::rgba_unorm8(rgba);
                if (d.depth) d.depth[o] = aux.depth;
                if (d.aux) d.aux[o] = aux;
            }
        }
    };
    unsigned n = n_threads > 0 ? (unsigned)n_threads : WorkerPool::usable_cpus();
    if ((uint64_t)n > n_rows) n = (unsigned)n_rows;
    WorkerPool pool;
    pool.begin(n);
    try {
        pool.run(n, work);
    } catch (...) {
        pool.end();
        throw;
    }
    pool.end();
}

void ProgramSDF::cast(const sdfv_program_cast_desc& d, int n_threads) const {
    if (d.n == 0) return;
    sdfv::pcast::Cast c;
    c.ops = ops_;
    c.n_ops = (uint32_t)n_ops_;
    c.flags = d.flags;
    for (int a = 0; a < 3; ++a) {
        c.bounds_min[a] = d.bb_min ? d.bb_min[a] : bb_[a];
        c.bounds_max[a] = d.bb_max ? d.bb_max[a] : bb_[3 + a];
    }
    c.max_steps = d.max_steps;
    c.hit_eps = d.hit_eps;
    c.normal_eps = d.normal_eps;
    // the list is dealt out in runs of 256 rays: a run across the object costs many times a run of misses
    constexpr uint64_t kRun = 256;
    const uint64_t n_runs = (d.n + kRun - 1) / kRun;
    const sdfv::prog::Interpreter eval{ops_, (uint32_t)n_ops_};
    std::atomic<uint64_t> next{0};
    const auto work = [&](unsigned) {
        for (uint64_t r = next.fetch_add(1, std::memory_order_relaxed); r < n_runs; r = next.fetch_add(1, std::memory_order_relaxed)) {
            const uint64_t end = (r + 1) * kRun < d.n ? (r + 1) * kRun : d.n;
            for (uint64_t i = r * kRun; i < end; ++i) {
                sdfv_ray ray;  // (the arrays need no more than 4-byte alignment)
                sdfv_ray_hit hit;
                memcpy(&ray, d.rays + i, sizeof(ray));
                sdfv::pcast::cast_ray_program(c, eval, ray, true, hit);
                memcpy(d.hits + i, &hit, sizeof(hit));
            }
        }
    };
    unsigned n = n_threads > 0 ? (unsigned)n_threads : WorkerPool::usable_cpus();
    if ((uint64_t)n > n_runs) n = (unsigned)n_runs;
    WorkerPool pool;
    pool.begin(n);
    try {
        pool.run(n, work);
    } catch (...) {
        pool.end();
        throw;
    }
    pool.end();
}

}  // namespace sdfviewer

extern "C" int sdfv_program_raycast_host(const sdfv_program_cast_desc* desc) {
    sdfv_program_cast_desc d;
    if (int rc = sdfv_program_raycast_check(desc, &d)) return rc;
    try {  // nothing crosses the C boundary
        sdfviewer::ProgramSDF(d.program).cast(d, 0);
    } catch (...) {
        return SDFV_ERR_INVALID_ARGUMENT;
    }
    return SDFV_OK;
}

extern "C" int sdfv_program_raymarch_host(const sdfv_program_march_desc* desc, int n_threads) {
    sdfv_program_march_desc d;
    float h = 0.0f;
    if (int rc = sdfv_program_raymarch_check(desc, &d, &h)) return rc;
    uint64_t srgb_round = 0;
    if (int rc = sdfv_get_option(SDFV_OPT_EXT_SRGB_QUANT, &srgb_round)) return rc;
    try {  // nothing crosses the C boundary
        sdfviewer::ProgramSDF(d.program).raymarch(d, h, srgb_round != 0, n_threads);
    } catch (...) {
        return SDFV_ERR_INVALID_ARGUMENT;
    }
    return SDFV_OK;
}

// (libsdfviewer_host.so is built with default visibility: exported there, hidden in the test and provider libraries)
extern "C" int sdfv_program_as_surface(const sdfv_program* p, sdfv_surface* out) {
    if (!p || !out) return SDFV_ERR_INVALID_ARGUMENT;
    bool device = false;
    if (sdfviewer::through_program_sdf(const_cast<sdfv_program*>(p), [&](const sdfviewer::ProgramSDF& sdf) { device = sdf.has_device_sampler(); }))
        return SDFV_ERR_INVALID_ARGUMENT;
    sdfv_surface s = {};
    s.user = const_cast<sdfv_program*>(p);
    s.bounding_box = sdfviewer::cb_bounding_box;
    s.sample = sdfviewer::cb_sample;
    s.sample_batch = sdfviewer::cb_sample_batch;
    s.sample_concurrency = sdfviewer::cb_sample_concurrency;
    s.sample_batch_device = device ? sdfviewer::cb_sample_batch_device : nullptr;
    *out = s;
    return SDFV_OK;
}
