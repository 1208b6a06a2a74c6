// viewer_capi.cpp -- include/sdfviewer.h: SDFViewer and SDFViewerAppScene behind typed opaque handles, over any SDF the caller
// describes as an sdfv_surface (CallbackSDF below).  Exported by libsdfviewer_host.so (built with default visibility); the
// other artefacts that link these sources keep it hidden.
#include <hip/hip_runtime_api.h>

#include <atomic>
#include <chrono>
#include <cstring>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <thread>

#include "../../include/sdfprogram.h"
#include "../../include/sdfviewer.h"
#include "../../include/sdfviewer_mesh.h"
#include "program_editor.hpp"
#include "scene.hpp"
#include "sdf_viewer.hpp"

using namespace sdfviewer;

namespace {

// A callback reported a failure: the call ends with SDFV_ERR_CALLBACK.
struct CallbackError : std::runtime_error {
    using std::runtime_error::runtime_error;
};

// `impl SDFSurface` over an sdfv_surface.  A failing host callback throws on the thread that drives the update; on a worker
// thread (where an exception ends the process) it is recorded and thrown by check_samples() once the run's workers are done.
class CallbackSDF final : public SDFSurface {
   public:
    explicit CallbackSDF(const sdfv_surface& s) : s_(s) {}
    const sdfv_surface& surface() const { return s_; }
    // At the start of every call that may sample: the calling thread, and no failure left over from an earlier call (a worker
    // may have failed in a run that a failure on the calling thread had already ended).  The workers are idle between calls.
    void begin_call() {
        caller_ = std::this_thread::get_id();
        failed_ = false;
    }

    BoundingBox bounding_box() const override {
        float b[6] = {0, 0, 0, 0, 0, 0};
        s_.bounding_box(s_.user, b);
        return {Vec3{b[0], b[1], b[2]}, Vec3{b[3], b[4], b[5]}};
    }
    SDFSample sample(Vec3 p, bool distance_only) const override {
        SDFSample out;
        sample_batch(&p, 1, distance_only, &out);
        return out;
    }
    void sample_batch(const Vec3* p, size_t n, bool distance_only, SDFSample* out) const override {
        static_assert(sizeof(Vec3) == 12, "points are handed over as 3 floats each");
        int rc = 0;
        const char* what = "sample_batch";
        auto* o = reinterpret_cast<sdfv_sample*>(out);
        if (s_.sample_batch) {
            rc = s_.sample_batch(s_.user, &p[0].x, n, distance_only ? 1 : 0, o);
        } else if (s_.sample) {
            what = "sample";
            for (size_t i = 0; i < n && rc == 0; ++i) rc = s_.sample(s_.user, &p[i].x, distance_only ? 1 : 0, o + i);
        } else {
            what = "sample (the surface has no host sampling)";
            rc = -1;
        }
        if (rc == 0) return;
        const std::string msg = std::string("sdfv_surface.") + what + " returned " + std::to_string(rc);
        if (std::this_thread::get_id() == caller_) throw CallbackError(msg);
        for (size_t i = 0; i < n; ++i) out[i] = SDFSample();  // (dropped with the run: check_samples() throws before it is shipped)
        std::lock_guard<std::mutex> lock(m_);
        if (!failed_.exchange(true)) worker_error_ = msg;
    }
    void check_samples() const override {
        if (!failed_.load()) return;
        std::string msg;
        {
            std::lock_guard<std::mutex> lock(m_);
            msg = worker_error_;
            failed_ = false;
        }
        throw CallbackError(msg);
    }
    unsigned sample_concurrency() const override {
        if (!s_.sample_concurrency) return 1;
        const uint32_t n = s_.sample_concurrency(s_.user);
        return n ? n : 1;
    }
    std::optional<BoundingBox> changed() override {
        float b[6];
        if (!s_.changed || s_.changed(s_.user, b) != 1) return std::nullopt;
        return BoundingBox{Vec3{b[0], b[1], b[2]}, Vec3{b[3], b[4], b[5]}};
    }
    std::optional<DeviceSDF> device_sdf() const override {
        if (!s_.device_params) return std::nullopt;
        return DeviceSDF{*s_.device_params, s_.device_sdf_id};
    }
    bool has_device_sampler() const override { return s_.sample_batch_device != nullptr; }
    void sample_batch_device(const float* points_dev, size_t n, sdfv_sample* out_dev, void* stream) const override {
        const int rc = s_.sample_batch_device(s_.user, points_dev, n, out_dev, stream);
        if (rc != 0) throw CallbackError("sdfv_surface.sample_batch_device returned " + std::to_string(rc));
    }

   private:
    sdfv_surface s_;
    std::thread::id caller_;
    mutable std::mutex m_;
    mutable std::atomic<bool> failed_{false};
    mutable std::string worker_error_;
};

int check_surface(const sdfv_surface* s, std::string& err) {
    if (!s) return err = "surface is NULL", SDFV_ERR_INVALID_ARGUMENT;
    if (!s->bounding_box) return err = "sdfv_surface.bounding_box is required", SDFV_ERR_INVALID_ARGUMENT;
    if (!s->sample && !s->sample_batch && !s->sample_batch_device && !s->device_params)
        return err = "sdfv_surface needs sample, sample_batch, sample_batch_device or device_params", SDFV_ERR_INVALID_ARGUMENT;
    return SDFV_OK;
}

// The adapter of `s`: the previous one while the caller hands over the same struct (the ingest path keeps what it measured
// about an SDF per adapter), a new one otherwise.
std::shared_ptr<CallbackSDF> adapter_for(std::shared_ptr<CallbackSDF>& cached, const sdfv_surface& s) {
    if (!cached || memcmp(&cached->surface(), &s, sizeof(s)) != 0) cached = std::make_shared<CallbackSDF>(s);
    cached->begin_call();
    return cached;
}

int need_device() {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0) {
        (void)hipGetLastError();
        return SDFV_ERR_NO_DEVICE;
    }
    return SDFV_OK;
}

template <class F>
int guarded(std::string& err, F&& body) {
    try {
        err.clear();
        return body();
    } catch (const CallbackError& e) {
        err = e.what();
        return SDFV_ERR_CALLBACK;
    } catch (const std::exception& e) {
        err = std::string("internal error: ") + e.what();
        return SDFV_ERR_INTERNAL;
    } catch (...) {
        err = "internal error";
        return SDFV_ERR_INTERNAL;
    }
}

BoundingBox box_of(const float bb[6]) { return {Vec3{bb[0], bb[1], bb[2]}, Vec3{bb[3], bb[4], bb[5]}}; }

Camera camera_of(const sdfv_view& v) {
    return Camera::new_perspective(0, 0, Vec3{v.position[0], v.position[1], v.position[2]}, Vec3{v.target[0], v.target[1], v.target[2]},
                                   Vec3{v.up[0], v.up[1], v.up[2]}, v.fovy_degrees, v.z_near, v.z_far);
}

}  // namespace

struct sdfv_viewer {
    std::unique_ptr<SDFViewer> owned;  // (null for the view of a scene's viewer)
    SDFViewer* v = nullptr;
    std::shared_ptr<CallbackSDF> sdf;
    std::string err;
};

struct sdfv_scene {
    std::unique_ptr<SDFViewerAppScene> scene;
    std::shared_ptr<CallbackSDF> sdf;
    sdfv_viewer view;  // the scene's current viewer, borrowed
    sdfv_clock_fn clock = nullptr;
    void* clock_user = nullptr;
    std::string err;
};

namespace {
int wrap_viewer(std::unique_ptr<SDFViewer> v, sdfv_viewer** out) {
    if (!v) return SDFV_ERR_INTERNAL;
    auto* h = new sdfv_viewer();
    h->v = v.get();
    h->owned = std::move(v);
    *out = h;
    return SDFV_OK;
}

// One SDFViewer::update over the SDF that `pick` returns (or NULL and the error code it refuses with): *visited on success
// and on a throw, last_error() as SDFV_ERR_HIP.
template <class Pick>
int update_viewer(sdfv_viewer* v, uint64_t budget_ns, size_t* visited, Pick&& pick) {
    if (visited) *visited = 0;
    if (!v || !v->v) return SDFV_ERR_INVALID_ARGUMENT;
    return guarded(v->err, [&] {
        int rc = SDFV_OK;
        SDFSurface* sdf = pick(rc);
        if (!sdf) return rc;
        const auto budget = std::chrono::nanoseconds((long long)std::min<uint64_t>(budget_ns, (uint64_t)INT64_MAX));
        size_t n = 0;
        try {
            n = v->v->update(*sdf, budget);
        } catch (...) {
            if (visited) *visited = v->v->visited_before_throw();  // (the runs packed before the one that failed)
            throw;
        }
        if (visited) *visited = n;
        if (v->v->last_error()[0]) {
            v->err = v->v->last_error();
            return (int)SDFV_ERR_HIP;
        }
        return (int)SDFV_OK;
    });
}
}  // namespace

extern "C" {

uint32_t sdfv_viewer_abi_version(void) { return SDFV_VIEWER_ABI_VERSION; }

int sdfv_viewer_from_bb(const float bb[6], uint32_t max_voxels_side, uint32_t loading_passes, sdfv_viewer** out) {
    if (!bb || !out) return SDFV_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    if (int rc = need_device()) return rc;
    try {
        return wrap_viewer(SDFViewer::from_bb(box_of(bb), max_voxels_side, loading_passes), out);
    } catch (...) {
        return SDFV_ERR_INTERNAL;
    }
}

int sdfv_viewer_new_voxels(const uint32_t dims[3], const float bb[6], uint32_t loading_passes, sdfv_volume_layout layout,
                           sdfv_viewer** out) {
    if (!dims || !bb || !out || (unsigned)layout > SDFV_LAYOUT_INTERLEAVED)
        return SDFV_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    if (int rc = need_device()) return rc;
    try {
        return wrap_viewer(SDFViewer::new_voxels({dims[0], dims[1], dims[2]}, box_of(bb), loading_passes,
                                                 (SDFViewer::VolumeLayout)layout),
                           out);
    } catch (...) {
        return SDFV_ERR_INTERNAL;
    }
}

int sdfv_viewer_update(sdfv_viewer* v, const sdfv_surface* surface, uint64_t budget_ns, size_t* visited) {
    return update_viewer(v, budget_ns, visited, [&](int& rc) -> SDFSurface* {
        rc = check_surface(surface, v->err);
        return rc ? nullptr : adapter_for(v->sdf, *surface).get();  // (v->sdf keeps it alive)
    });
}

// include/sdfprogram.h: the same call with the editor's own class as the SDF, which opts in to whole passes
int sdfv_viewer_update_program(sdfv_viewer* v, sdfv_program_editor* e, uint64_t budget_ns, size_t* visited) {
    return update_viewer(v, budget_ns, visited, [&](int& rc) -> SDFSurface* {
        if (e && e->sdf) return e->sdf.get();
        v->err = "editor is NULL";
        rc = SDFV_ERR_INVALID_ARGUMENT;
        return nullptr;
    });
}

// include/sdfviewer_mesh.h: SDFViewer::mesh_device
int sdfv_viewer_mesh(sdfv_viewer* v, uint32_t algorithm, uint32_t flags, sdfv_mesh* out) {
    if (out) memset(out, 0, sizeof(*out));
    if (!v || !v->v || !out) return SDFV_ERR_INVALID_ARGUMENT;
    return guarded(v->err, [&] {
        const int rc = v->v->mesh_device(algorithm, flags, out);
        if (rc != SDFV_OK) v->err = v->v->last_error();
        return rc;
    });
}

int sdfv_viewer_commit(sdfv_viewer* v) {
    if (!v || !v->v) return SDFV_ERR_INVALID_ARGUMENT;
    return guarded(v->err, [&] {
        v->v->commit();
        return (int)SDFV_OK;
    });
}

int sdfv_viewer_state(const sdfv_viewer* v, sdfv_load_state* out) {
    if (!v || !v->v || !out) return SDFV_ERR_INVALID_ARGUMENT;
    const SDFViewer& w = *v->v;
    out->remaining = w.loading_mgr.len();
    out->total_iterations = w.loading_mgr.total_iterations();
    out->passes_left = (uint32_t)w.loading_mgr.passes_left();
    out->has_changed_box = w.changed_box ? 1u : 0u;
    out->lod_dist_between_samples = w.material.lod_dist_between_samples;
    for (int i = 0; i < 3; ++i) out->dims[i] = w.material.tex_size[i];
    return SDFV_OK;
}

int sdfv_viewer_textures(const sdfv_viewer* v, float** tex0, float** tex1, sdfv_grid* grid) {
    if (!v || !v->v) return SDFV_ERR_INVALID_ARGUMENT;
    // a virgin grid's unvisited rows hold new_voxels' [AIR_DIST; 4] once somebody else reads them
    if (v->v->material.materialize(v->v->stream) != 0) {
        const_cast<sdfv_viewer*>(v)->err = sdfv_last_error();
        return SDFV_ERR_HIP;
    }
    if (tex0) *tex0 = v->v->tex0_device();
    if (tex1) *tex1 = v->v->tex1_device();
    if (grid) *grid = v->v->grid();
    return SDFV_OK;
}

int sdfv_viewer_download(sdfv_viewer* v, float* tex0_host, float* tex1_host) {
    if (!v || !v->v || !tex0_host || !tex1_host) return SDFV_ERR_INVALID_ARGUMENT;
    return guarded(v->err, [&] {
        if (v->v->download(tex0_host, tex1_host) != 0) {
            (void)hipGetLastError();
            v->err = "cannot download the textures";
            return (int)SDFV_ERR_HIP;
        }
        return (int)SDFV_OK;
    });
}

int sdfv_viewer_render(sdfv_viewer* v, const sdfv_view* view, uint32_t width, uint32_t height, float* rgba_device) {
    if (!v || !v->v || !rgba_device) return SDFV_ERR_INVALID_ARGUMENT;
    return guarded(v->err, [&] {
        Camera cam;  // the scene's default camera (scene/mod.rs:82-95)
        if (view) cam = camera_of(*view);
        cam.set_viewport(width, height);
        if (v->v->material.render(cam, rgba_device, nullptr, v->v->stream) != 0) {
            v->err = sdfv_last_error();
            return (int)SDFV_ERR_HIP;
        }
        return (int)SDFV_OK;
    });
}

int sdfv_viewer_set_stream(sdfv_viewer* v, void* stream) {
    if (!v || !v->v) return SDFV_ERR_INVALID_ARGUMENT;
    v->v->stream = stream;
    return SDFV_OK;
}

int sdfv_viewer_set_ingest(sdfv_viewer* v, uint32_t host_threads, size_t capacity) {
    if (!v || !v->v) return SDFV_ERR_INVALID_ARGUMENT;
    v->v->host_threads = host_threads;
    v->v->ingest_capacity = capacity;
    return SDFV_OK;
}

const char* sdfv_viewer_last_error(const sdfv_viewer* v) { return v ? v->err.c_str() : "viewer is NULL"; }

void sdfv_viewer_free(sdfv_viewer* v) {
    if (v && v->owned) delete v;  // (a scene's view belongs to the scene)
}

// ---- the scene ----
int sdfv_scene_new(const sdfv_surface* surface, sdfv_clock_fn clock, void* clock_user, sdfv_scene** out) {
    if (!out) return SDFV_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    std::string err;
    if (int rc = check_surface(surface, err)) return rc;
    if (int rc = need_device()) return rc;
    auto* h = new sdfv_scene();
    h->clock = clock;
    h->clock_user = clock_user;
    const int rc = guarded(h->err, [&] {
        SDFViewerAppScene::Clock c;
        if (clock) c = [h] { return std::chrono::steady_clock::time_point(std::chrono::nanoseconds((long long)h->clock(h->clock_user))); };
        h->scene.reset(new SDFViewerAppScene(adapter_for(h->sdf, *surface), c));
        return h->scene->sdf_viewer ? (int)SDFV_OK : (int)SDFV_ERR_INTERNAL;
    });
    if (rc != SDFV_OK) {
        delete h;
        return rc;
    }
    *out = h;
    return SDFV_OK;
}

int sdfv_scene_set_surface(sdfv_scene* s, const sdfv_surface* surface, uint32_t max_voxels_side, uint32_t loading_passes) {
    if (!s) return SDFV_ERR_INVALID_ARGUMENT;
    return guarded(s->err, [&] {
        if (int rc = check_surface(surface, s->err)) return rc;
        const bool ok = s->scene->set_sdf(adapter_for(s->sdf, *surface),
                                          max_voxels_side ? std::optional<size_t>(max_voxels_side) : std::nullopt,
                                          loading_passes ? std::optional<size_t>(loading_passes) : std::nullopt);
        if (!ok) {
            s->err = "cannot create the viewer for this surface";
            return (int)SDFV_ERR_INTERNAL;
        }
        return (int)SDFV_OK;
    });
}

int sdfv_scene_set_camera(sdfv_scene* s, const sdfv_view* view) {
    if (!s || !view) return SDFV_ERR_INVALID_ARGUMENT;
    s->scene->camera = camera_of(*view);
    return SDFV_OK;
}

int sdfv_scene_set_budget(sdfv_scene* s, uint32_t load_budget_ms, uint32_t commit_interval_ms) {
    if (!s) return SDFV_ERR_INVALID_ARGUMENT;
    s->scene->load_budget = std::chrono::milliseconds(load_budget_ms);
    s->scene->commit_interval = std::chrono::milliseconds(commit_interval_ms);
    return SDFV_OK;
}

int sdfv_scene_render(sdfv_scene* s, uint32_t width, uint32_t height, float* rgba_device, sdfv_render_report* out) {
    if (out) memset(out, 0, sizeof(*out));
    if (!s) return SDFV_ERR_INVALID_ARGUMENT;
    return guarded(s->err, [&] {
        if (s->sdf) s->sdf->begin_call();
        const RenderReport r = s->scene->render(width, height, rgba_device);
        if (out) {
            out->cpu_updates = r.cpu_updates;
            out->committed = r.committed;
            out->last_chunk = r.last_chunk;
            out->request_repaint = r.request_repaint;
        }
        if (s->scene->sdf_viewer && s->scene->sdf_viewer->last_error()[0]) {
            s->err = s->scene->sdf_viewer->last_error();
            return (int)SDFV_ERR_HIP;
        }
        return (int)SDFV_OK;
    });
}

int sdfv_scene_load_progress(const sdfv_scene* s, int* loading, float* progress, char* text, size_t text_len) {
    if (!s || !loading) return SDFV_ERR_INVALID_ARGUMENT;
    const auto p = s->scene->load_progress();
    *loading = p ? 1 : 0;
    if (progress) *progress = p ? p->first : 0.0f;
    if (text && text_len) {
        const std::string t = p ? p->second : std::string();
        strncpy(text, t.c_str(), text_len - 1);
        text[text_len - 1] = 0;
    }
    return SDFV_OK;
}

sdfv_viewer* sdfv_scene_viewer(sdfv_scene* s) {
    if (!s || !s->scene->sdf_viewer) return nullptr;
    s->view.v = s->scene->sdf_viewer.get();
    s->view.sdf = s->sdf;
    return &s->view;
}

const char* sdfv_scene_last_error(const sdfv_scene* s) { return s ? s->err.c_str() : "scene is NULL"; }

void sdfv_scene_free(sdfv_scene* s) { delete s; }

}  // extern "C"
