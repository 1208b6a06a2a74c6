// sdf_viewer_device.cpp -- SDFViewer::update for an SDF that the application samples on the device itself
// (SDFSurface::has_device_sampler; sdfv_surface.sample_batch_device in include/sdfviewer.h).  See sdf_viewer.hpp.
//
// The reference's loop (src/app/scene/sdf/mod.rs:173-215) with no host round trip per voxel.  Per RUN of consecutive
// LoadingManager points of one pass:
//   1. sdfv_emit_update_points: positions and update_required on the device, the points that need a sample written out in
//      LoadingManager order (their positions and flat indices) with their count;
//   2. the count comes back (one 4-byte copy per run) and sample_batch_device enqueues the caller's sampling of those points on
//      the viewer's stream;
//   3. sdfv_pack_samples packs the records through the emitted indices -- the ingest path's packing, bit for bit.
// The budget is checked between runs, and a run is timed to its end: the host waits for the run's sampling and packing before it
// reads the clock, so no run is left in flight when a call returns.  The first run of a call is small; every further one is
// sized to end within half of what is left even if every voxel of it needs a sample -- at the scan's cost per point plus the
// LARGEST cost per sample seen for this SDF (a run of cheap skips says nothing about the next one), growing by at most 16x,
// as the ingest path sizes its runs.  The voxels a call visits are a prefix of the LoadingManager's remaining order, and the
// return value counts them, as in the reference.  What the route leaves known about the grid: LoadState (load_state.hpp),
// device_route_entered and records_packed.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <exception>

#include "sdf_viewer.hpp"

namespace sdfviewer {

namespace {
constexpr size_t kFirstRun = 4096;             // points of a call's first run
constexpr size_t kDefaultCapacity = 1u << 23;  // points per run at most (44 B of device memory each)
constexpr size_t kCostSamples = 4096;          // a run's cost per sample is taken as a measurement from this many samples on
}  // namespace

struct SDFViewer::DeviceRuns {
    DeviceBuffer points, indices, samples, count, scratch;
    uint32_t* h_count = nullptr;  // pinned
    size_t capacity = 0;
    const SDFSurface* cost_sdf = nullptr;  // the SDF sample_cost was measured on
    double sample_cost = 0.0;              // ... its largest cost per sample (sample_batch_device + packing), seconds
    ~DeviceRuns() {
        if (h_count) (void)hipHostFree(h_count);
    }
    bool reserve(size_t n) {
        if (capacity == n) return true;
        capacity = 0;
        points = DeviceBuffer(n * 12);
        indices = DeviceBuffer(n * 4);
        samples = DeviceBuffer(n * sizeof(sdfv_sample));
        count = DeviceBuffer(4);
        const size_t scratch_bytes = sdfv_emit_update_points_scratch_bytes(n);
        scratch = DeviceBuffer(scratch_bytes);
        if (!h_count && hipHostMalloc(reinterpret_cast<void**>(&h_count), 4, hipHostMallocDefault) != hipSuccess) {
            (void)hipGetLastError();
            h_count = nullptr;
        }
        if (!points.ok() || !indices.ok() || !samples.ok() || !count.ok() || scratch_bytes == 0 || !scratch.ok() || !h_count)
            return false;
        capacity = n;
        return true;
    }
};

size_t SDFViewer::update_device(SDFSurface& sdf, std::chrono::nanoseconds max_delta_time) {
    const size_t start_iter = loading_mgr.total_iterations();
    const auto start_time = std::chrono::steady_clock::now();
    if (loading_mgr.step_size() == 0) return 0;  // No more work to do!
    const sdfv_grid g = grid();
    const size_t n_voxels = (size_t)g.dims[0] * g.dims[1] * g.dims[2];
    if (n_voxels == 0) return 0;
    if (n_voxels > 0x100000000ull) {
        error_ = "device-sampled grids are addressed with 32-bit voxel indices: at most 2^32 voxels";
        return 0;
    }
    if (!load_.has_volume()) {
        error_ = "device-sampled loads read the distance volume, which this viewer could not allocate";
        return 0;
    }
    hipStream_t st = (hipStream_t)stream;
    load_.device_route_entered();
    // update_required reads the distance volume: the rows of a virgin grid no pass has written must hold AIR first
    if (!materialize_grid()) return 0;
    if (!device_runs_) device_runs_ = std::make_shared<DeviceRuns>();
    DeviceRuns& dr = *device_runs_;
    if (!dr.reserve(ingest_capacity ? ingest_capacity : std::min(n_voxels, kDefaultCapacity))) {
        error_ = "cannot allocate the device-sampled load's buffers";
        return 0;
    }
    load_.records_packed();

    const uint32_t flags = load_.layout_flag();
    float* dist = material.dist->f32();
    float box[6];
    const float* box_ptr = box_floats(changed_box, box);
    if (dr.cost_sdf != &sdf) {
        dr.cost_sdf = &sdf;
        dr.sample_cost = 0.0;
    }
    auto fail_run = [&](const char* what) {
        (void)hipGetLastError();
        error_ = std::string("device sampling: ") + what;
    };
    size_t run_len = kFirstRun;
    bool first = true;
    // "while first || start_time.elapsed() < max_delta_time" with a run as the unit of work  (:173)
    while (first || std::chrono::steady_clock::now() - start_time < max_delta_time) {
        first = false;
        const size_t step = loading_mgr.step_size();
        if (step == 0) break;  // No more work to do!
        const size_t n = std::min({run_len, loading_mgr.pass_remaining(), dr.capacity});
        const auto run_start = std::chrono::steady_clock::now();
        if (sdfv_emit_update_points(&g, (uint32_t)step, loading_mgr.cursor(), n, box_ptr, dist, flags, dr.points.f32(),
                                    static_cast<uint32_t*>(dr.indices.get()), static_cast<uint32_t*>(dr.count.get()),
                                    dr.scratch.get(), dr.scratch.bytes(), stream) != 0) {
            error_ = sdfv_last_error();
            break;
        }
        if (hipMemcpyAsync(dr.h_count, dr.count.get(), 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
            hipStreamSynchronize(st) != hipSuccess) {
            fail_run("cannot read the run's point count back");
            break;
        }
        const auto scanned = std::chrono::steady_clock::now();
        const size_t count = *dr.h_count;
        auto* samples = static_cast<sdfv_sample*>(dr.samples.get());
        if (count) {
            try {
                sdf.sample_batch_device(dr.points.f32(), count, samples, stream);  // :193, the caller's kernel
            } catch (...) {
                // nothing of this run has reached the textures and the LoadingManager stays where it is
                rethrow_described("device sampling: the SDF's sample_batch_device failed", start_iter);
            }
            if (sdfv_pack_samples(&g, 0, static_cast<const uint32_t*>(dr.indices.get()), samples, count, tex0_device(),
                                  tex1_device(), dist, flags, stream) != 0) {
                error_ = std::string("device sampling: ") + sdfv_last_error();
                break;
            }
            // the run is timed to its end (and none is left in flight when the call returns)
            if (hipStreamSynchronize(st) != hipSuccess) {
                fail_run("the run's sampling or packing failed on the device");
                break;
            }
        }
        finish_step(n);
        // ---- the next run (next_run_length): every voxel of it may need a sample ----
        const auto now = std::chrono::steady_clock::now();
        const double scan_cost = std::chrono::duration<double>(scanned - run_start).count() / (double)n;
        if (count >= kCostSamples)
            dr.sample_cost = std::max(dr.sample_cost, std::chrono::duration<double>(now - scanned).count() / (double)count);
        const double per_voxel = std::max(std::chrono::duration<double>(now - run_start).count() / (double)n,
                                          scan_cost + dr.sample_cost);
        const double left = std::chrono::duration<double>(max_delta_time - (now - start_time)).count();
        run_len = next_run_length(left, per_voxel, 16.0 * (double)n, dr.capacity);
    }
    return loading_mgr.total_iterations() - start_iter;
}

}  // namespace sdfviewer
