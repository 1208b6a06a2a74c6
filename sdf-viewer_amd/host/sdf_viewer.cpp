// sdf_viewer.cpp -- see sdf_viewer.hpp.  Of SDFViewer::update's three routes this file holds the entry and the WHOLE-PASS route
// (the demo tree, an SDF program that opted in): a LoadingManager pass is one launch, a load that fits the call one dense fill.
// What a launch may assume about the grid is LoadState's to say (load_state.hpp).
#include "sdf_viewer.hpp"

#include <hip/hip_runtime_api.h>

#include <cmath>
#include <cstdio>
#include <exception>

namespace sdfviewer {

// ---- DeviceBuffer ----
DeviceBuffer::DeviceBuffer(size_t bytes) : bytes_(bytes) {
    if (bytes && hipMalloc(&ptr_, bytes) != hipSuccess) {
        (void)hipGetLastError();
        ptr_ = nullptr;
    }
}
DeviceBuffer::~DeviceBuffer() {
    if (owned_ && ptr_) (void)hipFree(ptr_);
}
DeviceBuffer& DeviceBuffer::operator=(DeviceBuffer&& o) noexcept {
    if (this != &o) {
        if (owned_ && ptr_) (void)hipFree(ptr_);
        ptr_ = o.ptr_;
        bytes_ = o.bytes_;
        owned_ = o.owned_;
        o.ptr_ = nullptr;
        o.bytes_ = 0;
    }
    return *this;
}

// ---- Camera ----
Camera Camera::new_perspective(uint32_t width, uint32_t height, Vec3 position, Vec3 target, Vec3 up,
                               float fovy_degrees, float z_near, float z_far) {
    Camera c;
    c.viewport_width = width;
    c.viewport_height = height;
    c.position = position;
    c.target = target;
    c.up = up;
    c.fovy_degrees = fovy_degrees;
    c.z_near = z_near;
    c.z_far = z_far;
    return c;
}

sdfv_camera Camera::to_device() const {
    sdfv_camera cam;
    const float aspect = viewport_height ? (float)viewport_width / (float)viewport_height : 1.0f;
    sdfv_camera_look_at(&cam, &position.x, &target.x, &up.x, fovy_degrees, aspect, z_near, z_far);
    return cam;
}

// ---- SDFViewerMaterial ----
sdfv_render_params SDFViewerMaterial::uniforms() const {
    sdfv_render_params rp;
    sdfv_render_params_default(&rp, nullptr);
    rp.bounds_min[0] = voxels_bounds[0].x; rp.bounds_min[1] = voxels_bounds[0].y; rp.bounds_min[2] = voxels_bounds[0].z;
    rp.bounds_max[0] = voxels_bounds[1].x; rp.bounds_max[1] = voxels_bounds[1].y; rp.bounds_max[2] = voxels_bounds[1].z;
    for (int i = 0; i < 3; ++i) rp.tex_size[i] = tex_size[i];
    rp.lod_dist_between_samples = lod_dist_between_samples;
    for (int i = 0; i < 4; ++i) rp.tint[i] = color[i];
    rp.gamma = gamma;
    return rp;
}

int SDFViewerMaterial::materialize(void* stream) const {
    if (!undefined_rows) return 0;
    sdfv_grid g{};
    for (int i = 0; i < 3; ++i) g.dims[i] = tex_size[i];
    g.z_end = g.dims[2];  // (the bounding box plays no part in an initialisation)
    const int rc = sdfv_grid_init_unvisited_ex(&g, defined_step, tex0->f32(), tex1->f32(), dist ? dist->f32() : nullptr,
                                               dist && dist_interleaved ? SDFV_PASS_VOLUME_INTERLEAVED : 0u, stream);
    if (rc == 0) undefined_rows = false;
    return rc;
}

int SDFViewerMaterial::render(const Camera& camera, float* rgba_device, sdfv_march_aux* aux_device, void* stream) const {
    // a frame in the middle of a virgin load reads voxels no pass has written (NEAREST snaps onto the lattice, but
    // MirroredRepeat folds coordinate 1.0 onto voxel N - 1): they must hold the AIR the reference's textures hold
    if (int rc = materialize(stream)) return rc;
    const sdfv_render_params rp = uniforms();
    const sdfv_camera cam = camera.to_device();
    // the distance volume is only meaningful for the fully loaded grid (LINEAR filter, lod == 1)
    const float* d = (dist && lod_dist_between_samples == 1.0f) ? dist->f32() : nullptr;
    if (d && dist_interleaved)  // the volume the fill wrote IS the march's y-interleaved volume
        return sdfv_raymarch_volumes(&rp, tex0->f32(), tex1->f32(), nullptr, nullptr, d, &cam, 1, camera.viewport_width,
                                     camera.viewport_height, 0, camera.viewport_height, rgba_device, nullptr, aux_device, stream);
    // a viewer renders many frames per load: the pair volume commit() built halves the march's gathers (same bits)
    const float* p = (d && pairs && pairs_valid) ? pairs->f32() : nullptr;
    return sdfv_raymarch_volumes(&rp, tex0->f32(), tex1->f32(), d, pairs_interleaved ? nullptr : p, pairs_interleaved ? p : nullptr,
                                 &cam, 1, camera.viewport_width, camera.viewport_height, 0, camera.viewport_height, rgba_device,
                                 nullptr, aux_device, stream);
}

// ---- SDFViewer ----
namespace {
// The distance of tex1 from tex0's end (see the constructor).
constexpr size_t kPlacementSlack = 64u << 10;
size_t default_skew(size_t texture_bytes) {
    return texture_bytes == ((size_t)1 << 28) ? 12288 : (texture_bytes == ((size_t)1 << 30) ? 20480 : 0);
}
}  // namespace

SDFViewer::SDFViewer(std::array<size_t, 3> voxels, const BoundingBox& bb, size_t passes)
    : loading_mgr(voxels, passes), bounding_box(bb) {
    const size_t bytes = voxels[0] * voxels[1] * voxels[2] * 16;
    // Both textures in one block (allocation only, nothing is launched or waited for here).  If the block cannot be had, two
    // plain allocations do.  The distance between them: what MI355X boxes have shown reproducibly since round 1 for the
    // texture sizes that matter (the fill's rate is periodic in the distance between the textures, EXPERIMENTS R4.1,
    // profiles/r04_place_width.json): textures of 256 MiB (256^3 and every other shape of that size) run 6-8 % faster with
    // tex1 12 KiB after tex0's end, textures of 1 GiB with 20 KiB, 4 GiB (512^3) with none.  Anything else: none.  (Rounds 3-5
    // also shipped a run-time probe, SDFViewer::tune(): in two driver runs it cost 100 ms and never beat these constants.)
    const size_t skew = default_skew(bytes);
    block_ = std::make_shared<DeviceBuffer>(2 * bytes + kPlacementSlack);
    if (bytes > 0 && block_->ok()) {
        material.tex0 = std::make_shared<DeviceBuffer>(static_cast<char*>(block_->get()), bytes);
        material.tex1 = std::make_shared<DeviceBuffer>(static_cast<char*>(block_->get()) + bytes + skew, bytes);
    } else {
        block_.reset();
        material.tex0 = std::make_shared<DeviceBuffer>(bytes);
        material.tex1 = std::make_shared<DeviceBuffer>(bytes);
    }
    material.tex_size = {(uint32_t)voxels[0], (uint32_t)voxels[1], (uint32_t)voxels[2]};
    material.voxels_bounds = bb;
}

std::unique_ptr<SDFViewer> SDFViewer::from_bb(const BoundingBox& bb, size_t max_voxels_side, size_t loading_passes) {
    sdfv_grid g;
    if (sdfv_grid_from_bb(&bb[0].x, &bb[1].x, (uint32_t)max_voxels_side, &g) != 0) return nullptr;
    fprintf(stderr, "Using %ux%ux%u voxels (dimensions: %gx%gx%g)\n", g.dims[0], g.dims[1], g.dims[2],
            (double)(bb[1].x - bb[0].x), (double)(bb[1].y - bb[0].y), (double)(bb[1].z - bb[0].z));  // :69-70
    return new_voxels({g.dims[0], g.dims[1], g.dims[2]}, bb, loading_passes);
}

std::unique_ptr<SDFViewer> SDFViewer::new_voxels(std::array<size_t, 3> voxels, const BoundingBox& bb,
                                                 size_t loading_passes, VolumeLayout layout) {
    std::unique_ptr<SDFViewer> v(new SDFViewer(voxels, bb, loading_passes));
    if (!v->material.tex0->ok() || !v->material.tex1->ok()) return nullptr;
    // The reference fills both textures with [AIR_DIST; 4] here (:76-77).  This grid is VIRGIN instead: that state is
    // recorded, not written -- the first update() overwrites every byte of it anyway (36 B/voxel the load never pays for).
    // The compact distance volume (tex0.r, 4 B/voxel) lives next to the textures from the start and every fill keeps
    // it in sync: passes read it for update_required instead of tex0's 16-byte texels, commit() has nothing to derive.
    v->material.dist = std::make_shared<DeviceBuffer>(v->material.tex0->bytes() / 4);
    const bool volume = v->material.dist->ok();
    if (!volume) v->material.dist.reset();  // out of memory: march tex0.r in place, passes read tex0
    v->load_.created_virgin(volume);
    // Beyond the last-level cache the march gathers fastest from the y-interleaved volume (sdfv_march_volume_advice): the
    // fills and passes of THIS viewer write the volume in that layout from the start, so a load ends with the march's volume
    // in place and commit() builds nothing (512^3: 0.70 + 0.20 ms -> 0.70).  Smaller cubic grids keep the plain volume and
    // let commit() derive the pair volume from it.
    if (volume && layout == VolumeLayout::Auto) {
        const sdfv_grid g = v->grid();
        uint32_t kind = SDFV_MARCH_VOLUME_NONE;
        if (sdfv_march_volume_advice(&g, &kind) == 0 && kind == SDFV_MARCH_VOLUME_INTERLEAVED) v->material.dist_interleaved = true;
    } else if (volume && layout == VolumeLayout::Interleaved) {
        if (voxels[1] & 1) return nullptr;  // rows are paired
        v->material.dist_interleaved = true;
    }
    return v;
}

sdfv_grid SDFViewer::grid() const {
    sdfv_grid g;
    for (int i = 0; i < 3; ++i) g.dims[i] = material.tex_size[i];
    g.bb_min[0] = bounding_box[0].x; g.bb_min[1] = bounding_box[0].y; g.bb_min[2] = bounding_box[0].z;
    g.bb_max[0] = bounding_box[1].x; g.bb_max[1] = bounding_box[1].y; g.bb_max[2] = bounding_box[1].z;
    g.z_begin = 0;
    g.z_end = g.dims[2];
    return g;
}

// update(): observe the SDF, renew the manager for a pending box, pick the route.  The whole-pass route below asks LoadState
// (load_state.hpp) what every launch may assume; the rules are stated there.
size_t SDFViewer::update(SDFSurface& sdf, std::chrono::nanoseconds max_delta_time) {
    error_.clear();  // last_error() describes THIS call
    visited_before_throw_ = 0;
    // Check whether the SDF self-reports updates.  (:130-141)
    const auto dev_now = sdf.device_sdf();
    const sdfv_program* prog = sdf.takes_whole_passes() ? sdf.device_program() : nullptr;
    const auto new_box = sdf.changed();
    load_.observe(dev_now, prog, new_box.has_value());
    if (new_box) {
        changed_box = changed_box ? merge_bounding_boxes(*changed_box, *new_box) : *new_box;
        changed_box_while_loading = loading_mgr.len() > 0 || changed_box_while_loading;
    }
    // Another full (3-pass) manager while changes are pending and the manager is idle.  (:146-156)
    if (changed_box && loading_mgr.len() == 0) {
        loading_mgr = LoadingManager(loading_mgr.limits, 3);
        if (!new_box) {
            if (!changed_box_while_loading) changed_box.reset();
            changed_box_while_loading = false;
        }
    }

    const size_t start_iter = loading_mgr.total_iterations();
    const auto dev = sdf.device_sdf();
    if (dev) prog = nullptr;  // (the demo's device form comes first, as in sdfv_surface)
    if (!dev && !prog && sdf.has_device_sampler()) return update_device(sdf, max_delta_time);  // sampled by the caller's kernel
    if (!dev && !prog) return update_host(sdf, max_delta_time);  // any `impl SDFSurface`: sampled on the host, packed on the device
    load_.device_route_entered();
    const sdfv_grid g = grid();
    float* const dist = load_.has_volume() ? material.dist->f32() : nullptr;  // every fill keeps it in sync (+4 B/voxel)
    float box[6];
    const float* box_ptr = box_floats(changed_box, box);
    // From here on a unit of work is one launch over the demo tree (dev) or over an SDF program that opted in (prog,
    // SDFSurface::takes_whole_passes).  The two differ in their entry points only: the pass and the dense fill.
    auto run_pass = [&](uint32_t step) {
        const LoadState::Pass pass = load_.next_pass(changed_box.has_value(), prog != nullptr);
        if (pass.materialize_first && !materialize_grid()) return false;
        const int rc = prog ? sdfv_program_grid_pass(prog, &g, step, box_ptr, tex0_device(), tex1_device(), dist, pass.flags, stream)
                            : sdfv_fill_grid_pass_ex(&dev->params, dev->sdf_id, &g, step, box_ptr, tex0_device(), tex1_device(), dist,
                                                     pass.flags, stream);
        if (rc != 0) error_ = sdfv_last_error();
        return rc == 0;
    };
    auto run_dense = [&] {
        // The demo's dense entry point carries no layout.  Over an interleaved volume the same launch goes through its pass entry
        // point: a step-1 pass in which update_required holds everywhere (a virgin / fresh grid, or a box that covers it) IS the
        // dense fused fill.
        if (!prog && load_.layout_flag()) return run_pass(1u);
        const int rc = prog ? sdfv_program_fill_grid_commit(prog, &g, tex0_device(), tex1_device(), dist, load_.layout_flag(), stream)
                            : sdfv_fill_grid_commit(&dev->params, dev->sdf_id, &g, tex0_device(), tex1_device(), dist, stream);
        if (rc != 0) error_ = sdfv_last_error();
        return rc == 0;
    };
    const auto start_time = std::chrono::steady_clock::now();
    if (load_.dense_shortcut(loading_mgr.total_iterations(), loading_mgr.step_size(), max_delta_time, g, changed_box)) {
        if (!run_dense()) return 0;
        load_.dense_fill_ran();
        // the LoadingManager is advanced exactly as the passes would have advanced it
        while (loading_mgr.step_size() != 0) finish_step(kRestOfPass);
        return loading_mgr.total_iterations() - start_iter;
    }
    bool first = true;
    // "while first || start_time.elapsed() < max_delta_time" with a pass as the unit of work  (:173)
    while (first || std::chrono::steady_clock::now() - start_time < max_delta_time) {
        first = false;
        const size_t step = loading_mgr.step_size();
        if (step == 0) break;  // No more work to do!
        if (!run_pass((uint32_t)step)) break;
        load_.pass_ran(step);
        finish_step(kRestOfPass);
    }
    return loading_mgr.total_iterations() - start_iter;
}

bool SDFViewer::materialize_grid() {
    if (material.materialize(stream) == 0) return true;
    error_ = sdfv_last_error();
    return false;
}

void SDFViewer::finish_step(size_t points) {
    if (points == kRestOfPass) loading_mgr.finish_pass();
    else loading_mgr.advance(points);
    if (loading_mgr.step_size() == 0) load_.manager_finished();
    publish_lod();
}

void SDFViewer::rethrow_described(const char* what, size_t start_iter) {
    visited_before_throw_ = loading_mgr.total_iterations() - start_iter;
    error_ = what;
    try {
        throw;
    } catch (const std::exception& e) {
        error_ += std::string(": ") + e.what();
    } catch (...) {
    }
    throw;
}

// The reference's textures change only in commit(), together with the LOD uniform (scene/sdf/mod.rs:220-239).  Here a
// pass rewrites the device textures the moment it runs, so the uniform that tells the shader how to read them (NEAREST
// snap to the coarse lattice while loading, LINEAR + distance volume when loaded) must move with the data, not with the
// scene's 500 ms commit throttle: a frame rendered between two commits would otherwise sample a half-rewritten grid
// with the filter of the previous state.
void SDFViewer::publish_lod() {
    material.lod_dist_between_samples = std::pow(2.0f, (float)(uint8_t)loading_mgr.passes_left());  // :226
}

void SDFViewer::commit() {
    // tex0.fill / tex1.fill re-upload nothing here: the textures already live on the device.  (:222-234)
    publish_lod();  // idempotent: update() has already published it with the data
    // lod == 1 switches the GL filter to LINEAR (:227-230): the kernel selects the filter from the same uniform.
    // Where the reference uploads both textures there is nothing to move, and nothing to derive either: the compact
    // distance volume the LINEAR march reads has been kept in sync by every fill.  Without one (allocation failed at
    // creation) the march reads tex0.r in place.
    // What a commit of the fully loaded grid does derive is the pair volume: the frames that follow (the reference renders
    // one per repaint) march over it.  12 B/voxel of traffic -- against the reference's re-upload of 32 B/voxel over PCIe.
    // (an interleaved volume is the march's volume: the fills wrote it themselves)
    if (load_.commit_derives_pairs(loading_mgr.step_size() == 0)) {
        const sdfv_grid g = grid();
        if (!material.pairs && !material.no_march_volume) {
            // beyond the last-level cache the interleaved volume (4 B/voxel) marches faster than the pair volume (8)
            uint32_t kind = SDFV_MARCH_VOLUME_PAIRS;
            (void)sdfv_march_volume_advice(&g, &kind);
            material.pairs_interleaved = kind == SDFV_MARCH_VOLUME_INTERLEAVED;
            material.no_march_volume = kind == SDFV_MARCH_VOLUME_NONE;  // (a grid that is not cubic: the distance volume it is)
            if (!material.no_march_volume)
                material.pairs = std::make_shared<DeviceBuffer>(material.dist->bytes() * (material.pairs_interleaved ? 1 : 2));
        }
        if (!material.pairs) return;
        const int rc = !material.pairs->ok() ? -1
                       : material.pairs_interleaved ? sdfv_commit_interleaved(&g, material.dist->f32(), material.pairs->f32(), stream)
                                                    : sdfv_commit_pairs(&g, material.dist->f32(), material.pairs->f32(), stream);
        if (rc == 0)
            load_.pairs_built();
        else {
            material.pairs.reset();  // out of memory: the march keeps reading the distance volume ...
            material.no_march_volume = true;  // ... and later commits do not retry the allocation
        }
    }
}

int SDFViewer::mesh_device(uint32_t algorithm, uint32_t flags, sdfv_mesh* out) {
    if (out) *out = sdfv_mesh{};
    if (load_.mesh_materializes_first()) {
        if (const int rc = material.materialize(stream)) {  // its own status goes through
            error_ = sdfv_last_error();
            return rc;
        }
    }
    // 2^passes_left as a float: a step a grid can have fits 32 bits (the conversion of anything else is not defined)
    const float published = material.lod_dist_between_samples;
    if (!(published >= 1.0f && published <= 2147483648.0f)) {
        error_ = "lod_dist_between_samples " + std::to_string(published) + " is no step of a grid";
        return SDFV_ERR_INVALID_ARGUMENT;
    }
    const LoadState::MeshSource src = load_.mesh_source();
    const sdfv_grid g = grid();
    const int rc = sdfv_grid_mesh_extract(&g, tex0_device(), tex1_device(), src.volume && material.dist ? material.dist->f32() : nullptr,
                                          src.volume && material.dist ? src.layout : 0u, (uint32_t)published, algorithm, flags, out, stream);
    if (rc != SDFV_OK) error_ = sdfv_last_error();
    return rc;
}

bool SDFViewer::mesh(Meshers mesher, bool with_materials, Mesh* out, std::string* err) {
    auto fail = [&](const std::string& m) {
        if (err) *err = m;
        return false;
    };
    if (!out) return fail("out is NULL");
    const auto algorithm = device_algorithm(mesher);
    if (!algorithm) return fail("Unsupported algorithm");
    sdfv_mesh m{};
    if (mesh_device(*algorithm, with_materials ? SDFV_MESH_WITH_MATERIALS : 0u, &m) != SDFV_OK) return fail(error_);
    auto host = take_mesh(m, err);
    if (!host) return false;
    *out = std::move(*host);
    return true;
}

int SDFViewer::download(float* tex0_host, float* tex1_host) const {
    if (material.materialize(stream) != 0) return -1;  // a virgin grid shows new_voxels' [AIR_DIST; 4] like any other
    if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess) return -1;
    if (hipMemcpy(tex0_host, tex0_device(), material.tex0->bytes(), hipMemcpyDeviceToHost) != hipSuccess) return -1;
    if (hipMemcpy(tex1_host, tex1_device(), material.tex1->bytes(), hipMemcpyDeviceToHost) != hipSuccess) return -1;
    return 0;
}

}  // namespace sdfviewer
