// load_state.hpp -- what an SDFViewer KNOWS about its grid, and the rules between those facts, stated once.
//
// SDFViewer::update has three routes (sdf_viewer.cpp: whole passes; sdf_viewer_device.cpp: device-sampled runs;
// sdf_viewer_ingest.cpp: host-sampled runs).  All of them, and commit(), read and write the same knowledge.  They tell this
// class what HAPPENED (the events) and ask it what that allows (the decisions); none of them holds a fact of its own.  A wrong
// answer here is silent or slow, never loud: a flag too many gives wrong texels, a flag too few a load 1.5x slower with every
// bit right -- which is why the rules live in one place, free of HIP, where a test can drive them without a device
// (tests/test_load_state_cpu.py).
//
// The facts:
//   fresh          both textures still hold new_voxels' [AIR_DIST; 4] everywhere -- written, or (virgin) only recorded
//   virgin rows    the rows no pass has written hold undefined bytes, logically AIR (GridFacts::undefined_rows / defined_step;
//                  they live in the material because a frame or a download materialises them without the viewer)
//   same load      every pass so far belongs to ONE load: one SDF, one parameter block, no change reported.  Once lost it never
//                  comes back for this viewer.
//   loaded once    some LoadingManager has run to its end over this grid: a later pass without a box finds nothing to do
//   volume         the 4 B/voxel distance volume exists (every fill and pack keeps it equal to tex0.r), in which layout
//   pairs valid    the pair volume commit() built still mirrors the distance volume (GridFacts::pairs_valid; render() reads it)
//   mirror valid   the ingest route's host mirror of tex0.r equals what the device holds
#pragma once

#include <chrono>
#include <cstring>
#include <optional>

#include "sdf_surface.hpp"

namespace sdfviewer {

// The coordinate of voxel `index` along an axis of `dim` voxels over [lo, hi]: index / (dim - 1) * size + min in three
// separately rounded steps (scene/sdf/mod.rs:179-182) -- the kernels' arithmetic.  An axis of one voxel gives 0/0 = NaN.
inline float voxel_coordinate(float index, uint32_t dim, float lo, float hi) {
    const float dm1 = (float)dim - 1.0f, size = hi - lo;
    float p = index / dm1;
    p = p * size;
    p = p + lo;
    return p;
}

// The facts SDFViewerMaterial holds (its render() and the viewer's download() read and materialise them too).
struct GridFacts {
    bool& undefined_rows;
    uint32_t& defined_step;
    bool& pairs_valid;
    const bool& dist_interleaved;
};

class LoadState {
   public:
    explicit LoadState(GridFacts material) : m_(material) {}

    // ---- creation (new_voxels) ----
    // Nothing is written: the initial state is only recorded.  `volume`: the distance volume could be allocated.
    void created_virgin(bool volume) {
        m_.undefined_rows = true;
        m_.defined_step = 0;
        volume_ = volume;
    }

    // ---- the SDF of this update() call: is this still the same load? ----
    // The passes of one load share one SDF and one set of parameters.  Another device SDF (or parameter block) than the one the
    // load began with, another snapshot of a program that is loaded by whole passes (an edit is a new sdfv_program; so is a
    // change between a program and none), or any reported change ends it.  While the grid is fresh there is nothing an earlier
    // pass could have written, so only a reported change counts.
    bool observe(const std::optional<DeviceSDF>& device_sdf, const sdfv_program* whole_pass_program, bool change_reported) {
        const bool other_sdf = device_sdf && (!load_sdf_ || memcmp(&*load_sdf_, &*device_sdf, sizeof(*device_sdf)) != 0);
        if (other_sdf) load_sdf_ = *device_sdf;
        const bool other_program = whole_pass_program != load_program_;
        load_program_ = whole_pass_program;
        if (change_reported || (!fresh_ && (other_sdf || other_program))) same_load_ = false;
        return same_load_;
    }

    // ---- decisions ----
    // The next whole pass (sdfv_fill_grid_pass_ex / sdfv_program_grid_pass): whether the rows no pass has reached must be
    // given their initial state first (SDFViewerMaterial::materialize), and the SDFV_PASS_* flags of the pass once they were.
    //   A pass of a single load without a box knows what it will find (SAME_LOAD): a virgin grid (VIRGIN_GRID: it writes the
    //   rows it visits whole and reads nothing), a fresh one (FRESH_GRID: AIR everywhere), or only what the load's earlier
    //   passes wrote.  A pass that must READ the grid -- a changed box, another SDF mid-load -- gets no flag and a materialised
    //   grid.  A program pass never takes a virgin grid: it is materialised and becomes a fresh one.
    //   EXPECT_NOOP is a hint, not knowledge: the manager the reference runs once a changed box has been worked off
    //   (scene/sdf/mod.rs:146-156, no box any more) scans a loaded grid and finds nothing.  Only when nothing but the layout is
    //   flagged.
    struct Pass {
        bool materialize_first;
        uint32_t flags;
    };
    Pass next_pass(bool has_box, bool program) const {
        const bool known = same_load_ && !has_box;
        Pass p;
        p.materialize_first = m_.undefined_rows && (program || !known);
        const bool virgin = m_.undefined_rows && !p.materialize_first;
        p.flags = known ? (virgin ? SDFV_PASS_VIRGIN_GRID : fresh_ ? SDFV_PASS_FRESH_GRID : 0u) | SDFV_PASS_SAME_LOAD : 0u;
        p.flags |= layout_flag();
        if (loaded_once_ && !has_box && p.flags == layout_flag()) p.flags |= SDFV_PASS_EXPECT_NOOP;
        return p;
    }

    // The layout of the distance volume as sdfv_pack_samples, sdfv_emit_update_points and the fills take it.
    uint32_t layout_flag() const { return volume_ && m_.dist_interleaved ? SDFV_PASS_VOLUME_INTERLEAVED : 0u; }
    bool has_volume() const { return volume_; }

    // Meshing the loaded grid (SDFViewer::mesh): where the lattice's distances are read.  The volume, where it exists, equals
    // tex0.r after every fill, pass, pack and materialisation, at every LOD -- 4 B/voxel against tex0's 16; without one, tex0.
    struct MeshSource {
        bool volume;
        uint32_t layout;  // SDFV_PASS_VOLUME_INTERLEAVED or 0
    };
    MeshSource mesh_source() const { return MeshSource{volume_, layout_flag()}; }
    // ... and whether the rows no pass has reached must be written first: the extraction reads every published voxel's texels.
    bool mesh_materializes_first() const { return m_.undefined_rows; }

    // Does `box` contain every voxel of the grid?  Decided on the voxels' own coordinates, first and last index per axis.  A NaN
    // (a bound, or the 0/0 of an axis with one voxel) fails every comparison: not covered.
    static bool box_covers_grid(const sdfv_grid& g, const BoundingBox& box) {
        const float lo[3] = {box[0].x, box[0].y, box[0].z}, hi[3] = {box[1].x, box[1].y, box[1].z};
        for (int i = 0; i < 3; ++i) {
            const float first = voxel_coordinate(0.0f, g.dims[i], g.bb_min[i], g.bb_max[i]);
            const float last = voxel_coordinate((float)g.dims[i] - 1.0f, g.dims[i], g.bb_min[i], g.bb_max[i]);
            if (!(first >= lo[i] && first <= hi[i] && last >= lo[i] && last <= hi[i])) return false;
        }
        return true;
    }

    // The dense shortcut: may the passes of this manager be replaced by the one dense fill they all converge to?
    //   Nothing handed out yet, a pass left, and a budget that lets every pass be enqueued in this call anyway (a pass is one
    //   asynchronous launch; no intermediate state is observable inside one update() call) -- over a fresh grid with nothing
    //   pending, or for a changed box that contains every voxel (the demo reports its whole bounding box on any parameter edit,
    //   demo/mod.rs:135-144): inside the box update_required holds for every visited voxel, so the passes' common final state
    //   is again the dense fill, which moves 32 B/voxel once instead of re-reading and partly rewriting the grid per pass.
    bool dense_shortcut(size_t iterations_so_far, size_t step, std::chrono::nanoseconds budget, const sdfv_grid& g,
                        const std::optional<BoundingBox>& box) const {
        if (iterations_so_far != 0 || step == 0 || budget < std::chrono::milliseconds(1)) return false;
        return box ? box_covers_grid(g, *box) : fresh_;
    }

    // What the ingest route must do about its host mirror of tex0.r before it reads it.
    enum class Mirror { Valid, AllAir /* nothing has been sampled into this grid */, ReadBack /* the device wrote it */ };
    Mirror mirror() const { return mirror_valid_ ? Mirror::Valid : fresh_ ? Mirror::AllAir : Mirror::ReadBack; }

    // commit(): is there a pair volume to derive from the distance volume?  (An interleaved volume IS the march's volume.)
    bool commit_derives_pairs(bool loaded) const { return volume_ && !m_.dist_interleaved && loaded && !m_.pairs_valid; }

    // ---- events ----
    // update() picked a route that writes tex0.r on the device behind the mirror's back (whole passes, device-sampled runs).
    // At entry, even when the call then launches nothing.
    void device_route_entered() { mirror_valid_ = false; }
    // A whole pass of this step ran.
    void pass_ran(size_t step) {
        fresh_ = false;
        if (m_.undefined_rows) {  // (only virgin passes get here with the rows still undefined)
            m_.defined_step = (uint32_t)step;
            if (step == 1) m_.undefined_rows = false;
        }
        m_.pairs_valid = false;
    }
    // A dense fill ran: it wrote every voxel.
    void dense_fill_ran() {
        fresh_ = false;
        m_.undefined_rows = false;
        m_.pairs_valid = false;
    }
    // A record route is about to pack records (sdfv_pack_samples): this is no longer a load the whole-pass route can assume
    // anything about.
    void records_packed() {
        same_load_ = false;
        load_sdf_.reset();
        fresh_ = false;
        m_.pairs_valid = false;
    }
    // (The grid was materialised: SDFViewerMaterial::materialize clears GridFacts::undefined_rows itself -- a frame or a
    // download does it without the viewer.)
    // A LoadingManager ran to its end.
    void manager_finished() { loaded_once_ = true; }
    // The ingest route: the mirror was rebuilt / holds samples the device never received.
    void mirror_rebuilt() { mirror_valid_ = true; }
    void mirror_lost() { mirror_valid_ = false; }
    // commit() built the pair volume.
    void pairs_built() { m_.pairs_valid = true; }

   private:
    GridFacts m_;
    bool fresh_ = true;
    bool same_load_ = true;
    bool loaded_once_ = false;
    bool volume_ = false;
    bool mirror_valid_ = false;
    std::optional<DeviceSDF> load_sdf_;           // what the load samples ...
    const sdfv_program* load_program_ = nullptr;  // ... or the snapshot, for an SDF that takes whole passes
};

}  // namespace sdfviewer
