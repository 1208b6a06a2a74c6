// march_plan.h -- the launch plan of the grid march: everything that is decided on the host before raymarch_kernel starts, as
// plain C++17 (no kernel, no launch, no thread-local option): what the render parameters imply, which of the instantiated
// kernels a launch takes and over which volume, the tile order with its box-first rectangle, the occupancy cap, and how a batch
// of cameras is cut into launches.  march_plan.cpp is compiled into the library and, as it stands, into a CPU test program
// (tests/c/march_plan_check.cpp); the kernel's half of the tile order is march_tile_order.h.
#pragma once

#include "raymarch_kernels.h"

namespace sdfv {

// Everything RaymarchArgs derives from the render parameters alone (exactness flags, tap sizes, cull sphere); `disable` is the
// SDFV_RM_NO_* mask of SDFV_OPT_RAYMARCH_DISABLE.  Clears `a` first.
void derive_raymarch_args(const sdfv_render_params* rp, uint32_t disable, RaymarchArgs& a);

// What a launch is told beyond its render parameters: three facts about the device and three of the caller's options.
struct MarchPolicy {
    bool gfx950;                      // the hand-written loop is gfx950 code (anything else takes the compiler's loop, bit-identical)
    uint32_t cus, xcds;               // the XCD-aware tile orders assume the workgroup -> XCD placement L % 8 of an eight-XCD part
    uint64_t last_level_cache_bytes;  // 0 = unknown
    uint32_t tile_group;              // SDFV_OPT_RAYMARCH_TILE_GROUP: 0 auto, 1 launch order, v >= 2: groups of 2^(v-1) x 2^(v-1) tiles
    uint32_t waves_per_simd;          // SDFV_OPT_RAYMARCH_WAVES_PER_SIMD: 0 = the occupancy rule, 7 = never cap, 2..6 = that cap
    uint32_t box_first;               // SDFV_OPT_RAYMARCH_BOX_FIRST
};
// ... into group_shift, rotate_columns, waves_per_simd, box_first, asm_loop, wave_slots_per_simd_unit, last_level_cache_bytes
// of a call that renders n_cameras (speed only, asm_loop apart: which of two bit-identical loops runs).
void apply_march_policy(RaymarchArgs& a, const MarchPolicy& p, uint32_t n_cameras);

bool asm_addressing_ok(const RaymarchArgs& a);
bool hand_written_loop_applies(const RaymarchArgs& a);
bool volume_fits_loop(const RaymarchArgs& a, int mode);
// would the launcher march over a pair (kind kMarchPairs) / y-interleaved (kind kMarchIlv) volume for these arguments, pointers apart?
bool march_volume_applicable(const RaymarchArgs& a, int kind);
// the launcher's choice among the volumes taken as present: kMarchIlv, kMarchPairs, or 0 = neither (dist / tex0.r is marched)
int march_volume_choice(const RaymarchArgs& a, bool have_dist, bool have_pairs, bool have_ilv);
int march_volume_mode(const RaymarchArgs& a);  // ... among the volumes `a` points to

// The kernel a launch takes (DESIGN.md 3.3 has this as a table).  The pair / interleaved volumes are acceleration structures
// of the hand-written loop only: wherever that loop's specialisation does not apply the march reads the distance volume /
// tex0.r as before -- the same bits either way.
struct MarchKernel {
    int mode;                // kMarch*
    bool linear;             // LINEAR filter (lod_dist_between_samples == 1), else sdfSampleRawNearest or (kMarchLattice) the lattice filter
    int xf;                  // 0 = IEEE divide, 1 = exact power-of-two reciprocal, 2 = ... and the fused scale (fast march only)
    bool symm;               // |p| - max for the out-of-bounds distance (fast march with xf >= 1 only)
    bool hand_written_loop;  // ASM
};
// lod_filter: SDFV_OPT_RAYMARCH_LOD_FILTER, read only when rp.lod_dist_between_samples != 1
MarchKernel select_march_kernel(const RaymarchArgs& a, uint32_t lod_filter);

// Every instantiated raymarch_kernel, one line per (MODE, LINEAR, XF, SYMM, ASM): the launcher's switch is generated from this
// list (raymarch_kernels.hip: launch_selected), and the CPU test holds select_march_kernel to it.
#define SDFV_MARCH_VARIANTS(X)          \
    X(kMarchIlv, true, 2, true, true)       \
    X(kMarchPairs, true, 2, true, true)     \
    X(kMarchDist, true, 2, true, true)      \
    X(kMarchDist, true, 2, true, false)     \
    X(kMarchDist, true, 2, false, false)    \
    X(kMarchDist, true, 1, true, false)     \
    X(kMarchDist, true, 1, false, false)    \
    X(kMarchDist, true, 0, false, false)    \
    X(kMarchTex0, true, 2, true, true)      \
    X(kMarchTex0, true, 2, true, false)     \
    X(kMarchTex0, true, 2, false, false)    \
    X(kMarchTex0, true, 1, true, false)     \
    X(kMarchTex0, true, 1, false, false)    \
    X(kMarchTex0, true, 0, false, false)    \
    X(kMarchGeneral, true, 1, false, false) \
    X(kMarchGeneral, true, 0, false, false) \
    X(kMarchGeneral, false, 1, false, false) \
    X(kMarchGeneral, false, 0, false, false) \
    X(kMarchLattice, false, 1, false, false) \
    X(kMarchLattice, false, 0, false, false)
constexpr int variant_key(int mode, bool linear, int xf, bool symm, bool hand_written_loop) {
    return mode | (linear ? 8 : 0) | (xf << 4) | (symm ? 64 : 0) | (hand_written_loop ? 128 : 0);
}
bool march_variant_instantiated(const MarchKernel& k);

// Screen rectangle (in groups of tiles) of the bounding box seen from camera 0, for the box-first launch order; reads
// group_shift and groups_x, writes first_* and m_* (first_w == 0: the order is off).
void box_first_rectangle(RaymarchArgs& ag, uint32_t groups_y);
// Resident waves per SIMD for this launch (7 = what the register file allows = no cap), and the unused dynamic LDS that caps them.
uint32_t occupancy_rule(const RaymarchArgs& ag);
uint32_t lds_cap_for(uint32_t waves_per_simd);

// One launch, planned: the arguments completed (tile order, box-first rectangle, LDS cap), the kernel and the grid.  A grid
// with a zero in it has nothing to render.
struct MarchLaunch {
    RaymarchArgs args;
    MarchKernel kernel;
    dim3 grid;
};
MarchLaunch plan_march_launch(const RaymarchArgs& a, uint32_t lod_filter);

// Cameras per launch.  Up to kInlineCameras ride in the kernel-argument block.  A larger batch is read from device memory, so
// that kMaxCamerasPerLaunch of them still make ONE launch: the caller's own array if that is where it lies (read in place, for
// any count), else a stream-ordered staging copy per launch -- unless the stream is being captured (the staging ring's events
// do not belong in somebody's graph) or SDFV_OPT_RAYMARCH_CAMERA_STAGING is off: then launches of kInlineCameras (same pixels).
enum class CameraSource { kInline, kInPlace, kStaged };
CameraSource camera_source(uint32_t n_cameras, bool on_device, bool capturing, bool staging);
inline uint32_t cameras_per_launch(CameraSource s) { return s == CameraSource::kInline ? kInlineCameras : kMaxCamerasPerLaunch; }
// Several launches, each small, overlap on side streams (tools/split_balance.py: a launch of 17 000 workgroups gains 34 % from
// overlapping with its siblings, one of 35 000 11 %, one of 65 000 nothing, one of 130 000 loses 4 %).
bool launches_overlap(uint32_t n_cameras, uint32_t per_launch, uint64_t groups_per_launch);

}  // namespace sdfv
