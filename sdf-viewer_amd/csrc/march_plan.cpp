// march_plan.cpp -- the launch plan of the grid march (march_plan.h): host arithmetic over render parameters, option bits and
// three device facts.  No kernel and no HIP call, so that a CPU test can hold every decision to DESIGN.md 3.3.
#include "march_plan.h"

#include <math.h>
#include <string.h>

#include "march_common.h"

#pragma GCC visibility push(default)
extern "C" void sdfv_render_params_default(sdfv_render_params* rp, const sdfv_grid* grid) {
    if (!rp) return;
    memset(rp, 0, sizeof(*rp));
    for (int i = 0; i < 3; ++i) {
        if (grid) {
            rp->bounds_min[i] = grid->bb_min[i];
            rp->bounds_max[i] = grid->bb_max[i];
            rp->tex_size[i] = grid->dims[i];
        }
        rp->ambient[i] = 1.0f;  // AmbientLight::new(&ctx, 1.0, Srgba::WHITE), scene/mod.rs:106
    }
    rp->lod_dist_between_samples = 1.0f;  // material.rs:28
    rp->tint[0] = rp->tint[1] = rp->tint[2] = rp->tint[3] = 1.0f;  // Srgba::WHITE, material.rs:29
    rp->gamma = 0.0f;
    rp->tone_mapping = 2;   // three-d 0.18 default (ACES)
    rp->color_mapping = 1;  // three-d 0.18 default (compute to sRGB)
}
#pragma GCC visibility pop

namespace sdfv {

void derive_raymarch_args(const sdfv_render_params* rp, uint32_t off, RaymarchArgs& a) {
    memset(&a, 0, sizeof(a));
    a.rp = *rp;
    a.pow2_extent = (off & SDFV_RM_NO_POW2_EXTENT) ? 0u : 1u;
    a.fast_index = (off & SDFV_RM_NO_FAST_INDEX) ? 0u : 1u;
    a.pow2_size = 1;
    a.symmetric_box = 1;
    a.fast_normal = 1;
    float radius2 = 0.0f;
    // sdfNormal's tap offset as the kernels take it (march_common.h): ((sx^2 + sy^2) + sz^2), the order of the loop that stood
    // here -- whose leading 0 + sx^2 was exact -- and unchecked, so that fast_normal is what it was for every input
    const float h_world = march::tap_distance((float)rp->tex_size[0], (float)rp->tex_size[1], (float)rp->tex_size[2],
                                              rp->lod_dist_between_samples);
    for (int i = 0; i < 3; ++i) {
        a.bsize[i] = rp->bounds_max[i] - rp->bounds_min[i];
        a.inv_bsize[i] = 1.0f / a.bsize[i];
        const float n = (float)rp->tex_size[i];
        // a marching ray stays within 1e-4 of the box (material.frag:106): floor(u) in [-1, N-1] needs
        // 1e-4 * N / size well below 0.5; the normal's taps sit h_world further out
        if (!(a.bsize[i] > 0.0f) || !(1e-4f * n / a.bsize[i] <= 0.25f)) a.fast_index = 0;
        if (!(a.bsize[i] > 0.0f) || !((1e-4f + h_world) * n / a.bsize[i] <= 0.45f)) a.fast_normal = 0;
        int e = 0;
        // x / 2^k == x * 2^-k exactly (both correctly rounded), provided 2^-k is itself normal
        if (!(a.bsize[i] > 0.0f) || frexpf(a.bsize[i], &e) != 0.5f || e < -100 || e > 100) a.pow2_extent = 0;
        if (rp->tex_size[i] >= (1u << 24)) a.pow2_size = 0;  // (N as a float is exact below 2^24)
        if (rp->bounds_min[i] != -rp->bounds_max[i]) a.symmetric_box = 0;
        a.cull_center[i] = 0.5f * (rp->bounds_min[i] + rp->bounds_max[i]);
        radius2 += 0.25f * a.bsize[i] * a.bsize[i];
    }
    a.cull_radius2 = radius2 * 1.0201f + 1e-12f;  // (1.01 r)^2
    if (!(a.cull_radius2 > 0.0f) || !isfinite(a.cull_radius2)) a.cull_radius2 = INFINITY;  // never cull
    a.asm_loop = (off & SDFV_RM_NO_ASM_LOOP) ? 0u : 1u;
    a.no_interior_fetch = (off & SDFV_RM_NO_INTERIOR_FETCH) ? 1u : 0u;
    a.cube_box = (a.symmetric_box && rp->bounds_max[0] == rp->bounds_max[1] && rp->bounds_max[1] == rp->bounds_max[2]) ? 1u : 0u;
    if (off & SDFV_RM_NO_SYMMETRIC) a.symmetric_box = 0;
    if (off & SDFV_RM_NO_POW2_SIZE) a.pow2_size = 0;
}

void apply_march_policy(RaymarchArgs& a, const MarchPolicy& p, uint32_t n_cameras) {
    a.waves_per_simd = p.waves_per_simd;
    a.box_first = p.box_first;
    if (!p.gfx950) a.asm_loop = 0;
    a.wave_slots_per_simd_unit = p.cus * 4u;  // SIMDs: resident waves at w per SIMD = w * this
    a.last_level_cache_bytes = p.last_level_cache_bytes;
    // tile order: auto = for a single frame the launcher's XCD-aware choice (groups of 2 x 2 tiles, those under the projected
    // bounding box first; profiles/r02/box_first_*.json, EXPERIMENTS R2-R3), launch order for batches of cameras, which
    // lose 3-8 % with any grouping
    const bool xcd_order_ok = p.xcds == 8;
    a.group_shift = p.tile_group == 0 ? (n_cameras == 1 && xcd_order_ok ? kGroupAuto : 0u) : (p.tile_group == 1 ? 0u : p.tile_group - 1u);
    // launches that keep launch order (batches, tile bands): tile columns rotated by row and camera, so that the XCDs' static
    // shares balance (auto only: SDFV_OPT_RAYMARCH_TILE_GROUP 1 is the plain launch order, for A/B runs)
    a.rotate_columns = p.tile_group == 0 && xcd_order_ok ? 1u : 0u;
}

// The hand-written loop addresses rows and slices by 24-bit multiplies (v_mad_u32_u24: full rate, any size -- not only powers
// of two): row numbers k * H + j and the bytes of a row (16 * W for tex0) must stay below 2^24.
bool asm_addressing_ok(const RaymarchArgs& a) {
    return a.rp.tex_size[0] < (1u << 20) && (uint64_t)a.rp.tex_size[1] * a.rp.tex_size[2] < (1ull << 24);
}

// Does the hand-written loop's specialisation apply to these render parameters?  LINEAR filter, clamp for mirror, the fused
// scale (power-of-two extents, N below 2^24), symmetric box, the loop switched on (gfx950 only: apply_march_policy clears
// asm_loop elsewhere), at least two texels in x (its 8-byte border fetch) and its 24-bit addressing.
bool hand_written_loop_applies(const RaymarchArgs& a) {
    return a.rp.lod_dist_between_samples == 1.0f && a.fast_index && a.pow2_extent && a.pow2_size && a.symmetric_box && a.asm_loop &&
           a.rp.tex_size[0] >= 2 && asm_addressing_ok(a);
}

// Does a volume of this MODE fit the loop's 32-bit byte offsets?  16 B/texel of tex0 and 8 B/texel of pairs reach 2^28 texels
// with the loop's shifts, 4 B/voxel of dist and ilv 2^30.  The interleaved volume pairs rows: H even (and not 0).
bool volume_fits_loop(const RaymarchArgs& a, int mode) {
    const uint64_t texels = (uint64_t)a.rp.tex_size[0] * a.rp.tex_size[1] * a.rp.tex_size[2];
    switch (mode) {
    case kMarchTex0:
    case kMarchPairs: return texels <= (1ull << 28);
    case kMarchDist: return texels <= (1ull << 30);
    case kMarchIlv: return a.rp.tex_size[1] >= 2 && (a.rp.tex_size[1] & 1u) == 0 && texels <= (1ull << 30);
    default: return false;
    }
}

// Pointers apart, everything march_volume_choice decides on for `kind` -- asked BEFORE a volume exists (the advice
// once checked less than the launcher, so a host could be advised a layout no march would ever read and then gather 16-byte
// tex0 texels instead of its 4-byte distance volume).
bool march_volume_applicable(const RaymarchArgs& a, int kind) {
    return (kind == kMarchPairs || kind == kMarchIlv) && hand_written_loop_applies(a) && volume_fits_loop(a, kind);
}

// Which volume the hand-written loop marches over, of those at hand: kMarchIlv, kMarchPairs, or 0 for neither (the loop's
// specialisation does not apply, or neither is there).  With both: the pair volume while its 8 B/voxel fit the last-level
// cache (fewest gathers), the interleaved one beyond (half the footprint) -- profiles/r03_pairs_bench.json.
int march_volume_choice(const RaymarchArgs& a, bool have_dist, bool have_pairs, bool have_ilv) {
    const uint64_t texels = (uint64_t)a.rp.tex_size[0] * a.rp.tex_size[1] * a.rp.tex_size[2];
    // a non-cubic grid never takes the loop's interior fetch (one compare for all three cell indices), and the border fetch of
    // these two volumes is eight single loads against the distance volume's four 8-byte ones: with `dist` at hand, use it
    const bool cubic = a.rp.tex_size[0] == a.rp.tex_size[1] && a.rp.tex_size[1] == a.rp.tex_size[2];
    if (!cubic && have_dist) return 0;
    const bool pairs_ok = have_pairs && march_volume_applicable(a, kMarchPairs);
    const bool ilv_ok = have_ilv && march_volume_applicable(a, kMarchIlv);
    if (pairs_ok && ilv_ok) return (a.last_level_cache_bytes && texels * 8u > a.last_level_cache_bytes) ? kMarchIlv : kMarchPairs;
    return ilv_ok ? kMarchIlv : (pairs_ok ? kMarchPairs : 0);
}

int march_volume_mode(const RaymarchArgs& a) { return march_volume_choice(a, a.dist != nullptr, a.pairs != nullptr, a.ilv != nullptr); }

MarchKernel select_march_kernel(const RaymarchArgs& a, uint32_t lod_filter) {
    MarchKernel k{kMarchGeneral, a.rp.lod_dist_between_samples == 1.0f, a.pow2_extent ? 1 : 0, false, false};
    if (!k.linear && lod_filter == 1) k.mode = kMarchLattice;  // a loading grid under SDFV_OPT_RAYMARCH_LOD_FILTER 1: any box, any size
    if (!k.linear || !a.fast_index) return k;
    k.mode = march_volume_mode(a);
    if (k.mode == 0) k.mode = a.dist ? kMarchDist : kMarchTex0;
    if (a.pow2_extent && a.pow2_size) k.xf = 2;
    k.symm = k.xf >= 1 && a.symmetric_box;
    k.hand_written_loop = hand_written_loop_applies(a) && volume_fits_loop(a, k.mode);
    return k;
}

bool march_variant_instantiated(const MarchKernel& k) {
    switch (variant_key(k.mode, k.linear, k.xf, k.symm, k.hand_written_loop)) {
#define SDFV_VARIANT(MODE, LINEAR, XF, SYMM, ASM) case variant_key(MODE, LINEAR, XF, SYMM, ASM):
        SDFV_MARCH_VARIANTS(SDFV_VARIANT)
#undef SDFV_VARIANT
        return true;
    default: return false;
    }
}

// The eight corners through the same pinhole model as pixel_ray_raw, one pixel of margin.  Order only: any rectangle renders
// the same image, so a corner behind the camera simply switches the ordering off.
void box_first_rectangle(RaymarchArgs& ag, uint32_t groups_y) {
    const sdfv_camera& cam = ag.cameras[0];
    float x_lo = 3.0e38f, x_hi = -3.0e38f, y_lo = 3.0e38f, y_hi = -3.0e38f;
    for (int c = 0; c < 8; ++c) {
        const float p[3] = {(c & 1 ? ag.rp.bounds_max : ag.rp.bounds_min)[0], (c & 2 ? ag.rp.bounds_max : ag.rp.bounds_min)[1],
                            (c & 4 ? ag.rp.bounds_max : ag.rp.bounds_min)[2]};
        const float v[3] = {p[0] - cam.eye[0], p[1] - cam.eye[1], p[2] - cam.eye[2]};
        const float zc = v[0] * cam.forward[0] + v[1] * cam.forward[1] + v[2] * cam.forward[2];
        if (!(zc > 1e-6f)) return;
        const float xc = v[0] * cam.right[0] + v[1] * cam.right[1] + v[2] * cam.right[2];
        const float yc = v[0] * cam.up[0] + v[1] * cam.up[1] + v[2] * cam.up[2];
        const float px = (xc / (zc * cam.aspect * cam.tan_half_fovy) + 1.0f) * 0.5f * (float)ag.width;
        const float py = (1.0f - yc / (zc * cam.tan_half_fovy)) * 0.5f * (float)ag.height - (float)ag.y0;
        if (!(px == px) || !(py == py)) return;
        x_lo = fminf(x_lo, px), x_hi = fmaxf(x_hi, px), y_lo = fminf(y_lo, py), y_hi = fmaxf(y_hi, py);
    }
    const float edge = (float)(16u << ag.group_shift), gxs = (float)ag.groups_x, gys = (float)groups_y;
    const float fx0 = fminf(fmaxf(floorf((x_lo - 1.0f) / edge), 0.0f), gxs), fx1 = fminf(fmaxf(floorf((x_hi + 1.0f) / edge) + 1.0f, 0.0f), gxs);
    const float fy0 = fminf(fmaxf(floorf((y_lo - 1.0f) / edge), 0.0f), gys), fy1 = fminf(fmaxf(floorf((y_hi + 1.0f) / edge) + 1.0f, 0.0f), gys);
    if (!(fx1 > fx0) || !(fy1 > fy0)) return;  // the box is off screen
    ag.first_gx0 = (uint32_t)fx0, ag.first_gy0 = (uint32_t)fy0;
    ag.first_w = (uint32_t)(fx1 - fx0), ag.first_h = (uint32_t)(fy1 - fy0);
    if (ag.first_w == ag.groups_x && ag.first_h == groups_y) {
        ag.first_w = 0;  // covers the image: plain order
        return;
    }
    auto magic = [](uint32_t d) { return d <= 1 ? 0u : (uint32_t)(((1ull << 32) + d - 1) / d); };  // d == 1: the kernel does not divide
    ag.m_groups_x = magic(ag.groups_x), ag.m_first_w = magic(ag.first_w), ag.m_rest_w = magic(ag.groups_x - ag.first_w);
}

// A frame is as long as its longest wave.  While every wave that can be active is resident at once, a long wave shares its
// CU's gather path with up to 27 others and advances at a fraction of its lone speed; with fewer resident waves the ones that
// started first (box-first order: those under the box) finish sooner and the rest fill in behind them.  That only pays when
// (i) the frame is bound by its long waves, not by throughput -- a box covering a small multiple of the machine, not the
// whole image; (ii) a gather that misses L2 is expensive -- a marched volume larger than the Infinity Cache; smaller ones
// (256^3: 64 MB) move by +-3 % either way (profiles/r03_occupancy_rule.json: 13 views x
// 1080p/256^3, 1440p/512^3, 4K/512^3 x every cap).  What the launcher knows: the screen rectangle of the projected bounding
// box (box-first order) in waves, the machine's wave slots, the volume's bytes.  Rule: cap at 4 when the rectangle holds
// between 1x and 3.5x the slots at 7 per SIMD and the volume exceeds the last-level cache; no cap otherwise (camera
// inside, box filling the image, batches of cameras, small volumes, a box of a few tiles).  Speed only.
uint32_t occupancy_rule(const RaymarchArgs& ag) {
    if (ag.waves_per_simd >= 2 && ag.waves_per_simd <= 6) return ag.waves_per_simd;  // the caller's cap
    if (ag.waves_per_simd == 7) return 7;
    if (ag.n_cameras != 1 || ag.first_w == 0 || ag.group_shift == 0 || ag.wave_slots_per_simd_unit == 0) return 7;
    const uint64_t texels = (uint64_t)ag.rp.tex_size[0] * ag.rp.tex_size[1] * ag.rp.tex_size[2];
    const int mode = march_volume_mode(ag);
    const uint64_t volume_bytes = texels * (mode == kMarchPairs ? 8u : ((mode == kMarchIlv || ag.dist) ? 4u : 16u));
    if (ag.last_level_cache_bytes == 0 || volume_bytes <= ag.last_level_cache_bytes) return 7;
    const uint64_t rect_waves = (uint64_t)ag.first_w * ag.first_h * (4ull << (2 * ag.group_shift));  // 4 waves per 16 x 16 tile
    const uint64_t slots7 = 7ull * ag.wave_slots_per_simd_unit;
    if (rect_waves < slots7 || 2 * rect_waves > 7 * slots7) return 7;
    return 4;
}

// w waves per SIMD = w workgroups per CU: each asks for a w-th of the CU's 160 KB of LDS (less a little for rounding)
uint32_t lds_cap_for(uint32_t w) {
    uint32_t bytes = (w >= 2 && w <= 6) ? (160u * 1024u) / w - 1024u : 0u;
    if (bytes > 65536u) bytes = 65536u;  // the launch limit without an opt-in: 2 waves per SIMD
    return bytes;
}

MarchLaunch plan_march_launch(const RaymarchArgs& a, uint32_t lod_filter) {
    MarchLaunch p{a, MarchKernel{}, dim3((a.width + 15) / 16, (a.rows_out + 15) / 16, a.n_cameras)};
    if (p.grid.x == 0 || p.grid.y == 0 || p.grid.z == 0) return p;
    RaymarchArgs& ag = p.args;
    const dim3 tiles = p.grid;
    // the 1-D launch over groups of 2^shift x 2^shift tiles (padded to whole groups, a multiple of 8 of them), with the
    // box-first rectangle where one exists
    auto grouped = [&](uint32_t shift) {
        ag.group_shift = shift;
        ag.tiles_x = tiles.x;
        ag.tiles_y = tiles.y;
        ag.groups_x = (tiles.x + (1u << shift) - 1) >> shift;
        const uint32_t groups_y = (tiles.y + (1u << shift) - 1) >> shift;
        const uint32_t groups = ((ag.groups_x * groups_y + 7u) / 8u) * 8u;
        ag.first_w = 0;
        if (a.box_first && a.n_cameras == 1 && groups < 65536u) box_first_rectangle(ag, groups_y);  // 16-bit quotients
        p.grid = dim3(groups << (2 * shift), 1, a.n_cameras);
    };
#ifdef SDFV_TUNING
    if (a.tile_order) {  // 1-D launch over the tiles, in the order given; no rectangle: the caller's cap or none
        ag.group_shift = 0;
        p.grid = dim3(tiles.x * tiles.y, 1, 1);
    } else
#endif
    if (a.band_skip) {
        ag.group_shift = 0;  // interleaved bands: launch order (the tile orders below assume a contiguous range of rows)
    } else if (a.group_shift == kGroupAuto) {
        // one camera: groups of 2 x 2 tiles with the box-first order where the bounding box projects to a proper part of the
        // image, otherwise (camera inside the box, box filling the image, order switched off) groups of 4 x 4
        grouped(1);
        if (ag.first_w == 0) grouped(2);
    } else if (a.group_shift) {
        grouped(a.group_shift);
    }
    ag.lds_cap_bytes = lds_cap_for(occupancy_rule(ag));
    p.kernel = select_march_kernel(ag, lod_filter);
    return p;
}

CameraSource camera_source(uint32_t n_cameras, bool on_device, bool capturing, bool staging) {
    if (on_device) return CameraSource::kInPlace;
    return n_cameras > kInlineCameras && !capturing && staging ? CameraSource::kStaged : CameraSource::kInline;
}

bool launches_overlap(uint32_t n_cameras, uint32_t per_launch, uint64_t groups_per_launch) {
    return n_cameras > per_launch && groups_per_launch <= 40000;
}

}  // namespace sdfv
