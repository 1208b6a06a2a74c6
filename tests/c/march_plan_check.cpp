// march_plan_check.cpp -- the launch plan of the grid march (csrc/march_plan.cpp) and the kernel's workgroup-to-tile mapping
// (csrc/march_tile_order.h) held, on the CPU, to DESIGN.md 3.3 and to the rule that every tile of every image is rendered
// exactly once.  Built with march_plan.cpp by tests/test_march_plan_cpu.py; exit status 0 = every case held, else each failed
// case is printed.  The device is taken as gfx950 with 8 XCDs, 256 CUs and a 256 MB last-level cache.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <set>
#include <vector>

#include "march_plan.h"
#include "march_tile_order.h"

using namespace sdfv;

static int g_failed = 0;
#define CHECK(cond, ...)                               \
    do {                                               \
        if (!(cond)) {                                 \
            ++g_failed;                                \
            printf("FAILED %s: ", #cond);              \
            printf(__VA_ARGS__);                       \
            printf("\n");                              \
        }                                              \
    } while (0)

static const MarchPolicy kMI355X{true, 256, 8, 256ull << 20, 0, 0, 1};
static const float kSomewhere[2] = {0.0f, 0.0f};  // a volume that is "present": the plan only asks whether the pointer is null
enum { kDist = 1, kPairs = 2, kIlv = 4 };

struct Grid {
    uint32_t w, h, d;
};
struct Box {
    float lo, hi;
};
static const Grid kGrids[] = {{256, 256, 256}, {512, 512, 512}, {256, 128, 64}, {64, 63, 64}};
static const Box kBoxes[] = {{-1.0f, 1.0f}, {-1.5f, 1.5f}, {0.0f, 2.0f}, {-1e-3f, 1e-3f}};
static const Box kUnit = kBoxes[0];

// What a march of this grid is told: sdfv_render_params_default over it, then the plan's own two steps.
static RaymarchArgs args_for(Grid g, Box b, int volumes, uint32_t disable = 0, float lod = 1.0f, const MarchPolicy& policy = kMI355X) {
    sdfv_grid grid{{g.w, g.h, g.d}, {b.lo, b.lo, b.lo}, {b.hi, b.hi, b.hi}, 0, g.d};
    sdfv_render_params rp;
    sdfv_render_params_default(&rp, &grid);
    rp.lod_dist_between_samples = lod;
    RaymarchArgs a;
    derive_raymarch_args(&rp, disable, a);
    apply_march_policy(a, policy, 1);
    a.dist = volumes & kDist ? kSomewhere : nullptr;
    a.pairs = volumes & kPairs ? kSomewhere : nullptr;
    a.ilv = volumes & kIlv ? kSomewhere : nullptr;
    return a;
}

static bool is(const MarchKernel& k, int mode, bool linear, int xf, bool symm, bool loop) {
    return k.mode == mode && k.linear == linear && k.xf == xf && k.symm == symm && k.hand_written_loop == loop;
}
#define KFMT "(mode %d, linear %d, xf %d, symm %d, loop %d)"
#define KARGS(k) (k).mode, (int)(k).linear, (k).xf, (int)(k).symm, (int)(k).hand_written_loop

static void check_selection() {
    const Grid g256 = kGrids[0], g512 = kGrids[1], slabby = kGrids[2], odd_h = kGrids[3];
    MarchKernel k = select_march_kernel(args_for(g256, kUnit, kIlv), 0);
    CHECK(is(k, kMarchIlv, true, 2, true, true), "256^3, ilv only: " KFMT, KARGS(k));
    k = select_march_kernel(args_for(g256, kUnit, kPairs | kIlv), 0);
    CHECK(is(k, kMarchPairs, true, 2, true, true), "256^3, pairs and ilv (128 MB <= cache): " KFMT, KARGS(k));
    k = select_march_kernel(args_for(g512, kUnit, kPairs | kIlv), 0);
    CHECK(is(k, kMarchIlv, true, 2, true, true), "512^3, pairs and ilv: " KFMT, KARGS(k));
    k = select_march_kernel(args_for(slabby, kUnit, kDist | kPairs | kIlv), 0);
    CHECK(is(k, kMarchDist, true, 2, true, true), "256x128x64, all volumes: " KFMT, KARGS(k));
    k = select_march_kernel(args_for(slabby, kUnit, kIlv), 0);
    CHECK(is(k, kMarchIlv, true, 2, true, true), "256x128x64, ilv without dist: " KFMT, KARGS(k));
    k = select_march_kernel(args_for(odd_h, kUnit, kIlv), 0);
    CHECK(is(k, kMarchTex0, true, 2, true, true), "64x63x64, ilv only (H is odd): " KFMT, KARGS(k));
    for (int volumes = 0; volumes < 8; ++volumes) {
        k = select_march_kernel(args_for(g256, kBoxes[1], volumes), 0);
        CHECK(is(k, volumes & kDist ? kMarchDist : kMarchTex0, true, 0, false, false), "box +-1.5, volumes %d: " KFMT, volumes, KARGS(k));
        k = select_march_kernel(args_for(g256, kBoxes[2], volumes), 0);
        CHECK(k.linear && k.xf == 2 && !k.symm && !k.hand_written_loop, "box [0, 2], volumes %d: " KFMT, volumes, KARGS(k));
        MarchPolicy other = kMI355X;
        other.gfx950 = false;
        const MarchKernel off[2] = {select_march_kernel(args_for(g256, kUnit, volumes, 0, 1.0f, other), 0),
                                    select_march_kernel(args_for(g256, kUnit, volumes, SDFV_RM_NO_ASM_LOOP), 0)};
        for (const MarchKernel& o : off)
            CHECK(!o.hand_written_loop && o.mode != kMarchPairs && o.mode != kMarchIlv, "no gfx950 / NO_ASM_LOOP, volumes %d: " KFMT, volumes, KARGS(o));
    }
    k = select_march_kernel(args_for(g256, kUnit, kDist, 0, 2.0f), 0);
    CHECK(is(k, kMarchGeneral, false, 1, false, false), "lod 2, filter 0: " KFMT, KARGS(k));
    k = select_march_kernel(args_for(g256, kUnit, kDist, 0, 2.0f), 1);
    CHECK(is(k, kMarchLattice, false, 1, false, false), "lod 2, filter 1: " KFMT, KARGS(k));
    k = select_march_kernel(args_for(g256, kBoxes[1], kDist, 0, 2.0f), 1);
    CHECK(is(k, kMarchLattice, false, 0, false, false), "lod 2, filter 1, box +-1.5: " KFMT, KARGS(k));
    k = select_march_kernel(args_for(g256, kBoxes[3], kDist | kPairs | kIlv), 0);
    CHECK(k.mode == kMarchGeneral && k.linear, "box +-1e-3 at 256^3 (fast_index fails): " KFMT, KARGS(k));
    k = select_march_kernel(args_for(g256, kUnit, kDist | kPairs | kIlv, SDFV_RM_NO_FAST_INDEX), 0);
    CHECK(is(k, kMarchGeneral, true, 1, false, false), "SDFV_RM_NO_FAST_INDEX: " KFMT, KARGS(k));
}

// Grids x boxes x volume subsets x single disable bits x lod x filter: every selection is instantiated, every instantiated
// variant is selected, and the advice names the volume the selection marches when all three are there.
static void check_sweep() {
    std::set<int> selected;
    for (Grid g : kGrids)
        for (Box b : kBoxes) {
            for (int volumes = 0; volumes < 8; ++volumes)
                for (int bit = -1; bit < 8; ++bit)
                    for (float lod : {1.0f, 2.0f})
                        for (uint32_t filter : {0u, 1u}) {
                            const uint32_t disable = bit < 0 ? 0u : 1u << bit;
                            const MarchKernel k = select_march_kernel(args_for(g, b, volumes, disable, lod), filter);
                            CHECK(march_variant_instantiated(k), "%ux%ux%u box [%g, %g] volumes %d disable %u lod %g filter %u selects " KFMT, g.w,
                                  g.h, g.d, b.lo, b.hi, volumes, disable, lod, filter, KARGS(k));
                            selected.insert(variant_key(k.mode, k.linear, k.xf, k.symm, k.hand_written_loop));
                        }
            const int advice = march_volume_choice(args_for(g, b, 0), true, true, true);
            const MarchKernel k = select_march_kernel(args_for(g, b, kDist | kPairs | kIlv), 0);
            const int marched = k.mode == kMarchPairs || k.mode == kMarchIlv ? k.mode : 0;
            CHECK(advice == marched, "%ux%ux%u box [%g, %g]: advice %d, the selection marches %d", g.w, g.h, g.d, b.lo, b.hi, advice, marched);
        }
#define SDFV_VARIANT(MODE, LINEAR, XF, SYMM, ASM) \
    CHECK(selected.count(variant_key(MODE, LINEAR, XF, SYMM, ASM)) == 1, "no member of the sweep selects (%s, %s, %d, %s, %s)", #MODE, #LINEAR, XF, #SYMM, #ASM);
    SDFV_MARCH_VARIANTS(SDFV_VARIANT)
#undef SDFV_VARIANT
}

// ---- tile order ---------------------------------------------------------------------------------------------------------
// The arguments of a grouped launch with this rectangle, set as plan_march_launch's grouped() and box_first_rectangle's tail do.
static RaymarchArgs grouped_args(uint32_t shift, uint32_t tiles_x, uint32_t tiles_y, uint32_t gx0, uint32_t gy0, uint32_t w, uint32_t h,
                                 uint32_t& grid_x) {
    RaymarchArgs a;
    memset(&a, 0, sizeof(a));
    a.group_shift = shift;
    a.tiles_x = tiles_x;
    a.tiles_y = tiles_y;
    a.groups_x = (tiles_x + (1u << shift) - 1) >> shift;
    const uint32_t groups_y = (tiles_y + (1u << shift) - 1) >> shift;
    grid_x = (((a.groups_x * groups_y + 7u) / 8u) * 8u) << (2 * shift);
    a.first_gx0 = gx0, a.first_gy0 = gy0, a.first_w = w, a.first_h = h;
    if (w == a.groups_x && h == groups_y) a.first_w = 0;  // covers the image: plain order
    auto magic = [](uint32_t d) { return d <= 1 ? 0u : (uint32_t)(((1ull << 32) + d - 1) / d); };
    if (a.first_w) a.m_groups_x = magic(a.groups_x), a.m_first_w = magic(a.first_w), a.m_rest_w = magic(a.groups_x - a.first_w);
    return a;
}

// Over the workgroups of the launch: every tile exactly once, every other workgroup padding, the rectangle's groups first.
static void check_tiles_once(const RaymarchArgs& a, uint32_t grid_x, const char* what) {
    std::vector<uint32_t> seen((size_t)a.tiles_x * a.tiles_y, 0);
    const uint32_t g = a.group_shift, n_in = a.first_w * a.first_h;
    uint32_t rendered = 0, bad = 0;
    for (uint32_t L = 0; L < grid_x; ++L) {
        uint32_t bx, by;
        const bool renders = march_tile_of(a, L, 0, 0, grid_x, bx, by);
        const bool inside = bx < a.tiles_x && by < a.tiles_y;
        if (renders != inside) ++bad;
        if (renders && inside) ++seen[(size_t)by * a.tiles_x + bx], ++rendered;
        if (a.first_w) {
            const uint32_t G = ((L >> 3) >> (2 * g)) * 8u + (L & 7u), gx = bx >> g, gy = by >> g;
            const bool in_rect = gx >= a.first_gx0 && gx < a.first_gx0 + a.first_w && gy >= a.first_gy0 && gy < a.first_gy0 + a.first_h;
            if (in_rect != (G < n_in)) ++bad;
        }
    }
    uint32_t not_once = 0;
    for (uint32_t c : seen) not_once += c != 1;
    CHECK(bad == 0 && not_once == 0 && rendered == a.tiles_x * a.tiles_y,
          "%s: shift %u, %ux%u tiles, rectangle (%u, %u) %ux%u: %u tiles not rendered exactly once, %u workgroups misreported", what, g,
          a.tiles_x, a.tiles_y, a.first_gx0, a.first_gy0, a.first_w, a.first_h, not_once, bad);
}

static void check_tile_order() {
    const uint32_t counts[][2] = {{1, 1}, {2, 3}, {7, 5}, {8, 8}, {9, 17}, {120, 68}, {160, 90}, {240, 135}};
    for (uint32_t shift : {1u, 2u})
        for (const auto& c : counts) {
            const uint32_t tx = c[0], ty = c[1], gxs = (tx + (1u << shift) - 1) >> shift, gys = (ty + (1u << shift) - 1) >> shift;
            uint32_t grid_x;
            auto with = [&](uint32_t gx0, uint32_t gy0, uint32_t w, uint32_t h, const char* what) {
                if (w == 0 || h == 0 || gx0 + w > gxs || gy0 + h > gys) return;  // no such rectangle in an image this small
                const RaymarchArgs a = grouped_args(shift, tx, ty, gx0, gy0, w, h, grid_x);
                if (w == gxs && h == gys) CHECK(a.first_w == 0, "%s: the whole image must switch the order off", what);
                check_tiles_once(a, grid_x, what);
            };
            const RaymarchArgs plain = grouped_args(shift, tx, ty, 0, 0, 0, 0, grid_x);
            check_tiles_once(plain, grid_x, "plain order");
            if (tx * ty <= 9 * 17) {
                for (uint32_t gy0 = 0; gy0 < gys; ++gy0)
                    for (uint32_t gx0 = 0; gx0 < gxs; ++gx0)
                        for (uint32_t h = 1; gy0 + h <= gys; ++h)
                            for (uint32_t w = 1; gx0 + w <= gxs; ++w) with(gx0, gy0, w, h, "every rectangle");
                continue;
            }
            const uint32_t w = gxs / 3, h = gys / 3;
            with(0, 0, w, h, "corner"), with(gxs - w, 0, w, h, "corner"), with(0, gys - h, w, h, "corner"), with(gxs - w, gys - h, w, h, "corner");
            with(gxs / 3, 0, w, h, "edge"), with(gxs / 3, gys - h, w, h, "edge"), with(0, gys / 3, w, h, "edge"), with(gxs - w, gys / 3, w, h, "edge");
            with((gxs - w) / 2, (gys - h) / 2, w, h, "centred");
            with(gxs / 2, gys / 2, 1, h, "first_w == 1");
            with(0, gys / 2, gxs - 1, h, "groups_x - first_w == 1"), with(1, gys / 2, gxs - 1, h, "groups_x - first_w == 1");
            with(gxs / 2, 0, w, gys, "first_gy0 == 0"), with(0, 0, gxs, h, "first_gy0 == 0");
            with(0, 0, gxs, gys, "whole image");
        }
    // launch order with rotated columns: each row of each camera is a permutation of its tile columns
    RaymarchArgs a;
    memset(&a, 0, sizeof(a));
    a.rotate_columns = 1;
    for (const auto& c : counts)
        for (uint32_t cam = 0; cam < 3; ++cam)
            for (uint32_t wy = 0; wy < c[1]; ++wy) {
                std::vector<uint32_t> seen(c[0], 0);
                bool ok = true;
                for (uint32_t wx = 0; wx < c[0]; ++wx) {
                    uint32_t bx, by;
                    ok = march_tile_of(a, wx, wy, cam, c[0], bx, by) && by == wy && bx < c[0] && ok;
                    if (bx < c[0]) ++seen[bx];
                }
                for (uint32_t n : seen) ok = ok && n == 1;
                CHECK(ok, "rotate_columns: %ux%u tiles, camera %u, row %u is no permutation of its columns", c[0], c[1], cam, wy);
            }
}

// ---- rectangle, occupancy, LDS cap ------------------------------------------------------------------------------------------
// The textbook right-handed look-at (f = normalize(target - eye), s = normalize(f x up), u = s x f).
static sdfv_camera look_at(const double eye[3], const double target[3], double fovy_degrees, double aspect) {
    const double up[3] = {0.0, 1.0, 0.0};
    double f[3] = {target[0] - eye[0], target[1] - eye[1], target[2] - eye[2]};
    const double fl = sqrt(f[0] * f[0] + f[1] * f[1] + f[2] * f[2]);
    for (double& c : f) c /= fl;
    double s[3] = {f[1] * up[2] - f[2] * up[1], f[2] * up[0] - f[0] * up[2], f[0] * up[1] - f[1] * up[0]};
    const double sl = sqrt(s[0] * s[0] + s[1] * s[1] + s[2] * s[2]);
    for (double& c : s) c /= sl;
    const double u[3] = {s[1] * f[2] - s[2] * f[1], s[2] * f[0] - s[0] * f[2], s[0] * f[1] - s[1] * f[0]};
    sdfv_camera cam;
    memset(&cam, 0, sizeof(cam));
    for (int i = 0; i < 3; ++i) cam.eye[i] = (float)eye[i], cam.right[i] = (float)s[i], cam.up[i] = (float)u[i], cam.forward[i] = (float)f[i];
    cam.tan_half_fovy = (float)tan(fovy_degrees * (3.14159265358979323846 / 180.0) / 2.0);
    cam.aspect = (float)aspect;
    return cam;
}

static RaymarchArgs frame_args(Grid g, int volumes, const sdfv_camera& cam, uint32_t width, uint32_t height) {
    RaymarchArgs a = args_for(g, kUnit, volumes);
    a.width = width, a.height = height, a.y0 = 0, a.y1 = height, a.rows_out = height, a.band_shift = 4;
    a.n_cameras = 1;
    a.cameras[0] = cam;
    return a;
}

static void check_rectangle() {
    const double origin[3] = {0.0, 0.0, 0.0}, eye0[3] = {2.5, 3.0, 5.0}, near_z[3] = {0.0, 0.0, 1.5}, plus_x[3] = {5.0, 0.0, 1.5};
    const uint32_t width = 1920, height = 1080;
    const double aspect = (double)width / height;
    MarchLaunch p = plan_march_launch(frame_args(kGrids[0], kDist, look_at(origin, eye0, 45.0, aspect), width, height), 0);
    CHECK(p.args.first_w == 0 && p.args.group_shift == 2, "a camera inside the box: first_w %u, group_shift %u", p.args.first_w, p.args.group_shift);
    p = plan_march_launch(frame_args(kGrids[0], kDist, look_at(near_z, plus_x, 45.0, aspect), width, height), 0);
    CHECK(p.args.first_w == 0 && p.args.group_shift == 2, "a corner behind the camera: first_w %u, group_shift %u", p.args.first_w, p.args.group_shift);

    // the default view: the rectangle holds the projection of every corner, here in float64 through the same pinhole model
    const sdfv_camera cam = look_at(eye0, origin, 45.0, aspect);
    p = plan_march_launch(frame_args(kGrids[0], kDist, cam, width, height), 0);
    const RaymarchArgs& a = p.args;
    CHECK(a.group_shift == 1 && a.first_w > 0 && a.tiles_x == 120 && a.tiles_y == 68 && a.groups_x == 60 && p.grid.x == 2040u * 4u && p.grid.y == 1 &&
              p.grid.z == 1,
          "default view at 1080p: shift %u, first_w %u, %ux%u tiles, groups_x %u, grid %u", a.group_shift, a.first_w, a.tiles_x, a.tiles_y, a.groups_x,
          p.grid.x);
    for (int c = 0; c < 8; ++c) {
        const double corner[3] = {c & 1 ? 1.0 : -1.0, c & 2 ? 1.0 : -1.0, c & 4 ? 1.0 : -1.0};
        double v[3], zc = 0.0, xc = 0.0, yc = 0.0;
        for (int i = 0; i < 3; ++i) v[i] = corner[i] - (double)cam.eye[i];
        for (int i = 0; i < 3; ++i) zc += v[i] * cam.forward[i], xc += v[i] * cam.right[i], yc += v[i] * cam.up[i];
        const double px = (xc / (zc * cam.aspect * cam.tan_half_fovy) + 1.0) * 0.5 * width;
        const double py = (1.0 - yc / (zc * cam.tan_half_fovy)) * 0.5 * height;
        const double gx = floor(px / 32.0), gy = floor(py / 32.0);  // groups of 2 x 2 tiles of 16 x 16 pixels
        CHECK(gx >= a.first_gx0 && gx < a.first_gx0 + a.first_w && gy >= a.first_gy0 && gy < a.first_gy0 + a.first_h,
              "corner %d projects to pixel (%.2f, %.2f) = group (%g, %g), outside the rectangle (%u, %u) %ux%u", c, px, py, gx, gy, a.first_gx0,
              a.first_gy0, a.first_w, a.first_h);
    }
    check_tiles_once(a, p.grid.x, "the plan of the default view");
    CHECK(march_variant_instantiated(p.kernel) && p.kernel.mode == kMarchDist && p.kernel.hand_written_loop, "default view: " KFMT, KARGS(p.kernel));
    RaymarchArgs none = frame_args(kGrids[0], kDist, cam, 0, height);
    CHECK(plan_march_launch(none, 0).grid.x == 0, "an image without columns has nothing to launch");
}

static void check_occupancy() {
    const double origin[3] = {0.0, 0.0, 0.0}, eye0[3] = {2.5, 3.0, 5.0};
    const sdfv_camera cam = look_at(eye0, origin, 45.0, 16.0 / 9.0);
    // a 512^3 march over tex0 (2 GB), groups of 2 x 2 tiles: 16 waves per group, 7 x 1024 = 7 168 slots at 7 per SIMD
    auto capped = [&](uint32_t w, uint32_t h) {
        RaymarchArgs a = frame_args(kGrids[1], 0, cam, 3840, 2160);
        a.group_shift = 1, a.first_w = w, a.first_h = h;
        return a;
    };
    CHECK(occupancy_rule(capped(28, 16)) == 4, "448 groups = 1x the slots");
    CHECK(occupancy_rule(capped(149, 3)) == 7, "447 groups: just below 1x");
    CHECK(occupancy_rule(capped(49, 32)) == 4, "1568 groups = 3.5x the slots");
    CHECK(occupancy_rule(capped(523, 3)) == 7, "1569 groups: just above 3.5x");
    for (uint32_t w = 2; w <= 7; ++w) {
        RaymarchArgs a = capped(149, 3);  // where the rule itself says 7
        a.waves_per_simd = w;
        CHECK(occupancy_rule(a) == w, "the caller's cap %u", w);
        a = capped(28, 16);  // ... and where it says 4
        a.waves_per_simd = w;
        CHECK(occupancy_rule(a) == w, "the caller's cap %u", w);
    }
    RaymarchArgs a = capped(28, 16);
    a.n_cameras = 2;
    CHECK(occupancy_rule(a) == 7, "two cameras: no cap");
    a = capped(28, 16);
    a.rp.tex_size[0] = a.rp.tex_size[1] = a.rp.tex_size[2] = 256;  // 16 B x 256^3 = 256 MB: within the cache
    CHECK(occupancy_rule(a) == 7, "a volume within the cache: no cap");
    a = capped(28, 16);
    a.dist = kSomewhere;  // 4 B x 512^3 = 512 MB: still beyond it
    CHECK(occupancy_rule(a) == 4, "512^3 over the distance volume");
    CHECK(lds_cap_for(4) == 39936 && lds_cap_for(2) == 65536 && lds_cap_for(7) == 0, "lds_cap_for: %u %u %u", lds_cap_for(4), lds_cap_for(2), lds_cap_for(7));
}

static void check_batching() {
    CHECK(cameras_per_launch(camera_source(64, false, false, true)) == 64 && camera_source(64, false, false, true) == CameraSource::kStaged,
          "64 host cameras, not capturing, staging on");
    CHECK(cameras_per_launch(camera_source(64, false, true, true)) == 16, "64 host cameras while capturing");
    CHECK(cameras_per_launch(camera_source(64, false, false, false)) == 16, "64 host cameras with staging off");
    CHECK(cameras_per_launch(camera_source(5, true, false, true)) == 64 && camera_source(5, true, false, true) == CameraSource::kInPlace,
          "a device array of 5 is read in place");
    CHECK(camera_source(16, false, false, true) == CameraSource::kInline, "16 host cameras ride in the argument block");
    CHECK(launches_overlap(256, 64, 40000), "overlap at 40 000 groups per launch");
    CHECK(!launches_overlap(256, 64, 40001), "no overlap at 40 001 groups per launch");
    CHECK(!launches_overlap(64, 64, 100), "a batch that is one launch does not overlap");
}

int main() {
    check_selection();
    check_sweep();
    check_tile_order();
    check_rectangle();
    check_occupancy();
    check_batching();
    if (g_failed) printf("%d case(s) failed\n", g_failed);
    else printf("ok\n");
    return g_failed ? 1 : 0;
}
