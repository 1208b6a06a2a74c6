// march_tile_order.h -- which 16 x 16 tile of the image a workgroup of raymarch_kernel renders: the kernel's half of the
// bijection whose other half is the launch plan (march_plan.cpp: grouped(), box_first_rectangle).  The same text for the
// device and for the host, so that a CPU test can walk every workgroup of a launch and see every tile rendered exactly once.
#pragma once

#include "raymarch_kernels.h"

namespace sdfv {

// n / d by m = ceil(2^32 / d) (the plan's m_*): exact for n, d < 2^16, which the plan guarantees (fewer than 65 536 groups).
__host__ __device__ __forceinline__ uint32_t tile_order_div(uint32_t n, uint32_t d, uint32_t m) {
#if defined(__HIP_DEVICE_COMPILE__)
    return d == 1 ? n : __umulhi(n, m);
#else
    return d == 1 ? n : (uint32_t)(((uint64_t)n * m) >> 32);
#endif
}

// Launch order (batches of cameras, tile bands; group_shift == 0 and rotate_columns): the tile column of workgroup (wx, wy, wz)
// in a grid of tiles_x columns.  The workgroups of a launch are dealt to the eight XCDs round robin by
// their linear number and every XCD works through ITS share at its own pace: the launch is as long as the busiest
// XCD's share.  With a tile row a multiple of 8 wide (1080p: 120, 4K: 240, 1440p: 160) XCD k would render tile columns
// k, k + 8, ... of EVERY row of EVERY camera -- and an object 44 columns wide gives six columns to some XCDs and five
// to others: 24 % more marching on the busiest XCD than on the idlest (profiles/r04_batch_timeline_*.json, EXPERIMENTS R4.12: they finish 290 us
// apart in a 1.75 ms batch).  Rotating the columns by row and camera deals every XCD every column in turn.
__host__ __device__ __forceinline__ uint32_t rotated_tile_column(uint32_t wx, uint32_t wy, uint32_t wz, uint32_t tiles_x) {
    const uint32_t r = (wy + wz) % tiles_x;  // scalar
    uint32_t bx = wx + r;
    if (bx >= tiles_x) bx -= tiles_x;
    return bx;
}

// XCD-aware order (a.group_shift = g > 0): the launch is 1-D over workgroups; workgroup L runs on XCD L % 8 (observed
// placement, used for speed only).  The image is cut into groups of 2^g x 2^g tiles; group number G goes to XCD
// G % 8, so that the tiles one XCD's L2 serves are compact patches spread evenly over the image.  The tile of workgroup L;
// one outside tiles_x x tiles_y is padding of the last groups.
__host__ __device__ __forceinline__ void grouped_tile(const RaymarchArgs& a, uint32_t L, uint32_t& bx, uint32_t& by) {
    const uint32_t g = a.group_shift, per = 1u << (2 * g);
    const uint32_t xcd = L & 7u, k = L >> 3;
    const uint32_t G = (k >> (2 * g)) * 8u + xcd, t = k & (per - 1u);
    uint32_t gx, gy;
    if (a.first_w == 0) {
        gx = G % a.groups_x;
        gy = G / a.groups_x;
    } else {
        // box-first: the groups under the projected bounding box start first -- the frame is as long as its longest
        // wave, and those are all there; the groups that only see background fill in behind them
        const uint32_t n_in = a.first_w * a.first_h, top = a.first_gy0 * a.groups_x, rest_w = a.groups_x - a.first_w;
        uint32_t j = G - n_in;
        if (G < n_in) {
            const uint32_t r = tile_order_div(G, a.first_w, a.m_first_w);
            gx = a.first_gx0 + (G - r * a.first_w);
            gy = a.first_gy0 + r;
        } else if (j < top) {
            gy = tile_order_div(j, a.groups_x, a.m_groups_x);
            gx = j - gy * a.groups_x;
        } else if ((j -= top) < a.first_h * rest_w) {
            const uint32_t r = tile_order_div(j, rest_w, a.m_rest_w), c = j - r * rest_w;
            gy = a.first_gy0 + r;
            gx = c < a.first_gx0 ? c : c + a.first_w;
        } else {
            j -= a.first_h * rest_w;
            const uint32_t r = tile_order_div(j, a.groups_x, a.m_groups_x);
            gy = a.first_gy0 + a.first_h + r;
            gx = j - r * a.groups_x;
        }
    }
    bx = (gx << g) + (t & ((1u << g) - 1u));
    by = (gy << g) + (t >> g);
}

// Workgroup (wx, wy, wz) = blockIdx of a launch whose grid is grid_x wide -> tile (bx, by); false: padding, nothing to render.
// raymarch_kernel spells these three lines out around its own `return` (a padding flag handed back through a function
// changes the layout of its scalar branches, which the kernel-by-kernel comparison of a refactor forbids): keep them alike.
__host__ __device__ __forceinline__ bool march_tile_of(const RaymarchArgs& a, uint32_t wx, uint32_t wy, uint32_t wz, uint32_t grid_x,
                                                       uint32_t& bx, uint32_t& by) {
    bx = wx, by = wy;
    if (a.group_shift == 0 && a.rotate_columns) bx = rotated_tile_column(wx, wy, wz, grid_x);
    else if (a.group_shift) grouped_tile(a, wx, bx, by);
    return !(a.group_shift && (bx >= a.tiles_x || by >= a.tiles_y));
}

}  // namespace sdfv
