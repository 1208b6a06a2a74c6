// march_loops.h -- sdfRaycast's loop as hipcc compiles it: the fast march over tex0.r or the compact distance volume
// (march_fast) and the lattice filter of a loading grid (march_lattice).  The same loop written by hand is march_asm_loop.h;
// the shader's nested loop for every other case stands in raymarch_kernel itself.  Device text only.
#pragma once

#include "march_sampler.h"

namespace sdfv {
namespace {

// sdfRaycast's loop (material.frag:97-126) for the LINEAR filter, with everything the loop does not need
// taken out of it.  Per iteration and lane: out-of-bounds test, texel coordinates, (re)fetch, trilinear
// mix, hit test, advance.
//  * Predicated straight-line code with ONE branch (the re-fetch): lanes that stopped no longer commit
//    results, so the wave does not pay exec-mask bookkeeping for the shader's nested if/else.
//  * One-cell register cache: sphere tracing takes its smallest steps exactly on the longest rays
//    (grazing a surface), so consecutive samples usually fall in the same texel cell; the 8 corner values
//    live in registers and are re-fetched only when floor(u,v,w) changes.
//  * MirroredRepeat needs no modulo: a marching ray is within 1e-4 of the box, hence (the launcher checks
//    1e-4 * N / size <= 0.25 per axis before selecting this kernel) floor(u) is in [-1, N-1], where
//    mirror(i) == clamp(i, 0, N-1).
//  * XF == 2: extents AND texture sizes are powers of two, so ((p-min)*inv)*N == (p-min)*(inv*N) exactly.
//  * No per-iteration status/step counters: a stopped lane's ray_pos no longer moves, so afterwards
//    "out of bounds" is re-derived from it (oob(ray_pos) > 1e-4 <=> it stopped on that test), and the
//    step count is 1 + the last iteration the lane sampled in.
//  * kMarchTex0 (STRIDE 4) reads tex0.r in place, kMarchDist (STRIDE 1) the compact distance volume (sdfv_commit_distance), where
//    x-neighbours are adjacent floats and each (y, z) pair of corners is ONE 8-byte load.
//  * T: accumulate distanceFromOrigin (only the aux record consumes it).
// Values and operation order are exactly those of sample_r() / the oracle; only redundant work is skipped.
template <int MODE, int XF, bool SYMM, bool T>
__device__ __forceinline__ void march_fast(const RaymarchArgs& a, const Tex& t, V3 ray_dir, bool covered, V3& ray_pos,
                                           float& dist_from_origin, int& status, int& steps, int& iterations) {
    static_assert(MODE == kMarchTex0 || MODE == kMarchDist, "the pair and interleaved volumes are read by the hand-written loop only");
    constexpr int STRIDE = MODE == kMarchTex0 ? 4 : 1;
    const float* __restrict__ vol = march_volume<MODE>(a);
    const float fw_ = (float)t.w, fh_ = (float)t.h, fd_ = (float)t.d;
    const float kx = a.inv_bsize[0] * fw_, ky = a.inv_bsize[1] * fh_, kz = a.inv_bsize[2] * fd_;  // exact if XF == 2
    const int wm1 = t.w - 1, hm1 = t.h - 1, dm1 = t.d - 1;
    const uint32_t sy = (uint32_t)t.w, sz = (uint32_t)t.w * (uint32_t)t.h;
    bool marching = covered;
    int last_i = -1;
    float cfu = -4.0f, cfv = -4.0f, cfw = -4.0f;  // never a valid floor(u) of a marching lane
    float t000 = 0.0f, t100 = 0.0f, t010 = 0.0f, t110 = 0.0f, t001 = 0.0f, t101 = 0.0f, t011 = 0.0f, t111 = 0.0f;
    for (int i = 0; i < 255; ++i) {
        // Stop condition: out of bounds (material.frag:106-109)
        marching = marching && !(oob_dist<SYMM>(a, ray_pos) > 1e-4f);
        if (__ballot(marching) == 0ull) break;  // wave-level early termination
        ++iterations;
        last_i = marching ? i : last_i;
        float u, v, w;
        if (XF == 2) {
            u = (ray_pos.x - a.rp.bounds_min[0]) * kx - 0.5f;
            v = (ray_pos.y - a.rp.bounds_min[1]) * ky - 0.5f;
            w = (ray_pos.z - a.rp.bounds_min[2]) * kz - 0.5f;
        } else {
            const V3 q = to_p01<XF>(a, ray_pos);
            u = q.x * fw_ - 0.5f; v = q.y * fh_ - 0.5f; w = q.z * fd_ - 0.5f;
        }
        const float fu = floorf(u), fv = floorf(v), fw = floorf(w);
        const float ax = u - fu, ay = v - fv, az = w - fw;
        if (marching && (fu != cfu || fv != cfv || fw != cfw)) {
            cfu = fu; cfv = fv; cfw = fw;
            const int i0 = (int)fu, j0 = (int)fv, k0 = (int)fw;
            const uint32_t i0c = (uint32_t)max(i0, 0), i1c = (uint32_t)min(i0 + 1, wm1);
            const uint32_t j0c = (uint32_t)max(j0, 0) * sy, j1c = (uint32_t)min(j0 + 1, hm1) * sy;
            const uint32_t k0c = (uint32_t)max(k0, 0) * sz, k1c = (uint32_t)min(k0 + 1, dm1) * sz;
            const uint32_t r00 = k0c + j0c, r10 = k0c + j1c, r01 = k1c + j0c, r11 = k1c + j1c;
            if (STRIDE == 1 && wm1 >= 1) {
                // x-neighbours are adjacent floats in the distance volume: one 8-byte load per (y, z) pair.
                // b = clamp(i0, 0, W-2) makes {b, b+1} cover {i0c, i1c} also where the clamp folds them together.
                const uint32_t b = (uint32_t)min(max(i0, 0), wm1 - 1);
                const bool lo_is_x = i0c == b, hi_is_y = i1c == b + 1;
                typedef float f2 __attribute__((ext_vector_type(2), aligned(4)));
                const f2 q00 = *reinterpret_cast<const f2*>(vol + (uint64_t)(r00 + b));
                const f2 q10 = *reinterpret_cast<const f2*>(vol + (uint64_t)(r10 + b));
                const f2 q01 = *reinterpret_cast<const f2*>(vol + (uint64_t)(r01 + b));
                const f2 q11 = *reinterpret_cast<const f2*>(vol + (uint64_t)(r11 + b));
                t000 = lo_is_x ? q00.x : q00.y; t100 = hi_is_y ? q00.y : q00.x;
                t010 = lo_is_x ? q10.x : q10.y; t110 = hi_is_y ? q10.y : q10.x;
                t001 = lo_is_x ? q01.x : q01.y; t101 = hi_is_y ? q01.y : q01.x;
                t011 = lo_is_x ? q11.x : q11.y; t111 = hi_is_y ? q11.y : q11.x;
            } else {
                t000 = vol[(uint64_t)(r00 + i0c) * STRIDE]; t100 = vol[(uint64_t)(r00 + i1c) * STRIDE];
                t010 = vol[(uint64_t)(r10 + i0c) * STRIDE]; t110 = vol[(uint64_t)(r10 + i1c) * STRIDE];
                t001 = vol[(uint64_t)(r01 + i0c) * STRIDE]; t101 = vol[(uint64_t)(r01 + i1c) * STRIDE];
                t011 = vol[(uint64_t)(r11 + i0c) * STRIDE]; t111 = vol[(uint64_t)(r11 + i1c) * STRIDE];
            }
        }
        const float sample_dist = trilerp(t000, t100, t010, t110, t001, t101, t011, t111, ax, ay, az) - 1e-1f;
        // Stop condition: actually hit the surface (material.frag:117-121)
        marching = marching && !(sample_dist < 1e-5f);
        // Move the ray forward by the minimum distance to the surface (material.frag:124-125)
        const V3 np = madd(ray_pos, ray_dir, sample_dist);
        ray_pos.x = marching ? np.x : ray_pos.x;
        ray_pos.y = marching ? np.y : ray_pos.y;
        ray_pos.z = marching ? np.z : ray_pos.z;
        if (T) {
            const float nt = dist_from_origin + sample_dist;
            dist_from_origin = marching ? nt : dist_from_origin;
        }
    }
    steps = last_i + 1;
    if (covered) status = marching ? -1 : (oob_dist<SYMM>(a, ray_pos) > 1e-4f ? -2 : 1);
}

// ---- the lattice filter: trilinear over the points a loading grid already holds (SDFV_OPT_RAYMARCH_LOD_FILTER = 1) ----------
// While a grid loads, only the texels whose three indices are multiples of L = lod_dist_between_samples (a power of two) are
// there; include/sdfgrid.h states the filter over them operation by operation.  Per axis with N texels: u = q * N - 0.5 (the
// LINEAR footprint's coordinate), s = u / L, cell floor(s), weight s - floor(s), the two texels clamp(m, 0, M - 1) * L and
// clamp(m + 1, 0, M - 1) * L with M = ceil(N / L) lattice points.  The clamp is the rule everywhere (no mirror, no condition on
// the box), so no texel off the lattice is ever read.
struct Lattice {
    uint32_t shift;     // log2(L)
    float inv_l;        // 1 / L: a power of two, so u * inv_l == u / L bit for bit
    int mx1, my1, mz1;  // M - 1 per axis
};
__device__ __forceinline__ Lattice lattice_of(const RaymarchArgs& a, const Tex& t) {
    const uint32_t l = (uint32_t)a.rp.lod_dist_between_samples;  // the API layer checked: a power of two in [2, 2^15]
    Lattice g;
    g.shift = 31u - (uint32_t)__builtin_clz(l);
    g.inv_l = 1.0f / a.rp.lod_dist_between_samples;
    g.mx1 = (int)(((uint32_t)t.w + l - 1u) >> g.shift) - 1;
    g.my1 = (int)(((uint32_t)t.h + l - 1u) >> g.shift) - 1;
    g.mz1 = (int)(((uint32_t)t.d + l - 1u) >> g.shift) - 1;
    return g;
}
// The eight texel offsets of lattice cell (floor(s) per axis = fu, fv, fw): the one place the index rule is written.
__device__ __forceinline__ void lattice_cell(const Tex& t, const Lattice& g, float fu, float fv, float fw, Footprint& f) {
    const int i0 = (int)fu, j0 = (int)fv, k0 = (int)fw;
    const uint32_t sy = (uint32_t)t.w, sz = (uint32_t)t.w * (uint32_t)t.h;
    const uint32_t i0m = (uint32_t)min(max(i0, 0), g.mx1) << g.shift, i1m = (uint32_t)min(max(i0 + 1, 0), g.mx1) << g.shift;
    const uint32_t j0m = ((uint32_t)min(max(j0, 0), g.my1) << g.shift) * sy, j1m = ((uint32_t)min(max(j0 + 1, 0), g.my1) << g.shift) * sy;
    const uint32_t k0m = ((uint32_t)min(max(k0, 0), g.mz1) << g.shift) * sz, k1m = ((uint32_t)min(max(k0 + 1, 0), g.mz1) << g.shift) * sz;
    f.o000 = k0m + j0m + i0m; f.o100 = k0m + j0m + i1m;
    f.o010 = k0m + j1m + i0m; f.o110 = k0m + j1m + i1m;
    f.o001 = k1m + j0m + i0m; f.o101 = k1m + j0m + i1m;
    f.o011 = k1m + j1m + i0m; f.o111 = k1m + j1m + i1m;
}
__device__ __forceinline__ Footprint lattice_footprint(const Tex& t, const Lattice& g, V3 p01) {
    const float u = p01.x * (float)t.w - 0.5f, v = p01.y * (float)t.h - 0.5f, w = p01.z * (float)t.d - 0.5f;
    const float su = u * g.inv_l, sv = v * g.inv_l, sw = w * g.inv_l;
    const float fu = floorf(su), fv = floorf(sv), fw = floorf(sw);
    Footprint f;
    f.ax = su - fu; f.ay = sv - fv; f.az = sw - fw;
    lattice_cell(t, g, fu, fv, fw, f);
    return f;
}

// sdfRaycast's loop for the lattice filter: march_fast's shape (predicated straight-line code, the ballot as the wave-level
// exit, status and step count derived after the loop) over tex0.r in place, with the one-cell register cache keyed on
// floor(s).  A lattice cell is L voxels wide, so a ray stays in its cell for more steps than on the loaded grid.  The cache
// starts with a NaN key: no floor(s) compares equal to it, whatever the box (there is no fast_index condition here).
template <int XF, bool SYMM, bool T>
__device__ __forceinline__ void march_lattice(const RaymarchArgs& a, const Tex& t, const Lattice& g, V3 ray_dir, bool covered, V3& ray_pos,
                                              float& dist_from_origin, int& status, int& steps, int& iterations) {
    static_assert(XF == 0 || XF == 1, "no fused scale: s = (q * N - 0.5) / L keeps the LINEAR footprint's u");
    const float* __restrict__ vol = reinterpret_cast<const float*>(a.tex0);
    const float fw_ = (float)t.w, fh_ = (float)t.h, fd_ = (float)t.d;
    bool marching = covered;
    int last_i = -1;
    float cfu = __int_as_float(0x7fc00000), cfv = cfu, cfw = cfu;
    float t000 = 0.0f, t100 = 0.0f, t010 = 0.0f, t110 = 0.0f, t001 = 0.0f, t101 = 0.0f, t011 = 0.0f, t111 = 0.0f;
    for (int i = 0; i < 255; ++i) {
        // Stop condition: out of bounds (material.frag:106-109)
        marching = marching && !(oob_dist<SYMM>(a, ray_pos) > 1e-4f);
        if (__ballot(marching) == 0ull) break;  // wave-level early termination
        ++iterations;
        last_i = marching ? i : last_i;
        const V3 q = to_p01<XF>(a, ray_pos);
        const float su = (q.x * fw_ - 0.5f) * g.inv_l, sv = (q.y * fh_ - 0.5f) * g.inv_l, sw = (q.z * fd_ - 0.5f) * g.inv_l;
        const float fu = floorf(su), fv = floorf(sv), fw = floorf(sw);
        const float ax = su - fu, ay = sv - fv, az = sw - fw;
        if (marching && (fu != cfu || fv != cfv || fw != cfw)) {
            cfu = fu; cfv = fv; cfw = fw;
            Footprint c;
            lattice_cell(t, g, fu, fv, fw, c);
            t000 = vol[(uint64_t)c.o000 * 4]; t100 = vol[(uint64_t)c.o100 * 4];
            t010 = vol[(uint64_t)c.o010 * 4]; t110 = vol[(uint64_t)c.o110 * 4];
            t001 = vol[(uint64_t)c.o001 * 4]; t101 = vol[(uint64_t)c.o101 * 4];
            t011 = vol[(uint64_t)c.o011 * 4]; t111 = vol[(uint64_t)c.o111 * 4];
        }
        const float sample_dist = trilerp(t000, t100, t010, t110, t001, t101, t011, t111, ax, ay, az) - 1e-1f;
        // Stop condition: actually hit the surface (material.frag:117-121)
        marching = marching && !(sample_dist < 1e-5f);
        // Move the ray forward by the minimum distance to the surface (material.frag:124-125)
        const V3 np = madd(ray_pos, ray_dir, sample_dist);
        ray_pos.x = marching ? np.x : ray_pos.x;
        ray_pos.y = marching ? np.y : ray_pos.y;
        ray_pos.z = marching ? np.z : ray_pos.z;
        if (T) {
            const float nt = dist_from_origin + sample_dist;
            dist_from_origin = marching ? nt : dist_from_origin;
        }
    }
    steps = last_i + 1;
    if (covered) status = marching ? -1 : (oob_dist<SYMM>(a, ray_pos) > 1e-4f ? -2 : 1);
}

}  // namespace
}  // namespace sdfv
