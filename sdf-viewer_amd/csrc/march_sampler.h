// march_sampler.h -- texture(sampler3D) restated in full fp32 for the grid march: the texel footprint of a LINEAR fetch (GL
// texel-centre convention, MirroredRepeat or the clamp that equals it, mix() along x, then y, then z), the gathers, the NEAREST
// fetch, p01, the out-of-bounds distance and the ray's bbox fragment.  Shared by the frame kernel (raymarch_kernels.hip), its
// march loops (march_loops.h, march_asm_loop.h) and the march over a z-slab (raymarch_slab_kernels.hip).  Device text only.
#pragma once

#include <hip/hip_runtime.h>

#include "march_common.h"
#include "raymarch_kernels.h"

namespace sdfv {
namespace {

using namespace march;  // V3, the ray set-up, the taps, the record and the stores: march_common.h, shared with the direct
                        // march of SDF programs (mixf, shade() and the depth formula: march_shade.h)

// GL MIRRORED_REPEAT on a texel index (general form).
__device__ __forceinline__ uint32_t mirror_index(int i, int n) {
    if (i >= 0 && i < n) return (uint32_t)i;
    int period = 2 * n;
    int m = i % period;
    if (m < 0) m += period;
    return (uint32_t)(m < n ? m : period - 1 - m);
}

struct Tex {
    const float4* data;
    int w, h, d;  // size of the WHOLE texture
    int z_lo;     // first slice that `data` holds (kClampSlab; 0 everywhere else)
};

struct Footprint {  // the 8 texel offsets and 3 weights of one LINEAR fetch
    uint32_t o000, o100, o010, o110, o001, o101, o011, o111;
    float ax, ay, az;
};

// How a LINEAR fetch turns texel indices into offsets: kMirror = GL MirroredRepeat in full; kClamp = floor(u) is known to be
// in [-1, N-1] on every axis, where MirroredRepeat == clamp; kClampSlab = clamp, z rebased to the first resident slice.
constexpr int kMirror = 0, kClamp = 1, kClampSlab = 2;

// k0c (the clamp policies): clamp(floor(w), 0, D - 1), the slice that owns the cell -- what the march over z-slabs goes by.
template <int POLICY>
__device__ __forceinline__ Footprint footprint(const Tex& t, V3 p01, int& k0c) {
    float u = p01.x * (float)t.w - 0.5f, v = p01.y * (float)t.h - 0.5f, w = p01.z * (float)t.d - 0.5f;
    float fu = floorf(u), fv = floorf(v), fw = floorf(w);
    Footprint f;
    f.ax = u - fu; f.ay = v - fv; f.az = w - fw;
    int i0 = (int)fu, j0 = (int)fv, k0 = (int)fw;
    uint32_t i0m, i1m, j0m, j1m, k0m, k1m;
    const uint32_t sy = (uint32_t)t.w, sz = (uint32_t)t.w * (uint32_t)t.h;
    k0c = 0;
    if (POLICY == kMirror) {
        i0m = mirror_index(i0, t.w); i1m = mirror_index(i0 + 1, t.w);
        j0m = mirror_index(j0, t.h) * sy; j1m = mirror_index(j0 + 1, t.h) * sy;
        k0m = mirror_index(k0, t.d) * sz; k1m = mirror_index(k0 + 1, t.d) * sz;
    } else {
        const int z0 = POLICY == kClampSlab ? t.z_lo : 0;
        i0m = (uint32_t)max(i0, 0); i1m = (uint32_t)min(i0 + 1, t.w - 1);
        j0m = (uint32_t)max(j0, 0) * sy; j1m = (uint32_t)min(j0 + 1, t.h - 1) * sy;
        k0c = min(max(k0, 0), t.d - 1);
        k0m = (uint32_t)(max(k0, 0) - z0) * sz; k1m = (uint32_t)(min(k0 + 1, t.d - 1) - z0) * sz;
    }
    f.o000 = k0m + j0m + i0m; f.o100 = k0m + j0m + i1m;
    f.o010 = k0m + j1m + i0m; f.o110 = k0m + j1m + i1m;
    f.o001 = k1m + j0m + i0m; f.o101 = k1m + j0m + i1m;
    f.o011 = k1m + j1m + i0m; f.o111 = k1m + j1m + i1m;
    return f;
}

__device__ __forceinline__ float trilerp(float t000, float t100, float t010, float t110, float t001, float t101,
                                         float t011, float t111, float ax, float ay, float az) {
    float c00 = mixf(t000, t100, ax), c10 = mixf(t010, t110, ax);
    float c01 = mixf(t001, t101, ax), c11 = mixf(t011, t111, ax);
    return mixf(mixf(c00, c10, ay), mixf(c01, c11, ay), az);
}

template <int POLICY>
__device__ __forceinline__ Footprint footprint(const Tex& t, V3 p01) {
    int k0c;
    return footprint<POLICY>(t, p01, k0c);
}

// The eight-corner gather of one component, filtered: `stride` floats per texel (4 = tex0.r in place, 1 = the compact
// distance volume).
__device__ __forceinline__ float gather_r(const float* base, uint32_t stride, const Footprint& f) {
    const float t000 = base[(uint64_t)f.o000 * stride], t100 = base[(uint64_t)f.o100 * stride];
    const float t010 = base[(uint64_t)f.o010 * stride], t110 = base[(uint64_t)f.o110 * stride];
    const float t001 = base[(uint64_t)f.o001 * stride], t101 = base[(uint64_t)f.o101 * stride];
    const float t011 = base[(uint64_t)f.o011 * stride], t111 = base[(uint64_t)f.o111 * stride];
    return trilerp(t000, t100, t010, t110, t001, t101, t011, t111, f.ax, f.ay, f.az);
}

__device__ __forceinline__ float4 gather_rgba(const float4* data, const Footprint& f) {
    const float4 t000 = data[f.o000], t100 = data[f.o100], t010 = data[f.o010], t110 = data[f.o110];
    const float4 t001 = data[f.o001], t101 = data[f.o101], t011 = data[f.o011], t111 = data[f.o111];
    float4 r;
    r.x = trilerp(t000.x, t100.x, t010.x, t110.x, t001.x, t101.x, t011.x, t111.x, f.ax, f.ay, f.az);
    r.y = trilerp(t000.y, t100.y, t010.y, t110.y, t001.y, t101.y, t011.y, t111.y, f.ax, f.ay, f.az);
    r.z = trilerp(t000.z, t100.z, t010.z, t110.z, t001.z, t101.z, t011.z, t111.z, f.ax, f.ay, f.az);
    r.w = trilerp(t000.w, t100.w, t010.w, t110.w, t001.w, t101.w, t011.w, t111.w, f.ax, f.ay, f.az);
    return r;
}

// p01 = (p - sdfBoundsMin) / (sdfBoundsMax - sdfBoundsMin), material.frag:44.  XF >= 1: every extent is an
// exact power of two (the demo's [-1,1]^3: 2.0), so dividing equals multiplying by the exact reciprocal,
// bit for bit, and three IEEE divides (~12 instructions each) leave the per-step dependency chain.
template <int XF>
__device__ __forceinline__ V3 to_p01(const RaymarchArgs& a, V3 p) {
    if (XF >= 1)
        return mk((p.x - a.rp.bounds_min[0]) * a.inv_bsize[0], (p.y - a.rp.bounds_min[1]) * a.inv_bsize[1],
                  (p.z - a.rp.bounds_min[2]) * a.inv_bsize[2]);
    return mk((p.x - a.rp.bounds_min[0]) / a.bsize[0], (p.y - a.rp.bounds_min[1]) / a.bsize[1],
              (p.z - a.rp.bounds_min[2]) / a.bsize[2]);
}

// sdfSampleRawNearest's snapped coordinate + NEAREST fetch, material.frag:27-36
__device__ __forceinline__ uint32_t nearest_offset(const RaymarchArgs& a, const Tex& t, V3 p01) {
    float rx = (float)t.w / a.rp.lod_dist_between_samples;
    float ry = (float)t.h / a.rp.lod_dist_between_samples;
    float rz = (float)t.d / a.rp.lod_dist_between_samples;
    float qx = roundf(p01.x * rx) / rx, qy = roundf(p01.y * ry) / ry, qz = roundf(p01.z * rz) / rz;
    int i = (int)floorf(qx * (float)t.w), j = (int)floorf(qy * (float)t.h), k = (int)floorf(qz * (float)t.d);
    return (mirror_index(k, t.d) * (uint32_t)t.h + mirror_index(j, t.h)) * (uint32_t)t.w + mirror_index(i, t.w);
}

// sdfSampleRawInterp(.., p).r only -- what the march and the normal need.  material.frag:42-53.  `base`, `stride`: tex0 itself
// (4 floats per texel) or, LINEAR only, the compact distance volume (1).
template <bool LINEAR, int XF, int POLICY>
__device__ __forceinline__ float sample_r(const RaymarchArgs& a, const float* __restrict__ base, uint32_t stride, const Tex& t, V3 p) {
    V3 q = to_p01<XF>(a, p);
    if (LINEAR) return gather_r(base, stride, footprint<POLICY>(t, q));
    return base[(uint64_t)nearest_offset(a, t, q) * stride];
}

template <bool LINEAR, int XF, int POLICY>
__device__ __forceinline__ float4 sample_rgba(const RaymarchArgs& a, const Tex& t, V3 p) {
    V3 q = to_p01<XF>(a, p);
    if (LINEAR) return gather_rgba(t.data, footprint<POLICY>(t, q));
    return t.data[nearest_offset(a, t, q)];
}

// sdfOutOfBoundsDist, material.frag:83-88.  SYMM: sdfBoundsMin == -sdfBoundsMax (the demo's box); then
// max(min - p, p - max) == |p| - max exactly (the larger operand is always the one equal to |p| - max),
// which is one subtraction with an abs modifier per axis instead of two subtractions and a max.
template <bool SYMM>
__device__ __forceinline__ float oob_dist(const RaymarchArgs& a, V3 p) {
    if (SYMM) {
        return fmaxf(fabsf(p.x) - a.rp.bounds_max[0],
                     fmaxf(fabsf(p.y) - a.rp.bounds_max[1], fabsf(p.z) - a.rp.bounds_max[2]));
    }
    return march::oob_dist(a.rp, p);
}

// The volume a fast march (MODE != kMarchGeneral) reads its distances from.
template <int MODE>
__device__ __forceinline__ const float* march_volume(const RaymarchArgs& a) {
    return MODE == kMarchTex0 ? reinterpret_cast<const float*>(a.tex0) : MODE == kMarchDist ? a.dist : MODE == kMarchPairs ? a.pairs : a.ilv;
}

// The bbox fragment of that ray and main()'s ray set-up (march_common.h).  Returns whether the pixel is covered by the box.
__device__ __forceinline__ bool box_fragment_ray(const RaymarchArgs& a, V3 eye, V3 d_raw, bool in_image,
                                                 V3& ray_origin, V3& ray_dir) {
    const V3 d0 = normalize(d_raw);
    float tfrag;
    const bool covered = box_slab_test(a.rp, eye, d0, in_image, tfrag);
    fragment_ray(a.rp, eye, d0, tfrag, ray_origin, ray_dir);
    return covered;
}

}  // namespace
}  // namespace sdfv
