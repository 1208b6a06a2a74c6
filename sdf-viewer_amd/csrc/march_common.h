// march_common.h -- what every march does with a pixel BEFORE and AROUND its march loop: the primary ray, the bbox fragment
// and main()'s ray set-up (which pixels are covered), sdfOutOfBoundsDist, sdfNormal's taps, the fields of the march record
// and, on the device, the tile-to-pixel mapping and the streamed stores of outColor.  march_shade.h holds what follows a hit
// (shading, depth formula, 8-bit conversion); this header holds the rest.  One text for the grid march and the sharded march
// (raymarch_kernels.hip), the direct march of SDF programs (program_march.h) and that march's host mirror: compiled by hipcc
// and by g++ like march_shade.h, every f32 step rounded on its own, in one order.  Everything is forced inline on the device.
#pragma once

#include "march_shade.h"

#if defined(__HIPCC__)
#define SDFV_MARCH_FN __device__ __forceinline__
#define SDFV_MARCH_HD __host__ __device__ __forceinline__
#else
#define SDFV_MARCH_FN inline
#define SDFV_MARCH_HD inline
#endif

namespace sdfv {
namespace march {

struct V3 {
    float x, y, z;
};
SDFV_MARCH_FN V3 mk(float x, float y, float z) { V3 r; r.x = x; r.y = y; r.z = z; return r; }
SDFV_MARCH_FN V3 sub(V3 a, V3 b) { return mk(a.x - b.x, a.y - b.y, a.z - b.z); }
SDFV_MARCH_FN V3 madd(V3 a, V3 d, float t) { return mk(a.x + d.x * t, a.y + d.y * t, a.z + d.z * t); }
SDFV_MARCH_FN float length(V3 a) { return sqrtf(a.x * a.x + a.y * a.y + a.z * a.z); }
SDFV_MARCH_FN V3 normalize(V3 a) {
    const float l = length(a);
    return mk(a.x / l, a.y / l, a.z / l);
}

// Primary ray through the centre of pixel (px, py) of the width x height image (row 0 = top), not yet normalised.
SDFV_MARCH_FN V3 pixel_ray_raw(uint32_t width, uint32_t height, const sdfv_camera& cam, uint32_t px, uint32_t py) {
    const float ndc_x = (((float)px + 0.5f) / (float)width) * 2.0f - 1.0f;
    const float ndc_y = 1.0f - (((float)py + 0.5f) / (float)height) * 2.0f;
    const float sx = ndc_x * cam.aspect * cam.tan_half_fovy;
    const float sy = ndc_y * cam.tan_half_fovy;
    return mk(cam.forward[0] + cam.right[0] * sx + cam.up[0] * sy,
              cam.forward[1] + cam.right[1] * sx + cam.up[1] * sy,
              cam.forward[2] + cam.right[2] * sx + cam.up[2] * sy);
}

// sdfOutOfBoundsDist, material.frag:83-88
SDFV_MARCH_FN float oob_dist(const sdfv_render_params& rp, V3 p) {
    const float ox = fmaxf(rp.bounds_min[0] - p.x, p.x - rp.bounds_max[0]);
    const float oy = fmaxf(rp.bounds_min[1] - p.y, p.y - rp.bounds_max[1]);
    const float oz = fmaxf(rp.bounds_min[2] - p.z, p.z - rp.bounds_max[2]);
    return fmaxf(ox, fmaxf(oy, oz));
}

// The slab test's arithmetic -- where the line eye + t * d0 enters and leaves the box [b.bounds_min, b.bounds_max]
// (sdfv_render_params, or the cast's own block): six divisions, then
// tnear = max(max(min x, min y), min z) and tfar = min(min(max x, max y), max z).  The ray cast of program_cast.h clips a
// caller's [t_min, t_max] against the two.
template <typename Box>
SDFV_MARCH_FN void box_slab_interval(const Box& b, V3 eye, V3 d0, float& tnear, float& tfar) {
    const float tx1 = (b.bounds_min[0] - eye.x) / d0.x, tx2 = (b.bounds_max[0] - eye.x) / d0.x;
    const float ty1 = (b.bounds_min[1] - eye.y) / d0.y, ty2 = (b.bounds_max[1] - eye.y) / d0.y;
    const float tz1 = (b.bounds_min[2] - eye.z) / d0.z, tz2 = (b.bounds_max[2] - eye.z) / d0.z;
    tnear = fmaxf(fmaxf(fminf(tx1, tx2), fminf(ty1, ty2)), fminf(tz1, tz2));
    tfar = fminf(fminf(fmaxf(tx1, tx2), fmaxf(ty1, ty2)), fmaxf(tz1, tz2));
}
// The bbox fragment of the ray eye + t * d0 (d0 normalised): slab test standing in for the rasterised cube
// (scene/sdf/mod.rs:254-282).  Returns whether the pixel is covered by the box; tfrag = the fragment's distance from the eye --
// the entry point when the camera is outside the box, the exit point when it is inside -- feeds fragment_ray.
SDFV_MARCH_FN bool box_slab_test(const sdfv_render_params& rp, V3 eye, V3 d0, bool in_image, float& tfrag) {
    float tnear, tfar;
    box_slab_interval(rp, eye, d0, tnear, tfar);
    tfrag = tnear > 0.0f ? tnear : tfar;
    return in_image && (tfar >= tnear && tfar > 0.0f);
}
// main()'s ray set-up, material.frag:133-139: a ray that would leave the box within 0.2 starts 0.2 in front of the eye instead.
SDFV_MARCH_FN void fragment_ray(const sdfv_render_params& rp, V3 eye, V3 d0, float tfrag, V3& ray_origin, V3& ray_dir) {
    ray_origin = madd(eye, d0, tfrag);
    ray_dir = normalize(sub(ray_origin, eye));
    if (oob_dist(rp, madd(ray_origin, ray_dir, 0.2f)) > 0.0f) ray_origin = madd(eye, ray_dir, 0.2f);
}

// sdfNormal, material.frag:73-80.  h = 1 / length(texSize / lod) (:74), unchecked: whatever the formula gives for the sizes.
SDFV_MARCH_HD float tap_distance(float w, float h, float d, float lod) {
    const float sx = w / lod, sy = h / lod, sz = d / lod;
    return 1.0f / sqrtf(sx * sx + sy * sy + sz * sz);
}
// h as a descriptor states it: normal_h when it gives one, else the grid route's for rp.tex_size, so that a caller comparing
// the two routes gets the same taps.  0 when neither is there.
SDFV_MARCH_HD float normal_tap_distance(const sdfv_render_params& rp, float normal_h) {
    if (normal_h > 0.0f) return normal_h;
    if (rp.tex_size[0] == 0 || rp.tex_size[1] == 0 || rp.tex_size[2] == 0 || !(rp.lod_dist_between_samples > 0.0f)) return 0.0f;
    return tap_distance((float)rp.tex_size[0], (float)rp.tex_size[1], (float)rp.tex_size[2], rp.lod_dist_between_samples);
}
// Tap t = 0..3 is at p + k * h with k = k.xyy, k.yyx, k.yxy, k.xxx, k = (1, -1); the normal is the taps' distances times
// their k, summed in that order, normalised.
SDFV_MARCH_FN V3 tap_sign(int t) { return mk((t == 0 || t == 3) ? 1.0f : -1.0f, t >= 2 ? 1.0f : -1.0f, (t & 1) ? 1.0f : -1.0f); }
SDFV_MARCH_FN V3 normal_tap(V3 p, float h, int t) {
    const V3 k = tap_sign(t);
    return mk(p.x + k.x * h, p.y + k.y * h, p.z + k.z * h);
}
SDFV_MARCH_FN V3 normal_of_taps(float d1, float d2, float d3, float d4) {
    return normalize(mk(d1 + -d2 + -d3 + d4, -d1 + -d2 + d3 + d4, -d1 + d2 + -d3 + d4));
}

// The march record (sdfv_march_aux): a pixel off the box, what the march of a covered pixel ended with, what a hit adds.
SDFV_MARCH_FN void aux_clear(sdfv_march_aux& aux) {
    aux.status = 0; aux.steps = 0;
    aux.hit_pos[0] = aux.hit_pos[1] = aux.hit_pos[2] = 0.0f;
    aux.t = 0.0f;
    aux.raw0[0] = aux.raw0[1] = aux.raw0[2] = aux.raw0[3] = 0.0f;
    aux.raw1[0] = aux.raw1[1] = aux.raw1[2] = aux.raw1[3] = 0.0f;
    aux.normal[0] = aux.normal[1] = aux.normal[2] = 0.0f;
    aux.depth = 1.0f;
}
SDFV_MARCH_FN void aux_set_march(sdfv_march_aux& aux, int status, int steps, V3 ray_pos, float dist_from_origin) {
    aux.status = status;
    aux.steps = steps;
    aux.hit_pos[0] = ray_pos.x; aux.hit_pos[1] = ray_pos.y; aux.hit_pos[2] = ray_pos.z;
    aux.t = dist_from_origin;
}
SDFV_MARCH_FN void aux_set_hit(sdfv_march_aux& aux, float4 raw0, float4 raw1, V3 n, float depth) {
    aux.raw0[0] = raw0.x; aux.raw0[1] = raw0.y; aux.raw0[2] = raw0.z; aux.raw0[3] = raw0.w;
    aux.raw1[0] = raw1.x; aux.raw1[1] = raw1.y; aux.raw1[2] = raw1.z; aux.raw1[3] = raw1.w;
    aux.normal[0] = n.x; aux.normal[1] = n.y; aux.normal[2] = n.z;
    aux.depth = depth;  // gl_FragDepth, material.frag:180-181
}

#if defined(__HIPCC__)
// 8x8 pixel tile per wave, 2x2 waves per workgroup: this thread's column and output row in workgroup tile (bx, by).
SDFV_MARCH_FN void tile_pixel(uint32_t bx, uint32_t by, uint32_t& px, uint32_t& row) {
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    px = bx * 16 + (wave & 1) * 8 + (lane & 7);
    row = by * 16 + (wave >> 1) * 8 + (lane >> 3);
}

// outColor into whichever output planes the argument block a (RaymarchArgs, ProgramMarchArgs) asks for (wave-uniform pointers,
// read where they are used).  It is written once and never re-read by the kernel: streaming stores keep it from evicting what
// the march is re-reading out of L2.
template <typename Args>
SDFV_MARCH_FN void store_color(const Args& a, uint64_t out_index, float4 v) {
    typedef float v4f __attribute__((ext_vector_type(4)));
    if (a.rgba) {
        const v4f t = {v.x, v.y, v.z, v.w};
        __builtin_nontemporal_store(t, reinterpret_cast<v4f*>(a.rgba + out_index));
    }
    if (a.rgba8) __builtin_nontemporal_store(rgba_unorm8(v), a.rgba8 + out_index);
}
#endif

}  // namespace march
}  // namespace sdfv
