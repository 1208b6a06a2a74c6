// program_march.h -- sphere tracing an SDF program directly, per pixel, without a voxel grid: material.frag's main() /
// sdfRaycast with the texture replaced by the interpreter of program_eval.h.  One function, march_pixel_program, compiled
// twice like the interpreter: by hipcc for the kernels (program_march_kernels.hip) and by g++ for the host mirror
// (host/program_sdf.cpp), both with -ffp-contract=off -- every f32 step is rounded on its own, in the order the grid march and
// its CPU restatement take them, so the device, the host mirror and any restatement agree bit for bit on everything before
// the shading.
//
// What differs from the grid route, and only this:
//  * the march's distance is the program's own value at ray_pos: no +0.1 / -0.1 through a texel, no clamp, no filtering;
//  * the hit's texel pair is pack_sample() of the program's sample AT THE HIT POINT -- what the fill would write for a voxel
//    centred there, sRGB quantisation policy included -- and shade() / the depth formula (march_shade.h) consume it unchanged;
//  * the normal's four taps are the program's distances at p + k * h, h from the descriptor or, failing that, the grid
//    route's spacing for rp.tex_size (normal_tap_distance).
//
// The function is written for a WAVE: the march loop runs while any lane marches (wave_any), finished lanes fall out of the
// `if`, the loop carries no material data (the interpreter's value is a distance and an index), materials are resolved once
// after it and the four taps run once, under the lanes that hit.  On the host a "wave" is one pixel and wave_any is the
// identity.  The instruction stream stays wave-uniform throughout: every marching lane runs the whole program per step.
#pragma once

#include "march_shade.h"
#include "program_resolve.h"

#if defined(__HIPCC__)
#define SDFV_MARCH_FN __device__ __forceinline__
#else
#define SDFV_MARCH_FN inline
#endif

namespace sdfv {
namespace pmarch {

// What a launch knows about the frame (wave-uniform: kernel arguments).
struct Frame {
    const sdfv_prog_op* ops;
    uint32_t n_ops;
    uint32_t width, height;  // the FULL image
    float normal_h;          // the taps' distance, > 0 (normal_tap_distance)
    float air_dist;
    uint32_t srgb_round;     // SDFV_OPT_EXT_SRGB_QUANT
    sdfv_render_params rp;
};

// h of sdfNormal: the descriptor's when it gives one, else material.frag:74 for rp.tex_size -- 1 / length(texSize / lod), the
// grid route's tap distance, so that a caller comparing the two routes gets the same taps.  0 when neither is there.
inline float normal_tap_distance(const sdfv_render_params& rp, float normal_h) {
    if (normal_h > 0.0f) return normal_h;
    if (rp.tex_size[0] == 0 || rp.tex_size[1] == 0 || rp.tex_size[2] == 0 || !(rp.lod_dist_between_samples > 0.0f)) return 0.0f;
    const float sx = (float)rp.tex_size[0] / rp.lod_dist_between_samples;
    const float sy = (float)rp.tex_size[1] / rp.lod_dist_between_samples;
    const float sz = (float)rp.tex_size[2] / rp.lod_dist_between_samples;
    return 1.0f / sqrtf(sx * sx + sy * sy + sz * sz);
}

#if defined(__HIPCC__)
SDFV_MARCH_FN bool wave_any(bool b) { return __ballot(b) != 0ull; }
#else
SDFV_MARCH_FN bool wave_any(bool b) { return b; }
#endif

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

// sdfOutOfBoundsDist, material.frag:83-88
SDFV_MARCH_FN float oob_dist(const sdfv_render_params& rp, V3 p) {
    const float ox = fmaxf(rp.bounds_min[0] - p.x, p.x - rp.bounds_max[0]);
    const float oy = fmaxf(rp.bounds_min[1] - p.y, p.y - rp.bounds_max[1]);
    const float oz = fmaxf(rp.bounds_min[2] - p.z, p.z - rp.bounds_max[2]);
    return fmaxf(ox, fmaxf(oy, oz));
}

SDFV_MARCH_FN void aux_clear(sdfv_march_aux& aux) {
    aux.status = 0; aux.steps = 0;
    aux.hit_pos[0] = aux.hit_pos[1] = aux.hit_pos[2] = 0.0f;
    aux.t = 0.0f;
    aux.raw0[0] = aux.raw0[1] = aux.raw0[2] = aux.raw0[3] = 0.0f;
    aux.raw1[0] = aux.raw1[1] = aux.raw1[2] = aux.raw1[3] = 0.0f;
    aux.normal[0] = aux.normal[1] = aux.normal[2] = 0.0f;
    aux.depth = 1.0f;
}

// Pixel (px, py) of the full image (row 0 = top) through `cam`.  in_image = false: a lane of the tile beyond the image's edge
// (it takes part in nothing and its outputs are not stored).  lut: the sRGB table (LDS on the device).  rgba: outColor; aux:
// everything main() knows before shading, aux.depth = gl_FragDepth (1.0 without a hit).
// status: 1 hit | 0 the pixel is off the box | -1 out of steps | -2 out of bounds | -3 a hit behind the origin (dropped).
template <typename Lut>
SDFV_MARCH_FN void march_pixel_program(const Frame& f, const sdfv_camera& cam, uint32_t px, uint32_t py, bool in_image,
                                       const Lut& lut, float4& rgba, sdfv_march_aux& aux) {
    const sdfv_render_params& rp = f.rp;
    rgba = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    aux_clear(aux);

    // primary ray through the pixel centre
    const float ndc_x = (((float)px + 0.5f) / (float)f.width) * 2.0f - 1.0f;
    const float ndc_y = 1.0f - (((float)py + 0.5f) / (float)f.height) * 2.0f;
    const float sx = ndc_x * cam.aspect * cam.tan_half_fovy;
    const float sy = ndc_y * cam.tan_half_fovy;
    const V3 eye = mk(cam.eye[0], cam.eye[1], cam.eye[2]);
    const V3 d0 = normalize(mk(cam.forward[0] + cam.right[0] * sx + cam.up[0] * sy,
                               cam.forward[1] + cam.right[1] * sx + cam.up[1] * sy,
                               cam.forward[2] + cam.right[2] * sx + cam.up[2] * sy));

    // the bbox fragment: slab test standing in for the rasterised cube (scene/sdf/mod.rs:254-282) -- the entry point when the
    // camera is outside the box, the exit point when it is inside
    const float tx1 = (rp.bounds_min[0] - eye.x) / d0.x, tx2 = (rp.bounds_max[0] - eye.x) / d0.x;
    const float ty1 = (rp.bounds_min[1] - eye.y) / d0.y, ty2 = (rp.bounds_max[1] - eye.y) / d0.y;
    const float tz1 = (rp.bounds_min[2] - eye.z) / d0.z, tz2 = (rp.bounds_max[2] - eye.z) / d0.z;
    const float tnear = fmaxf(fmaxf(fminf(tx1, tx2), fminf(ty1, ty2)), fminf(tz1, tz2));
    const float tfar = fminf(fminf(fmaxf(tx1, tx2), fmaxf(ty1, ty2)), fmaxf(tz1, tz2));
    const bool covered = in_image && (tfar >= tnear && tfar > 0.0f);
    if (!wave_any(covered)) return;  // a tile off the box leaves before it touches the program

    // main(), material.frag:133-139
    const float tfrag = tnear > 0.0f ? tnear : tfar;
    V3 ray_origin = madd(eye, d0, tfrag);
    const V3 ray_dir = normalize(sub(ray_origin, eye));
    if (oob_dist(rp, madd(ray_origin, ray_dir, 0.2f)) > 0.0f) ray_origin = madd(eye, ray_dir, 0.2f);

    // sdfRaycast(rayOrigin, rayDir, 256), material.frag:92-128: iteration 255 is the one that gives up
    V3 ray_pos = ray_origin;
    float dist_from_origin = 0.0f;
    int status = covered ? -1 : 0;
    int steps = 0;
    prog::Value v;
    v.d = 0.0f;
    v.m = prog::kNoMaterial;
    bool marching = covered;
    for (int i = 0; i < 255; ++i) {
        if (!wave_any(marching)) break;
        if (marching) {
            if (oob_dist(rp, ray_pos) > 1e-4f) {
                status = -2;
                marching = false;
            } else {
                v = prog::run(f.ops, f.n_ops, ray_pos.x, ray_pos.y, ray_pos.z);
                ++steps;
                if (v.d < 1e-5f) {
                    status = 1;
                    marching = false;
                } else {
                    dist_from_origin += v.d;
                    ray_pos = madd(ray_pos, ray_dir, v.d);
                }
            }
        }
    }
    if (status == 1 && dist_from_origin < 0.0f) status = -3;  // material.frag:145: hit.w < 0 is "no hit"
    if (covered) {
        aux.status = status;
        aux.steps = steps;
        aux.hit_pos[0] = ray_pos.x; aux.hit_pos[1] = ray_pos.y; aux.hit_pos[2] = ray_pos.z;
        aux.t = dist_from_origin;
    }
    const bool hit = status == 1;
    if (!wave_any(hit)) return;
    if (hit) {
        // the texel pair of a voxel centred on the hit: v is the program's value there (the march's last evaluation)
        const Sample s = resolve(f.ops, v, false);
        float4 raw0, raw1;
        if (f.srgb_round) pack_sample<true>(s, lut, f.air_dist, raw0, raw1);
        else pack_sample<false>(s, lut, f.air_dist, raw0, raw1);
        // sdfNormal, material.frag:73-80: taps k.xyy, k.yyx, k.yxy, k.xxx with k = (1, -1), summed in that order
        const float h = f.normal_h;
        V3 acc = mk(0.0f, 0.0f, 0.0f);
#if defined(__HIPCC__)
#pragma unroll 1
#endif
        for (int t = 0; t < 4; ++t) {  // (one copy of the interpreter for the four)
            const float kx = (t == 0 || t == 3) ? 1.0f : -1.0f, ky = t >= 2 ? 1.0f : -1.0f, kz = (t & 1) ? 1.0f : -1.0f;
            const float d = prog::run(f.ops, f.n_ops, ray_pos.x + kx * h, ray_pos.y + ky * h, ray_pos.z + kz * h).d;
            acc = t == 0 ? mk(kx * d, ky * d, kz * d) : mk(acc.x + kx * d, acc.y + ky * d, acc.z + kz * d);
        }
        const V3 n = normalize(acc);
        rgba = shade(rp, raw0, raw1);
        aux.raw0[0] = raw0.x; aux.raw0[1] = raw0.y; aux.raw0[2] = raw0.z; aux.raw0[3] = raw0.w;
        aux.raw1[0] = raw1.x; aux.raw1[1] = raw1.y; aux.raw1[2] = raw1.z; aux.raw1[3] = raw1.w;
        aux.normal[0] = n.x; aux.normal[1] = n.y; aux.normal[2] = n.z;
        aux.depth = frag_depth_of(cam.bvp, ray_pos.x, ray_pos.y, ray_pos.z);
    }
}

}  // namespace pmarch
}  // namespace sdfv
