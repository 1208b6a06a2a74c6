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

#include "march_common.h"
#include "program_resolve.h"

namespace sdfv {
namespace pmarch {
using namespace march;  // the ray set-up, the taps and the record: march_common.h

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

#if defined(__HIPCC__)
SDFV_MARCH_FN bool wave_any(bool b) { return __ballot(b) != 0ull; }
#else
SDFV_MARCH_FN bool wave_any(bool b) { return b; }
#endif

// Pixel (px, py) of the full image (row 0 = top) through `cam`.  in_image = false: a lane of the tile beyond the image's edge
// (it takes part in nothing and its outputs are not stored).  lut: the sRGB table (LDS on the device).  rgba: outColor; aux:
// everything main() knows before shading, aux.depth = gl_FragDepth (1.0 without a hit).
// status: 1 hit | 0 the pixel is off the box | -1 out of steps | -2 out of bounds | -3 a hit behind the origin (dropped).
// eval: the program's evaluator (program_eval.h) -- it gives the march step, the hit sample and the four taps.
template <typename Eval, typename Lut>
SDFV_MARCH_FN void march_pixel_program(const Frame& f, const Eval& eval, const sdfv_camera& cam, uint32_t px, uint32_t py, bool in_image,
                                       const Lut& lut, float4& rgba, sdfv_march_aux& aux) {
    const sdfv_render_params& rp = f.rp;
    rgba = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    aux_clear(aux);

    const V3 eye = mk(cam.eye[0], cam.eye[1], cam.eye[2]);
    const V3 d0 = normalize(pixel_ray_raw(f.width, f.height, cam, px, py));
    float tfrag;
    const bool covered = box_slab_test(rp, eye, d0, in_image, tfrag);
    if (!wave_any(covered)) return;  // a tile off the box leaves before it touches the program
    V3 ray_origin, ray_dir;
    fragment_ray(rp, eye, d0, tfrag, ray_origin, ray_dir);

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
                v = eval(ray_pos.x, ray_pos.y, ray_pos.z);
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
    if (covered) aux_set_march(aux, status, steps, ray_pos, dist_from_origin);
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
            const V3 k = tap_sign(t);
            const float d = eval(ray_pos.x + k.x * h, ray_pos.y + k.y * h, ray_pos.z + k.z * h).d;
            acc = t == 0 ? mk(k.x * d, k.y * d, k.z * d) : mk(acc.x + k.x * d, acc.y + k.y * d, acc.z + k.z * d);
        }
        const V3 n = normalize(acc);
        rgba = shade(rp, raw0, raw1);
        aux_set_hit(aux, raw0, raw1, n, frag_depth_of(cam.bvp, ray_pos.x, ray_pos.y, ray_pos.z));
    }
}

// ... with the interpreter over f.ops as the evaluator (the kernels of the library, the host mirror)
template <typename Lut>
SDFV_MARCH_FN void march_pixel_program(const Frame& f, const sdfv_camera& cam, uint32_t px, uint32_t py, bool in_image,
                                       const Lut& lut, float4& rgba, sdfv_march_aux& aux) {
    march_pixel_program(f, prog::Interpreter{f.ops, f.n_ops}, cam, px, py, in_image, lut, rgba, aux);
}

}  // namespace pmarch
}  // namespace sdfv
