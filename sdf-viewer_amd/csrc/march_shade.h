// march_shade.h -- what every march does with a hit once the two texels are known: the shading tail (material.frag:158-173),
// gl_FragDepth (:180-181) and the 8-bit framebuffer conversion.  Shared by the grid march (raymarch_kernels.hip), the direct
// march of SDF programs (program_march.h) and that march's host mirror, so that the routes' colours come from one text.
//
// Compiled by hipcc for the kernels and by g++ for the host mirror.  The arithmetic is the same and in the same order; what
// differs is how pow and the tone mapping's divisions are evaluated (see shader_pow), which is why shaded colours are compared
// to a tolerance and everything before them bit for bit.
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC_RTC__)  // the run-time compiler is handed the headers by name (program_compile.hip)
#include "sdfgrid.h"
#else
#include "../../include/sdfgrid.h"
#endif

#if defined(__HIPCC__)
#define SDFV_SHADE_FN __device__ __forceinline__
#else
#define SDFV_SHADE_FN inline
#endif

namespace sdfv {

SDFV_SHADE_FN float mixf(float a, float b, float t) { return a * (1.0f - t) + b * t; }

// pow and division of the shading tail the way a GLSL compiler emits them for a GPU: exp2(y * log2(x)) and a * rcp(b) on
// the hardware's transcendental unit (v_log_f32 / v_exp_f32 / v_rcp_f32, 1 ulp each).  The results feed outColor only, whose
// gate is 1e-4 against the CPU restatement (libm powf, IEEE divide): measured distance 2.4e-7 at most (1.2e-7 with the
// scene's ACES + sRGB defaults, as with ocml's powf before).  x >= 0 here;
// x == 0 gives exp2(-inf) = 0 like powf.  The host mirror evaluates libm's powf and the IEEE divide.
#if defined(__HIPCC__)
SDFV_SHADE_FN float shader_pow(float x, float y) { return __builtin_amdgcn_exp2f(y * __builtin_amdgcn_logf(x)); }
SDFV_SHADE_FN float shader_div(float a, float b) { return a * __builtin_amdgcn_rcpf(b); }
#else
SDFV_SHADE_FN float shader_pow(float x, float y) { return powf(x, y); }
SDFV_SHADE_FN float shader_div(float a, float b) { return a / b; }
#endif

// three-d 0.18.2 tone_mapping / color_mapping (material.frag:167-168) [not vendored in the reference]
SDFV_SHADE_FN float tone_map(uint32_t type, float c) {
    if (type == 1) c = shader_div(c, c + 1.0f);
    else if (type == 2) c = shader_div(c * (2.51f * c + 0.03f), c * (2.43f * c + 0.59f) + 0.14f);
    else if (type == 3) {
        float x = fmaxf(0.0f, c - 0.004f);
        c = shader_div(x * (6.2f * x + 0.5f), x * (6.2f * x + 1.7f) + 0.06f);
        c = shader_pow(c, 2.2f);
    }
    return fminf(fmaxf(c, 0.0f), 1.0f);
}
SDFV_SHADE_FN float color_map(uint32_t type, float c) {
    if (type != 1) return c;
    float ginv = 1.0f / 2.4f;
    float select = c >= 0.0031308f ? 1.0f : 0.0f;
    float lo = c * 12.92f;
    float hi = 1.055f * shader_pow(c, ginv) - 0.055f;
    return mixf(lo, hi, select);
}

// material.frag:158-173 with the scene's single ambient light (scene/mod.rs:106-110)
SDFV_SHADE_FN float4 shade(const sdfv_render_params& rp, float4 raw0, float4 raw1) {
    float metallic = raw1.x, occlusion = raw1.z;
    float albedo[3] = {raw0.y * rp.tint[0], raw0.z * rp.tint[1], raw0.w * rp.tint[2]};
    float out[3];
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int c = 0; c < 3; ++c) {
        float lit = occlusion * rp.ambient[c] * mixf(albedo[c], 0.0f, metallic);
        // further ambient lights of the light list: calculate_lighting sums the lights' contributions
        for (uint32_t l = 0; l < rp.n_lights; ++l)
            lit += occlusion * (rp.lights[l].intensity * rp.lights[l].color[c]) * mixf(albedo[c], 0.0f, metallic);
        lit = tone_map(rp.tone_mapping, lit);
        lit = color_map(rp.color_mapping, lit);
        if (rp.gamma > 0.0f) lit = shader_pow(lit, rp.gamma);
        out[c] = lit;
    }
    return make_float4(out[0], out[1], out[2], rp.tint[3]);
}

// gl_FragDepth, material.frag:180-181: (BVP * vec4(p, 1)).z / .w; m = sdfv_camera::bvp (column-major)
SDFV_SHADE_FN float frag_depth_of(const float* m, float x, float y, float z) {
    const float hz = m[2] * x + m[6] * y + m[10] * z + m[14];
    const float hw = m[3] * x + m[7] * y + m[11] * z + m[15];
    return hz / hw;
}

// float -> 8-bit UNORM as a GL framebuffer converts it: clamp to [0, 1], scale by 255, round to nearest (even); NaN -> 0
SDFV_SHADE_FN uint32_t unorm8(float c) {
    const float v = fminf(fmaxf(c, 0.0f), 1.0f) * 255.0f;
#if defined(__HIPCC__)
    return (uint32_t)__float2uint_rn(v);
#else
    return (uint32_t)nearbyintf(v);
#endif
}
// R in the low byte
SDFV_SHADE_FN uint32_t rgba_unorm8(float4 v) { return unorm8(v.x) | unorm8(v.y) << 8 | unorm8(v.z) << 16 | unorm8(v.w) << 24; }

}  // namespace sdfv
