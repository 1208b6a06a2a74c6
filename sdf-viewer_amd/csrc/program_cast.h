// program_cast.h -- one ray of a caller's list against an SDF program (include/sdfgrid.h, sdfv_program_cast_desc): where it
// hits, and what is there.  One function, cast_ray_program, compiled twice like march_pixel_program of program_march.h: by hipcc
// for the kernel (program_cast_kernels.hip) and by g++ for the host mirror (host/program_sdf.cpp), both with -ffp-contract=off,
// so that every f32 step is rounded on its own, in the header's order, and the two agree on every byte of a record.
//
// What differs from the per-pixel march: the ray is the caller's (no camera, no 0.2 origin shift), the march is clipped to
// [t_min, t_max] and to the box by the slab test's own tnear / tfar, the position is origin + u * t from the accumulated t (not
// itself accumulated), and the result is a record: no texel packing, no shading.  The normal is the mesh route's
// (normal_default_impl: the taps and sums of program_mesh_device.h's tap_normal, 1 / length and three products), because a
// caller compares it with sdfv_program_normal_points.
//
// Written for a WAVE, as the march is: the loop runs while any lane marches, finished lanes fall out of the `if`, the loop carries
// a distance and a material INDEX, materials are resolved once after it and the four taps run once, under the lanes that hit,
// through one further copy of the evaluator.  The instruction stream stays wave-uniform: the interpreter's scalar fetch works
// as it does everywhere else.  On the host a "wave" is one ray.
#pragma once

#include "program_march.h"

namespace sdfv {
namespace pcast {
using namespace march;  // V3, normalize, madd, length, the slab arithmetic: march_common.h
using pmarch::wave_any;

// What a launch knows about the list (wave-uniform: kernel arguments); the defaults are already in place
// (sdfv_program_raycast_check).
struct Cast {
    const sdfv_prog_op* ops;
    uint32_t n_ops;
    uint32_t flags;      // SDFV_CAST_*
    float bounds_min[3], bounds_max[3];  // the descriptor's box, under the names the slab arithmetic reads
    uint32_t max_steps;  // 1 .. 4096
    float hit_eps;       // > 0
    float normal_eps;    // > 0
};

SDFV_MARCH_FN void hit_clear(sdfv_ray_hit& h) {
    h.status = 0; h.steps = 0;
    h.t = 0.0f;
    h.pos[0] = h.pos[1] = h.pos[2] = 0.0f;
    h.normal[0] = h.normal[1] = h.normal[2] = 0.0f;
    h.sample.distance = 0.0f;
    h.sample.color[0] = h.sample.color[1] = h.sample.color[2] = 0.0f;
    h.sample.metallic = h.sample.roughness = h.sample.occlusion = 0.0f;
}

// `ray` against the program behind `eval` (program_eval.h's evaluator).  live = false: a lane beyond the list (it takes part in
// nothing and its record is not stored).  Every field of `hit` is written.
template <typename Eval>
SDFV_MARCH_FN void cast_ray_program(const Cast& c, const Eval& eval, const sdfv_ray& ray, bool live, sdfv_ray_hit& hit) {
    hit_clear(hit);
    const V3 origin = mk(ray.origin[0], ray.origin[1], ray.origin[2]);
    const V3 u = normalize(mk(ray.dir[0], ray.dir[1], ray.dir[2]));
    float tnear, tfar;
    box_slab_interval(c, origin, u, tnear, tfar);
    const float t0 = fmaxf(ray.t_min, tnear), t1 = fminf(ray.t_max, tfar);
    // (fmaxf / fminf drop a NaN operand, so t1 >= t0 alone would let a ray whose slab values are ALL NaN -- a zero or NaN
    // direction, a NaN origin -- march from t_min to t_max; tfar >= tnear is implied by t1 >= t0 for numbers and false for those)
    const bool crosses = live && t1 >= t0 && tfar >= tnear;
    if (!wave_any(crosses)) return;         // a wave off the box leaves before it touches the program

    // The loop keeps, per lane, what the march of program_march.h keeps and no more: t is the parameter of the LAST EVALUATION
    // -- the advance t + v.d is compared in the iteration that computes it and committed only if another evaluation follows -- so
    // pos, the final t and the status all follow from (t, v) once the loop is over, by the very operations the header lists.
    float t = t0;
    int steps = 0;
    prog::Value v;
    v.d = 0.0f;
    v.m = prog::kNoMaterial;
    bool marching = crosses;
    // p: where the lane's last evaluation was, origin + u * t.  It is computed at ONE place, for the march and for the record,
    // by every lane that crosses: a second copy of the expression behind the loop made the compiler keep origin and u twice, in
    // two register pairings (87 VGPRs against 78).  The loop is bounded whatever the distances are: a NaN runs it out.
    V3 p;
    for (uint32_t i = 0;; ++i) {
        p = madd(origin, u, t);
        if (i == c.max_steps || !wave_any(marching)) break;
        if (marching) {
            v = eval(p.x, p.y, p.z);
            ++steps;
            if (v.d < c.hit_eps) {
                marching = false;
            } else {
                const float advanced = t + v.d;
                if (advanced > t1) marching = false;
                else if (i + 1 < c.max_steps) t = advanced;
            }
        }
    }
    const bool struck = crosses && v.d < c.hit_eps;
    if (crosses) {
        if (!struck) t = t + v.d;
        hit.status = struck ? 1 : (t > t1 ? -2 : -1);
        hit.steps = steps;
        hit.t = t;
        hit.pos[0] = p.x; hit.pos[1] = p.y; hit.pos[2] = p.z;
    }
    if (!wave_any(struck)) return;
    if (struck) {
        // sample(pos, false): v is the program's value at pos (the march's last evaluation); without SDFV_CAST_MATERIALS the
        // distance alone
        const Sample s = resolve(c.ops, v, !(c.flags & SDFV_CAST_MATERIALS));
        hit.sample.distance = s.distance;
        hit.sample.color[0] = s.m.r; hit.sample.color[1] = s.m.g; hit.sample.color[2] = s.m.b;
        hit.sample.metallic = s.m.metallic; hit.sample.roughness = s.m.roughness; hit.sample.occlusion = s.m.occlusion;
        if (c.flags & SDFV_CAST_NORMALS) {
            // normal_default_impl (defaults.rs:49-56): taps at p + (e, -e, -e), (-e, e, -e), (-e, -e, e), (e, e, e), the sums
            // left to right in tap order with the first term standing alone, then times 1 / length
            const float e = c.normal_eps;
            V3 acc = mk(0.0f, 0.0f, 0.0f);
#if defined(__HIPCC__)
#pragma unroll 1
#endif
            for (int k = 0; k < 4; ++k) {  // (one copy of the evaluator for the four)
                const float kx = (k == 0 || k == 3) ? 1.0f : -1.0f;
                const float ky = (k == 1 || k == 3) ? 1.0f : -1.0f;
                const float kz = (k == 2 || k == 3) ? 1.0f : -1.0f;
                const float d = eval(p.x + kx * e, p.y + ky * e, p.z + kz * e).d;
                acc = k == 0 ? mk(kx * d, ky * d, kz * d) : mk(acc.x + kx * d, acc.y + ky * d, acc.z + kz * d);
            }
            const float inv = 1.0f / length(acc);
            hit.normal[0] = acc.x * inv; hit.normal[1] = acc.y * inv; hit.normal[2] = acc.z * inv;
        }
    }
}

}  // namespace pcast
}  // namespace sdfv
