// program_eval.h -- the SDF program interpreter (include/sdfgrid.h, "SDF programs"): one stack machine, compiled twice.
//
// The gfx950 kernels (program_kernels.hip) and the host mirror (host/program_sdf.cpp) both include this file, so that the two
// evaluate the same expressions in the same order.  Only + - * / sqrt, |x| and compares are used and every translation unit
// that includes it is built with -ffp-contract=off: each step is one correctly rounded IEEE f32 operation, host and device
// agree bit for bit.
//
// Shape (the point of the exercise on the device):
//  * the instruction stream is the same for every lane of a wave: `ops` is indexed by the loop counter alone, so an
//    instruction arrives by scalar loads into SGPRs (as built for gfx950: s_load_dword for the opcode, s_load_dwordx8 +
//    s_load_dwordx4 for the twelve operands; the reserved words are not fetched), one instruction ahead of the one that
//    runs, and the dispatch is a uniform branch;
//  * per-lane state lives in named registers only.  The value stack (8 deep) and the frame stack (4 deep) are fixed sets of
//    variables that SHIFT on push and pop -- every index is static, nothing is a runtime-indexed array, nothing goes to
//    scratch.  sdfv_program_create() has checked the depths, so the machine never does;
//  * a value is (distance, material INDEX): the index of the MATERIAL instruction that was current when the primitive was
//    evaluated (kNoMaterial before the first one).  A stack slot is 2 registers instead of 7, a push moves 14 registers
//    instead of 49; the six floats are fetched once, for the result -- per DISTINCT index of the wave, through a scalar load.
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC_RTC__)  // the run-time compiler is handed the headers by name (program_compile.hip)
#include "sdfgrid.h"
#else
#include "../../include/sdfgrid.h"
#endif

#if defined(__HIPCC__)
#define SDFV_PROG_FN __host__ __device__ __forceinline__
#else
#define SDFV_PROG_FN inline
#endif

namespace sdfv {
namespace prog {

constexpr uint32_t kNoMaterial = 0xffffffffu;

// fminf / fmaxf for the finite inputs a program sees, as a compare and a select: C leaves the sign of min(+0, -0) open, this
// pins it (the second operand wins only when it is strictly smaller / larger), so host, device and numpy cannot disagree.
SDFV_PROG_FN float pmin(float a, float b) { return b < a ? b : a; }
SDFV_PROG_FN float pmax(float a, float b) { return a < b ? b : a; }
// vec_length of demo_sdf_device.h: (x*x + y*y) + z*z, then sqrt
SDFV_PROG_FN float length3(float x, float y, float z) { return sqrtf(x * x + y * y + z * z); }
SDFV_PROG_FN float length2(float x, float y) { return sqrtf(x * x + y * y); }

struct Value {
    float d;
    uint32_t m;
};

struct Machine {
    float x, y, z;                                   // the current point q
    float f0x, f0y, f0z, f1x, f1y, f1z, f2x, f2y, f2z, f3x, f3y, f3z;  // saved points, f0 = innermost
    Value v0, v1, v2, v3, v4, v5, v6, v7;            // value stack, v0 = top
    uint32_t cur;                                    // current material

    SDFV_PROG_FN void push_value(float d) {
        v7 = v6; v6 = v5; v5 = v4; v4 = v3; v3 = v2; v2 = v1; v1 = v0;
        v0.d = d;
        v0.m = cur;
    }
    // b = v0, a = v1 are replaced by one value
    SDFV_PROG_FN void combine(float d, uint32_t m) {
        v0.d = d;
        v0.m = m;
        v1 = v2; v2 = v3; v3 = v4; v4 = v5; v5 = v6; v6 = v7;
    }
    SDFV_PROG_FN void push_frame() {
        f3x = f2x; f3y = f2y; f3z = f2z;
        f2x = f1x; f2y = f1y; f2z = f1z;
        f1x = f0x; f1y = f0y; f1z = f0z;
        f0x = x; f0y = y; f0z = z;
    }
    SDFV_PROG_FN void pop_frame() {
        x = f0x; y = f0y; z = f0z;
        f0x = f1x; f0y = f1y; f0z = f1z;
        f1x = f2x; f1y = f2y; f1z = f2z;
        f2x = f3x; f2y = f3y; f2z = f3z;
    }
};

// One instruction.  `o` is wave-uniform on the device (SGPRs); `pc` is its index.
SDFV_PROG_FN void step(Machine& s, const sdfv_prog_op& o, uint32_t pc) {
    const float* a = o.a;
    switch (o.op) {
        case SDFV_OP_SPHERE:
            s.push_value(length3(s.x, s.y, s.z) - a[0]);
            break;
        case SDFV_OP_CUBE:
            s.push_value(pmax(pmax(fabsf(s.x), fabsf(s.y)), fabsf(s.z)) - a[0]);
            break;
        case SDFV_OP_BOX: {
            const float ex = fabsf(s.x) - a[0], ey = fabsf(s.y) - a[1], ez = fabsf(s.z) - a[2];
            const float outside = length3(pmax(ex, 0.0f), pmax(ey, 0.0f), pmax(ez, 0.0f));
            s.push_value(outside + pmin(pmax(ex, pmax(ey, ez)), 0.0f));
            break;
        }
        case SDFV_OP_CYLINDER: {
            const float dx = length2(s.x, s.y) - a[0], dz = fabsf(s.z) - a[1];
            const float mx = pmax(dx, 0.0f), mz = pmax(dz, 0.0f);
            s.push_value(pmin(pmax(dx, dz), 0.0f) + sqrtf(mx * mx + mz * mz));
            break;
        }
        case SDFV_OP_TORUS: {
            const float u = length2(s.x, s.y) - a[0];
            s.push_value(sqrtf(u * u + s.z * s.z) - a[1]);
            break;
        }
        case SDFV_OP_PLANE:
            s.push_value(a[0] * s.x + a[1] * s.y + a[2] * s.z + a[3]);
            break;
        case SDFV_OP_PUSH_AFFINE: {
            s.push_frame();
            const float px = s.f0x, py = s.f0y, pz = s.f0z;
            s.x = a[0] * px + a[1] * py + a[2] * pz + a[3];
            s.y = a[4] * px + a[5] * py + a[6] * pz + a[7];
            s.z = a[8] * px + a[9] * py + a[10] * pz + a[11];
            break;
        }
        case SDFV_OP_PUSH_SCALE:
            s.push_frame();
            s.x = s.x * a[1];
            s.y = s.y * a[1];
            s.z = s.z * a[1];
            break;
        case SDFV_OP_POP:
            s.pop_frame();
            break;
        case SDFV_OP_POP_SCALE:
            s.pop_frame();
            s.v0.d = s.v0.d * a[0];
            break;
        case SDFV_OP_UNION: {
            const bool first = s.v1.d <= s.v0.d;
            s.combine(first ? s.v1.d : s.v0.d, first ? s.v1.m : s.v0.m);
            break;
        }
        case SDFV_OP_INTERSECT: {
            const bool first = s.v1.d >= s.v0.d;
            s.combine(first ? s.v1.d : s.v0.d, first ? s.v1.m : s.v0.m);
            break;
        }
        case SDFV_OP_SUBTRACT: {
            const float ad = s.v1.d, bd = s.v0.d;
            s.combine(pmax(ad, -bd), fabsf(ad) - fabsf(bd) < 0.0f ? s.v1.m : s.v0.m);
            break;
        }
        case SDFV_OP_SMOOTH_UNION: {
            const float ad = s.v1.d, bd = s.v0.d, k = a[0];
            const float h = pmax(k - fabsf(ad - bd), 0.0f) / k;
            s.combine(pmin(ad, bd) - (h * h) * (k * 0.25f), ad <= bd ? s.v1.m : s.v0.m);
            break;
        }
        case SDFV_OP_SMOOTH_SUBTRACT: {
            const float ad = s.v1.d, bd = s.v0.d, nb = -bd, k = a[0];
            const float h = pmax(k - fabsf(ad - nb), 0.0f) / k;
            s.combine(pmax(ad, nb) + (h * h) * (k * 0.25f), fabsf(ad) - fabsf(bd) < 0.0f ? s.v1.m : s.v0.m);
            break;
        }
        case SDFV_OP_ROUND:
            s.v0.d = s.v0.d - a[0];
            break;
        case SDFV_OP_SHELL:
            s.v0.d = fabsf(s.v0.d) - a[0];
            break;
        case SDFV_OP_MATERIAL:
            s.cur = pc;
            break;
        default:  // sdfv_program_create() lets no other opcode through
            break;
    }
}

// The whole program at one point: the result's distance and material index.
// The machine before the first instruction, at the point (px, py, pz).
SDFV_PROG_FN void start(Machine& s, float px, float py, float pz) {
    s.x = px; s.y = py; s.z = pz;
    s.f0x = s.f0y = s.f0z = s.f1x = s.f1y = s.f1z = s.f2x = s.f2y = s.f2z = s.f3x = s.f3y = s.f3z = 0.0f;
    s.v0.d = s.v1.d = s.v2.d = s.v3.d = s.v4.d = s.v5.d = s.v6.d = s.v7.d = 0.0f;
    s.v0.m = s.v1.m = s.v2.m = s.v3.m = s.v4.m = s.v5.m = s.v6.m = s.v7.m = kNoMaterial;
    s.cur = kNoMaterial;
}

SDFV_PROG_FN Value run(const sdfv_prog_op* __restrict__ ops, uint32_t n_ops, float px, float py, float pz) {
    Machine s;
    start(s, px, py, pz);
    // One instruction ahead: the scalar load of instruction pc + 1 is issued before instruction pc runs, so its latency hides
    // behind that instruction's vector work instead of standing between every two instructions.
    sdfv_prog_op cur = ops[0];
    for (uint32_t pc = 0; pc < n_ops; ++pc) {
        const sdfv_prog_op next = ops[pc + 1 < n_ops ? pc + 1 : pc];
        step(s, cur, pc);
        cur = next;
    }
    return s.v0;
}

// An EVALUATOR is what the shared kernel text (the fill's and the sampler's evaluators of program_device.h, march_pixel_program
// of program_march.h) asks for a program's value at a point: `Value operator()(float, float, float) const`.  This one is the
// interpreter -- the evaluator of every kernel built into the library.  A program compiled at run time (program_compile.hip)
// brings one of its own: the same step() per instruction, with the instruction a compile-time constant.
struct Interpreter {
    const sdfv_prog_op* ops;
    uint32_t n_ops;
    SDFV_PROG_FN Value operator()(float px, float py, float pz) const { return run(ops, n_ops, px, py, pz); }
};

}  // namespace prog
}  // namespace sdfv
