// program_device.h -- the bodies of the SDF-program kernels that exist once per way of evaluating a program: the dense fill,
// the point samplers and the direct march, each over an EVALUATOR (program_eval.h), and at the end the kernels themselves, each
// stated once as a definition over two evaluator expressions.  hipcc instantiates them with the interpreter
// (program_kernels.hip, program_march_kernels.hip); the translation unit that sdfv_program_compile generates
// (program_compile.hip) includes this very text and instantiates it with the evaluator of one program.  Everything else of a
// kernel -- parameters, skeleton, texel packing, material fetch, stores -- is the same code either way, which is why the two
// take the same arguments and give the same bits.
#pragma once

#include "kernel_common.h"
#include "program_eval.h"
#include "program_kernels.h"
#include "program_march_kernels.h"
#include "program_resolve.h"

namespace sdfv {

// The program as the fill's evaluator.  The Srgba::from policy is a wave-uniform branch here (the evaluation is the body: six
// kernels instead of twelve).
template <typename Eval>
struct ProgramFillEval {
    Eval eval;
    const sdfv_prog_op* ops;  // the device copy: the materials of the result (resolve)
    uint32_t srgb_round;
    __device__ __forceinline__ ProgramFillEval(const ProgramFillArgs& a, const Eval& e) : eval(e), ops(a.ops), srgb_round(a.srgb_round) {}
    __device__ __forceinline__ void operator()(float px, float py, float pz, const LdsLut& lut, float air_dist, float4& t0,
                                               float4& t1) const {
        const Sample s = resolve(ops, eval(px, py, pz), false);
        if (srgb_round) pack_sample<true>(s, lut, air_dist, t0, t1);
        else pack_sample<false>(s, lut, air_dist, t0, t1);
    }
};

// ... and as the element map's for the samplers: a point in, its 28-byte record out
template <typename Eval>
struct ProgramSampleEval {
    Eval eval;
    const sdfv_prog_op* ops;
    bool distance_only;
    __device__ __forceinline__ void operator()(float* v, bool live) const {
        if (live) write_record(v, resolve(ops, eval(v[0], v[1], v[2]), distance_only));
    }
};

// One pixel of the direct march per thread: tile, camera, march_pixel_program, stores.
template <bool AUX, typename Eval>
__device__ __forceinline__ void program_march(const ProgramMarchArgs& a, const Eval& eval) {
    __shared__ float s_lut[256];
    const LdsLut lut = stage_srgb_lut(s_lut);
    __syncthreads();

    uint32_t px, row;  // row of the output
    march::tile_pixel(blockIdx.x, blockIdx.y, px, row);
    const uint32_t py = a.y0 + row;
    const uint32_t cam_idx = blockIdx.z;
    const bool in_image = px < a.f.width && py < a.y1;
    const sdfv_camera& cam = a.cameras[cam_idx];  // wave-uniform: scalar loads from the kernel arguments
    const uint64_t out_index = ((uint64_t)cam_idx * (a.y1 - a.y0) + row) * a.f.width + px;

    float4 rgba;
    sdfv_march_aux aux;
    pmarch::march_pixel_program(a.f, eval, cam, px, py, in_image, lut, rgba, aux);
    if (!in_image) return;
    march::store_color(a, out_index, rgba);
    if (a.depth) a.depth[out_index] = aux.depth;
    if (AUX) a.aux[out_index] = aux;
}

}  // namespace sdfv

// ---- the kernels: SDFV_PROGRAM_KERNEL_<stem>(name), one per row of SDFV_PROGRAM_KERNELS (program_kernels.h) ----
// Each states a kernel's parameter list and body ONCE; the translation unit that invokes it has defined the two evaluators:
//   SDFV_EVAL_ONCE(ops, n_ops)    the program where it is run outside any loop (the fill, the samplers, the lattices, the
//                                 material run),
//   SDFV_EVAL_LOOPED(ops, n_ops)  ... and inside one (the march, the four taps of a normal).
// In the library both are prog::Interpreter{ops, n_ops} and the name is sdfprog_<stem>; in the unit sdfv_program_compile
// generates they are Compiled<false>{} and Compiled<true>{}, which ignore their arguments, and the name is sdfprogc_<stem>.  So
// the two kernels of a pair cannot differ in their parameters: ProgramKernels::launch hands either the same argument array.
#define SDFV_PROGRAM_KERNEL_FILL(name, TX, NT)                                       \
    extern "C" __global__ __launch_bounds__(kBlock) void name(ProgramFillArgs a) {  \
        dense_fill_rows<TX, NT, false>(a, ProgramFillEval(a, SDFV_EVAL_ONCE(a.ops, a.n_ops))); \
    }
#define SDFV_PROGRAM_KERNEL_fill_tx64(name) SDFV_PROGRAM_KERNEL_FILL(name, 64, false)
#define SDFV_PROGRAM_KERNEL_fill_tx64_nt(name) SDFV_PROGRAM_KERNEL_FILL(name, 64, true)
#define SDFV_PROGRAM_KERNEL_fill_tx128(name) SDFV_PROGRAM_KERNEL_FILL(name, 128, false)
#define SDFV_PROGRAM_KERNEL_fill_tx128_nt(name) SDFV_PROGRAM_KERNEL_FILL(name, 128, true)
#define SDFV_PROGRAM_KERNEL_fill_tx256(name) SDFV_PROGRAM_KERNEL_FILL(name, 256, false)
#define SDFV_PROGRAM_KERNEL_fill_tx256_nt(name) SDFV_PROGRAM_KERNEL_FILL(name, 256, true)

#define SDFV_PROGRAM_KERNEL_sample_points(name)                                                                        \
    extern "C" __global__ __launch_bounds__(kBlock) void name(const sdfv_prog_op* __restrict__ ops, uint32_t n_ops,   \
                                                              const float* __restrict__ points, size_t first, size_t n, \
                                                              bool distance_only, float* __restrict__ out) {          \
        auto eval = SDFV_EVAL_ONCE(ops, n_ops);                                                                        \
        map_elements<3, 7>(ProgramSampleEval<decltype(eval)>{eval, ops, distance_only}, points, first, n, out);        \
    }
#define SDFV_PROGRAM_KERNEL_sample_points_staged(name)                                                                 \
    extern "C" __global__ __launch_bounds__(kBlock) void name(const sdfv_prog_op* __restrict__ ops, uint32_t n_ops,   \
                                                              const float4* __restrict__ points, bool distance_only,  \
                                                              float4* __restrict__ out) {                             \
        auto eval = SDFV_EVAL_ONCE(ops, n_ops);                                                                        \
        map_elements_staged<3, 7>(ProgramSampleEval<decltype(eval)>{eval, ops, distance_only}, points, out);           \
    }

#define SDFV_PROGRAM_KERNEL_MARCH(name, AUX)                                          \
    extern "C" __global__ __launch_bounds__(kBlock) void name(ProgramMarchArgs a) {  \
        program_march<AUX>(a, SDFV_EVAL_LOOPED(a.f.ops, a.f.n_ops));                  \
    }
#define SDFV_PROGRAM_KERNEL_march(name) SDFV_PROGRAM_KERNEL_MARCH(name, false)
#define SDFV_PROGRAM_KERNEL_march_aux(name) SDFV_PROGRAM_KERNEL_MARCH(name, true)
