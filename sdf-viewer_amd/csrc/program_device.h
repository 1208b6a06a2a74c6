// program_device.h -- the bodies of the SDF-program kernels that exist once per way of evaluating a program: the dense fill,
// the point samplers and the direct march, each over an EVALUATOR (program_eval.h).  hipcc instantiates them with the
// interpreter (program_kernels.hip, program_march_kernels.hip); the translation unit that sdfv_program_compile generates
// (program_compile.hip) includes this very text and instantiates it with the evaluator of one program.  Everything else of a
// kernel -- skeleton, texel packing, material fetch, stores -- is the same code either way, which is why the two give the
// same bits.
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
