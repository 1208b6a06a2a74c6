// program_kernels.h -- launch interface of the SDF-program kernels (see program_kernels.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/sdfgrid.h"

namespace sdfv {

struct ProgramFillArgs {
    const sdfv_prog_op* ops;  // DEVICE copy of the validated program
    uint32_t n_ops;
    uint32_t W, H;            // global width and height
    uint32_t z_begin;         // first global slice held by tex0 / tex1
    uint32_t slab_d;          // slices held
    float dm1[3];             // (float)dim - 1.0f          (scene/sdf/mod.rs:168)
    float bb_size[3];         // bb[1] - bb[0]              (scene/sdf/mod.rs:167)
    float bb_min[3];
    float air_dist;
    uint32_t x_chunks;        // set by the launcher: ceil(W / TX)
    float4* tex0;
    float4* tex1;
    float* dist;              // optional distance volume written in the same pass
    uint32_t dist_ilv;        // its layout: 0 texture order, 1 y-interleaved (fill_kernels.h FillArgs::dist_ilv)
    uint32_t srgb_round;      // SDFV_OPT_EXT_SRGB_QUANT
    uint32_t nontemporal;     // texture stores pass L2 by (picks the _nt kernels)
};

hipError_t launch_program_fill(const ProgramFillArgs& a, hipStream_t stream);
hipError_t launch_program_sample_points(const sdfv_prog_op* ops, uint32_t n_ops, const float* points, size_t n,
                                        bool distance_only, sdfv_sample* out, hipStream_t stream);

}  // namespace sdfv
