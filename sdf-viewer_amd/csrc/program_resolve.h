// program_resolve.h -- from the interpreter's result (distance, material INDEX) to a sample: the six operands of the MATERIAL
// instruction the value carries.  Shared by the program kernels (program_kernels.hip, program_march_kernels.hip) and, in its
// plain form, by the host mirror of the direct march.
#pragma once

#include "demo_sdf_device.h"
#include "program_eval.h"

namespace sdfv {

#if defined(__HIPCC__)
// The index differs between lanes, the instruction memory is read by scalar loads only: one round per DISTINCT index among the
// wave's lanes (a wave of neighbouring voxels or pixels sees one to three materials).
__device__ __forceinline__ Sample resolve(const sdfv_prog_op* __restrict__ ops, const prog::Value& v, bool distance_only) {
    Sample s;
    s.distance = v.d;
    s.m = zero_mat();
    bool pending = !distance_only && v.m != prog::kNoMaterial;
    while (pending) {
        if (v.m == (uint32_t)__builtin_amdgcn_readfirstlane(v.m)) {
            // (read again under the narrowed EXEC: the compiler forwards the equality into this block, and an index it takes
            // for the per-lane v.m would turn the fetch into a vector load)
            const float* a = ops[__builtin_amdgcn_readfirstlane(v.m)].a;
            s.m.r = a[0]; s.m.g = a[1]; s.m.b = a[2];
            s.m.metallic = a[3]; s.m.roughness = a[4]; s.m.occlusion = a[5];
            pending = false;
        }
    }
    return s;
}
#else
inline Sample resolve(const sdfv_prog_op* ops, const prog::Value& v, bool distance_only) {
    Sample s;
    s.distance = v.d;
    s.m = zero_mat();
    if (!distance_only && v.m != prog::kNoMaterial) {
        const float* a = ops[v.m].a;
        s.m.r = a[0]; s.m.g = a[1]; s.m.b = a[2];
        s.m.metallic = a[3]; s.m.roughness = a[4]; s.m.occlusion = a[5];
    }
    return s;
}
#endif

}  // namespace sdfv
