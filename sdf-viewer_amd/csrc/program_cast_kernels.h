// program_cast_kernels.h -- launch interface of the ray cast over SDF programs (see program_cast_kernels.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "program_cast.h"

namespace sdfv {

struct ProgramCastArgs {
    pcast::Cast c;
    const sdfv_ray* rays;   // DEVICE, n
    sdfv_ray_hit* hits;     // DEVICE, n
    uint64_t first, n;      // this launch has rays [first, n); set by the launcher
    uint32_t rays16, hits16;  // the arrays are 16-byte aligned: 16-byte accesses (wave-uniform, decided on the host)
};

// Enqueues the cast of a.n rays on `stream` (a.first is the launcher's); n == 0 launches nothing.
hipError_t launch_program_cast(const ProgramCastArgs& a, hipStream_t stream);

}  // namespace sdfv
