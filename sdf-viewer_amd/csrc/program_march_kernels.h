// program_march_kernels.h -- launch interface of the direct march of SDF programs (see program_march_kernels.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "program_march.h"

namespace sdfv {

constexpr uint32_t kProgramMarchCameras = 16;  // cameras of one launch: they ride in the kernel arguments (16 x 120 B)

struct ProgramMarchArgs {
    pmarch::Frame f;
    uint32_t y0, y1;        // rows rendered by this launch; outputs hold n_cameras x (y1 - y0) x width pixels
    uint32_t n_cameras;     // <= kProgramMarchCameras
    float4* rgba;           // or nullptr (rgba8 only)
    uint32_t* rgba8;        // or nullptr
    sdfv_march_aux* aux;    // or nullptr
    float* depth;           // or nullptr
    sdfv_camera cameras[kProgramMarchCameras];
};

#if !defined(__HIPCC_RTC__)
struct ProgramKernels;  // program_kernels.h
hipError_t launch_program_march(const ProgramMarchArgs& a, const ProgramKernels& k, hipStream_t stream);
#endif

}  // namespace sdfv
