// program_march_kernels.hip -- SDF programs rendered directly on gfx950: one thread per pixel sphere-traces the program itself
// (program_march.h), no voxel grid in between.
//
// Shape: a 64-lane wave is an 8x8 pixel tile (neighbouring rays take similar numbers of steps: a wave lasts as long as its
// longest ray, DESIGN.md 3.7 has the lane utilisation of 8x8 against 64x1), a 256-thread workgroup 16x16, blockIdx.z the
// camera.  The march loop is a wave loop around the wave-uniform instruction stream: per step every marching lane runs the
// whole program once, instructions arrive by scalar loads (program_eval.h), finished lanes are masked out and the wave leaves
// when none is left.  All per-lane state is in registers; the only memory traffic is the sRGB table (LDS, as in the fills) and
// the outputs: 16-byte streaming stores for rgba, 4-byte ones for rgba8 and depth, the 72-byte record when asked for.  ALU-bound
// where the grid march is gather-latency-bound.  The loop is bounded by 255 steps of at most 256 instructions: it cannot hang.
#include "program_march_kernels.h"

#include "program_device.h"

namespace sdfv {

// the interpreter as the evaluator of the kernel definitions (program_device.h)
#define SDFV_EVAL_LOOPED(ops, n_ops) prog::Interpreter{ops, n_ops}

SDFV_PROGRAM_KERNEL_march(sdfprog_march)
SDFV_PROGRAM_KERNEL_march_aux(sdfprog_march_aux)

hipError_t launch_program_march(const ProgramMarchArgs& a, const ProgramKernels& k, hipStream_t stream) {
    if (a.f.width == 0 || a.y1 <= a.y0 || a.n_cameras == 0) return hipSuccess;
    if (a.n_cameras > kProgramMarchCameras) return hipErrorInvalidValue;
    const uint32_t tiles_x = (a.f.width + 15) / 16, tiles_y = (a.y1 - a.y0 + 15) / 16;
    if (tiles_y > 65535u) return hipErrorInvalidValue;
    void* params[] = {const_cast<ProgramMarchArgs*>(&a)};
    return k.launch(a.aux ? kKernelMarchAux : kKernelMarch, a.aux ? (const void*)sdfprog_march_aux : (const void*)sdfprog_march,
                    dim3(tiles_x, tiles_y, a.n_cameras), dim3(kBlock), params, stream);
}

}  // namespace sdfv
