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

#include "kernel_common.h"

namespace sdfv {

namespace {

template <bool AUX>
__device__ __forceinline__ void program_march(const ProgramMarchArgs& a) {
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
    pmarch::march_pixel_program(a.f, cam, px, py, in_image, lut, rgba, aux);
    if (!in_image) return;
    march::store_color(a, out_index, rgba);
    if (a.depth) a.depth[out_index] = aux.depth;
    if (AUX) a.aux[out_index] = aux;
}

}  // namespace

extern "C" {

__global__ __launch_bounds__(kBlock) void sdfprog_march(ProgramMarchArgs a) { program_march<false>(a); }
__global__ __launch_bounds__(kBlock) void sdfprog_march_aux(ProgramMarchArgs a) { program_march<true>(a); }

}  // extern "C"

hipError_t launch_program_march(const ProgramMarchArgs& a, hipStream_t stream) {
    if (a.f.width == 0 || a.y1 <= a.y0 || a.n_cameras == 0) return hipSuccess;
    if (a.n_cameras > kProgramMarchCameras) return hipErrorInvalidValue;
    const uint32_t tiles_x = (a.f.width + 15) / 16, tiles_y = (a.y1 - a.y0 + 15) / 16;
    if (tiles_y > 65535u) return hipErrorInvalidValue;
    hipLaunchKernelGGL(a.aux ? sdfprog_march_aux : sdfprog_march, dim3(tiles_x, tiles_y, a.n_cameras), dim3(kBlock), 0, stream, a);
    return hipGetLastError();
}

}  // namespace sdfv
