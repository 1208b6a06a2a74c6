// program_pass_kernels.hip -- one LoadingManager pass with an SDF program as the SDF (sdfv_program_grid_pass): the progressive
// load and the changed-box edit of a caller's own model, on gfx950.
//
// update_required (scene/sdf/mod.rs:184-190) is "the voxel holds AIR_DIST, or its position lies inside the changed box".
// voxel_coord is non-decreasing in the index on every axis, so the second half is a product of three index ranges on the pass
// lattice, which the caller computes once per call (ProgramPassArgs' sub-box).  That splits a pass into two launches with
// nothing to decide per voxel:
//  * sdfprog_pass_box: threads map onto the lattice points of the sub-box only, x fastest ACROSS the sub-box -- a wave spans
//    as many short rows as it takes to be full.  No box compare, no load (but tex1.a where there is no volume to vouch for it):
//    the interpreter once per lane, resolve + pack_sample, 16-byte streamed stores.  The rows' (y, z) coordinates -- two IEEE
//    divides each -- are staged per row in LDS by the workgroup's first lanes, as the flat dense fill stages them;
//  * sdfprog_pass_scan: the lattice points outside the sub-box.  One load of the volume (or of tex0.r) per lane; a wave that
//    finds no AIR_DIST leaves after that load (sdfprog_pass_scan_nt: a nontemporal one), otherwise the rare lanes that did run the interpreter under their mask.
// In both the instruction stream is wave-uniform (program_eval.h): scalar loads, no vector memory operation in the loop.
#include "program_pass_kernels.h"

#include "kernel_common.h"
#include "program_eval.h"
#include "program_resolve.h"

namespace sdfv {

namespace {

// The rewrite of one lattice voxel (the demo's pass_store with the interpreter as the SDF): the texel pair the dense program
// fill writes, stored as every pass stores (pass_store_texels).
template <typename Lut>
__device__ __forceinline__ void program_pass_store(const ProgramPassArgs& a, const Lut& lut, float px, float py, float pz, uint64_t row,
                                                   uint32_t x) {
    const Sample s = resolve(a.ops, prog::run(a.ops, a.n_ops, px, py, pz), false);
    float4 v0, v1;
    if (a.srgb_round) pack_sample<true>(s, lut, a.air_dist, v0, v1);
    else pack_sample<false>(s, lut, a.air_dist, v0, v1);
    pass_store_texels(a, a.dist, row, x, v0, v1);
}

// STREAM: the one load is nontemporal (a template policy like store_texel's: as a run-time choice the two loads are merged
// into one plain load).
template <bool STREAM>
__device__ __forceinline__ void program_pass_scan(const ProgramPassArgs& a) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;  // (no wrap: the grid covers a.n <= 2^32 points)
    if ((uint64_t)i >= a.n) return;
    const uint32_t r = div_u32(i, a.div_x), ix = i - r * a.nx;
    const uint32_t iz = div_u32(r, a.div_y), iy = r - iz * a.ny;
    // the sub-box is the box launch's (unsigned wrap: one compare per axis); its voxels are not even read here
    if (ix - a.bx0 < a.bnx && iy - a.by0 < a.bny && iz - a.bz0 < a.bnz) return;
    const uint32_t x = ix * a.step, y = iy * a.step, z = a.z_first + iz * a.step;  // global z
    const uint64_t row = (uint64_t)(z - a.z_begin) * a.H + y;
    const float* stored = a.dist ? a.dist + vol_index(a.dist_ilv, row, (uint64_t)x, a.W) : &a.tex0[row * a.W + x].x;
    const float held = STREAM ? load_once(stored) : *stored;
    if (held != a.air_dist) return;  // a wave of a loaded grid ends here, on its one load
    program_pass_store(a, LdsLut{c_srgb_lut}, voxel_coord(x, a.dm1[0], a.bb_size[0], a.bb_min[0]),
                       voxel_coord(y, a.dm1[1], a.bb_size[1], a.bb_min[1]), voxel_coord(z, a.dm1[2], a.bb_size[2], a.bb_min[2]), row, x);
}

}  // namespace

extern "C" {

__global__ __launch_bounds__(kBlock) void sdfprog_pass_box(ProgramPassArgs a) {
    __shared__ float s_lut[256];
    __shared__ float2 s_yz[kBlock + 1];  // the (y, z) coordinates of the sub-box rows this workgroup touches ...
    __shared__ uint2 s_at[kBlock + 1];   // ... and their voxel y and LOCAL slice
    const uint32_t tid = threadIdx.x;
    const uint32_t t0 = blockIdx.x * kBlock;  // < a.n <= 2^32: the launcher's grid
    const uint32_t t_last = (uint32_t)min((uint64_t)t0 + kBlock - 1, a.n - 1);
    const uint32_t row_first = div_u32(t0, a.div_x);  // sub-box row = bz * bny + by
    const uint32_t n_rows_here = div_u32(t_last, a.div_x) - row_first + 1;  // <= kBlock (bnx == 1: one row per thread)
    const LdsLut lut = stage_srgb_lut(s_lut);
    for (uint32_t r = tid; r < n_rows_here; r += kBlock) {
        const uint32_t br = row_first + r, bz = div_u32(br, a.div_y), by = br - bz * a.bny;
        const uint32_t y = (a.by0 + by) * a.step, z = a.z_first + (a.bz0 + bz) * a.step;
        s_yz[r] = make_float2(voxel_coord(y, a.dm1[1], a.bb_size[1], a.bb_min[1]), voxel_coord(z, a.dm1[2], a.bb_size[2], a.bb_min[2]));
        s_at[r] = make_uint2(y, z - a.z_begin);
    }
    __syncthreads();
    if ((uint64_t)t0 + tid >= a.n) return;
    const uint32_t t = t0 + tid;
    const uint32_t br = div_u32(t, a.div_x), bx = t - br * a.bnx;
    const uint32_t x = (a.bx0 + bx) * a.step;
    const float2 yz = s_yz[br - row_first];
    const uint2 at = s_at[br - row_first];
    program_pass_store(a, lut, voxel_coord(x, a.dm1[0], a.bb_size[0], a.bb_min[0]), yz.x, yz.y, (uint64_t)at.y * a.H + at.x, x);
}

__global__ __launch_bounds__(kBlock) void sdfprog_pass_scan(ProgramPassArgs a) { program_pass_scan<false>(a); }
__global__ __launch_bounds__(kBlock) void sdfprog_pass_scan_nt(ProgramPassArgs a) { program_pass_scan<true>(a); }

}  // extern "C"

namespace {
bool lattice_in_slab(const ProgramPassArgs& a) {
    return a.step >= 1 && (uint64_t)(a.nx - 1) * a.step < a.W && (uint64_t)(a.ny - 1) * a.step < a.H && a.z_first >= a.z_begin &&
           (uint64_t)(a.z_first - a.z_begin) + (uint64_t)(a.nz - 1) * a.step < a.slab_d;
}
}  // namespace

hipError_t launch_program_pass_box(const ProgramPassArgs& args, hipStream_t stream) {
    ProgramPassArgs a = args;
    a.n = (uint64_t)a.bnx * a.bny * a.bnz;
    if (a.n == 0) return hipSuccess;
    // the sub-box lies on the lattice, the lattice in the slab: no store can leave the textures
    if ((uint64_t)a.bx0 + a.bnx > a.nx || (uint64_t)a.by0 + a.bny > a.ny || (uint64_t)a.bz0 + a.bnz > a.nz || !lattice_in_slab(a))
        return hipErrorInvalidValue;
    if (a.dist == nullptr) a.dist_ilv = 0;
    const uint32_t blocks = blocks_for(a.n, 1ull << 32);  // the kernel's 32-bit index covers 2^32 points
    if (!blocks) return hipErrorInvalidValue;
    a.div_x = make_div(a.bnx);
    a.div_y = make_div(a.bny);
    hipLaunchKernelGGL(sdfprog_pass_box, dim3(blocks), dim3(kBlock), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_program_pass_scan(const ProgramPassArgs& args, hipStream_t stream) {
    ProgramPassArgs a = args;
    a.n = (uint64_t)a.nx * a.ny * a.nz;
    if (a.n == 0) return hipSuccess;
    if (!lattice_in_slab(a)) return hipErrorInvalidValue;
    if (a.dist == nullptr) a.dist_ilv = 0;
    const uint32_t blocks = blocks_for(a.n, 1ull << 32);  // the kernel's 32-bit index covers 2^32 points
    if (!blocks) return hipErrorInvalidValue;
    a.div_x = make_div(a.nx);
    a.div_y = make_div(a.ny);
    hipLaunchKernelGGL(a.stream_loads ? sdfprog_pass_scan_nt : sdfprog_pass_scan, dim3(blocks), dim3(kBlock), 0, stream, a);
    return hipGetLastError();
}

}  // namespace sdfv
