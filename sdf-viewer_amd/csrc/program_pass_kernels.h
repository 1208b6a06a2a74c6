// program_pass_kernels.h -- launch interface of the SDF-program pass kernels (see program_pass_kernels.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fill_kernels.h"

namespace sdfv {

// One LoadingManager pass with a program as the SDF.  The pass lattice: voxels whose x, y and GLOBAL z are multiples of
// `step`, nx * ny * nz of them in this slab, lattice point (ix, iy, iz) = voxel (ix * step, iy * step, z_first + iz * step).
// "Inside the changed box" is a product of three index ranges on that lattice (voxel_coord is monotone in the index): the
// SUB-BOX [bx0, bx0 + bnx) x [by0, by0 + bny) x [bz0, bz0 + bnz), made by the caller from the kernels' own coordinates.
struct ProgramPassArgs {
    const sdfv_prog_op* ops;  // DEVICE copy of the validated program
    uint32_t n_ops;
    uint32_t W, H;            // global width and height
    uint32_t z_begin;         // first global slice held by tex0 / tex1
    uint32_t slab_d;          // slices held
    float dm1[3];             // (float)dim - 1.0f          (scene/sdf/mod.rs:168)
    float bb_size[3];         // bb[1] - bb[0]              (scene/sdf/mod.rs:167)
    float bb_min[3];
    float air_dist;
    float4* tex0;
    float4* tex1;
    float* dist;              // optional distance volume: read for update_required, rewritten with the texels
    uint32_t dist_ilv;        // its layout (fill_kernels.h FillArgs::dist_ilv)
    uint32_t srgb_round;      // SDFV_OPT_EXT_SRGB_QUANT
    uint32_t step;
    uint32_t nx, ny, nz;      // lattice points per axis in this slab
    uint32_t z_first;         // first visited GLOBAL z (multiple of step, >= z_begin)
    uint32_t bx0, by0, bz0;   // the sub-box, in lattice indices ...
    uint32_t bnx, bny, bnz;   // ... and its extents (any of them 0: empty)
    uint32_t stream_loads;    // the scan reads the volume / tex0.r with nontemporal loads (picks sdfprog_pass_scan_nt)
    // set by the launchers:
    uint64_t n;               // lattice points of the launch: bnx * bny * bnz (box), nx * ny * nz (scan); at most 2^32
    DivU32 div_x, div_y;      // by (bnx, bny) in the box launch, by (nx, ny) in the scan
};

// Every lattice point of the sub-box gets the program's texel pair; nothing is read but tex1.a when there is no volume.
hipError_t launch_program_pass_box(const ProgramPassArgs& a, hipStream_t stream);
// The lattice points OUTSIDE the sub-box that hold AIR_DIST get the program's texel pair; everything else is left alone.
hipError_t launch_program_pass_scan(const ProgramPassArgs& a, hipStream_t stream);

}  // namespace sdfv
