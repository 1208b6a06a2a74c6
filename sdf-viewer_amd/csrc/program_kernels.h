// program_kernels.h -- launch interface of the SDF-program kernels (see program_kernels.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#if !defined(__HIPCC_RTC__)
#include <atomic>
#endif

#if defined(__HIPCC_RTC__)  // the run-time compiler is handed the headers by name (program_compile.hip)
#include "sdfgrid.h"
#else
#include "../../include/sdfgrid.h"
#endif

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

// The kernels a program is evaluated by on the routes sdfv_program_compile covers, in the order a compiled handle keeps its
// specialised ones (program_compile.hip holds their names in this order).
enum ProgramKernel {
    kKernelFillTx64, kKernelFillTx64Nt, kKernelFillTx128, kKernelFillTx128Nt, kKernelFillTx256, kKernelFillTx256Nt,
    kKernelPoints, kKernelPointsStaged, kKernelMarch, kKernelMarchAux,
    // SDFV_COMPILE_MESH (program_mesh_kernels.hip, sparse_mesh_kernels.hip)
    kKernelMeshLattice, kKernelMeshVertices, kKernelMeshVerticesMat, kKernelNormalPoints, kKernelNormalPointsStaged,
    kKernelMeshPostproc, kKernelMeshPostprocUnaligned, kKernelSparseRefine, kKernelSparseBricks, kProgramKernels
};

#if !defined(__HIPCC_RTC__)
// What a compiled handle gives a launcher for the current device: its specialised kernels (nullptr where the route was not
// compiled) and the counter of their launches.  A launcher given none launches the interpreter's kernel; the checks and the
// launch geometry are computed before that choice, so the two cannot accept different calls.
struct ProgramKernels {
    const hipFunction_t* fn = nullptr;  // kProgramKernels entries, or nullptr: a plain handle, or a route that interprets
    std::atomic<uint64_t>* launches = nullptr;  // sdfv_compiled_info::launches of that handle
    // kernel `which` over `args` (one address per kernel argument) if it is there; *mine says whether it was
    hipError_t launch(ProgramKernel which, dim3 grid, dim3 block, void** args, hipStream_t stream, bool* mine) const {
        *mine = fn && fn[which];
        if (!*mine) return hipSuccess;
        const hipError_t e = hipModuleLaunchKernel(fn[which], grid.x, grid.y, grid.z, block.x, block.y, block.z, 0, stream, args, nullptr);
        if (e == hipSuccess) launches->fetch_add(1, std::memory_order_relaxed);
        return e;
    }
};

hipError_t launch_program_fill(const ProgramFillArgs& a, const ProgramKernels& k, hipStream_t stream);
hipError_t launch_program_sample_points(const sdfv_prog_op* ops, uint32_t n_ops, const float* points, size_t n,
                                        bool distance_only, sdfv_sample* out, const ProgramKernels& k, hipStream_t stream);
#endif

}  // namespace sdfv
