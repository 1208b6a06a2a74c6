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

// The kernels a program is evaluated by on the routes sdfv_program_compile covers, stated once: X(index, stem, route bit).
// The interpreter's kernel is sdfprog_<stem>, a compiled handle's sdfprogc_<stem>, both defined by SDFV_PROGRAM_KERNEL_<stem>
// (program_device.h, program_mesh_device.h); a handle keeps its kernels by index (CompiledProgram::Loaded::fn), so a new row goes
// at the end.  The enum below, the handle's name table and route_of() (program_compile.hip) and the kernels the generated
// translation unit defines all come from these rows and from nothing else.
#define SDFV_PROGRAM_KERNELS(X)                                            \
    X(kKernelFillTx64, fill_tx64, SDFV_COMPILE_FILL)                       \
    X(kKernelFillTx64Nt, fill_tx64_nt, SDFV_COMPILE_FILL)                  \
    X(kKernelFillTx128, fill_tx128, SDFV_COMPILE_FILL)                     \
    X(kKernelFillTx128Nt, fill_tx128_nt, SDFV_COMPILE_FILL)                \
    X(kKernelFillTx256, fill_tx256, SDFV_COMPILE_FILL)                     \
    X(kKernelFillTx256Nt, fill_tx256_nt, SDFV_COMPILE_FILL)                \
    X(kKernelPoints, sample_points, SDFV_COMPILE_POINTS)                   \
    X(kKernelPointsStaged, sample_points_staged, SDFV_COMPILE_POINTS)      \
    X(kKernelMarch, march, SDFV_COMPILE_MARCH)                             \
    X(kKernelMarchAux, march_aux, SDFV_COMPILE_MARCH)                      \
    X(kKernelMeshLattice, mesh_lattice, SDFV_COMPILE_MESH)                 \
    X(kKernelMeshVertices, mesh_vertices, SDFV_COMPILE_MESH)               \
    X(kKernelMeshVerticesMat, mesh_vertices_mat, SDFV_COMPILE_MESH)        \
    X(kKernelNormalPoints, normal_points, SDFV_COMPILE_MESH)               \
    X(kKernelNormalPointsStaged, normal_points_staged, SDFV_COMPILE_MESH)  \
    X(kKernelMeshPostproc, mesh_postproc, SDFV_COMPILE_MESH)               \
    X(kKernelMeshPostprocUnaligned, mesh_postproc_unaligned, SDFV_COMPILE_MESH) \
    X(kKernelSparseRefine, sparse_refine, SDFV_COMPILE_MESH)               \
    X(kKernelSparseBricks, sparse_bricks, SDFV_COMPILE_MESH)

enum ProgramKernel {
#define SDFV_X(index, stem, route) index,
    SDFV_PROGRAM_KERNELS(SDFV_X)
#undef SDFV_X
    kProgramKernels
};
static_assert(kProgramKernels == 19 && kKernelSparseBricks == 18, "a handle's kernels are kept by index: rows are added at the end");

#if !defined(__HIPCC_RTC__)
// What a compiled handle gives a launcher for the current device: its specialised kernels (nullptr where the route was not
// compiled) and the counter of their launches.  The checks and the launch geometry are computed before launch() chooses, so the
// two kernels of a pair cannot accept different calls.
struct ProgramKernels {
    const hipFunction_t* fn = nullptr;  // kProgramKernels entries, or nullptr: a plain handle, or a route that interprets
    std::atomic<uint64_t>* launches = nullptr;  // sdfv_compiled_info::launches of that handle
    // The handle's kernel `which` if it is there (counted), the interpreter's kernel `interpreted` (sdfprog_<stem>) otherwise,
    // over the same `args`: one address per kernel argument, the two having one parameter list (SDFV_PROGRAM_KERNEL_<stem>).
    hipError_t launch(ProgramKernel which, const void* interpreted, dim3 grid, dim3 block, void** args, hipStream_t stream) const {
        if (!fn || !fn[which]) return hipLaunchKernel(interpreted, grid, block, args, 0, stream);
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
