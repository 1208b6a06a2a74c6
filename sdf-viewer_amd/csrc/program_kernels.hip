// program_kernels.hip -- SDF programs on gfx950: the dense grid fill and the batched point sampler for a caller-defined CSG
// tree (include/sdfgrid.h, "SDF programs").
//
// Both kernels are the skeletons of kernel_common.h -- the ones the demo's kernels are built from -- with the interpreter of
// program_eval.h as the evaluator (the definitions are program_device.h's, shared with the kernels a compiled handle brings):
//  * sdfprog_fill_tx{64,128,256}[_nt]: dense_fill_rows -- one voxel per thread, x fastest, the sRGB table and the rows' (y, z)
//    coordinates in LDS, pack_sample() for the texels, 16-byte stores front to back, the distance volume in either layout
//    from the same launch.  The store policy stays a template parameter;
//  * sdfprog_sample_points{,_staged}: map_elements{,_staged}<3, 7> -- points in, 28-byte records out.
// The instruction stream is read through wave-uniform addresses: scalar loads, no vector memory traffic per instruction, and
// no kernel arguments beyond a pointer and a count (the handle owns a device copy of the instructions).
// The kernels carry C names: tests and profiles find them under the same symbol whatever the toolchain mangles.
#include "program_kernels.h"

#include "program_device.h"

namespace sdfv {

// the interpreter as both evaluators of the kernel definitions (program_device.h)
#define SDFV_EVAL_ONCE(ops, n_ops) prog::Interpreter{ops, n_ops}
#define SDFV_EVAL_LOOPED(ops, n_ops) prog::Interpreter{ops, n_ops}

SDFV_PROGRAM_KERNEL_fill_tx64(sdfprog_fill_tx64)
SDFV_PROGRAM_KERNEL_fill_tx64_nt(sdfprog_fill_tx64_nt)
SDFV_PROGRAM_KERNEL_fill_tx128(sdfprog_fill_tx128)
SDFV_PROGRAM_KERNEL_fill_tx128_nt(sdfprog_fill_tx128_nt)
SDFV_PROGRAM_KERNEL_fill_tx256(sdfprog_fill_tx256)
SDFV_PROGRAM_KERNEL_fill_tx256_nt(sdfprog_fill_tx256_nt)
SDFV_PROGRAM_KERNEL_sample_points(sdfprog_sample_points)
SDFV_PROGRAM_KERNEL_sample_points_staged(sdfprog_sample_points_staged)

hipError_t launch_program_fill(const ProgramFillArgs& args, const ProgramKernels& k, hipStream_t stream) {
    if (args.W == 0 || args.H == 0 || args.slab_d == 0) return hipSuccess;
    ProgramFillArgs a = args;
    if (a.dist == nullptr) a.dist_ilv = 0;
    if (a.dist_ilv && ((a.H & 1u) || ((uintptr_t)a.dist & 7))) return hipErrorInvalidValue;
    // the interleaved volume leaves from workgroups that hold both rows of a pair: two or four rows per workgroup
    const uint32_t tx = a.W <= 64 ? 64u : ((a.W <= 128 || a.dist_ilv) ? 128u : 256u);
    const uint32_t ty = kBlock / tx;
    a.x_chunks = (a.W + tx - 1) / tx;
    const uint64_t n_rows = (uint64_t)a.H * a.slab_d;
    const uint32_t blocks = grid_size((uint64_t)a.x_chunks * ((n_rows + ty - 1) / ty));  // (the rows fit: check_one_launch)
    if (!blocks) return hipErrorInvalidValue;
    const int which = (tx == 64 ? kKernelFillTx64 : (tx == 128 ? kKernelFillTx128 : kKernelFillTx256)) + (a.nontemporal ? 1 : 0);
    static const void* const kernels[] = {(const void*)sdfprog_fill_tx64,  (const void*)sdfprog_fill_tx64_nt,
                                          (const void*)sdfprog_fill_tx128, (const void*)sdfprog_fill_tx128_nt,
                                          (const void*)sdfprog_fill_tx256, (const void*)sdfprog_fill_tx256_nt};  // by `which`
    void* params[] = {&a};
    return k.launch((ProgramKernel)which, kernels[which - kKernelFillTx64], dim3(blocks), dim3(kBlock), params, stream);
}

hipError_t launch_program_sample_points(const sdfv_prog_op* ops, uint32_t n_ops, const float* points, size_t n,
                                        bool distance_only, sdfv_sample* out, const ProgramKernels& k, hipStream_t stream) {
    float* o = reinterpret_cast<float*>(out);
    hipError_t first = hipSuccess;  // of the launches
    const hipError_t e = launch_staged_then_tail(
        n, (((uintptr_t)points | (uintptr_t)out) & 15) == 0,
        [&](uint32_t whole) {
            const float4* in4 = reinterpret_cast<const float4*>(points);
            float4* out4 = reinterpret_cast<float4*>(o);
            void* params[] = {&ops, &n_ops, &in4, &distance_only, &out4};
            const hipError_t es = k.launch(kKernelPointsStaged, (const void*)sdfprog_sample_points_staged, dim3(whole), dim3(kBlock), params, stream);
            if (first == hipSuccess) first = es;
        },
        [&](uint32_t blocks, size_t done) {
            void* params[] = {&ops, &n_ops, &points, &done, &n, &distance_only, &o};
            const hipError_t es = k.launch(kKernelPoints, (const void*)sdfprog_sample_points, dim3(blocks), dim3(kBlock), params, stream);
            if (first == hipSuccess) first = es;
        });
    return first != hipSuccess ? first : e;
}

}  // namespace sdfv
