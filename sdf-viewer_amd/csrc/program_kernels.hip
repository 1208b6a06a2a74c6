// program_kernels.hip -- SDF programs on gfx950: the dense grid fill and the batched point sampler for a caller-defined CSG
// tree (include/sdfgrid.h, "SDF programs").
//
// Both kernels are the skeletons of kernel_common.h -- the ones the demo's kernels are built from -- with the interpreter of
// program_eval.h as the evaluator:
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

namespace {
using Interp = prog::Interpreter;
__device__ __forceinline__ ProgramFillEval<Interp> fill_eval(const ProgramFillArgs& a) { return ProgramFillEval<Interp>(a, Interp{a.ops, a.n_ops}); }
}  // namespace

extern "C" {

__global__ __launch_bounds__(kBlock) void sdfprog_fill_tx64(ProgramFillArgs a) { dense_fill_rows<64, false, false>(a, fill_eval(a)); }
__global__ __launch_bounds__(kBlock) void sdfprog_fill_tx64_nt(ProgramFillArgs a) { dense_fill_rows<64, true, false>(a, fill_eval(a)); }
__global__ __launch_bounds__(kBlock) void sdfprog_fill_tx128(ProgramFillArgs a) { dense_fill_rows<128, false, false>(a, fill_eval(a)); }
__global__ __launch_bounds__(kBlock) void sdfprog_fill_tx128_nt(ProgramFillArgs a) { dense_fill_rows<128, true, false>(a, fill_eval(a)); }
__global__ __launch_bounds__(kBlock) void sdfprog_fill_tx256(ProgramFillArgs a) { dense_fill_rows<256, false, false>(a, fill_eval(a)); }
__global__ __launch_bounds__(kBlock) void sdfprog_fill_tx256_nt(ProgramFillArgs a) { dense_fill_rows<256, true, false>(a, fill_eval(a)); }

__global__ __launch_bounds__(kBlock) void sdfprog_sample_points(const sdfv_prog_op* __restrict__ ops, uint32_t n_ops,
                                                                const float* __restrict__ points, size_t first, size_t n,
                                                                bool distance_only, float* __restrict__ out) {
    map_elements<3, 7>(ProgramSampleEval<Interp>{Interp{ops, n_ops}, ops, distance_only}, points, first, n, out);
}

__global__ __launch_bounds__(kBlock) void sdfprog_sample_points_staged(const sdfv_prog_op* __restrict__ ops, uint32_t n_ops,
                                                                       const float4* __restrict__ points, bool distance_only,
                                                                       float4* __restrict__ out) {
    map_elements_staged<3, 7>(ProgramSampleEval<Interp>{Interp{ops, n_ops}, ops, distance_only}, points, out);
}

}  // extern "C"

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
    void* params[] = {&a};
    bool mine = false;
    const hipError_t e = k.launch((ProgramKernel)which, dim3(blocks), dim3(kBlock), params, stream, &mine);
    if (mine) return e;
    auto kernel = a.nontemporal ? (tx == 64 ? sdfprog_fill_tx64_nt : (tx == 128 ? sdfprog_fill_tx128_nt : sdfprog_fill_tx256_nt))
                                : (tx == 64 ? sdfprog_fill_tx64 : (tx == 128 ? sdfprog_fill_tx128 : sdfprog_fill_tx256));
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(kBlock), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_program_sample_points(const sdfv_prog_op* ops, uint32_t n_ops, const float* points, size_t n,
                                        bool distance_only, sdfv_sample* out, const ProgramKernels& k, hipStream_t stream) {
    float* o = reinterpret_cast<float*>(out);
    hipError_t first = hipSuccess;  // of the specialised launches (the interpreter's report through hipGetLastError)
    bool mine = false;
    const hipError_t e = launch_staged_then_tail(
        n, (((uintptr_t)points | (uintptr_t)out) & 15) == 0,
        [&](uint32_t whole) {
            const float4* in4 = reinterpret_cast<const float4*>(points);
            float4* out4 = reinterpret_cast<float4*>(o);
            void* params[] = {&ops, &n_ops, &in4, &distance_only, &out4};
            const hipError_t es = k.launch(kKernelPointsStaged, dim3(whole), dim3(kBlock), params, stream, &mine);
            if (first == hipSuccess) first = es;
            if (mine) return;
            hipLaunchKernelGGL(sdfprog_sample_points_staged, dim3(whole), dim3(kBlock), 0, stream, ops, n_ops,
                               reinterpret_cast<const float4*>(points), distance_only, reinterpret_cast<float4*>(o));
        },
        [&](uint32_t blocks, size_t done) {
            void* params[] = {&ops, &n_ops, &points, &done, &n, &distance_only, &o};
            const hipError_t es = k.launch(kKernelPoints, dim3(blocks), dim3(kBlock), params, stream, &mine);
            if (first == hipSuccess) first = es;
            if (mine) return;
            hipLaunchKernelGGL(sdfprog_sample_points, dim3(blocks), dim3(kBlock), 0, stream, ops, n_ops, points, done, n,
                               distance_only, o);
        });
    return first != hipSuccess ? first : e;
}

}  // namespace sdfv
