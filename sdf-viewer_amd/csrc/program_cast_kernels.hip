// program_cast_kernels.hip -- a caller's list of rays cast against an SDF program on gfx950 (program_cast.h): one ray per lane,
// rays in list order, 256-thread workgroups, a 64-bit ray index.
//
// Shape: the march loop is the wave loop of the direct march (program_march_kernels.hip) around the wave-uniform instruction
// stream -- per step every marching lane runs the whole program once, instructions arrive by scalar loads (program_eval.h),
// finished lanes are masked out and the wave leaves when none is left; a wave whose rays all miss the box leaves before it
// touches the program.  All per-lane state is in registers: no LDS, no scratch.  The only vector memory traffic is the ray coming
// in (32 bytes: two 16-byte loads when the array is 16-byte aligned, eight dword loads otherwise) and the record going out (64
// bytes: four 16-byte streaming stores, or sixteen dword stores) -- it is written once and never re-read here.  The loop is
// bounded by max_steps <= 4096 runs of at most 256 instructions: it cannot hang.
//
// The kernel stands outside SDFV_PROGRAM_KERNELS (program_kernels.h): the cast is no compiled route, a handle from
// sdfv_program_compile is interpreted here like any other.
#include "program_cast_kernels.h"

#include "kernel_common.h"

namespace sdfv {

namespace {
typedef float v4f __attribute__((ext_vector_type(4)));

// The workgroup's 256 rays and records start at a wave-uniform 64-bit base (rays, hits: scalar registers); a lane adds its
// 32-bit thread index, the only index it keeps across the march.
__device__ __forceinline__ sdfv_ray load_ray(const sdfv_ray* rays, uint32_t lane, bool aligned16) {
    sdfv_ray r;
    if (aligned16) {
        const v4f* q = reinterpret_cast<const v4f*>(rays + lane);
        const v4f lo = q[0], hi = q[1];
        r.origin[0] = lo.x; r.origin[1] = lo.y; r.origin[2] = lo.z; r.t_min = lo.w;
        r.dir[0] = hi.x; r.dir[1] = hi.y; r.dir[2] = hi.z; r.t_max = hi.w;
    } else {
        r = rays[lane];
    }
    return r;
}

__device__ __forceinline__ void store_hit(sdfv_ray_hit* hits, uint32_t lane, bool aligned16, const sdfv_ray_hit& h) {
    if (aligned16) {
        v4f* q = reinterpret_cast<v4f*>(hits + lane);
        const v4f q0 = {__int_as_float(h.status), __int_as_float(h.steps), h.t, h.pos[0]};
        const v4f q1 = {h.pos[1], h.pos[2], h.normal[0], h.normal[1]};
        const v4f q2 = {h.normal[2], h.sample.distance, h.sample.color[0], h.sample.color[1]};
        const v4f q3 = {h.sample.color[2], h.sample.metallic, h.sample.roughness, h.sample.occlusion};
        __builtin_nontemporal_store(q0, q);
        __builtin_nontemporal_store(q1, q + 1);
        __builtin_nontemporal_store(q2, q + 2);
        __builtin_nontemporal_store(q3, q + 3);
    } else {
        hits[lane] = h;
    }
}
}  // namespace

extern "C" __global__ __launch_bounds__(kBlock) void sdfprog_cast(ProgramCastArgs a) {
    const uint64_t base = a.first + (uint64_t)blockIdx.x * kBlock;  // < a.n: the launcher counts the workgroups
    const uint64_t left = a.n - base;
    const uint32_t count = left < (uint64_t)kBlock ? (uint32_t)left : (uint32_t)kBlock;
    const uint32_t lane = threadIdx.x;
    const bool live = lane < count;
    sdfv_ray ray;
    ray.origin[0] = ray.origin[1] = ray.origin[2] = ray.t_min = 0.0f;
    ray.dir[0] = ray.dir[1] = ray.dir[2] = ray.t_max = 0.0f;
    if (live) ray = load_ray(a.rays + base, lane, a.rays16 != 0);
    sdfv_ray_hit hit;
    pcast::cast_ray_program(a.c, prog::Interpreter{a.c.ops, a.c.n_ops}, ray, live, hit);
    if (live) store_hit(a.hits + base, lane, a.hits16 != 0, hit);
}

hipError_t launch_program_cast(const ProgramCastArgs& args, hipStream_t stream) {
    ProgramCastArgs a = args;
    constexpr uint64_t kMaxBlocks = 0x7fffffffull;  // of one launch; a longer list takes several
    for (a.first = 0; a.first < a.n; a.first += kMaxBlocks * kBlock) {
        const uint64_t left = a.n - a.first;
        const uint64_t blocks = left / kBlock + (left % kBlock != 0);
        void* params[] = {&a};
        const hipError_t e = hipLaunchKernel((const void*)sdfprog_cast, dim3((uint32_t)(blocks < kMaxBlocks ? blocks : kMaxBlocks)),
                                             dim3(kBlock), params, 0, stream);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace sdfv
