// program_kernels.hip -- SDF programs on gfx950: the dense grid fill and the batched point sampler for a caller-defined CSG
// tree (include/sdfgrid.h, "SDF programs").
//
// Both kernels are the demo's kernels with the SDF evaluation replaced by the interpreter of program_eval.h:
//  * sdfprog_fill_tx{64,128,256}[_nt]: the skeleton of fill_dense_kernel (fill_kernels.hip) -- one voxel per thread, x fastest, the
//    sRGB table and the rows' (y, z) coordinates in LDS, pack_sample() for the texels, 16-byte stores front to back, the
//    distance volume in either layout from the same launch.  The Srgba::from policy is a wave-uniform branch here (the
//    interpreter loop is the body: six kernels instead of twelve); the store policy stays a template parameter;
//  * sdfprog_sample_points{,_staged}: points in, 28-byte records out, as sample_points{,_staged}_kernel (points_kernels.hip).
// The instruction stream is read through wave-uniform addresses: scalar loads, no vector memory traffic per instruction, and
// no kernel arguments beyond a pointer and a count (the handle owns a device copy of the instructions).
// The kernels carry C names: tests and profiles find them under the same symbol whatever the toolchain mangles.
#include "program_kernels.h"

#include "demo_sdf_device.h"
#include "program_eval.h"

namespace sdfv {

namespace {

__constant__ float c_program_srgb_lut[256] = {  // (a table per translation unit: the library is built without -fgpu-rdc)
#include "srgb_lut.inc"
};

constexpr int kBlock = 256;

typedef float v4f __attribute__((ext_vector_type(4)));

struct LdsLut {
    const float* p;
    __device__ __forceinline__ float operator[](uint32_t i) const { return p[i]; }
};

// The result's material: the six operands of the MATERIAL instruction the value carries.  The index differs between lanes,
// the instruction memory is read by scalar loads only: one round per DISTINCT index among the wave's lanes (a wave of
// neighbouring voxels sees one to three materials).
__device__ __forceinline__ Sample resolve(const sdfv_prog_op* __restrict__ ops, const prog::Value& v, bool distance_only) {
    Sample s;
    s.distance = v.d;
    s.m = zero_mat();
    bool pending = !distance_only && v.m != prog::kNoMaterial;
    while (pending) {
        if (v.m == (uint32_t)__builtin_amdgcn_readfirstlane(v.m)) {
            // (read again under the narrowed EXEC: the compiler forwards the equality into this block, and an index it takes
            // for the per-lane v.m would turn the fetch into a vector load)
            const float* a = ops[__builtin_amdgcn_readfirstlane(v.m)].a;
            s.m.r = a[0]; s.m.g = a[1]; s.m.b = a[2];
            s.m.metallic = a[3]; s.m.roughness = a[4]; s.m.occlusion = a[5];
            pending = false;
        }
    }
    return s;
}

template <bool NT>
__device__ __forceinline__ void store_texel(float4* dst, const float4& v) {
    if (NT) {  // (a template policy: as a run-time branch the two stores are merged into one plain store)
        v4f t = {v.x, v.y, v.z, v.w};
        __builtin_nontemporal_store(t, reinterpret_cast<v4f*>(dst));
    } else {
        *dst = v;
    }
}

template <int TX, bool NT>
__device__ __forceinline__ void program_fill(const ProgramFillArgs& a) {
    constexpr int TY = kBlock / TX;
    __shared__ float s_lut[256];
    __shared__ float2 s_yz[TY];

    const uint32_t tid = threadIdx.x;
    const uint32_t n_rows = a.H * a.slab_d;  // rows of the slab: row = z_local * H + y
    const uint32_t row_group = a.x_chunks == 1 ? blockIdx.x : blockIdx.x / a.x_chunks;
    const uint32_t chunk = blockIdx.x - row_group * a.x_chunks;
    const uint32_t row0 = row_group * TY;
    s_lut[tid] = c_program_srgb_lut[tid];
    if (tid < TY && row0 + tid < n_rows) {
        const uint32_t row = row0 + tid;
        const uint32_t zl = row / a.H, y = row - zl * a.H;
        s_yz[tid] = make_float2(voxel_coord(y, a.dm1[1], a.bb_size[1], a.bb_min[1]),
                                voxel_coord(a.z_begin + zl, a.dm1[2], a.bb_size[2], a.bb_min[2]));
    }
    __syncthreads();

    const LdsLut lut{s_lut};
    const uint32_t tx = tid % TX, ty = tid / TX;
    const uint32_t x = chunk * TX + tx;
    const uint32_t row = row0 + ty;
    const bool in_range = x < a.W && row < n_rows;
    const bool ilv = TY >= 2 && a.dist_ilv;  // block-uniform; the launcher picks TY >= 2 for this layout
    if (!ilv && !in_range) return;
    float4 v0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), v1 = v0;
    const uint64_t o = (uint64_t)row * a.W + x;
    if (in_range) {
        const float px = voxel_coord(x, a.dm1[0], a.bb_size[0], a.bb_min[0]);
        const float2 yz = s_yz[ty];
        const Sample s = resolve(a.ops, prog::run(a.ops, a.n_ops, px, yz.x, yz.y), false);
        if (a.srgb_round) pack_sample<true>(s, lut, a.air_dist, v0, v1);
        else pack_sample<false>(s, lut, a.air_dist, v0, v1);
        store_texel<NT>(a.tex0 + o, v0);
        store_texel<NT>(a.tex1 + o, v1);
        if (a.dist && !ilv) a.dist[o] = v0.x;
    }
    if (TY >= 2 && ilv) {
        // y-interleaved volume: rows 2p and 2p + 1 of this workgroup meet in LDS and leave as one row of pairs (row0 is even
        // because TY is, and so is the slab's row count because H is)
        __shared__ float s_d[kBlock];
        s_d[tid] = v0.x;
        __syncthreads();
        if ((ty & 1u) == 0 && in_range)
            reinterpret_cast<float2*>(a.dist)[(uint64_t)(row >> 1) * a.W + x] = make_float2(s_d[tid], s_d[tid + TX]);
    }
}

__device__ __forceinline__ void write_record(float* o, const Sample& s) {
    o[0] = s.distance;
    o[1] = s.m.r; o[2] = s.m.g; o[3] = s.m.b;
    o[4] = s.m.metallic; o[5] = s.m.roughness; o[6] = s.m.occlusion;
}

}  // namespace

extern "C" {

__global__ __launch_bounds__(kBlock) void sdfprog_fill_tx64(ProgramFillArgs a) { program_fill<64, false>(a); }
__global__ __launch_bounds__(kBlock) void sdfprog_fill_tx64_nt(ProgramFillArgs a) { program_fill<64, true>(a); }
__global__ __launch_bounds__(kBlock) void sdfprog_fill_tx128(ProgramFillArgs a) { program_fill<128, false>(a); }
__global__ __launch_bounds__(kBlock) void sdfprog_fill_tx128_nt(ProgramFillArgs a) { program_fill<128, true>(a); }
__global__ __launch_bounds__(kBlock) void sdfprog_fill_tx256(ProgramFillArgs a) { program_fill<256, false>(a); }
__global__ __launch_bounds__(kBlock) void sdfprog_fill_tx256_nt(ProgramFillArgs a) { program_fill<256, true>(a); }

// Scalar form: any alignment, any n (also finishes the last partial workgroup of the staged form).
__global__ __launch_bounds__(kBlock) void sdfprog_sample_points(const sdfv_prog_op* __restrict__ ops, uint32_t n_ops,
                                                                const float* __restrict__ points, size_t first, size_t n,
                                                                bool distance_only, float* __restrict__ out) {
    const size_t i = first + (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const float px = points[i * 3 + 0], py = points[i * 3 + 1], pz = points[i * 3 + 2];
    write_record(out + i * 7, resolve(ops, prog::run(ops, n_ops, px, py, pz), distance_only));
}

// Staged form for whole workgroups of 256 points: 3 KiB in and 7 KiB out cross global memory as dwordx4 and are re-sliced per
// point in LDS (strides of 3 and 7 dwords are conflict-free).
__global__ __launch_bounds__(kBlock) void sdfprog_sample_points_staged(const sdfv_prog_op* __restrict__ ops, uint32_t n_ops,
                                                                       const float4* __restrict__ points, bool distance_only,
                                                                       float4* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) float s_in[kBlock * 3];
    __shared__ __attribute__((aligned(16))) float s_out[kBlock * 7];
    const uint32_t t = threadIdx.x;
    const size_t in4 = (size_t)blockIdx.x * (kBlock * 3 / 4), out4 = (size_t)blockIdx.x * (kBlock * 7 / 4);
    if (t < kBlock * 3 / 4) reinterpret_cast<v4f*>(s_in)[t] = __builtin_nontemporal_load(reinterpret_cast<const v4f*>(points) + in4 + t);
    __syncthreads();
    const float px = s_in[t * 3 + 0], py = s_in[t * 3 + 1], pz = s_in[t * 3 + 2];
    write_record(s_out + t * 7, resolve(ops, prog::run(ops, n_ops, px, py, pz), distance_only));
    __syncthreads();
    __builtin_nontemporal_store(reinterpret_cast<const v4f*>(s_out)[t], reinterpret_cast<v4f*>(out) + out4 + t);
    if (t < kBlock * 7 / 4 - kBlock)
        __builtin_nontemporal_store(reinterpret_cast<const v4f*>(s_out)[kBlock + t], reinterpret_cast<v4f*>(out) + out4 + kBlock + t);
}

}  // extern "C"

hipError_t launch_program_fill(const ProgramFillArgs& args, hipStream_t stream) {
    if (args.W == 0 || args.H == 0 || args.slab_d == 0) return hipSuccess;
    ProgramFillArgs a = args;
    if (a.dist == nullptr) a.dist_ilv = 0;
    if (a.dist_ilv && ((a.H & 1u) || ((uintptr_t)a.dist & 7))) return hipErrorInvalidValue;
    // the interleaved volume leaves from workgroups that hold both rows of a pair: two or four rows per workgroup
    const uint32_t tx = a.W <= 64 ? 64u : ((a.W <= 128 || a.dist_ilv) ? 128u : 256u);
    const uint32_t ty = kBlock / tx;
    a.x_chunks = (a.W + tx - 1) / tx;
    const uint64_t n_rows = (uint64_t)a.H * a.slab_d;
    const uint64_t blocks = (uint64_t)a.x_chunks * ((n_rows + ty - 1) / ty);
    if (n_rows > 0x7fffffffull || blocks > 0x7fffffffull) return hipErrorInvalidValue;
    auto kernel = a.nontemporal ? (tx == 64 ? sdfprog_fill_tx64_nt : (tx == 128 ? sdfprog_fill_tx128_nt : sdfprog_fill_tx256_nt))
                                : (tx == 64 ? sdfprog_fill_tx64 : (tx == 128 ? sdfprog_fill_tx128 : sdfprog_fill_tx256));
    hipLaunchKernelGGL(kernel, dim3((uint32_t)blocks), dim3(kBlock), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_program_sample_points(const sdfv_prog_op* ops, uint32_t n_ops, const float* points, size_t n,
                                        bool distance_only, sdfv_sample* out, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    float* o = reinterpret_cast<float*>(out);
    size_t done = 0;
    const size_t whole = n / kBlock;
    if (whole > 0 && whole <= 0x7fffffffull && (((uintptr_t)points | (uintptr_t)out) & 15) == 0) {
        hipLaunchKernelGGL(sdfprog_sample_points_staged, dim3((uint32_t)whole), dim3(kBlock), 0, stream, ops, n_ops,
                           reinterpret_cast<const float4*>(points), distance_only, reinterpret_cast<float4*>(o));
        done = whole * kBlock;
    }
    if (done < n) {
        const size_t blocks = (n - done + kBlock - 1) / kBlock;
        if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
        hipLaunchKernelGGL(sdfprog_sample_points, dim3((uint32_t)blocks), dim3(kBlock), 0, stream, ops, n_ops, points, done, n,
                           distance_only, o);
    }
    return hipGetLastError();
}

}  // namespace sdfv
