// kernel_common.h -- what the SDF kernels share on the device: the small helpers every .hip file used to restate, the
// 28-byte sample record, the LDS staging of arrays of structures, the store of one voxel a pass rewrites (pass_store_texels),
// the block-count rule of every launcher (blocks_for), and the skeletons that are instantiated once per way of evaluating
// an SDF (the demo tree of demo_sdf_device.h, the interpreter of program_eval.h):
//  * dense_fill_rows: the dense row-chunk fill (fill_dense_kernel and the sdfprog_fill_* kernels);
//  * map_elements / map_elements_staged: IN words per element in, OUT words out (the samplers, the batched normals, the
//    source scalars and the demo's Mesh::postproc).
// An evaluator is a small object of wave-uniform state: for the fill `void operator()(px, py, pz, lut, air_dist, t0, t1)`
// writes the two texels, for the element map `void operator()(float* v, bool live)` turns an element into its result in
// place.  Everything here is __forceinline__ and takes its arguments by reference: a kernel built from these pieces is the
// kernel that spelled them out.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "demo_sdf_device.h"
#include "fill_kernels.h"

namespace sdfv {

constexpr int kBlock = 256;

typedef float v4f __attribute__((ext_vector_type(4)));

namespace {
// sRGB u8 -> linear (colour passes through u8, scene/sdf/mod.rs:201).  A table per translation unit: the library is built
// without -fgpu-rdc.
__constant__ float c_srgb_lut[256] = {
#include "srgb_lut.inc"
};
}  // namespace

struct LdsLut {
    const float* p;
    __device__ __forceinline__ float operator[](uint32_t i) const { return p[i]; }
};

// The table into a workgroup's LDS, one entry per thread (kBlock = 256 = its length); readable after the next barrier.
__device__ __forceinline__ LdsLut stage_srgb_lut(float* s_lut) {
    s_lut[threadIdx.x] = c_srgb_lut[threadIdx.x];
    return LdsLut{s_lut};
}

template <bool NT>
__device__ __forceinline__ void store_texel(float4* dst, const float4& v) {
    // global_store_dwordx4 ... nt: write-once stream, nothing re-reads it from L2.  (A template policy: as a run-time branch
    // the two stores are merged into one plain store.)
    if (NT) {
        v4f t = {v.x, v.y, v.z, v.w};
        __builtin_nontemporal_store(t, reinterpret_cast<v4f*>(dst));
    } else {
        *dst = v;
    }
}

// A load of data this kernel looks at ONCE (the distance volume under a pass's update_required test, tex0 under a commit):
// nontemporal -- global_load ... nt does not allocate in L2 / the Infinity Cache, so a scan that follows a fill does not have to
// push the fill's dirty lines out of the way first.  tools/ubench/read_stream.hip, 512 MiB read once behind 1 GiB of stores:
// plain loads 0.128 ms (4.2 TB/s), nt loads 0.080 ms (6.7 TB/s); eight reads in a row: 6.7 vs 7.0 TB/s.  The step-1 no-op pass
// of a loaded 512^3 grid went 0.144 -> see EXPERIMENTS R6.2.
__device__ __forceinline__ float4 load_once(const float4* p) {
    const v4f t = __builtin_nontemporal_load(reinterpret_cast<const v4f*>(p));
    return make_float4(t.x, t.y, t.z, t.w);
}
__device__ __forceinline__ float load_once(const float* p) { return __builtin_nontemporal_load(p); }

// Entry of the distance volume for voxel x of slab row `row` (= z_local * H + y) in either layout (FillArgs::dist_ilv).
// Index = the caller's index type: 64 bits in the fills, 32 where the whole grid is indexed with 32.
template <typename Index, typename X>
__device__ __forceinline__ Index vol_index(uint32_t ilv, Index row, X x, uint32_t W) {
    return ilv ? ((row >> 1) * W + x) * 2 + (row & 1) : row * W + x;
}

// The rewrite of voxel x of slab row `row` by a LoadingManager pass: the texel pair (v0, v1) an evaluation gave, and the
// entry of the distance volume `vol` (nullptr = the grid has none).  Args = FillArgs or ProgramPassArgs.
template <typename Args>
__device__ __forceinline__ void pass_store_texels(const Args& a, float* vol, uint64_t row, uint32_t x, const float4& v0, float4 v1) {
    const uint64_t flat = row * a.W + x;
    // Texture stores stream past L2 (nt), like the fused dense fill's: nothing re-reads them before the march's few texels
    // under the hits, while the volume -- which this very pass READS -- keeps the cache.  tools/ubench/rw_mix.hip: a
    // 4 B/voxel read stream next to the 36 B/voxel store stream costs 0.108 ms with plain stores and 0.094 with nt at 256^3.
    store_texel<true>(a.tex0 + flat, v0);
    if (vol) {
        // The volume's contract: the textures were initialised / filled by this library, so tex1.a holds AIR_DIST
        // everywhere (update() never writes it, scene/sdf/mod.rs:205-208) and need not be read back.
        vol[vol_index(a.dist_ilv, row, (uint64_t)x, a.W)] = v0.x;
        v1.w = a.air_dist;
    } else {
        // tex1.a is not update()'s to touch: carry the stored value through a full 16-byte store (12-byte partial
        // stores make the memory side read-modify-write the line; ~10 % slower on the step-1 pass)
        v1.w = reinterpret_cast<const float*>(a.tex1 + flat)[3];
    }
    store_texel<true>(a.tex1 + flat, v1);
}

// The (y, z) coordinates of slab row `row` (= z_local * H + y): an IEEE
// divide per axis, so once per row (through LDS) instead of once per voxel.
template <typename Args>
__device__ __forceinline__ float2 stage_row_yz(const Args& a, uint32_t row) {
    const uint32_t zl = row / a.H, y = row - zl * a.H;
    return make_float2(voxel_coord(y, a.dm1[1], a.bb_size[1], a.bb_min[1]),
                       voxel_coord(a.z_begin + zl, a.dm1[2], a.bb_size[2], a.bb_min[2]));
}

// "This launch has started" = everything enqueued before it on its stream has finished: the multi-GPU fill step lets the
// communicator's stream wait on this word (hipStreamWaitValue32) instead of on an event recorded before the fill.
__device__ __forceinline__ void signal_launch_started(const FillArgs& a) {
    if (a.signal && blockIdx.x == 0 && threadIdx.x == 0)
        __hip_atomic_store(a.signal, a.signal_value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// ---- #[repr(C)] SDFSample, 28 bytes = 7 floats ----
__device__ __forceinline__ void write_record(float* o, const Sample& s) {
    o[0] = s.distance;
    o[1] = s.m.r; o[2] = s.m.g; o[3] = s.m.b;
    o[4] = s.m.metallic; o[5] = s.m.roughness; o[6] = s.m.occlusion;
}
__device__ __forceinline__ Sample read_record(const float* r) {
    Sample s;
    s.distance = r[0];
    s.m.r = r[1]; s.m.g = r[2]; s.m.b = r[3];
    s.m.metallic = r[4]; s.m.roughness = r[5]; s.m.occlusion = r[6];
    return s;
}

// ---- arrays of structures through LDS ----
// Workgroup b's kBlock elements of K dwords each are kBlock * K / 4 contiguous dwordx4: they cross global memory as such,
// streamed (nt: the read stream and the store stream get along better when they pass L2 by, EXPERIMENTS R3.4), and are
// re-sliced per element in LDS (strides of 3, 7 and 12 dwords are conflict-free or nearly so).  `lds` is 16-byte aligned and
// holds kBlock * K floats, `global` is the array's base; the caller places the barriers.
template <int K>
__device__ __forceinline__ void tile_load(float* lds, const float4* global) {
    constexpr int kVec = kBlock * K / 4;
    const size_t tile = (size_t)blockIdx.x * kVec;
    const uint32_t t = threadIdx.x;
#pragma unroll
    for (int r = 0; r < kVec; r += kBlock)  // whole rounds, then the lanes of the partial one
        if (kVec - r >= kBlock || t < kVec - r)
            reinterpret_cast<v4f*>(lds)[r + t] = __builtin_nontemporal_load(reinterpret_cast<const v4f*>(global) + tile + r + t);
}
template <int K>
__device__ __forceinline__ void tile_store(float4* global, const float* lds) {
    constexpr int kVec = kBlock * K / 4;
    const size_t tile = (size_t)blockIdx.x * kVec;
    const uint32_t t = threadIdx.x;
#pragma unroll
    for (int r = 0; r < kVec; r += kBlock)
        if (kVec - r >= kBlock || t < kVec - r)
            __builtin_nontemporal_store(reinterpret_cast<const v4f*>(lds)[r + t], reinterpret_cast<v4f*>(global) + tile + r + t);
}

// ---- the element map: n elements of IN words in, OUT words out, one thread per element ----
// Every per-element kernel over caller arrays (samples, normals, source scalars, Mesh::postproc; the demo tree's and the
// program's) is one of these two calls around an evaluator `void operator()(float* v, bool live)`: v[0 .. IN) holds the
// element, the evaluator leaves the result in v[0 .. OUT), and words [SKIP, OUT) of it are written.  `live` is false under
// the lanes beyond n, whose v is zero: an evaluator either leaves them at once or, where its loop is the wave's (the
// interpreter), runs them under the mask.  The element is read whole before anything is written: in == out is allowed.
// Scalar form: any 4-byte alignment, any n -- element first + workgroup * kBlock + thread; it also finishes what the staged
// form leaves over (launch_staged_then_tail).
template <int IN, int OUT, int SKIP = 0, typename Eval>
__device__ __forceinline__ void map_elements(const Eval& eval, const float* in, size_t first, size_t n, float* out) {
    const size_t i = first + (size_t)blockIdx.x * kBlock + threadIdx.x;
    const bool live = i < n;
    float v[IN > OUT ? IN : OUT] = {};
    if (live)
        for (int k = 0; k < IN; ++k) v[k] = in[i * IN + k];
    eval(v, live);
    if (live)
        for (int k = SKIP; k < OUT; ++k) out[i * OUT + k] = v[k];
}

// Staged form: WHOLE workgroups of kBlock elements through 16-byte aligned arrays, and nothing else -- per-lane accesses to
// an array of structures would be IN and OUT dword operations at an IN * 4 / OUT * 4-byte stride, so a workgroup's tile goes
// through tile_load / tile_store instead.  The way out follows from the sizes: OUT == IN -- the result goes back into the
// thread's own words of the input tile (no barrier in between), which is stored whole; OUT == 1 -- the 4-byte results are
// coalesced as they are, one streamed dword per lane; otherwise a second tile.
template <int OUT>
using StagedOut = std::conditional_t<OUT == 1, float, float4>;
template <int IN, int OUT, int SKIP = 0, typename Eval>
__device__ __forceinline__ void map_elements_staged(const Eval& eval, const float4* in, StagedOut<OUT>* out) {
    __shared__ __attribute__((aligned(16))) float s_in[kBlock * IN];
    const uint32_t t = threadIdx.x;
    tile_load<IN>(s_in, in);
    __syncthreads();
    float v[IN > OUT ? IN : OUT];
    for (int k = 0; k < IN; ++k) v[k] = s_in[t * IN + k];
    eval(v, true);
    if constexpr (OUT == 1) {
        __builtin_nontemporal_store(v[0], out + (size_t)blockIdx.x * kBlock + t);
    } else if constexpr (OUT == IN) {
        for (int k = SKIP; k < OUT; ++k) s_in[t * OUT + k] = v[k];
        __syncthreads();
        tile_store<OUT>(out, s_in);
    } else {
        __shared__ __attribute__((aligned(16))) float s_out[kBlock * OUT];
        for (int k = SKIP; k < OUT; ++k) s_out[t * OUT + k] = v[k];
        __syncthreads();
        tile_store<OUT>(out, s_out);
    }
}

// Mesh::postproc's rule (meshers/mesh.rs:22-33): the normal is recomputed where the mesher left |n|^2 < 1e-4 (distance2 to the
// zero vector).
__device__ __forceinline__ bool normal_unset(float nx, float ny, float nz) {
    const float dx = nx - 0.0f, dy = ny - 0.0f, dz = nz - 0.0f;
    return dx * dx + dy * dy + dz * dz < 0.0001f;
}

// ---- the dense row-chunk fill ----
// Boundary-first order (FillArgs::order_*): logical workgroup `b` of a launch -> the workgroup of the memory-order grid whose
// voxels it fills.  The first order_lead * bps workgroups are the slab's leading slices, the next bps its LAST slice, then the
// interior in memory order.  All operands are wave-uniform (SGPRs).
struct OrderedBlock {
    uint32_t block;     // memory-order workgroup index
    bool boundary;      // one of the slices a z-neighbour waits for
    bool last_slice;    // ... the slab's last one (goes to the upper neighbour)
};
__device__ __forceinline__ OrderedBlock ordered_block(const FillArgs& a, uint32_t b) {
    OrderedBlock r;
    const uint32_t lead = a.order_lead * a.order_bps;
    r.boundary = b < lead + a.order_bps;
    r.last_slice = r.boundary && b >= lead;
    r.block = r.last_slice ? (a.slab_d - 1) * a.order_bps + (b - lead) : (r.boundary ? b : b - a.order_bps);
    return r;
}

// The boundary workgroups' packed copies (one message per neighbour and direction instead of one per texture).
__device__ __forceinline__ void store_staged(const FillArgs& a, const OrderedBlock& ob, uint64_t o, const float4& v0,
                                             const float4& v1) {
    const uint64_t slice = (uint64_t)a.W * a.H;
    float4 *d0 = nullptr, *d1 = nullptr;
    if (ob.last_slice) {
        if (a.stage_hi) {
            const uint64_t w = o - (uint64_t)(a.slab_d - 1) * slice;
            d0 = a.stage_hi + w;
            d1 = a.stage_hi + slice + w;
        }
    } else if (a.stage_lo) {
        d0 = a.stage_lo + o;  // o < order_lead * slice
        d1 = a.stage_lo + a.order_lead * slice + o;
    }
    if (!d0) return;
    *d0 = v0;
    *d1 = v1;
}

// TX = lanes along x per row segment (64, 128 or 256); a workgroup owns TY = 256 / TX consecutive rows x TX voxels and does
// ONE voxel per thread, x fastest, so a 64-lane wave emits two contiguous 1 KiB bursts (tex0, tex1) of global_store_dwordx4
// and the grid walks memory front to back in dispatch order exactly like a memset.  Measured on MI355X
// (profiles/r01/v1_fill_sweep.json, r01/v2_fill_sweep.json): persistent strided workgroups lose 25-40 % of the store rate
// and 2/4/8 rows per thread lose 7/11/14 %.  No global loads beyond the table: the position derives from the index.
// Args = FillArgs or ProgramFillArgs (the fields both carry under the same names); ORDERED (FillArgs only) = boundary-first
// order with its packed copies.
template <int TX, bool NT, bool ORDERED, typename Args, typename Eval>
__device__ __forceinline__ void dense_fill_rows(const Args& a, const Eval& eval) {
    constexpr int TY = kBlock / TX;
    __shared__ float s_lut[256];
    __shared__ float2 s_yz[TY];

    const uint32_t tid = threadIdx.x;
    const uint32_t n_rows = a.H * a.slab_d;  // rows of the slab: row = z_local * H + y
    OrderedBlock ob{blockIdx.x, false, false};
    if constexpr (ORDERED) ob = ordered_block(a, blockIdx.x + a.block_base);
    // 1-D grid, x-chunk fastest: workgroup id -> (row group, x chunk); both uniform (SGPRs)
    const uint32_t row_group = a.x_chunks == 1 ? ob.block : ob.block / a.x_chunks;
    const uint32_t chunk = ob.block - row_group * a.x_chunks;
    const uint32_t row0 = row_group * TY;
    const LdsLut lut = stage_srgb_lut(s_lut);
    if (tid < TY && row0 + tid < n_rows) s_yz[tid] = stage_row_yz(a, row0 + tid);
    __syncthreads();

    const uint32_t tx = tid % TX, ty = tid / TX;
    const uint32_t x = chunk * TX + tx;
    const uint32_t row = row0 + ty;
    const bool in_range = ORDERED || (x < a.W && row < n_rows);  // ordered launches cover whole workgroups only
    const bool ilv = !ORDERED && TY >= 2 && a.dist_ilv;          // block-uniform; the launcher picks TY >= 2 for this layout
    if (!ilv && !in_range) return;
    float4 v0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), v1 = v0;
    const uint64_t o = (uint64_t)row * a.W + x;
    bool stores = true;
    if constexpr (ORDERED) stores = !a.stage_only;
    if (in_range) {
        const float px = voxel_coord(x, a.dm1[0], a.bb_size[0], a.bb_min[0]);
        const float2 yz = s_yz[ty];
        eval(px, yz.x, yz.y, lut, a.air_dist, v0, v1);
        if (stores) {
            store_texel<NT>(a.tex0 + o, v0);
            store_texel<NT>(a.tex1 + o, v1);
            if (a.dist && !ilv) a.dist[o] = v0.x;  // wave-uniform: +4 B/voxel instead of a second pass over tex0
        }
    }
    if (ilv) {
        // y-interleaved volume: rows 2p and 2p + 1 of this workgroup meet in LDS and leave as ONE row of pairs -- 8-byte
        // stores, whole lines, from the workgroup that computed both (two workgroups writing the halves of a line would make
        // the memory side merge partial lines).  row0 is even (TY even), and so is the slab's row count (H even).
        __shared__ float s_d[kBlock];
        s_d[tid] = v0.x;
        __syncthreads();
        if ((ty & 1u) == 0 && in_range)
            reinterpret_cast<float2*>(a.dist)[(uint64_t)(row >> 1) * a.W + x] = make_float2(s_d[tid], s_d[tid + TX]);
    }
    if constexpr (ORDERED)
        if (ob.boundary) store_staged(a, ob, o, v0, v1);  // wave-uniform
}

// The demo tree as the fill's evaluator: fill_voxel<Cfg> over the parameter block in the kernel arguments (SGPRs).
template <typename Cfg>
struct DemoFillEval {
    const sdfv_demo_params& prm;
    uint32_t sdf_id;
    __device__ __forceinline__ void operator()(float px, float py, float pz, const LdsLut& lut, float air_dist, float4& t0,
                                               float4& t1) const {
        fill_voxel<Cfg>(prm, sdf_id, px, py, pz, lut, air_dist, t0, t1);
    }
};

// ---- how many workgroups, and is that launchable ----
// A launch takes 2^31 - 1 workgroups at the most: here a 64-bit count of them becomes a grid, or 0 = not launchable.
inline uint32_t grid_size(uint64_t blocks) { return blocks > 0x7fffffffull ? 0u : (uint32_t)blocks; }
// n >= 1 elements, one per thread: ceil(n / kBlock) workgroups.  A kernel that indexes its elements with 32 bits names the
// largest n it can take as well.  0 = refuse with hipErrorInvalidValue; where the caller has held n to 32 bits already
// (MeshGrid::launchable(), a uint32_t kernel argument) it goes straight into the launch, which takes no empty grid.
inline uint32_t blocks_for(uint64_t n, uint64_t max_n = ~0ull) { return n > max_n ? 0u : grid_size(n / kBlock + (n % kBlock != 0)); }

// n elements through a kernel with a staged form: whole workgroups of kBlock through `staged(whole)` if `aligned` (the
// pointers allow 16-byte accesses), the rest -- [done, n) -- through `scalar(blocks, done)`, which takes any alignment.
// An n that needs more workgroups than one launch takes is refused before anything is launched, whatever the alignment.
#if !defined(__HIPCC_RTC__)  // (host only: the run-time compiler reads this header for the device code)
template <typename Staged, typename Scalar>
hipError_t launch_staged_then_tail(size_t n, bool aligned, Staged&& staged, Scalar&& scalar) {
    if (n == 0) return hipSuccess;
    const uint32_t all = blocks_for(n);
    if (!all) return hipErrorInvalidValue;
    const uint32_t whole = aligned ? (uint32_t)(n / kBlock) : 0u;  // <= all
    const size_t done = (size_t)whole * kBlock;
    if (whole > 0) staged(whole);
    if (done < n) scalar(all - whole, done);
    return hipGetLastError();
}
#endif

}  // namespace sdfv
