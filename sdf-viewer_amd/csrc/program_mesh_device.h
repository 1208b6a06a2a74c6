// program_mesh_device.h -- the bodies of the mesh pipeline's SDF-program kernels, each over an EVALUATOR (program_eval.h), as
// program_device.h has the fill's, the samplers' and the march's: the lattice, the vertex phase, the batched normal,
// Mesh::postproc (program_mesh_kernels.hip) and the two evaluating kernels of the sparse route (sparse_mesh_kernels.hip).  hipcc
// instantiates them with the interpreter; the translation unit that sdfv_program_compile generates for SDFV_COMPILE_MESH
// (program_compile.hip) includes this very text and instantiates it with the evaluator of one program.  The nine kernels
// themselves are stated at the end, once each, as definitions over the two evaluator expressions.  Parameters, index
// arithmetic, masks and stores are the same code either way, which is why the two take the same arguments and give the same bits.
#pragma once

#include "kernel_common.h"
#include "mesh_lattice.h"
#include "program_eval.h"
#include "program_resolve.h"
#include "sparse_mesh_kernels.h"

namespace sdfv {

__device__ __forceinline__ bool wave_any(bool b) { return __ballot(b) != 0ull; }

// normal_default_impl (defaults.rs:49-56) of the program at p -> (nx, ny, nz), per lane, written for a WAVE: under the lanes
// with `taps`, left alone under the others, skipped by the wave when no lane wants it.  The operation sequence is
// demo_normal(..., use_default = true) of demo_sdf_device.h with the program's distance in the demo's place:
// e = eps > 0 ? eps : 0.001; taps at p + (e, -e, -e), (-e, e, -e), (-e, -e, e), (e, e, e), a coordinate being p + k * e with
// k = 1.0f or -1.0f (k * e is exact); sums left to right in tap order, the first term standing alone (d1 + -d2 + -d3 + d4 for
// x; a term is k * d, exact); normalize3.
// The four runs go through ONE copy of the evaluator: a loop that is not unrolled, as program_march.h does for its taps.  Only
// the distance of a run is used, so this copy carries no material indices (the compiler drops them: 56 VGPRs for a bare run of
// the interpreter, as in sdfprog_mesh_lattice, against 72 with them).
template <typename Eval>
__device__ __forceinline__ void tap_normal(const Eval& eval, float px, float py, float pz, float eps, bool taps, float& nx,
                                           float& ny, float& nz) {
    if (!wave_any(taps)) return;
    const float e = eps > 0.0f ? eps : 0.001f;
    float ax = 0.0f, ay = 0.0f, az = 0.0f;
#pragma unroll 1
    for (int t = 0; t < 4; ++t) {
        if (taps) {
            const float kx = (t == 0 || t == 3) ? 1.0f : -1.0f;
            const float ky = (t == 1 || t == 3) ? 1.0f : -1.0f;
            const float kz = (t == 2 || t == 3) ? 1.0f : -1.0f;
            const float d = eval(px + kx * e, py + ky * e, pz + kz * e).d;
            ax = t == 0 ? kx * d : ax + kx * d;
            ay = t == 0 ? ky * d : ay + ky * d;
            az = t == 0 ? kz * d : az + kz * d;
        }
    }
    if (taps) normalize3(ax, ay, az, nx, ny, nz);
}

// The material fields of sample(p, false) under the lanes with `live`: a fifth, full run (this one does carry the material
// index) + resolve() over the device copy of the instructions -- raw fields, not packed, not clamped.  It comes BEFORE the taps
// in every kernel below: a run with material indices needs 72 VGPRs by itself under the interpreter, and after it only the six
// fields (or the two that share a store with the normal) stay live across the cheaper taps -- the other way round the normal
// and the point would have to survive the expensive run.
template <typename Eval>
__device__ __forceinline__ Mat material_at(const Eval& eval, const sdfv_prog_op* __restrict__ ops, float px, float py, float pz,
                                           bool live) {
    prog::Value v;
    v.d = 0.0f;
    v.m = prog::kNoMaterial;
    if (live) v = eval(px, py, pz);
    return resolve(ops, v, false).m;
}

// TapEval: the evaluator of the four taps; Eval: the one of the material run (the same program, possibly another copy of it).
template <bool MAT, typename Eval, typename TapEval>
__device__ __forceinline__ void mesh_vertices(const Eval& eval, const TapEval& tap_eval, const sdfv_prog_op* __restrict__ ops,
                                              float4* __restrict__ vertices, uint32_t n) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    const bool live = i < n;
    float4* v = vertices + (size_t)(live ? i : 0) * 3;
    float4 p = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (live) p = v[0];  // the position (w: not yet written, not used)
    // the 48-byte record leaves as three 16-byte stores: {b, metallic, roughness, occlusion} as soon as it is known
    Mat m = zero_mat();  // without MAT: Vertex::default()'s zero material
    if (MAT) m = material_at(eval, ops, p.x, p.y, p.z, live);
    if (live) v[2] = make_float4(m.b, m.metallic, m.roughness, m.occlusion);
    float nx = 0.0f, ny = 0.0f, nz = 0.0f;
    tap_normal(tap_eval, p.x, p.y, p.z, 0.0f, live, nx, ny, nz);
    if (live) {
        v[0] = make_float4(p.x, p.y, p.z, nx);
        v[1] = make_float4(ny, nz, m.r, m.g);
    }
}

// The batched normal as the element map's evaluator (kernel_common.h): a point in, the normal there out.  EVERY lane goes into
// tap_normal, the lanes beyond n (whose point is zero) under its mask: the evaluator's loop is the wave's.
template <typename Eval>
struct ProgramNormalEval {
    Eval eval;
    float eps;
    __device__ __forceinline__ void operator()(float* v, bool live) const {
        float nx = 0.0f, ny = 0.0f, nz = 0.0f;
        tap_normal(eval, v[0], v[1], v[2], eps, live, nx, ny, nz);
        v[0] = nx; v[1] = ny; v[2] = nz;
    }
};

// One lattice point per thread, x fastest: the distance alone.
template <typename Eval>
__device__ __forceinline__ void mesh_lattice_points(const Eval& eval, const MeshGrid& g, float* __restrict__ dist) {
    const Lattice L(g);
    const uint32_t v = blockIdx.x * kBlock + threadIdx.x;
    if (v >= L.points()) return;
    uint32_t i, j, k;
    L.unflat(v, i, j, k);
    float px, py, pz;
    lattice_position(g, i, j, k, px, py, pz);
    dist[v] = eval(px, py, pz).d;
}

// Mesh::postproc over 16-byte aligned vertices: 16-byte accesses.  A kept normal goes back as it was read.
template <typename Eval, typename TapEval>
__device__ __forceinline__ void mesh_postproc_aligned(const Eval& eval, const TapEval& tap_eval, const sdfv_prog_op* __restrict__ ops,
                                                      float4* __restrict__ vertices, size_t n) {
    const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    const bool live = i < n;
    float4* v = vertices + (live ? i : 0) * 3;
    float4 a = make_float4(0.0f, 0.0f, 0.0f, 1.0f), b = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (live) {
        a = v[0];
        b = v[1];
    }
    const Mat m = material_at(eval, ops, a.x, a.y, a.z, live);
    if (live) v[2] = make_float4(m.b, m.metallic, m.roughness, m.occlusion);
    float nx = a.w, ny = b.x, nz = b.y;
    const bool taps = live && normal_unset(nx, ny, nz);
    tap_normal(tap_eval, a.x, a.y, a.z, 0.0f, taps, nx, ny, nz);
    if (taps) v[0] = make_float4(a.x, a.y, a.z, nx);
    if (live) v[1] = make_float4(ny, nz, m.r, m.g);
}

// ... over any 4-byte aligned vertex array: dword accesses; position and a kept normal are not written.
template <typename Eval, typename TapEval>
__device__ __forceinline__ void mesh_postproc_words(const Eval& eval, const TapEval& tap_eval, const sdfv_prog_op* __restrict__ ops,
                                                    float* __restrict__ vertices, size_t n) {
    const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    const bool live = i < n;
    float* v = vertices + (live ? i : 0) * 12;
    float px = 0.0f, py = 0.0f, pz = 0.0f, nx = 1.0f, ny = 0.0f, nz = 0.0f;
    if (live) {
        px = v[0]; py = v[1]; pz = v[2];
        nx = v[3]; ny = v[4]; nz = v[5];
    }
    const Mat m = material_at(eval, ops, px, py, pz, live);
    if (live) {
        v[6] = m.r; v[7] = m.g; v[8] = m.b;
        v[9] = m.metallic; v[10] = m.roughness; v[11] = m.occlusion;
    }
    const bool taps = live && normal_unset(nx, ny, nz);
    tap_normal(tap_eval, px, py, pz, 0.0f, taps, nx, ny, nz);
    if (taps) {
        v[3] = nx; v[4] = ny; v[5] = nz;
    }
}

// ---- the sparse route: blocks are Morton keys in units of their own side, x the lowest bit ----
constexpr uint32_t kSparseKept = 0x80000000u;  // a candidate's flag in SparseWork::cand

// every third bit of a Morton key -> a 10-bit coordinate
__device__ __forceinline__ uint32_t gather3(uint32_t x) {
    x &= 0x09249249u;
    x = (x ^ (x >> 2)) & 0x030c30c3u;
    x = (x ^ (x >> 4)) & 0x0300f00fu;
    x = (x ^ (x >> 8)) & 0x030000ffu;
    x = (x ^ (x >> 16)) & 0x000003ffu;
    return x;
}

// thread t of a brick-major array of 125 per brick -> the brick and the local point (x fastest)
__device__ __forceinline__ void unbrick(uint32_t t, uint32_t& b, uint32_t& lx, uint32_t& ly, uint32_t& lz) {
    b = t / kBrickPoints;
    const uint32_t l = t - b * kBrickPoints;
    lz = l / 25u;
    const uint32_t r = l - lz * 25u;
    ly = r / 5u;
    lx = r - ly * 5u;
}

// One CHILD block per thread (8 per block of the list): the distance at its centre lattice point, kept iff !(|d| > threshold).
template <typename Eval>
__device__ __forceinline__ void sparse_refine_children(const Eval& eval, const MeshGrid& g, const uint32_t* __restrict__ parents,
                                                       uint32_t n, uint32_t shift, float threshold, uint32_t* __restrict__ cand,
                                                       uint32_t* __restrict__ pos) {
    const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
    if (t >= n) return;
    const uint32_t key = parents[t >> 3] * 8u + (t & 7u);
    const uint32_t half = (1u << shift) >> 1;  // the centre lattice point: o + s / 2
    float px, py, pz;
    lattice_position(g, (gather3(key) << shift) + half, (gather3(key >> 1) << shift) + half, (gather3(key >> 2) << shift) + half,
                     px, py, pz);
    const float d = eval(px, py, pz).d;
    const bool keep = !(fabsf(d) > threshold);  // a NaN distance keeps the block
    cand[t] = key | (keep ? kSparseKept : 0u);
    pos[t] = keep ? 1u : 0u;
}

// Thread t has lattice point t % 125 of brick t / 125: the distances, brick-major.
template <typename Eval>
__device__ __forceinline__ void sparse_brick_points(const Eval& eval, const MeshGrid& g, const uint32_t* __restrict__ bricks,
                                                    uint32_t n, float* __restrict__ dist) {
    const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
    if (t >= n) return;
    uint32_t b, lx, ly, lz;
    unbrick(t, b, lx, ly, lz);
    const uint32_t key = bricks[b];
    float px, py, pz;
    lattice_position(g, gather3(key) * 4u + lx, gather3(key >> 1) * 4u + ly, gather3(key >> 2) * 4u + lz, px, py, pz);
    dist[t] = eval(px, py, pz).d;
}

}  // namespace sdfv

// ---- the kernels of SDFV_COMPILE_MESH: SDFV_PROGRAM_KERNEL_<stem>(name) over SDFV_EVAL_ONCE / SDFV_EVAL_LOOPED, as in
// program_device.h.  The four taps sit in tap_normal's loop, which is not unrolled: one copy of the evaluator, the looped one
// (a compiled program keeps its operands from being hoisted out of that loop, as in the march); the material run and the
// lattices stand outside any loop. ----
#define SDFV_PROGRAM_KERNEL_mesh_lattice(name)                                                                                \
    extern "C" __global__ __launch_bounds__(kBlock) void name(const sdfv_prog_op* __restrict__ ops, uint32_t n_ops, MeshGrid g, \
                                                              float* __restrict__ dist) {                                    \
        mesh_lattice_points(SDFV_EVAL_ONCE(ops, n_ops), g, dist);                                                             \
    }
#define SDFV_PROGRAM_KERNEL_MESH_VERTICES(name, MAT)                                                                         \
    extern "C" __global__ __launch_bounds__(kBlock) void name(const sdfv_prog_op* __restrict__ ops, uint32_t n_ops,          \
                                                              float4* __restrict__ vertices, uint32_t n) {                   \
        mesh_vertices<MAT>(SDFV_EVAL_ONCE(ops, n_ops), SDFV_EVAL_LOOPED(ops, n_ops), ops, vertices, n);                       \
    }
#define SDFV_PROGRAM_KERNEL_mesh_vertices(name) SDFV_PROGRAM_KERNEL_MESH_VERTICES(name, false)
#define SDFV_PROGRAM_KERNEL_mesh_vertices_mat(name) SDFV_PROGRAM_KERNEL_MESH_VERTICES(name, true)
#define SDFV_PROGRAM_KERNEL_normal_points(name)                                                                              \
    extern "C" __global__ __launch_bounds__(kBlock) void name(const sdfv_prog_op* __restrict__ ops, uint32_t n_ops,          \
                                                              const float* __restrict__ points, size_t first, size_t n,      \
                                                              float eps, float* __restrict__ out) {                          \
        auto tap = SDFV_EVAL_LOOPED(ops, n_ops);                                                                              \
        map_elements<3, 3>(ProgramNormalEval<decltype(tap)>{tap, eps}, points, first, n, out);                                \
    }
#define SDFV_PROGRAM_KERNEL_normal_points_staged(name)                                                                       \
    extern "C" __global__ __launch_bounds__(kBlock) void name(const sdfv_prog_op* __restrict__ ops, uint32_t n_ops,          \
                                                              const float4* __restrict__ points, float eps,                  \
                                                              float4* __restrict__ out) {                                    \
        auto tap = SDFV_EVAL_LOOPED(ops, n_ops);                                                                              \
        map_elements_staged<3, 3>(ProgramNormalEval<decltype(tap)>{tap, eps}, points, out);                                   \
    }
#define SDFV_PROGRAM_KERNEL_mesh_postproc(name)                                                                              \
    extern "C" __global__ __launch_bounds__(kBlock) void name(const sdfv_prog_op* __restrict__ ops, uint32_t n_ops,          \
                                                              float4* __restrict__ vertices, size_t n) {                     \
        mesh_postproc_aligned(SDFV_EVAL_ONCE(ops, n_ops), SDFV_EVAL_LOOPED(ops, n_ops), ops, vertices, n);                    \
    }
#define SDFV_PROGRAM_KERNEL_mesh_postproc_unaligned(name)                                                                    \
    extern "C" __global__ __launch_bounds__(kBlock) void name(const sdfv_prog_op* __restrict__ ops, uint32_t n_ops,          \
                                                              float* __restrict__ vertices, size_t n) {                      \
        mesh_postproc_words(SDFV_EVAL_ONCE(ops, n_ops), SDFV_EVAL_LOOPED(ops, n_ops), ops, vertices, n);                      \
    }
#define SDFV_PROGRAM_KERNEL_sparse_refine(name)                                                                              \
    extern "C" __global__ __launch_bounds__(kBlock) void name(const sdfv_prog_op* __restrict__ ops, uint32_t n_ops, MeshGrid g, \
                                                              const uint32_t* __restrict__ parents, uint32_t n, uint32_t shift, \
                                                              float threshold, uint32_t* __restrict__ cand,                  \
                                                              uint32_t* __restrict__ pos) {                                  \
        sparse_refine_children(SDFV_EVAL_ONCE(ops, n_ops), g, parents, n, shift, threshold, cand, pos);                       \
    }
#define SDFV_PROGRAM_KERNEL_sparse_bricks(name)                                                                              \
    extern "C" __global__ __launch_bounds__(kBlock) void name(const sdfv_prog_op* __restrict__ ops, uint32_t n_ops, MeshGrid g, \
                                                              const uint32_t* __restrict__ bricks, uint32_t n,               \
                                                              float* __restrict__ dist) {                                    \
        sparse_brick_points(SDFV_EVAL_ONCE(ops, n_ops), g, bricks, n, dist);                                                  \
    }
