// grid_mesh_kernels.hip -- meshing the grid a viewer has loaded (include/sdfgrid.h, "Meshing a loaded grid"; grid_mesh_kernels.h
// has the rules), on gfx950: the lattice of distances out of the grid's storage, and the per-vertex material out of its texels.
//
// Shape.
//  * grid_lattice_copy / _volume / _tex0: one thread per lattice point, x fastest, one kernel per source so that the choice
//    costs nothing in the loop.  _copy is lod 1 over the plain volume, where the lattice IS the volume: the flat index serves
//    both sides and the kernel is a streaming copy with a subtraction.  _volume takes either layout of the volume (vol_index,
//    wave-uniform) and any lod, _tex0 reads the r channel at a 16-byte stride.  The source is read once (load_once: it does not
//    push the lattice out of the cache); the lattice is read next, by the count, so it is stored normally.
//  * grid_vertex_materials, grid_normals_materials: one thread per VERTEX of the compacted list, as lattice_normals.  The two
//    texels are plain loads (of the 12 live bytes each, as the compiler narrows them): the lanes of a wave are neighbours on
//    the surface and share lines of the textures no more than they share voxels, so two 32-byte sectors per vertex is what
//    the gather costs.
//  * The sRGB table is inverted by an 8-step search of the table itself in LDS (stage_srgb_lut, one entry per thread):
//    idx = the number of entries < x is what a lower-bound search computes, so the result is the rule's by construction, for
//    every float, NaN included (every comparison fails: 0).  A closed-form guess would put a powf and a fix-up against the same
//    table in its place -- more instructions than the 8 LDS reads, and one more rounding argument to keep.  The three channels'
//    searches are independent and interleave (and share their first probe): 22 ds_read_b32 per vertex next to two gathers
//    from HBM.
// Every float step is one rounded f32 operation (the translation unit is built with -ffp-contract=off).
// The kernels carry C names: tests and profiles find them under the same symbol whatever the toolchain mangles.
#include "grid_mesh_kernels.h"

#include "kernel_common.h"
#include "lattice_vertex.h"
#include "mesh_lattice.h"

namespace sdfv {

namespace {

enum GridSource { kCopy, kVolume, kTex0 };

template <GridSource SRC>
__device__ __forceinline__ void unpack_point(const GridTexels& t, const MeshGrid& g, float* __restrict__ lattice) {
    const Lattice L(g);
    const uint32_t point = blockIdx.x * kBlock + threadIdx.x;
    if (point >= L.points()) return;
    float s;
    if (SRC == kCopy) {
        s = load_once(t.vol + point);
    } else {
        uint32_t i, j, k;
        L.unflat(point, i, j, k);
        const uint64_t x = (uint64_t)i * t.lod, row = ((uint64_t)k * t.lod) * t.H + (uint64_t)j * t.lod;
        if (SRC == kVolume)
            s = load_once(t.vol + vol_index(t.ilv, row, x, t.W));
        else
            s = load_once(reinterpret_cast<const float*>(t.tex0 + (row * t.W + x)));
    }
    lattice[point] = s - 0.1f;
}

// The number of table entries < x, at the most 255: a lower bound over 256 entries in 8 steps.  Invariant: `idx` entries are
// known to be < x; lut[idx + step - 1] < x shows that idx + step are (the table increases).
__device__ __forceinline__ float srgb_index(const LdsLut& lut, float x) {
    uint32_t idx = 0;
#pragma unroll
    for (uint32_t step = 128u; step; step >>= 1)
        if (lut[idx + step - 1u] < x) idx += step;
    return (float)idx / 255.0f;
}

// The six material words of the vertex in cell c at place f: grid_mesh_kernels.h, steps 2-5.
__device__ __forceinline__ void grid_material(const GridTexels& t, const LdsLut& lut, const uint32_t c[3], const float f[3],
                                              float m[6]) {
    uint64_t q[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) q[a] = (uint64_t)(c[a] + (f[a] > 0.5f ? 1u : 0u)) * t.lod;
    const uint64_t voxel = (q[2] * t.H + q[1]) * t.W + q[0];
    const float4 t0 = t.tex0[voxel], t1 = t.tex1[voxel];
    m[0] = srgb_index(lut, t0.y);
    m[1] = srgb_index(lut, t0.z);
    m[2] = srgb_index(lut, t0.w);
    m[3] = t1.x;
    m[4] = t1.y;
    m[5] = t1.z;
}

// vertex_normal's third material (lattice_vertex.h): the grid's, into the extractor's own 8-byte aligned records.
struct GridMaterial {
    const GridTexels& t;
    const LdsLut& lut;
    __device__ __forceinline__ void operator()(float* v, const uint32_t* c, const float* f) const {
        float m[6];
        grid_material(t, lut, c, f, m);
        float2* o = reinterpret_cast<float2*>(v + 6);
        o[0] = make_float2(m[0], m[1]);
        o[1] = make_float2(m[2], m[3]);
        o[2] = make_float2(m[4], m[5]);
    }
};

}  // namespace

extern "C" {

__global__ __launch_bounds__(kBlock) void grid_lattice_copy(GridTexels t, MeshGrid g, float* __restrict__ lattice) {
    unpack_point<kCopy>(t, g, lattice);
}

__global__ __launch_bounds__(kBlock) void grid_lattice_volume(GridTexels t, MeshGrid g, float* __restrict__ lattice) {
    unpack_point<kVolume>(t, g, lattice);
}

__global__ __launch_bounds__(kBlock) void grid_lattice_tex0(GridTexels t, MeshGrid g, float* __restrict__ lattice) {
    unpack_point<kTex0>(t, g, lattice);
}

__global__ __launch_bounds__(kBlock) void grid_vertex_materials(GridTexels t, MeshGrid g, float* __restrict__ vertices, uint32_t n) {
    __shared__ float s_lut[256];
    const LdsLut lut = stage_srgb_lut(s_lut);
    __syncthreads();
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    float* v = vertices + (size_t)i * 12;
    const float p[3] = {v[0], v[1], v[2]};
    uint32_t c[3];
    float f[3], m[6];
#pragma unroll
    for (int a = 0; a < 3; ++a) c[a] = lattice_cell(g, a, p[a], f[a]);
    grid_material(t, lut, c, f, m);
#pragma unroll
    for (int k = 0; k < 6; ++k) v[6 + k] = m[k];
}

__global__ __launch_bounds__(kBlock) void grid_normals_materials(const float* __restrict__ lattice, GridTexels t, MeshGrid g,
                                                                 float* __restrict__ vertices, uint32_t n) {
    __shared__ float s_lut[256];
    const LdsLut lut = stage_srgb_lut(s_lut);
    __syncthreads();
    vertex_normal(lattice, g, vertices, n, GridMaterial{t, lut});
}

}  // extern "C"

namespace {
// The lattice lies within the grid: the last point's voxel exists on every axis (W and H are the grid's; the depth is the
// caller's to have checked, it is not among the kernels' arguments).
bool lattice_fits(const GridTexels& t, const MeshGrid& g) {
    return g.launchable() && t.lod >= 1 && (uint64_t)g.cells[0] * t.lod < t.W && (uint64_t)g.cells[1] * t.lod < t.H;
}
}  // namespace

hipError_t launch_grid_lattice(const GridTexels& t, const MeshGrid& g, float* lattice, hipStream_t stream) {
    if (!lattice_fits(t, g) || !lattice || (!t.vol && !t.tex0)) return hipErrorInvalidValue;
    const dim3 blocks(blocks_for(g.n_points())), block(kBlock);
    if (!t.vol)
        hipLaunchKernelGGL(grid_lattice_tex0, blocks, block, 0, stream, t, g, lattice);
    else if (t.lod == 1 && !t.ilv && g.cells[0] + 1 == t.W && g.cells[1] + 1 == t.H)
        hipLaunchKernelGGL(grid_lattice_copy, blocks, block, 0, stream, t, g, lattice);
    else
        hipLaunchKernelGGL(grid_lattice_volume, blocks, block, 0, stream, t, g, lattice);
    return hipGetLastError();
}

hipError_t launch_grid_vertex_materials(const GridTexels& t, const MeshGrid& g, sdfv_vertex* vertices, size_t n,
                                        hipStream_t stream) {
    if (!vertices || n == 0) return hipSuccess;
    if (!lattice_fits(t, g) || !t.tex0 || !t.tex1 || n > 0xffffffffull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(grid_vertex_materials, dim3(blocks_for(n)), dim3(kBlock), 0, stream, t, g, reinterpret_cast<float*>(vertices),
                       (uint32_t)n);
    return hipGetLastError();
}

hipError_t launch_grid_normals_materials(const float* lattice, const GridTexels& t, const MeshGrid& g, sdfv_vertex* vertices,
                                         size_t n, hipStream_t stream) {
    if (!vertices || n == 0) return hipSuccess;
    if (!lattice_fits(t, g) || !t.tex0 || !t.tex1 || n > 0xffffffffull || ((uintptr_t)vertices & 7)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(grid_normals_materials, dim3(blocks_for(n)), dim3(kBlock), 0, stream, lattice, t, g,
                       reinterpret_cast<float*>(vertices), (uint32_t)n);
    return hipGetLastError();
}

}  // namespace sdfv
