// api_points_mesh.hip -- point, normal and source sampling, and mesh extraction for every SDF kind.
#include <cstring>
#include <type_traits>

#include "api_internal.h"
#include "mesh_kernels.h"
#include "points_kernels.h"
#include "program_kernels.h"
#include "program_mesh_kernels.h"
#include "dual_contour_kernels.h"
#include "lattice_mesh_kernels.h"
#include "grid_mesh_kernels.h"
#include "sparse_mesh_kernels.h"

using namespace sdfv;

namespace {

struct MeshScratch {
    void* p = nullptr;
    size_t bytes = 0;
    int device = -1;
    void release() {
        if (p) (void)hipFree(p);
        *this = MeshScratch{};
    }
    // Make the block at least `need` bytes on the current device, keeping the `keep` bytes at offset `at` (none: the block's
    // content is then not defined, and the old block goes before the new one comes).
    int reserve(size_t need, size_t at, size_t keep, hipStream_t st) {
        const int device_now = current_device();
        if (bytes >= need && device == device_now) return SDFV_OK;
        if (!keep || device != device_now) release();
        void* fresh = nullptr;
        SDFV_HIP(hipMalloc(&fresh, need));
        if (p) {
            hipError_t e = hipMemcpyAsync((char*)fresh + at, (char*)p + at, keep, hipMemcpyDeviceToDevice, st);
            if (e == hipSuccess) e = hipStreamSynchronize(st);
            if (e != hipSuccess) {
                (void)hipFree(fresh);
                return hip_fail(e, "sparse scratch copy");
            }
            release();
        }
        p = fresh;
        bytes = need;
        device = device_now;
        return SDFV_OK;
    }
};
// One block per host thread and route, grown on demand and kept between calls (allocating ~13 B per lattice point afresh costs
// more than the extraction itself); sdfv_mesh_trim() gives both back, a thread that exits without it leaks them.
thread_local MeshScratch g_mesh_scratch, g_sparse_scratch;

// The sub-blocks of a scratch block, in the order they are taken, each on a 256-byte boundary.  Without a block (base NULL)
// nothing is handed out and `at` only adds up: a layout is written once, run once for its size and once over the block.
struct Carve {
    char* base;
    size_t at = 0;
    template <typename T>
    T* take(size_t n) {
        T* sub = base ? reinterpret_cast<T*>(base + at) : nullptr;
        at += (n * sizeof(T) + 255) & ~(size_t)255;
        return sub;
    }
};

// The dense extraction's scratch; dual contouring has one more scan.  Returns the bytes it takes.
size_t lay_out(sdfv::MeshWork& w, void* block, size_t n_points, size_t n_cells, bool dual) {
    Carve c{static_cast<char*>(block)};
    w.scan_tmp_bytes = sdfv::mesh_scan_tmp_bytes(n_points);
    w.dist = c.take<float>(n_points);
    w.point_first = c.take<uint32_t>(n_points);
    w.cell_first = c.take<uint32_t>(n_cells);
    w.point_mask = c.take<uint8_t>(n_points);
    w.scan_tmp = c.take<char>(w.scan_tmp_bytes);
    w.totals = c.take<uint32_t>(64);
    w.quad_first = dual ? c.take<uint32_t>(n_points) : nullptr;
    return c.at;
}

// The two phases of the sparse extraction's: the totals word (256 bytes), then the block list at a FIXED offset, so that a block
// that has to grow takes the list along with one copy, then what the phase adds.  Refinement of n parents: room for their 8 n
// children in the list, and 8 n candidates ...
constexpr size_t kSparseListAt = 256;
size_t lay_out_refinement(sdfv::SparseWork& w, void* block, size_t n_parents) {
    Carve c{static_cast<char*>(block)};
    const size_t children = n_parents * 8;
    w.mesh.scan_tmp_bytes = sdfv::mesh_scan_tmp_bytes(children);
    w.mesh.totals = c.take<uint32_t>(64);
    w.list = c.take<uint32_t>(children);
    w.cand = c.take<uint32_t>(children);
    w.pos = c.take<uint32_t>(children);
    w.mesh.scan_tmp = c.take<char>(w.mesh.scan_tmp_bytes);
    return c.at;
}
// ... the brick phase over n bricks: 125 n points and 64 n cells, each scan with one entry more (the total).
size_t lay_out_bricks(sdfv::SparseWork& w, void* block, size_t n) {
    Carve c{static_cast<char*>(block)};
    const size_t points = n * sdfv::kBrickPoints, cells = n * sdfv::kBrickCells;
    w.mesh.scan_tmp_bytes = sdfv::mesh_scan_tmp_bytes(points + 1);
    w.mesh.totals = c.take<uint32_t>(64);
    w.list = c.take<uint32_t>(n);
    w.mesh.dist = c.take<float>(points);
    w.mesh.point_first = c.take<uint32_t>(points + 1);
    w.mesh.cell_first = c.take<uint32_t>(cells + 1);
    w.mesh.point_mask = c.take<uint8_t>(points);
    w.neighbours = c.take<uint32_t>(n * 8);
    w.mesh.scan_tmp = c.take<char>(w.mesh.scan_tmp_bytes);
    return c.at;
}

// The output buffers for the counts in m.  On failure nothing is left allocated.
int allocate_mesh(sdfv_mesh& m) {
    if (m.n_vertices) SDFV_HIP(hipMalloc((void**)&m.vertices, m.n_vertices * sizeof(sdfv_vertex)));
    if (m.n_indices) {
        hipError_t e = hipMalloc((void**)&m.indices, m.n_indices * 4);
        if (e != hipSuccess) {
            (void)hipFree(m.vertices);
            return hip_fail(e, "hipMalloc(indices)");
        }
    }
    return SDFV_OK;
}
// ... and the end of an extraction whose emit chain returned e: the mesh goes out once the stream is done with it (the next
// extraction on this thread reuses the scratch), or, on any failure, both buffers go back.
int finish_mesh(hipError_t e, const sdfv_mesh& m, sdfv_mesh* out, hipStream_t st, const char* what) {
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) {
        (void)hipFree(m.vertices);
        (void)hipFree(m.indices);
        return hip_fail(e, what);
    }
    *out = m;
    return SDFV_OK;
}

// Meshers::mesh for any kind of SDF: the arguments are checked by the caller.  An SDF kind supplies two things:
// `lattice(g, w, stream)` writes the distances of the lattice points into w.dist (or points w.dist at distances that exist: a
// caller's lattice, which no step writes), and `attributes(vertices, n, final, stream)` everything but
// the position of n vertices whose positions are written.  Counting, the scans, the positions of the crossing edges, the
// triangles (mesh_kernels.h) and dual contouring's solve and quads (dual_contour_kernels.h) do not depend on the SDF.  `final` is
// false only for dual contouring's Hermite records: crossing-edge vertices in a temporary, of which the solve reads position and
// normal and nothing else.  The scratch is the calling thread's dense block, laid out by lay_out.
// An SDF kind whose attributes are cheap enough to write under the positions' sparse mask may also give
// `fused(g, w, vertices, n, stream)`: marching cubes then calls it in the place of positions + attributes (the demo tree does).
// The lattice is `g`: any number of cells per axis (MeshGrid::launchable).
template <typename LatticeFn, typename AttributesFn, typename FusedFn = std::nullptr_t>
int extract_mesh(const sdfv::MeshGrid& g, uint32_t algorithm, sdfv_mesh* out, hipStream_t st, LatticeFn&& lattice,
                 AttributesFn&& attributes, FusedFn&& fused = nullptr) {
    const bool dual = algorithm == SDFV_MESHER_DUAL_CONTOURING_PARTICLE;
    const size_t n_points = g.n_points(), n_cells = g.n_cells();
    sdfv::MeshWork w{};
    if (int rc = g_mesh_scratch.reserve(lay_out(w, nullptr, n_points, n_cells, dual), 0, 0, st)) return rc;
    lay_out(w, g_mesh_scratch.p, n_points, n_cells, dual);
    SDFV_HIP(lattice(g, w, st));
    SDFV_HIP(dual ? sdfv::launch_dc_count(g, w, w.totals, st) : sdfv::launch_mesh_count(g, w, w.totals, st));
    uint32_t n[3] = {0, 0, 0};  // marching cubes: vertices, triangles; dual contouring: Hermite records, vertices, quads
    SDFV_HIP(hipMemcpyAsync(n, w.totals, dual ? 12 : 8, hipMemcpyDeviceToHost, st));
    SDFV_HIP(hipStreamSynchronize(st));
    sdfv_mesh m{};
    m.n_vertices = dual ? n[1] : n[0];
    m.n_indices = dual ? (size_t)n[2] * 6 : (size_t)n[1] * 3;
    if (int rc = allocate_mesh(m)) return rc;
    hipError_t e = hipSuccess;
    void* hermite = nullptr;  // dual contouring: n[0] Hermite records, then the list of the n[1] active cells
    if (!dual) {
        if constexpr (std::is_same_v<std::decay_t<FusedFn>, std::nullptr_t>) {
            e = sdfv::launch_mesh_edge_positions(g, w, m.vertices, m.n_vertices, st);
            if (e == hipSuccess) e = attributes(m.vertices, m.n_vertices, true, st);
        } else {
            e = fused(g, w, m.vertices, m.n_vertices, st);
        }
        if (e == hipSuccess) e = sdfv::launch_mesh_triangles(g, w, m.indices, st);
    } else if (m.n_vertices) {
        const size_t records = (size_t)n[0] * sizeof(sdfv_vertex);
        e = hipMalloc(&hermite, records + m.n_vertices * 4);
        if (e == hipSuccess) e = sdfv::launch_mesh_edge_positions(g, w, (sdfv_vertex*)hermite, n[0], st);
        if (e == hipSuccess) e = attributes((sdfv_vertex*)hermite, n[0], false, st);
        if (e == hipSuccess)
            e = sdfv::launch_dc_vertices(g, w, (const sdfv_vertex*)hermite, (uint32_t*)((char*)hermite + records), m.vertices,
                                         m.n_vertices, st);
        if (e == hipSuccess) e = attributes(m.vertices, m.n_vertices, true, st);
        if (e == hipSuccess) e = sdfv::launch_dc_quads(g, w, m.indices, st);
    }
    const int rc = finish_mesh(e, m, out, st, "mesh emit");
    if (hermite) (void)hipFree(hermite);  // after finish_mesh: the stream is done with it, or has failed
    return rc;
}

// ... over the cube every mesher of the reference takes: max_voxels_per_axis cells on each axis of the box
sdfv::MeshGrid lattice_grid(const float bb_min[3], const float bb_max[3], uint32_t cells) {
    sdfv::MeshGrid g;
    for (int i = 0; i < 3; ++i) {
        g.cells[i] = cells;
        g.bb_min[i] = bb_min[i];
        g.bb_size[i] = bb_max[i] - bb_min[i];
    }
    return g;
}
template <typename LatticeFn, typename AttributesFn, typename FusedFn = std::nullptr_t>
int extract_mesh(const float bb_min[3], const float bb_max[3], uint32_t max_voxels_per_axis, uint32_t algorithm, sdfv_mesh* out,
                 hipStream_t st, LatticeFn&& lattice, AttributesFn&& attributes, FusedFn&& fused = nullptr) {
    return extract_mesh(lattice_grid(bb_min, bb_max, max_voxels_per_axis), algorithm, out, st, lattice, attributes, fused);
}

}  // namespace

#pragma GCC visibility push(default)
extern "C" {

int sdfv_sample_points(const sdfv_demo_params* params, uint32_t sdf_id, const float* points, size_t n,
                       int distance_only, sdfv_sample* out, void* stream) {
    if (int rc = check_params(params, sdf_id)) return rc;
    if (int rc = check_point_buffers(points, out, n)) return rc;
    if (int rc = need_device()) return rc;
    SDFV_HIP_RETURN(sdfv::launch_sample_points(*params, sdf_id, points, n, distance_only != 0, out, (hipStream_t)stream));
}

int sdfv_normal_points(const sdfv_demo_params* params, uint32_t sdf_id, const float* points, size_t n, float eps,
                       int use_default, float* out, void* stream) {
    if (int rc = check_params(params, sdf_id)) return rc;
    if (int rc = check_point_buffers(points, out, n)) return rc;
    if (int rc = need_device()) return rc;
    SDFV_HIP_RETURN(sdfv::launch_normal_points(*params, sdf_id, nullptr, nullptr, points, n, eps, use_default != 0, out,
                                        (hipStream_t)stream));
}

int sdfv_source_sample_scalar(const sdfv_demo_params* params, uint32_t sdf_id, const float bb_min[3],
                              const float bb_max[3], const float* unit_points, size_t n, float* dist_out, void* stream) {
    if (int rc = check_params(params, sdf_id)) return rc;
    if (!bb_min || !bb_max) return set_error(SDFV_ERR_INVALID_ARGUMENT, "bounding box is NULL");
    if (int rc = check_point_buffers(unit_points, dist_out, n)) return rc;
    if (int rc = need_device()) return rc;
    SDFV_HIP_RETURN(sdfv::launch_source_scalar(*params, sdf_id, bb_min, bb_max, unit_points, n, dist_out, (hipStream_t)stream));
}

int sdfv_source_sample_normal(const sdfv_demo_params* params, uint32_t sdf_id, const float bb_min[3],
                              const float bb_max[3], const float* unit_points, size_t n, float* normal_out,
                              void* stream) {
    if (int rc = check_params(params, sdf_id)) return rc;
    if (!bb_min || !bb_max) return set_error(SDFV_ERR_INVALID_ARGUMENT, "bounding box is NULL");
    if (int rc = check_point_buffers(unit_points, normal_out, n)) return rc;
    if (int rc = need_device()) return rc;
    SDFV_HIP_RETURN(sdfv::launch_normal_points(*params, sdf_id, bb_min, bb_max, unit_points, n, 0.0f, false, normal_out,
                                        (hipStream_t)stream));
}

int sdfv_mesh_postproc(const sdfv_demo_params* params, uint32_t sdf_id, sdfv_vertex* vertices, size_t n, void* stream) {
    if (int rc = check_params(params, sdf_id)) return rc;
    if (int rc = check_point_buffers(vertices, vertices, n)) return rc;
    if (int rc = check_word_aligned("vertices", vertices)) return rc;
    if (int rc = need_device()) return rc;
    SDFV_HIP_RETURN(sdfv::launch_mesh_postproc(*params, sdf_id, vertices, n, (hipStream_t)stream));
}

int sdfv_mesh_extract(const sdfv_demo_params* params, uint32_t sdf_id, const float bb_min[3], const float bb_max[3],
                      uint32_t max_voxels_per_axis, uint32_t algorithm, sdfv_mesh* out, void* stream) {
    if (!out) return set_error(SDFV_ERR_INVALID_ARGUMENT, "out is NULL");
    memset(out, 0, sizeof(*out));
    if (int rc = check_params(params, sdf_id)) return rc;
    if (!bb_min || !bb_max) return set_error(SDFV_ERR_INVALID_ARGUMENT, "bounding box is NULL");
    if (int rc = check_mesher(algorithm, max_voxels_per_axis)) return rc;
    if (int rc = need_device()) return rc;
    return extract_mesh(
        bb_min, bb_max, max_voxels_per_axis, algorithm, out, (hipStream_t)stream,
        [&](const sdfv::MeshGrid& g, const sdfv::MeshWork& w, hipStream_t st) {
            return sdfv::launch_mesh_lattice(*params, sdf_id, g, w, st);
        },
        [&](sdfv_vertex* vertices, size_t n, bool, hipStream_t st) {
            return sdfv::launch_mesh_vertex_normals(*params, sdf_id, vertices, n, st);
        },
        [&](const sdfv::MeshGrid& g, const sdfv::MeshWork& w, sdfv_vertex* vertices, size_t n, hipStream_t st) {
            return sdfv::launch_mesh_fused_vertices(*params, sdf_id, g, w, vertices, n, st);
        });
}

int sdfv_program_mesh_extract(const sdfv_program* p, const float bb_min[3], const float bb_max[3], uint32_t max_voxels_per_axis,
                              uint32_t algorithm, uint32_t flags, sdfv_mesh* out, void* stream) {
    if (!out) return set_error(SDFV_ERR_INVALID_ARGUMENT, "out is NULL");
    memset(out, 0, sizeof(*out));
    if (!p) return set_error(SDFV_ERR_INVALID_ARGUMENT, "program is NULL");
    if ((bb_min == nullptr) != (bb_max == nullptr))
        return set_error(SDFV_ERR_INVALID_ARGUMENT, "bounding box: bb_min and bb_max are both given or both NULL (the program's box)");
    if (int rc = check_mesher(algorithm, max_voxels_per_axis)) return rc;
    if (flags & ~SDFV_MESH_WITH_MATERIALS) return set_error(SDFV_ERR_INVALID_ARGUMENT, "unknown flags 0x%x", flags);
    if (int rc = need_device()) return rc;
    sdfv::ProgramKernels compiled;  // (a compiled handle on the wrong device is refused before its device copy is made)
    if (int rc = program_compiled_kernels(p, SDFV_COMPILE_MESH, &compiled)) return rc;
    const sdfv_prog_op* dev_ops = nullptr;
    uint32_t n_ops = 0;
    const float* bb = nullptr;
    if (int rc = program_on_device(p, &dev_ops, &n_ops, &bb)) return rc;
    const bool materials = (flags & SDFV_MESH_WITH_MATERIALS) != 0;
    return extract_mesh(
        bb_min ? bb_min : bb, bb_max ? bb_max : bb + 3, max_voxels_per_axis, algorithm, out, (hipStream_t)stream,
        [&](const sdfv::MeshGrid& g, const sdfv::MeshWork& w, hipStream_t st) {
            return sdfv::launch_program_mesh_lattice(dev_ops, n_ops, g, w, compiled, st);
        },
        [&](sdfv_vertex* vertices, size_t n, bool final, hipStream_t st) {  // the materials belong to the output vertices only
            return sdfv::launch_program_vertex_normals(dev_ops, n_ops, vertices, n, materials && final, compiled, st);
        });
}

// ---- sparse meshing of a program: refine blocks towards the surface, then marching cubes over the surviving bricks ----
namespace {
// t = (L * r) * 1.001f for blocks of s cells (include/sdfgrid.h): f32, one rounding per step (this file is built with
// -ffp-contract=off like the kernels)
float sparse_threshold(const sdfv::MeshGrid& g, uint32_t s, float L) {
    float e[3];
    for (int a = 0; a < 3; ++a) e[a] = (float)s / (float)g.cells[a] * g.bb_size[a];
    const float r = 0.5f * sqrtf((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]);
    return (L * r) * 1.001f;
}

int extract_sparse(const sdfv_prog_op* dev_ops, uint32_t n_ops, const sdfv::ProgramKernels& compiled, const sdfv::MeshGrid& g, float L,
                   bool materials, sdfv_mesh* out, sdfv_sparse_mesh_stats* stats, hipStream_t st) {
    const uint32_t N = g.cells[0];
    sdfv_sparse_mesh_stats s{};
    while ((4u << s.levels) < N) ++s.levels;
    size_t scratch = 0;
    sdfv::SparseWork w{};
    // the block for a phase that takes `need` bytes, with the first `keep` entries of the list as they are
    auto reserve = [&](size_t need, size_t keep) {
        scratch = need > scratch ? need : scratch;
        return g_sparse_scratch.reserve(need, kSparseListAt, keep * 4, st);
    };
    // ---- refinement: the root (key 0) is not tested
    uint32_t n = 1;
    for (uint32_t level = 0; level < s.levels && n; ++level) {
        if (int rc = reserve(lay_out_refinement(w, nullptr, n), level ? n : 0)) return rc;
        lay_out_refinement(w, g_sparse_scratch.p, n);
        if (level == 0) SDFV_HIP(hipMemsetAsync(w.list, 0, 4, st));
        const uint32_t shift = 31u - (uint32_t)__builtin_clz(N >> (level + 1));  // children of N / 2^(level + 1) cells
        SDFV_HIP(sdfv::launch_sparse_refine(dev_ops, n_ops, g, shift, sparse_threshold(g, 1u << shift, L), w, n, w.mesh.totals, compiled, st));
        s.tested[level] = n * 8u;
        SDFV_HIP(hipMemcpyAsync(&n, w.mesh.totals, 4, hipMemcpyDeviceToHost, st));
        SDFV_HIP(hipStreamSynchronize(st));
        s.kept[level] = n;
        s.evaluations += s.tested[level];
    }
    s.bricks = n;
    s.evaluations += (uint64_t)sdfv::kBrickPoints * n;
    sdfv_mesh m{};
    if (n) {
        if ((uint64_t)n * 3u * sdfv::kBrickPoints > 0xffffffffull)
            return set_error(SDFV_ERR_INVALID_ARGUMENT, "%u bricks: more than %u could overflow the 32-bit vertex and triangle counts", n,
                             0xffffffffu / (3u * sdfv::kBrickPoints));
        // ---- the brick phase
        if (int rc = reserve(lay_out_bricks(w, nullptr, n), s.levels ? n : 0)) return rc;
        lay_out_bricks(w, g_sparse_scratch.p, n);
        if (s.levels == 0) SDFV_HIP(hipMemsetAsync(w.list, 0, 4, st));
        SDFV_HIP(sdfv::launch_sparse_brick_lattice(dev_ops, n_ops, g, w, n, compiled, st));
        SDFV_HIP(sdfv::launch_sparse_count(g, w, n, st));
        uint32_t totals[2] = {0, 0};  // vertices, triangles: the extra last entry of each scan
        SDFV_HIP(hipMemcpyAsync(&totals[0], w.mesh.point_first + (size_t)n * sdfv::kBrickPoints, 4, hipMemcpyDeviceToHost, st));
        SDFV_HIP(hipMemcpyAsync(&totals[1], w.mesh.cell_first + (size_t)n * sdfv::kBrickCells, 4, hipMemcpyDeviceToHost, st));
        SDFV_HIP(hipStreamSynchronize(st));
        m.n_vertices = totals[0];
        m.n_indices = (size_t)totals[1] * 3;
        if (int rc = allocate_mesh(m)) return rc;
        hipError_t e = sdfv::launch_sparse_positions(g, w, n, m.vertices, m.n_vertices, st);  // marching cubes' chain, as extract_mesh
        if (e == hipSuccess) e = sdfv::launch_program_vertex_normals(dev_ops, n_ops, m.vertices, m.n_vertices, materials, compiled, st);
        if (e == hipSuccess) e = sdfv::launch_sparse_triangles(g, w, n, m.indices, st);
        if (int rc = finish_mesh(e, m, out, st, "sparse mesh emit")) return rc;
    }
    *out = m;
    if (stats) {
        s.size = stats->size;
        s.scratch_bytes = scratch;
        memcpy(stats, &s, sizeof(s));
    }
    return SDFV_OK;
}
}  // namespace

int sdfv_program_mesh_extract_sparse(const sdfv_sparse_mesh_desc* desc, void* stream) {
    sdfv_sparse_mesh_desc d;
    if (int rc = read_sized_desc(desc, sizeof(sdfv_sparse_mesh_desc), "sdfv_sparse_mesh_desc", d)) {
        if (desc && desc->size >= sizeof(sdfv_sparse_mesh_desc) && desc->out) memset(desc->out, 0, sizeof(*desc->out));
        return rc;
    }
    if (d.out) memset(d.out, 0, sizeof(*d.out));
    if (d.reserved) return set_error(SDFV_ERR_INVALID_ARGUMENT, "sdfv_sparse_mesh_desc.reserved must be 0");
    if (!d.out) return set_error(SDFV_ERR_INVALID_ARGUMENT, "out is NULL");
    if (!d.program) return set_error(SDFV_ERR_INVALID_ARGUMENT, "program is NULL");
    if ((d.bb_min == nullptr) != (d.bb_max == nullptr))
        return set_error(SDFV_ERR_INVALID_ARGUMENT, "bounding box: bb_min and bb_max are both given or both NULL (the program's box)");
    if (d.algorithm != SDFV_MESHER_MARCHING_CUBES) return set_error(SDFV_ERR_INVALID_ARGUMENT, "Unsupported algorithm %u", d.algorithm);
    if (d.cells < 4 || d.cells > 4096 || (d.cells & (d.cells - 1u)))
        return set_error(SDFV_ERR_INVALID_ARGUMENT, "cells %u is not a power of two in [4, 4096]", d.cells);
    if (d.flags & ~SDFV_MESH_WITH_MATERIALS) return set_error(SDFV_ERR_INVALID_ARGUMENT, "unknown flags 0x%x", d.flags);
    if (!(d.lipschitz == 0.0f || (d.lipschitz >= 1.0f && d.lipschitz <= 3.402823466e+38f)))
        return set_error(SDFV_ERR_INVALID_ARGUMENT, "lipschitz %g is neither 0 (= 1) nor a finite number >= 1", (double)d.lipschitz);
    if (d.stats && d.stats->size < sizeof(sdfv_sparse_mesh_stats))
        return set_error(SDFV_ERR_INVALID_ARGUMENT, "sdfv_sparse_mesh_stats.size = %u is smaller than the structure (%zu)", d.stats->size,
                         sizeof(sdfv_sparse_mesh_stats));
    if (int rc = need_device()) return rc;
    sdfv::ProgramKernels compiled;  // (as above: the wrong device is refused first)
    if (int rc = program_compiled_kernels(d.program, SDFV_COMPILE_MESH, &compiled)) return rc;
    const sdfv_prog_op* dev_ops = nullptr;
    uint32_t n_ops = 0;
    const float* bb = nullptr;
    if (int rc = program_on_device(d.program, &dev_ops, &n_ops, &bb)) return rc;
    return extract_sparse(dev_ops, n_ops, compiled, lattice_grid(d.bb_min ? d.bb_min : bb, d.bb_max ? d.bb_max : bb + 3, d.cells),
                          d.lipschitz == 0.0f ? 1.0f : d.lipschitz, (d.flags & SDFV_MESH_WITH_MATERIALS) != 0, d.out, d.stats,
                          (hipStream_t)stream);
}

// ---- meshing a sampled lattice: the SDF is the caller's, the library sees (cells + 1)^3 distances ----
namespace {
int check_lattice(const float* dist, const float bb_min[3], const float bb_max[3]) {
    if (!dist) return set_error(SDFV_ERR_INVALID_ARGUMENT, "dist is NULL");
    if (!bb_min || !bb_max) return set_error(SDFV_ERR_INVALID_ARGUMENT, "bounding box is NULL");
    return check_word_aligned("dist", dist);
}
}  // namespace

int sdfv_lattice_points(const float bb_min[3], const float bb_max[3], uint32_t cells, size_t first, size_t n, float* points,
                        void* stream) {
    if (!bb_min || !bb_max) return set_error(SDFV_ERR_INVALID_ARGUMENT, "bounding box is NULL");
    if (int rc = check_mesher(SDFV_MESHER_MARCHING_CUBES, cells)) return rc;
    const sdfv::MeshGrid g = lattice_grid(bb_min, bb_max, cells);
    if (first > g.n_points() || n > g.n_points() - first)
        return set_error(SDFV_ERR_INVALID_ARGUMENT, "points [%zu, %zu + %zu) are not all among the lattice's %zu", first, first, n,
                         g.n_points());
    if (int rc = check_point_buffers(points, points, n)) return rc;
    if (int rc = check_word_aligned("points", points)) return rc;
    if (int rc = need_device()) return rc;
    SDFV_HIP_RETURN(sdfv::launch_lattice_points(g, (uint32_t)first, (uint32_t)n, points, (hipStream_t)stream));
}

int sdfv_lattice_from_samples(const sdfv_sample* samples, size_t n, float* dist, void* stream) {
    if (int rc = check_point_buffers(samples, dist, n)) return rc;
    if (int rc = check_word_aligned("samples and dist", samples, dist)) return rc;
    if (int rc = need_device()) return rc;
    SDFV_HIP_RETURN(sdfv::launch_lattice_from_samples(samples, n, dist, (hipStream_t)stream));
}

int sdfv_lattice_normals(const float* dist, const float bb_min[3], const float bb_max[3], uint32_t cells, sdfv_vertex* vertices,
                         size_t n, void* stream) {
    if (int rc = check_lattice(dist, bb_min, bb_max)) return rc;
    if (int rc = check_mesher(SDFV_MESHER_MARCHING_CUBES, cells)) return rc;
    if (int rc = check_point_buffers(vertices, vertices, n)) return rc;
    if (int rc = check_word_aligned("vertices", vertices)) return rc;
    if (n > 0xffffffffull) return set_error(SDFV_ERR_INVALID_ARGUMENT, "%zu vertices are too many for one launch", n);
    if (int rc = need_device()) return rc;
    SDFV_HIP_RETURN(sdfv::launch_lattice_normals(dist, lattice_grid(bb_min, bb_max, cells), vertices, n, false, (hipStream_t)stream));
}

int sdfv_lattice_mesh_extract(const float* dist, const float bb_min[3], const float bb_max[3], uint32_t max_voxels_per_axis,
                              uint32_t algorithm, uint32_t flags, sdfv_mesh* out, void* stream) {
    if (!out) return set_error(SDFV_ERR_INVALID_ARGUMENT, "out is NULL");
    memset(out, 0, sizeof(*out));
    if (int rc = check_lattice(dist, bb_min, bb_max)) return rc;
    if (int rc = check_mesher(algorithm, max_voxels_per_axis)) return rc;
    if (flags) return set_error(SDFV_ERR_INVALID_ARGUMENT, "unknown flags 0x%x", flags);
    if (int rc = need_device()) return rc;
    const sdfv::MeshGrid grid = lattice_grid(bb_min, bb_max, max_voxels_per_axis);
    return extract_mesh(
        bb_min, bb_max, max_voxels_per_axis, algorithm, out, (hipStream_t)stream,
        [&](const sdfv::MeshGrid&, sdfv::MeshWork& w, hipStream_t) {  // read in place: every step takes w.dist as const
            w.dist = const_cast<float*>(dist);
            return hipSuccess;
        },
        [&](sdfv_vertex* vertices, size_t n, bool final, hipStream_t st) {  // the zero material belongs to the output vertices
            return sdfv::launch_lattice_normals(dist, grid, vertices, n, final, st);
        });
}

// ---- meshing a loaded grid: the lattice is the grid's own voxels at step `lod`, the materials are its texels' ----
namespace {
// The checks both entry points share, and what they derive: the lattice (cells per axis, the sub-box [bb_min, position of voxel
// cells * lod]) and where the kernels read.
int grid_lattice_of(const sdfv_grid* grid, const float* tex0, const float* tex1, bool need_tex1, const float* dist,
                    uint32_t volume_flags, uint32_t lod, sdfv::MeshGrid& g, sdfv::GridTexels& t) {
    if (int rc = check_grid(grid)) return rc;
    if (grid->z_begin != 0 || (grid->z_end != 0 && grid->z_end != grid->dims[2]))
        return set_error(SDFV_ERR_INVALID_ARGUMENT, "slab [%u,%u) of depth %u: meshing takes a whole grid", grid->z_begin, grid->z_end,
                         grid->dims[2]);
    if (!tex0 || (need_tex1 && !tex1)) return set_error(SDFV_ERR_INVALID_ARGUMENT, "texture pointer is NULL");
    if (int rc = check_texel_alignment(tex0, tex1)) return rc;
    if (int rc = check_word_aligned("dist", dist)) return rc;
    if (volume_flags & ~SDFV_PASS_VOLUME_INTERLEAVED) return set_error(SDFV_ERR_INVALID_ARGUMENT, "unknown flags 0x%x", volume_flags);
    if (int rc = check_interleaved_volume(grid, dist, volume_flags)) return rc;
    if (lod == 0 || (lod & (lod - 1u))) return set_error(SDFV_ERR_INVALID_ARGUMENT, "lod %u is not a power of two", lod);
    for (int a = 0; a < 3; ++a) {
        g.cells[a] = grid->dims[a] ? (grid->dims[a] - 1u) / lod : 0u;
        if (g.cells[a] < 1 || g.cells[a] > 1024)
            return set_error(SDFV_ERR_INVALID_ARGUMENT, "%u cells along axis %d (dims %u at lod %u) are outside [1, 1024]", g.cells[a], a,
                             grid->dims[a], lod);
        // voxel_coord of the lattice's last voxel: idx / (dim - 1) * size + min, three separately rounded steps
        const float last = (float)(g.cells[a] * lod) / ((float)grid->dims[a] - 1.0f) * (grid->bb_max[a] - grid->bb_min[a]) + grid->bb_min[a];
        g.bb_min[a] = grid->bb_min[a];
        g.bb_size[a] = last - grid->bb_min[a];
    }
    if (g.n_points() > 0xffffffffull)
        return set_error(SDFV_ERR_INVALID_ARGUMENT, "a lattice of %zu points is too large for one launch", g.n_points());
    t.tex0 = reinterpret_cast<const float4*>(tex0);
    t.tex1 = reinterpret_cast<const float4*>(tex1);
    t.vol = dist;
    t.ilv = (volume_flags & SDFV_PASS_VOLUME_INTERLEAVED) ? 1u : 0u;
    t.W = grid->dims[0];
    t.H = grid->dims[1];
    t.lod = lod;
    return SDFV_OK;
}
}  // namespace

int sdfv_grid_mesh_extract(const sdfv_grid* grid, const float* tex0, const float* tex1, const float* dist, uint32_t volume_flags,
                           uint32_t lod, uint32_t algorithm, uint32_t flags, sdfv_mesh* out, void* stream) {
    if (!out) return set_error(SDFV_ERR_INVALID_ARGUMENT, "out is NULL");
    memset(out, 0, sizeof(*out));
    if (flags & ~SDFV_MESH_WITH_MATERIALS) return set_error(SDFV_ERR_INVALID_ARGUMENT, "unknown flags 0x%x", flags);
    const bool materials = (flags & SDFV_MESH_WITH_MATERIALS) != 0;
    sdfv::MeshGrid g{};
    sdfv::GridTexels t{};
    if (int rc = grid_lattice_of(grid, tex0, tex1, materials, dist, volume_flags, lod, g, t)) return rc;
    if (int rc = check_mesher(algorithm, g.cells[0])) return rc;
    if (int rc = need_device()) return rc;
    const float* lattice = nullptr;
    return extract_mesh(
        g, algorithm, out, (hipStream_t)stream,
        [&](const sdfv::MeshGrid&, const sdfv::MeshWork& w, hipStream_t st) {
            lattice = w.dist;
            return sdfv::launch_grid_lattice(t, g, w.dist, st);
        },
        [&](sdfv_vertex* vertices, size_t n, bool final, hipStream_t st) {  // the materials belong to the output vertices only
            if (final && materials) return sdfv::launch_grid_normals_materials(lattice, t, g, vertices, n, st);
            return sdfv::launch_lattice_normals(lattice, g, vertices, n, final, st);
        });
}

int sdfv_grid_vertex_materials(const sdfv_grid* grid, const float* tex0, const float* tex1, uint32_t lod, sdfv_vertex* vertices,
                               size_t n, void* stream) {
    sdfv::MeshGrid g{};
    sdfv::GridTexels t{};
    if (int rc = grid_lattice_of(grid, tex0, tex1, true, nullptr, 0, lod, g, t)) return rc;
    if (int rc = check_point_buffers(vertices, vertices, n)) return rc;
    if (int rc = check_word_aligned("vertices", vertices)) return rc;
    if (n > 0xffffffffull) return set_error(SDFV_ERR_INVALID_ARGUMENT, "%zu vertices are too many for one launch", n);
    if (int rc = need_device()) return rc;
    SDFV_HIP_RETURN(sdfv::launch_grid_vertex_materials(t, g, vertices, n, (hipStream_t)stream));
}

int sdfv_mesh_trim(void) {
    g_mesh_scratch.release();
    g_sparse_scratch.release();
    release_march_caches();
    return SDFV_OK;
}

int sdfv_mesh_free(sdfv_mesh* mesh) {
    if (!mesh) return SDFV_OK;
    if (mesh->vertices) (void)hipFree(mesh->vertices);
    if (mesh->indices) (void)hipFree(mesh->indices);
    memset(mesh, 0, sizeof(*mesh));
    return SDFV_OK;
}

}  // extern "C"
#pragma GCC visibility pop
