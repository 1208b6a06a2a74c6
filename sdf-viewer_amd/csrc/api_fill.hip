// api_fill.hip -- grid initialisation, the dense fill, passes, packing, the committed volumes, and the slab helpers of slab_comm.hip.
#include <cstring>

#include "api_internal.h"
#include "fill_kernels.h"
#include "ingest_kernels.h"
#include "program_kernels.h"
#include "program_pass_kernels.h"

using namespace sdfv;

namespace {

// The part of a dense fill's kernel arguments that says WHERE it writes, for either argument block (FillArgs,
// ProgramFillArgs: the fields dense_fill_rows reads); x_chunks is the launcher's.  `a` comes zeroed.
template <typename Args>
void set_grid_fill_args(Args& a, const sdfv_grid& g, float* tex0, float* tex1, float* dist = nullptr, uint32_t dist_ilv = 0) {
    a.W = g.dims[0];
    a.H = g.dims[1];
    a.z_begin = g.z_begin;
    a.slab_d = g.z_end - g.z_begin;
    sdfv::set_voxel_coords(a, g);
    a.air_dist = air_dist();
    a.tex0 = reinterpret_cast<float4*>(tex0);
    a.tex1 = reinterpret_cast<float4*>(tex1);
    a.dist = dist;
    a.dist_ilv = dist_ilv;
    a.srgb_round = g_options.ext_srgb_quant;
}

sdfv::FillArgs make_fill_args(const sdfv_demo_params& p, uint32_t sdf_id, const sdfv_grid& g, float* tex0,
                              float* tex1) {
    sdfv::FillArgs a;
    memset(&a, 0, sizeof(a));
    a.prm = p;
    a.sdf_id = sdf_id;
    a.D = g.dims[2];
    set_grid_fill_args(a, g, tex0, tex1);
    return a;
}

// Store policy and index form of the dense fill (SDFV_OPT_FILL_*).  Store policy "auto": a launch that also writes the
// compact distance volume streams the two textures past L2 (nt) -- nothing re-reads them before the march's few texels
// under the hits, while the distance volume, which the march gathers from, keeps its place in the caches: the fused
// fill itself runs 6 % faster (0.097 -> 0.091 ms at 256^3) and fill + march 0.188 -> 0.177 ms (EXPERIMENTS, round 2 store-policy probe).
// The plain fill keeps plain stores (nt: within noise alone, +3 % on the 256^3 pipeline, -3 % on the 512^3 one).
sdfv::FillLaunch fill_launch_config(bool writes_distance_volume) {
    sdfv::FillLaunch c;
    c.nontemporal = g_options.fill_nontemporal == 1 || (g_options.fill_nontemporal == 0 && writes_distance_volume);
    c.force_rows = g_options.fill_form == 1;
    c.force_flat = g_options.fill_form == 2;
    c.force_paired = g_options.fill_form == 3;
    c.force_pairrows = g_options.fill_form == 4;
    // the interleaved-volume fill with the rows of a pair on one XCD rests on workgroup b -> XCD b % 8 (as the march's tile orders do)
    c.xcd_pairing = device_facts().xcds == 8;
    return c;
}

}  // namespace

namespace sdfv {
int ordered_fill_blocks(const sdfv_grid* slab, uint32_t* per_slice, uint32_t* total) {
    if (int rc = check_grid(slab)) return rc;
    sdfv_demo_params prm;
    sdfv_demo_params_default(&prm);
    const FillArgs a = make_fill_args(prm, SDFV_SDF_DEMO, *slab, nullptr, nullptr);
    const OrderedBlocks b = ordered_blocks(a);
    *per_slice = b.per_slice;
    *total = b.total;
    return SDFV_OK;
}

int fill_slab_ordered(const sdfv_demo_params* params, uint32_t sdf_id, const sdfv_grid* slab, float* o0, float* o1,
                      const OrderedFill& of, uint32_t block_begin, uint32_t block_end, void* stream) {
    if (int rc = check_params(params, sdf_id)) return rc;
    if (int rc = check_grid(slab)) return rc;
    if (int rc = check_texel_alignment(o0, o1, of.stage_lo, of.stage_hi)) return rc;
    if (int rc = need_device()) return rc;
    FillArgs a = make_fill_args(*params, sdf_id, *slab, o0, o1);
    a.order_lead = of.lead;
    a.stage_only = of.stage_only ? 1u : 0u;
    a.dist = of.dist;
    a.stage_lo = reinterpret_cast<float4*>(of.stage_lo);
    a.stage_hi = reinterpret_cast<float4*>(of.stage_hi);
    SDFV_HIP_RETURN(launch_fill_dense_ordered(a, block_begin, block_end, (hipStream_t)stream));
}

int copy_texel_segments(const float* const src[4], float* const dst[4], const size_t n[4], float* const r_out[4],
                        void* stream) {
    if (int rc = need_device()) return rc;
    CopySegments c;
    memset(&c, 0, sizeof(c));
    for (int i = 0; i < 4; ++i) {
        if (n[i] >= (1ull << 32)) return set_error(SDFV_ERR_INVALID_ARGUMENT, "segment too large");
        if (n[i] == 0) continue;
        if (int rc = check_texel_alignment(src[i], dst[i])) return rc;  // the kernel moves float4 texels
        if (r_out && check_word_aligned("r_out", r_out[i])) return SDFV_ERR_INVALID_ARGUMENT;
        c.src[i] = reinterpret_cast<const float4*>(src[i]);
        c.dst[i] = reinterpret_cast<float4*>(dst[i]);
        c.n[i] = (uint32_t)n[i];
        c.r_out[i] = r_out ? r_out[i] : nullptr;
    }
    SDFV_HIP_RETURN(launch_copy_segments(c, (hipStream_t)stream));
}

int extract_distance(const float* tex0, float* dist, size_t n, void* stream) {
    if (n == 0) return SDFV_OK;
    if (int rc = check_texel_alignment(tex0)) return rc;  // read as float4 texels
    if (int rc = check_word_aligned("dist", dist)) return rc;
    if (int rc = need_device()) return rc;
    SDFV_HIP_RETURN(launch_commit_distance(tex0, dist, n, (hipStream_t)stream));
}

int fill_grid_signalling_start(const sdfv_demo_params* params, uint32_t sdf_id, const sdfv_grid* grid, float* tex0,
                               float* tex1, float* dist, uint32_t* signal, uint32_t value, void* stream) {
    if (int rc = check_params(params, sdf_id)) return rc;
    if (int rc = check_grid(grid)) return rc;
    if (int rc = check_textures(tex0, tex1)) return rc;
    if (int rc = need_device()) return rc;
    if (int rc = check_word_aligned("dist", dist)) return rc;
    FillArgs a = make_fill_args(*params, sdf_id, *grid, tex0, tex1);
    a.dist = dist;
    a.signal = signal;
    a.signal_value = value;
    if (int rc = check_one_launch(a)) return rc;
    SDFV_HIP_RETURN(launch_fill_dense(a, fill_launch_config(dist != nullptr), (hipStream_t)stream));
}
}  // namespace sdfv

#pragma GCC visibility push(default)
extern "C" {

int sdfv_grid_init(const sdfv_grid* grid, float* tex0, float* tex1, void* stream) {
    if (int rc = check_grid(grid)) return rc;
    if (int rc = check_textures(tex0, tex1)) return rc;
    if (int rc = need_device()) return rc;
    SDFV_HIP_RETURN(sdfv::launch_grid_init(tex0, tex1, slab_voxels(grid), air_dist(), (hipStream_t)stream));
}

int sdfv_grid_init_unvisited(const sdfv_grid* grid, uint32_t step, float* tex0, float* tex1, float* dist, void* stream) {
    return sdfv_grid_init_unvisited_ex(grid, step, tex0, tex1, dist, 0u, stream);
}

int sdfv_grid_init_unvisited_ex(const sdfv_grid* grid, uint32_t step, float* tex0, float* tex1, float* dist, uint32_t flags,
                                void* stream) {
    if (int rc = check_grid(grid)) return rc;
    if (flags & ~SDFV_PASS_VOLUME_INTERLEAVED) return set_error(SDFV_ERR_INVALID_ARGUMENT, "unknown flags 0x%x", flags);
    if ((flags & SDFV_PASS_VOLUME_INTERLEAVED) && dist && ((grid->dims[1] & 1u) || ((uintptr_t)dist & 7)))
        return set_error(SDFV_ERR_INVALID_ARGUMENT, "the interleaved volume pairs rows: H even, 8-byte aligned");
    if (int rc = need_textures(tex0, tex1)) return rc;
    if (step & (step - 1)) return set_error(SDFV_ERR_INVALID_ARGUMENT, "step %u is neither 0 nor a power of two", step);
    if (int rc = check_texel_alignment(tex0, tex1)) return rc;
    if (int rc = check_word_aligned("dist", dist)) return rc;
    if (int rc = need_device()) return rc;
    if (step == 1) return SDFV_OK;  // a step-1 pass wrote every row
    SDFV_HIP_RETURN(sdfv::launch_grid_init_unvisited(tex0, tex1, dist, grid->dims[0], grid->dims[1], grid->z_begin,
                                              grid->z_end - grid->z_begin, step, air_dist(),
                                              (flags & SDFV_PASS_VOLUME_INTERLEAVED) ? 1u : 0u, (hipStream_t)stream));
}

int sdfv_fill_grid_commit(const sdfv_demo_params* params, uint32_t sdf_id, const sdfv_grid* grid, float* tex0,
                          float* tex1, float* dist, void* stream) {
    if (int rc = check_params(params, sdf_id)) return rc;
    if (int rc = check_grid(grid)) return rc;
    if (int rc = check_textures(tex0, tex1)) return rc;
    if (int rc = check_word_aligned("dist", dist)) return rc;
    if (int rc = need_device()) return rc;
    sdfv::FillArgs a = make_fill_args(*params, sdf_id, *grid, tex0, tex1);
    a.dist = dist;
    if (int rc = check_one_launch(a)) return rc;
    SDFV_HIP_RETURN(sdfv::launch_fill_dense(a, fill_launch_config(dist != nullptr), (hipStream_t)stream));
}

int sdfv_fill_grid(const sdfv_demo_params* params, uint32_t sdf_id, const sdfv_grid* grid, float* tex0, float* tex1,
                   void* stream) {
    return sdfv_fill_grid_commit(params, sdf_id, grid, tex0, tex1, nullptr, stream);
}

int sdfv_fill_grid_pass_ex(const sdfv_demo_params* params, uint32_t sdf_id, const sdfv_grid* grid, uint32_t step,
                           const float* changed_box, float* tex0, float* tex1, float* dist, uint32_t flags, void* stream) {
    if (int rc = check_params(params, sdf_id)) return rc;
    if (int rc = check_grid(grid)) return rc;
    if (int rc = need_textures(tex0, tex1)) return rc;
    if (step == 0 || (step & (step - 1))) return set_error(SDFV_ERR_INVALID_ARGUMENT, "step %u is not a power of two", step);
    if (flags & ~(SDFV_PASS_FRESH_GRID | SDFV_PASS_SAME_LOAD | SDFV_PASS_VIRGIN_GRID | SDFV_PASS_VOLUME_INTERLEAVED | SDFV_PASS_EXPECT_NOOP))
        return set_error(SDFV_ERR_INVALID_ARGUMENT, "unknown pass flags 0x%x", flags);
    if (int rc = check_interleaved_volume(grid, dist, flags)) return rc;
    if ((flags & SDFV_PASS_VIRGIN_GRID) && changed_box)
        return set_error(SDFV_ERR_INVALID_ARGUMENT, "SDFV_PASS_VIRGIN_GRID with a changed box: a box test reads the grid (sdfv_grid_init_unvisited first)");
    if (int rc = check_texel_alignment(tex0, tex1)) return rc;
    if (int rc = check_word_aligned("dist", dist)) return rc;
    if (int rc = need_device()) return rc;
    sdfv::FillArgs a = make_fill_args(*params, sdf_id, *grid, tex0, tex1);
    a.dist_ilv = (flags & SDFV_PASS_VOLUME_INTERLEAVED) ? 1u : 0u;
    // what the caller KNOWS about the grid (the layout bit and the hint say nothing about update_required)
    const uint32_t knowledge = flags & ~(SDFV_PASS_VOLUME_INTERLEAVED | SDFV_PASS_EXPECT_NOOP);
    sdfv::PassArgs p;
    memset(&p, 0, sizeof(p));
    p.step = step;
    p.nx = (a.W + step - 1) / step;  // loading.rs:82: ceil(limit / step) visits per axis
    p.ny = (a.H + step - 1) / step;
    p.z_first = ((grid->z_begin + step - 1) / step) * step;
    p.nz = p.z_first < grid->z_end ? (grid->z_end - p.z_first + step - 1) / step : 0;
    p.has_box = changed_box != nullptr;
    p.dist = dist;
    if (changed_box) memcpy(p.box, changed_box, sizeof(p.box));
    // Does update_required (scene/sdf/mod.rs:184-190) hold for EVERY visited voxel?  Then the pass reads nothing.
    //  * the caller says so (flags): a fresh grid is all AIR_DIST; within one load a stored voxel already holds what this pass
    //    would write;
    //  * the changed box contains every voxel of the slab -- decided on the voxels' own first and last coordinates per axis
    //    (the kernels' arithmetic: idx / (dim - 1) * size + min, three roundings; monotonic in idx, so the ends decide; a NaN
    //    coordinate fails the comparison and keeps the general path).  The demo reports its whole bounding box on every
    //    parameter edit (demo/mod.rs:135-144), so its edits take this path.
    bool covers = changed_box != nullptr;
    for (int i = 0; i < 3 && covers; ++i) {
        const uint32_t first_idx = i == 2 ? grid->z_begin : 0u, last_idx = i == 2 ? grid->z_end - 1 : grid->dims[i] - 1;
        float first = (float)first_idx / a.dm1[i];
        first = first * a.bb_size[i];
        first = first + a.bb_min[i];
        float last = (float)last_idx / a.dm1[i];
        last = last * a.bb_size[i];
        last = last + a.bb_min[i];
        covers = first >= changed_box[i] && first <= changed_box[3 + i] && last >= changed_box[i] && last <= changed_box[3 + i];
    }
    p.fresh = (flags & SDFV_PASS_FRESH_GRID) ? 1u : 0u;
    p.virgin = (flags & SDFV_PASS_VIRGIN_GRID) ? 1u : 0u;
    p.index_limit = g_options.pass_index_limit;
    p.no_adaptive = g_options.pass_form == 1 ? 1u : 0u;
    // The scan's loads.  Auto: nontemporal when the caller expects a no-op pass AND the volume is larger than the last-level
    // cache -- a smaller one is still resident from the fill that wrote it, and cached loads hit (same box, tools/pass_loads_ab.py:
    // no-op pass at 512^3 0.128 -> 0.085 ms with nt loads, at 256^3 0.0128 -> 0.0150; passes that update most voxels +7..13 %).
    const uint64_t volume_bytes = slab_voxels(grid) * 4u, llc = device_facts().last_level_cache_bytes;
    const bool hinted = (flags & SDFV_PASS_EXPECT_NOOP) != 0 && (llc == 0 || volume_bytes > llc);
    p.stream_loads = g_options.pass_loads == 0 ? (hinted ? 1u : 0u) : (g_options.pass_loads == 2 ? 1u : 0u);
    p.all_required = (knowledge != 0 || covers) ? 1u : 0u;
    SDFV_HIP_RETURN(sdfv::launch_fill_pass(a, p, fill_launch_config(dist != nullptr), (hipStream_t)stream));
}

int sdfv_pack_samples(const sdfv_grid* grid, uint64_t index_base, const uint32_t* indices, const sdfv_sample* samples, size_t n,
                      float* tex0, float* tex1, float* dist, uint32_t flags, void* stream) {
    if (int rc = check_grid(grid)) return rc;
    if (int rc = need_textures(tex0, tex1)) return rc;
    if (n && !samples) return set_error(SDFV_ERR_INVALID_ARGUMENT, "samples is NULL");
    if (flags & ~SDFV_PASS_VOLUME_INTERLEAVED) return set_error(SDFV_ERR_INVALID_ARGUMENT, "unknown flags 0x%x", flags);
    if (int rc = check_interleaved_volume(grid, dist, flags)) return rc;
    if (int rc = check_texel_alignment(tex0, tex1)) return rc;
    if (int rc = check_word_aligned("samples, indices and dist", dist, samples, indices)) return rc;
    if (int rc = need_device()) return rc;
    sdfv::PackArgs a;
    memset(&a, 0, sizeof(a));
    a.samples = samples;
    a.indices = indices;
    a.index_base = index_base;
    a.n = n;
    a.n_voxels = slab_voxels(grid);
    a.W = grid->dims[0];
    a.tex0 = reinterpret_cast<float4*>(tex0);
    a.tex1 = tex1;
    a.dist = dist;
    a.dist_ilv = (flags & SDFV_PASS_VOLUME_INTERLEAVED) ? 1u : 0u;
    a.srgb_round = g_options.ext_srgb_quant;
    SDFV_HIP_RETURN(sdfv::launch_pack_samples(a, (hipStream_t)stream));
}

int sdfv_commit_distance(const sdfv_grid* grid, const float* tex0, float* dist, void* stream) {
    if (int rc = check_grid(grid)) return rc;
    if (!tex0 || !dist) return set_error(SDFV_ERR_INVALID_ARGUMENT, "NULL buffer");
    if (int rc = check_texel_alignment(tex0)) return rc;
    if (int rc = check_word_aligned("dist", dist)) return rc;
    if (int rc = need_device()) return rc;
    SDFV_HIP_RETURN(sdfv::launch_commit_distance(tex0, dist, slab_voxels(grid), (hipStream_t)stream));
}

int sdfv_commit_pairs(const sdfv_grid* grid, const float* dist, float* pairs, void* stream) {
    if (int rc = check_grid(grid)) return rc;
    if (!dist || !pairs) return set_error(SDFV_ERR_INVALID_ARGUMENT, "dist or pairs is NULL");
    if (((uintptr_t)dist & 3) || ((uintptr_t)pairs & 7)) return set_error(SDFV_ERR_INVALID_ARGUMENT, "dist: 4-byte, pairs: 8-byte aligned");
    if (grid->z_begin != 0 || grid->z_end != grid->dims[2])
        return set_error(SDFV_ERR_INVALID_ARGUMENT, "the pair volume is built over the whole grid (the march reads the whole grid)");
    if (int rc = need_device()) return rc;
    SDFV_HIP_RETURN(sdfv::launch_commit_pairs(dist, pairs, grid->dims[0], grid->dims[1], slab_voxels(grid), (hipStream_t)stream));
}

int sdfv_commit_interleaved(const sdfv_grid* grid, const float* dist, float* ilv, void* stream) {
    if (int rc = check_grid(grid)) return rc;
    if (!dist || !ilv) return set_error(SDFV_ERR_INVALID_ARGUMENT, "dist or ilv is NULL");
    if (((uintptr_t)dist & 3) || ((uintptr_t)ilv & 7)) return set_error(SDFV_ERR_INVALID_ARGUMENT, "dist: 4-byte, ilv: 8-byte aligned");
    if (grid->z_begin != 0 || grid->z_end != grid->dims[2])
        return set_error(SDFV_ERR_INVALID_ARGUMENT, "the interleaved volume is built over the whole grid");
    if (grid->dims[1] & 1) return set_error(SDFV_ERR_INVALID_ARGUMENT, "the interleaved volume pairs rows: H = %u is odd", grid->dims[1]);
    if (int rc = need_device()) return rc;
    SDFV_HIP_RETURN(sdfv::launch_commit_interleaved(dist, ilv, grid->dims[0], slab_voxels(grid), (hipStream_t)stream));
}

int sdfv_program_fill_grid_commit(const sdfv_program* p, const sdfv_grid* grid, float* tex0, float* tex1, float* dist,
                                  uint32_t flags, void* stream) {
    if (!p) return set_error(SDFV_ERR_INVALID_ARGUMENT, "program is NULL");
    if (int rc = check_grid(grid)) return rc;
    if (int rc = need_textures(tex0, tex1)) return rc;
    if (flags & ~SDFV_PASS_VOLUME_INTERLEAVED) return set_error(SDFV_ERR_INVALID_ARGUMENT, "unknown flags 0x%x", flags);
    if (int rc = check_interleaved_volume(grid, dist, flags)) return rc;
    if (int rc = check_texel_alignment(tex0, tex1)) return rc;
    if (int rc = check_word_aligned("dist", dist)) return rc;
    if (int rc = need_device()) return rc;
    sdfv::ProgramFillArgs a;
    memset(&a, 0, sizeof(a));
    sdfv::ProgramKernels compiled;
    if (int rc = program_compiled_kernels(p, SDFV_COMPILE_FILL, &compiled)) return rc;
    if (int rc = program_on_device(p, &a.ops, &a.n_ops)) return rc;
    set_grid_fill_args(a, *grid, tex0, tex1, dist, (flags & SDFV_PASS_VOLUME_INTERLEAVED) ? 1u : 0u);
    a.nontemporal = fill_launch_config(dist != nullptr).nontemporal ? 1u : 0u;
    if (int rc = check_one_launch(a)) return rc;
    SDFV_HIP_RETURN(sdfv::launch_program_fill(a, compiled, (hipStream_t)stream));
}

int sdfv_program_grid_pass(const sdfv_program* p, const sdfv_grid* grid, uint32_t step, const float* changed_box, float* tex0,
                           float* tex1, float* dist, uint32_t flags, void* stream) {
    if (!p) return set_error(SDFV_ERR_INVALID_ARGUMENT, "program is NULL");
    if (int rc = check_grid(grid)) return rc;
    if (int rc = need_textures(tex0, tex1)) return rc;
    if (step == 0 || (step & (step - 1))) return set_error(SDFV_ERR_INVALID_ARGUMENT, "step %u is not a power of two", step);
    if (flags & ~(SDFV_PASS_FRESH_GRID | SDFV_PASS_SAME_LOAD | SDFV_PASS_VIRGIN_GRID | SDFV_PASS_VOLUME_INTERLEAVED | SDFV_PASS_EXPECT_NOOP))
        return set_error(SDFV_ERR_INVALID_ARGUMENT, "unknown pass flags 0x%x", flags);
    if (flags & SDFV_PASS_VIRGIN_GRID)
        return set_error(SDFV_ERR_INVALID_ARGUMENT, "SDFV_PASS_VIRGIN_GRID is not supported for programs (sdfv_grid_init first)");
    if (int rc = check_interleaved_volume(grid, dist, flags)) return rc;
    if (int rc = check_texel_alignment(tex0, tex1)) return rc;
    if (int rc = check_word_aligned("dist", dist)) return rc;
    if (slab_voxels(grid) > (1ull << 32))
        return set_error(SDFV_ERR_INVALID_ARGUMENT, "a program pass takes slabs of at most 2^32 voxels, not %llu",
                         (unsigned long long)slab_voxels(grid));
    if (int rc = need_device()) return rc;
    const uint32_t ilv = (flags & SDFV_PASS_VOLUME_INTERLEAVED) ? 1u : 0u;
    sdfv::ProgramFillArgs f;
    memset(&f, 0, sizeof(f));
    if (int rc = program_on_device(p, &f.ops, &f.n_ops)) return rc;
    set_grid_fill_args(f, *grid, tex0, tex1, dist, ilv);
    sdfv::ProgramPassArgs a;
    memset(&a, 0, sizeof(a));
    a.ops = f.ops;
    a.n_ops = f.n_ops;
    set_grid_fill_args(a, *grid, tex0, tex1, dist, ilv);
    a.step = step;
    a.nx = (a.W + step - 1) / step;  // loading.rs:82: ceil(limit / step) visits per axis
    a.ny = (a.H + step - 1) / step;
    a.z_first = ((grid->z_begin + step - 1) / step) * step;
    a.nz = a.z_first < grid->z_end ? (grid->z_end - a.z_first + step - 1) / step : 0;
    if ((uint64_t)a.nx * a.ny * a.nz == 0) return SDFV_OK;
    // update_required is known to hold for every visited voxel (sdfv_fill_grid_pass_ex: FRESH_GRID, SAME_LOAD): the sub-box is the
    // whole lattice.  Otherwise it is the lattice points INSIDE the closed changed box: voxel_coord -- three separately rounded
    // steps, spelled out below as the kernels compute them (this file is built with -ffp-contract=off) -- does not decrease with
    // the index, so per axis the points with coord >= lo are a tail of the lattice, those with coord <= hi a head, and two
    // bisections find where they meet.  A NaN bound (or coordinate) fails both compares: the sub-box is empty.
    const uint32_t n_axis[3] = {a.nx, a.ny, a.nz};
    uint32_t first[3] = {0, 0, 0}, count[3] = {a.nx, a.ny, a.nz};
    if (!(flags & (SDFV_PASS_FRESH_GRID | SDFV_PASS_SAME_LOAD))) {
        for (int i = 0; i < 3; ++i) {
            if (!changed_box) {
                count[i] = 0;
                continue;
            }
            auto coord = [&](uint32_t k) {
                float c = (float)((i == 2 ? a.z_first : 0u) + k * step);
                c = c / a.dm1[i];
                c = c * a.bb_size[i];
                c = c + a.bb_min[i];
                return c;
            };
            // the first k in [0, n] for which `reached(k)` holds, given that it holds on a tail of the lattice
            auto bisect = [&](auto reached) {
                uint32_t lo = 0, hi = n_axis[i];
                while (lo < hi) {
                    const uint32_t mid = lo + (hi - lo) / 2;
                    if (reached(mid)) hi = mid;
                    else lo = mid + 1;
                }
                return lo;
            };
            const uint32_t begin = bisect([&](uint32_t k) { return coord(k) >= changed_box[i]; });
            const uint32_t end = bisect([&](uint32_t k) { return !(coord(k) <= changed_box[3 + i]); });
            first[i] = begin;
            count[i] = end > begin ? end - begin : 0;
        }
    }
    a.bx0 = first[0], a.by0 = first[1], a.bz0 = first[2];
    a.bnx = count[0], a.bny = count[1], a.bnz = count[2];
    const bool whole = a.bnx == a.nx && a.bny == a.ny && a.bnz == a.nz;
    // ... and a step-1 pass over the whole lattice is the dense program fill, where that writes the same tex1.a: with a volume
    // (AIR_DIST by contract) or over a fresh grid (AIR_DIST is what it holds)
    if (whole && step == 1 && (dist || (flags & SDFV_PASS_FRESH_GRID)) && (uint64_t)f.H * f.slab_d <= 0x7fffffffull && f.W <= 0x7fffffffu) {
        f.nontemporal = fill_launch_config(dist != nullptr).nontemporal ? 1u : 0u;
        sdfv::ProgramKernels compiled;  // the one place where a pass IS the dense fill: a compiled handle's FILL route
        if (int rc = program_compiled_kernels(p, SDFV_COMPILE_FILL, &compiled)) return rc;
        SDFV_HIP_RETURN(sdfv::launch_program_fill(f, compiled, (hipStream_t)stream));
    }
    SDFV_HIP(sdfv::launch_program_pass_box(a, (hipStream_t)stream));
    if (whole) return SDFV_OK;
    // the scan's loads, as sdfv_fill_grid_pass_ex chooses them
    const uint64_t volume_bytes = slab_voxels(grid) * 4u, llc = device_facts().last_level_cache_bytes;
    const bool hinted = (flags & SDFV_PASS_EXPECT_NOOP) != 0 && (llc == 0 || volume_bytes > llc);
    a.stream_loads = g_options.pass_loads == 0 ? (hinted ? 1u : 0u) : (g_options.pass_loads == 2 ? 1u : 0u);
    SDFV_HIP_RETURN(sdfv::launch_program_pass_scan(a, (hipStream_t)stream));
}

}  // extern "C"
#pragma GCC visibility pop
