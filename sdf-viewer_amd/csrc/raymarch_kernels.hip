// raymarch_kernels.hip -- per-pixel sphere tracing of the voxel grid on gfx950:
// the fragment shader of the reference (src/app/scene/sdf/material.frag, whole file) as a HIP kernel.
//
// One thread per pixel.  A 64-lane wave covers an 8x8 pixel tile (neighbouring rays walk neighbouring
// texels, so the gathers of a trilinear fetch land in few cache lines); a 256-thread workgroup covers
// 16x16; blockIdx.z is the camera.  The march loop is wave-synchronous: each iteration ballots the lanes
// still marching and the wave leaves the loop as soon as the ballot is empty (early ray termination)
// instead of running the shader's fixed 255-iteration bound.
//
// texture(sampler3D) is restated in full fp32 (GL texel-centre convention, MirroredRepeat, mix() along
// x, then y, then z): hardware texture filtering uses low-precision fixed-point weights and would not
// hold the 1e-4 RGBA tolerance, so no hipTextureObject is used.  The march reads only tex0.r (or its
// compact copy); the full tex0/tex1 texels are fetched once, at the hit.
//
// Ray set-up: the reference rasterises the bbox cube and the fragment's `pos` is a point on its
// surface (scene/sdf/mod.rs:254-282, material.rs:75-81 Cull::None).  Here `pos` comes from a ray/AABB
// slab test through the pixel centre: the entry point when the camera is outside the box, the exit
// point when it is inside; pixels whose ray misses the box are transparent.
//
// What profiling says (profiles/, tools/wave_timing.py): a frame is latency-bound by its longest wave (one
// grazing ray, up to 255 dependent iterations, ~8 cycles per instruction for a lone wave on its SIMD) and a
// batch of cameras is VALU-issue-bound.  Both regimes pay per INSTRUCTION, so the fast kernels
// spend their effort on removing instructions from the per-iteration path without changing a single bit
// of the result (see march_fast); the general kernel keeps the shader's structure for every other case.
//
// This file: the frame kernel, its launcher and the camera staging kernel.  The texel sampler is march_sampler.h, the march
// loops march_loops.h and march_asm_loop.h, the workgroup-to-tile mapping march_tile_order.h, and everything decided on the
// host before a launch march_plan.h; the march over a z-slab is raymarch_slab_kernels.hip.
#include "raymarch_kernels.h"

#include <hip/hip_runtime.h>
#include <string.h>

#include "march_asm_loop.h"
#include "march_loops.h"
#include "march_plan.h"
#include "march_tile_order.h"

namespace sdfv {
namespace {

#ifdef SDFV_TUNING
__device__ __forceinline__ void stamp_wave(const RaymarchArgs& a, uint32_t bx, uint32_t by, uint32_t wave,
                                           unsigned long long t_start, unsigned long long t_start_rt, int iterations,
                                           unsigned long long covered_mask) {
    // indexed by the TILE (whatever workgroup rendered it): stamps of any tile order land in the same slots
    const uint32_t tiles_x = (a.width + 15) / 16, tiles_y = (a.rows_out + 15) / 16;
    const uint64_t wave_id = ((uint64_t)(blockIdx.z * tiles_y + by) * tiles_x + bx) * 4 + wave;
    a.wave_timing[wave_id * 4 + 0] = t_start;
    a.wave_timing[wave_id * 4 + 1] = __builtin_readcyclecounter();
    // bits 32..47 / 48..63: the 100 MHz real-time counter (one clock for the whole device; the cycle counters above are
    // per XCD) at the wave's start / end, modulo 2^16 ticks
    a.wave_timing[wave_id * 4 + 2] = (unsigned long long)(uint32_t)iterations | ((t_start_rt & 0xffffull) << 32) |
                                     ((__builtin_amdgcn_s_memrealtime() & 0xffffull) << 48);
    a.wave_timing[wave_id * 4 + 3] = covered_mask;
}
#endif

// MODE: kMarchGeneral .. kMarchIlv = 0 .. 4, what the march loop reads (raymarch_kernels.h); kMarchLattice = 5: the lattice
//       filter of a loading grid (march_lattice; LINEAR false, XF 0 or 1).
// XF:   0 = IEEE divide, 1 = exact power-of-two reciprocal, 2 = power-of-two extents and texture sizes.
// AUX:  the per-pixel march record is stored (and distanceFromOrigin accumulated).
#ifndef SDFV_RM_MIN_WAVES
#define SDFV_RM_MIN_WAVES 1
#endif
// NORMAL: sdfNormal's four taps are compiled in (always with the aux record; without it only for
// SDFV_OPT_RAYMARCH_KEEP_NORMAL).  A compile-time switch: the taps' 32 gathers with 64-bit addresses would otherwise set the
// register count of the kernel that never runs them (79 -> 72 VGPRs = one more wave per SIMD).
template <int MODE, bool LINEAR, int XF, bool SYMM, bool AUX, bool ASM = false, bool NORMAL = AUX>
__global__ __launch_bounds__(256, SDFV_RM_MIN_WAVES) void raymarch_kernel(RaymarchArgs a) {
    constexpr bool FAST = MODE != 0;
    static_assert(NORMAL || !AUX, "the aux record carries the normal");
#ifdef SDFV_TUNING
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#endif
    uint32_t bx = blockIdx.x, by = blockIdx.y;
#ifdef SDFV_TUNING
    if (a.tile_order) {  // 1-D launch over the tiles, in the order given
        const uint32_t tiles_x = (a.width + 15) / 16, t = a.tile_order[blockIdx.x];
        bx = t % tiles_x;
        by = t / tiles_x;
    } else
#endif
    // march_tile_of (march_tile_order.h), spelt out around the kernel's own `return`
    if (a.group_shift == 0 && a.rotate_columns) {
        bx = rotated_tile_column(blockIdx.x, blockIdx.y, blockIdx.z, gridDim.x);
    } else if (a.group_shift) {
        grouped_tile(a, blockIdx.x, bx, by);
        if (bx >= a.tiles_x || by >= a.tiles_y) return;  // padding of the last groups
    }
    uint32_t px, row;  // row of the output: within [y0, y1), or of the bands
    tile_pixel(bx, by, px, row);
    const uint32_t py = a.y0 + row + (row >> a.band_shift) * a.band_skip;  // band k of the set = rows [k << shift, ...) of the output
    const uint32_t cam_idx = blockIdx.z;
    const bool in_image = px < a.width && py < a.y1;
    // (two scalar-load sequences under a uniform branch; a reference chosen by `?:` would mix the address spaces)
    sdfv_camera cam;
    if (a.camera_list) cam = a.camera_list[cam_idx];
    else cam = a.cameras[cam_idx];
    const uint64_t out_index = ((uint64_t)cam_idx * a.rows_out + row) * a.width + px;
#ifdef SDFV_TUNING
    if (a.priority_map && a.priority_map[by * ((a.width + 15) / 16) + bx]) __builtin_amdgcn_s_setprio(3);
    const unsigned long long t_start = a.wave_timing ? __builtin_readcyclecounter() : 0ull;
    const unsigned long long t_start_rt = a.wave_timing ? __builtin_amdgcn_s_memrealtime() : 0ull;
#endif

    const V3 eye = mk(cam.eye[0], cam.eye[1], cam.eye[2]);
    const V3 d_raw = pixel_ray_raw(a.width, a.height, cam, px, py);

    // Conservative tile cull (the reference gets it from rasterising the box).  A ray that misses the box's
    // bounding sphere inflated by 1 % cannot be covered; if no lane of the wave can be covered, the wave
    // writes its transparent pixels and leaves before the divisions of the exact slab test.
    {
        const V3 m = sub(eye, mk(a.cull_center[0], a.cull_center[1], a.cull_center[2]));
        const float dd = d_raw.x * d_raw.x + d_raw.y * d_raw.y + d_raw.z * d_raw.z;
        const float mm = m.x * m.x + m.y * m.y + m.z * m.z;
        const float md = m.x * d_raw.x + m.y * d_raw.y + m.z * d_raw.z;
        const float r2 = a.cull_radius2;
        const bool miss = mm > r2 && (md >= 0.0f || mm * dd - md * md > r2 * dd);
        if (__ballot(in_image && !miss) == 0ull) {
            if (in_image) {
                store_color(a, out_index, make_float4(0.0f, 0.0f, 0.0f, 0.0f));
                if (AUX) {
                    sdfv_march_aux aux;
                    aux_clear(aux);
                    a.aux[out_index] = aux;
                }
            }
            if (in_image && a.depth) a.depth[out_index] = 1.0f;
#ifdef SDFV_TUNING
            if (a.wave_timing && lane == 0) stamp_wave(a, bx, by, wave, t_start, t_start_rt, 0, 0ull);
#endif
            return;
        }
    }

    const Tex tex0{a.tex0, (int)a.rp.tex_size[0], (int)a.rp.tex_size[1], (int)a.rp.tex_size[2], 0};
    const Tex tex1{a.tex1, tex0.w, tex0.h, tex0.d, 0};
    const float* tex0_r = reinterpret_cast<const float*>(a.tex0);
    V3 ray_origin, ray_dir;
    const bool covered = box_fragment_ray(a, eye, d_raw, in_image, ray_origin, ray_dir);

    // sdfRaycast(rayOrigin, rayDir, 256), material.frag:92-128
    V3 ray_pos = ray_origin;
    float dist_from_origin = 0.0f;
    int status = covered ? -1 : 0;  // -1 = out of steps unless something else ends the ray
    int steps = 0;
    int iterations = 0;
#ifdef SDFV_TUNING
    const unsigned long long t_loop0 = a.wave_timing ? __builtin_readcyclecounter() : 0ull;
#endif
    if constexpr (MODE == kMarchLattice) {
        march_lattice<XF, SYMM, AUX>(a, tex0, lattice_of(a, tex0), ray_dir, covered, ray_pos, dist_from_origin, status, steps, iterations);
    } else if constexpr (FAST && ASM) {
        march_asm<MODE, AUX>(a, tex0, ray_dir, covered, ray_pos, dist_from_origin, status, steps, iterations);
    } else if constexpr (FAST) {  // the C++ loop, where the hand-written one's specialisation does not apply
        march_fast<MODE, XF, SYMM, AUX>(a, tex0, ray_dir, covered, ray_pos, dist_from_origin, status, steps, iterations);
    } else {
        bool marching = covered;
        for (int i = 0; i < 255; ++i) {
            if (__ballot(marching) == 0ull) break;  // wave-level early termination
            ++iterations;
            if (marching) {
                if (oob_dist<false>(a, ray_pos) > 1e-4f) {
                    status = -2;
                    marching = false;
                } else {
                    float sample_dist = sample_r<LINEAR, XF, kMirror>(a, tex0_r, 4, tex0, ray_pos) - 1e-1f;
                    ++steps;
                    if (sample_dist < 1e-5f) {
                        status = 1;
                        marching = false;
                    } else {
                        dist_from_origin += sample_dist;
                        ray_pos = madd(ray_pos, ray_dir, sample_dist);
                    }
                }
            }
        }
    }

#ifdef SDFV_TUNING
    const unsigned long long t_loop1 = a.wave_timing ? __builtin_readcyclecounter() : 0ull;
#endif
    float4 rgba = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    float frag_depth = 1.0f;  // material.frag:147 (no hit); also where no fragment exists
    sdfv_march_aux aux;
    if (AUX) {
        aux_clear(aux);
        if (covered) aux_set_march(aux, status, steps, ray_pos, dist_from_origin);
    }
    if (status == 1) {
        // The fast kernels know the hit point is within 1e-4 of the box; the normal's taps are h further out,
        // a.fast_normal says whether floor(u) still stays in [-1, N-1] for them.
        float4 raw0;
        if constexpr (MODE == kMarchLattice) raw0 = gather_rgba(tex0.data, lattice_footprint(tex0, lattice_of(a, tex0), to_p01<XF>(a, ray_pos)));
        else raw0 = sample_rgba<LINEAR, XF, FAST ? kClamp : kMirror>(a, tex0, ray_pos);  // == the march's last sample
        // one texture's eight 16-byte corners at a time: both sets in flight together cost 6 more VGPRs (78: one wave per
        // SIMD less) and buy nothing even for single frames, which are not occupancy-limited -- measured 1 % SLOWER on
        // every view at 1080p / 256^3 and 4K / 512^3 (round 3 A/B, profiles/r03_hit_path_ab.json)
        V3 pos1 = ray_pos;
        asm volatile("" : "+v"(pos1.x) : "v"(raw0.x), "v"(raw0.y), "v"(raw0.z), "v"(raw0.w));  // same value, after raw0
        float4 raw1;  // material.frag:154
        if constexpr (MODE == kMarchLattice) raw1 = gather_rgba(tex1.data, lattice_footprint(tex1, lattice_of(a, tex1), to_p01<XF>(a, pos1)));
        else raw1 = sample_rgba<LINEAR, XF, FAST ? kClamp : kMirror>(a, tex1, pos1);
        rgba = shade(a.rp, raw0, raw1);
        if (a.depth) {  // gl_FragDepth, material.frag:180-181
            frag_depth = frag_depth_of(cam.bvp, ray_pos.x, ray_pos.y, ray_pos.z);
        }
        if (NORMAL) {
            // sdfNormal, material.frag:73-80
            const float h = tap_distance((float)tex0.w, (float)tex0.h, (float)tex0.d, a.rp.lod_dist_between_samples);
            const V3 p1 = normal_tap(ray_pos, h, 0), p2 = normal_tap(ray_pos, h, 1), p3 = normal_tap(ray_pos, h, 2), p4 = normal_tap(ray_pos, h, 3);
            float d1, d2, d3, d4;
            if constexpr (MODE == kMarchLattice) {  // the taps go through the lattice footprint as well
                const Lattice g = lattice_of(a, tex0);
                d1 = gather_r(tex0_r, 4, lattice_footprint(tex0, g, to_p01<XF>(a, p1))) - 1e-1f;
                d2 = gather_r(tex0_r, 4, lattice_footprint(tex0, g, to_p01<XF>(a, p2))) - 1e-1f;
                d3 = gather_r(tex0_r, 4, lattice_footprint(tex0, g, to_p01<XF>(a, p3))) - 1e-1f;
                d4 = gather_r(tex0_r, 4, lattice_footprint(tex0, g, to_p01<XF>(a, p4))) - 1e-1f;
            } else if (MODE >= kMarchDist && a.dist && a.fast_normal) {  // the taps read the compact distance volume too
                d1 = sample_r<true, XF, kClamp>(a, a.dist, 1, tex0, p1) - 1e-1f;
                d2 = sample_r<true, XF, kClamp>(a, a.dist, 1, tex0, p2) - 1e-1f;
                d3 = sample_r<true, XF, kClamp>(a, a.dist, 1, tex0, p3) - 1e-1f;
                d4 = sample_r<true, XF, kClamp>(a, a.dist, 1, tex0, p4) - 1e-1f;
            } else if (FAST && a.fast_normal) {
                d1 = sample_r<LINEAR, XF, kClamp>(a, tex0_r, 4, tex0, p1) - 1e-1f;
                d2 = sample_r<LINEAR, XF, kClamp>(a, tex0_r, 4, tex0, p2) - 1e-1f;
                d3 = sample_r<LINEAR, XF, kClamp>(a, tex0_r, 4, tex0, p3) - 1e-1f;
                d4 = sample_r<LINEAR, XF, kClamp>(a, tex0_r, 4, tex0, p4) - 1e-1f;
            } else {
                d1 = sample_r<LINEAR, XF, kMirror>(a, tex0_r, 4, tex0, p1) - 1e-1f;
                d2 = sample_r<LINEAR, XF, kMirror>(a, tex0_r, 4, tex0, p2) - 1e-1f;
                d3 = sample_r<LINEAR, XF, kMirror>(a, tex0_r, 4, tex0, p3) - 1e-1f;
                d4 = sample_r<LINEAR, XF, kMirror>(a, tex0_r, 4, tex0, p4) - 1e-1f;
            }
            const V3 n = normal_of_taps(d1, d2, d3, d4);
            if (AUX) {
                aux_set_hit(aux, raw0, raw1, n, frag_depth_of(cam.bvp, ray_pos.x, ray_pos.y, ray_pos.z));
            } else {
                // keep the normal live when nobody stores it: the shader text computes it per hit
                asm volatile("" ::"v"(n.x), "v"(n.y), "v"(n.z));
            }
        }
    }

#ifdef SDFV_TUNING
    // slot 3: cycles before the march loop (ray set-up) | cycles of the loop << 32; what is left of end - start is the hit's
    // texel gathers and shading
    if (a.wave_timing && lane == 0)
        stamp_wave(a, bx, by, wave, t_start, t_start_rt, iterations, ((t_loop0 - t_start) & 0xffffffffull) | ((t_loop1 - t_loop0) << 32));
#endif
    if (in_image) {
        store_color(a, out_index, rgba);
        if (a.depth) a.depth[out_index] = frag_depth;
        if (AUX) a.aux[out_index] = aux;
    }
}

constexpr uint32_t kStoreChunk = 32;  // 32 x 120 B + the two scalars: 3 856 B of kernel arguments
struct CameraChunk {
    sdfv_camera c[kStoreChunk];
};
static_assert(sizeof(sdfv_camera) % 4 == 0, "cameras are copied word by word");
__global__ __launch_bounds__(256) void store_cameras_kernel(CameraChunk chunk, uint32_t words, uint32_t* __restrict__ out) {
    const uint32_t* src = reinterpret_cast<const uint32_t*>(&chunk);
    for (uint32_t w = threadIdx.x; w < words; w += 256) out[w] = src[w];
}
}  // namespace

hipError_t launch_store_cameras(const sdfv_camera* host, uint32_t n, sdfv_camera* device, hipStream_t stream) {
    for (uint32_t c0 = 0; c0 < n; c0 += kStoreChunk) {
        const uint32_t nc = n - c0 < kStoreChunk ? n - c0 : kStoreChunk;
        CameraChunk chunk;
        memcpy(chunk.c, host + c0, nc * sizeof(sdfv_camera));
        hipLaunchKernelGGL(store_cameras_kernel, dim3(1), dim3(256), 0, stream, chunk, (uint32_t)(nc * sizeof(sdfv_camera) / 4),
                           reinterpret_cast<uint32_t*>(device + c0));
        if (hipError_t e = hipGetLastError()) return e;
    }
    return hipSuccess;
}

namespace {

// AUX: the record is stored (and carries the normal); else NORMAL only for SDFV_OPT_RAYMARCH_KEEP_NORMAL.  The dynamic LDS is
// unused: it caps the resident waves (lds_cap_for).
template <int MODE, bool LINEAR, int XF, bool SYMM, bool ASM>
void launch_variant(const RaymarchArgs& a, dim3 grid, hipStream_t stream) {
    if (a.aux)
        hipLaunchKernelGGL((raymarch_kernel<MODE, LINEAR, XF, SYMM, true, ASM>), grid, dim3(256), a.lds_cap_bytes, stream, a);
    else if (a.compute_normal)
        hipLaunchKernelGGL((raymarch_kernel<MODE, LINEAR, XF, SYMM, false, ASM, true>), grid, dim3(256), a.lds_cap_bytes, stream, a);
    else
        hipLaunchKernelGGL((raymarch_kernel<MODE, LINEAR, XF, SYMM, false, ASM>), grid, dim3(256), a.lds_cap_bytes, stream, a);
}

// One case per entry of SDFV_MARCH_VARIANTS (march_plan.h), which instantiates them.
hipError_t launch_selected(const MarchKernel& k, const RaymarchArgs& a, dim3 grid, hipStream_t stream) {
#define SDFV_VARIANT(MODE, LINEAR, XF, SYMM, ASM) \
    case variant_key(MODE, LINEAR, XF, SYMM, ASM): launch_variant<MODE, LINEAR, XF, SYMM, ASM>(a, grid, stream); break;
    switch (variant_key(k.mode, k.linear, k.xf, k.symm, k.hand_written_loop)) {
        SDFV_MARCH_VARIANTS(SDFV_VARIANT)
    default: return hipErrorInvalidValue;  // select_march_kernel names no other (tests/c/march_plan_check.cpp)
    }
#undef SDFV_VARIANT
    return hipGetLastError();
}

}  // namespace

hipError_t launch_raymarch(const RaymarchArgs& a, hipStream_t stream, uint32_t lod_filter) {
    const MarchLaunch p = plan_march_launch(a, lod_filter);
    if (p.grid.x == 0 || p.grid.y == 0 || p.grid.z == 0) return hipSuccess;
    return launch_selected(p.kernel, p.args, p.grid, stream);
}

}  // namespace sdfv
