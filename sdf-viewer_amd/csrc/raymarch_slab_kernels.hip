// raymarch_slab_kernels.hip -- the march over a z-slab of the grid (multi-GPU: the grid stays sharded across GPUs and rays
// are handed between ranks): the kernel of one round and its launcher.  The sampler is the frame kernel's (march_sampler.h).
#include <hip/hip_runtime.h>

#include "march_sampler.h"

namespace sdfv {
namespace {

// ---- march over a z-slab: the grid stays sharded across GPUs and rays are handed between ranks ----------------
// Same arithmetic, same order as the MODE 0 loop of raymarch_kernel (hence as the oracle); what differs is WHO executes an
// iteration: the rank whose slab holds the ray's cell.  Texel z-indices are clamped (the launcher requires the
// fast_index condition) and rebased to the first resident slice.
template <int XF, bool AUX>
__global__ __launch_bounds__(256) void raymarch_slab_kernel(RaymarchArgs a, SlabMarchArgs s) {
    const bool device_counts = s.in_count[0] != nullptr || s.in_count[1] != nullptr;
    const bool first_round = s.in == nullptr && !device_counts;
    const uint32_t gid = blockIdx.x * 256 + threadIdx.x;
    const sdfv_camera& cam = a.cameras[0];
    uint32_t px, py;
    bool live;            // this thread carries a ray (first round: a pixel of the image)
    int i = 0;
    V3 ray_pos = mk(0.0f, 0.0f, 0.0f);
    float dist_from_origin = 0.0f;
    if (first_round) {
        // 8x8 pixel tiles per wave, like the single-GPU kernel
        const uint32_t tiles_x = (a.width + 7) / 8, tile = gid >> 6, lane = gid & 63;
        px = (tile % tiles_x) * 8 + (lane & 7);
        py = (tile / tiles_x) * 8 + (lane >> 3);
        live = px < a.width && py < a.height;
    } else {
        sdfv_ray_state st{};
        if (device_counts) {
            // the neighbours' ray buffers as they arrived: their counts are read here, on the device
            const uint32_t n0 = s.in_count[0] ? min(*s.in_count[0], s.capacity) : 0u;
            const uint32_t n1 = s.in_count[1] ? min(*s.in_count[1], s.capacity) : 0u;
            live = gid < n0 + n1;
            if (live) st = gid < n0 ? s.in_rays[0][gid] : s.in_rays[1][gid - n0];
        } else {
            live = gid < s.n_in;
            st = s.in[live ? gid : 0];
        }
        // a continuation round is launched for the most rays that COULD arrive (their number is only known on the device):
        // waves beyond the lists leave before the ray set-up
        if (__ballot(live) == 0ull) return;
        px = st.pixel % a.width;
        py = st.pixel / a.width;
        i = (int)st.iteration;
        ray_pos = mk(st.pos[0], st.pos[1], st.pos[2]);
        dist_from_origin = st.t;
    }
    const uint32_t pixel = py * a.width + px;
    const V3 eye = mk(cam.eye[0], cam.eye[1], cam.eye[2]);
    V3 ray_origin, ray_dir;
    const bool covered = box_fragment_ray(a, eye, pixel_ray_raw(a.width, a.height, cam, px, py), live, ray_origin, ray_dir);
    const Tex tex{a.tex0, (int)a.rp.tex_size[0], (int)a.rp.tex_size[1], (int)a.rp.tex_size[2], (int)s.z_lo};
    const float* dist_r = reinterpret_cast<const float*>(a.tex0);

    bool marching = live && covered;
    if (first_round) {
        ray_pos = ray_origin;
        // every pixel of this rank's image starts transparent; the rank a ray ends on overwrites it
        if (live) {
            a.rgba[pixel] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (AUX) {
                sdfv_march_aux z;
                aux_clear(z);
                z.depth = 0.0f;  // summed over ranks; the caller restores 1.0 where no rank reports a status
                a.aux[pixel] = z;
            }
        }
        // a ray that starts in another rank's slab is that rank's to begin
        int k0c;
        (void)footprint<kClampSlab>(tex, to_p01<XF>(a, ray_pos), k0c);
        marching = marching && k0c >= (int)s.own_begin && k0c < (int)s.own_end;
    }
    const bool mine = marching;  // this rank reports the ray's end unless it hands the ray over
    int status = 0, steps = 0;
    bool exported = false;
    int export_dir = 0;
    Footprint hit_fp{};
    // one-cell cache (round 4), as in the single-GPU kernels: the eight corner distances are re-fetched only when the ray
    // enters another cell -- (o000, o111) identify the cell with its clamps -- and the longest rays are the ones that crawl
    uint32_t cell0 = 0xffffffffu, cell7 = 0xffffffffu;
    float c000 = 0.0f, c100 = 0.0f, c010 = 0.0f, c110 = 0.0f, c001 = 0.0f, c101 = 0.0f, c011 = 0.0f, c111 = 0.0f;
    for (;;) {
        marching = marching && i < 255;  // sdfRaycast's `for (i < 255)`; a ray that runs out keeps status 0 for now
        if (__ballot(marching) == 0ull) break;
        if (!marching) continue;
        if (oob_dist<false>(a, ray_pos) > 1e-4f) {  // material.frag:106-109
            status = -2;
            steps = i;
            marching = false;
            continue;
        }
        int k0c;
        const Footprint f = footprint<kClampSlab>(tex, to_p01<XF>(a, ray_pos), k0c);
        if (k0c < (int)s.own_begin || k0c >= (int)s.own_end) {
            // the cell belongs to a z-neighbour: hand the ray over exactly as it is -- after the loop, a wave at a time
            export_dir = k0c < (int)s.own_begin ? 0 : 1;
            exported = true;
            marching = false;
            continue;
        }
        if (f.o000 != cell0 || f.o111 != cell7) {
            cell0 = f.o000;
            cell7 = f.o111;
            c000 = dist_r[(uint64_t)f.o000 * 4]; c100 = dist_r[(uint64_t)f.o100 * 4];
            c010 = dist_r[(uint64_t)f.o010 * 4]; c110 = dist_r[(uint64_t)f.o110 * 4];
            c001 = dist_r[(uint64_t)f.o001 * 4]; c101 = dist_r[(uint64_t)f.o101 * 4];
            c011 = dist_r[(uint64_t)f.o011 * 4]; c111 = dist_r[(uint64_t)f.o111 * 4];
        }
        const float sample_dist = trilerp(c000, c100, c010, c110, c001, c101, c011, c111, f.ax, f.ay, f.az) - 1e-1f;
        ++i;  // one more tex0 fetch done
        if (sample_dist < 1e-5f) {  // material.frag:117-121
            status = 1;
            steps = i;
            hit_fp = f;
            marching = false;
        } else {  // material.frag:124-125
            dist_from_origin += sample_dist;
            ray_pos = madd(ray_pos, ray_dir, sample_dist);
        }
    }
    // Rays for the neighbours: one counter update per wave and direction (round 4; it was one same-address atomic per ray,
    // two with `leftover`, which serialise in one L2 channel), the states stored side by side.  All lanes of the wave are here:
    // the loop ends on a ballot and every return above is wave-uniform.
    if (__ballot(exported) != 0ull) {
        const uint32_t lane = __lane_id();
#pragma unroll
        for (int dir = 0; dir < 2; ++dir) {
            const uint64_t m = __ballot(exported && export_dir == dir);
            if (m == 0ull) continue;
            const uint32_t n = (uint32_t)__popcll(m);
            const int leader = __ffsll((long long)m) - 1;
            uint32_t base = 0;
            if ((int)lane == leader) {
                base = atomicAdd(dir == 0 ? s.count_down : s.count_up, n);
                if (base + n > s.capacity && s.overflow) *s.overflow = 1u;  // the caller's capacity was too small: the image is incomplete
                if (s.leftover) atomicAdd(s.leftover, n);
            }
            base = __shfl(base, leader);
            const uint32_t at = base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
            if (exported && export_dir == dir && at < s.capacity) {
                sdfv_ray_state st;
                st.pixel = pixel;
                st.iteration = (uint32_t)i;
                st.pos[0] = ray_pos.x; st.pos[1] = ray_pos.y; st.pos[2] = ray_pos.z;
                st.t = dist_from_origin;
                (dir == 0 ? s.out_down : s.out_up)[at] = st;
            }
        }
    }
    if (!mine || exported) return;
    if (status == 0) {  // out of steps, material.frag:99-101
        status = -1;
        steps = i;
    }

    float4 rgba = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    float4 raw0 = rgba, raw1 = rgba;
    if (status == 1) {
        raw0 = gather_rgba(a.tex0, hit_fp);  // == the march's last sample
        raw1 = gather_rgba(a.tex1, hit_fp);  // material.frag:154
        rgba = shade(a.rp, raw0, raw1);
    }
    a.rgba[pixel] = rgba;
    if (AUX) {
        sdfv_march_aux aux;
        aux_clear(aux);
        aux_set_march(aux, status, steps, ray_pos, dist_from_origin);
        if (status == 1) {
            const float depth = frag_depth_of(cam.bvp, ray_pos.x, ray_pos.y, ray_pos.z);
            aux_set_hit(aux, raw0, raw1, mk(0.0f, 0.0f, 0.0f), depth);
            // sdfNormal (material.frag:73-80): four taps h away from the hit; each needs the two slices around its own
            // floor(w), which can be one slice further than the march's fetch -- resident only with a second upper ghost
            // slice (or at the ends of the grid).  Without it the normal stays (0, 0, 0).
            if (a.fast_normal) {
                const float h = tap_distance((float)tex.w, (float)tex.h, (float)tex.d, a.rp.lod_dist_between_samples);
                const V3 taps[4] = {normal_tap(ray_pos, h, 0), normal_tap(ray_pos, h, 1), normal_tap(ray_pos, h, 2), normal_tap(ray_pos, h, 3)};
                float d[4];
                bool resident = true;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const V3 q = to_p01<XF>(a, taps[k]);
                    const float w = q.z * (float)tex.d - 0.5f;
                    const int k0 = (int)floorf(w);
                    const int lo = max(k0, 0), hi = min(k0 + 1, tex.d - 1);
                    resident = resident && lo >= (int)s.z_lo && hi < (int)(s.z_lo + s.z_count);
                    d[k] = 0.0f;
                    if (resident) {  // only then are the eight texels inside this rank's allocation
                        d[k] = gather_r(dist_r, 4, footprint<kClampSlab>(tex, q)) - 1e-1f;
                    }
                }
                if (resident) aux_set_hit(aux, raw0, raw1, normal_of_taps(d[0], d[1], d[2], d[3]), depth);
            }
        }
        a.aux[pixel] = aux;
    }
}

}  // namespace

hipError_t launch_raymarch_slab(const RaymarchArgs& a, const SlabMarchArgs& s, hipStream_t stream) {
    const bool device_counts = s.in_count[0] || s.in_count[1];
    const uint64_t threads = device_counts ? (uint64_t)s.max_in
                             : s.in ? (uint64_t)s.n_in
                                    : (uint64_t)((a.width + 7) / 8) * ((a.height + 7) / 8) * 64;  // whole 8x8 tiles
    if (threads == 0) return hipSuccess;
    const dim3 grid((uint32_t)((threads + 255) / 256));
    if (a.pow2_extent) {
        if (a.aux) hipLaunchKernelGGL((raymarch_slab_kernel<1, true>), grid, dim3(256), 0, stream, a, s);
        else hipLaunchKernelGGL((raymarch_slab_kernel<1, false>), grid, dim3(256), 0, stream, a, s);
    } else {
        if (a.aux) hipLaunchKernelGGL((raymarch_slab_kernel<0, true>), grid, dim3(256), 0, stream, a, s);
        else hipLaunchKernelGGL((raymarch_slab_kernel<0, false>), grid, dim3(256), 0, stream, a, s);
    }
    return hipGetLastError();
}

}  // namespace sdfv
