// demo_sdf_device.h -- the embedded demo SDF (cube minus sphere) as gfx950 device code.
//
// Implements SDFSurface::sample for the three ids of the demo hierarchy, op for op in the order the
// reference evaluates them (all device code is built with -ffp-contract=off; HIP's default
// correctly-rounded fp32 divide/sqrt is relied upon):
//   SDFDemo::sample          src/sdf/demo/mod.rs:51-75
//   SDFDemoCube::sample      src/sdf/demo/cube.rs:79-89,  normal :164-177
//   Material::render         src/sdf/demo/cube.rs:51-58
//   sample_brick_texture     src/sdf/demo/cube.rs:181-222
//   SDFDemoSphere::sample    src/sdf/demo/sphere.rs:37-47, normal :122-124
// and the texel packing of SDFViewer::update, src/app/scene/sdf/mod.rs:196-208.
//
// Work whose result the reference discards is skipped (e.g. the sphere's normalize when the cube's
// sample wins, or any material when the custom inter-surface material overrides it); every value that
// reaches the output is computed by the same operations.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#if defined(__HIPCC_RTC__)  // the run-time compiler is handed the headers by name (program_compile.hip)
#include "sdfgrid.h"
#else
#include "../../include/sdfgrid.h"
#endif

namespace sdfv {

// f32 `%` with a power-of-two modulus m (inv_m = 1/m), a >= 0.  a*inv_m, trunc, *m and the final
// subtraction are all exact, so this equals fmodf(a, m) bit for bit (cube.rs:192 `% BRICK_WIDTH`).
__device__ __forceinline__ float fmod_pow2(float a, float m, float inv_m) {
    return a - truncf(a * inv_m) * m;
}

struct Mat {
    float r, g, b, metallic, roughness, occlusion;
};

// compute_tex2d, cube.rs:189-202.  v/0.25 == v*4 and floor(row)/4 == floor(row)*0.25 exactly.
__device__ __forceinline__ Mat brick_tex2d(float u, float v) {
    const float BRICK_WIDTH = 0.5f, BRICK_HEIGHT = 0.25f;
    const float max_cement_displacement = 0.2f / 2.0f * 0.25f;  // CEMENT_THICKNESS / 2.0 * BRICK_HEIGHT
    float row_num = v * 4.0f;
    float brick_offset = floorf(row_num) * 0.25f;
    float bx = fmod_pow2(fabsf(u + brick_offset), BRICK_WIDTH, 2.0f);
    float by = fmod_pow2(fabsf(v), BRICK_HEIGHT, 4.0f);
    bool cement = bx < max_cement_displacement || bx > BRICK_WIDTH - max_cement_displacement ||
                  by < max_cement_displacement || by > BRICK_HEIGHT - max_cement_displacement;
    Mat m;
    m.r = cement ? 56.0f / 255.0f : 150.0f / 255.0f;
    m.g = cement ? 70.0f / 255.0f : 24.0f / 255.0f;
    m.b = cement ? 60.0f / 255.0f : 10.0f / 255.0f;
    m.metallic = cement ? 0.4f : 0.2f;
    m.roughness = cement ? 0.5f : 0.8f;
    m.occlusion = cement ? 1.0f : 0.0f;
    return m;
}

// Material::render (cube.rs:51-58) on normal n.  Brick: tri-planar uv pick, cube.rs:205-220.
__device__ __forceinline__ Mat material_render(uint32_t material, float px, float py, float pz,
                                               float nx, float ny, float nz) {
    float ax = fabsf(nx), ay = fabsf(ny), az = fabsf(nz);
    if (material == SDFV_MATERIAL_BRICK) {
        float u, v;
        if (ax > ay) {
            if (ax > az) { u = pz; v = py; } else { u = px; v = py; }
        } else if (ay > az) { u = pz; v = px; }
        else { u = px; v = py; }
        return brick_tex2d(u, v);
    }
    Mat m;  // SDFSample::new(dist, |n|): metallic = roughness = occlusion = 0 (src/sdf/mod.rs:120-126)
    m.r = ax; m.g = ay; m.b = az;
    m.metallic = 0.0f; m.roughness = 0.0f; m.occlusion = 0.0f;
    return m;
}

__device__ __forceinline__ float signum_f32(float x) {  // f32::signum (NaN never reaches it here)
    return __builtin_signbit(x) ? -1.0f : 1.0f;
}

__device__ __forceinline__ Mat zero_mat() {
    Mat m; m.r = m.g = m.b = m.metallic = m.roughness = m.occlusion = 0.0f; return m;
}

// SDFDemoCube::sample material part; d_box already known.  cube.rs:83-88 + normal :164-177.
__device__ __forceinline__ Mat cube_material(const sdfv_demo_params& prm, float px, float py, float pz,
                                             float d_box, bool distance_only) {
    if (distance_only || d_box > 0.1f) return zero_mat();
    float side = prm.cube_half_side;
    float nx = fabsf(px) > side ? signum_f32(px) : 0.0f;
    float ny = fabsf(py) > side ? signum_f32(py) : 0.0f;
    float nz = fabsf(pz) > side ? signum_f32(pz) : 0.0f;
    return material_render(prm.cube_material, px, py, pz, nx, ny, nz);
}

// SDFDemoSphere::sample material part; len = |p| already known.  sphere.rs:41-46 + normal :122-124
// (cgmath normalize = p * (1/|p|)).
__device__ __forceinline__ Mat sphere_material(const sdfv_demo_params& prm, float px, float py, float pz,
                                               float len, float d_sph, bool distance_only) {
    if (distance_only || d_sph > 0.1f) return zero_mat();
    float inv = 1.0f / len;
    return material_render(prm.sphere_material, px, py, pz, px * inv, py * inv, pz * inv);
}

__device__ __forceinline__ float cube_distance(const sdfv_demo_params& prm, float px, float py, float pz) {
    return fmaxf(fmaxf(fabsf(px), fabsf(py)), fabsf(pz)) - prm.cube_half_side;  // cube.rs:81
}

// p.distance(0): |0 - p|, dot = (x*x + y*y) + z*z (cgmath 0.18).  sphere.rs:39
__device__ __forceinline__ float vec_length(float x, float y, float z) {
    return sqrtf(x * x + y * y + z * z);
}

struct Sample {
    float distance;
    Mat m;
};

// SDFSurface::sample(p, distance_only) for sdf_id in {demo, cube, sphere}.
__device__ __forceinline__ Sample demo_sample(const sdfv_demo_params& prm, uint32_t sdf_id,
                                              float px, float py, float pz, bool distance_only) {
    Sample s;
    if (sdf_id == SDFV_SDF_CUBE) {
        s.distance = cube_distance(prm, px, py, pz);
        s.m = cube_material(prm, px, py, pz, s.distance, distance_only);
        return s;
    }
    if (sdf_id == SDFV_SDF_SPHERE) {
        float len = vec_length(px, py, pz);
        s.distance = len - prm.sphere_radius;
        s.m = sphere_material(prm, px, py, pz, len, s.distance, distance_only);
        return s;
    }
    // SDFDemo::sample, demo/mod.rs:51-75
    float d_box = cube_distance(prm, px, py, pz);
    if (prm.disable_sphere) {
        s.distance = d_box;
        s.m = cube_material(prm, px, py, pz, d_box, distance_only);
        return s;
    }
    float len = vec_length(px, py, pz);
    float d_sph = len - prm.sphere_radius;
    s.distance = fmaxf(d_box, -d_sph);
    float inter = fabsf(d_box) - fabsf(d_sph);
    if (fabsf(inter) <= prm.max_distance_custom_material) {
        s.m.r = 0.5f; s.m.g = 0.6f; s.m.b = 0.7f;
        s.m.metallic = 0.5f; s.m.roughness = 0.0f; s.m.occlusion = 0.0f;
    } else if (inter < 0.0f) {
        s.m = cube_material(prm, px, py, pz, d_box, distance_only);
    } else {
        s.m = sphere_material(prm, px, py, pz, len, d_sph, distance_only);
    }
    return s;
}

// f32::clamp(0.0, 1.0) as used at scene/sdf/mod.rs:196: a NaN stays a NaN (fminf/fmaxf would turn it into 0).
// Only reachable through the dim == 1 quirk (0/0 coordinates), but the packing is reproduced exactly.
__device__ __forceinline__ float clamp01_rust(float v) {
    return v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v);
}

// three-d-asset Srgba::from(Vec3) [EXT: that crate's source is not under the reference tree].  ROUND = false is the
// restatement the product ships: (c * 255.0) as u8 -- truncating, saturating, NaN -> 0.  ROUND = true is the one plausible
// alternative with visible consequences (profiles/ext_sensitivity.json): (c * 255.0 + 0.5) as u8, what the oracle evaluates
// under OR_EXT_SRGB_QUANT_ROUND.  Chosen per call by SDFV_OPT_EXT_SRGB_QUANT, compiled in as a template policy.
template <bool ROUND>
__device__ __forceinline__ uint32_t srgb_quantize(float c) {
    float v = c * 255.0f;
    if (ROUND) v = v + 0.5f;
    v = fminf(fmaxf(v, 0.0f), 255.0f);  // fmaxf(NaN, 0) = 0
    return (uint32_t)v;
}

// SDFViewer::update's packing, scene/sdf/mod.rs:196-208.  lut = to_linear_srgb per u8 (256 floats).
template <bool ROUND, typename Lut>
__device__ __forceinline__ void pack_sample(const Sample& s, const Lut& lut, float air_dist,
                                            float4& t0, float4& t1) {
    float r = s.m.r, g = s.m.g, b = s.m.b;
    if (r == 0.0f && g == 0.0f && b == 0.0f) { r = 0.5f; g = 0.5f; b = 0.5f; }
    t0.x = clamp01_rust(1e-1f + s.distance);
    t0.y = lut[srgb_quantize<ROUND>(r)];
    t0.z = lut[srgb_quantize<ROUND>(g)];
    t0.w = lut[srgb_quantize<ROUND>(b)];
    t1.x = s.m.metallic;
    t1.y = s.m.roughness;
    t1.z = s.m.occlusion <= 0.0f ? 1.0f : s.m.occlusion;
    t1.w = air_dist;  // never written by update(): new_voxels' init value (scene/sdf/mod.rs:76-77)
}


// ---------------------------------------------------------------------------------------------
// Fused sample + pack for the dense fill (scene/sdf/mod.rs:193-208 applied to SDFDemo::sample).
//
// Same arithmetic as demo_sample() + pack_sample(), arranged for the store-bound kernel:
//  * every material whose colour is a constant (brick, cement, the custom inter-surface material,
//    the 0.5 grey that replaces an all-zero colour) is packed at COMPILE time: quantise + table lookup
//    of a constant is a constant, so only the "normal" material (colour = |n|) touches the table;
//  * the configuration (which SDF, which materials) is a template policy, so the common default
//    configuration carries no uniform branches; RuntimeCfg reads them from the parameter block.
// ---------------------------------------------------------------------------------------------
constexpr float kSrgbToLinear[256] = {
#include "srgb_lut.inc"
};

template <bool ROUND>
constexpr uint32_t quantize_constexpr(float c) {  // srgb_quantize<ROUND>() for compile-time constants
    float v = c * 255.0f;
    if (ROUND) v = v + 0.5f;
    return !(v > 0.0f) ? 0u : (v >= 255.0f ? 255u : (uint32_t)v);
}
template <bool ROUND>
constexpr float linear_of(float c) { return kSrgbToLinear[quantize_constexpr<ROUND>(c)]; }

struct Packed {  // what update() writes besides tex0.r: tex0.gba and tex1.rgb
    float lr, lg, lb, metallic, roughness, occlusion;
};

// Both sets of packed constants are compiled in (one per Srgba::from policy); occlusion <= 0 -> 1 (scene/sdf/mod.rs:208) is
// folded into them.  (Truncation maps 0.5 / 0.6 / 0.7 to 127 / 153 / 178, rounding to 128 / 153 / 179; the brick and cement
// colours are k / 255 and land on k either way unless k / 255 * 255 rounds below k.)
template <bool ROUND>
struct PackedSet {
    static constexpr Packed kCement = {linear_of<ROUND>(56.0f / 255.0f), linear_of<ROUND>(70.0f / 255.0f),
                                       linear_of<ROUND>(60.0f / 255.0f), 0.4f, 0.5f, 1.0f};
    static constexpr Packed kBrick = {linear_of<ROUND>(150.0f / 255.0f), linear_of<ROUND>(24.0f / 255.0f),
                                      linear_of<ROUND>(10.0f / 255.0f), 0.2f, 0.8f, 1.0f};
    static constexpr Packed kCustom = {linear_of<ROUND>(0.5f), linear_of<ROUND>(0.6f), linear_of<ROUND>(0.7f), 0.5f, 0.0f, 1.0f};
    static constexpr Packed kAir = {linear_of<ROUND>(0.5f), linear_of<ROUND>(0.5f), linear_of<ROUND>(0.5f), 0.0f, 0.0f, 1.0f};  // zero colour -> 0.5
};

template <bool ROUND>
struct DefaultCfgT {  // SDFDemo::default(): brick cube minus normal-shaded sphere
    static constexpr bool kStatic = true;
    static constexpr bool kRound = ROUND;
    __device__ static __forceinline__ uint32_t sdf_id(uint32_t) { return SDFV_SDF_DEMO; }
    __device__ static __forceinline__ uint32_t cube_material(const sdfv_demo_params&) { return SDFV_MATERIAL_BRICK; }
    __device__ static __forceinline__ uint32_t sphere_material(const sdfv_demo_params&) { return SDFV_MATERIAL_NORMAL; }
    __device__ static __forceinline__ bool disable_sphere(const sdfv_demo_params&) { return false; }
};
template <bool ROUND>
struct RuntimeCfgT {
    static constexpr bool kStatic = false;
    static constexpr bool kRound = ROUND;
    __device__ static __forceinline__ uint32_t sdf_id(uint32_t id) { return id; }
    __device__ static __forceinline__ uint32_t cube_material(const sdfv_demo_params& p) { return p.cube_material; }
    __device__ static __forceinline__ uint32_t sphere_material(const sdfv_demo_params& p) { return p.sphere_material; }
    __device__ static __forceinline__ bool disable_sphere(const sdfv_demo_params& p) { return p.disable_sphere != 0; }
};
using DefaultCfg = DefaultCfgT<false>;
using RuntimeCfg = RuntimeCfgT<false>;

__device__ __forceinline__ Packed select_packed(bool c, const Packed& a, const Packed& b) {
    Packed r;
    r.lr = c ? a.lr : b.lr; r.lg = c ? a.lg : b.lg; r.lb = c ? a.lb : b.lb;
    r.metallic = c ? a.metallic : b.metallic; r.roughness = c ? a.roughness : b.roughness;
    r.occlusion = c ? a.occlusion : b.occlusion;
    return r;
}

// Material::render + packing for a normal n.  `lut` is only read by the Normal material.
template <bool ROUND, typename Lut>
__device__ __forceinline__ Packed render_packed(uint32_t material, float px, float py, float pz,
                                                float nx, float ny, float nz, const Lut& lut) {
    float ax = fabsf(nx), ay = fabsf(ny), az = fabsf(nz);
    if (material == SDFV_MATERIAL_BRICK) {
        float u, v;
        if (ax > ay) {
            if (ax > az) { u = pz; v = py; } else { u = px; v = py; }
        } else if (ay > az) { u = pz; v = px; }
        else { u = px; v = py; }
        const float BRICK_WIDTH = 0.5f, BRICK_HEIGHT = 0.25f;
        const float mcd = 0.2f / 2.0f * 0.25f;
        float brick_offset = floorf(v * 4.0f) * 0.25f;
        float bx = fmod_pow2(fabsf(u + brick_offset), BRICK_WIDTH, 2.0f);
        float by = fmod_pow2(fabsf(v), BRICK_HEIGHT, 4.0f);
        bool cement = bx < mcd || bx > BRICK_WIDTH - mcd || by < mcd || by > BRICK_HEIGHT - mcd;
        return select_packed(cement, PackedSet<ROUND>::kCement, PackedSet<ROUND>::kBrick);
    }
    Packed r;  // colour |n|, metallic = roughness = 0, occlusion 0 -> 1
    bool zero = ax == 0.0f && ay == 0.0f && az == 0.0f;
    float cr = zero ? 0.5f : ax, cg = zero ? 0.5f : ay, cb = zero ? 0.5f : az;
    r.lr = lut[srgb_quantize<ROUND>(cr)];
    r.lg = lut[srgb_quantize<ROUND>(cg)];
    r.lb = lut[srgb_quantize<ROUND>(cb)];
    r.metallic = 0.0f; r.roughness = 0.0f; r.occlusion = 1.0f;
    return r;
}

template <typename Cfg, typename Lut>
__device__ __forceinline__ Packed cube_packed(const sdfv_demo_params& prm, float px, float py, float pz,
                                              float d_box, const Lut& lut) {
    if (d_box > 0.1f) return PackedSet<Cfg::kRound>::kAir;  // cube.rs:83-85
    float side = prm.cube_half_side;
    float nx = fabsf(px) > side ? signum_f32(px) : 0.0f;
    float ny = fabsf(py) > side ? signum_f32(py) : 0.0f;
    float nz = fabsf(pz) > side ? signum_f32(pz) : 0.0f;
    return render_packed<Cfg::kRound>(Cfg::cube_material(prm), px, py, pz, nx, ny, nz, lut);
}

template <typename Cfg, typename Lut>
__device__ __forceinline__ Packed sphere_packed(const sdfv_demo_params& prm, float px, float py, float pz,
                                                float len, float d_sph, const Lut& lut) {
    if (d_sph > 0.1f) return PackedSet<Cfg::kRound>::kAir;  // sphere.rs:41-43
    float inv = 1.0f / len;
    return render_packed<Cfg::kRound>(Cfg::sphere_material(prm), px, py, pz, px * inv, py * inv, pz * inv, lut);
}

// sample(p, false) + packing.  xx_yy = px*px + py*py may be hoisted by the caller.
template <typename Cfg, typename Lut>
__device__ __forceinline__ void fill_voxel(const sdfv_demo_params& prm, uint32_t sdf_id_rt, float px, float py,
                                           float pz, const Lut& lut, float air_dist, float4& t0, float4& t1) {
    const uint32_t sdf_id = Cfg::sdf_id(sdf_id_rt);
    float distance;
    Packed m;
    if (sdf_id == SDFV_SDF_CUBE || (sdf_id == SDFV_SDF_DEMO && Cfg::disable_sphere(prm))) {
        distance = cube_distance(prm, px, py, pz);
        m = cube_packed<Cfg>(prm, px, py, pz, distance, lut);
    } else if (sdf_id == SDFV_SDF_SPHERE) {
        float len = vec_length(px, py, pz);
        distance = len - prm.sphere_radius;
        m = sphere_packed<Cfg>(prm, px, py, pz, len, distance, lut);
    } else {
        float d_box = cube_distance(prm, px, py, pz);
        float len = vec_length(px, py, pz);
        float d_sph = len - prm.sphere_radius;
        distance = fmaxf(d_box, -d_sph);
        float inter = fabsf(d_box) - fabsf(d_sph);
        if (fabsf(inter) <= prm.max_distance_custom_material) {
            m = PackedSet<Cfg::kRound>::kCustom;
        } else if (inter < 0.0f) {
            m = cube_packed<Cfg>(prm, px, py, pz, d_box, lut);
        } else {
            m = sphere_packed<Cfg>(prm, px, py, pz, len, d_sph, lut);
        }
    }
    t0.x = clamp01_rust(1e-1f + distance);
    t0.y = m.lr; t0.z = m.lg; t0.w = m.lb;
    t1.x = m.metallic; t1.y = m.roughness; t1.z = m.occlusion; t1.w = air_dist;
}

// voxel index -> position, scene/sdf/mod.rs:178-182: idx/(dim-1), *size, +min, each rounded.
__device__ __forceinline__ float voxel_coord(uint32_t idx, float dim_minus_1, float bb_size, float bb_min) {
    float p = (float)idx;
    p = p / dim_minus_1;
    p = p * bb_size;
    p = p + bb_min;
    return p;
}

// ---- SDFSurface::normal and the meshers' unit-cube mapping (shared by points_kernels.hip, mesh_kernels.hip) ----

// SDFDemoCube::normal, cube.rs:164-177
__device__ __forceinline__ void cube_normal(const sdfv_demo_params& prm, float px, float py, float pz,
                                            float& nx, float& ny, float& nz) {
    float side = prm.cube_half_side;
    nx = fabsf(px) > side ? signum_f32(px) : 0.0f;
    ny = fabsf(py) > side ? signum_f32(py) : 0.0f;
    nz = fabsf(pz) > side ? signum_f32(pz) : 0.0f;
}

// cgmath normalize: v * (1 / |v|)
__device__ __forceinline__ void normalize3(float x, float y, float z, float& nx, float& ny, float& nz) {
    float inv = 1.0f / vec_length(x, y, z);
    nx = x * inv; ny = y * inv; nz = z * inv;
}

// SDFSurface::normal(p, eps) for the demo tree: the overrides (demo/mod.rs:147-156, cube.rs:164-177,
// sphere.rs:122-124) ignore eps; use_default = the trait's default body (defaults.rs:49-56).
__device__ __forceinline__ void demo_normal(const sdfv_demo_params& prm, uint32_t sdf_id, float px, float py, float pz,
                                            float eps, bool use_default, float& nx, float& ny, float& nz) {
    if (use_default) {
        // normal_default_impl, defaults.rs:49-56: eps.unwrap_or(0.001), 4 taps of sample(.., true)
        const float e = eps > 0.0f ? eps : 0.001f;
        float d1 = demo_sample(prm, sdf_id, px + e, py + -1.0f * e, pz + -1.0f * e, true).distance;
        float d2 = demo_sample(prm, sdf_id, px + -1.0f * e, py + e, pz + -1.0f * e, true).distance;
        float d3 = demo_sample(prm, sdf_id, px + -1.0f * e, py + -1.0f * e, pz + e, true).distance;
        float d4 = demo_sample(prm, sdf_id, px + e, py + e, pz + e, true).distance;
        normalize3(d1 + -d2 + -d3 + d4, -d1 + d2 + -d3 + d4, -d1 + -d2 + d3 + d4, nx, ny, nz);
    } else if (sdf_id == SDFV_SDF_CUBE) {
        cube_normal(prm, px, py, pz, nx, ny, nz);
    } else if (sdf_id == SDFV_SDF_SPHERE) {
        normalize3(px, py, pz, nx, ny, nz);  // sphere.rs:122-124
    } else {
        // SDFDemo::normal, demo/mod.rs:147-156: normal of the closest surface, sphere negated
        float d_box = cube_distance(prm, px, py, pz);
        float d_sph = vec_length(px, py, pz) - prm.sphere_radius;
        if (fabsf(d_box) < fabsf(d_sph)) {
            cube_normal(prm, px, py, pz, nx, ny, nz);
        } else {
            normalize3(px, py, pz, nx, ny, nz);
            nx = -nx; ny = -ny; nz = -nz;
        }
    }
}

// SDFSurfaceWrapper::vert_pos_to, meshers/isosurface.rs:95-99: the meshers work in the unit cube.
struct SourceBox {
    float bb_min[3], bb_size[3];
    bool unit_cube;  // false: points are already in world space
    __device__ __forceinline__ void to_world(float& x, float& y, float& z) const {
        if (!unit_cube) return;
        x = x * bb_size[0] + bb_min[0];
        y = y * bb_size[1] + bb_min[1];
        z = z * bb_size[2] + bb_min[2];
    }
};

}  // namespace sdfv
