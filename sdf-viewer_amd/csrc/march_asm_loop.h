// march_asm_loop.h -- sdfRaycast's loop in gfx950 assembly (march_asm): the SDFV_MARCH_ASM_* pieces of its text and the C++
// around them.  What the loop computes is march_loops.h's march_fast, instruction for instruction.  Device text only.
#pragma once

#include "march_sampler.h"

namespace sdfv {
namespace {

// ---- the march loop in gfx950 assembly -------------------------------------------------------------------------------
// A frame is as long as its longest wave: ONE grazing ray doing up to 255 dependent iterations alone on its SIMD, where
// a lone wave issues one instruction every ~6-11 cycles whatever the instruction is.  So the loop is priced per
// INSTRUCTION, and hipcc's lowering of either C++ form (the predicated march_fast above: 78 per iteration; the same loop
// written as a plain divergent loop with breaks: ~83, the structurizer's mask bookkeeping -- tried and removed) leaves
// half of the cost on the table.  This is the same loop written by hand (profiles/r02/raymarch_loop_isa.md):
//   * the set of marching lanes IS the EXEC mask: v_cmpx removes the lanes that stop (out-of-bounds test, hit test), so
//     nothing is predicated and no mask register is maintained; s_cbranch_execz is the wave-level early exit;
//   * the one-cell cache is tested on the interpolation weights themselves: a = u - floor_cached(u) is the weight if the
//     cell is unchanged, and it is in [0, 1) -- as an unsigned integer: below 0x3f800000 -- exactly when it is unchanged;
//     three subtractions the filter needs anyway + v_max3_u32 + one compare replace 3 floors + 3 compares + 2 s_or;
//   * (y, z) components ride in packed-f32 instructions (v_pk_add/mul_f32), the corner values are kept as z-pairs so
//     that the x and y levels of the trilinear filter are packed as well;
//   * no per-iteration status or step counters (derived after the loop as in march_fast; the aux variant counts).
// 40 instructions per iteration on the common path (42 for a non-cubic box).  Every arithmetic instruction is the one the C++ form performs, in
// the same order on the same operands (no fma, no reassociation): results are bit-identical, which the parity tests
// check against the oracle for every pixel.  Covers: LINEAR filter, power-of-two extents and texture sizes (XF == 2),
// symmetric box, clamp-for-mirror (fast_index); every MODE but kMarchGeneral (kMarchDist: one 8-byte load per corner row,
// kMarchTex0: tex0.r in place).  Byte offsets are 32-bit: the launcher checks the volume's size (volume_fits_loop).
// Registers: v24-v71 (less v41, v45, v49, v69) and s64-s87 are this block's (declared as clobbers; low enough that the kernel stays at 96
// VGPRs = 5 waves per SIMD); operands stay where hipcc put them.
#ifdef SDFV_TUNING
#define SDFV_MARCH_ASM_TUNE(x) x
#else
#define SDFV_MARCH_ASM_TUNE(x) ""
#endif
#define SDFV_MARCH_ASM_HEAD(ROW_BYTES)                                                                                         \
    "s_mov_b64 s[76:77], exec\n"                                                                                    \
    "s_and_b64 exec, exec, %[cov]\n"                                                                                \
    "s_cbranch_execz .Ldone_%=\n"                                                                                   \
    /* position v40, v[42:43] and direction v44, v[46:47] ARE the operands px..dz (explicit register variables) */      \
    "s_mov_b32 s66, %[miny]\n s_mov_b32 s67, %[minz]\n"      /* (miny, minz) */                                      \
    "s_mov_b32 s70, %[ky]\n s_mov_b32 s71, %[kz]\n"          /* (ky, kz) */                                          \
    "s_mov_b32 s72, 0xbf000000\n s_mov_b32 s73, 0xbf000000\n" /* (-0.5, -0.5) */                                     \
    "s_add_i32 s75, %[wm1], -1\n"                            /* W - 2 */                                             \
    "s_lshl_b32 s82, %[w], 2\n s_lshl_b32 s83, %[w], 4\n"    /* bytes per row: W * 4 (distance volume), W * 16 (tex0) */     \
    "s_lshl_b32 s85, %[w], 3\n"                              /* ... W * 8: the y-pair / y-interleaved volumes */        \
    "s_movk_i32 s74, 254\n"                                  /* 255 iterations */                                    \
    /* interior cells (all eight corners inside the volume, no clamp): the four corner rows are one offset against four  \
     * bases -- b00 = base, b10 = base + a row, b01 = base + a slice, b11 = both (row bytes: s82 for the distance volume, \
     * s83 for tex0, s85 for the pair volume).  Sizes need not be powers of two: rows and slices go by multiplication */ \
    "s_mov_b32 s64, " ROW_BYTES "\n"                                                                                 \
    "s_mul_i32 s86, %[h], " ROW_BYTES "\n"                                                                           \
    "s_add_u32 s68, %[base_lo], s86\n s_addc_u32 s69, %[base_hi], 0\n"   /* b01 */                                   \
    "s_add_u32 s64, %[base_lo], s64\n s_addc_u32 s65, %[base_hi], 0\n"   /* b10 */                                   \
    "s_add_u32 s86, s64, s86\n s_addc_u32 s87, s65, 0\n"                 /* b11 */                                   \
    SDFV_MARCH_ASM_TUNE("s_mov_b32 s84, 0\n")                /* tuning build: iterations that ran the fetch block */  \
    "v_mov_b32 v68, 0x7f800000\n v_mov_b32 v70, 0x7f800000\n v_mov_b32 v71, 0x7f800000\n" /* no cell cached */    \
    ".Lloop_%=:\n"
// One iteration, top half.  Two independent chains are interleaved so that a lone wave rarely issues an instruction
// that waits for the one before it: (A) out of bounds? max(|p| - max) > 1e-4 (material.frag:106-109) -> v_cmpx removes
// the lanes that left the box; (B) u = (p - min) * (N / size) - 0.5, x alone and (y, z) packed.  Then the weights
// relative to the cached cell: all three in [0, 1) <=> the cell is unchanged.
// OOB4 / OOB2: the out-of-bounds distance max(|p| - max) in four instructions, or in two when the box is a cube
// (max_x == max_y == max_z = m): max3(|p|) - m -- identical bits, rounding is monotonic so max and "- m" commute.
#define SDFV_MARCH_ASM_OOB4_A "v_sub_f32_e64 v32, |v40|, %[mx]\n"
#define SDFV_MARCH_ASM_OOB4_B "v_sub_f32_e64 v33, |v42|, %[my]\n"
#define SDFV_MARCH_ASM_OOB4_C "v_sub_f32_e64 v34, |v43|, %[mz]\n"
#define SDFV_MARCH_ASM_OOB4_D "v_max3_f32 v32, v32, v33, v34\n"
#define SDFV_MARCH_ASM_OOB2_A "v_max3_f32 v32, |v40|, |v42|, |v43|\n"
#define SDFV_MARCH_ASM_OOB2_D "v_subrev_f32_e32 v32, %[mx], v32\n"
#define SDFV_MARCH_ASM_TOP(T_STEP, OOB_A, OOB_B, OOB_C, OOB_D)                                                      \
    OOB_A                                                                                                           \
    "v_subrev_f32_e32 v48, %[minx], v40\n"                                                                          \
    OOB_B                                                                                                           \
    "v_pk_add_f32 v[50:51], v[42:43], s[66:67] neg_lo:[0,1] neg_hi:[0,1]\n"                                         \
    OOB_C                                                                                                           \
    "v_mul_f32_e32 v48, %[kx], v48\n"                                                                               \
    "v_pk_mul_f32 v[50:51], v[50:51], s[70:71]\n"                                                                   \
    OOB_D                                                                                                           \
    "v_add_f32_e32 v48, -0.5, v48\n"                                                                                \
    "v_pk_add_f32 v[50:51], v[50:51], s[72:73]\n"                                                                   \
    "v_cmpx_nlt_f32_e32 vcc, 0x38d1b717, v32\n"              /* exec &= !(1e-4 < oob) */                             \
    "s_cbranch_execz .Ldone_%=\n"                                                                                   \
    "v_sub_f32_e32 v52, v48, v68\n"                                                                              \
    "v_sub_f32_e32 v54, v50, v70\n"                                                                              \
    "v_sub_f32_e32 v56, v51, v71\n" T_STEP                                                                       \
    "v_max3_u32 v32, v52, v54, v56\n"                                                                            \
    "v_cmp_gt_u32_e32 vcc, 0x3f800000, v32\n"                                                                       \
    "s_andn1_saveexec_b64 s[78:79], vcc\n"                   /* exec = lanes whose cell changed */                   \
    "s_cbranch_execnz .Lfetch_%=\n"                          /* out of line: the cached case falls through */        \
    ".Lcached_%=:\n"
// The cell fetch, out of line behind the loop (one taken branch less in every iteration that stays in its cells).
#define SDFV_MARCH_ASM_FETCH_PREP(INTERIOR)                                                                         \
    ".Lfetch_%=:\n"                                                                                                 \
    SDFV_MARCH_ASM_TUNE("s_add_u32 s84, s84, 1\n")                                                                  \
    /* new cell: floor, weights, clamped corner indices (MirroredRepeat == clamp here), row numbers by shifts */    \
    "v_floor_f32_e32 v68, v48\n v_floor_f32_e32 v70, v50\n v_floor_f32_e32 v71, v51\n"                         \
    "v_cvt_i32_f32_e32 v32, v68\n v_cvt_i32_f32_e32 v33, v70\n v_cvt_i32_f32_e32 v34, v71\n"                      \
    "v_sub_f32_e32 v52, v48, v68\n v_sub_f32_e32 v54, v50, v70\n v_sub_f32_e32 v56, v51, v71\n"             \
    /* every fetching lane's cell inside the volume (cubic volumes: 0 <= i0, j0, k0 <= N - 2, one unsigned compare)? */ \
    "v_max3_u32 v35, v32, v33, v34\n"                                                                               \
    "v_cmp_gt_u32_e32 vcc, %[thresh], v35\n"                                                                        \
    "s_xor_b64 vcc, vcc, exec\n"                                                                                    \
    "s_cbranch_scc1 .Lborder_%=\n"                                                                                  \
    "v_mad_u32_u24 v39, v34, %[h], v33\n"                    /* (k0 * H + j0) * W + i0: 24-bit factors (the launcher checks) */ \
    "v_mad_u32_u24 v39, v39, %[w], v32\n" INTERIOR                                                               \
    "s_branch .Lcached_%=\n"                                                                                        \
    ".Lborder_%=:\n"                                                                                                \
    "v_max_i32_e32 v35, 0, v32\n v_max_i32_e32 v37, 0, v33\n v_max_i32_e32 v38, 0, v34\n"  /* i0c, j0c, k0c */       \
    "v_add_u32_e32 v32, 1, v32\n v_add_u32_e32 v33, 1, v33\n v_add_u32_e32 v34, 1, v34\n"                            \
    "v_min_i32_e32 v32, %[wm1], v32\n v_min_i32_e32 v33, %[hm1], v33\n v_min_i32_e32 v34, %[dm1], v34\n" /* i1c.. */  \
    "v_mad_u32_u24 v28, v38, %[h], v37\n"                    /* rows: (k0c, j0c) */                                  \
    "v_mad_u32_u24 v29, v38, %[h], v33\n"                    /*       (k0c, j1c) */                                  \
    "v_mad_u32_u24 v30, v34, %[h], v37\n"                    /*       (k1c, j0c) */                                  \
    "v_mad_u32_u24 v31, v34, %[h], v33\n"                    /*       (k1c, j1c) */
// Interior fetch (v39 = texel index of corner (i0, j0, k0)): no clamps, no selects.
#define SDFV_MARCH_ASM_INTERIOR_DIST                                                                                \
    "v_lshlrev_b32_e32 v39, 2, v39\n"                                                                               \
    "global_load_dwordx2 v[24:25], v39, %[base]\n"           /* (z0, y0): t000, t100 */                             \
    "global_load_dwordx2 v[26:27], v39, s[64:65]\n"          /* (z0, y1): t010, t110 */                             \
    "global_load_dwordx2 v[28:29], v39, s[68:69]\n"          /* (z1, y0): t001, t101 */                             \
    "global_load_dwordx2 v[30:31], v39, s[86:87]\n"          /* (z1, y1): t011, t111 */                             \
    "s_waitcnt vmcnt(1)\n"                                                                                          \
    "v_pk_mov_b32 v[60:61], v[24:25], v[28:29] op_sel:[0,0]\n" /* (t000, t001) */                                   \
    "v_pk_mov_b32 v[62:63], v[24:25], v[28:29] op_sel:[1,1]\n" /* (t100, t101) */                                   \
    "s_waitcnt vmcnt(0)\n"                                                                                          \
    "v_pk_mov_b32 v[64:65], v[26:27], v[30:31] op_sel:[0,0]\n" /* (t010, t011) */                                   \
    "v_pk_mov_b32 v[66:67], v[26:27], v[30:31] op_sel:[1,1]\n" /* (t110, t111) */
#define SDFV_MARCH_ASM_INTERIOR_TEX0                                                                                \
    "v_lshlrev_b32_e32 v39, 4, v39\n"                                                                               \
    "global_load_dword v60, v39, %[base]\n global_load_dword v62, v39, %[base] offset:16\n"                       \
    "global_load_dword v64, v39, s[64:65]\n global_load_dword v66, v39, s[64:65] offset:16\n"                     \
    "global_load_dword v61, v39, s[68:69]\n global_load_dword v63, v39, s[68:69] offset:16\n"                     \
    "global_load_dword v65, v39, s[86:87]\n global_load_dword v67, v39, s[86:87] offset:16\n"                     \
    "s_waitcnt vmcnt(0)\n"
// The y-pair volume (sdfv_commit_pairs): texel (x, y, z) holds (d[y], d[min(y + 1, H - 1)]), 8 bytes, so the four corners of a
// cell's z-level -- (x0, y0), (x0, y1), (x1, y0), (x1, y1) -- are 16 CONTIGUOUS bytes: ONE dwordx4 per z-level, two gathers and
// two cache lines per cell instead of four and four.  The gather count is what a fetch costs (tools: profiles/EXPERIMENTS.md).
#define SDFV_MARCH_ASM_INTERIOR_PAIRS                                                                               \
    "v_lshlrev_b32_e32 v39, 3, v39\n"                                                                               \
    "global_load_dwordx4 v[24:27], v39, %[base]\n"           /* z0: t000, t010, t100, t110 */                       \
    "global_load_dwordx4 v[28:31], v39, s[68:69]\n"          /* z1: t001, t011, t101, t111 */                       \
    "s_waitcnt vmcnt(0)\n"                                                                                          \
    "v_pk_mov_b32 v[60:61], v[24:25], v[28:29] op_sel:[0,0]\n" /* (t000, t001) */                                   \
    "v_pk_mov_b32 v[64:65], v[24:25], v[28:29] op_sel:[1,1]\n" /* (t010, t011) */                                   \
    "v_pk_mov_b32 v[62:63], v[26:27], v[30:31] op_sel:[0,0]\n" /* (t100, t101) */                                   \
    "v_pk_mov_b32 v[66:67], v[26:27], v[30:31] op_sel:[1,1]\n" /* (t110, t111) */
// Border cells of the pair volume: the first component of eight texels (clamped corners), one dword load each.
#define SDFV_MARCH_ASM_FETCH_PAIRS                                                                                  \
    "v_lshlrev_b32_e32 v35, 3, v35\n v_lshlrev_b32_e32 v32, 3, v32\n"   /* i0c, i1c as byte offsets */               \
    "v_mad_u32_u24 v24, v28, s85, v35\n v_mad_u32_u24 v25, v28, s85, v32\n"                                          \
    "global_load_dword v60, v24, %[base]\n global_load_dword v62, v25, %[base]\n"                                  \
    "v_mad_u32_u24 v26, v29, s85, v35\n v_mad_u32_u24 v27, v29, s85, v32\n"                                          \
    "global_load_dword v64, v26, %[base]\n global_load_dword v66, v27, %[base]\n"                                  \
    "v_mad_u32_u24 v24, v30, s85, v35\n v_mad_u32_u24 v25, v30, s85, v32\n"                                          \
    "global_load_dword v61, v24, %[base]\n global_load_dword v63, v25, %[base]\n"                                  \
    "v_mad_u32_u24 v26, v31, s85, v35\n v_mad_u32_u24 v27, v31, s85, v32\n"                                          \
    "global_load_dword v65, v26, %[base]\n global_load_dword v67, v27, %[base]\n"                                  \
    "s_waitcnt vmcnt(0)\n"                                                                                          \
    "s_branch .Lcached_%=\n"
// The y-INTERLEAVED volume (sdfv_commit_interleaved): rows 2p and 2p + 1 of a slice share one row of (d[2p][x], d[2p+1][x])
// pairs -- 4 B/voxel like the distance volume, no duplication.  A cell whose j0 is even finds the four corners of a z-level
// in 16 contiguous bytes of pair-row j0/2; an odd j0 takes (x0, x1) of row j0 from pair-row (j0-1)/2 and of row j0+1 from
// pair-row (j0+1)/2.  Branch-free: every lane loads pair-rows j0 >> 1 and (j0 + 1) >> 1 (the same address, hence the same
// line, when j0 is even) and picks by parity -- four dwordx4 gathers over 2 (even) or 4 (odd) lines instead of four dwordx2
// over 4 lines: the line count is what a fetch costs (EXPERIMENTS R3.1, R3.10).
#define SDFV_MARCH_ASM_INTERIOR_ILV                                                                                 \
    "s_lshr_b32 s80, %[h], 1\n"                                                                                     \
    "v_and_b32_e32 v48, 1, v33\n"                            /* parity of j0 */                                      \
    "v_lshrrev_b32_e32 v35, 1, v33\n"                        /* p0 = j0 >> 1 */                                      \
    "v_add_u32_e32 v36, 1, v33\n"                                                                                   \
    "v_lshrrev_b32_e32 v36, 1, v36\n"                        /* p1 = (j0 + 1) >> 1 */                                \
    "v_mad_u32_u24 v35, v34, s80, v35\n v_mad_u32_u24 v36, v34, s80, v36\n"     /* pair rows k0 * H/2 + p */         \
    "v_mad_u32_u24 v35, v35, %[w], v32\n v_mad_u32_u24 v37, v36, %[w], v32\n"                                        \
    "v_lshlrev_b32_e32 v36, 3, v35\n v_lshlrev_b32_e32 v37, 3, v37\n"                                               \
    "v_cmp_eq_u32_e32 vcc, 1, v48\n"                                                                                \
    "global_load_dwordx4 v[24:27], v36, %[base]\n"           /* z0, pair-row p0: (y_lo, y_hi) at x0, x1 */           \
    "global_load_dwordx4 v[32:35], v36, s[68:69]\n"          /* z1, p0 */                                            \
    "s_and_saveexec_b64 s[80:81], vcc\n"                     /* odd j0 only: row j0 + 1 lives in the next pair-row */ \
    "global_load_dwordx3 v[28:30], v37, %[base]\n"           /* z0, p1: its y_lo at x0, x1 */                        \
    "global_load_dwordx3 v[36:38], v37, s[68:69]\n"          /* z1, p1 */                                            \
    "s_mov_b64 exec, s[80:81]\n"                                                                                    \
    "s_waitcnt vmcnt(2)\n"                                                                                          \
    "v_cndmask_b32_e32 v60, v24, v25, vcc\n v_cndmask_b32_e32 v62, v26, v27, vcc\n"   /* t000, t100: row j0 */       \
    "v_cndmask_b32_e32 v61, v32, v33, vcc\n v_cndmask_b32_e32 v63, v34, v35, vcc\n"   /* t001, t101 */               \
    "s_waitcnt vmcnt(0)\n"                                                                                          \
    "v_cndmask_b32_e32 v64, v25, v28, vcc\n v_cndmask_b32_e32 v66, v27, v30, vcc\n"   /* t010, t110: row j0 + 1 */   \
    "v_cndmask_b32_e32 v65, v33, v36, vcc\n v_cndmask_b32_e32 v67, v35, v38, vcc\n"   /* t011, t111 */
// Border cells of the interleaved volume: eight dword loads at (pair-row * W + x) * 8 + (y & 1) * 4.  The clamped row
// numbers of FETCH_PREP are k * H + j with H even: the pair-row is row >> 1, the half row & 1.
#define SDFV_MARCH_ASM_ILV_ROW(R)                            /* v R: row number k * H + j  ->  byte offset of (x = 0) */ \
    "v_and_b32_e32 v36, 1, v" #R "\n"                        /* y & 1 */                                             \
    "v_lshrrev_b32_e32 v" #R ", 1, v" #R "\n"                /* k * H/2 + (j >> 1): H is even */                     \
    "v_mul_u32_u24_e32 v" #R ", s85, v" #R "\n"              /* * W * 8 */                                           \
    "v_lshl_add_u32 v" #R ", v36, 2, v" #R "\n"              /* + (y & 1) * 4 */
#define SDFV_MARCH_ASM_FETCH_ILV                                                                                    \
    "v_lshlrev_b32_e32 v35, 3, v35\n v_lshlrev_b32_e32 v32, 3, v32\n"   /* i0c, i1c as byte offsets (8 per x) */      \
    SDFV_MARCH_ASM_ILV_ROW(28) SDFV_MARCH_ASM_ILV_ROW(29) SDFV_MARCH_ASM_ILV_ROW(30) SDFV_MARCH_ASM_ILV_ROW(31)       \
    "v_add_u32_e32 v24, v28, v35\n v_add_u32_e32 v25, v28, v32\n"                                                    \
    "global_load_dword v60, v24, %[base]\n global_load_dword v62, v25, %[base]\n"                                  \
    "v_add_u32_e32 v26, v29, v35\n v_add_u32_e32 v27, v29, v32\n"                                                    \
    "global_load_dword v64, v26, %[base]\n global_load_dword v66, v27, %[base]\n"                                  \
    "v_add_u32_e32 v24, v30, v35\n v_add_u32_e32 v25, v30, v32\n"                                                    \
    "global_load_dword v61, v24, %[base]\n global_load_dword v63, v25, %[base]\n"                                  \
    "v_add_u32_e32 v26, v31, v35\n v_add_u32_e32 v27, v31, v32\n"                                                    \
    "global_load_dword v65, v26, %[base]\n global_load_dword v67, v27, %[base]\n"                                  \
    "s_waitcnt vmcnt(0)\n"                                                                                          \
    "s_branch .Lcached_%=\n"
// The distance volume: x-neighbours are adjacent floats: one 8-byte load per (y, z) row at b = clamp(i0, 0, W - 2); where the clamp
// folds the two x-corners together both come from the same half (lo_is_x / hi_is_y).
#define SDFV_MARCH_ASM_FETCH_DIST                                                                                   \
    "v_min_i32_e32 v36, s75, v35\n"                          /* b = min(i0c, W - 2) */                               \
    "v_lshlrev_b32_e32 v39, 2, v36\n"                                                                               \
    "v_mad_u32_u24 v28, v28, s82, v39\n v_mad_u32_u24 v29, v29, s82, v39\n"                                          \
    "v_mad_u32_u24 v30, v30, s82, v39\n v_mad_u32_u24 v31, v31, s82, v39\n"                                          \
    "global_load_dwordx2 v[24:25], v28, %[base]\n"           /* (z0, y0) */                                          \
    "global_load_dwordx2 v[26:27], v29, %[base]\n"           /* (z0, y1) */                                          \
    "global_load_dwordx2 v[28:29], v30, %[base]\n"           /* (z1, y0) */                                          \
    "global_load_dwordx2 v[30:31], v31, %[base]\n"           /* (z1, y1) */                                          \
    "v_cmp_eq_u32_e64 s[80:81], v35, v36\n"                  /* lo_is_x */                                           \
    "v_add_u32_e32 v36, 1, v36\n"                                                                                   \
    "v_cmp_eq_u32_e32 vcc, v32, v36\n"                       /* hi_is_y */                                           \
    "s_waitcnt vmcnt(3)\n"                                                                                          \
    "v_cndmask_b32_e64 v60, v25, v24, s[80:81]\n v_cndmask_b32_e32 v62, v24, v25, vcc\n" /* t000, t100 */          \
    "s_waitcnt vmcnt(2)\n"                                                                                          \
    "v_cndmask_b32_e64 v64, v27, v26, s[80:81]\n v_cndmask_b32_e32 v66, v26, v27, vcc\n" /* t010, t110 */          \
    "s_waitcnt vmcnt(1)\n"                                                                                          \
    "v_cndmask_b32_e64 v61, v29, v28, s[80:81]\n v_cndmask_b32_e32 v63, v28, v29, vcc\n" /* t001, t101 */          \
    "s_waitcnt vmcnt(0)\n"                                                                                          \
    "v_cndmask_b32_e64 v65, v31, v30, s[80:81]\n v_cndmask_b32_e32 v67, v30, v31, vcc\n" /* t011, t111 */          \
    "s_branch .Lcached_%=\n"
// tex0.r out of 16-byte texels, one dword load per corner.
#define SDFV_MARCH_ASM_FETCH_TEX0                                                                                   \
    "v_lshlrev_b32_e32 v35, 4, v35\n v_lshlrev_b32_e32 v32, 4, v32\n"   /* i0c, i1c as byte offsets */               \
    "v_mad_u32_u24 v24, v28, s83, v35\n v_mad_u32_u24 v25, v28, s83, v32\n"                                          \
    "global_load_dword v60, v24, %[base]\n global_load_dword v62, v25, %[base]\n"                                  \
    "v_mad_u32_u24 v26, v29, s83, v35\n v_mad_u32_u24 v27, v29, s83, v32\n"                                          \
    "global_load_dword v64, v26, %[base]\n global_load_dword v66, v27, %[base]\n"                                  \
    "v_mad_u32_u24 v24, v30, s83, v35\n v_mad_u32_u24 v25, v30, s83, v32\n"                                          \
    "global_load_dword v61, v24, %[base]\n global_load_dword v63, v25, %[base]\n"                                  \
    "v_mad_u32_u24 v26, v31, s83, v35\n v_mad_u32_u24 v27, v31, s83, v32\n"                                          \
    "global_load_dword v65, v26, %[base]\n global_load_dword v67, v27, %[base]\n"                                  \
    "s_waitcnt vmcnt(0)\n"                                                                                          \
    "s_branch .Lcached_%=\n"
// Corner registers as z-pairs: A0 = v[60:61] = (t000, t001), A1 = v[62:63] = (t100, t101), B0 = v[64:65] =
// (t010, t011), B1 = v[66:67] = (t110, t111); weights (a, 1 - a) as pairs v[52:53], v[54:55], v[56:57].
#define SDFV_MARCH_ASM_FILTER                                                                                       \
    "s_mov_b64 exec, s[78:79]\n"                                                                                    \
    "v_sub_f32_e32 v53, 1.0, v52\n v_sub_f32_e32 v55, 1.0, v54\n v_sub_f32_e32 v57, 1.0, v56\n"                \
    /* mix along x: c = t(x0) * (1 - ax) + t(x1) * ax */                                                            \
    "v_pk_mul_f32 v[34:35], v[62:63], v[52:53] op_sel_hi:[1,0]\n"                                                \
    "v_pk_mul_f32 v[38:39], v[66:67], v[52:53] op_sel_hi:[1,0]\n"                                                \
    "v_pk_mul_f32 v[32:33], v[60:61], v[52:53] op_sel:[0,1] op_sel_hi:[1,1]\n"                                   \
    "v_pk_mul_f32 v[36:37], v[64:65], v[52:53] op_sel:[0,1] op_sel_hi:[1,1]\n"                                   \
    "v_pk_add_f32 v[32:33], v[32:33], v[34:35]\n"            /* (c00, c01) */                                        \
    "v_pk_add_f32 v[36:37], v[36:37], v[38:39]\n"            /* (c10, c11) */                                        \
    /* mix along y */                                                                                               \
    "v_pk_mul_f32 v[32:33], v[32:33], v[54:55] op_sel:[0,1] op_sel_hi:[1,1]\n"                                     \
    "v_pk_mul_f32 v[36:37], v[36:37], v[54:55] op_sel_hi:[1,0]\n"                                                  \
    "v_pk_add_f32 v[32:33], v[32:33], v[36:37]\n"            /* (c0, c1) */                                          \
    /* mix along z, then sample_dist = r - 0.1 */                                                                   \
    "v_pk_mul_f32 v[32:33], v[32:33], v[56:57] op_sel:[0,1] op_sel_hi:[1,0]\n" /* (c0 * (1 - az), c1 * az) */      \
    "v_add_f32_e32 v36, v32, v33\n"                                                                                 \
    "v_add_f32_e32 v36, 0xbdcccccd, v36\n"                                                                          \
    /* hit?  (material.frag:117-121) */                                                                             \
    "v_cmpx_ngt_f32_e32 vcc, 0x3727c5ac, v36\n"              /* exec &= !(1e-5 > sample_dist) */
#define SDFV_MARCH_ASM_ADVANCE                                                                                      \
    /* advance the rays that go on (material.frag:124-125) */                                                       \
    "v_mul_f32_e32 v32, v44, v36\n"                                                                                \
    "v_pk_mul_f32 v[34:35], v[46:47], v[36:37] op_sel_hi:[1,0]\n"                                                  \
    "v_add_f32_e32 v40, v40, v32\n"                                                                                 \
    "v_pk_add_f32 v[42:43], v[42:43], v[34:35]\n"                                                                   \
    "s_add_u32 s74, s74, -1\n"                               /* carry out <=> iterations left */                     \
    "s_cbranch_scc1 .Lloop_%=\n"                                                                                    \
    "s_branch .Ldone_%=\n"
#define SDFV_MARCH_ASM_EPILOGUE                                                                                     \
    ".Ldone_%=:\n"                                                                                                  \
    "s_mov_b64 %[ran], exec\n"                               /* lanes still marching after 255 iterations */         \
    "s_mov_b32 %[left], s74\n"                                                                                      \
    SDFV_MARCH_ASM_TUNE("s_lshl_b32 s84, s84, 16\n s_and_b32 %[left], %[left], 0xffff\n s_or_b32 %[left], %[left], s84\n") \
    "s_and_b64 exec, s[76:77], %[cov]\n"                                                                            \
    "s_nop 0\n"
#define SDFV_MARCH_ASM_END "s_mov_b64 exec, s[76:77]\n"
#define SDFV_MARCH_ASM_OPERANDS                                                                                     \
    [dx] "v"(dirx), [dy] "v"(diry), [dz] "v"(dirz), [cov] "s"(cov), [mx] "s"(a.rp.bounds_max[0]),    \
        [my] "s"(a.rp.bounds_max[1]), [mz] "s"(a.rp.bounds_max[2]), [minx] "s"(a.rp.bounds_min[0]),                 \
        [miny] "s"(a.rp.bounds_min[1]), [minz] "s"(a.rp.bounds_min[2]), [kx] "s"(kx), [ky] "s"(ky), [kz] "s"(kz),   \
        [wm1] "s"(wm1), [hm1] "s"(hm1), [dm1] "s"(dm1), [w] "s"(t.w), [h] "s"(t.h), [base] "s"(vol), [base_lo] "s"(base_lo), [base_hi] "s"(base_hi), [thresh] "s"(thresh)
#define SDFV_MARCH_ASM_CLOBBERS                                                                                     \
    "vcc", "scc", "memory", "s64", "s65", "s66", "s67", "s68", "s69", "s70", "s71", "s72", "s73", "s74", "s75",    \
        "s76", "s77", "s78", "s79", "s80", "s81", "s82", "s83", "s84", "s85", "s86", "s87", "v24", "v25", "v26", "v27", "v28",  \
        "v29", "v30", "v31", "v32", "v33", "v34", "v35", "v36", "v37", "v38", "v39", "v48", "v50", "v51", "v52",    \
        "v53", "v54", "v55", "v56", "v57", "v58", "v59", "v60", "v61", "v62", "v63", "v64", "v65", "v66", "v67", "v68",   \
        "v70", "v71"

template <int MODE, bool T>
__device__ __forceinline__ void march_asm(const RaymarchArgs& a, const Tex& t, V3 ray_dir, bool covered, V3& ray_pos,
                                          float& dist_from_origin, int& status, int& steps, int& iterations) {
    const float* __restrict__ vol = march_volume<MODE>(a);
    // float multiplies are VALU work on gfx950: the (uniform) products are moved to scalar registers explicitly
    auto uniform = [](float f) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(f))); };
    const float kx = uniform(a.inv_bsize[0] * (float)t.w), ky = uniform(a.inv_bsize[1] * (float)t.h),
                kz = uniform(a.inv_bsize[2] * (float)t.d);  // exact: a power of two times an integer below 2^24
    const int wm1 = t.w - 1, hm1 = t.h - 1, dm1 = t.d - 1;
    const unsigned long long cov = __ballot(covered);
    const uint32_t base_lo = (uint32_t)(uintptr_t)vol, base_hi = (uint32_t)((uintptr_t)vol >> 32);
    // the interior fetch path tests all three cell indices with ONE compare: cubic volumes only (0: never taken)
    const uint32_t thresh = (t.w == t.h && t.h == t.d && !a.no_interior_fetch) ? (uint32_t)t.w - 1u : 0u;
    unsigned long long ran_out;
    int left = 254;  // the loop's down-counter at exit (tuning build: iterations the wave ran)
    // The block's position and direction registers are the operands themselves (explicit register variables: no copies in
    // or out, and six registers fewer than operands + copies): (py, pz) and (dy, dz) must be aligned pairs for v_pk_*.
    register float px asm("v40") = ray_pos.x;
    register float py asm("v42") = ray_pos.y;
    register float pz asm("v43") = ray_pos.z;
    register float dirx asm("v44") = ray_dir.x;
    register float diry asm("v46") = ray_dir.y;
    register float dirz asm("v47") = ray_dir.z;
#define SDFV_MARCH_ASM_OOB_BOX SDFV_MARCH_ASM_OOB4_A, SDFV_MARCH_ASM_OOB4_B, SDFV_MARCH_ASM_OOB4_C, SDFV_MARCH_ASM_OOB4_D
#define SDFV_MARCH_ASM_OOB_CUBE SDFV_MARCH_ASM_OOB2_A, "", "", SDFV_MARCH_ASM_OOB2_D
#define SDFV_MARCH_ASM_TOP_(T_STEP, ...) SDFV_MARCH_ASM_TOP(T_STEP, __VA_ARGS__)
// aux variant: distanceFromOrigin (v58) and the per-ray fetch count (v59) ride along
#define SDFV_MARCH_ASM_RUN_AUX(SHIFT, INTERIOR, FETCH, OOB)                                                         \
    asm volatile("v_mov_b32 v58, %[tt]\n v_mov_b32 v59, 0\n" SDFV_MARCH_ASM_HEAD(SHIFT)                             \
                 SDFV_MARCH_ASM_TOP_("v_add_u32_e32 v59, 1, v59\n", OOB) SDFV_MARCH_ASM_FILTER                       \
                 "v_add_f32_e32 v58, v58, v36\n" SDFV_MARCH_ASM_ADVANCE SDFV_MARCH_ASM_FETCH_PREP(INTERIOR) FETCH    \
                 SDFV_MARCH_ASM_EPILOGUE "v_mov_b32 %[tt], v58\n v_mov_b32 %[n], v59\n" SDFV_MARCH_ASM_END           \
                 : [px] "+v"(px), [py] "+v"(py), [pz] "+v"(pz), [tt] "+v"(tt), [n] "+v"(n), [ran] "=&s"(ran_out),   \
                   [left] "=&s"(left)                                                                               \
                 : SDFV_MARCH_ASM_OPERANDS                                                                          \
                 : SDFV_MARCH_ASM_CLOBBERS)
#define SDFV_MARCH_ASM_RUN(SHIFT, INTERIOR, FETCH, OOB)                                                             \
    asm volatile(SDFV_MARCH_ASM_HEAD(SHIFT) SDFV_MARCH_ASM_TOP_("", OOB) SDFV_MARCH_ASM_FILTER SDFV_MARCH_ASM_ADVANCE \
                     SDFV_MARCH_ASM_FETCH_PREP(INTERIOR) FETCH SDFV_MARCH_ASM_EPILOGUE SDFV_MARCH_ASM_END            \
                 : [px] "+v"(px), [py] "+v"(py), [pz] "+v"(pz), [ran] "=&s"(ran_out), [left] "=&s"(left)            \
                 : SDFV_MARCH_ASM_OPERANDS                                                                          \
                 : SDFV_MARCH_ASM_CLOBBERS)
// each volume's row-bytes register, interior fetch and border fetch
#define SDFV_MARCH_ASM_VOL_TEX0 "s83", SDFV_MARCH_ASM_INTERIOR_TEX0, SDFV_MARCH_ASM_FETCH_TEX0
#define SDFV_MARCH_ASM_VOL_DIST "s82", SDFV_MARCH_ASM_INTERIOR_DIST, SDFV_MARCH_ASM_FETCH_DIST
#define SDFV_MARCH_ASM_VOL_PAIRS "s85", SDFV_MARCH_ASM_INTERIOR_PAIRS, SDFV_MARCH_ASM_FETCH_PAIRS
#define SDFV_MARCH_ASM_VOL_ILV "s82", SDFV_MARCH_ASM_INTERIOR_ILV, SDFV_MARCH_ASM_FETCH_ILV
#define SDFV_MARCH_ASM_PER_BOX(RUN, ...)                                                                            \
    if (cube) RUN(__VA_ARGS__, SDFV_MARCH_ASM_OOB_CUBE);                                                            \
    else RUN(__VA_ARGS__, SDFV_MARCH_ASM_OOB_BOX)
#define SDFV_MARCH_ASM_PER_VOLUME(RUN)                                                                              \
    if (MODE == kMarchIlv) { SDFV_MARCH_ASM_PER_BOX(RUN, SDFV_MARCH_ASM_VOL_ILV); }                                 \
    else if (MODE == kMarchPairs) { SDFV_MARCH_ASM_PER_BOX(RUN, SDFV_MARCH_ASM_VOL_PAIRS); }                        \
    else if (MODE == kMarchDist) { SDFV_MARCH_ASM_PER_BOX(RUN, SDFV_MARCH_ASM_VOL_DIST); }                          \
    else { SDFV_MARCH_ASM_PER_BOX(RUN, SDFV_MARCH_ASM_VOL_TEX0); }
    const bool cube = a.cube_box != 0;  // wave-uniform: one scalar branch per kernel
    if (T) {
        float tt = dist_from_origin;
        int n = 0;
        SDFV_MARCH_ASM_PER_VOLUME(SDFV_MARCH_ASM_RUN_AUX)
        dist_from_origin = tt;
        steps = n;
    } else {
        SDFV_MARCH_ASM_PER_VOLUME(SDFV_MARCH_ASM_RUN)
    }
#ifdef SDFV_TUNING  // left = (iterations that ran the fetch block) << 16 | the down-counter at exit
    iterations = cov ? (min(255, 255 - (int)(short)(left & 0xffff)) | (left & 0xffff0000)) : 0;
#else
    (void)iterations;
    (void)left;
#endif
    if (covered) {
        ray_pos = mk(px, py, pz);
        const bool ran = ((ran_out >> (threadIdx.x & 63)) & 1ull) != 0;
        // a stopped ray's position no longer moves: "out of bounds" is re-derived from it, as in march_fast
        status = ran ? -1 : (oob_dist<true>(a, ray_pos) > 1e-4f ? -2 : 1);
    }
}

}  // namespace
}  // namespace sdfv
