/*
 * sdfprogram.h -- an SDF program (sdfgrid.h, "SDF programs") as a surface of the viewer.  Exported by libsdfviewer_host.so.
 *
 * The viewer of sdfviewer.h loads any `sdfv_surface`; this header makes one out of a program, so that sdfv_viewer_update and
 * the sdfv_scene_* calls load a caller-defined CSG tree progressively through the viewer's device-sampled route -- the
 * LoadingManager's points are emitted on the device, sampled by the program interpreter (sdfv_program_sample_points) and
 * packed, with nothing crossing to the host -- and no change to the viewer.  It also holds the host mirror of the direct march.
 */
#ifndef SDFPROGRAM_H
#define SDFPROGRAM_H

#include "sdfviewer.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Fills *out with a surface over `p`:
 *   bounding_box         the box the program was created with
 *   sample, sample_batch the program evaluated ON THE HOST by the same interpreter source as the kernels (bit for bit the
 *                        device's results); stateless, so sample_concurrency answers "any number of threads"
 *   sample_batch_device  sdfv_program_sample_points on the viewer's stream; NULL when no HIP device is visible (the host
 *                        callbacks are then the only usable ones, and the call still succeeds)
 *   changed, device_params  NULL: a program does not change -- an edit is a new program and a new surface
 *                        (sdfv_scene_set_surface), or goes through a program editor (below), whose surface does report changes
 * `user` is the program: it must outlive every use of the surface.  A caller that wants the host route on purpose clears
 * out->sample_batch_device.  Returns SDFV_ERR_INVALID_ARGUMENT for a NULL argument. */
int sdfv_program_as_surface(const sdfv_program *p, sdfv_surface *out);

/* sdfv_program_raymarch (sdfgrid.h) evaluated ON THE HOST: the same descriptor, the same checks and messages
 * (sdfv_program_raymarch_check; sdfv_last_error() has the text), the same per-pixel source as the kernel -- rgba, depth, aux and
 * rgba8 are HOST buffers here, and everything in aux and depth is bit for bit what the device writes (rgba within 1e-4: libm's
 * powf against the device's).  Needs no device: the route of a caller without one, and the CPU baseline of the device's.
 * n_threads: rows are dealt to that many threads (the viewer's worker pool); <= 0 = the CPUs this process may use. */
int sdfv_program_raymarch_host(const sdfv_program_march_desc *desc, int n_threads);

/* sdfv_program_raycast (sdfgrid.h) evaluated ON THE HOST: the same descriptor, the same checks and messages
 * (sdfv_program_raycast_check; sdfv_last_error() has the text), the same per-ray source as the kernel -- rays and hits are HOST
 * arrays here, and every byte of every record is what the device writes.  Needs no device.  Runs of 256 rays are dealt to the
 * CPUs this process may use (the viewer's worker pool). */
int sdfv_program_raycast_host(const sdfv_program_cast_desc *desc);

/* ---- the program editor: parameters, set_parameter and changed (src/sdf/mod.rs:60-86) for a program ----
 * Program handles stay immutable.  An editor holds the instructions, a list of float parameters and the CURRENT SNAPSHOT, an
 * sdfv_program made by sdfv_program_create; every accepted edit makes a new snapshot through the same validator.  Replaced
 * snapshots stay alive until sdfv_program_editor_free, or until the caller calls sdfv_program_editor_trim AFTER synchronising
 * the streams that may still run one: the library synchronises nothing behind the caller's back, and nothing races with a
 * kernel in flight.  An editor is single-owner: one thread at a time.
 *
 * A parameter mirrors the reference's SDFParam with kind Float{range: min..=max, step}: id, name, description, a current value,
 * and up to SDFV_PARAM_MAX_TARGETS targets -- operand `operand` of instruction `op` receives the value (SDFV_PARAM_VALUE), its
 * negation -v (SDFV_PARAM_NEGATED: the translation column of a pure-translation PUSH_AFFINE, which holds the inverse) or its
 * reciprocal 1.0f / v, one IEEE division (SDFV_PARAM_RECIPROCAL: inv_s of PUSH_SCALE s inv_s ... POP_SCALE s).  `box`
 * (has_box != 0) is the part of space an edit of this parameter can change, DECLARED by the caller as in the reference, where
 * the SDF says what changed; without it the program's bounding box stands in.  The library derives no boxes. */
typedef struct sdfv_program_editor sdfv_program_editor;
enum { SDFV_PARAM_VALUE = 0, SDFV_PARAM_NEGATED = 1, SDFV_PARAM_RECIPROCAL = 2 };
#define SDFV_PARAM_MAX_TARGETS 4
typedef struct sdfv_param_target {
    uint32_t op;      /* instruction index */
    uint32_t operand; /* 0 .. 11 */
    uint32_t kind;    /* SDFV_PARAM_* */
} sdfv_param_target;
typedef struct sdfv_program_param {
    uint32_t id;
    const char *name;
    const char *description; /* may be NULL */
    float min, max, step;
    float value;
    uint32_t n_targets;
    sdfv_param_target targets[SDFV_PARAM_MAX_TARGETS];
    uint32_t has_box;
    float box[6]; /* min.xyz max.xyz */
} sdfv_program_param;

/* Copies everything (the strings too), writes every parameter's value to its targets and makes the first snapshot.
 * SDFV_ERR_INVALID_ARGUMENT for: NULL arguments, duplicate ids, a NULL name, a range that is
 * not finite or has max < min, a value outside it, no target or more than SDFV_PARAM_MAX_TARGETS, a target outside the program,
 * an unknown kind, a box that is not finite or inverted -- and whatever sdfv_program_create refuses, with its message
 * (sdfv_program_editor_last_error(NULL) has the text). */
int sdfv_program_editor_create(const sdfv_prog_op *ops, size_t n, const float bb[6], const sdfv_program_param *params,
                               size_t n_params, sdfv_program_editor **out);
void sdfv_program_editor_free(sdfv_program_editor *e); /* NULL is fine; synchronise the streams that use its snapshots first */
/* the parameters with their current values; *params stays valid until the editor is freed (the values move with every set) */
int sdfv_program_editor_parameters(const sdfv_program_editor *e, const sdfv_program_param **params, size_t *n);
/* set_parameter.  Refused with SDFV_ERR_INVALID_ARGUMENT -- value, snapshot and pending box unchanged,
 * sdfv_program_editor_last_error() has the text -- for an unknown id, a value that is not finite or lies outside [min, max],
 * and a value the validator refuses (k <= 0, ...: the validator's own message).  Otherwise the new snapshot becomes current and
 * the parameter's box is merged into the pending box (merge_bounding_boxes, defaults.rs:59-72). */
int sdfv_program_editor_set(sdfv_program_editor *e, uint32_t id, float value);
/* SDFDemo::changed: 1 = the pending box written to out, and it is pending no more; 0 = None */
int sdfv_program_editor_changed(sdfv_program_editor *e, float out[6]);
/* the current snapshot: owned by the editor, alive until sdfv_program_editor_trim after a later set, or the editor's end */
const sdfv_program *sdfv_program_editor_program(const sdfv_program_editor *e);
/* frees the replaced snapshots; the caller has synchronised every stream that may still run one */
int sdfv_program_editor_trim(sdfv_program_editor *e);
/* never NULL; e == NULL: the calling thread's last failed sdfv_program_editor_create */
const char *sdfv_program_editor_last_error(const sdfv_program_editor *e);
/* sdfv_program_as_surface over the current snapshot, whichever that is at the time of each call, with `changed` set
 * (sdfv_program_editor_changed): it loads and RE-loads through the viewer's device-sampled route -- sdfv_viewer_update finds the
 * box and re-samples the voxels inside it.  `user` is the editor. */
int sdfv_program_editor_as_surface(sdfv_program_editor *e, sdfv_surface *out);

/* SDFViewer::update(editor, max_delta_time) with WHOLE PASSES as the unit of work, as the demo loads: the same load state
 * machine as sdfv_viewer_update (the editor's changed() is asked once at the start), but every LoadingManager pass is one
 * sdfv_program_grid_pass over the current snapshot -- its box launch and its scan -- and a fresh load or a box that covers
 * the grid is one sdfv_program_fill_grid_commit; the budget is checked between passes.  Same textures and the same
 * sdfv_load_state as sdfv_viewer_update with sdfv_program_editor_as_surface once both have run their passes. */
int sdfv_viewer_update_program(sdfv_viewer *v, sdfv_program_editor *e, uint64_t budget_ns, size_t *visited);

#ifdef __cplusplus
}
#endif
#endif
