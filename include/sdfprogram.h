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
 *   changed, device_params  NULL: a program does not change -- an edit is a new program and a new surface (sdfv_scene_set_surface)
 * `user` is the program: it must outlive every use of the surface.  A caller that wants the host route on purpose clears
 * out->sample_batch_device.  Returns SDFV_ERR_INVALID_ARGUMENT for a NULL argument. */
int sdfv_program_as_surface(const sdfv_program *p, sdfv_surface *out);

/* sdfv_program_raymarch (sdfgrid.h) evaluated ON THE HOST: the same descriptor, the same checks and messages
 * (sdfv_program_raymarch_check; sdfv_last_error() has the text), the same per-pixel source as the kernel -- rgba, depth, aux and
 * rgba8 are HOST buffers here, and everything in aux and depth is bit for bit what the device writes (rgba within 1e-4: libm's
 * powf against the device's).  Needs no device: the route of a caller without one, and the CPU baseline of the device's.
 * n_threads: rows are dealt to that many threads (the viewer's worker pool); <= 0 = the CPUs this process may use. */
int sdfv_program_raymarch_host(const sdfv_program_march_desc *desc, int n_threads);

#ifdef __cplusplus
}
#endif
#endif
