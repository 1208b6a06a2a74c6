/*
 * sdfviewer_mesh.h -- the viewer's mesh call: SDFViewer::mesh over the C ABI.  Exported by libsdfviewer_host.so.
 *
 * An addition beside sdfviewer.h, which stays ABI version 1 as it is (as sdfv_viewer_update_program lives in sdfprogram.h): a
 * binder that does not mesh needs nothing from here.  Conventions are sdfviewer.h's: an sdfv_status is returned, the handle
 * keeps the message of its last failure (sdfv_viewer_last_error), a handle is used by one thread at a time.
 */
#ifndef SDFVIEWER_MESH_H
#define SDFVIEWER_MESH_H

#include <stdint.h>

#include "sdfgrid.h"
#include "sdfviewer.h"

#ifdef __cplusplus
extern "C" {
#endif

/* SDFViewer::mesh: the grid as it is loaded now through sdfv_grid_mesh_extract (sdfgrid.h, "Meshing a loaded grid") -- the
 * voxels published at the current lod_dist_between_samples, on the viewer's stream, read from the distance volume in the layout
 * the viewer keeps (tex0 without one), the rows no pass has reached materialised first.  Not while an update is running.
 * algorithm: SDFV_MESHER_*; flags: 0 or SDFV_MESH_WITH_MATERIALS.  out: a DEVICE mesh, freed with sdfv_mesh_free; zeroed on
 * failure. */
int sdfv_viewer_mesh(sdfv_viewer *v, uint32_t algorithm, uint32_t flags, sdfv_mesh *out);

#ifdef __cplusplus
}
#endif
#endif
