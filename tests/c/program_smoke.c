/* program_smoke.c -- SDF programs from plain C (C11, no C++, no Python): a two-primitive program is built, filled densely at
 * 32^3 and loaded through sdfv_viewer_update; the two results must be the same bits. */
#include <hip/hip_runtime_api.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "sdfprogram.h"

#define N 32
#define CHECK(call)                                                                      \
    do {                                                                                 \
        int rc_ = (call);                                                                \
        if (rc_ != 0) {                                                                  \
            fprintf(stderr, "%s:%d: %s -> %d (%s)\n", __FILE__, __LINE__, #call, rc_, sdfv_last_error()); \
            return 1;                                                                    \
        }                                                                                \
    } while (0)

int main(void) {
    sdfv_prog_op ops[5];
    const float bb[6] = {-1.0f, -1.0f, -1.0f, 1.0f, 1.0f, 1.0f};
    const uint32_t dims[3] = {N, N, N};
    const size_t texels = (size_t)N * N * N, bytes = texels * 16;
    sdfv_program *prog = NULL;
    sdfv_surface surface;
    sdfv_viewer *viewer = NULL;
    sdfv_grid grid;
    sdfv_load_state state;
    float *d0 = NULL, *d1 = NULL, *fill0, *fill1, *load0, *load1;
    size_t visited = 0, calls = 0;

    memset(ops, 0, sizeof(ops));
    ops[0].op = SDFV_OP_MATERIAL; /* red, a little metallic */
    ops[0].a[0] = 0.8f; ops[0].a[1] = 0.1f; ops[0].a[2] = 0.1f; ops[0].a[3] = 0.3f; ops[0].a[4] = 0.5f; ops[0].a[5] = 1.0f;
    ops[1].op = SDFV_OP_BOX;
    ops[1].a[0] = 0.7f; ops[1].a[1] = 0.5f; ops[1].a[2] = 0.3f;
    ops[2].op = SDFV_OP_MATERIAL; /* blue */
    ops[2].a[0] = 0.1f; ops[2].a[1] = 0.2f; ops[2].a[2] = 0.9f; ops[2].a[4] = 0.2f; ops[2].a[5] = 0.5f;
    ops[3].op = SDFV_OP_SPHERE;
    ops[3].a[0] = 0.6f;
    ops[4].op = SDFV_OP_SMOOTH_UNION;
    ops[4].a[0] = 0.1f;
    CHECK(sdfv_program_create(ops, 5, bb, &prog));

    /* the dense fill */
    memset(&grid, 0, sizeof(grid));
    for (int i = 0; i < 3; ++i) {
        grid.dims[i] = N;
        grid.bb_min[i] = bb[i];
        grid.bb_max[i] = bb[3 + i];
    }
    grid.z_end = N;
    if (hipMalloc((void **)&d0, bytes) != hipSuccess || hipMalloc((void **)&d1, bytes) != hipSuccess) return 2;
    CHECK(sdfv_program_fill_grid_commit(prog, &grid, d0, d1, NULL, 0, NULL));
    fill0 = malloc(bytes); fill1 = malloc(bytes); load0 = malloc(bytes); load1 = malloc(bytes);
    if (!fill0 || !fill1 || !load0 || !load1) return 2;
    if (hipMemcpy(fill0, d0, bytes, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(fill1, d1, bytes, hipMemcpyDeviceToHost) != hipSuccess)
        return 2;

    /* the progressive load of the same program through the viewer */
    CHECK(sdfv_program_as_surface(prog, &surface));
    if (!surface.sample_batch_device || !surface.sample) return 3;
    CHECK(sdfv_viewer_new_voxels(dims, bb, 3, SDFV_LAYOUT_AUTO, &viewer));
    do {
        CHECK(sdfv_viewer_update(viewer, &surface, 30000000u, &visited));
        CHECK(sdfv_viewer_state(viewer, &state));
        if (++calls > 100000) return 4;
    } while (state.remaining);
    CHECK(sdfv_viewer_download(viewer, load0, load1));
    if (memcmp(fill0, load0, bytes) != 0 || memcmp(fill1, load1, bytes) != 0) {
        fprintf(stderr, "the loaded textures differ from the dense fill\n");
        return 5;
    }
    /* something was drawn into it: both materials and air */
    {
        size_t inside = 0;
        for (size_t i = 0; i < texels; ++i) inside += fill0[4 * i] < 0.1f;
        if (inside == 0 || inside == texels) return 6;
    }
    sdfv_viewer_free(viewer);
    sdfv_program_free(prog);
    (void)hipFree(d0);
    (void)hipFree(d1);
    free(fill0); free(fill1); free(load0); free(load1);
    printf("program_smoke ok (%zu update calls)\n", calls);
    return 0;
}
