/* dep_exports.c -- TEST FIXTURE: an ordinary library that a provider links against and that happens to export functions with
 * the provider ABI's generic optional names (init, name, normal, children, sample_concurrency; include/sdf_provider.h).  A
 * consumer must not take them for the provider's own exports.  dep_init_calls() tells the test whether init() ran. */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "sdf_provider.h"

#define EXPORT __attribute__((visibility("default")))

static int g_init_calls = 0;

EXPORT int dep_init_calls(void) { return g_init_calls; }

EXPORT void init(void) { g_init_calls += 1; }

EXPORT PointerLength *name(uint32_t sdf_id) {
    (void)sdf_id;
    PointerLength *ret = (PointerLength *)calloc(1, sizeof *ret);
    char *s = (char *)malloc(10);
    memcpy(s, "Dependency", 10);
    ret->ptr = s;
    ret->len_bytes = 10;
    return ret;
}

EXPORT PointerLength *children(uint32_t sdf_id) {
    (void)sdf_id;
    PointerLength *ret = (PointerLength *)calloc(1, sizeof *ret);
    uint32_t *ids = (uint32_t *)malloc(2 * sizeof *ids);
    ids[0] = 1;
    ids[1] = 2;
    ret->ptr = ids;
    ret->len_bytes = 2 * sizeof *ids;
    return ret;
}

EXPORT SDFVec3 *normal(uint32_t sdf_id, SDFVec3 p, float eps) {
    (void)sdf_id, (void)p, (void)eps;
    SDFVec3 *ret = (SDFVec3 *)calloc(1, sizeof *ret);
    ret->x = 0.25f;
    ret->y = 0.5f;
    ret->z = 1.0f;
    return ret;
}

EXPORT uint32_t sample_concurrency(void) { return 7; }
