/* bare_provider.c -- TEST FIXTURE: a provider that exports only the two required functions of include/sdf_provider.h and
 * their frees, linked (--no-as-needed) against libdep_exports.so (tests/c/dep_exports.c), which exports init, name, normal,
 * children and sample_concurrency.  Loaded as a provider it must behave as one without those exports. */
#include <stdlib.h>

#include "sdf_provider.h"

#define EXPORT __attribute__((visibility("default")))

EXPORT SDFBoundingBox *bounding_box(uint32_t sdf_id) {
    SDFBoundingBox *ret = (SDFBoundingBox *)calloc(1, sizeof *ret);
    if (sdf_id == 0) {
        ret->min.x = ret->min.y = ret->min.z = -1.0f;
        ret->max.x = ret->max.y = ret->max.z = 1.0f;
    }
    return ret;
}
EXPORT void bounding_box_free(SDFBoundingBox *ret) { free(ret); }

EXPORT SDFSample *sample(uint32_t sdf_id, SDFVec3 p, bool distance_only) {
    (void)distance_only;
    SDFSample *ret = (SDFSample *)calloc(1, sizeof *ret);
    if (sdf_id == 0) ret->distance = p.x * p.x + p.y * p.y + p.z * p.z - 0.25f;
    return ret;
}
EXPORT void sample_free(SDFSample *ret) { free(ret); }
