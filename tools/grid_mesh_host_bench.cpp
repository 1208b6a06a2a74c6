// grid_mesh_host_bench.cpp -- tools/grid_mesh_bench.py --host builds and runs this: for a provider library (host-only SDF), the
// two ways to the mesh of the SAME lattice, cells^3 cells over the provider's box, alternated for `rounds` rounds in one process:
//   resample   mesh_any_sdf + postproc_any: sample the (cells + 1)^3 lattice on the host, mesh it, sample every vertex again;
//   viewer     SDFViewer::mesh (with materials, download included) on a (cells + 1)^3 grid the viewer has loaded -- the load is
//              timed apart: a viewer pays it whether or not anything is meshed.
//   grid_mesh_host_bench <provider library> <cells> <rounds>      -> one JSON line
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "provider_sdf.hpp"
#include "sdf_viewer.hpp"

using namespace sdfviewer;
using Clock = std::chrono::steady_clock;

static double ms_since(Clock::time_point t0) { return std::chrono::duration<double, std::milli>(Clock::now() - t0).count(); }
static double median(std::vector<double> v) {
    std::sort(v.begin(), v.end());
    return v.size() % 2 ? v[v.size() / 2] : 0.5 * (v[v.size() / 2 - 1] + v[v.size() / 2]);
}

int main(int argc, char** argv) {
    if (argc != 4) return 2;
    const size_t cells = strtoul(argv[2], nullptr, 10);
    const int rounds = atoi(argv[3]);
    std::string err;
    auto sdf = ProviderSDF::load(argv[1], &err);
    if (!sdf) return std::fprintf(stderr, "%s\n", err.c_str()), 1;
    std::vector<double> resample, viewer, load;
    size_t v_resample = 0, v_viewer = 0;
    for (int r = 0; r < rounds + 1; ++r) {  // round 0 warms up (code objects, the scratch pool) and is dropped
        auto t0 = Clock::now();
        MesherConfig cfg;
        cfg.max_voxels_per_axis = cells;
        auto m = mesh_any_sdf(Meshers::MarchingCubes, *sdf, cfg, &err);
        if (!m || postproc_any(*m, *sdf) != 0) return std::fprintf(stderr, "resample: %s\n", err.c_str()), 1;
        const double a = ms_since(t0);
        v_resample = m->vertices.size();

        auto v = SDFViewer::new_voxels({cells + 1, cells + 1, cells + 1}, sdf->bounding_box(), 2);
        if (!v) return std::fprintf(stderr, "cannot create the viewer\n"), 1;
        t0 = Clock::now();
        while (v->update(*sdf, std::chrono::milliseconds(30)) != 0) v->commit();
        v->commit();
        if (*v->last_error() || hipStreamSynchronize((hipStream_t)v->stream) != hipSuccess) return std::fprintf(stderr, "load failed\n"), 1;
        const double l = ms_since(t0);
        t0 = Clock::now();
        Mesh g;
        if (!v->mesh(Meshers::MarchingCubes, true, &g, &err)) return std::fprintf(stderr, "viewer: %s\n", err.c_str()), 1;
        const double b = ms_since(t0);
        v_viewer = g.vertices.size();
        if (r == 0) continue;
        resample.push_back(a);
        viewer.push_back(b);
        load.push_back(l);
    }
    std::printf("{\"cells\": %zu, \"lattice_points\": %zu, \"rounds\": %d, \"sampling_threads\": %u, \"resample_then_mesh_ms\": %.3f, "
                "\"viewer_mesh_ms\": %.3f, \"viewer_load_ms_paid_anyway\": %.3f, \"resample_vertices\": %zu, \"viewer_vertices\": %zu}\n",
                cells, (cells + 1) * (cells + 1) * (cells + 1), rounds, sdf->sample_concurrency(), median(resample), median(viewer),
                median(load), v_resample, v_viewer);
    return 0;
}
