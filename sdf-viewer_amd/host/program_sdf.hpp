// program_sdf.hpp -- an SDF program (include/sdfgrid.h, "SDF programs") as an SDFSurface: the host mirror of the device
// interpreter, as SDFDemo is the host mirror of the demo kernels.
#pragma once

#include "sdf_surface.hpp"

namespace sdfviewer {

class ProgramSDF final : public SDFSurface {
   public:
    // `program` stays the caller's and must outlive this object
    explicit ProgramSDF(const sdfv_program* program);

    BoundingBox bounding_box() const override;
    // evaluated on the host, by the interpreter source the kernels are built from (csrc/program_eval.h)
    SDFSample sample(Vec3 p, bool distance_only) const override;
    void sample_batch(const Vec3* p, size_t n, bool distance_only, SDFSample* out) const override;
    unsigned sample_concurrency() const override { return 0xffffu; }  // stateless: as many threads as the host has
    std::string name() const override { return "Program"; }
    // the device route: sdfv_program_sample_points on `stream`
    bool has_device_sampler() const override;
    void sample_batch_device(const float* points_dev, size_t n, sdfv_sample* out_dev, void* stream) const override;

    // The direct march on the host (include/sdfprogram.h, sdfv_program_raymarch_host): `checked` and `normal_h` as
    // sdfv_program_raymarch_check hands them out, outputs in HOST memory; csrc/program_march.h per pixel, rows dealt to
    // n_threads workers (<= 0: the CPUs this process may use).  srgb_round: SDFV_OPT_EXT_SRGB_QUANT.
    void raymarch(const sdfv_program_march_desc& checked, float normal_h, bool srgb_round, int n_threads) const;

    // The ray cast on the host (include/sdfprogram.h, sdfv_program_raycast_host): `checked` as sdfv_program_raycast_check hands it
    // out, rays and hits in HOST memory; csrc/program_cast.h per ray, runs of rays dealt to n_threads workers (<= 0: the CPUs this
    // process may use).  Every byte of every record is the device's.
    void cast(const sdfv_program_cast_desc& checked, int n_threads) const;

    // meshing on the device: sdfv_program_mesh_extract / sdfv_program_mesh_postproc through mesh_sdf() and Mesh::postproc()
    const sdfv_program* device_program() const override { return program_; }

    const sdfv_program* program() const { return program_; }

   private:
    const sdfv_program* program_;
    const sdfv_prog_op* ops_ = nullptr;
    size_t n_ops_ = 0;
    float bb_[6] = {0, 0, 0, 0, 0, 0};
};

}  // namespace sdfviewer
