// program_editor.hpp -- an SDF program with parameters (include/sdfprogram.h, "program editor"): the reference's design loop --
// parameters(), set_parameter(), changed() (src/sdf/mod.rs:60-86) -- for a caller-defined CSG tree.
//
// Program handles do not change: every accepted edit makes a NEW sdfv_program through sdfv_program_create (the same validator),
// the "snapshot", and the ones it replaces stay alive until trim() or the destructor -- a kernel in flight keeps reading the
// snapshot it was launched with, and nothing here synchronises a stream.
#pragma once

#include <memory>
#include <string>
#include <vector>

#include "../../include/sdfprogram.h"
#include "program_sdf.hpp"

namespace sdfviewer {

class EditableProgramSDF final : public SDFSurface {
   public:
    // The instructions, the model's box and the parameters (their strings are copied).  Every parameter's value is written to
    // its targets before the first snapshot is made.  Throws std::invalid_argument with the message of what was refused.
    EditableProgramSDF(const sdfv_prog_op* ops, size_t n, const float bb[6], const sdfv_program_param* params, size_t n_params);
    ~EditableProgramSDF() override;
    EditableProgramSDF(const EditableProgramSDF&) = delete;
    EditableProgramSDF& operator=(const EditableProgramSDF&) = delete;

    // ---- SDFSurface over the CURRENT snapshot ----
    BoundingBox bounding_box() const override { return view_->bounding_box(); }
    SDFSample sample(Vec3 p, bool distance_only) const override { return view_->sample(p, distance_only); }
    void sample_batch(const Vec3* p, size_t n, bool distance_only, SDFSample* out) const override {
        view_->sample_batch(p, n, distance_only, out);
    }
    unsigned sample_concurrency() const override { return view_->sample_concurrency(); }
    std::string name() const override { return "Program"; }
    bool has_device_sampler() const override { return view_->has_device_sampler(); }
    void sample_batch_device(const float* points_dev, size_t n, sdfv_sample* out_dev, void* stream) const override {
        view_->sample_batch_device(points_dev, n, out_dev, stream);
    }
    const sdfv_program* device_program() const override { return snapshots_.back(); }
    bool takes_whole_passes() const override { return true; }

    // ---- parameters (src/sdf/mod.rs:60-86) ----
    std::vector<SDFParam> parameters() const override;
    // Float values only.  Refused -- and nothing changes -- for an unknown id, a value outside [min, max] or not finite, and a
    // value sdfv_program_create refuses (its message).  Otherwise the new snapshot is current and the parameter's box is
    // merged into the pending one.
    SetParameterResult set_parameter(uint32_t param_id, const SDFParamValue& value) override;
    // the pending box, once (SDFDemo::changed)
    std::optional<BoundingBox> changed() override;

    // the parameters as the C structs (strings owned by this object; valid until it is destroyed)
    const std::vector<sdfv_program_param>& params() const { return params_; }
    // Frees the snapshots that have been replaced.  The caller has synchronised every stream that may still run one.
    void trim();
    size_t snapshots() const { return snapshots_.size(); }

   private:
    void apply(const sdfv_program_param& p, float value, std::vector<sdfv_prog_op>& ops) const;
    void adopt(sdfv_program* snapshot);

    std::vector<sdfv_prog_op> ops_;  // the current snapshot's instructions
    float bb_[6];
    std::vector<sdfv_program_param> params_;
    std::vector<std::unique_ptr<std::string>> strings_;
    std::vector<sdfv_program*> snapshots_;  // back() is current
    std::unique_ptr<ProgramSDF> view_;      // over back()
    std::optional<BoundingBox> pending_;
};

}  // namespace sdfviewer

// the C handle (include/sdfprogram.h): the class and the message of the last refusal
struct sdfv_program_editor {
    std::unique_ptr<sdfviewer::EditableProgramSDF> sdf;
    std::string err;
};
