// program_editor.cpp -- EditableProgramSDF and the sdfv_program_editor_* calls (include/sdfprogram.h): see program_editor.hpp.
// The C functions go through the class, as ProgramSDF's do.
#include "program_editor.hpp"

#include <cmath>
#include <cstring>
#include <stdexcept>

namespace sdfviewer {

namespace {

BoundingBox box_of(const float b[6]) { return {Vec3{b[0], b[1], b[2]}, Vec3{b[3], b[4], b[5]}}; }

std::string check_param(const sdfv_program_param& p, size_t n_ops) {
    const std::string who = "parameter " + std::to_string(p.id);
    if (!p.name) return who + ": name is NULL";
    if (!std::isfinite(p.min) || !std::isfinite(p.max) || !std::isfinite(p.step) || p.max < p.min)
        return who + ": the range [" + std::to_string(p.min) + ", " + std::to_string(p.max) + "] step " + std::to_string(p.step) + " is not one";
    if (!(p.value >= p.min && p.value <= p.max)) return who + ": value " + std::to_string(p.value) + " is outside its range";
    if (p.n_targets == 0 || p.n_targets > SDFV_PARAM_MAX_TARGETS)
        return who + ": " + std::to_string(p.n_targets) + " targets, not 1 .. " + std::to_string(SDFV_PARAM_MAX_TARGETS);
    for (uint32_t t = 0; t < p.n_targets; ++t) {
        const sdfv_param_target& g = p.targets[t];
        if (g.op >= n_ops || g.operand >= 12)
            return who + ": target " + std::to_string(t) + " (op " + std::to_string(g.op) + ", operand " + std::to_string(g.operand) + ") is outside the program";
        if (g.kind > SDFV_PARAM_RECIPROCAL) return who + ": target " + std::to_string(t) + " has the unknown kind " + std::to_string(g.kind);
    }
    if (p.has_box)
        for (int i = 0; i < 3; ++i)
            if (!std::isfinite(p.box[i]) || !std::isfinite(p.box[3 + i]) || p.box[3 + i] < p.box[i]) return who + ": its box is not finite or inverted";
    return "";
}

}  // namespace

EditableProgramSDF::EditableProgramSDF(const sdfv_prog_op* ops, size_t n, const float bb[6], const sdfv_program_param* params,
                                       size_t n_params) {
    if (!ops || !bb || (n_params && !params)) throw std::invalid_argument("ops, bb or params is NULL");
    ops_.assign(ops, ops + n);
    memcpy(bb_, bb, sizeof(bb_));
    for (size_t i = 0; i < n_params; ++i) {
        const std::string why = check_param(params[i], n);
        if (!why.empty()) throw std::invalid_argument(why);
        for (size_t k = 0; k < i; ++k)
            if (params[k].id == params[i].id) throw std::invalid_argument("parameter id " + std::to_string(params[i].id) + " appears twice");
        sdfv_program_param p = params[i];
        strings_.push_back(std::make_unique<std::string>(p.name));
        p.name = strings_.back()->c_str();
        strings_.push_back(std::make_unique<std::string>(p.description ? p.description : ""));
        p.description = strings_.back()->c_str();
        params_.push_back(p);
        apply(p, p.value, ops_);
    }
    sdfv_program* first = nullptr;
    if (sdfv_program_create(ops_.data(), ops_.size(), bb_, &first) != SDFV_OK) throw std::invalid_argument(sdfv_last_error());
    try {
        adopt(first);
    } catch (...) {
        sdfv_program_free(first);
        throw;
    }
}

EditableProgramSDF::~EditableProgramSDF() {
    for (sdfv_program* p : snapshots_) sdfv_program_free(p);
}

void EditableProgramSDF::adopt(sdfv_program* snapshot) {
    auto view = std::make_unique<ProgramSDF>(snapshot);
    snapshots_.push_back(snapshot);
    view_ = std::move(view);
}

void EditableProgramSDF::apply(const sdfv_program_param& p, float value, std::vector<sdfv_prog_op>& ops) const {
    for (uint32_t t = 0; t < p.n_targets; ++t) {
        const sdfv_param_target& g = p.targets[t];
        ops[g.op].a[g.operand] = g.kind == SDFV_PARAM_NEGATED ? -value : (g.kind == SDFV_PARAM_RECIPROCAL ? 1.0f / value : value);
    }
}

std::vector<SDFParam> EditableProgramSDF::parameters() const {
    std::vector<SDFParam> out;
    for (const sdfv_program_param& p : params_) {
        SDFParam q;
        q.id = p.id;
        q.name = p.name;
        q.description = p.description;
        q.kind.tag = SDFParamKind::Tag::Float;
        q.kind.float_lo = p.min;
        q.kind.float_hi = p.max;
        q.kind.float_step = p.step;
        q.value = p.value;
        out.push_back(std::move(q));
    }
    return out;
}

SetParameterResult EditableProgramSDF::set_parameter(uint32_t param_id, const SDFParamValue& value) {
    const float* v = std::get_if<float>(&value);
    if (!v) return SetParameterResult::Err("parameter " + std::to_string(param_id) + ": a program's parameters are floats");
    for (sdfv_program_param& p : params_) {
        if (p.id != param_id) continue;
        if (!(*v >= p.min && *v <= p.max))  // (a NaN fails both)
            return SetParameterResult::Err("parameter " + std::to_string(param_id) + " (" + p.name + "): " + std::to_string(*v) +
                                           " is outside [" + std::to_string(p.min) + ", " + std::to_string(p.max) + "]");
        std::vector<sdfv_prog_op> edited = ops_;
        apply(p, *v, edited);
        sdfv_program* next = nullptr;
        if (sdfv_program_create(edited.data(), edited.size(), bb_, &next) != SDFV_OK) return SetParameterResult::Err(sdfv_last_error());
        try {
            adopt(next);
        } catch (...) {
            sdfv_program_free(next);
            throw;
        }
        ops_.swap(edited);
        p.value = *v;
        const BoundingBox reach = box_of(p.has_box ? p.box : bb_);
        pending_ = pending_ ? merge_bounding_boxes(*pending_, reach) : reach;
        return SetParameterResult::Ok();
    }
    return SetParameterResult::Err("unknown parameter id " + std::to_string(param_id));
}

std::optional<BoundingBox> EditableProgramSDF::changed() {
    std::optional<BoundingBox> out;
    out.swap(pending_);
    return out;
}

void EditableProgramSDF::trim() {
    for (size_t i = 0; i + 1 < snapshots_.size(); ++i) sdfv_program_free(snapshots_[i]);
    snapshots_.erase(snapshots_.begin(), snapshots_.end() - 1);
}

namespace editor_callbacks {

// ---- the callbacks of sdfv_program_editor_as_surface: `user` is the editor, every call goes through the class ----
template <class F>
int through_editor(void* user, F&& body) {
    try {
        body(*static_cast<sdfv_program_editor*>(user)->sdf);
        return 0;
    } catch (...) {
        return 1;
    }
}
void ecb_bounding_box(void* user, float out[6]) {
    through_editor(user, [&](EditableProgramSDF& sdf) {
        box_floats(sdf.bounding_box(), out);
    });
}
int ecb_sample_batch(void* user, const float* p, size_t n, int distance_only, sdfv_sample* out) {
    return through_editor(user, [&](EditableProgramSDF& sdf) {
        sdf.sample_batch(reinterpret_cast<const Vec3*>(p), n, distance_only != 0, reinterpret_cast<SDFSample*>(out));
    });
}
int ecb_sample(void* user, const float p[3], int distance_only, sdfv_sample* out) { return ecb_sample_batch(user, p, 1, distance_only, out); }
uint32_t ecb_sample_concurrency(void* user) {
    uint32_t n = 1;
    through_editor(user, [&](EditableProgramSDF& sdf) { n = sdf.sample_concurrency(); });
    return n;
}
int ecb_changed(void* user, float out[6]) {
    int some = 0;
    through_editor(user, [&](EditableProgramSDF& sdf) {
        some = box_floats(sdf.changed(), out) ? 1 : 0;
    });
    return some;
}
int ecb_sample_batch_device(void* user, const float* points_dev, size_t n, sdfv_sample* out_dev, void* stream) {
    return through_editor(user, [&](EditableProgramSDF& sdf) { sdf.sample_batch_device(points_dev, n, out_dev, stream); });
}

}  // namespace editor_callbacks
}  // namespace sdfviewer

using sdfviewer::EditableProgramSDF;

namespace {
thread_local std::string t_create_error;  // sdfv_program_editor_create has no handle to leave its message in

template <class F>
int guarded(sdfv_program_editor* e, F&& body) {
    if (!e || !e->sdf) return SDFV_ERR_INVALID_ARGUMENT;
    try {  // nothing crosses the C boundary
        e->err.clear();
        return body(*e->sdf);
    } catch (const std::exception& x) {
        e->err = x.what();
        return SDFV_ERR_INTERNAL;
    } catch (...) {
        e->err = "internal error";
        return SDFV_ERR_INTERNAL;
    }
}
}  // namespace

// (libsdfviewer_host.so is built with default visibility: exported there, hidden in the test and provider libraries)
extern "C" {

int sdfv_program_editor_create(const sdfv_prog_op* ops, size_t n, const float bb[6], const sdfv_program_param* params, size_t n_params,
                               sdfv_program_editor** out) {
    t_create_error.clear();
    if (!out) return t_create_error = "out is NULL", SDFV_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    try {
        auto e = std::make_unique<sdfv_program_editor>();
        e->sdf = std::make_unique<EditableProgramSDF>(ops, n, bb, params, n_params);
        *out = e.release();
        return SDFV_OK;
    } catch (const std::invalid_argument& x) {
        t_create_error = x.what();
        return SDFV_ERR_INVALID_ARGUMENT;
    } catch (...) {
        t_create_error = "internal error";
        return SDFV_ERR_INTERNAL;
    }
}

void sdfv_program_editor_free(sdfv_program_editor* e) { delete e; }

int sdfv_program_editor_parameters(const sdfv_program_editor* e, const sdfv_program_param** params, size_t* n) {
    if (!e || !e->sdf) return SDFV_ERR_INVALID_ARGUMENT;
    if (params) *params = e->sdf->params().data();
    if (n) *n = e->sdf->params().size();
    return SDFV_OK;
}

int sdfv_program_editor_set(sdfv_program_editor* e, uint32_t id, float value) {
    return guarded(e, [&](EditableProgramSDF& sdf) {
        const sdfviewer::SetParameterResult r = sdf.set_parameter(id, sdfviewer::SDFParamValue(value));
        if (r.ok) return (int)SDFV_OK;
        e->err = r.error;
        return (int)SDFV_ERR_INVALID_ARGUMENT;
    });
}

int sdfv_program_editor_changed(sdfv_program_editor* e, float out[6]) {
    if (!e || !e->sdf || !out) return 0;
    return sdfviewer::editor_callbacks::ecb_changed(e, out);
}

const sdfv_program* sdfv_program_editor_program(const sdfv_program_editor* e) { return e && e->sdf ? e->sdf->device_program() : nullptr; }

int sdfv_program_editor_trim(sdfv_program_editor* e) {
    return guarded(e, [&](EditableProgramSDF& sdf) {
        sdf.trim();
        return (int)SDFV_OK;
    });
}

const char* sdfv_program_editor_last_error(const sdfv_program_editor* e) { return e ? e->err.c_str() : t_create_error.c_str(); }

int sdfv_program_editor_as_surface(sdfv_program_editor* e, sdfv_surface* out) {
    if (!e || !e->sdf || !out) return SDFV_ERR_INVALID_ARGUMENT;
    sdfv_surface s = {};
    s.user = e;
    s.bounding_box = sdfviewer::editor_callbacks::ecb_bounding_box;
    s.sample = sdfviewer::editor_callbacks::ecb_sample;
    s.sample_batch = sdfviewer::editor_callbacks::ecb_sample_batch;
    s.sample_concurrency = sdfviewer::editor_callbacks::ecb_sample_concurrency;
    s.changed = sdfviewer::editor_callbacks::ecb_changed;
    s.sample_batch_device = e->sdf->has_device_sampler() ? sdfviewer::editor_callbacks::ecb_sample_batch_device : nullptr;
    *out = s;
    return SDFV_OK;
}

}  // extern "C"
