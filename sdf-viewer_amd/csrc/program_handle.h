// program_handle.h -- what an sdfv_program handle is, for the two files that look inside: api_program.hip (the handle, the
// entry points) and program_compile.hip (sdfv_program_compile and what a compiled handle adds).
#pragma once

#include <atomic>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "api_internal.h"
#include "program_kernels.h"

namespace sdfv {

// What sdfv_program_compile adds to a handle: one code object for one architecture, the modules it has been loaded as (one per
// device that used a compiled route) and the counter of specialised launches.
struct CompiledProgram {
    uint32_t routes = 0;
    std::string arch;    // "gfx950": the processor, without feature suffixes
    std::string source;  // the generated translation unit
    std::vector<char> code;
    double compile_seconds = 0.0;
    std::atomic<uint64_t> launches{0};
    struct Loaded {
        int device;
        hipModule_t module;
        hipFunction_t fn[kProgramKernels];
    };
    std::vector<Loaded*> loaded;  // under sdfv_program::mu; entries never move: launchers keep a pointer to fn
};

}  // namespace sdfv

// The handle: the validated instructions (host), one device copy per device that has used it, and the compiled part or nullptr.
struct sdfv_program {
    std::vector<sdfv_prog_op> ops;
    float bb[6];
    std::mutex mu;
    std::vector<std::pair<int, void*>> device_copies;  // (HIP device, n * 64 bytes)
    sdfv::CompiledProgram* compiled = nullptr;
};
