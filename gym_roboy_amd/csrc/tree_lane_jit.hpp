// tree_lane_jit.hpp - run-time build of the generated joint-tree kernels (tree_lane.hpp, tree_lane_split.hpp) for ONE robot: the
// source tree_lane_gen.hpp writes for a form (jit_source), compiled with hiprtc (loaded with dlopen: msj_jit.hpp).  One program per
// kernel (step / env step of the handle's integrator), built by the first call that needs it: ~10 s each.  Host code.
#pragma once
#include "msj_jit.hpp"
#include "tree_lane_gen.hpp"

namespace rblj {

struct Kernel {
    hipModule_t mod = nullptr;
    hipFunction_t fn = nullptr;
    int state = 0;            // 0 = not tried yet, 1 = ready, -1 = not available
    std::string why;
};

// one generated form of a handle's robot: its text and launch geometry, whether the library's ahead-of-time instances serve it,
// and otherwise its hiprtc-built kernels
struct TreeForm {
    bool ok = false;          // gen is valid (the generator supports the robot in this form)
    bool baked = false;       // gen is the text the ahead-of-time instances were compiled from
    rblg::FormText gen;
    Kernel step, env;
    Kernel &kernel(int kind) { return kind ? env : step; }
    const Kernel &kernel(int kind) const { return kind ? env : step; }
};

// builds the kernel of `kind` (0 = step, 1 = env step) of `form` (rblg::FORM_*) on `device`; more than 64 KiB of dynamic LDS
// (robots with many joints) is granted here
inline bool build(int device, int form, const rblg::FormText &g, int integ, int kind, Kernel &out) {
    if (hipSetDevice(device) != hipSuccess) { out.state = -1; out.why = "hipSetDevice failed"; return false; }
    const rblg::JitSource j = rblg::jit_source(form, g.text, g.lds, integ, kind);
    const char *names[1] = {j.kernel.c_str()};
    hipFunction_t *slots[1] = {&out.fn};
    out.state = rbj::compile_and_load(j.src, j.program.c_str(), names, 1, out.mod, slots, out.why) ? 1 : -1;
    if (out.state == 1 && g.lds > 64 * 1024 &&
        hipFuncSetAttribute(reinterpret_cast<const void *>(out.fn), hipFuncAttributeMaxDynamicSharedMemorySize, int(g.lds)) != hipSuccess) {
        out.state = -1; out.why = "LDS of the " + j.program + " kernel not granted";
    }
    return out.state == 1;
}

inline void unload(Kernel &k) {
    if (k.mod) (void)hipModuleUnload(k.mod);
    k = Kernel();
}
inline void unload(TreeForm &f) { unload(f.step); unload(f.env); }

}  // namespace rblj
