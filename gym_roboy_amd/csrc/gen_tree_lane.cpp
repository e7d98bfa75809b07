// gen_tree_lane.cpp - C entry of the lane-kernel source generator (tree_lane_gen.hpp) for the tools and the CPU
// tests: writes the generated header of a robot to `path`.  tools/gen_tree_lane_baked.py runs it on the committed
// upper body (tree_lane_baked.hpp, compiled into the library ahead of time); tests/test_tree_lane_gen.py runs it
// on random robots and checks the text, compiled with g++, against the fp64 oracle.  Built with g++.
#include <cstdio>
#include <cstdlib>
#include <string>

#include "tree_lane_gen.hpp"

// lds_c: bit 0 - park the velocity-product accelerations in LDS; bit 1 - do NOT write structurally identical subtrees as pair values
extern "C" int rb_gen_tree_lane(const rb_robot_desc *d, int lds_c, const char *path, int *lds_slots, int *n_stmt,
                                unsigned long long *hash, int *flops, int *max_live) {
    rblg::Generated g;
    std::string err;
    const int rc = rblg::generate(d, (lds_c & 1) != 0, g, err, (lds_c & 2) == 0);
    if (rc) { std::fprintf(stderr, "rb_gen_tree_lane: %s\n", err.c_str()); return rc; }
    FILE *f = std::fopen(path, "w");
    if (!f) return RB_EINVAL;
    std::fputs(g.text.c_str(), f);
    // the hash of the text above: a handle whose robot generates the same text runs the instances compiled from this file
    std::fprintf(f, "#define RBL_TEXT_HASH 0x%llxull\n", (unsigned long long)g.hash);
    std::fclose(f);
    if (lds_slots) *lds_slots = g.lds_slots;
    if (n_stmt) *n_stmt = g.n_stmt;
    if (hash) *hash = g.hash;
    if (flops) *flops = g.flops;
    if (max_live) *max_live = g.max_live;
    return RB_OK;
}

// mates of the links and tendons (-1: none, -2: is some link's / tendon's mate), as generate() pairs them
extern "C" int rb_gen_tree_lane_mates(const rb_robot_desc *d, int *mate, int *tmate) {
    rblg::Robot rob;
    std::string err;
    if (int rc = rblg::build_robot(d, rob, err)) return rc;
    std::vector<int> m, tm;
    rblg::find_mates(rob, m, tm);
    for (int i = 0; i < rob.nq; ++i) mate[i] = m[i];
    for (int k = 0; k < rob.nt; ++k) tmate[k] = tm[k];
    return RB_OK;
}

// the split form (several waves per env group): writes the header, returns parts / slots / statement counts.
// max_helpers: helper waves at most (tendon helpers of the longest parts; 0: the three-wave form of round 3)
extern "C" int rb_gen_tree_lane_split_h(const rb_robot_desc *d, int max_parts, int max_helpers, const char *path, int *n_parts, int *part_lds,
                                        int *x_slots, int *max_stmt, int *n_stmt, int *part_of_joint, unsigned long long *hash,
                                        int *n_helpers, int *helper_stmt) {
    rblg::SplitGenerated g;
    std::string err;
    // max_helpers: low byte = helper waves at most; bits 8-15 = the helpers' share of their parts' tendons in percent (0: the default)
    // ... bit 16 = the backward pass in two sweeps (inertias before barrier T, bias forces behind it); bit 17 unused;
    // bit 18 = one part evaluates the trunk links' inertias for all
    const int share = (max_helpers >> 8) & 0xff;
    const bool two_sweeps = ((max_helpers >> 16) & 1) != 0;
    const bool share_trunk = ((max_helpers >> 18) & 1) != 0;
    const int rc = rblg::generate_split(d, max_parts, g, err, max_helpers & 0xff, share ? share : 45, two_sweeps, share_trunk);
    if (rc) { std::fprintf(stderr, "rb_gen_tree_lane_split: %s\n", err.c_str()); return rc; }
    FILE *f = std::fopen(path, "w");
    if (!f) return RB_EINVAL;
    std::fputs(g.text.c_str(), f);
    std::fprintf(f, "#define RBL_SPLIT_TEXT_HASH 0x%llxull\n", (unsigned long long)g.hash);
    std::fclose(f);
    if (n_parts) *n_parts = g.n_parts;
    if (part_lds) *part_lds = g.part_lds;
    if (x_slots) *x_slots = g.x_slots;
    if (max_stmt) *max_stmt = g.max_stmt;
    if (n_stmt) *n_stmt = g.n_stmt;
    if (part_of_joint) for (int i = 0; i < g.n_q; ++i) part_of_joint[i] = g.part_of_joint[i];
    if (hash) *hash = g.hash;
    if (n_helpers) *n_helpers = g.n_helpers;
    if (helper_stmt) *helper_stmt = g.helper_stmt;
    return RB_OK;
}
extern "C" int rb_gen_tree_lane_split(const rb_robot_desc *d, int max_parts, const char *path, int *n_parts, int *part_lds, int *x_slots,
                                      int *max_stmt, int *n_stmt, int *part_of_joint, unsigned long long *hash) {
    return rb_gen_tree_lane_split_h(d, max_parts, 0, path, n_parts, part_lds, x_slots, max_stmt, n_stmt, part_of_joint, hash, nullptr, nullptr);
}

// the library's split forms (tree_lane_gen.hpp; form 0: SPLIT_FORM, the five-wave form, 1: SPLIT2_FORM, the lean two-part form) as
// rb_gen_tree_lane_split_h takes them: max_parts and the max_helpers word
extern "C" int rb_gen_tree_lane_split_form(int form, int *max_parts, int *max_helpers) {
    if (form != 0 && form != 1) return RB_EINVAL;
    const rblg::SplitForm &f = form == 0 ? rblg::SPLIT_FORM : rblg::SPLIT2_FORM;
    *max_parts = f.max_parts;
    *max_helpers = f.max_helpers | f.helper_share << 8 | int(f.two_sweeps) << 16 | int(f.share_trunk) << 18;
    return RB_OK;
}

// what the library hands to hiprtc for the kernel of `kind` (0 = step, 1 = env step; integ: 0 = Euler, 1 = RK4) of generated form
// `form` (tree_lane_gen.hpp: FORM_LANE, FORM_SPLIT, FORM_SPLIT2) of a robot: writes the source to `path`, the program's name and the
// kernel's name expression to `program` / `kernel` (buffers of `cap` bytes)
extern "C" int rb_gen_tree_jit_source(const rb_robot_desc *d, int form, int integ, int kind, const char *path, char *program, char *kernel, int cap) {
    if (form < 0 || form >= rblg::N_FORMS) return RB_EINVAL;
    rblg::FormText g;
    std::string err;
    if (int rc = rblg::generate_form(d, form, g, err)) { std::fprintf(stderr, "rb_gen_tree_jit_source: %s\n", err.c_str()); return rc; }
    const rblg::JitSource j = rblg::jit_source(form, g.text, g.lds, integ, kind);
    if (int(j.program.size()) >= cap || int(j.kernel.size()) >= cap) return RB_EINVAL;
    FILE *f = std::fopen(path, "w");
    if (!f) return RB_EINVAL;
    std::fputs(j.src.c_str(), f);
    std::fclose(f);
    std::snprintf(program, size_t(cap), "%s", j.program.c_str());
    std::snprintf(kernel, size_t(cap), "%s", j.kernel.c_str());
    return RB_OK;
}
