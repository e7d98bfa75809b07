// env_host.hpp - the fused env layer and its options on the host.
// Part of roboy_sim.hip (included there once, at file scope, behind the dispatch table; not a stand-alone header): everything
// RoboyEnv.step's layer (rb_env_*) and its options - per-env parameters, tendon channels, io and the action ring, action rows,
// episode-end codes, critic rows, the goal pool with its curriculum and row counts, reward shaping, random pushes, the episode log, start poses - do outside a kernel.  Each option is ONE record in
// rb_sim (roboy_sim.hip), is switched by ONE entry point that opens with reconfigure(), and has ONE line in behind_step() /
// behind_reset() if it launches anything there.  The kernels are in env_*.hpp and roboy_sim.hip; which env-step kernel runs is the
// dispatch table's business, or extension_launch()'s where extension_serves().  DESIGN.md §6 has the table of options.

namespace {
// ---- shared by the entry points ----
// What an entry point that changes an option opens with, in this order: the handle; rb_env_configure done (NEEDS_ENV); the call's own
// argument tests (`valid`: refusals leave the handle as it was); the device; nothing of this handle in flight; and - DROP_GRAPHS - no
// cached graph either: a captured graph holds its kernels and their arguments by value.  Without DROP_GRAPHS the graphs are kept, on
// purpose: the site says why a replay may see the change.
#define RB_RC(...) do { const int rc_ = (__VA_ARGS__); if (rc_) return rc_; } while (0)      // a failed call's code is the caller's
enum : unsigned { NEEDS_ENV = 1u, DROP_GRAPHS = 2u, KEEP_GRAPHS = 0u };
template <typename Valid>
int reconfigure(rb_sim *s, unsigned how, Valid &&valid) {
    if (check(s)) return RB_EINVAL;
    if ((how & NEEDS_ENV) && !s->env_ready) return fail(RB_EINVAL, "rb_env_configure has not been called");
    RB_RC(valid());
    RB_HIP(hipSetDevice(s->device));
    RB_RC(drain(s));
    return (how & DROP_GRAPHS) ? drop_graphs(s) : RB_OK;
}
int reconfigure(rb_sim *s, unsigned how) { return reconfigure(s, how, []() -> int { return RB_OK; }); }

// device memory for `what` (the message's head): out of memory is RB_ENOMEM, anything else RB_EHIP; *p is null on failure
template <typename T>
int dev_alloc(T **p, size_t bytes, const char *what) {
    const hipError_t e = hipMalloc(p, bytes);
    if (e == hipSuccess) return RB_OK;
    *p = nullptr;
    return fail(e == hipErrorOutOfMemory ? RB_ENOMEM : RB_EHIP, std::string(what) + hipGetErrorString(e));
}
// grid of the grid-stride kernels over the envs: at most 1024 blocks of 256
unsigned stride_grid(long n) { const unsigned g = blocks_for(n, 256); return g > 1024u ? 1024u : g; }
// refusal of the entry points that have no parameter form
int params_refuse(rb_sim *s, const char *what) {
    return fail(RB_EUNSUPPORTED, std::string(what) + " has no per-env-parameter form: the handle has parameters enabled (rb_params_disable first)");
}
// rb_sample_goals(_dev) on a handle with a goal curriculum: without an env step there is no episode outcome to move a level
int curriculum_refuse_sample(rb_sim *) {
    return fail(RB_EUNSUPPORTED, "rb_sample_goals: the handle has a goal curriculum, whose levels move with the env layer's episode ends");
}

// ---- tendon channels in the observation (env_obs.hpp): the arguments of a launch while a mask is set ----
// dynamic LDS of an extended env-step launch: the rows of its workgroup's envs, where they fit beside the instance's own columns (0: per-lane stores)
size_t obs_stage_bytes(const rb_sim *s, int block = 256) {
    const size_t columns = (s->baked ? 0 : s->ntx ? 4 * block * NTX : 4 * block * NT8) * (s->par.on ? 2 : 1);
    const size_t rows = size_t(4) * block * s->obs_dim();
    return columns + rows <= 65536 ? rows : 0;
}
template <int NT>
rbo::ObsArgs<NT> obs_args(const rb_sim *s, bool staged = false) {
    rbo::ObsArgs<NT> oa;
    oa.mask = s->chan.mask; oa.obs_dim = s->obs_dim(); oa.staged = staged ? 1 : 0; oa.pad_ = 0;
    for (int c = 0; c < 4; ++c) oa.scale[c] = s->chan.scale[c];
    for (int k = 0; k < NT; ++k) oa.units[k] = s->ts_units.u[k];
    return oa;
}
// ---- action latency and sensor noise (env_io.hpp): the argument of a launch while rb_env_io_configure holds ----
// first: the launch's first env (the planes and the ring inside each slot are shifted by it)
rbio::IoArgs io_args(const rb_sim *s, long first) {
    rbio::IoArgs io;
    std::memset(&io, 0, sizeof(io));
    const OptIo &o = s->io;
    const rb_env_io_config cfg = o.on ? o.cfg : rb_env_io_config{};      // (no io configuration, K > 0: zeros and the ring)
    if (o.on) { io.delay = o.d_delay + first; io.delay_draws = o.d_draws + first; io.rows = o.d_rows + first; }
    io.hist = o.d_ring ? o.d_ring + first * s->n_t : nullptr;
    io.slot_stride = long(s->n) * s->n_t;
    io.slot_mask = o.slots ? o.slots - 1 : 0;
    io.delay_lo = cfg.delay_lo; io.delay_hi = cfg.delay_hi; io.resample = cfg.resample_on_reset ? 1 : 0;
    // row positions: q, qd, (goal: never), then the selected channels in row order, each sigma in the units the column reports (x scale)
    const int nq = s->n_q;
    for (int j = 0; j < nq; ++j) { io.colsig[j] = cfg.sigma_q; io.colsig[nq + j] = cfg.sigma_qd; }
    int col = 3 * nq;
    for (int ch = 0; ch < 4; ++ch)
        if (s->chan.mask >> ch & 1)
            for (int k = 0; k < s->n_t; ++k) io.colsig[col++] = cfg.sigma_tendon[ch] * s->chan.scale[ch];
    for (int c = 0; c < col; ++c)
        if (io.colsig[c] != 0.0f) io.noise_blocks |= 1u << (c >> 2);
    return io;
}
// the ring both options share: S slots, the smallest power of two above max(delay_hi, K - 1); none without a delay range and K = 0
int ring_slots_wanted(int delay_hi, int hist_rows) {
    if (delay_hi <= 0 && hist_rows <= 0) return 0;
    const int reach = delay_hi > hist_rows - 1 ? delay_hi : hist_rows - 1;
    int slots = 1;
    while (slots <= reach) slots *= 2;
    return slots;
}
// ... rebuilt (zeroed) for the handle as configured
int ring_rebuild(rb_sim *s) {
    OptIo &o = s->io;
    (void)hipFree(o.d_ring);
    o.d_ring = nullptr;
    o.slots = ring_slots_wanted(o.on ? o.cfg.delay_hi : 0, s->hist.rows);
    if (!o.slots) return RB_OK;
    const size_t bytes = sizeof(float) * size_t(o.slots) * size_t(s->n) * size_t(s->n_t);
    const hipError_t e = hipMalloc(&o.d_ring, bytes);
    if (e != hipSuccess) {                   // no ring: neither a delay range nor action rows (their kernels index it unasked)
        o.d_ring = nullptr; o.slots = 0; s->hist.rows = 0;
        if (o.on) o.cfg.delay_lo = o.cfg.delay_hi = 0;
        return fail(RB_EHIP, std::string("the action history ring: ") + hipGetErrorString(e));
    }
    RB_HIP(hipMemsetAsync(o.d_ring, 0, bytes, s->stream));
    return RB_OK;
}
// rb_env_reset_dev's observation rows on a handle with channels or action rows: the state the reset kernel has just written, every set-point 0
void obs_rows_launch(rb_sim *s, float *d_obs) {
    const dim3 grid(blocks_for(s->n, 256)), block(256);
    const float *par = s->par.on ? s->par.d_planes : nullptr;
    if (s->ntx)
        hipLaunchKernelGGL((rbo::msj_obs_rows<256, ConstX>), grid, block, 0, s->stream, s->cx, obs_args<NTX>(s), s->d_q, s->d_qd, s->d_goal, par, d_obs, s->n);
    else
        hipLaunchKernelGGL((rbo::msj_obs_rows<256, Const8>), grid, block, 0, s->stream, s->c8, obs_args<NT8>(s), s->d_q, s->d_qd, s->d_goal, par, d_obs, s->n);
}

// ---- what dispatch() launches where extension_serves() (roboy_dispatch.hpp): the kernels of env_params.hpp, env_obs.hpp, env_io.hpp ----
// The constants an instance is compiled for, chosen here and nowhere else: f(the constants object, BK as a type) with BK = the
// constants are MsjRobot's literals (msj_baked.hpp), the object then only fills the argument's place
template <typename F>
int with_consts(const rb_sim *s, F &&f) {
    if (s->ntx) return f(s->cx, std::false_type{});
    if (s->baked) return f(s->c8, std::true_type{});
    return f(s->c8, std::false_type{});
}
rbp::ParamArgs param_args(const rb_sim *s, const Launch &L) {
    return rbp::ParamArgs{s->par.d_planes + L.i0, s->par.d_draws + L.i0, s->par.d_ranges, s->n, s->par.n, s->par.resample ? 1 : 0};
}
// the plain step under parameters: three argument lists of their own
template <int INTEG>
int params_step_launch(rb_sim *s, const Launch &L) {
    constexpr int B = 256;
    const dim3 grid(blocks_for(L.cnt, B)), block(B);
    float *q = s->d_q + L.i0, *qd = s->d_qd + L.i0, *par = s->par.d_planes + L.i0;
    uint32_t *feas = s->d_feas + L.i0;
    const float *act = L.act + size_t(L.i0) * s->n_t;
    return with_consts(s, [&](const auto &c, auto bk) {
        if constexpr (std::is_same<std::decay_t<decltype(c)>, ConstX>::value)
            hipLaunchKernelGGL((rbp::msj_params_step_nt<INTEG, B>), grid, block, 0, L.stream, c, q, qd, feas, act, L.act_scale, par, s->n, L.cnt);
        else
            hipLaunchKernelGGL((rbp::msj_params_step<INTEG, B, decltype(bk)::value>), grid, block, 0, L.stream, c, q, qd, feas, act, scale8(s, L.act_scale), par, s->n, L.cnt);
        return RB_OK;
    });
}
// The env step of a handle with any combination of parameters, channels and io: the env-step body with the extension of the last
// header that applies (io over channels over none), in its parameter form where parameters are enabled.
template <int INTEG>
int ext_env_launch(rb_sim *s, const Launch &L) {
    MsjEnvArgs a = msj_env_args(s, L);
    a.obs = L.obs + L.i0 * s->obs_dim();                 // the row stride is the handle's obs_dim (9 without channels)
    const int K = s->hist.rows;                           // > 0: the history kernels (env_hist.hpp), an io argument of zeros without io
    const bool par = s->par.on, io = s->io.on || K > 0, rows = io || s->chan.mask;       // rows: TendonObs writes them (env_obs.hpp)
    return with_consts(s, [&](const auto &c, auto bk) {
        using CONST = std::decay_t<decltype(c)>;
        constexpr bool BK = decltype(bk)::value;
        constexpr int NT = rbo::NtOf<CONST>::N;
        // the unroll factors of the large-batch env-per-lane rows (0: run-time tendon count)
        constexpr int U = NT == NTX ? 0 : BK ? (INTEG == 0 ? UBE : UBR) : (INTEG == 0 ? UKE : UKR);
        // An io kernel is the text of the kernel it stands in for.  Without parameters and channels that is the table's env-per-lane
        // row, which for MsjRobot's baked constants at small batches is the 64-thread instance with tendons AND integrator stages written
        // out - another summation order of the RK4 stages than the large-batch text (rolled stages): a configuration of zeros steps like
        // no configuration there too.  (Kernarg constants: the large-batch text's rolled tendon loop adds the same terms in the same order
        // as the written-out 64-thread row, and that row has no scalar register to spare - with the io arguments it would spill.)
        const bool small = BK && io && !par && !s->chan.mask && s->n <= RB_SMALL_BATCH;
        const int B = small ? 64 : 256;
        const size_t lds = rows ? obs_stage_bytes(s, B) : 0;
        const rbo::ObsArgs<NT> oa = obs_args<NT>(s, lds != 0);
        auto go = [&](auto kernel, const auto &...behind) {      // every instance takes (constants, MsjEnvArgs, ...)
            hipLaunchKernelGGL(kernel, dim3(blocks_for(L.cnt, B)), dim3(B), lds, L.stream, c, a, behind...);
            return RB_OK;
        };
        auto io_step = [&](auto block, auto unroll) {
            return go(rbio::msj_io_env_step<INTEG, decltype(block)::value, decltype(unroll)::value, CONST, BK>, oa, io_args(s, L.i0));
        };
        if (K > 0) {
            const rbh::HistIoArgs hio{io_args(s, L.i0), {K, s->obs_dim() - K * s->n_t}};
            if (par) return go(rbh::msj_hist_params_env_step<INTEG, 256, CONST, BK>, param_args(s, L), oa, hio);
            if constexpr (BK) if (small) return go(rbh::msj_hist_env_step<INTEG, 64, 8, CONST, BK>, oa, hio);
            return go(rbh::msj_hist_env_step<INTEG, 256, U, CONST, BK>, oa, hio);
        }
        if (par && io) return go(rbio::msj_io_params_env_step<INTEG, 256, CONST, BK>, param_args(s, L), oa, io_args(s, L.i0));
        if (io) {
            if constexpr (BK) if (small) return io_step(std::integral_constant<int, 64>{}, std::integral_constant<int, 8>{});
            return io_step(std::integral_constant<int, 256>{}, std::integral_constant<int, U>{});
        }
        if (par && rows) return go(rbo::msj_obs_params_env_step<INTEG, 256, CONST, BK>, param_args(s, L), oa);
        if (rows) return go(rbo::msj_obs_env_step<INTEG, 256, U, CONST, BK>, oa);
        return go(rbp::msj_params_env_step<INTEG, 256, CONST, BK>, param_args(s, L));
    });
}
int extension_launch(rb_sim *s, int entry, const Launch &L) {
    if (L.cnt <= 0) return RB_OK;
    const bool euler = s->integrator == RB_EULER;
    if (entry == ENTRY_STEP) return euler ? params_step_launch<0>(s, L) : params_step_launch<1>(s, L);
    if (entry == ENTRY_ENV) return euler ? ext_env_launch<0>(s, L) : ext_env_launch<1>(s, L);
    return fail(RB_EUNSUPPORTED, "per-env parameters have no fused-rollout kernel (rb_params_disable first)");
}

// ---- privileged critic rows (env_critic.hpp): one launch behind an env step or a reset, over the envs [i0, i0 + cnt) ----
// the options the mask was configured against are still there, and the row is as wide as the plane's
int critic_check(rb_sim *s) {
    const int m = s->critic.mask;
    if ((m & rbc::PARAMS && !s->par.on) || (m & rbc::DELAY && !s->io.on) || (m & rbc::ACTIONS && !s->hist.rows) || s->critic_width() != s->critic.dim)
        return fail(RB_EINVAL, "an option the critic rows depend on changed after rb_env_critic_obs_configure: configure the rows again");
    return RB_OK;
}
// d_obs: the observation rows the step has just written (null: no rows, zero action blocks); out: rows [n][Dc] of the whole batch
int critic_launch(rb_sim *s, long i0, long cnt, hipStream_t stream, const float *d_obs, float *out) {
    if (cnt <= 0) return RB_OK;
    rbc::CriticArgs a;
    a.q = s->d_q; a.qd = s->d_qd; a.goal = s->d_goal; a.step_num = s->d_step_num;
    a.par = s->par.on ? s->par.d_planes : nullptr;
    a.delay = s->io.on ? s->io.d_delay : nullptr;
    a.obs = d_obs; a.out = out;
    a.n = s->n; a.i0 = i0; a.i1 = i0 + cnt;
    a.max_len = float(s->env.max_len);
    a.nq = s->n_q; a.np = s->par.on ? s->par.n : 0; a.mask = s->critic.mask; a.dc = s->critic.dim;
    a.od = s->obs_dim(); a.act_cols = s->hist.rows * s->n_t; a.lead = a.od - a.act_cols;
    a.flat = reinterpret_cast<uintptr_t>(out) % 16 == 0 ? 1 : 0;
    hipLaunchKernelGGL(rbc::critic_rows_kernel, dim3(blocks_for(cnt, 256)), dim3(256), sizeof(float) * 256 * size_t(a.dc), stream, a);
    RB_HIP(hipGetLastError());
    return RB_OK;
}
// ---- goal pool (env_goal.hpp): one launch behind an env step (d_done: its done words) or a reset (null: every env), over [i0, i0 + cnt) ----
int goal_pool_launch(rb_sim *s, long i0, long cnt, hipStream_t stream, const uint32_t *d_done, float *d_obs) {
    const OptGoals &g = s->goals;
    rbg::GoalPoolArgs a;
    a.pool = g.d_pool; a.done = d_done; a.goal_count = s->d_goal_count; a.goal = s->d_goal; a.obs = d_obs;
    a.n = s->n; a.i0 = i0; a.i1 = i0 + cnt;
    a.seed = s->seed; a.env0 = uint64_t(s->env0);
    a.m = uint32_t(g.m);
    a.nq = s->n_q; a.od = s->obs_dim(); a.rows = s->tree ? 1 : 0;
    if (g.L) {                                // a curriculum: the same launch, the row drawn inside the env's window
        rbg::GoalCurriculumArgs c;
        c.p = a;
        c.level = g.d_level; c.index = g.d_index; c.seen = g.d_seen;
        c.reached = s->d_ep_cnt + 2 * size_t(s->n);
        c.L = g.L; c.up = g.up; c.down = g.down;
        if (g.d_row_stats) {                  // outcome counts per row: the same launch again, two adds per episode end more
            rbg::GoalCurriculumStatsArgs t;
            t.c = c; t.counts = reinterpret_cast<unsigned long long *>(g.d_row_stats);
            hipLaunchKernelGGL(rbg::goal_curriculum_stats_kernel, dim3(blocks_for(cnt, RBG_STATS_BLOCK)), dim3(RBG_STATS_BLOCK), 0, stream, t);
        } else
            hipLaunchKernelGGL(rbg::goal_curriculum_kernel, dim3(blocks_for(cnt, 256)), dim3(256), 0, stream, c);
    } else
        hipLaunchKernelGGL(rbg::goal_pool_kernel, dim3(blocks_for(cnt, 256)), dim3(256), 0, stream, a);
    RB_HIP(hipGetLastError());
    return RB_OK;
}

// ---- reward shaping (env_shaping.hpp): one launch in front of an env step and one behind it, over the envs [i0, i0 + cnt) ----
const char *const SHAPING_TENDON_TERMS = "the reward-shaping tendon terms (rb_env_shaping_configure: tension, activation)";
int shaping_refuse_delay() {
    return fail(RB_EUNSUPPORTED, std::string(SHAPING_TENDON_TERMS) + " need the row applied to be the row handed: the handle's action-delay range "
                                 "reaches above 0 (action_rate alone combines with a delay)");
}
// what holds between the option and the others, asked by whichever of two calls comes second (w: the weights asked for or configured)
int shaping_compatible(rb_sim *s, const rb_env_shaping_config &w, bool params, int delay_hi) {
    if (w.tension == 0.0f && w.activation == 0.0f) return RB_OK;
    if (params) return params_refuse(s, SHAPING_TENDON_TERMS);
    return delay_hi > 0 ? shaping_refuse_delay() : RB_OK;
}
// before anything of a step is enqueued: the options as they stand now, and the step's own refusals (a step that is refused
// behind the cost kernel would have moved the previous rows; behind the push kernel, velocities and counters).  step_form_check: what
// dispatch() would refuse - shared by every option that launches in front of the step
int step_form_check(rb_sim *s, long i0, long cnt) {
    if (extension_serves(s, ENTRY_ENV)) return RB_OK;
    std::string why;
    const Row *r = row_for(s, ENTRY_ENV, true, &why);
    if (!r) return fail(RB_EUNSUPPORTED, why);
    if (!r->ranges && !(i0 == 0 && cnt == s->n)) return fail(RB_EUNSUPPORTED, "this kernel form steps whole batches only (rb_range_capable)");
    return RB_OK;
}
int shaping_check(rb_sim *s, long i0, long cnt) {
    RB_RC(shaping_compatible(s, s->shaping.cfg, s->par.on, s->io.on ? s->io.cfg.delay_hi : 0));
    return step_form_check(s, i0, cnt);
}
size_t shaping_tree_lds(const rb_sim *s, int waves) {
    return rbt::tree_lds_bytes(s->tree_host, waves) + sizeof(float) * size_t(waves) * 3 * rbt::TREE_E * size_t(s->n_t);
}
int shaping_cost_launch(rb_sim *s, long i0, long cnt, hipStream_t stream, const float *d_act) {
    if (cnt <= 0) return RB_OK;
    const OptShaping &o = s->shaping;
    rbs::CostArgs a;
    a.q = s->d_q; a.qd = s->d_qd; a.act = d_act; a.step_num = s->d_step_num; a.prev = o.d_prev; a.cost = o.d_cost;
    a.w_rate = o.cfg.action_rate; a.w_tension = o.cfg.tension; a.w_act = o.cfg.activation;
    a.slope = s->env.slope; a.act_hi = s->env.act_hi;
    a.n = s->n; a.i0 = i0; a.i1 = i0 + cnt;
    constexpr int BLOCK = 256;
    if (s->tree) {
        const int wv = o.tree_waves;
        const long per_block = long(wv) * rbt::TREE_E;
        const dim3 grid(unsigned((cnt + per_block - 1) / per_block)), block(64 * wv);
        if (s->tree_host.dev.single_pass)
            hipLaunchKernelGGL((rbt::tree_shaping_cost<rbt::TREE_E, true>), grid, block, shaping_tree_lds(s, wv), stream, s->tree_host.dev, s->d_ts_lconst, a);
        else
            hipLaunchKernelGGL((rbt::tree_shaping_cost<rbt::TREE_E, false>), grid, block, shaping_tree_lds(s, wv), stream, s->tree_host.dev, s->d_ts_lconst, a);
    } else if (s->ntx) {
        hipLaunchKernelGGL(rbs::msj_shaping_cost_nt<BLOCK>, dim3(blocks_for(cnt, BLOCK)), dim3(BLOCK), 0, stream, s->cx, s->ts_units, a);
    } else {
        rbts::Units<NT8> u8;
        for (int k = 0; k < NT8; ++k) u8.u[k] = s->ts_units.u[k];
        hipLaunchKernelGGL(rbs::msj_shaping_cost8<BLOCK>, dim3(blocks_for(cnt, BLOCK)), dim3(BLOCK), 0, stream, s->c8, u8, a);
    }
    RB_HIP(hipGetLastError());
    return RB_OK;
}
// ---- random pushes (env_push.hpp): one launch in front of an env step (and of its shaping cost), over the envs [i0, i0 + cnt) ----
int push_launch(rb_sim *s, long i0, long cnt, hipStream_t stream) {
    if (cnt <= 0) return RB_OK;
    const OptPush &o = s->push;
    rbpush::PushArgs a;
    std::memset(&a, 0, sizeof(a));
    a.qd = s->d_qd; a.count = o.d_count; a.last = o.d_last; a.n_pushes = o.d_n; a.impulse = o.d_impulse;
    a.n = s->n; a.i0 = i0; a.i1 = i0 + cnt;
    a.seed = s->seed; a.env0 = uint64_t(s->env0);
    a.threshold = o.cfg.threshold; a.nq = s->n_q; a.rows = s->tree ? 1 : 0;
    for (int j = 0; j < s->n_q; ++j) { a.sigma[j] = o.cfg.sigma[j]; a.qd_max[j] = s->qd_max[j]; }
    hipLaunchKernelGGL(rbpush::env_push, dim3(blocks_for(cnt, 256)), dim3(256), 0, stream, a);
    RB_HIP(hipGetLastError());
    return RB_OK;
}
int push_clear(rb_sim *s) {
    const OptPush &o = s->push;
    const size_t plane = sizeof(uint32_t) * size_t(s->n);
    RB_HIP(hipMemsetAsync(o.d_count, 0, plane, s->stream));
    RB_HIP(hipMemsetAsync(o.d_last, 0, plane, s->stream));
    RB_HIP(hipMemsetAsync(o.d_n, 0, plane, s->stream));
    RB_HIP(hipMemsetAsync(o.d_impulse, 0, sizeof(float) * size_t(s->n) * size_t(s->n_q), s->stream));
    return RB_OK;
}
int shaping_apply_launch(rb_sim *s, long i0, long cnt, hipStream_t stream, float *d_reward, const uint32_t *d_done) {
    if (cnt <= 0) return RB_OK;
    const OptShaping &o = s->shaping;
    const rbs::ApplyArgs a{d_reward, o.d_cost, d_done, o.d_run, o.d_sums, o.d_cnt, s->n, i0, i0 + cnt};
    hipLaunchKernelGGL(rbs::shaping_apply, dim3(blocks_for(cnt, 256)), dim3(256), 0, stream, a);
    RB_HIP(hipGetLastError());
    return RB_OK;
}
// the sums and counts to zero (rb_env_configure, rb_env_shaping_stats with reset); the running episode costs and the cost plane to
// zero (a reset: the episodes it abandons are not counted)
int shaping_clear_sums(rb_sim *s) {
    RB_HIP(hipMemsetAsync(s->shaping.d_sums, 0, sizeof(double) * 2 * size_t(s->n), s->stream));
    RB_HIP(hipMemsetAsync(s->shaping.d_cnt, 0, sizeof(uint32_t) * 2 * size_t(s->n), s->stream));
    return RB_OK;
}
int shaping_restart(rb_sim *s) {
    RB_HIP(hipMemsetAsync(s->shaping.d_run, 0, sizeof(double) * size_t(s->n), s->stream));
    RB_HIP(hipMemsetAsync(s->shaping.d_cost, 0, sizeof(float) * size_t(s->n), s->stream));
    return RB_OK;
}
// ---- episode log (env_episode_log.hpp): one launch behind an env step, over the envs [i0, i0 + cnt) ----
int episode_log_launch(rb_sim *s, long i0, long cnt, hipStream_t stream, const float *d_reward, const uint32_t *d_done) {
    if (cnt <= 0) return RB_OK;
    const OptEpisodeLog &o = s->elog;
    rbel::LogArgs a;
    a.reward = d_reward; a.done = d_done; a.reached = s->d_ep_cnt + 2 * size_t(s->n);
    a.acc = o.d_acc; a.age = o.d_age; a.seen = o.d_seen; a.count = o.d_count;
    a.ret = o.d_ret; a.len = o.d_len; a.kind = o.d_kind; a.full = o.d_full;
    a.n = s->n; a.i0 = i0; a.i1 = i0 + cnt;
    a.E = uint32_t(o.E); a.pad_ = 0;
    hipLaunchKernelGGL(rbel::episode_log_kernel, dim3(blocks_for(cnt, 256)), dim3(256), 0, stream, a);
    RB_HIP(hipGetLastError());
    return RB_OK;
}
// the running episodes to zero (a reset: the episode it abandons is not recorded; records and counts stay)
int episode_log_restart(rb_sim *s) {
    RB_HIP(hipMemsetAsync(s->elog.d_acc, 0, sizeof(float) * size_t(s->n), s->stream));
    RB_HIP(hipMemsetAsync(s->elog.d_age, 0, sizeof(uint32_t) * size_t(s->n), s->stream));
    return RB_OK;
}
// `seen` follows the goals-reached counters as they stand: the next episode end is judged against them
int episode_log_rebase(rb_sim *s) {
    RB_HIP(hipMemcpyAsync(s->elog.d_seen, s->d_ep_cnt + 2 * size_t(s->n), sizeof(uint32_t) * size_t(s->n), hipMemcpyDeviceToDevice, s->stream));
    return RB_OK;
}
// no records, no episode under way (rb_env_episode_log_configure, rb_env_episode_log_clear); the record planes keep their content,
// which nothing reads at or beyond count
int episode_log_clear(rb_sim *s) {
    RB_HIP(hipMemsetAsync(s->elog.d_count, 0, sizeof(uint32_t) * size_t(s->n), s->stream));
    RB_HIP(hipMemsetAsync(s->elog.d_full, 0, sizeof(uint32_t), s->stream));
    RB_RC(episode_log_restart(s));
    return episode_log_rebase(s);
}

// ---- start poses (env_start.hpp): one launch behind an env step (d_done: its done words) or the reset kernel (null: every env), over [i0, i0 + cnt) ----
const char *const START_POSES_TENDON_OBS =
    "start poses and tendon channels in the observation do not combine: a started env's tendon columns would have to be evaluated at "
    "the new pose under the held command, and no readout does that yet";
int start_launch(rb_sim *s, long i0, long cnt, hipStream_t stream, const uint32_t *d_done, float *d_obs) {
    if (cnt <= 0) return RB_OK;
    const OptStart &o = s->start;
    rbstart::StartArgs a;
    std::memset(&a, 0, sizeof(a));
    a.pool = o.d_pool; a.done = d_done; a.q = s->d_q; a.qd = s->d_qd; a.feas = s->d_feas; a.count = o.d_count; a.index = o.d_index; a.obs = d_obs;
    a.n = s->n; a.i0 = i0; a.i1 = i0 + cnt;
    a.seed = s->seed; a.env0 = uint64_t(s->env0);
    a.m = uint32_t(o.m); a.threshold = o.threshold;
    a.nq = s->n_q; a.od = s->obs_dim(); a.rows = s->tree ? 1 : 0;
    if (d_done && s->io.on) {                 // behind a step: the noise of the row the step has just written, on the columns replaced
        const rbio::IoArgs io = io_args(s, 0);
        a.noise_rows = io.noise_blocks ? s->io.d_rows : nullptr;
        for (int c = 0; c < 2 * s->n_q; ++c) {
            a.colsig[c] = io.colsig[c];
            if (io.colsig[c] != 0.0f) a.noise_blocks |= 1u << (c >> 2);
        }
    }
    hipLaunchKernelGGL(rbstart::env_start, dim3(blocks_for(cnt, 256)), dim3(256), 0, stream, a);
    RB_HIP(hipGetLastError());
    return RB_OK;
}
// no start counted, every running episode began at the rest pose (rb_env_start_poses_configure)
int start_clear(rb_sim *s) {
    const size_t plane = sizeof(uint32_t) * size_t(s->n);
    RB_HIP(hipMemsetAsync(s->start.d_count, 0, plane, s->stream));
    RB_HIP(hipMemsetAsync(s->start.d_index, 0xFF, plane, s->stream));      // RB_START_INDEX_REST, every byte 0xFF
    return RB_OK;
}
// the rows of a pool [m][n_q]: finite and inside the robot's joint limits
int start_rows_check(const rb_sim *s, const float *rows, int64_t m) {
    for (int64_t r = 0; r < m; ++r)
        for (int j = 0; j < s->n_q; ++j) {
            const float v = rows[r * s->n_q + j];
            if (!std::isfinite(v) || v < s->box.lo[j] || v > s->box.hi[j])
                return fail(RB_EINVAL, "start poses: row " + std::to_string(r) + ", joint " + std::to_string(j) + " is not finite or outside the joint limits");
        }
    return RB_OK;
}

// ---- the episode counters and the planes that mirror them ----
// d_ep_sum, d_ep_cnt (episodes, lengths, goals reached), d_infeas_n and env_steps count since the last clear; d_done_seen (episode-end
// codes) and d_goal_seen (curriculum) hold each env's goals-reached counter as of its last episode end, so they follow it.  A new
// plane that mirrors a counter is added HERE.  Everything is enqueued on the handle's stream.
//   COUNTERS_CONFIGURE (rb_env_configure) and COUNTERS_CLEAR (rb_env_stats*(reset)): counters and mirrors to zero; the latter on a
//     handle without the env layer has only d_infeas_n and env_steps to clear.  The shaping sums are cleared by the former only:
//     rb_env_stats(reset) leaves them to rb_env_shaping_stats(reset)
//   COUNTERS_REBASE (rb_env_reset_dev): a reset is no episode end - the counters stand, d_done_seen is set to them and no code is
//     reported; d_goal_seen is re-based by the curriculum's own kernel, which behind_reset launches; the episode log's `seen` is set to
//     them too.  The log's plane is zeroed with the others where the counters are: a clear in the middle of a run would otherwise
//     mislabel the next outcome of every env
enum CounterSite { COUNTERS_CONFIGURE, COUNTERS_CLEAR, COUNTERS_REBASE };
int done_rebase(rb_sim *s) {
    const size_t plane = sizeof(uint32_t) * size_t(s->n);
    RB_HIP(hipMemcpyAsync(s->done.d_seen, s->d_ep_cnt + 2 * size_t(s->n), plane, hipMemcpyDeviceToDevice, s->stream));
    RB_HIP(hipMemsetAsync(s->done.d_kind, 0, plane, s->stream));
    return RB_OK;
}
int episode_counters(rb_sim *s, CounterSite site) {
    if (site == COUNTERS_REBASE) {
        if (s->elog.E) RB_RC(episode_log_rebase(s));
        return s->done.on ? done_rebase(s) : RB_OK;
    }
    const size_t n = size_t(s->n);
    if (site == COUNTERS_CONFIGURE || s->env_ready) {
        RB_HIP(hipMemsetAsync(s->d_ep_sum, 0, sizeof(double) * n * 2, s->stream));
        RB_HIP(hipMemsetAsync(s->d_ep_cnt, 0, sizeof(uint32_t) * n * 3, s->stream));
        if (s->done.on) RB_HIP(hipMemsetAsync(s->done.d_seen, 0, sizeof(uint32_t) * n, s->stream));
        if (s->goals.L) RB_HIP(hipMemsetAsync(s->goals.d_seen, 0, sizeof(uint32_t) * n, s->stream));
        if (s->elog.E) RB_HIP(hipMemsetAsync(s->elog.d_seen, 0, sizeof(uint32_t) * n, s->stream));
    }
    RB_HIP(hipMemsetAsync(s->d_infeas_n, 0, sizeof(uint32_t) * n, s->stream));
    s->env_steps = 0.0;
    if (site == COUNTERS_CONFIGURE && s->shaping.on) RB_RC(shaping_clear_sums(s));
    return RB_OK;
}

// ---- what runs behind an env step and behind a reset ----
// ONE stream each, so every kernel sees what those in front of it wrote.  The order, and why:
//   step:   the random push - IN FRONT of everything (env_step_launch): it makes the state s_t the step really starts from
//           the shaping cost of (s_t, a_t) - IN FRONT of the env-step kernel (env_step_launch), which overwrites the state it reads
//           the env-step kernel (dispatch)
//           0. shaping apply - reward -= cost, the cost statistics; reads the done words as flags, like 1.
//           1. goal pool / curriculum / row counts - the done envs' new goal becomes a pool row, IN FRONT of everything that reads the goal
//           1a. start poses (auto_reset only) - the done envs' zero pose becomes a pool row or stays, in the planes and in the row's
//               q / qd columns (with the noise the step put on them), IN FRONT of the critic rows, which report the true start pose.
//               Nothing of the option runs in front of the step: a refused step (step_form_check, dispatch) has enqueued nothing of it
//           2. critic rows - from the planes as 1. left them
//           3. episode log - the reward as 0. left it (what the caller receives); in front of 4. by convention only: log and codes
//              both test the done word against 0 and keep a `seen` plane of their own, so either order records the same
//           4. episode-end codes - last: it turns the range's done words, which 0., 1. and 3. read as flags, into codes
//   reset:  the reset kernel
//           0. start poses - every env's zero pose becomes a pool row or stays, IN FRONT of everything below: the row kernels, the
//              noise and the critic rows all work from the planes and rows as it left them
//           1. observation rows (channels, action rows) - the tendon columns at the zero pose, every set-point 0
//           2. the done-seen re-base (episode_counters)
//           3. sensor noise on the rows of 1., in place (the episode restarts, the history needs nothing)
//           4. zero action blocks - nothing has been handed yet
//           5. goal pool / curriculum - every env's goal becomes the pool row of the draw the reset kernel made, in the rows too
//           6. critic rows - behind every kernel that wrote the rows above
//           7. shaping - the running episode costs and the cost plane to zero (step_num is 1: the rate term restarts by itself)
//           8. episode log - the running return and age to zero: the abandoned episode is not recorded, records and counts stay
// A new option that launches behind either adds its line here.
int behind_step(rb_sim *s, long i0, long cnt, hipStream_t stream, float *d_obs, float *d_reward, uint32_t *d_done, float *d_cobs) {
    if (s->shaping.on) RB_RC(shaping_apply_launch(s, i0, cnt, stream, d_reward, d_done));
    if (s->goals.d_pool) RB_RC(goal_pool_launch(s, i0, cnt, stream, d_done, d_obs));
    if (s->start.d_pool && s->env.auto_reset) RB_RC(start_launch(s, i0, cnt, stream, d_done, d_obs));
    if (s->critic.mask) RB_RC(critic_launch(s, i0, cnt, stream, d_obs, d_cobs ? d_cobs : s->critic.d_rows));
    if (s->elog.E) RB_RC(episode_log_launch(s, i0, cnt, stream, d_reward, d_done));
    if (s->done.on) {
        hipLaunchKernelGGL(done_kind_kernel, dim3(blocks_for(cnt, 256)), dim3(256), 0, stream, d_done, s->d_ep_cnt + 2 * size_t(s->n),
                           s->done.d_seen, s->done.d_kind, i0, i0 + cnt);
        RB_HIP(hipGetLastError());
    }
    return RB_OK;
}
int behind_reset(rb_sim *s, float *d_obs) {
    const int od = s->obs_dim(), lead = od - s->hist.rows * s->n_t;      // (the noise stops in front of the action blocks: row stride and noised width apart)
    const dim3 grid(blocks_for(s->n, 256)), block(256);
    if (s->start.d_pool) RB_RC(start_launch(s, 0, s->n, s->stream, nullptr, d_obs));
    if ((s->chan.mask || s->hist.rows) && d_obs) {
        obs_rows_launch(s, d_obs);
        RB_HIP(hipGetLastError());
    }
    RB_RC(episode_counters(s, COUNTERS_REBASE));
    if (s->io.on && d_obs) {
        const rbio::IoArgs io = io_args(s, 0);
        if (io.noise_blocks) {
            if (s->hist.rows)
                hipLaunchKernelGGL(rbh::hist_noise_rows, grid, block, 0, s->stream, d_obs, od, lead, io, long(s->n), s->seed, uint64_t(s->env0));
            else
                hipLaunchKernelGGL(rbio::io_noise_rows, grid, block, 0, s->stream, d_obs, od, io, s->n, s->seed, uint64_t(s->env0));
            RB_HIP(hipGetLastError());
        }
    }
    if (s->hist.rows && d_obs) {
        hipLaunchKernelGGL(rbh::hist_zero_rows, grid, block, 0, s->stream, d_obs, od, lead, long(s->n));
        RB_HIP(hipGetLastError());
    }
    if (s->goals.d_pool) RB_RC(goal_pool_launch(s, 0, s->n, s->stream, nullptr, d_obs));
    if (s->critic.mask) {
        RB_RC(critic_check(s));
        RB_RC(critic_launch(s, 0, s->n, s->stream, d_obs, s->critic.d_rows));
    }
    if (s->shaping.on) RB_RC(shaping_restart(s));
    if (s->elog.E) RB_RC(episode_log_restart(s));
    return RB_OK;
}

// RoboyEnv.step for envs [i0, i0 + cnt) on `stream`; the array arguments are those of the whole batch (the launchers apply the
// offsets).  Sub-ranges: every ball-joint form and the joint trees' one-wave-per-64-envs form (Row::ranges).
// d_cobs: where the range's critic rows go while rb_env_critic_obs_configure holds (null: the handle's plane)
int env_step_launch(rb_sim *s, long i0, long cnt, hipStream_t stream, const float *d_act, float *d_obs, float *d_reward, uint32_t *d_done, float *d_cobs) {
    if (s->critic.mask) RB_RC(critic_check(s));          // (before anything is enqueued)
    if (s->shaping.on) RB_RC(shaping_check(s, i0, cnt));
    else if (s->push.on) RB_RC(step_form_check(s, i0, cnt));
    Launch L;
    L.i0 = i0; L.cnt = cnt; L.stream = stream; L.act = d_act; L.obs = d_obs; L.reward = d_reward; L.done = d_done;
    if (s->push.on) RB_RC(push_launch(s, i0, cnt, stream));
    if (s->shaping.on) RB_RC(shaping_cost_launch(s, i0, cnt, stream, d_act));
    RB_RC(dispatch(s, ENTRY_ENV, L));
    return behind_step(s, i0, cnt, stream, d_obs, d_reward, d_done, d_cobs);
}
// The one function behind the four rb_env_step*_dev exports.  range: envs [first, first + count) on hip_stream (null: the handle's) -
// the call's stream is visible to the build guards for its duration (a first call captured on the caller's stream defers the run-time
// builds: capturing()) and remembered for drain(); otherwise the whole batch on the handle's stream, which needs neither.
// critic: the entry points with a d_cobs argument - they need the rows enabled, and test the action slab's alignment for joint trees too.
int env_step_entry(rb_sim *s, bool range, int64_t first, int64_t count, void *hip_stream, const float *d_act, float *d_obs, float *d_reward,
                   uint32_t *d_done, bool critic, float *d_cobs) {
    if (check(s) || !d_act || !d_obs || !d_reward || !d_done || (critic && !d_cobs)) return fail(RB_EINVAL, "null argument");
    RB_HIP(hipSetDevice(s->device));
    if (!s->env_ready) return fail(RB_EINVAL, "rb_env_configure has not been called");
    if (critic && s->critic.need()) return RB_EINVAL;
    if ((critic || !s->tree) && reinterpret_cast<uintptr_t>(d_act) % 16) return fail(RB_EINVAL, "action slab must be 16-byte aligned");
    if (!range) {
        const int rc = env_step_launch(s, 0, s->n, s->stream, d_act, d_obs, d_reward, d_done, d_cobs);
        if (rc == RB_OK) s->env_steps += double(s->n);
        return rc;
    }
    if (range_ok(s, first, count)) return RB_EINVAL;
    hipStream_t st = hip_stream ? static_cast<hipStream_t>(hip_stream) : s->stream;
    CallStreamScope scope(s, st);
    int rc = env_step_launch(s, long(first), long(count), st, d_act, d_obs, d_reward, d_done, d_cobs);
    if (rc == RB_OK) { s->env_steps += double(count); rc = note_caller_stream(s, st); }
    return rc;
}

// ---- env statistics ----
int stats_launch(rb_sim *s, double *d_out2) {
    unsigned g = blocks_for(s->n, 256);
    if (g > unsigned(STATS_BLOCKS)) g = STATS_BLOCKS;
    double *partials = s->d_stats + 8;
    unsigned int *ticket = reinterpret_cast<unsigned int *>(s->d_stats + 8 * (STATS_BLOCKS + 1));
    // (ENV: the env layer's accumulators exist; without it only the infeasible envs are counted)
    hipLaunchKernelGGL(s->env_ready ? stats_reduce_kernel<true> : stats_reduce_kernel<false>, dim3(g), dim3(256), 0, s->stream,
                       s->env_ready ? s->d_ep_sum : nullptr, s->d_ep_cnt, s->d_ep_ret, s->d_infeas_n, s->d_feas, partials, ticket, s->d_stats, d_out2, s->env_steps, s->n);
    RB_HIP(hipGetLastError());
    return RB_OK;
}

}  // namespace

extern "C" {
// ---- the env layer itself ----
int rb_env_configure(rb_sim *s, const rb_env_config *cfg) {
    if (check(s) || !cfg) return fail(RB_EINVAL, "null argument");
    if (!s->tree && s->n_q != 3) return fail(RB_EUNSUPPORTED, "fused env layer: unsupported robot");
    if (cfg->max_episode_length < 1) return fail(RB_EINVAL, "max_episode_length must be >= 1");
    if (!(cfg->angle_hi > cfg->angle_lo) || !(cfg->vel_hi > cfg->vel_lo) || !(cfg->action_hi > cfg->action_lo))
        return fail(RB_EINVAL, "empty box in env config");
    RB_HIP(hipSetDevice(s->device));
    EnvParams &e = s->env;
    e.vel_penalty = cfg->joint_vel_penalty != 0; e.bonus = cfg->goal_bonus != 0;
    e.max_len = cfg->max_episode_length; e.auto_reset = cfg->auto_reset != 0;
    e.penalty = cfg->penalty_boundary; e.bonus_val = cfg->bonus_goal;
    e.a_lo = cfg->angle_lo; e.a_hi = cfg->angle_hi; e.v_lo = cfg->vel_lo; e.v_hi = cfg->vel_hi;
    e.act_hi = cfg->action_hi;
    // (out.high - out.low) / (in.high - in.low) evaluated in fp32 like the reference's float32 Boxes
    e.slope = (cfg->action_hi - cfg->action_lo) / (1.0f - (-1.0f));
    e.tol_a2 = cfg->goal_angle_tol * cfg->goal_angle_tol; e.tol_v2 = cfg->goal_vel_tol * cfg->goal_vel_tol;
    e.a_scale = 2.0f / (cfg->angle_hi - cfg->angle_lo); e.v_scale = 2.0f / (cfg->vel_hi - cfg->vel_lo);
    if (!s->d_goal) {
        const size_t plane = sizeof(float) * size_t(s->n);
        RB_HIP(hipMalloc(&s->d_goal, plane * s->n_q));
        RB_HIP(hipMalloc(&s->d_ep_ret, plane));
        RB_HIP(hipMalloc(&s->d_step_num, sizeof(uint32_t) * size_t(s->n)));
        RB_HIP(hipMalloc(&s->d_ep_sum, sizeof(double) * size_t(s->n) * 2));
        RB_HIP(hipMalloc(&s->d_ep_cnt, sizeof(uint32_t) * size_t(s->n) * 3));
    }
    RB_RC(episode_counters(s, COUNTERS_CONFIGURE));
    s->env_ready = true;
    // the run-time specialised kernels are built here, outside any capture a caller may wrap around its first step
    maybe_jit(s);
    if (s->tree) (void)resolve_form(s, ENTRY_ENV, /*build=*/true, nullptr);      // (the env step's kernel of the generated form it runs)
    return rb_env_reset_dev(s, nullptr);
}
int rb_env_reset_dev(rb_sim *s, float *d_obs) {
    if (check(s)) return RB_EINVAL;
    RB_HIP(hipSetDevice(s->device));
    if (!s->env_ready) return fail(RB_EINVAL, "rb_env_configure has not been called");
    if (s->tree)
        hipLaunchKernelGGL(rbt::tree_env_reset_kernel, dim3(blocks_for(s->n, 256)), dim3(256), 0, s->stream,
                           s->box, s->d_q, s->d_qd, s->d_feas, s->d_goal, s->d_step_num, s->d_ep_ret,
                           s->d_goal_count, d_obs, s->n_q, s->n, s->seed, uint64_t(s->env0));
    else                                      // (rows of obs_dim floats are behind_reset's: the kernel writes rows of 9)
        hipLaunchKernelGGL(env_reset_kernel, dim3(blocks_for(s->n, 256)), dim3(256), 0, s->stream,
                           s->box, s->d_q, s->d_qd, s->d_feas, s->d_goal, s->d_step_num, s->d_ep_ret,
                           s->d_goal_count, s->chan.mask || s->hist.rows ? nullptr : d_obs, s->n, s->seed, uint64_t(s->env0));
    RB_HIP(hipGetLastError());
    return behind_reset(s, d_obs);
}
int rb_env_obs_dim(rb_sim *s, int32_t *obs_dim) {
    if (check(s) || !obs_dim) return fail(RB_EINVAL, "null argument");
    *obs_dim = s->obs_dim();
    return RB_OK;
}
int rb_env_set_goal(rb_sim *s, const float *goal_q, const uint32_t *step_num) {
    if (check(s) || !goal_q) return fail(RB_EINVAL, "null argument");
    RB_HIP(hipSetDevice(s->device));
    if (!s->env_ready) return fail(RB_EINVAL, "rb_env_configure has not been called");
    const long n = s->n;
    RB_HIP(hipMemcpyAsync(s->d_rows, goal_q, sizeof(float) * n * s->n_q, hipMemcpyHostToDevice, s->stream));
    hipLaunchKernelGGL(unpack_rows_kernel, dim3(blocks_for(n, 256)), dim3(256), 0, s->stream, s->d_rows, s->d_goal, s->n_q, n, s->tree ? 1 : 0);
    RB_HIP(hipGetLastError());
    if (step_num)
        RB_HIP(hipMemcpyAsync(s->d_step_num, step_num, sizeof(uint32_t) * n, hipMemcpyHostToDevice, s->stream));
    if (s->goals.L)                           // these goals are no row of the pool: RB_GOAL_INDEX_NONE, every byte 0xFF
        RB_HIP(hipMemsetAsync(s->goals.d_index, 0xFF, sizeof(uint32_t) * n, s->stream));
    RB_HIP(hipStreamSynchronize(s->stream));
    return RB_OK;
}

int rb_env_step_dev(rb_sim *s, const float *d_act, float *d_obs, float *d_reward, uint32_t *d_done) {
    return env_step_entry(s, false, 0, 0, nullptr, d_act, d_obs, d_reward, d_done, false, nullptr);
}
int rb_env_step_critic_dev(rb_sim *s, const float *d_act, float *d_obs, float *d_reward, uint32_t *d_done, float *d_cobs) {
    return env_step_entry(s, false, 0, 0, nullptr, d_act, d_obs, d_reward, d_done, true, d_cobs);
}
int rb_env_step_range_dev(rb_sim *s, int64_t first_env, int64_t n_envs, void *hip_stream, const float *d_act, float *d_obs, float *d_reward, uint32_t *d_done) {
    return env_step_entry(s, true, first_env, n_envs, hip_stream, d_act, d_obs, d_reward, d_done, false, nullptr);
}
int rb_env_step_range_critic_dev(rb_sim *s, int64_t first_env, int64_t n_envs, void *hip_stream, const float *d_act, float *d_obs, float *d_reward,
                                 uint32_t *d_done, float *d_cobs) {
    return env_step_entry(s, true, first_env, n_envs, hip_stream, d_act, d_obs, d_reward, d_done, true, d_cobs);
}

int rb_env_stats_dev(rb_sim *s, double *d_stats8, int reset) {
    if (check(s) || !d_stats8) return fail(RB_EINVAL, "null argument");
    RB_HIP(hipSetDevice(s->device));
    RB_RC(stats_launch(s, d_stats8));
    return reset ? episode_counters(s, COUNTERS_CLEAR) : RB_OK;
}
int rb_env_stats(rb_sim *s, double *stats8, int reset) {
    if (check(s) || !stats8) return fail(RB_EINVAL, "null argument");
    RB_HIP(hipSetDevice(s->device));
    RB_RC(stats_launch(s, nullptr));
    RB_HIP(hipMemcpyAsync(stats8, s->d_stats, sizeof(double) * 8, hipMemcpyDeviceToHost, s->stream));
    RB_HIP(hipStreamSynchronize(s->stream));
    return reset ? episode_counters(s, COUNTERS_CLEAR) : RB_OK;
}

// ---- tendon channels in the fused env step's observation (env_obs.hpp) ----
int32_t rb_env_obs_count(int32_t n_q, int32_t n_t, uint32_t channel_mask) {
    if (n_q < 0 || n_t < 0 || (channel_mask & ~uint32_t(RB_OBS_ALL))) return -1;
    return 3 * n_q + rbo::n_channels(int(channel_mask)) * n_t;
}
int rb_env_obs_configure(rb_sim *s, uint32_t channel_mask, const float *scale) {
    // nothing in flight may still write rows of the old width
    RB_RC(reconfigure(s, NEEDS_ENV | DROP_GRAPHS, [&]() -> int {
        if (channel_mask & ~uint32_t(RB_OBS_ALL)) return fail(RB_EINVAL, "unknown bits in the channel mask (RB_OBS_LENGTH | RB_OBS_RATE | RB_OBS_ACTIVATION | RB_OBS_FORCE)");
        if (scale)
            for (int c = 0; c < 4; ++c)
                if (!std::isfinite(scale[c])) return fail(RB_EINVAL, "channel scales must be finite");
        if (s->tree && channel_mask)
            return fail(RB_EUNSUPPORTED, "tendon channels in the observation are built for ball-joint robots (1-16 tendons); a joint tree's readout is "
                                         "rb_tendon_state_dev");
        if (s->start.d_pool && channel_mask) return fail(RB_EUNSUPPORTED, START_POSES_TENDON_OBS);
        return RB_OK;
    }));
    s->chan.mask = int(channel_mask);
    for (int c = 0; c < 4; ++c) s->chan.scale[c] = scale ? scale[c] : 1.0f;
    return RB_OK;
}

// ---- per-env action latency and sensor noise in the fused env step (env_io.hpp) ----
int rb_env_io_configure(rb_sim *s, const rb_env_io_config *cfg) {
    // nothing in flight may still use the planes or the ring
    RB_RC(reconfigure(s, NEEDS_ENV | DROP_GRAPHS, [&]() -> int {
        if (!cfg) return RB_OK;
        const float sig[6] = {cfg->sigma_q, cfg->sigma_qd, cfg->sigma_tendon[0], cfg->sigma_tendon[1], cfg->sigma_tendon[2], cfg->sigma_tendon[3]};
        for (float v : sig)
            if (!std::isfinite(v) || v < 0.0f) return fail(RB_EINVAL, "sensor-noise standard deviations must be finite and >= 0");
        if (cfg->delay_lo < 0 || cfg->delay_lo > cfg->delay_hi || cfg->delay_hi > RB_IO_MAX_DELAY)
            return fail(RB_EINVAL, "action delay: 0 <= delay_lo <= delay_hi <= RB_IO_MAX_DELAY");
        if (s->tree)
            return fail(RB_EUNSUPPORTED, "action latency and sensor noise are built for ball-joint robots (1-16 tendons); joint trees have none");
        if (s->shaping.on) RB_RC(shaping_compatible(s, s->shaping.cfg, false, cfg->delay_hi));
        return RB_OK;
    }));
    s->io.release();
    if (!cfg) return ring_rebuild(s);        // (the ring stays for the action columns, rb_env_action_obs_configure)
    const size_t n = size_t(s->n);
    auto planes = [&]() -> int {
        RB_HIP(hipMalloc(&s->io.d_delay, sizeof(uint32_t) * n));
        RB_HIP(hipMalloc(&s->io.d_draws, sizeof(uint32_t) * n));
        RB_HIP(hipMalloc(&s->io.d_rows, sizeof(uint32_t) * n));
        RB_HIP(hipMemsetAsync(s->io.d_draws, 0, sizeof(uint32_t) * n, s->stream));
        RB_HIP(hipMemsetAsync(s->io.d_rows, 0, sizeof(uint32_t) * n, s->stream));
        return RB_OK;
    };
    const int rc = planes();
    if (rc) {                                // no io configuration; action rows keep a ring of their own (or are switched off with it)
        s->io.release();
        (void)ring_rebuild(s);               // (clears the action rows itself where it fails too)
        return rc;
    }
    s->io.cfg = *cfg;
    s->io.on = true;
    RB_RC(ring_rebuild(s));
    return rb_env_io_sample_delay_dev(s, nullptr);      // draw 0 of every env
}
int rb_env_io_ptr(rb_sim *s, uint32_t **d_delay, uint32_t **d_delay_draws, uint32_t **d_rows, float **d_history, int32_t *slots) {
    if (check(s)) return RB_EINVAL;
    if (!s->io.on && !s->hist.rows) return fail(RB_EINVAL, "no io configuration (rb_env_io_configure)");
    if (d_delay) *d_delay = s->io.d_delay;
    if (d_delay_draws) *d_delay_draws = s->io.d_draws;
    if (d_rows) *d_rows = s->io.d_rows;
    if (d_history) *d_history = s->io.d_ring;
    if (slots) *slots = s->io.slots;
    return RB_OK;
}
int rb_env_io_sample_delay_dev(rb_sim *s, const uint8_t *d_mask) {
    if (check(s)) return RB_EINVAL;
    if (!s->io.on) return fail(RB_EINVAL, "no io configuration (rb_env_io_configure)");
    RB_HIP(hipSetDevice(s->device));
    hipLaunchKernelGGL(rbio::io_sample_delay, dim3(blocks_for(s->n, 256)), dim3(256), 0, s->stream, s->io.d_delay, s->io.d_draws, d_mask,
                       s->io.cfg.delay_lo, s->io.cfg.delay_hi, long(s->n), s->seed, uint64_t(s->env0));
    RB_HIP(hipGetLastError());
    return RB_OK;
}

// ---- the last K commanded actions as observation columns (env_hist.hpp) ----
int32_t rb_env_action_obs_count(int32_t n_q, int32_t n_t, uint32_t channel_mask, int32_t rows) {
    if (rows < 0 || rows > RB_ACTION_OBS_MAX) return -1;
    const int32_t lead = rb_env_obs_count(n_q, n_t, channel_mask);
    return lead < 0 ? -1 : lead + rows * n_t;
}
int rb_env_action_obs_configure(rb_sim *s, int32_t rows) {
    // nothing in flight may still write rows of the old width or use the ring
    RB_RC(reconfigure(s, NEEDS_ENV | DROP_GRAPHS, [&]() -> int {
        if (rows < 0 || rows > RB_ACTION_OBS_MAX) return fail(RB_EINVAL, "action rows in the observation: 0 <= rows <= RB_ACTION_OBS_MAX");
        if (s->tree && rows)
            return fail(RB_EUNSUPPORTED, "action columns in the observation are built for ball-joint robots (1-16 tendons); joint trees have none");
        return RB_OK;
    }));
    const bool resize = ring_slots_wanted(s->io.on ? s->io.cfg.delay_hi : 0, rows) != s->io.slots;
    s->hist.rows = rows;
    if (!resize) return RB_OK;
    if (!s->io.on) return ring_rebuild(s);
    const rb_env_io_config cfg = s->io.cfg;  // another S: planes, counters and ring as a fresh io configuration leaves them
    return rb_env_io_configure(s, &cfg);
}
int rb_env_action_obs_rows(rb_sim *s, int32_t *rows) {
    if (check(s) || !rows) return fail(RB_EINVAL, "null argument");
    *rows = s->hist.rows;
    return RB_OK;
}

// ---- episode-end codes of the fused env step (done_kind_kernel) ----
int rb_env_done_kind_configure(rb_sim *s, int enable) {
    RB_RC(reconfigure(s, NEEDS_ENV | DROP_GRAPHS));      // nothing in flight may still write the planes
    s->done.release();
    if (!enable) return RB_OK;
    const size_t plane = sizeof(uint32_t) * size_t(s->n);
    RB_HIP(hipMalloc(&s->done.d_seen, plane));
    RB_HIP(hipMalloc(&s->done.d_kind, plane));
    RB_RC(done_rebase(s));                   // the next episode end is judged against the counters as they stand
    s->done.on = true;
    return RB_OK;
}
int rb_env_done_kind_ptr(rb_sim *s, uint32_t **d_kind) {
    if (check(s) || !d_kind) return fail(RB_EINVAL, "null argument");
    if (s->done.need()) return RB_EINVAL;
    *d_kind = s->done.d_kind;
    return RB_OK;
}

// ---- privileged critic rows behind the fused env step (env_critic.hpp) ----
int32_t rb_env_critic_obs_count(int32_t n_q, int32_t n_t, uint32_t mask, int32_t n_params, int32_t action_rows) {
    if (n_q < 0 || n_t < 0 || n_params < 0 || action_rows < 0 || (mask & ~uint32_t(RB_CRITIC_ALL))) return -1;
    return mask ? rbc::row_dim(int(mask | RB_CRITIC_STATE), n_q, n_params, action_rows * n_t) : 0;
}
int rb_env_critic_obs_configure(rb_sim *s, uint32_t mask) {
    int dim = 0;
    // nothing in flight may still write rows of the old width
    RB_RC(reconfigure(s, NEEDS_ENV | DROP_GRAPHS, [&]() -> int {
        if (mask & ~uint32_t(RB_CRITIC_ALL))
            return fail(RB_EINVAL, "unknown bits in the critic-row mask (RB_CRITIC_STATE | _AGE | _PARAMS | _DELAY | _ACTIONS)");
        if (s->tree && mask)
            return fail(RB_EUNSUPPORTED, "critic rows are built for ball-joint robots (1-16 tendons); joint trees have none");
        if (mask) mask |= RB_CRITIC_STATE;       // (always selected)
        if (mask & RB_CRITIC_PARAMS && !s->par.on) return fail(RB_EINVAL, "critic rows: RB_CRITIC_PARAMS needs per-env parameters (rb_params_enable first)");
        if (mask & RB_CRITIC_DELAY && !s->io.on) return fail(RB_EINVAL, "critic rows: RB_CRITIC_DELAY needs an io configuration (rb_env_io_configure first)");
        if (mask & RB_CRITIC_ACTIONS && !s->hist.rows)
            return fail(RB_EINVAL, "critic rows: RB_CRITIC_ACTIONS needs action rows in the observation (rb_env_action_obs_configure first)");
        dim = rbc::row_dim(int(mask), s->n_q, s->par.on ? s->par.n : 0, s->hist.rows * s->n_t);
        if (dim > RB_CRITIC_OBS_MAX_DIM)
            return fail(RB_EINVAL, "critic rows: " + std::to_string(dim) + " columns, at most RB_CRITIC_OBS_MAX_DIM = 63 (the PPO gradient kernels' input limit)");
        return RB_OK;
    }));
    s->critic.release();
    if (!mask) return RB_OK;
    RB_HIP(hipMalloc(&s->critic.d_rows, sizeof(float) * size_t(s->n) * size_t(dim)));
    s->critic.mask = int(mask); s->critic.dim = dim;
    // the rows of the envs as they stand (no observation rows at hand: zero action blocks, as behind a reset)
    return critic_launch(s, 0, s->n, s->stream, nullptr, s->critic.d_rows);
}
int rb_env_critic_obs_dim(rb_sim *s, int32_t *dim) {
    if (check(s) || !dim) return fail(RB_EINVAL, "null argument");
    *dim = s->critic.dim;
    return RB_OK;
}
int rb_env_critic_obs_ptr(rb_sim *s, float **d_rows) {
    if (check(s) || !d_rows) return fail(RB_EINVAL, "null argument");
    if (s->critic.need()) return RB_EINVAL;
    *d_rows = s->critic.d_rows;
    return RB_OK;
}

// ---- goal pool: env goals drawn from a set of poses instead of the box (env_goal.hpp) ----
int rb_env_goal_pool_set(rb_sim *s, const float *goal_q, int64_t m) {
    if (check(s) || !goal_q) return fail(RB_EINVAL, "null argument");
    OptGoals &g = s->goals;
    // nothing in flight may still read the rows.  The graphs stay: the handle's own are rollouts of the physics step, which reads no
    // goal, and a caller's captured env step reads the rows behind a pointer that never moves - its next replay sees the new ones
    RB_RC(reconfigure(s, KEEP_GRAPHS, [&]() -> int {
        if (m < 1 || m > int64_t(UINT32_MAX)) return fail(RB_EINVAL, "goal pool: m must be >= 1 (and below 2^32)");
        if (g.d_pool && m != g.m)
            return fail(RB_EINVAL, "goal pool: the handle's pool has " + std::to_string(g.m) + " rows, fixed by the first call; got " + std::to_string(m));
        // the angle box of rb_env_configure, or the robot's own box (what rb_sample_goals draws from) without an env layer
        for (int64_t r = 0; r < m; ++r)
            for (int j = 0; j < s->n_q; ++j) {
                const float v = goal_q[r * s->n_q + j];
                const float lo = s->env_ready ? s->env.a_lo : s->box.lo[j], hi = s->env_ready ? s->env.a_hi : s->box.hi[j];
                if (!std::isfinite(v) || v < lo || v > hi)
                    return fail(RB_EINVAL, "goal pool: row " + std::to_string(r) + ", joint " + std::to_string(j) + " is not finite or outside the angle box");
            }
        return RB_OK;
    }));
    const size_t bytes = sizeof(float) * size_t(m) * size_t(s->n_q);
    if (!g.d_pool) {
        float *d = nullptr;
        RB_RC(dev_alloc(&d, bytes, "hipMalloc (goal pool): "));
        const hipError_t e = hipMemcpy(d, goal_q, bytes, hipMemcpyHostToDevice);
        if (e != hipSuccess) { (void)hipFree(d); return fail(RB_EHIP, std::string("hipMemcpy (goal pool): ") + hipGetErrorString(e)); }
        g.d_pool = d; g.m = m;                   // (from here on behind_step and behind_reset launch goal_pool_kernel)
        // an env layer already drew every env's goal from the box (rb_env_configure resets): that draw's pool row takes its place,
        // counters untouched, so from here on every goal of the handle is a row of the pool
        return s->env_ready ? goal_pool_launch(s, 0, s->n, s->stream, nullptr, nullptr) : RB_OK;
    }
    RB_HIP(hipMemcpy(g.d_pool, goal_q, bytes, hipMemcpyHostToDevice));
    return RB_OK;
}
int rb_env_goal_pool_ptr(rb_sim *s, float **d_pool, int64_t *m) {
    if (check(s) || !d_pool || !m) return fail(RB_EINVAL, "null argument");
    if (s->goals.need_pool()) return RB_EINVAL;
    *d_pool = s->goals.d_pool; *m = s->goals.m;
    return RB_OK;
}

// ---- goal curriculum: a level per env over the pool's row order (env_goal.hpp) ----
int rb_env_goal_curriculum_configure(rb_sim *s, int32_t levels, int32_t up, int32_t down, int32_t level0) {
    // nothing in flight may still launch the pool's own kernel
    RB_RC(reconfigure(s, NEEDS_ENV | DROP_GRAPHS, [&]() -> int {
        const OptGoals &g = s->goals;
        if (!g.d_pool) return fail(RB_EINVAL, "goal curriculum: no goal pool is set (rb_env_goal_pool_set first)");
        if (g.L) return fail(RB_EINVAL, "goal curriculum: already configured (once per handle: a captured graph holds the arguments by value)");
        const int64_t most = g.m < RB_GOAL_LEVELS_MAX ? g.m : int64_t(RB_GOAL_LEVELS_MAX);
        if (levels < 1 || levels > most)
            return fail(RB_EINVAL, "goal curriculum: levels must be in 1.." + std::to_string(most) + " (at most the pool's rows and RB_GOAL_LEVELS_MAX = 256), got " +
                                       std::to_string(levels));
        if (up < 0 || down < 0) return fail(RB_EINVAL, "goal curriculum: up and down must be >= 0");
        if (level0 < 0 || level0 >= levels) return fail(RB_EINVAL, "goal curriculum: level0 must be in 0..levels - 1");
        return RB_OK;
    }));
    OptGoals &g = s->goals;
    const size_t plane = sizeof(uint32_t) * size_t(s->n);
    if (!g.d_level) {                       // (one block: the three planes, then the host histogram's L counts)
        uint32_t *d = nullptr;
        RB_RC(dev_alloc(&d, 3 * plane + sizeof(uint64_t) * RB_GOAL_LEVELS_MAX + 8, "hipMalloc (goal curriculum): "));
        g.d_level = d; g.d_index = d + s->n; g.d_seen = d + 2 * s->n;
        g.d_hist = reinterpret_cast<uint64_t *>((reinterpret_cast<uintptr_t>(d + 3 * s->n) + 7) & ~uintptr_t(7));
    }
    {
        std::vector<uint32_t> l0(size_t(s->n), uint32_t(level0));
        RB_HIP(hipMemcpy(g.d_level, l0.data(), plane, hipMemcpyHostToDevice));
    }
    g.L = uint32_t(levels); g.up = uint32_t(up); g.down = uint32_t(down);      // (from here on goal_pool_launch enqueues goal_curriculum_kernel)
    // every env's current goal, a row of the whole pool, becomes the row of that same draw inside its window (counters untouched);
    // the launch also sets `seen` to the counters as they stand and fills the index plane
    return goal_pool_launch(s, 0, s->n, s->stream, nullptr, nullptr);
}
int rb_env_goal_level_ptr(rb_sim *s, uint32_t **d_level) {
    if (check(s) || s->goals.need_curriculum()) return RB_EINVAL;
    if (!d_level) return fail(RB_EINVAL, "null argument");
    *d_level = s->goals.d_level;
    return RB_OK;
}
int rb_env_goal_index_ptr(rb_sim *s, uint32_t **d_index) {
    if (check(s) || s->goals.need_curriculum()) return RB_EINVAL;
    if (!d_index) return fail(RB_EINVAL, "null argument");
    *d_index = s->goals.d_index;
    return RB_OK;
}
int rb_env_goal_levels_set(rb_sim *s, const uint32_t *levels) {
    // nothing in flight may still move a level.  The graphs stay: a captured env step holds the plane's address and reads the new levels
    RB_RC(reconfigure(s, KEEP_GRAPHS, [&]() -> int {
        if (s->goals.need_curriculum()) return RB_EINVAL;
        if (!levels) return fail(RB_EINVAL, "null argument");
        for (long i = 0; i < s->n; ++i)
            if (levels[i] >= s->goals.L)
                return fail(RB_EINVAL, "goal levels: env " + std::to_string(i) + " has level " + std::to_string(levels[i]) + ", the curriculum has " +
                                           std::to_string(s->goals.L) + " levels");
        return RB_OK;
    }));
    RB_HIP(hipMemcpy(s->goals.d_level, levels, sizeof(uint32_t) * size_t(s->n), hipMemcpyHostToDevice));
    return RB_OK;
}
int rb_env_goal_level_hist_dev(rb_sim *s, uint64_t *d_out, void *hip_stream) {
    if (check(s) || s->goals.need_curriculum()) return RB_EINVAL;
    if (!d_out) return fail(RB_EINVAL, "null argument");
    RB_HIP(hipSetDevice(s->device));
    hipStream_t st = hip_stream ? static_cast<hipStream_t>(hip_stream) : s->stream;
    RB_HIP(hipMemsetAsync(d_out, 0, sizeof(uint64_t) * s->goals.L, st));
    // (at most 1024 x L atomics into the output)
    hipLaunchKernelGGL(rbg::goal_level_hist_kernel, dim3(stride_grid(s->n)), dim3(256), 0, st, s->goals.d_level, long(s->n), s->goals.L,
                       reinterpret_cast<unsigned long long *>(d_out));
    RB_HIP(hipGetLastError());
    return RB_OK;
}
int rb_env_goal_level_hist(rb_sim *s, uint64_t *out) {
    if (check(s) || s->goals.need_curriculum()) return RB_EINVAL;
    if (!out) return fail(RB_EINVAL, "null argument");
    RB_HIP(hipSetDevice(s->device));
    RB_RC(rb_env_goal_level_hist_dev(s, s->goals.d_hist, nullptr));
    RB_HIP(hipMemcpyAsync(out, s->goals.d_hist, sizeof(uint64_t) * s->goals.L, hipMemcpyDeviceToHost, s->stream));
    RB_HIP(hipStreamSynchronize(s->stream));
    return RB_OK;
}

// ---- outcome counts per pool row, and re-ordering a live pool (env_goal.hpp) ----
int rb_env_goal_row_stats_enable(rb_sim *s) {
    // nothing in flight may still launch the curriculum's own kernel
    RB_RC(reconfigure(s, DROP_GRAPHS, [&]() -> int {
        if (s->goals.need_curriculum()) return RB_EINVAL;
        if (s->goals.d_row_stats) return fail(RB_EINVAL, "goal row stats: already enabled (once per handle: a captured graph holds the kernel it was captured with)");
        return RB_OK;
    }));
    const size_t bytes = sizeof(uint64_t) * 2 * size_t(s->goals.m);
    uint64_t *d = nullptr;
    RB_RC(dev_alloc(&d, bytes, "hipMalloc (goal row stats): "));
    hipError_t e = hipMemset(d, 0, bytes);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) { (void)hipFree(d); return fail(RB_EHIP, std::string("hipMemset (goal row stats): ") + hipGetErrorString(e)); }
    s->goals.d_row_stats = d;                // (from here on goal_pool_launch enqueues goal_curriculum_stats_kernel)
    return RB_OK;
}
int rb_env_goal_row_stats_ptr(rb_sim *s, uint64_t **d_counts, int64_t *m) {
    if (check(s) || s->goals.need_row_stats()) return RB_EINVAL;
    if (!d_counts || !m) return fail(RB_EINVAL, "null argument");
    *d_counts = s->goals.d_row_stats; *m = s->goals.m;
    return RB_OK;
}
int rb_env_goal_row_stats_read(rb_sim *s, uint64_t *host, int clear) {
    // every count enqueued so far is in.  The graphs stay: a read changes nothing they hold, a clear writes the planes in place
    RB_RC(reconfigure(s, KEEP_GRAPHS, [&]() -> int { return s->goals.need_row_stats() ? RB_EINVAL : host ? RB_OK : fail(RB_EINVAL, "null argument"); }));
    const size_t bytes = sizeof(uint64_t) * 2 * size_t(s->goals.m);
    RB_HIP(hipMemcpy(host, s->goals.d_row_stats, bytes, hipMemcpyDeviceToHost));
    if (clear) {
        RB_HIP(hipMemset(s->goals.d_row_stats, 0, bytes));
        RB_HIP(hipDeviceSynchronize());
    }
    return RB_OK;
}
int rb_env_goal_row_stats_set(rb_sim *s, const uint64_t *host) {
    const int64_t m = s ? s->goals.m : 0;
    // nothing in flight may still add to the planes.  The graphs stay: the planes are written in place
    RB_RC(reconfigure(s, KEEP_GRAPHS, [&]() -> int {
        if (s->goals.need_row_stats()) return RB_EINVAL;
        if (!host) return fail(RB_EINVAL, "null argument");
        for (int64_t k = 0; k < m; ++k)
            if (host[m + k] > host[k])
                return fail(RB_EINVAL, "goal row stats: row " + std::to_string(k) + " has reached " + std::to_string(host[m + k]) + " > attempts " +
                                           std::to_string(host[k]));
        return RB_OK;
    }));
    RB_HIP(hipMemcpy(s->goals.d_row_stats, host, sizeof(uint64_t) * 2 * size_t(m), hipMemcpyHostToDevice));
    return RB_OK;
}
int rb_env_goal_pool_permute(rb_sim *s, const uint32_t *order) {
    if (check(s) || !order) return fail(RB_EINVAL, "null argument");
    OptGoals &g = s->goals;
    const size_t m = size_t(g.m), nq = size_t(s->n_q);
    std::vector<uint32_t> inv(m, UINT32_MAX);        // inv[old row] = new row
    // nothing in flight may still read the rows, the indices or the counts.  The graphs stay: rows, counts and indices are re-ordered
    // IN PLACE - no pointer moves - so a graph captured earlier reads the new order
    RB_RC(reconfigure(s, KEEP_GRAPHS, [&]() -> int {
        if (g.need_pool()) return RB_EINVAL;
        for (size_t j = 0; j < m; ++j) {
            if (order[j] >= m) return fail(RB_EINVAL, "goal pool permute: entry " + std::to_string(j) + " is " + std::to_string(order[j]) + ", the pool has " + std::to_string(m) + " rows");
            if (inv[order[j]] != UINT32_MAX) return fail(RB_EINVAL, "goal pool permute: row " + std::to_string(order[j]) + " occurs twice (not a permutation)");
            inv[order[j]] = uint32_t(j);
        }
        return RB_OK;
    }));
    uint32_t *d_inv = nullptr;
    if (g.L) RB_RC(dev_alloc(&d_inv, sizeof(uint32_t) * m, "hipMalloc (goal pool permute): "));      // (before anything changes)
    auto done = [&](hipError_t e, const char *what) {
        (void)hipFree(d_inv);
        return e == hipSuccess ? RB_OK : fail(RB_EHIP, std::string(what) + " (goal pool permute): " + hipGetErrorString(e));
    };
    std::vector<float> rows(m * nq), out(m * nq);        // the rows through the host
    hipError_t e = hipMemcpy(rows.data(), g.d_pool, sizeof(float) * m * nq, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return done(e, "hipMemcpy");
    for (size_t j = 0; j < m; ++j) std::memcpy(&out[j * nq], &rows[size_t(order[j]) * nq], sizeof(float) * nq);
    e = hipMemcpy(g.d_pool, out.data(), sizeof(float) * m * nq, hipMemcpyHostToDevice);
    if (e != hipSuccess) return done(e, "hipMemcpy");
    if (g.d_row_stats) {                     // both count planes travel with their rows
        std::vector<uint64_t> cnt(2 * m), cout2(2 * m);
        e = hipMemcpy(cnt.data(), g.d_row_stats, sizeof(uint64_t) * 2 * m, hipMemcpyDeviceToHost);
        if (e != hipSuccess) return done(e, "hipMemcpy");
        for (size_t j = 0; j < m; ++j) { cout2[j] = cnt[order[j]]; cout2[m + j] = cnt[m + order[j]]; }
        e = hipMemcpy(g.d_row_stats, cout2.data(), sizeof(uint64_t) * 2 * m, hipMemcpyHostToDevice);
        if (e != hipSuccess) return done(e, "hipMemcpy");
    }
    if (g.L) {                               // every env keeps the pose it holds: its index becomes that row's new number
        e = hipMemcpy(d_inv, inv.data(), sizeof(uint32_t) * m, hipMemcpyHostToDevice);
        if (e != hipSuccess) return done(e, "hipMemcpy");
        hipLaunchKernelGGL(rbg::goal_index_permute_kernel, dim3(stride_grid(s->n)), dim3(256), 0, s->stream, g.d_index, d_inv, long(s->n), uint32_t(m));
        e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
        if (e != hipSuccess) return done(e, "index kernel");
    }
    return done(hipSuccess, "");
}

// ---- reward shaping around the fused env step (env_shaping.hpp) ----
int rb_env_shaping_configure(rb_sim *s, const rb_env_shaping_config *cfg) {
    rb_env_shaping_config w = {};
    if (cfg) { w.action_rate = cfg->action_rate; w.tension = cfg->tension; w.activation = cfg->activation; }
    const bool off = w.action_rate == 0.0f && w.tension == 0.0f && w.activation == 0.0f;      // (also -0.0)
    int waves = 1;
    // nothing in flight may still use the planes, and a captured graph holds the launches of the handle as it was
    RB_RC(reconfigure(s, NEEDS_ENV | DROP_GRAPHS, [&]() -> int {
        for (float v : {w.action_rate, w.tension, w.activation})
            if (!std::isfinite(v) || v < 0.0f) return fail(RB_EINVAL, "reward shaping: the weights must be finite and >= 0");
        if (off) return RB_OK;
        RB_RC(shaping_compatible(s, w, s->par.on, s->io.on ? s->io.cfg.delay_hi : 0));
        if (s->tree) {                          // the cost kernel's workgroup: the readout's, fewer waves where the terms do not fit beside them
            waves = s->tree_waves;
            while (waves > 0 && shaping_tree_lds(s, waves) > 160 * 1024) --waves;
            if (!waves) return fail(RB_EUNSUPPORTED, "reward shaping: the robot's working set and the per-tendon terms exceed the 160 KiB LDS of a CU");
        }
        return RB_OK;
    }));
    OptShaping &o = s->shaping;
    if (off) { o.release(); return RB_OK; }
    const size_t n = size_t(s->n);
    if (!o.d_prev) {
        auto alloc = [](auto **d, size_t bytes) { return dev_alloc(d, bytes, "hipMalloc (reward shaping): "); };
        int rc = alloc(&o.d_prev, sizeof(float) * n * size_t(s->n_t));
        if (rc == RB_OK) rc = alloc(&o.d_cost, sizeof(float) * n);
        if (rc == RB_OK) rc = alloc(&o.d_run, sizeof(double) * n);
        if (rc == RB_OK) rc = alloc(&o.d_sums, sizeof(double) * 2 * n);
        if (rc == RB_OK) rc = alloc(&o.d_cnt, sizeof(uint32_t) * 2 * n);
        if (rc == RB_OK) rc = alloc(&o.d_red, sizeof(double) * 4 * (rbs::REDUCE_BLOCKS + 1));
        if (rc) { o.release(); return rc; }
    }
    o.cfg = w; o.tree_waves = waves; o.on = true;
    // the episodes as they stand: no cost so far, and a previous row of zeros where an episode is already under way
    RB_HIP(hipMemsetAsync(o.d_prev, 0, sizeof(float) * n * size_t(s->n_t), s->stream));
    RB_RC(shaping_restart(s));
    return shaping_clear_sums(s);
}
int rb_env_shaping_cost_ptr(rb_sim *s, float **d_cost) {
    if (check(s) || !d_cost) return fail(RB_EINVAL, "null argument");
    if (s->shaping.need()) return RB_EINVAL;
    *d_cost = s->shaping.d_cost;
    return RB_OK;
}
int rb_env_shaping_stats(rb_sim *s, double *out, int reset) {
    // every cost enqueued so far is in.  The graphs stay: a read changes nothing they hold, a clear writes the planes in place
    RB_RC(reconfigure(s, KEEP_GRAPHS, [&]() -> int { return s->shaping.need() ? RB_EINVAL : out ? RB_OK : fail(RB_EINVAL, "null argument"); }));
    const OptShaping &o = s->shaping;
    unsigned g = blocks_for(s->n, 256);
    if (g > unsigned(rbs::REDUCE_BLOCKS)) g = rbs::REDUCE_BLOCKS;
    double *result = o.d_red + 4 * rbs::REDUCE_BLOCKS;
    hipLaunchKernelGGL(rbs::shaping_reduce, dim3(g), dim3(256), 0, s->stream, o.d_sums, o.d_cnt, o.d_red, long(s->n));
    hipLaunchKernelGGL(rbs::shaping_reduce_final, dim3(1), dim3(256), 0, s->stream, o.d_red, int(g), result);
    RB_HIP(hipGetLastError());
    RB_HIP(hipMemcpyAsync(out, result, sizeof(double) * 4, hipMemcpyDeviceToHost, s->stream));
    RB_HIP(hipStreamSynchronize(s->stream));
    return reset ? shaping_clear_sums(s) : RB_OK;
}

// ---- random velocity pushes in front of the fused env step (env_push.hpp) ----
int rb_env_push_configure(rb_sim *s, const rb_env_push_config *cfg) {
    rb_env_push_config c = {};
    bool off = true;
    // nothing in flight may still use the planes, and a captured graph holds the launches of the handle as it was
    RB_RC(reconfigure(s, NEEDS_ENV | DROP_GRAPHS, [&]() -> int {
        if (!cfg) return RB_OK;
        if (cfg->threshold > (1u << 24)) return fail(RB_EINVAL, "random pushes: threshold must be in 0 .. 2^24 (P(push per env step) = threshold / 2^24)");
        c.threshold = cfg->threshold;
        bool any = false;
        for (int j = 0; j < s->n_q; ++j) {
            const float v = cfg->sigma[j];
            if (!std::isfinite(v) || v < 0.0f) return fail(RB_EINVAL, "random pushes: the sigmas of the robot's joints must be finite and >= 0");
            c.sigma[j] = v;
            any = any || v != 0.0f;
        }
        off = c.threshold == 0u || !any;
        return RB_OK;
    }));
    OptPush &o = s->push;
    if (off) { o.release(); return RB_OK; }
    const size_t n = size_t(s->n);
    if (!o.d_count) {
        auto alloc = [](auto **d, size_t bytes) { return dev_alloc(d, bytes, "hipMalloc (random pushes): "); };
        OptPush fresh;
        int rc = alloc(&fresh.d_count, sizeof(uint32_t) * n);
        if (rc == RB_OK) rc = alloc(&fresh.d_last, sizeof(uint32_t) * n);
        if (rc == RB_OK) rc = alloc(&fresh.d_n, sizeof(uint32_t) * n);
        if (rc == RB_OK) rc = alloc(&fresh.d_impulse, sizeof(float) * n * size_t(s->n_q));
        if (rc == RB_OK) rc = alloc(&fresh.d_total, sizeof(unsigned long long));
        if (rc) { fresh.release(); return rc; }      // (the handle as it was: the option was off)
        o = fresh;
    }
    o.cfg = c; o.on = true;
    return push_clear(s);
}
int rb_env_push_ptr(rb_sim *s, uint32_t **d_count, uint32_t **d_last, uint32_t **d_n_pushes, float **d_impulse) {
    if (check(s) || s->push.need()) return RB_EINVAL;
    if (d_count) *d_count = s->push.d_count;
    if (d_last) *d_last = s->push.d_last;
    if (d_n_pushes) *d_n_pushes = s->push.d_n;
    if (d_impulse) *d_impulse = s->push.d_impulse;
    return RB_OK;
}
int rb_env_push_count(rb_sim *s, uint64_t *pushes, int reset) {
    // every push enqueued so far is in.  The graphs stay: a read changes nothing they hold, a clear writes the plane in place
    RB_RC(reconfigure(s, KEEP_GRAPHS, [&]() -> int { return s->push.need() ? RB_EINVAL : pushes ? RB_OK : fail(RB_EINVAL, "null argument"); }));
    const OptPush &o = s->push;
    unsigned long long total = 0;
    RB_HIP(hipMemsetAsync(o.d_total, 0, sizeof(total), s->stream));
    hipLaunchKernelGGL(rbpush::push_count_sum, dim3(stride_grid(s->n)), dim3(256), 0, s->stream, o.d_n, long(s->n), o.d_total);
    RB_HIP(hipGetLastError());
    RB_HIP(hipMemcpyAsync(&total, o.d_total, sizeof(total), hipMemcpyDeviceToHost, s->stream));
    RB_HIP(hipStreamSynchronize(s->stream));
    *pushes = uint64_t(total);
    if (reset) RB_HIP(hipMemsetAsync(o.d_n, 0, sizeof(uint32_t) * size_t(s->n), s->stream));
    return RB_OK;
}

// ---- per-env episode records behind the fused env step (env_episode_log.hpp) ----
int rb_env_episode_log_configure(rb_sim *s, int32_t capacity) {
    // nothing in flight may still write the planes, and a captured graph holds the launches of the handle as it was
    RB_RC(reconfigure(s, NEEDS_ENV | DROP_GRAPHS, [&]() -> int {
        if (capacity < 0 || capacity > RB_EPISODE_LOG_MAX)
            return fail(RB_EINVAL, "episode log: capacity must be in 0 .. RB_EPISODE_LOG_MAX = 64 (0 switches it off), got " + std::to_string(capacity));
        return RB_OK;
    }));
    OptEpisodeLog &o = s->elog;
    if (!capacity) { o.release(); return RB_OK; }
    const size_t n = size_t(s->n), E = size_t(capacity);
    if (o.E != capacity) {
        auto alloc = [](auto **d, size_t bytes) { return dev_alloc(d, bytes, "hipMalloc (episode log): "); };
        OptEpisodeLog fresh;
        int rc = alloc(&fresh.d_acc, sizeof(float) * n);
        if (rc == RB_OK) rc = alloc(&fresh.d_age, sizeof(uint32_t) * n);
        if (rc == RB_OK) rc = alloc(&fresh.d_seen, sizeof(uint32_t) * n);
        if (rc == RB_OK) rc = alloc(&fresh.d_count, sizeof(uint32_t) * n);
        if (rc == RB_OK) rc = alloc(&fresh.d_ret, sizeof(float) * E * n);
        if (rc == RB_OK) rc = alloc(&fresh.d_len, sizeof(uint32_t) * E * n);
        if (rc == RB_OK) rc = alloc(&fresh.d_kind, sizeof(uint32_t) * E * n);
        if (rc == RB_OK) rc = alloc(&fresh.d_full, sizeof(uint32_t));
        if (rc == RB_OK) rc = alloc(&fresh.d_red, sizeof(double) * 8 * (rbel::SUMMARY_BLOCKS + 2));
        if (rc) { fresh.release(); return rc; }      // (the handle as it was)
        o.release();
        o = fresh;
        o.E = capacity;
        RB_HIP(hipMemsetAsync(o.d_red, 0, sizeof(double) * 8 * (rbel::SUMMARY_BLOCKS + 2), s->stream));      // (the ticket word)
    }
    RB_HIP(hipMemsetAsync(o.d_ret, 0, sizeof(float) * E * n, s->stream));
    RB_HIP(hipMemsetAsync(o.d_len, 0, sizeof(uint32_t) * E * n, s->stream));
    RB_HIP(hipMemsetAsync(o.d_kind, 0, sizeof(uint32_t) * E * n, s->stream));
    return episode_log_clear(s);
}
int rb_env_episode_log_ptr(rb_sim *s, uint32_t **d_count, float **d_ret, uint32_t **d_len, uint32_t **d_kind, uint32_t **d_full, int32_t *capacity) {
    if (check(s) || s->elog.need()) return RB_EINVAL;
    if (d_count) *d_count = s->elog.d_count;
    if (d_ret) *d_ret = s->elog.d_ret;
    if (d_len) *d_len = s->elog.d_len;
    if (d_kind) *d_kind = s->elog.d_kind;
    if (d_full) *d_full = s->elog.d_full;
    if (capacity) *capacity = s->elog.E;
    return RB_OK;
}
int rb_env_episode_log_clear(rb_sim *s) {
    if (check(s) || s->elog.need()) return RB_EINVAL;
    RB_HIP(hipSetDevice(s->device));
    // (no drain, no graph dropped: memsets and one copy on the handle's stream, behind whatever was enqueued or replayed there; a
    // captured env step holds the planes' addresses and finds them cleared)
    return episode_log_clear(s);
}
int rb_env_episode_log_summary_dev(rb_sim *s, int32_t first_k, double *d_out8) {
    if (check(s) || s->elog.need()) return RB_EINVAL;
    if (first_k < 1) return fail(RB_EINVAL, "episode log summary: first_k must be >= 1");
    RB_HIP(hipSetDevice(s->device));
    const OptEpisodeLog &o = s->elog;
    unsigned g = blocks_for(s->n, 256);
    if (g > unsigned(rbel::SUMMARY_BLOCKS)) g = rbel::SUMMARY_BLOCKS;
    double *partials = o.d_red + 8;
    unsigned int *ticket = reinterpret_cast<unsigned int *>(o.d_red + 8 * (rbel::SUMMARY_BLOCKS + 1));
    hipLaunchKernelGGL(rbel::episode_log_summary, dim3(g), dim3(256), 0, s->stream, o.d_count, o.d_ret, o.d_len, o.d_kind, uint32_t(first_k), partials,
                       ticket, o.d_red, d_out8, long(s->n));
    RB_HIP(hipGetLastError());
    return RB_OK;
}
int rb_env_episode_log_summary(rb_sim *s, int32_t first_k, double *out8) {
    if (check(s) || !out8) return fail(RB_EINVAL, "null argument");
    RB_RC(rb_env_episode_log_summary_dev(s, first_k, nullptr));
    RB_HIP(hipMemcpyAsync(out8, s->elog.d_red, sizeof(double) * 8, hipMemcpyDeviceToHost, s->stream));
    RB_HIP(hipStreamSynchronize(s->stream));
    return RB_OK;
}

// ---- start poses: episodes begin at a row of a pool instead of the zero pose (env_start.hpp) ----
int rb_env_start_poses_configure(rb_sim *s, const float *rows, int64_t m, double prob) {
    uint32_t threshold = 0;
    // nothing in flight may still use the pool or the planes, and a captured graph holds the launches of the handle as it was
    RB_RC(reconfigure(s, NEEDS_ENV | DROP_GRAPHS, [&]() -> int {
        if (m == 0) return RB_OK;
        if (m < 1 || m > int64_t(UINT32_MAX)) return fail(RB_EINVAL, "start poses: m must be >= 1 (and below 2^32; 0 switches the option off)");
        if (!rows) return fail(RB_EINVAL, "null argument");
        if (!(prob >= 0.0 && prob <= 1.0)) return fail(RB_EINVAL, "start poses: prob must be in [0, 1]");
        threshold = uint32_t(std::nearbyint(prob * 16777216.0));
        if (s->chan.mask) return fail(RB_EUNSUPPORTED, START_POSES_TENDON_OBS);
        return start_rows_check(s, rows, m);
    }));
    OptStart &o = s->start;
    if (m == 0) { o.release(); return RB_OK; }
    const size_t bytes = sizeof(float) * size_t(m) * size_t(s->n_q), plane = sizeof(uint32_t) * size_t(s->n);
    if (o.m != m) {
        auto alloc = [](auto **d, size_t b) { return dev_alloc(d, b, "hipMalloc (start poses): "); };
        OptStart fresh;
        int rc = alloc(&fresh.d_pool, bytes);
        if (rc == RB_OK) rc = alloc(&fresh.d_count, plane);
        if (rc == RB_OK) rc = alloc(&fresh.d_index, plane);
        if (rc) { fresh.release(); return rc; }      // (the handle as it was)
        o.release();
        o = fresh;
        o.m = m;
    }
    o.threshold = threshold; o.prob = prob;
    RB_HIP(hipMemcpy(o.d_pool, rows, bytes, hipMemcpyHostToDevice));
    return start_clear(s);
}
int rb_env_start_poses_set(rb_sim *s, const float *rows, int64_t m) {
    // nothing in flight may still read the rows.  The graphs stay: a captured env step reads the rows behind a pointer that never
    // moves - its next replay sees the new ones
    RB_RC(reconfigure(s, KEEP_GRAPHS, [&]() -> int {
        if (s->start.need()) return RB_EINVAL;
        if (!rows) return fail(RB_EINVAL, "null argument");
        if (m != s->start.m)
            return fail(RB_EINVAL, "start poses: the handle's pool has " + std::to_string(s->start.m) + " rows, fixed by rb_env_start_poses_configure; got " +
                                       std::to_string(m));
        return start_rows_check(s, rows, m);
    }));
    RB_HIP(hipMemcpy(s->start.d_pool, rows, sizeof(float) * size_t(m) * size_t(s->n_q), hipMemcpyHostToDevice));
    return RB_OK;
}
int rb_env_start_poses_ptr(rb_sim *s, float **d_pool, int64_t *m, uint32_t **d_count, uint32_t **d_index) {
    if (check(s) || s->start.need()) return RB_EINVAL;
    if (d_pool) *d_pool = s->start.d_pool;
    if (m) *m = s->start.m;
    if (d_count) *d_count = s->start.d_count;
    if (d_index) *d_index = s->start.d_index;
    return RB_OK;
}

// ---- per-env physical parameters (env_params.hpp) ----
int rb_params_enable(rb_sim *s, int32_t *n_params) {
    // (no env layer needed: the plain step has a parameter form.)  Nothing in flight may read the planes while they are reset, and
    // captured graphs hold the nominal kernels' nodes
    RB_RC(reconfigure(s, DROP_GRAPHS, [&]() -> int {
        if (s->tree) return fail(RB_EUNSUPPORTED, "per-env parameters are built for ball-joint robots (the closed-form kernels); joint trees have none");
        return s->shaping.on ? shaping_compatible(s, s->shaping.cfg, true, 0) : RB_OK;
    }));
    OptParams &p = s->par;
    const int nt = s->n_t, P = rbp::n_params(nt);
    const size_t n = size_t(s->n);
    if (!p.d_planes) {
        auto alloc = [](auto **d, size_t bytes) { return dev_alloc(d, bytes, "parameter planes: "); };
        int rc1 = alloc(&p.d_planes, sizeof(float) * size_t(P) * n);
        if (rc1 == RB_OK) rc1 = alloc(&p.d_draws, sizeof(uint32_t) * n);
        if (rc1 == RB_OK) rc1 = alloc(&p.d_ranges, sizeof(float) * 2 * size_t(P));
        if (rc1) { p.release(); return rc1; }
    }
    // nominal values: force scales 1, offsets 0, mass scale 1, damping scales 1; counters 0; ranges lo = hi = nominal, no redraw
    uint32_t one, zero = 0u;
    const float onef = 1.0f;
    std::memcpy(&one, &onef, 4);
    RB_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(p.d_planes), int(one), size_t(nt) * n, s->stream));
    RB_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(p.d_planes + size_t(nt) * n), int(zero), size_t(nt) * n, s->stream));
    RB_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(p.d_planes + size_t(2 * nt) * n), int(one), 4 * n, s->stream));
    RB_HIP(hipMemsetAsync(p.d_draws, 0, sizeof(uint32_t) * n, s->stream));
    p.ranges.assign(2 * size_t(P), 1.0f);
    for (int k = 0; k < nt; ++k) p.ranges[nt + k] = p.ranges[P + nt + k] = 0.0f;
    RB_HIP(hipMemcpyAsync(p.d_ranges, p.ranges.data(), sizeof(float) * 2 * size_t(P), hipMemcpyHostToDevice, s->stream));
    RB_HIP(hipStreamSynchronize(s->stream));
    p.n = P; p.resample = false; p.on = true;
    if (n_params) *n_params = P;
    return RB_OK;
}
int rb_params_disable(rb_sim *s) {
    RB_RC(reconfigure(s, DROP_GRAPHS));      // captured graphs hold the parameter kernels' nodes
    s->par.release();
    return RB_OK;
}
int rb_params_ptr(rb_sim *s, float **d_params, uint32_t **d_draws) {
    if (check(s) || s->par.need()) return RB_EINVAL;
    if (d_params) *d_params = s->par.d_planes;
    if (d_draws) *d_draws = s->par.d_draws;
    return RB_OK;
}
int rb_params_set_ranges(rb_sim *s, const float *lo, const float *hi, int resample_on_reset) {
    if (check(s) || !lo || !hi) return fail(RB_EINVAL, "null argument");
    OptParams &p = s->par;
    // a kernel in flight may be reading the ranges.  The graphs stay: the ranges are written in place, behind the pointer a captured
    // launch holds (the resample flag travels by value: set it before anything is captured)
    RB_RC(reconfigure(s, KEEP_GRAPHS, [&]() -> int {
        if (p.need()) return RB_EINVAL;
        const int nt = s->n_t;
        for (int k = 0; k < p.n; ++k) {
            const std::string at = "parameter " + std::to_string(k) + ": ";
            if (!std::isfinite(lo[k]) || !std::isfinite(hi[k])) return fail(RB_EINVAL, at + "range bounds must be finite");
            if (lo[k] > hi[k]) return fail(RB_EINVAL, at + "lo > hi");
            if (k == 2 * nt && !(lo[k] > 0.0f)) return fail(RB_EINVAL, at + "mass_scale must stay > 0");
            if ((k < nt || k > 2 * nt) && lo[k] < 0.0f) return fail(RB_EINVAL, at + "force_scale and damping_scale must stay >= 0");
        }
        return RB_OK;
    }));
    p.ranges.assign(lo, lo + p.n);
    p.ranges.insert(p.ranges.end(), hi, hi + p.n);
    RB_HIP(hipMemcpyAsync(p.d_ranges, p.ranges.data(), sizeof(float) * 2 * size_t(p.n), hipMemcpyHostToDevice, s->stream));
    RB_HIP(hipStreamSynchronize(s->stream));
    p.resample = resample_on_reset != 0;
    return RB_OK;
}
int rb_params_sample_dev(rb_sim *s, const uint8_t *d_mask) {
    if (check(s) || s->par.need()) return RB_EINVAL;
    RB_HIP(hipSetDevice(s->device));
    hipLaunchKernelGGL(rbp::params_sample, dim3(blocks_for(s->n, 256)), dim3(256), 0, s->stream, s->par.d_planes, s->par.d_draws, s->par.d_ranges,
                       d_mask, s->par.n, s->n, s->seed, uint64_t(s->env0));
    RB_HIP(hipGetLastError());
    return RB_OK;
}

// ---- the handle's state as one blob (state_segments(), roboy_sim.hip) ----
int rb_env_state_segments(rb_sim *s, rb_state_segment *out, int32_t capacity, int32_t *count) {
    if (check(s) || !count || capacity < 0 || (capacity > 0 && !out)) return fail(RB_EINVAL, "null argument");
    const std::vector<StateSeg> segs = state_segments(s);
    std::vector<int64_t> offsets;
    state_layout(segs, &offsets);
    *count = int32_t(segs.size());
    for (size_t k = 0; k < segs.size() && k < size_t(capacity); ++k) {
        rb_state_segment &o = out[k];
        std::memset(&o, 0, sizeof(o));
        std::strncpy(o.name, segs[k].name, sizeof(o.name) - 1);
        o.dtype = segs[k].dtype; o.rows = segs[k].rows; o.cols = segs[k].cols; o.offset = offsets[k];
    }
    return RB_OK;
}
int rb_env_state_bytes(rb_sim *s, int64_t *bytes) {
    if (check(s) || !bytes) return fail(RB_EINVAL, "null argument");
    *bytes = state_layout(state_segments(s), nullptr);
    return RB_OK;
}
namespace {
int state_blob_check(const std::vector<StateSeg> &segs, const void *d_blob, int64_t bytes) {
    if (!d_blob) return fail(RB_EINVAL, "null argument");
    if (reinterpret_cast<uintptr_t>(d_blob) % 16) return fail(RB_EINVAL, "env state: the blob must be 16-byte aligned");
    const int64_t want = state_layout(segs, nullptr);
    if (bytes != want)
        return fail(RB_EINVAL, "env state: the handle's state has " + std::to_string(want) + " bytes (rb_env_state_bytes), got " + std::to_string(bytes));
    return RB_OK;
}
}  // namespace
int rb_env_state_save_dev(rb_sim *s, void *d_blob, int64_t bytes, rb_state_host *host) {
    if (check(s)) return RB_EINVAL;
    const std::vector<StateSeg> segs = state_segments(s);
    RB_RC(state_blob_check(segs, d_blob, bytes));
    RB_HIP(hipSetDevice(s->device));
    // (no drain, no graph dropped: copies on the handle's stream, behind whatever was enqueued or replayed there)
    std::vector<int64_t> offsets;
    state_layout(segs, &offsets);
    for (size_t k = 0; k < segs.size(); ++k)
        RB_HIP(hipMemcpyAsync(static_cast<char *>(d_blob) + offsets[k], segs[k].ptr, state_seg_bytes(segs[k]), hipMemcpyDeviceToDevice, s->stream));
    if (host) { std::memset(host, 0, sizeof(*host)); host->env_steps = s->env_steps; }
    return RB_OK;
}
int rb_env_state_load_dev(rb_sim *s, const void *d_blob, int64_t bytes, const rb_state_host *host) {
    std::vector<StateSeg> segs;
    // nothing in flight may still read or write a plane.  The graphs stay: every plane is written IN PLACE - no pointer moves - so a
    // captured graph's next replay continues from the restored state
    RB_RC(reconfigure(s, KEEP_GRAPHS, [&]() -> int {
        segs = state_segments(s);
        if (host && !(host->env_steps >= 0.0)) return fail(RB_EINVAL, "env state: env_steps must be >= 0");
        return state_blob_check(segs, d_blob, bytes);
    }));
    std::vector<int64_t> offsets;
    state_layout(segs, &offsets);
    for (size_t k = 0; k < segs.size(); ++k)
        RB_HIP(hipMemcpyAsync(segs[k].ptr, static_cast<const char *>(d_blob) + offsets[k], state_seg_bytes(segs[k]), hipMemcpyDeviceToDevice, s->stream));
    RB_HIP(hipStreamSynchronize(s->stream));      // (the blob is the caller's: it may free it when the call returns)
    if (host) s->env_steps = host->env_steps;
    return RB_OK;
}

}  // extern "C"
