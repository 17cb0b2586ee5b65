// fa_api.hip -- the core of the C ABI declared in include/fortattack.h: the handle (create / destroy), reset / step, the bound
// storage and the collector's step launches, state access.  Owns the fp64 SoA world state + RNG state in HBM; everything else
// belongs to the caller.  The exports of a subsystem live beside its kernels (fa_collect.hip, fa_policy.hip, fa_match.hip, ...);
// what they share with this file is fa_env.h.
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "fa_env.h"
#include "experiments/fa_step_experiments.h"

static thread_local std::string g_err;

int fa_api_fail(int code, const std::string &msg) {
    g_err = msg;
    return code;
}

namespace {
// Python float modulo (core.py:336: u[2] % (2*pi)): result takes the sign of the divisor.
double py_mod(double a, double b) {
    double r = std::fmod(a, b);
    if (r != 0.0 && ((b < 0) != (r < 0))) r += b;
    return r;
}

FaDerived derive(const fa_world_consts &w) {
    const double pi = 3.141592653589793; // np.pi
    FaDerived d;
    d.agent_size = w.agent_size;
    d.accel = w.accel;
    d.max_speed = w.max_speed;
    d.fort_dim = w.fort_dim;
    d.door_x = w.door_x;
    d.door_y = w.door_y;
    d.dt = w.dt;
    d.one_minus_damping = 1 - w.damping;           // core.py:328
    d.contact_force = w.contact_force;
    d.contact_margin = w.contact_margin;
    d.dist_min = w.agent_size + w.agent_size;      // core.py:449
    d.wall_xmin = w.wall_xmin;
    d.wall_xmax = w.wall_xmax;
    d.wall_ymin = w.wall_ymin;
    d.wall_ymax = w.wall_ymax;
    d.shoot_rad = w.shoot_rad;
    d.half_win = w.shoot_win / 2;                  // core.py:376
    d.cos_hw = std::cos(d.half_win);
    d.sin_hw = std::sin(d.half_win);
    d.shoot_far = w.shoot_rad * d.cos_hw;
    {   // largest double x with sqrt(x) <= max_speed (host sqrt is correctly rounded)
        double x = w.max_speed * w.max_speed;
        while (std::sqrt(x) > w.max_speed) x = std::nextafter(x, 0.0);
        while (std::sqrt(std::nextafter(x, INFINITY)) <= w.max_speed) x = std::nextafter(x, INFINITY);
        d.speed2_max = x;
    }
    {   // `sqrt(dd) < fort_dim` decided on dd: the largest double whose correctly rounded sqrt is < fort_dim
        double x = w.fort_dim * w.fort_dim;
        while (std::sqrt(x) >= w.fort_dim) x = std::nextafter(x, 0.0);
        while (std::sqrt(std::nextafter(x, INFINITY)) < w.fort_dim) x = std::nextafter(x, INFINITY);
        d.fort2_max = x;
    }
    d.rot_pos = py_mod(+w.max_rot, 2 * pi);        // core.py:336
    d.rot_neg = py_mod(-w.max_rot, 2 * pi);
    d.ang_guard = 3 * pi / 2;                      // fortattack_env_v1.py:59
    d.ang_attacker = pi / 2;
    // fortattack_env_v1.py:66  uniform(xMin,xMax), uniform(yMin, 0.8*yMin): lo + (hi-lo)*u
    d.att_x_lo = w.wall_xmin;
    d.att_x_rng = w.wall_xmax - w.wall_xmin;
    d.att_y_lo = w.wall_ymin;
    d.att_y_rng = 0.8 * w.wall_ymin - w.wall_ymin;
    // fortattack_env_v1.py:70  uniform(-0.8*fortDim/2, 0.8*fortDim/2), uniform(0.8*yMax, yMax)
    d.grd_x_lo = -0.8 * w.fort_dim / 2;
    d.grd_x_rng = 0.8 * w.fort_dim / 2 - d.grd_x_lo;
    d.grd_y_lo = 0.8 * w.wall_ymax;
    d.grd_y_rng = w.wall_ymax - d.grd_y_lo;
    // exact-zero contact shortcuts: clearance > 1000 * margin => exp(-1000) == +0.0
    const double clr = 1000.0 * w.contact_margin;
    d.contact_skip_d2 = (d.dist_min + clr) * (d.dist_min + clr) * (1.0 + 1e-12);
    d.wall_skip = clr;
    return d;
}

// The slab's regions in their order: the world and RNG state, the collector tail's scratch, then what each subsystem keeps.
void env_regions(fa_env *env, FaSlab &slab) {
    const size_t E = (size_t)env->cfg.num_envs, EN = E * env->N;
    FaState &s = env->s;
    slab.region(s.px, EN, true);
    slab.region(s.py, EN, true);
    slab.region(s.vx, EN, true);
    slab.region(s.vy, EN, true);
    slab.region(s.ang, EN, true);
    slab.region(s.prev, EN);
    slab.region(s.alive, EN);
    slab.region(s.tstep, E);
    slab.region(s.num_hit, EN, true);
    slab.region(s.num_was_hit, EN);
    slab.region(s.game_result, E * 3);
    slab.region(s.result_count, E * 3);
    slab.region(s.mt, E * FA_MT_N);
    slab.region(s.mt_pos, E);
    slab.region(s.reset_count, E);
    slab.region(s.ep_rew, EN, true);
    slab.region(s.ep_rew_sum, EN);
    slab.region(s.alive_end, EN);
    slab.region(env->adv_partial, (size_t)env->adv_blocks * FA_MAX_AGENTS * 2);
    slab.region(env->adv_stats, (size_t)FA_MAX_AGENTS * 5); // stats (3) + mean + std scratch
    fa_policy_regions(env, slab);
    fa_match_regions(env, slab);
    fa_behaviour_regions(env, slab);
}
} // namespace

extern "C" {

const char *fa_last_error(void) { return g_err.c_str(); }

int fa_config_default(fa_config *cfg) {
    if (!cfg) return fail(FA_ERR_INVALID, "fa_config_default: null cfg");
    std::memset(cfg, 0, sizeof(*cfg));
    cfg->num_envs = 1;
    cfg->num_guards = 3;
    cfg->num_attackers = 3;
    cfg->max_time_steps = 100; // arguments.py:24 --num-env-steps
    cfg->device_id = 0;
    cfg->rng_mode = FA_RNG_MT19937;
    cfg->base_seed = 0;
    cfg->env_offset = 0;
    cfg->rng_skip_doubles = -1;
    cfg->track_counters = 1;
    cfg->step_kernel = FA_KERNEL_AUTO;
    fa_world_consts &w = cfg->world;
    w.agent_size = 0.05;
    w.accel = 3;
    w.max_speed = 3;
    w.max_rot = 0.17;
    w.fort_dim = 0.15;
    w.door_x = 0;
    w.door_y = 0.8;
    w.dt = 0.1;
    w.damping = 0.25;
    w.contact_force = 1e+2;
    w.contact_margin = 1e-10;
    w.wall_xmin = -1;
    w.wall_xmax = 1;
    w.wall_ymin = -0.8;
    w.wall_ymax = 0.8;
    w.shoot_rad = 0.8;
    w.shoot_win = 3.141592653589793 / 4;
    return FA_OK;
}

int fa_create(const fa_config *cfg, fa_env **out) {
    if (!cfg || !out) return fail(FA_ERR_INVALID, "fa_create: null argument");
    const int N = cfg->num_guards + cfg->num_attackers;
    if (cfg->num_envs < 1) return fail(FA_ERR_INVALID, "fa_create: num_envs must be >= 1");
    if (cfg->num_guards < 1 || cfg->num_attackers < 1 || N > FA_MAX_AGENTS)
        return fail(FA_ERR_INVALID, "fa_create: need >=1 guard, >=1 attacker, <=16 agents");
    if (cfg->max_time_steps < 1) return fail(FA_ERR_INVALID, "fa_create: max_time_steps must be >= 1");
    if (cfg->rng_mode != FA_RNG_MT19937 && cfg->rng_mode != FA_RNG_PHILOX)
        return fail(FA_ERR_INVALID, "fa_create: unknown rng_mode");
    const bool experiment = cfg->step_kernel == FA_KERNEL_EXP_PAIRS || cfg->step_kernel == FA_KERNEL_EXP_CHAIN;
    if (experiment && !fa_step_experiments_linked())
        return fail(FA_ERR_INVALID, "fa_create: this library does not carry the experiment step kernels (build a variant: "
                                    "tools/build_variant.py experiments --add experiments/fa_step_experiments.hip)");
    if (!experiment && (cfg->step_kernel < FA_KERNEL_AUTO || cfg->step_kernel > FA_KERNEL_WAVES3))
        return fail(FA_ERR_INVALID, "fa_create: unknown step_kernel");
    if (cfg->step_kernel != FA_KERNEL_AUTO && cfg->step_kernel != FA_KERNEL_WAVES1 &&
        !((cfg->num_guards == 3 && cfg->num_attackers == 3) || (cfg->num_guards == 5 && cfg->num_attackers == 5)))
        return fail(FA_ERR_INVALID, "fa_create: the multi-wave step kernels exist for 3v3 and 5v5 only");
    if (cfg->step_kernel == FA_KERNEL_EXP_PAIRS && !(cfg->num_guards == 3 && cfg->num_attackers == 3))
        return fail(FA_ERR_INVALID, "fa_create: the pair-per-lane step kernel exists for 3v3 only");
    if (!(cfg->world.contact_margin > 0) || !(cfg->world.agent_size > 0))
        return fail(FA_ERR_INVALID, "fa_create: contact_margin and agent_size must be > 0");
    int ndev = 0;
    FA_HIP(hipGetDeviceCount(&ndev));
    if (cfg->device_id < 0 || cfg->device_id >= ndev) return fail(FA_ERR_INVALID, "fa_create: bad device_id");
    DeviceGuard guard(cfg->device_id);

    fa_env *env = new fa_env();
    std::memset(static_cast<void *>(env), 0, sizeof(*env));
    env->cfg = *cfg;
    env->N = N;
    if (env->cfg.rng_skip_doubles < 0) env->cfg.rng_skip_doubles = 2 * N;
    env->c = derive(cfg->world);
    env->adv_blocks = 1024;

    const size_t EN = (size_t)cfg->num_envs * N;
    FaSlab slab = {nullptr, 0}; // sizing pass
    env_regions(env, slab);
    env->slab_bytes = slab.bytes;
    hipError_t he = hipMalloc(&env->slab, env->slab_bytes);
    if (he != hipSuccess) {
        delete env;
        return fail(FA_ERR_HIP, std::string("hipMalloc: ") + hipGetErrorString(he));
    }
    slab = {static_cast<char *>(env->slab), 0}; // placing pass
    env_regions(env, slab);

    // construction state (core.py:102-104): alive, prevDist None (NaN); positions are
    // defined by the first reset.
    he = hipMemset(env->slab, 0, env->slab_bytes);
    if (he == hipSuccess) he = hipMemset(env->s.alive, 1, EN);
    if (he == hipSuccess) {
        std::vector<double> nan(EN, std::nan(""));
        he = hipMemcpy(env->s.prev, nan.data(), EN * sizeof(double), hipMemcpyHostToDevice);
    }
    if (he == hipSuccess)
        he = fa_launch_seed(env->s, cfg->num_envs, cfg->base_seed, cfg->env_offset,
                            2 * env->cfg.rng_skip_doubles, nullptr);
    if (he == hipSuccess) he = hipDeviceSynchronize();
    if (he != hipSuccess) {
        (void)hipFree(env->slab);
        delete env;
        return fail(FA_ERR_HIP, std::string("fa_create init: ") + hipGetErrorString(he));
    }
    *out = env;
    return FA_OK;
}

void fa_destroy(fa_env *env) {
    if (!env) return;
    DeviceGuard guard(env->cfg.device_id);
    (void)hipFree(env->slab);
    delete env;
}

int fa_num_agents(const fa_env *env) { return env ? env->N : FA_ERR_INVALID; }
int fa_num_envs(const fa_env *env) { return env ? env->cfg.num_envs : FA_ERR_INVALID; }

int fa_reset(fa_env *env, const uint8_t *env_mask, float *obs_f32, double *obs_f64, void *stream) {
    FA_ENTER(env, "fa_reset", false);
    FaStepArgs a = base_args(env);
    a.reset_mask = env_mask;
    a.obs32 = obs_f32;
    a.obs64 = obs_f64;
    FA_HIP(fa_launch_reset(a, static_cast<hipStream_t>(stream)));
    return FA_OK;
}

int fa_step(fa_env *env, const fa_step_io *io, void *stream) {
    FA_ENTER(env, "fa_step", false, io);
    if (!io->actions) return fail(FA_ERR_INVALID, "fa_step: actions is null");
    FaStepArgs a = base_args(env);
    a.actions = io->actions;
    a.as_e = io->act_stride_env;
    a.as_i = io->act_stride_agent;
    a.as_t = io->act_stride_step;
    a.nsteps = io->num_steps > 1 ? io->num_steps : 1;
    a.obs32 = io->obs_f32;
    a.rew32 = io->reward_f32;
    a.mask32 = io->mask_f32;
    a.done = io->done;
    a.obs64 = io->obs_f64;
    a.rew64 = io->reward_f64;
    a.hit = io->hit;
    a.was_hit = io->was_hit;
    a.auto_reset = io->auto_reset;
    FA_HIP(fa_launch_step(a, static_cast<hipStream_t>(stream)));
    return FA_OK;
}

int fa_set_reset_choice(fa_env *env, int32_t k, int32_t *choice_out) {
    if (int rc = fa_enter(env, "fa_set_reset_choice", false)) return rc;
    if (k < 0 || (k > 0 && !choice_out)) return fail(FA_ERR_INVALID, "fa_set_reset_choice: k >= 0, and k > 0 needs choice_out");
    env->choice_k = k;
    env->choice_out = k > 0 ? choice_out : nullptr;
    return FA_OK;
}

int fa_bind_storage(fa_env *env, const fa_storage *st) {
    if (int rc = fa_enter(env, "fa_bind_storage", false, st)) return rc;
    if (st->num_steps < 1) return fail(FA_ERR_INVALID, "fa_bind_storage: num_steps must be >= 1");
    if (!st->obs || !st->rewards || !st->value_preds || !st->returns || !st->actions || !st->masks ||
        !st->done)
        return fail(FA_ERR_INVALID, "fa_bind_storage: obs/rewards/value_preds/returns/actions/masks/done required");
    env->st = *st;
    env->bound = true;
    return FA_OK;
}

int fa_collect_step(fa_env *env, int32_t step, int32_t auto_reset, void *stream) {
    return fa_collect_rollout(env, step, 1, auto_reset, stream);
}

int fa_collect_rollout(fa_env *env, int32_t step, int32_t num_steps, int32_t auto_reset, void *stream) {
    FA_ENTER(env, "fa_collect_rollout", true);
    const fa_storage &st = env->st;
    if (step < 0 || num_steps < 1 || step + num_steps > st.num_steps)
        return fail(FA_ERR_INVALID, "fa_collect_rollout: step range outside the bound storage");
    const size_t EN = (size_t)env->cfg.num_envs * env->N;
    FaStepArgs a = base_args(env);
    a.actions = st.actions + (size_t)step * EN;
    a.as_e = env->N;
    a.as_i = 1;
    a.as_t = (int64_t)EN;
    a.nsteps = num_steps;
    a.obs32 = st.obs + (size_t)(step + 1) * EN * FA_OBS_DIM;
    a.rew32 = st.rewards + (size_t)step * EN;
    a.mask32 = st.masks + (size_t)(step + 1) * EN;
    a.done = st.done + (size_t)step * env->cfg.num_envs;
    a.auto_reset = auto_reset;
    FA_HIP(fa_launch_step(a, static_cast<hipStream_t>(stream)));
    return FA_OK;
}

int fa_collect_reset(fa_env *env, void *stream) {
    FA_ENTER(env, "fa_collect_reset", true);
    hipStream_t s = static_cast<hipStream_t>(stream);
    FaStepArgs a = base_args(env);
    a.obs32 = env->st.obs;
    FA_HIP(fa_launch_reset(a, s));
    // masks[0] = 1 (every agent alive after a reset): float 1.0f fill
    const size_t EN = (size_t)env->cfg.num_envs * env->N;
    FA_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(env->st.masks), 0x3f800000, EN, s));
    return FA_OK;
}

int fa_after_update(fa_env *env, void *stream) {
    FA_ENTER(env, "fa_after_update", true);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const fa_storage &st = env->st;
    const size_t EN = (size_t)env->cfg.num_envs * env->N, T = (size_t)st.num_steps;
    // storage.py:52-56: obs[0] = obs[-1]; obs[1:] = 0; hidden[0] = hidden[-1]; masks[0] = masks[-1]
    FA_HIP(hipMemcpyAsync(st.obs, st.obs + T * EN * FA_OBS_DIM, EN * FA_OBS_DIM * sizeof(float),
                          hipMemcpyDeviceToDevice, s));
    FA_HIP(hipMemsetAsync(st.obs + EN * FA_OBS_DIM, 0, T * EN * FA_OBS_DIM * sizeof(float), s));
    if (st.recurrent_hidden_states)
        FA_HIP(hipMemcpyAsync(st.recurrent_hidden_states, st.recurrent_hidden_states + T * EN,
                              EN * sizeof(float), hipMemcpyDeviceToDevice, s));
    FA_HIP(hipMemcpyAsync(st.masks, st.masks + T * EN, EN * sizeof(float), hipMemcpyDeviceToDevice, s));
    return FA_OK;
}

int fa_get_state(fa_env *env, const fa_state_host *o) {
    FA_ENTER(env, "fa_get_state", false, o);
    FA_HIP(hipDeviceSynchronize());
    const size_t E = (size_t)env->cfg.num_envs, EN = E * env->N;
    const FaState &s = env->s;
#define FA_D2H(dst, src, bytes) \
    if (dst) FA_HIP(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost))
    FA_D2H(o->pos_x, s.px, EN * 8);
    FA_D2H(o->pos_y, s.py, EN * 8);
    FA_D2H(o->vel_x, s.vx, EN * 8);
    FA_D2H(o->vel_y, s.vy, EN * 8);
    FA_D2H(o->ang, s.ang, EN * 8);
    FA_D2H(o->prev_dist, s.prev, EN * 8);
    FA_D2H(o->alive, s.alive, EN);
    FA_D2H(o->time_step, s.tstep, E * 4);
    FA_D2H(o->num_hit, s.num_hit, EN * 4);
    FA_D2H(o->num_was_hit, s.num_was_hit, EN * 4);
    FA_D2H(o->game_result, s.game_result, E * 3);
    FA_D2H(o->episode_reward_sum, s.ep_rew_sum, EN * 8);
#undef FA_D2H
    if (o->alive_at_end) {
        std::vector<uint32_t> ae(EN);
        FA_HIP(hipMemcpy(ae.data(), s.alive_end, EN * 4, hipMemcpyDeviceToHost));
        for (size_t k = 0; k < EN; ++k) o->alive_at_end[k] = (int64_t)ae[k];
    }
    if (o->result_count) {
        std::vector<uint32_t> rc(E * 3);
        FA_HIP(hipMemcpy(rc.data(), s.result_count, E * 3 * 4, hipMemcpyDeviceToHost));
        for (size_t k = 0; k < E * 3; ++k) o->result_count[k] = (int64_t)rc[k];
    }
    return FA_OK;
}

int fa_set_state(fa_env *env, const fa_state_host *in) {
    FA_ENTER(env, "fa_set_state", false, in);
    FA_HIP(hipDeviceSynchronize());
    const size_t E = (size_t)env->cfg.num_envs, EN = E * env->N;
    const FaState &s = env->s;
#define FA_H2D(dst, src, bytes) \
    if (src) FA_HIP(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice))
    FA_H2D(s.px, in->pos_x, EN * 8);
    FA_H2D(s.py, in->pos_y, EN * 8);
    FA_H2D(s.vx, in->vel_x, EN * 8);
    FA_H2D(s.vy, in->vel_y, EN * 8);
    FA_H2D(s.ang, in->ang, EN * 8);
    FA_H2D(s.prev, in->prev_dist, EN * 8);
    FA_H2D(s.alive, in->alive, EN);
    FA_H2D(s.tstep, in->time_step, E * 4);
    FA_H2D(s.num_hit, in->num_hit, EN * 4);
    FA_H2D(s.num_was_hit, in->num_was_hit, EN * 4);
    FA_H2D(s.game_result, in->game_result, E * 3);
#undef FA_H2D
    return FA_OK;
}

int fa_selftest_math(fa_env *env, uint64_t samples, uint64_t seed, uint64_t *mismatch_host) {
    FA_ENTER(env, "fa_selftest_math", false, mismatch_host);
    unsigned long long *d = reinterpret_cast<unsigned long long *>(env->adv_partial); // scratch
    FA_HIP(hipDeviceSynchronize());
    FA_HIP(hipMemset(d, 0, 24));
    const unsigned long long per = samples / (1024ull * 256ull) + 1ull;
    FA_HIP(fa_launch_selftest(per, seed, d, nullptr));
    FA_HIP(hipMemcpy(mismatch_host, d, 24, hipMemcpyDeviceToHost));
    return FA_OK;
}

const char *fa_step_variant(fa_env *env, int32_t num_steps) {
    if (!env) return "";
    return fa_step_variant_name(env->cfg.num_guards, env->cfg.num_attackers, env->cfg.num_envs, num_steps,
                                env->cfg.step_kernel, env->choice_k > 0);
}

int fa_rng_peek(fa_env *env, int32_t e, int32_t count, double *out_host) {
    FA_ENTER(env, "fa_rng_peek", false, out_host);
    if (e < 0 || e >= env->cfg.num_envs || count < 0) return fail(FA_ERR_INVALID, "fa_rng_peek: bad index");
    if (env->cfg.rng_mode != FA_RNG_MT19937) return fail(FA_ERR_STATE, "fa_rng_peek: MT19937 mode only");
    FA_HIP(hipDeviceSynchronize());
    std::vector<uint32_t> mt(FA_MT_N);
    int32_t pos = 0;
    FA_HIP(hipMemcpy(mt.data(), env->s.mt + (size_t)e * FA_MT_N, FA_MT_N * 4, hipMemcpyDeviceToHost));
    FA_HIP(hipMemcpy(&pos, env->s.mt_pos + e, 4, hipMemcpyDeviceToHost));
    auto next = [&]() {
        const int n1 = pos + 1 >= FA_MT_N ? pos + 1 - FA_MT_N : pos + 1;
        const int nm = pos + FA_MT_M >= FA_MT_N ? pos + FA_MT_M - FA_MT_N : pos + FA_MT_M;
        uint32_t y = (mt[pos] & 0x80000000u) | (mt[n1] & 0x7fffffffu);
        uint32_t nw = mt[nm] ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
        mt[pos] = nw;
        pos = n1;
        nw ^= (nw >> 11);
        nw ^= (nw << 7) & 0x9d2c5680u;
        nw ^= (nw << 15) & 0xefc60000u;
        nw ^= (nw >> 18);
        return nw;
    };
    for (int k = 0; k < count; ++k) {
        uint32_t a = next() >> 5, b = next() >> 6;
        out_host[k] = (a * 67108864.0 + b) / 9007199254740992.0;
    }
    return FA_OK;
}

} // extern "C"
