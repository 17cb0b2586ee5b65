// fa_api.hip -- host side of the C ABI declared in include/fortattack.h.
// Owns the fp64 SoA world state + RNG state in HBM; everything else belongs to the caller.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "fa_device.h"
#include "fa_collect.h"
#include "experiments/fa_step_experiments.h"
#include "fa_policy.h"
#include "fa_match.h"
#include "fa_render.h"
#include "fa_behaviour.h"
#include "fa_train.h"
#include "fortattack.h"

hipError_t fa_launch_step(const FaStepArgs &a, hipStream_t st);
hipError_t fa_launch_reset(const FaStepArgs &a, hipStream_t st);
const char *fa_step_variant_name(int G, int A, int E, int nsteps, int step_kernel, bool choice);
int fa_step_experiments_linked(); // fa_step_classic.hip: 1 in a variant library that carries csrc/experiments/
hipError_t fa_launch_seed(const FaState &s, int E, uint64_t base_seed, int64_t env_offset, int skip_words,
                          hipStream_t st);
hipError_t fa_launch_selftest(unsigned long long n_per_thread, unsigned long long seed, unsigned long long *mismatch,
                              hipStream_t st);
hipError_t fa_launch_attend(int width, bool backward, const float *g, const float *keys, float *out, float *attn,
                            const float *dout, float *dg, float *dkeys, int B, int n, int nk, int skip_self, hipStream_t st);

static thread_local std::string g_err;

static int fail(int code, const std::string &msg) {
    g_err = msg;
    return code;
}
int fa_api_fail(int code, const std::string &msg) { return fail(code, msg); } // for the other translation units
#define FA_HIP(expr)                                                                          \
    do {                                                                                      \
        hipError_t _e = (expr);                                                               \
        if (_e != hipSuccess)                                                                 \
            return fail(FA_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));       \
    } while (0)

struct fa_env {
    fa_config cfg;
    int N;
    FaDerived c;
    FaState s;
    void *slab;
    size_t slab_bytes;
    fa_storage st;
    bool bound;
    double *adv_partial; // [ADV_BLOCKS][N]
    double *adv_stats;   // [N][3] scratch of fa_adv_mean_std
    int adv_blocks;
    int choice_k;        // fa_set_reset_choice
    int32_t *choice_out;
    int32_t *grp_env_list[2], *grp_tile_strategy[2]; // fused policy with a guard [0] / attacker [1] ensemble: envs grouped by strategy
    int grp_tiles_max;
    // match bookkeeping (fa_match.hip): baseline + latched counters per env, see fa_match_begin
    FaMatch match;
    // behaviour maps (fa_behaviour.hip): per-env episode counters + the launch plan of fa_behaviour_begin
    FaBehaviour beh;
};

namespace {
struct DeviceGuard {
    int prev;
    bool changed;
    explicit DeviceGuard(int dev) : prev(-1), changed(false) {
        if (hipGetDevice(&prev) == hipSuccess && prev != dev) changed = hipSetDevice(dev) == hipSuccess;
    }
    ~DeviceGuard() {
        if (changed) (void)hipSetDevice(prev);
    }
};

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

size_t align_up(size_t x) { return (x + 255) & ~(size_t)255; }

FaStepArgs base_args(const fa_env *env) {
    FaStepArgs a;
    std::memset(&a, 0, sizeof(a));
    a.s = env->s;
    a.E = env->cfg.num_envs;
    a.G = env->cfg.num_guards;
    a.A = env->cfg.num_attackers;
    a.max_t = env->cfg.max_time_steps;
    a.rng_mode = env->cfg.rng_mode;
    a.track_counters = env->cfg.track_counters;
    a.step_kernel = env->cfg.step_kernel;
    a.choice_k = env->choice_k;
    a.choice_out = env->choice_out;
    a.seed = env->cfg.base_seed;
    a.env_offset = env->cfg.env_offset;
    a.c = env->c;
    a.nsteps = 1;
    return a;
}

// The bound storage as the collector tail's launchers take it (fa_collect.h); gamma, gamma * tau rounded to float32 once.
FaTailArgs tail_args(const fa_env *env, double gamma = 0.0, double tau = 0.0) {
    const fa_storage &st = env->st;
    FaTailArgs a;
    a.rewards = st.rewards;
    a.value_preds = st.value_preds;
    a.masks = st.masks;
    a.returns = st.returns;
    a.done = st.done;
    a.T = st.num_steps;
    a.E = env->cfg.num_envs;
    a.N = env->N;
    a.g32 = (float)gamma;
    a.gt32 = (float)(gamma * tau);
    return a;
}

// How the tail is launched for the bound storage: the workgroup count of every grid that depends on the shape alone.
struct FaTailPlan {
    int fused;   // fa_gae_mom_kernel's workgroups; 0: the shape is beyond the fused scan, the separate kernels serve
    int sweep;   // fa_adv_onepass[_vec]_kernel
    int twopass; // fa_adv_partial[_vec]_kernel
};
FaTailPlan tail_plan(const fa_env *env, const FaTailArgs &a) {
    FaTailPlan p;
    p.fused = fa_gae_mom_blocks(a.T, a.E, a.N, (long long)env->adv_blocks * FA_MAX_AGENTS * 2);
    // a lane takes 2 rows x 4 per trip: one workgroup per 2048 rows, at most two per CU (512: what the fold takes)
    long long want = (a.rows() + 2047) / 2048;
    p.sweep = (int)(want < 512 ? (want < 1 ? 1 : want) : 512);
    // a row per lane and trip, as many workgroups as adv_partial holds
    want = (a.rows() + 255) / 256;
    p.twopass = (int)(want < env->adv_blocks ? want : env->adv_blocks);
    return p;
}

// The scan and the {S, Q} partials of the advantage moments in env->adv_partial: the fused scan where it serves, else fa_gae
// and the one-pass sweep.  Returns where the partials come from and how many workgroups wrote them; the caller folds them
// (fa_launch_gae_mom_final) or folds and normalises (fa_launch_gae_mom_norm).
struct FaTailPartials {
    hipError_t err;
    FaStatSource src;
    int count;
};
FaTailPartials tail_scan_partials(const fa_env *env, const FaTailArgs &a, hipStream_t s) {
    const FaTailPlan p = tail_plan(env, a);
    if (p.fused) return {fa_launch_gae_mom(a, env->adv_partial, p.fused, s), FA_STATS_SCAN_PARTIALS, p.fused};
    hipError_t e = fa_launch_gae(a, s);
    if (e == hipSuccess) e = fa_launch_adv_onepass(a, env->adv_partial, p.sweep, s);
    return {e, FA_STATS_SWEEP_PARTIALS, p.sweep};
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

    const size_t E = (size_t)cfg->num_envs, EN = E * N;
    size_t off = 0;
    auto carve = [&](size_t bytes) { size_t o = off; off = align_up(off + bytes); return o; };
    const size_t o_f64 = carve(6 * EN * sizeof(double));
    const size_t o_alive = carve(EN);
    const size_t o_tstep = carve(E * sizeof(int32_t));
    const size_t o_nh = carve(2 * EN * sizeof(int32_t));
    const size_t o_gr = carve(E * 3);
    const size_t o_rc = carve(E * 3 * sizeof(uint32_t));
    const size_t o_mt = carve(E * FA_MT_N * sizeof(uint32_t));
    const size_t o_pos = carve(E * sizeof(int32_t));
    const size_t o_cnt = carve(E * sizeof(uint32_t));
    const size_t o_epr = carve(2 * EN * sizeof(double));
    const size_t o_ale = carve(EN * sizeof(uint32_t));
    const size_t o_adv = carve((size_t)env->adv_blocks * FA_MAX_AGENTS * 2 * sizeof(double));
    const size_t o_advs = carve((size_t)FA_MAX_AGENTS * 5 * sizeof(double)); // stats (3) + mean + std scratch
    const bool fused_ok = cfg->num_guards <= FA_POLICY_MAX_TEAM && cfg->num_attackers <= FA_POLICY_MAX_TEAM;
    // sized for the smallest tile the policy kernel may choose (64 rows), slots counted at the largest (96)
    const int n_max = cfg->num_guards > cfg->num_attackers ? cfg->num_guards : cfg->num_attackers;
    const int tile_envs = fused_ok ? 64 / n_max : 1;
    env->grp_tiles_max = fused_ok ? (cfg->num_envs + tile_envs - 1) / tile_envs + FA_POLICY_MAX_POOL : 0;
    size_t o_gel[2], o_gts[2];
    for (int t = 0; t < 2; ++t) {
        o_gel[t] = carve((size_t)env->grp_tiles_max * (FA_POLICY_ROWS / n_max + 1) * sizeof(int32_t));
        o_gts[t] = carve((size_t)env->grp_tiles_max * sizeof(int32_t));
    }
    // match bookkeeping: baseline and latched copies of the three counters, the per-env cell / latch flag, two scalars
    const bool match_ok = cfg->track_counters != 0;
    const size_t o_mrc = carve(match_ok ? 2 * E * 3 * sizeof(uint32_t) : 0);
    const size_t o_mae = carve(match_ok ? 2 * EN * sizeof(uint32_t) : 0);
    const size_t o_mrw = carve(match_ok ? 2 * EN * sizeof(double) : 0);
    const size_t o_mce = carve(match_ok ? 2 * E * sizeof(int32_t) : 0);
    const size_t o_msc = carve(2 * sizeof(int32_t));
    // behaviour maps: ep_count, ep_t, the env list (E each) and the slice table
    const int beh_slices = fa_behaviour_max_slices(cfg->num_envs);
    const size_t o_beh = carve(3 * E * sizeof(int32_t));
    const size_t o_bsl = carve((size_t)beh_slices * 4 * sizeof(int32_t));
    env->slab_bytes = off;
    hipError_t he = hipMalloc(&env->slab, env->slab_bytes);
    if (he != hipSuccess) {
        delete env;
        return fail(FA_ERR_HIP, std::string("hipMalloc: ") + hipGetErrorString(he));
    }
    char *b = static_cast<char *>(env->slab);
    double *f = reinterpret_cast<double *>(b + o_f64);
    env->s.px = f;
    env->s.py = f + EN;
    env->s.vx = f + 2 * EN;
    env->s.vy = f + 3 * EN;
    env->s.ang = f + 4 * EN;
    env->s.prev = f + 5 * EN;
    env->s.alive = reinterpret_cast<uint8_t *>(b + o_alive);
    env->s.tstep = reinterpret_cast<int32_t *>(b + o_tstep);
    env->s.num_hit = reinterpret_cast<int32_t *>(b + o_nh);
    env->s.num_was_hit = env->s.num_hit + EN;
    env->s.game_result = reinterpret_cast<uint8_t *>(b + o_gr);
    env->s.result_count = reinterpret_cast<uint32_t *>(b + o_rc);
    env->s.mt = reinterpret_cast<uint32_t *>(b + o_mt);
    env->s.mt_pos = reinterpret_cast<int32_t *>(b + o_pos);
    env->s.reset_count = reinterpret_cast<uint32_t *>(b + o_cnt);
    env->s.ep_rew = reinterpret_cast<double *>(b + o_epr);
    env->s.ep_rew_sum = env->s.ep_rew + EN;
    env->s.alive_end = reinterpret_cast<uint32_t *>(b + o_ale);
    env->adv_partial = reinterpret_cast<double *>(b + o_adv);
    env->adv_stats = reinterpret_cast<double *>(b + o_advs);
    for (int t = 0; t < 2; ++t) {
        env->grp_env_list[t] = reinterpret_cast<int32_t *>(b + o_gel[t]);
        env->grp_tile_strategy[t] = reinterpret_cast<int32_t *>(b + o_gts[t]);
    }
    if (match_ok) {
        FaMatch &m = env->match;
        m.base_rc = reinterpret_cast<uint32_t *>(b + o_mrc);
        m.lat_rc = m.base_rc + E * 3;
        m.base_alive = reinterpret_cast<uint32_t *>(b + o_mae);
        m.lat_alive = m.base_alive + EN;
        m.base_rew = reinterpret_cast<double *>(b + o_mrw);
        m.lat_rew = m.base_rew + EN;
        m.cell = reinterpret_cast<int32_t *>(b + o_mce);
        m.latched = m.cell + E;
        m.remaining = reinterpret_cast<int32_t *>(b + o_msc);
        m.overrun = m.remaining + 1;
    }
    env->beh.ep_count = reinterpret_cast<int32_t *>(b + o_beh);
    env->beh.ep_t = env->beh.ep_count + E;
    env->beh.env_list = env->beh.ep_t + E;
    env->beh.slices = reinterpret_cast<int32_t *>(b + o_bsl);
    env->beh.max_slices = beh_slices;

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
    if (!env) return fail(FA_ERR_INVALID, "fa_reset: null env");
    DeviceGuard guard(env->cfg.device_id);
    FaStepArgs a = base_args(env);
    a.reset_mask = env_mask;
    a.obs32 = obs_f32;
    a.obs64 = obs_f64;
    FA_HIP(fa_launch_reset(a, static_cast<hipStream_t>(stream)));
    return FA_OK;
}

int fa_step(fa_env *env, const fa_step_io *io, void *stream) {
    if (!env || !io) return fail(FA_ERR_INVALID, "fa_step: null argument");
    if (!io->actions) return fail(FA_ERR_INVALID, "fa_step: actions is null");
    DeviceGuard guard(env->cfg.device_id);
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
    if (!env) return fail(FA_ERR_INVALID, "fa_set_reset_choice: null env");
    if (k < 0 || (k > 0 && !choice_out)) return fail(FA_ERR_INVALID, "fa_set_reset_choice: k >= 0, and k > 0 needs choice_out");
    env->choice_k = k;
    env->choice_out = k > 0 ? choice_out : nullptr;
    return FA_OK;
}

int fa_bind_storage(fa_env *env, const fa_storage *st) {
    if (!env || !st) return fail(FA_ERR_INVALID, "fa_bind_storage: null argument");
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
    if (!env) return fail(FA_ERR_INVALID, "fa_collect_rollout: null env");
    if (!env->bound) return fail(FA_ERR_STATE, "fa_collect_rollout: no storage bound");
    const fa_storage &st = env->st;
    if (step < 0 || num_steps < 1 || step + num_steps > st.num_steps)
        return fail(FA_ERR_INVALID, "fa_collect_rollout: step range outside the bound storage");
    DeviceGuard guard(env->cfg.device_id);
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
    if (!env) return fail(FA_ERR_INVALID, "fa_collect_reset: null env");
    if (!env->bound) return fail(FA_ERR_STATE, "fa_collect_reset: no storage bound");
    DeviceGuard guard(env->cfg.device_id);
    hipStream_t s = static_cast<hipStream_t>(stream);
    FaStepArgs a = base_args(env);
    a.obs32 = env->st.obs;
    FA_HIP(fa_launch_reset(a, s));
    // masks[0] = 1 (every agent alive after a reset): float 1.0f fill
    const size_t EN = (size_t)env->cfg.num_envs * env->N;
    FA_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(env->st.masks), 0x3f800000, EN, s));
    return FA_OK;
}

int fa_gae(fa_env *env, double gamma, double tau, void *stream) {
    if (!env) return fail(FA_ERR_INVALID, "fa_gae: null env");
    if (!env->bound) return fail(FA_ERR_STATE, "fa_gae: no storage bound");
    DeviceGuard guard(env->cfg.device_id);
    FA_HIP(fa_launch_gae(tail_args(env, gamma, tau), static_cast<hipStream_t>(stream)));
    return FA_OK;
}

int fa_gae_moments(fa_env *env, double gamma, double tau, double *moments_out, double *mean_out, double *std_out,
                   void *stream) {
    if (!env) return fail(FA_ERR_INVALID, "fa_gae_moments: null env");
    if (!env->bound) return fail(FA_ERR_STATE, "fa_gae_moments: no storage bound");
    DeviceGuard guard(env->cfg.device_id);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const FaTailArgs a = tail_args(env, gamma, tau);
    // scan + moment partials (two launches beyond the fused scan), then one workgroup folds them
    const FaTailPartials p = tail_scan_partials(env, a, s);
    FA_HIP(p.err);
    FA_HIP(fa_launch_gae_mom_final(a, p.src, env->adv_partial, p.count, moments_out, mean_out, std_out, s));
    return FA_OK;
}

int fa_gae_normalize(fa_env *env, double gamma, double tau, float *adv_out, double *moments_out, double *mean_out,
                     double *std_out, void *stream) {
    if (!env || !adv_out) return fail(FA_ERR_INVALID, "fa_gae_normalize: null argument");
    if (!env->bound) return fail(FA_ERR_STATE, "fa_gae_normalize: no storage bound");
    DeviceGuard guard(env->cfg.device_id);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const FaTailArgs a = tail_args(env, gamma, tau);
    // scan + moment partials; fold + normalisation by every workgroup -- two launches, three beyond the fused scan (instead
    // of four), nothing dirty left behind the last one
    const FaTailPartials p = tail_scan_partials(env, a, s);
    FA_HIP(p.err);
    FA_HIP(fa_launch_gae_mom_norm(a, p.src, env->adv_partial, p.count, adv_out, moments_out, mean_out, std_out, s));
    return FA_OK;
}

int fa_adv_moments_onepass(fa_env *env, double *moments_out, double *mean_out, double *std_out, void *stream) {
    if (!env) return fail(FA_ERR_INVALID, "fa_adv_moments_onepass: null env");
    if (!env->bound) return fail(FA_ERR_STATE, "fa_adv_moments_onepass: no storage bound");
    DeviceGuard guard(env->cfg.device_id);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const FaTailArgs a = tail_args(env);
    const int nblocks = tail_plan(env, a).sweep;
    FA_HIP(fa_launch_adv_onepass(a, env->adv_partial, nblocks, s));
    FA_HIP(fa_launch_gae_mom_final(a, FA_STATS_SWEEP_PARTIALS, env->adv_partial, nblocks, moments_out, mean_out,
                                   std_out, s));
    return FA_OK;
}

int fa_adv_stats(fa_env *env, int32_t pass, const double *mean, double *stats, void *stream) {
    if (!env || !stats) return fail(FA_ERR_INVALID, "fa_adv_stats: null argument");
    if (!env->bound) return fail(FA_ERR_STATE, "fa_adv_stats: no storage bound");
    if (pass != 0 && pass != 1) return fail(FA_ERR_INVALID, "fa_adv_stats: pass must be 0 or 1");
    if (pass == 1 && !mean) return fail(FA_ERR_INVALID, "fa_adv_stats: pass 1 needs mean");
    DeviceGuard guard(env->cfg.device_id);
    const FaTailArgs a = tail_args(env);
    FA_HIP(fa_launch_adv_stats(pass, a.returns, a.value_preds, mean, a.rows(), a.N, env->adv_partial,
                               tail_plan(env, a).twopass, stats, nullptr, static_cast<hipStream_t>(stream)));
    return FA_OK;
}

int fa_adv_mean_std(fa_env *env, double *mean_out, double *std_out, void *stream) {
    if (!env || !mean_out || !std_out) return fail(FA_ERR_INVALID, "fa_adv_mean_std: null argument");
    if (!env->bound) return fail(FA_ERR_STATE, "fa_adv_mean_std: no storage bound");
    DeviceGuard guard(env->cfg.device_id);
    const FaTailArgs a = tail_args(env);
    const int nblocks = tail_plan(env, a).twopass;
    hipStream_t s = static_cast<hipStream_t>(stream);
    FA_HIP(fa_launch_adv_stats(0, a.returns, a.value_preds, nullptr, a.rows(), a.N, env->adv_partial, nblocks,
                               env->adv_stats, mean_out, s));
    FA_HIP(fa_launch_adv_stats(1, a.returns, a.value_preds, mean_out, a.rows(), a.N, env->adv_partial, nblocks,
                               env->adv_stats, std_out, s));
    return FA_OK;
}

int fa_adv_moments(fa_env *env, double *moments_out, void *stream) {
    if (!env || !moments_out) return fail(FA_ERR_INVALID, "fa_adv_moments: null argument");
    if (!env->bound) return fail(FA_ERR_STATE, "fa_adv_moments: no storage bound");
    DeviceGuard guard(env->cfg.device_id);
    const FaTailArgs a = tail_args(env);
    const int nblocks = tail_plan(env, a).twopass;
    hipStream_t s = static_cast<hipStream_t>(stream);
    double *mean = env->adv_stats + 3 * FA_MAX_AGENTS; // scratch: local mean
    FA_HIP(fa_launch_adv_stats(0, a.returns, a.value_preds, nullptr, a.rows(), a.N, env->adv_partial, nblocks,
                               moments_out, mean, s));
    FA_HIP(fa_launch_adv_stats(1, a.returns, a.value_preds, mean, a.rows(), a.N, env->adv_partial, nblocks,
                               moments_out, nullptr, s));
    FA_HIP(fa_launch_adv_moments_fix(moments_out, a.N, s));
    return FA_OK;
}

int fa_adv_merge(fa_env *env, const double *gathered, int32_t world, double *mean_out, double *std_out,
                 void *stream) {
    if (!env || !gathered || !mean_out || !std_out) return fail(FA_ERR_INVALID, "fa_adv_merge: null argument");
    if (world < 1) return fail(FA_ERR_INVALID, "fa_adv_merge: world must be >= 1");
    DeviceGuard guard(env->cfg.device_id);
    FA_HIP(fa_launch_adv_merge(gathered, world, env->N, mean_out, std_out, static_cast<hipStream_t>(stream)));
    return FA_OK;
}

int fa_adv_merge_normalize(fa_env *env, const double *gathered, int32_t world, float *adv_out, double *mean_out, double *std_out,
                           void *stream) {
    if (!env || !gathered || !adv_out) return fail(FA_ERR_INVALID, "fa_adv_merge_normalize: null argument");
    if (world < 1) return fail(FA_ERR_INVALID, "fa_adv_merge_normalize: world must be >= 1");
    if (!env->bound) return fail(FA_ERR_STATE, "fa_adv_merge_normalize: no storage bound");
    DeviceGuard guard(env->cfg.device_id);
    FA_HIP(fa_launch_gae_mom_norm(tail_args(env), FA_STATS_GATHERED_RANKS, gathered, world, adv_out, nullptr, mean_out,
                                  std_out, static_cast<hipStream_t>(stream)));
    return FA_OK;
}

int fa_adv_normalize(fa_env *env, const double *mean, const double *std_, float *adv_out, void *stream) {
    if (!env || !mean || !std_ || !adv_out) return fail(FA_ERR_INVALID, "fa_adv_normalize: null argument");
    if (!env->bound) return fail(FA_ERR_STATE, "fa_adv_normalize: no storage bound");
    DeviceGuard guard(env->cfg.device_id);
    FA_HIP(fa_launch_adv_norm(tail_args(env), mean, std_, adv_out, static_cast<hipStream_t>(stream)));
    return FA_OK;
}

int fa_after_update(fa_env *env, void *stream) {
    if (!env) return fail(FA_ERR_INVALID, "fa_after_update: null env");
    if (!env->bound) return fail(FA_ERR_STATE, "fa_after_update: no storage bound");
    DeviceGuard guard(env->cfg.device_id);
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

static int policy_launch(fa_env *env, const float *obs, const float *wg, const float *wa, float *value, int64_t *action,
                         float *logp, const int64_t *counter, uint64_t seed, int step, int deterministic, int value_only,
                         const float *pool, int pool_size, const int32_t *env_strategy, const float *guard_pool,
                         int guard_pool_size, const int32_t *env_guard_strategy, float *const *team_attn,
                         float *const *opp_attn, void *stream, const char *who) {
    if (!obs || (!wg && guard_pool_size <= 0) || (!wa && pool_size <= 0))
        return fail(FA_ERR_INVALID, std::string(who) + ": obs and both teams' weight buffers are required");
    if (!value_only && (!action || !logp)) return fail(FA_ERR_INVALID, std::string(who) + ": action and log_prob are required");
    if (value_only && !value) return fail(FA_ERR_INVALID, std::string(who) + ": value_only needs value");
    if (env->cfg.num_guards > FA_POLICY_MAX_TEAM || env->cfg.num_attackers > FA_POLICY_MAX_TEAM)
        return fail(FA_ERR_INVALID, std::string(who) + ": teams of more than 8 agents are not supported by the fused policy");
    if (pool_size > 0 && (!pool || !env_strategy || pool_size > FA_POLICY_MAX_POOL))
        return fail(FA_ERR_INVALID, std::string(who) + ": an attacker pool needs weights, env_strategy and <= 64 strategies");
    if (guard_pool_size > 0 && (!guard_pool || !env_guard_strategy || guard_pool_size > FA_POLICY_MAX_POOL))
        return fail(FA_ERR_INVALID, std::string(who) + ": a guard pool needs guard_pool, env_guard_strategy and <= 64 strategies");
    DeviceGuard guard(env->cfg.device_id);
    hipStream_t s = static_cast<hipStream_t>(stream);
    FaPolicyArgs a;
    std::memset(&a, 0, sizeof(a));
    a.obs = obs;
    a.w[0] = wg;
    a.w[1] = wa;
    a.value = value;
    a.action = action;
    a.logp = logp;
    a.counter = counter;
    a.seed = seed;
    a.env_offset = env->cfg.env_offset;
    a.E = env->cfg.num_envs;
    a.G = env->cfg.num_guards;
    a.A = env->cfg.num_attackers;
    a.step = step;
    a.deterministic = deterministic;
    a.value_only = value_only;
    for (int t = 0; t < 2; ++t) { // attention export: any non-null pointer selects the exporting kernel
        a.team_attn[t] = team_attn[t];
        a.opp_attn[t] = opp_attn[t];
    }
    if (pool_size > 0 || guard_pool_size > 0) { // group each pooled team's envs into tiles of equal strategy, then one launch
        const int32_t *const strat[2] = {env_guard_strategy, env_strategy};
        const float *const pools[2] = {guard_pool, pool};
        const int sizes[2] = {guard_pool_size > 0 ? guard_pool_size : 0, pool_size > 0 ? pool_size : 0};
        FA_HIP(fa_launch_group_envs(strat, a.E, sizes, a.G, a.A, env->grp_env_list, env->grp_tile_strategy,
                                    env->grp_tiles_max, s));
        for (int t = 0; t < 2; ++t) {
            if (sizes[t] == 0) continue;
            a.pool[t] = pools[t];
            a.env_list[t] = env->grp_env_list[t];
            a.tile_strategy[t] = env->grp_tile_strategy[t];
        }
        a.tiles = env->grp_tiles_max;
    }
    FA_HIP(fa_launch_policy(a, s));
    return FA_OK;
}

int fa_policy_act(fa_env *env, const fa_policy_io *io, void *stream) {
    if (!env || !io) return fail(FA_ERR_INVALID, "fa_policy_act: null argument");
    return policy_launch(env, io->obs, io->weights[0], io->weights[1], io->value, io->action, io->log_prob, io->counter,
                         io->seed, io->step, io->deterministic, io->value_only, io->attacker_pool, io->pool_size,
                         io->env_strategy, io->guard_pool, io->guard_pool_size, io->env_guard_strategy, io->team_attn,
                         io->opp_attn, stream, "fa_policy_act");
}

int fa_collect_act(fa_env *env, int32_t step, const fa_policy_io *io, void *stream) {
    if (!env || !io) return fail(FA_ERR_INVALID, "fa_collect_act: null argument");
    if (!env->bound) return fail(FA_ERR_STATE, "fa_collect_act: no storage bound");
    const fa_storage &st = env->st;
    const int value_only = io->value_only;
    if (step < 0 || step > st.num_steps || (!value_only && step == st.num_steps))
        return fail(FA_ERR_INVALID, "fa_collect_act: step outside the bound storage");
    if (!value_only && !st.action_log_probs) return fail(FA_ERR_STATE, "fa_collect_act: storage has no action_log_probs");
    const size_t EN = (size_t)env->cfg.num_envs * env->N;
    return policy_launch(env, st.obs + (size_t)step * EN * FA_OBS_DIM, io->weights[0], io->weights[1],
                         st.value_preds + (size_t)step * EN, value_only ? nullptr : st.actions + (size_t)step * EN,
                         value_only ? nullptr : st.action_log_probs + (size_t)step * EN, io->counter, io->seed, step,
                         io->deterministic, value_only, io->attacker_pool, io->pool_size, io->env_strategy, io->guard_pool,
                         io->guard_pool_size, io->env_guard_strategy, io->team_attn, io->opp_attn, stream, "fa_collect_act");
}

// ---- match bookkeeping (fa_match.hip) ------------------------------------------------------------------
int fa_match_begin(fa_env *env, const int32_t *env_cell, int32_t n_cells, int32_t episodes_per_env, void *stream) {
    if (!env || !env_cell) return fail(FA_ERR_INVALID, "fa_match_begin: null argument");
    if (!env->cfg.track_counters) return fail(FA_ERR_STATE, "fa_match_begin: the handle was created with track_counters = 0");
    if (n_cells < 1 || episodes_per_env < 1) return fail(FA_ERR_INVALID, "fa_match_begin: need n_cells >= 1 and episodes_per_env >= 1");
    DeviceGuard guard(env->cfg.device_id);
    env->match.n_cells = n_cells;
    env->match.episodes_per_env = episodes_per_env;
    env->match.begun = 1;
    FA_HIP(fa_launch_match_begin(env->s, env->match, env_cell, env->cfg.num_envs, env->N, static_cast<hipStream_t>(stream)));
    return FA_OK;
}

int fa_match_latch(fa_env *env, void *stream) {
    if (!env) return fail(FA_ERR_INVALID, "fa_match_latch: null env");
    if (!env->cfg.track_counters) return fail(FA_ERR_STATE, "fa_match_latch: the handle was created with track_counters = 0");
    if (!env->match.begun) return fail(FA_ERR_STATE, "fa_match_latch: no match begun (fa_match_begin)");
    DeviceGuard guard(env->cfg.device_id);
    FA_HIP(fa_launch_match_latch(env->s, env->match, env->cfg.num_envs, env->N, static_cast<hipStream_t>(stream)));
    return FA_OK;
}

int fa_match_table(fa_env *env, double *raw, int32_t *remaining_out, void *stream) {
    if (!env || !raw) return fail(FA_ERR_INVALID, "fa_match_table: null argument");
    if (!env->cfg.track_counters) return fail(FA_ERR_STATE, "fa_match_table: the handle was created with track_counters = 0");
    if (!env->match.begun) return fail(FA_ERR_STATE, "fa_match_table: no match begun (fa_match_begin)");
    DeviceGuard guard(env->cfg.device_id);
    hipStream_t s = static_cast<hipStream_t>(stream);
    FA_HIP(fa_launch_match_table(env->s, env->match, env->cfg.num_envs, env->N, raw, s));
    int32_t flags[2] = {0, 0}; // remaining, overrun: adjacent device scalars
    FA_HIP(hipMemcpyAsync(flags, env->match.remaining, sizeof(flags), hipMemcpyDeviceToHost, s));
    FA_HIP(hipStreamSynchronize(s));
    if (remaining_out) *remaining_out = flags[0];
    if (flags[1])
        return fail(FA_ERR_STATE, "fa_match_table: an env played beyond episodes_per_env before it was latched "
                                  "(fa_match_latch must follow every one-step launch)");
    return FA_OK;
}

// ---- behaviour maps (fa_behaviour.hip) ------------------------------------------------------------------
int64_t fa_behaviour_cell_words(const fa_env *env) {
    if (!env) return fail(FA_ERR_INVALID, "fa_behaviour_cell_words: null env");
    return FA_BEHAVIOUR_CELL_WORDS((int64_t)env->cfg.max_time_steps);
}

int fa_behaviour_begin(fa_env *env, const int32_t *env_cell, int32_t n_cells, int32_t episodes_per_env, uint64_t *counts,
                       void *stream) {
    if (!env || !env_cell || !counts) return fail(FA_ERR_INVALID, "fa_behaviour_begin: null argument");
    if (n_cells < 1 || n_cells > FA_BEH_MAX_CELLS) return fail(FA_ERR_INVALID, "fa_behaviour_begin: n_cells must be 1..4096");
    if (episodes_per_env < 0) return fail(FA_ERR_INVALID, "fa_behaviour_begin: episodes_per_env must be >= 0 (0 = no quota)");
    if (env->cfg.max_time_steps > FA_BEH_MAX_MT)
        return fail(FA_ERR_INVALID, "fa_behaviour_begin: max_time_steps must be <= 1024 (a cell's record is kept in LDS)");
    DeviceGuard guard(env->cfg.device_id);
    hipStream_t s = static_cast<hipStream_t>(stream);
    FaBehaviour &bh = env->beh;
    const int E = env->cfg.num_envs;
    bh.begun = 0;
    // the launch plan: the envs grouped by cell (counting sort, ascending inside a cell; the envs of no cell last), cut into
    // slices of at most FA_BEH_SLICE envs of one cell
    std::vector<int32_t> cell(E), list(E), slices;
    FA_HIP(hipMemcpyAsync(cell.data(), env_cell, (size_t)E * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    FA_HIP(hipStreamSynchronize(s));
    std::vector<int32_t> start(n_cells + 2, 0);
    auto group = [&](int32_t c) { return (c >= 0 && c < n_cells) ? c : n_cells; };
    for (int e = 0; e < E; ++e) ++start[group(cell[e]) + 1];
    for (int c = 0; c <= n_cells; ++c) start[c + 1] += start[c];
    {
        std::vector<int32_t> at(start.begin(), start.end() - 1);
        for (int e = 0; e < E; ++e) list[at[group(cell[e])]++] = e;
    }
    for (int c = 0; c <= n_cells; ++c)
        for (int32_t f = start[c]; f < start[c + 1]; f += FA_BEH_SLICE) {
            const int32_t cnt = start[c + 1] - f < FA_BEH_SLICE ? start[c + 1] - f : FA_BEH_SLICE;
            const int32_t row[4] = {c < n_cells ? c : -1, f, cnt, 0};
            slices.insert(slices.end(), row, row + 4);
        }
    const int n_slices = (int)(slices.size() / 4);
    if (n_slices > bh.max_slices) return fail(FA_ERR_STATE, "fa_behaviour_begin: slice table overflow");
    FA_HIP(hipMemcpyAsync(bh.env_list, list.data(), (size_t)E * sizeof(int32_t), hipMemcpyHostToDevice, s));
    if (n_slices)
        FA_HIP(hipMemcpyAsync(bh.slices, slices.data(), slices.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
    FA_HIP(hipMemsetAsync(bh.ep_count, 0, (size_t)E * sizeof(int32_t), s));
    FA_HIP(hipMemcpyAsync(bh.ep_t, env->s.tstep, (size_t)E * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    FA_HIP(hipMemsetAsync(counts, 0, (size_t)n_cells * FA_BEHAVIOUR_CELL_WORDS((size_t)env->cfg.max_time_steps) * sizeof(uint64_t), s));
    FA_HIP(hipStreamSynchronize(s)); // the host vectors go out of scope
    bh.counts = counts;
    bh.n_cells = n_cells;
    bh.quota = episodes_per_env;
    bh.n_slices = n_slices;
    bh.begun = 1;
    return FA_OK;
}

int fa_behaviour_chunk(fa_env *env, void *stream) {
    if (!env) return fail(FA_ERR_INVALID, "fa_behaviour_chunk: null env");
    if (!env->bound) return fail(FA_ERR_STATE, "fa_behaviour_chunk: no storage bound");
    if (!env->beh.begun) return fail(FA_ERR_STATE, "fa_behaviour_chunk: no record begun (fa_behaviour_begin)");
    if (env->st.num_steps >= (1 << 24)) return fail(FA_ERR_INVALID, "fa_behaviour_chunk: num_steps must be < 2^24");
    DeviceGuard guard(env->cfg.device_id);
    const FaBehaviour &bh = env->beh;
    FaBehaviourArgs a;
    a.obs = env->st.obs;
    a.actions = env->st.actions;
    a.done = env->st.done;
    a.ep_count = bh.ep_count;
    a.ep_t = bh.ep_t;
    a.env_list = bh.env_list;
    a.slices = bh.slices;
    a.counts = bh.counts;
    a.T = env->st.num_steps;
    a.E = env->cfg.num_envs;
    a.N = env->N;
    a.G = env->cfg.num_guards;
    a.MT = env->cfg.max_time_steps;
    a.quota = bh.quota;
    a.words = (int32_t)FA_BEHAVIOUR_CELL_WORDS(env->cfg.max_time_steps);
    const fa_world_consts &w = env->cfg.world;
    a.x0 = (float)w.wall_xmin;
    a.sx = (float)(FA_BEHAVIOUR_BX / (w.wall_xmax - w.wall_xmin));
    a.y0 = (float)w.wall_ymin;
    a.sy = (float)(FA_BEHAVIOUR_BY / (w.wall_ymax - w.wall_ymin));
    if (bh.n_slices) FA_HIP(fa_launch_behaviour(a, bh.n_slices, static_cast<hipStream_t>(stream)));
    return FA_OK;
}

int fa_behaviour_state(fa_env *env, int32_t *ep_count_host, int32_t *ep_t_host) {
    if (!env) return fail(FA_ERR_INVALID, "fa_behaviour_state: null env");
    if (!env->beh.begun) return fail(FA_ERR_STATE, "fa_behaviour_state: no record begun (fa_behaviour_begin)");
    DeviceGuard guard(env->cfg.device_id);
    const size_t bytes = (size_t)env->cfg.num_envs * sizeof(int32_t);
    FA_HIP(hipDeviceSynchronize());
    if (ep_count_host) FA_HIP(hipMemcpy(ep_count_host, env->beh.ep_count, bytes, hipMemcpyDeviceToHost));
    if (ep_t_host) FA_HIP(hipMemcpy(ep_t_host, env->beh.ep_t, bytes, hipMemcpyDeviceToHost));
    return FA_OK;
}

// ---- frames on the device (fa_render.hip) --------------------------------------------------------------
int fa_render(fa_env *env, const fa_render_io *io, void *stream) {
    if (!env || !io) return fail(FA_ERR_INVALID, "fa_render: null argument");
    if (!io->env_index || !io->rgb) return fail(FA_ERR_INVALID, "fa_render: env_index and rgb are required");
    if (io->num_frames < 1) return fail(FA_ERR_INVALID, "fa_render: num_frames must be >= 1");
    if (io->size < 8 || io->size > 2048) return fail(FA_ERR_INVALID, "fa_render: size must be 8..2048");
    if ((io->team_attn != nullptr) != (io->opp_attn != nullptr))
        return fail(FA_ERR_INVALID, "fa_render: team_attn and opp_attn go together (the guards' pair, or neither)");
    if ((long long)io->num_frames * fa_render_tiles(io->size) > 0x7fffffffLL)
        return fail(FA_ERR_INVALID, "fa_render: num_frames x size is more than one launch covers");
    DeviceGuard guard(env->cfg.device_id);
    FaRenderArgs a;
    std::memset(&a, 0, sizeof(a));
    a.s = env->s;
    a.env_index = io->env_index;
    a.rgb = io->rgb;
    a.actions = io->actions;
    a.as_e = io->act_stride_env;
    a.as_i = io->act_stride_agent;
    a.no_laser = io->no_laser;
    a.team_attn = io->team_attn;
    a.opp_attn = io->opp_attn;
    a.K = io->num_frames;
    a.size = io->size;
    a.E = env->cfg.num_envs;
    a.G = env->cfg.num_guards;
    a.A = env->cfg.num_attackers;
    a.viz_dead = io->viz_dead != 0;
    a.attn_on = io->team_attn && io->viz_attn != 0;
    const FaDerived &c = env->c;
    a.agent_size = c.agent_size;
    a.fort_dim = c.fort_dim;
    a.door_x = c.door_x;
    a.door_y = c.door_y;
    a.wall_xmin = c.wall_xmin;
    a.wall_xmax = c.wall_xmax;
    a.wall_ymin = c.wall_ymin;
    a.wall_ymax = c.wall_ymax;
    a.shoot_rad = c.shoot_rad;
    a.half_win = c.half_win;
    FA_HIP(fa_launch_render(a, static_cast<hipStream_t>(stream)));
    return FA_OK;
}

int64_t fa_policy_weight_floats(void) { return FA_POLICY_WEIGHT_FLOATS; }
int64_t fa_policy_plain_floats(void) { return FA_POLICY_PLAIN_FLOATS; }

int64_t fa_ppo_grad_floats(void) { return FA_SLAB_FLOATS; }
int64_t fa_adam_scratch_floats(void) { return FA_ADAM_SCRATCH; }
int64_t fa_policy_weight_t_floats(void) { return FA_TRANS_FLOATS; }

int fa_ppo_grad_scratch(int32_t B, int32_t G, int32_t A, int64_t *slab_floats, int64_t *hsave_floats) {
    if (B < 1 || G < 1 || A < 1 || G > FA_POLICY_MAX_TEAM || A > FA_POLICY_MAX_TEAM)
        return fail(FA_ERR_INVALID, "fa_ppo_grad_scratch: need B >= 1 and teams of 1..8");
    const int et = fa_train_tile_envs(G, A);
    const int64_t tiles = (B + et - 1) / et;
    // slabs: the tiles' small gradients | their stage-1 sums | the partial slabs of the weight-gradient GEMM | mask sums
    if (slab_floats) *slab_floats = tiles * FA_MSLAB_FLOATS + (int64_t)FA_MRED_PARTS * FA_MSLAB_FLOATS +
                                    (int64_t)FA_DW_WGS_A * FA_DWA_FLOATS + (int64_t)FA_DW_WGS_B * FA_DWB_FLOATS + FA_MASK_PARTS;
    // hsave: the records of the weight-gradient GEMM's operands: [tiles][3] x A, then [tiles] x B
    if (hsave_floats) *hsave_floats = tiles * FA_TR_SAVE_FLOATS;
    return FA_OK;
}

int fa_ppo_grad(const fa_ppo_grad_io *io, void *stream) {
    if (!io) return fail(FA_ERR_INVALID, "fa_ppo_grad: null io");
    if (!io->obs || !io->action || !io->value_pred || !io->ret || !io->old_log_prob || !io->weights ||
        !io->weights_t || !io->slabs || !io->hsave || !io->out)
        return fail(FA_ERR_INVALID, "fa_ppo_grad: every pointer but idx, scale and adv / adv_mean / adv_std is required");
    if ((io->adv_mean == nullptr) != (io->adv_std == nullptr) || (!io->adv && !io->adv_mean))
        return fail(FA_ERR_INVALID, "fa_ppo_grad: pass adv, or adv_mean and adv_std together");
    if (io->B < 1 || io->num_guards < 1 || io->num_attackers < 1 || io->num_guards > FA_POLICY_MAX_TEAM ||
        io->num_attackers > FA_POLICY_MAX_TEAM || (io->team != 0 && io->team != 1))
        return fail(FA_ERR_INVALID, "fa_ppo_grad: need B >= 1, teams of 1..8, team 0 or 1");
    FaTrainArgs a;
    std::memset(&a, 0, sizeof(a));
    a.obs = io->obs; a.action = io->action; a.value_pred = io->value_pred; a.ret = io->ret;
    a.old_logp = io->old_log_prob; a.adv = io->adv; a.w = io->weights; a.wt = io->weights_t;
    a.adv_mean = io->adv_mean; a.adv_std = io->adv_std;
    a.scale = io->scale; a.idx = io->idx;
    a.B = io->B; a.G = io->num_guards; a.A = io->num_attackers; a.team = io->team;
    a.clip = io->clip_param; a.c_value = io->value_loss_coef; a.c_entropy = io->entropy_coef;
    a.clipped_value_loss = io->clipped_value_loss;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int et = fa_train_tile_envs(a.G, a.A);
    const size_t tiles = (size_t)((a.B + et - 1) / et);
    float *mpart = io->slabs + tiles * FA_MSLAB_FLOATS, *dw_slabs = mpart + (size_t)FA_MRED_PARTS * FA_MSLAB_FLOATS;
    a.mslab = io->slabs;
    a.rec_a = io->hsave;
    a.rec_b = io->hsave + tiles * 3 * FA_RECA_FLOATS;
    a.rec_g = a.rec_b + tiles * FA_RECB_FLOATS;
    if (!a.scale) { // partial mask sums behind the partial slabs; the scale pair is left behind the loss sums of `out`
        float *part = dw_slabs + (size_t)FA_DW_WGS_A * FA_DWA_FLOATS + (size_t)FA_DW_WGS_B * FA_DWB_FLOATS;
        FA_HIP(fa_launch_mask_parts(a, part, s));
        a.mask_part = part;
        a.scale_out = io->out + FA_SLAB_LOSS + 8;
        a.normalize = io->normalize != 0;
    }
    FA_HIP(fa_launch_train(a, s));                                           // tiles: forward, losses, dL/dX
    FA_HIP(fa_launch_train_dw(a.rec_a, a.rec_b, (int)tiles, dw_slabs, s));   // dW = X^T dY over all rows
    FA_HIP(fa_launch_train_reduce(a.mslab, (int)tiles, mpart, dw_slabs, io->out, s)); // fixed-order sums -> out
    return FA_OK;
}

int fa_adam_step(float *params, float *grads, float *exp_avg, float *exp_avg_sq, float *steps, const int32_t *seg,
                 int32_t nseg, int32_t n, float lr, float beta1, float beta2, float eps, float max_grad_norm, float *scratch,
                 void *stream) {
    if (!params || !grads || !exp_avg || !exp_avg_sq || !steps || !seg || !scratch)
        return fail(FA_ERR_INVALID, "fa_adam_step: null argument");
    if (nseg < 1 || n < 1) return fail(FA_ERR_INVALID, "fa_adam_step: need nseg >= 1 and n >= 1");
    if (reinterpret_cast<uintptr_t>(scratch) & 15) return fail(FA_ERR_INVALID, "fa_adam_step: scratch must be 16-byte aligned");
    FA_HIP(fa_launch_adam(params, grads, exp_avg, exp_avg_sq, steps, seg, nseg, n, lr, beta1, beta2, eps, max_grad_norm, scratch,
                          nullptr, static_cast<hipStream_t>(stream)));
    return FA_OK;
}

int fa_adam_step_dev(float *params, float *grads, float *exp_avg, float *exp_avg_sq, float *steps, const int32_t *seg,
                     int32_t nseg, int32_t n, const float *hyper, float *scratch, void *stream) {
    if (!params || !grads || !exp_avg || !exp_avg_sq || !steps || !seg || !scratch || !hyper)
        return fail(FA_ERR_INVALID, "fa_adam_step_dev: null argument");
    if (nseg < 1 || n < 1) return fail(FA_ERR_INVALID, "fa_adam_step_dev: need nseg >= 1 and n >= 1");
    if (reinterpret_cast<uintptr_t>(scratch) & 15) return fail(FA_ERR_INVALID, "fa_adam_step_dev: scratch must be 16-byte aligned");
    FA_HIP(fa_launch_adam(params, grads, exp_avg, exp_avg_sq, steps, seg, nseg, n, 0.f, 0.f, 0.f, 0.f, 0.f, scratch, hyper,
                          static_cast<hipStream_t>(stream)));
    return FA_OK;
}

int fa_run_tasks(const fa_task *tasks, int32_t n, void *stream) {
    if (!tasks || n < 0) return fail(FA_ERR_INVALID, "fa_run_tasks: null task list");
    FA_HIP(fa_launch_tasks(tasks, n, static_cast<hipStream_t>(stream)));
    return FA_OK;
}

int fa_pack_weights(const float *plain, float *weights, float *weights_t, void *stream) {
    if (!plain || !weights || !weights_t) return fail(FA_ERR_INVALID, "fa_pack_weights: null argument");
    FA_HIP(fa_launch_pack(plain, weights, weights_t, static_cast<hipStream_t>(stream)));
    return FA_OK;
}

static int attend_check(const char *who, int B, int n, int nk, int width) {
    if (B < 1 || n < 1 || nk < 1 || n > FA_POLICY_MAX_TEAM || nk > FA_POLICY_MAX_TEAM)
        return fail(FA_ERR_INVALID, std::string(who) + ": need B >= 1 and 1 <= n, nk <= 8");
    if (width != 64 && width != 128) return fail(FA_ERR_INVALID, std::string(who) + ": width must be 64 or 128");
    return FA_OK;
}

int fa_attend_forward(const float *g, const float *keys, float *out, float *attn, int32_t B, int32_t n, int32_t nk,
                      int32_t width, int32_t skip_self, void *stream) {
    if (!g || !keys || !out || !attn) return fail(FA_ERR_INVALID, "fa_attend_forward: null argument");
    if (int rc = attend_check("fa_attend_forward", B, n, nk, width)) return rc;
    FA_HIP(fa_launch_attend(width, false, g, keys, out, attn, nullptr, nullptr, nullptr, B, n, nk, skip_self,
                            static_cast<hipStream_t>(stream)));
    return FA_OK;
}

int fa_attend_backward(const float *g, const float *keys, const float *attn, const float *dout, float *dg, float *dkeys,
                       int32_t B, int32_t n, int32_t nk, int32_t width, int32_t skip_self, void *stream) {
    if (!g || !keys || !attn || !dout || !dg || !dkeys) return fail(FA_ERR_INVALID, "fa_attend_backward: null argument");
    if (int rc = attend_check("fa_attend_backward", B, n, nk, width)) return rc;
    FA_HIP(fa_launch_attend(width, true, g, keys, nullptr, const_cast<float *>(attn), dout, dg, dkeys, B, n, nk, skip_self,
                            static_cast<hipStream_t>(stream)));
    return FA_OK;
}

int fa_get_state(fa_env *env, const fa_state_host *o) {
    if (!env || !o) return fail(FA_ERR_INVALID, "fa_get_state: null argument");
    DeviceGuard guard(env->cfg.device_id);
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
#undef FA_D2H
#define FA_D2H_LATE(dst, src, bytes) \
    if (dst) FA_HIP(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost))
    FA_D2H_LATE(o->episode_reward_sum, s.ep_rew_sum, EN * 8);
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
    if (!env || !in) return fail(FA_ERR_INVALID, "fa_set_state: null argument");
    DeviceGuard guard(env->cfg.device_id);
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
    if (!env || !mismatch_host) return fail(FA_ERR_INVALID, "fa_selftest_math: null argument");
    DeviceGuard guard(env->cfg.device_id);
    unsigned long long *d = reinterpret_cast<unsigned long long *>(env->adv_partial); // scratch
    FA_HIP(hipDeviceSynchronize());
    FA_HIP(hipMemset(d, 0, 24));
    const unsigned long long per = samples / (1024ull * 256ull) + 1ull;
    FA_HIP(fa_launch_selftest(per, seed, d, nullptr));
    FA_HIP(hipMemcpy(mismatch_host, d, 24, hipMemcpyDeviceToHost));
    return FA_OK;
}

const char *fa_policy_variant(fa_env *env) {
    if (!env) return "";
    const int E = env->cfg.num_envs, G = env->cfg.num_guards, A = env->cfg.num_attackers;
    if (G > FA_POLICY_MAX_TEAM || A > FA_POLICY_MAX_TEAM) return "";
    const int n_max = G > A ? G : A;
    return fa_policy_tile_envs(E, G, A) * n_max > 64 ? "fa_policy_kernel<3, 8>" : "fa_policy_kernel<2, 4>";
}

const char *fa_step_variant(fa_env *env, int32_t num_steps) {
    if (!env) return "";
    return fa_step_variant_name(env->cfg.num_guards, env->cfg.num_attackers, env->cfg.num_envs, num_steps,
                                env->cfg.step_kernel, env->choice_k > 0);
}

int fa_rng_peek(fa_env *env, int32_t e, int32_t count, double *out_host) {
    if (!env || !out_host) return fail(FA_ERR_INVALID, "fa_rng_peek: null argument");
    if (e < 0 || e >= env->cfg.num_envs || count < 0) return fail(FA_ERR_INVALID, "fa_rng_peek: bad index");
    if (env->cfg.rng_mode != FA_RNG_MT19937) return fail(FA_ERR_STATE, "fa_rng_peek: MT19937 mode only");
    DeviceGuard guard(env->cfg.device_id);
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
