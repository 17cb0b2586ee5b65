// fa_env.h -- internal: the handle behind the C ABI (include/fortattack.h) and what the exports of every translation unit
// share -- the error helper, the device guard, the checks that open an export, the slab carver.  Host side only; an export lives
// in the translation unit whose kernels it launches.
#pragma once
#include <cstring>
#include <string>

#include <hip/hip_runtime.h>

#include "fa_behaviour.h"
#include "fa_device.h"
#include "fa_match.h"
#include "fortattack.h"

int fa_api_fail(int code, const std::string &msg); // fa_api.hip: sets the thread-local message of fa_last_error
static inline int fail(int code, const std::string &msg) { return fa_api_fail(code, msg); }
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

// The checks that open an export: the handle -- with the export's other required pointers, when it passes any, folded into
// one "null argument" -- then, for an export that works on the bound storage, that one is bound.
template <class... P> int fa_enter(const fa_env *env, const char *who, bool needs_storage, const P *...required) {
    if (!env || (... || !required))
        return fail(FA_ERR_INVALID, std::string(who) + (sizeof...(required) ? ": null argument" : ": null env"));
    if (needs_storage && !env->bound) return fail(FA_ERR_STATE, std::string(who) + ": no storage bound");
    return FA_OK;
}
// ... and the handle's device for the rest of the export
#define FA_ENTER(env, who, needs_storage, ...)                                             \
    if (int _rc = fa_enter(env, who, needs_storage, ##__VA_ARGS__)) return _rc;            \
    DeviceGuard _guard((env)->cfg.device_id)

// The handle's one device allocation.  A region is named once -- pointer, element count -- in a list that is walked twice:
// without a base it sizes the slab, with the allocation it places the pointers.  Every region starts 256-byte aligned;
// `packed` lets the next one follow without padding (arrays of one type that the kernels index as one).
struct FaSlab {
    char *base;
    size_t bytes;
    template <class T> void region(T *&p, size_t count, bool packed = false) {
        if (base) p = reinterpret_cast<T *>(base + bytes);
        bytes += count * sizeof(T);
        if (!packed) bytes = (bytes + 255) & ~(size_t)255;
    }
};
// what each subsystem keeps in the slab, in the slab's order (fa_create)
void fa_policy_regions(fa_env *env, FaSlab &slab);    // fa_policy.hip
void fa_match_regions(fa_env *env, FaSlab &slab);     // fa_match.hip
void fa_behaviour_regions(fa_env *env, FaSlab &slab); // fa_behaviour.hip

inline FaStepArgs base_args(const fa_env *env) {
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

// the step launchers (fa_step_classic.hip)
hipError_t fa_launch_step(const FaStepArgs &a, hipStream_t st);
hipError_t fa_launch_reset(const FaStepArgs &a, hipStream_t st);
const char *fa_step_variant_name(int G, int A, int E, int nsteps, int step_kernel, bool choice);
int fa_step_experiments_linked(); // 1 in a variant library that carries csrc/experiments/
hipError_t fa_launch_seed(const FaState &s, int E, uint64_t base_seed, int64_t env_offset, int skip_words,
                          hipStream_t st);
hipError_t fa_launch_selftest(unsigned long long n_per_thread, unsigned long long seed, unsigned long long *mismatch,
                              hipStream_t st);
