// fa_match.hip -- cross-play bookkeeping on the device.  The reference's result scripts play a FIXED number of episodes per
// match-up (test_fortattack_v2.py:56-124, test_fortattack_v2_gen_plot_data.py:61-141) and emit one row per match-up.  The step
// kernels already count finished episodes per env (result_count / alive_end / ep_rew_sum, FaState); summed over a window of
// steps those over-weight the envs whose episodes are short.  Here every env contributes exactly `episodes_per_env` episodes:
//   begin  records the counters as the baseline,
//   latch  (after every one-step launch) copies counters - baseline of an env that has just reached its quota, once,
//   table  sums the latched numbers per cell in a fixed order (no floating-point atomics: equal bits run to run).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fa_env.h"

#define FA_MATCH_THREADS 256 // workgroup of the table kernel: one per cell

namespace {
__device__ __forceinline__ uint32_t episodes_since(const FaState &s, const FaMatch &m, int e) {
    uint32_t n = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) n += s.result_count[(size_t)e * 3 + k] - m.base_rc[(size_t)e * 3 + k];
    return n;
}

__global__ __launch_bounds__(256) void fa_match_begin_kernel(FaState s, FaMatch m, const int32_t *__restrict__ env_cell, int E, int N) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e == 0) { m.remaining[0] = E; m.overrun[0] = 0; }
    if (e >= E) return;
    m.cell[e] = env_cell[e];
    m.latched[e] = 0;
    for (int k = 0; k < 3; ++k) {
        m.base_rc[(size_t)e * 3 + k] = s.result_count[(size_t)e * 3 + k];
        m.lat_rc[(size_t)e * 3 + k] = 0u;
    }
    for (int i = 0; i < N; ++i) {
        const size_t idx = (size_t)e * N + i;
        m.base_alive[idx] = s.alive_end[idx];
        m.base_rew[idx] = s.ep_rew_sum[idx];
        m.lat_alive[idx] = 0u;
        m.lat_rew[idx] = 0.0;
        // the running return of an episode in flight is evaluation bookkeeping, not simulation state: the match starts clean
        // (a reset clears it as well, fa_step_classic.hip; the evaluator resets every env right after)
        s.ep_rew[idx] = 0.0;
    }
}

__global__ __launch_bounds__(256) void fa_match_latch_kernel(FaState s, FaMatch m, int E, int N, uint32_t quota) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E || m.latched[e]) return;
    const uint32_t n = episodes_since(s, m, e);
    if (n < quota) return;
    if (n > quota) atomicOr(m.overrun, 1); // the caller skipped latches: more than one episode ended since the last one
    for (int k = 0; k < 3; ++k) m.lat_rc[(size_t)e * 3 + k] = s.result_count[(size_t)e * 3 + k] - m.base_rc[(size_t)e * 3 + k];
    for (int i = 0; i < N; ++i) {
        const size_t idx = (size_t)e * N + i;
        m.lat_alive[idx] = s.alive_end[idx] - m.base_alive[idx];
        m.lat_rew[idx] = s.ep_rew_sum[idx] - m.base_rew[idx];
    }
    m.latched[e] = 1;
    atomicSub(m.remaining, 1);
}

// One workgroup per cell.  Column by column: thread t adds the cell's latched envs e = t, t + 256, ... in ascending order, then a
// fixed tree over the 256 partial sums -- the order of every addition is a function of (E, cell assignment) alone.
__global__ __launch_bounds__(FA_MATCH_THREADS) void fa_match_table_kernel(FaState s, FaMatch m, int E, int N, uint32_t quota,
                                                                          double *__restrict__ raw) {
    __shared__ double red[FA_MATCH_THREADS];
    const int c = blockIdx.x, tid = threadIdx.x, ncol = 5 + 2 * N;
    if (c == 0) // an env beyond its quota that no latch has seen yet
        for (int e = tid; e < E; e += FA_MATCH_THREADS)
            if (!m.latched[e] && episodes_since(s, m, e) > quota) atomicOr(m.overrun, 1);
    for (int col = 0; col < ncol; ++col) {
        double acc = 0.0;
        for (int e = tid; e < E; e += FA_MATCH_THREADS) {
            if (m.cell[e] != c || !m.latched[e]) continue;
            double v;
            if (col == 0) v = 1.0;
            else if (col == 1) v = (double)(m.lat_rc[(size_t)e * 3] + m.lat_rc[(size_t)e * 3 + 1] + m.lat_rc[(size_t)e * 3 + 2]);
            else if (col < 5) v = (double)m.lat_rc[(size_t)e * 3 + (col - 2)];
            else if (col < 5 + N) v = (double)m.lat_alive[(size_t)e * N + (col - 5)];
            else v = m.lat_rew[(size_t)e * N + (col - 5 - N)];
            acc += v;
        }
        red[tid] = acc;
        __syncthreads();
        for (int w = FA_MATCH_THREADS / 2; w > 0; w >>= 1) {
            if (tid < w) red[tid] += red[tid + w];
            __syncthreads();
        }
        if (tid == 0) raw[(size_t)c * ncol + col] = red[0];
        __syncthreads();
    }
}
} // namespace

static hipError_t fa_launch_match_begin(const FaState &s, const FaMatch &m, const int32_t *env_cell, int E, int N, hipStream_t st) {
    hipLaunchKernelGGL(fa_match_begin_kernel, dim3((E + 255) / 256), dim3(256), 0, st, s, m, env_cell, E, N);
    return hipGetLastError();
}

static hipError_t fa_launch_match_latch(const FaState &s, const FaMatch &m, int E, int N, hipStream_t st) {
    hipLaunchKernelGGL(fa_match_latch_kernel, dim3((E + 255) / 256), dim3(256), 0, st, s, m, E, N, (uint32_t)m.episodes_per_env);
    return hipGetLastError();
}

static hipError_t fa_launch_match_table(const FaState &s, const FaMatch &m, int E, int N, double *raw, hipStream_t st) {
    hipLaunchKernelGGL(fa_match_table_kernel, dim3(m.n_cells), dim3(FA_MATCH_THREADS), 0, st, s, m, E, N,
                       (uint32_t)m.episodes_per_env, raw);
    return hipGetLastError();
}

// baseline and latched copies of the three counters, the per-env cell / latch flag, two scalars; with track_counters = 0 the
// per-env regions are empty and the handle's pointers stay null (every export below refuses such a handle)
void fa_match_regions(fa_env *env, FaSlab &slab) {
    const bool on = env->cfg.track_counters != 0;
    FaMatch unused;
    FaMatch &m = on ? env->match : unused;
    const size_t E = on ? (size_t)env->cfg.num_envs : 0, EN = E * env->N;
    slab.region(m.base_rc, E * 3, true);
    slab.region(m.lat_rc, E * 3);
    slab.region(m.base_alive, EN, true);
    slab.region(m.lat_alive, EN);
    slab.region(m.base_rew, EN, true);
    slab.region(m.lat_rew, EN);
    slab.region(m.cell, E, true);
    slab.region(m.latched, E);
    slab.region(m.remaining, 1, true);
    slab.region(m.overrun, 1);
}

extern "C" {

int fa_match_begin(fa_env *env, const int32_t *env_cell, int32_t n_cells, int32_t episodes_per_env, void *stream) {
    FA_ENTER(env, "fa_match_begin", false, env_cell);
    if (!env->cfg.track_counters) return fail(FA_ERR_STATE, "fa_match_begin: the handle was created with track_counters = 0");
    if (n_cells < 1 || episodes_per_env < 1) return fail(FA_ERR_INVALID, "fa_match_begin: need n_cells >= 1 and episodes_per_env >= 1");
    env->match.n_cells = n_cells;
    env->match.episodes_per_env = episodes_per_env;
    env->match.begun = 1;
    FA_HIP(fa_launch_match_begin(env->s, env->match, env_cell, env->cfg.num_envs, env->N, static_cast<hipStream_t>(stream)));
    return FA_OK;
}

int fa_match_latch(fa_env *env, void *stream) {
    FA_ENTER(env, "fa_match_latch", false);
    if (!env->cfg.track_counters) return fail(FA_ERR_STATE, "fa_match_latch: the handle was created with track_counters = 0");
    if (!env->match.begun) return fail(FA_ERR_STATE, "fa_match_latch: no match begun (fa_match_begin)");
    FA_HIP(fa_launch_match_latch(env->s, env->match, env->cfg.num_envs, env->N, static_cast<hipStream_t>(stream)));
    return FA_OK;
}

int fa_match_table(fa_env *env, double *raw, int32_t *remaining_out, void *stream) {
    FA_ENTER(env, "fa_match_table", false, raw);
    if (!env->cfg.track_counters) return fail(FA_ERR_STATE, "fa_match_table: the handle was created with track_counters = 0");
    if (!env->match.begun) return fail(FA_ERR_STATE, "fa_match_table: no match begun (fa_match_begin)");
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

} // extern "C"
