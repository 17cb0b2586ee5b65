// fa_behaviour.hip -- strategy fingerprints: per match-up cell, integer histograms of where the agents of each team stand,
// fire and die and of how long episodes last, summed over the bound storage of one chunk (include/fortattack.h:
// fa_behaviour_begin / fa_behaviour_chunk; behaviour.py::behaviour_chunk_numpy is the definition, statement for statement).
//
// Shape: a workgroup owns a slice of up to FA_BEH_SLICE envs of ONE cell (the list fa_behaviour_begin built) and keeps that
// cell's whole record in LDS as uint32.  The chunk's steps are taken in blocks of FA_BEH_TB:
//   scan   lane j < slice size walks env j's `done` column over the block (the loads eight at a time, they do not depend on
//          the walk) and leaves per (step, env) the clamped step-in-episode t, the done flag, or "beyond the quota".  This is
//          the only sequential part; it also counts steps, episodes and the episode-length histogram.
//   sweep  all lanes take the block's (step, env, agent) samples, agent fastest: the obs row as two 8-byte loads (a row is
//          24 bytes, so it is 8- but not 16-byte aligned), the next row's alive flag and the action, all issued before any is
//          used; then LDS integer atomics.
// At the end the non-zero words go to the global uint64 record with one integer atomic per word and workgroup, and the two
// per-env counters are written back.  Integer sums only: the record does not depend on the order of anything.
// An env of no cell is scanned (its counters advance) and counted nowhere: its slices skip the sweep and the LDS record.
// A word of the LDS record is uint32: a workgroup adds at most T * FA_BEH_SLICE * N to one, so T < 2^24 (checked on the host).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "fa_env.h"

#define FA_BEH_THREADS 256
#define FA_BEH_SLICE 16  // envs of ONE cell per workgroup
#define FA_BEH_TB 64     // steps per block of the done scan / the sample sweep
#define FA_BEH_MAX_CELLS 4096
#define FA_BEH_MAX_MT 1024 // the largest record a workgroup keeps in LDS: (2 + 3 * 1024 + 6 * 32 * 40) * 4 = 43 016 bytes

struct FaBehaviourArgs {
    const float *obs;       // (T+1, E, N, 6)
    const int64_t *actions; // (T, E, N)
    const uint8_t *done;    // (T, E)
    int32_t *ep_count, *ep_t;
    const int32_t *env_list, *slices;
    uint64_t *counts;
    int32_t T, E, N, G, MT, quota, words;
    float x0, sx, y0, sy;
};

namespace {

#define FA_BEH_CUT 0xffffffffu // scan result: the env had played its episodes before this step
#define FA_BEH_DONE 0x10000u   // scan result: t in the low 16 bits (t < FA_BEH_MAX_MT), this flag where the step ended the episode

__device__ __forceinline__ int bin_of(float v, float v0, float scale, int n) {
    const float d = v - v0;     // two separately rounded float32 operations (-ffp-contract=off)
    const float f = floorf(d * scale);
    return (int)fminf(fmaxf(f, 0.0f), (float)(n - 1)); // clamped in float, then converted
}

__global__ __launch_bounds__(FA_BEH_THREADS) void fa_behaviour_kernel(FaBehaviourArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint32_t *const tinfo = reinterpret_cast<uint32_t *>(smem);                 // [FA_BEH_TB][FA_BEH_SLICE]
    int32_t *const senv = reinterpret_cast<int32_t *>(tinfo + FA_BEH_TB * FA_BEH_SLICE); // [FA_BEH_SLICE]
    uint32_t *const hist = reinterpret_cast<uint32_t *>(senv + FA_BEH_SLICE);   // [a.words]
    const int tid = threadIdx.x;
    const int32_t *const sl = a.slices + 4 * (size_t)blockIdx.x;
    const int cell = sl[0], first = sl[1], n = sl[2];
    const bool counted = cell >= 0;
    const int E = a.E, N = a.N, MT = a.MT, T = a.T;
    const int off_alive = FA_BEHAVIOUR_OFF_ALIVE_T(MT), off_occ = FA_BEHAVIOUR_OFF_OCC(MT);
    const int maps = 2 * FA_BEHAVIOUR_BY * FA_BEHAVIOUR_BX;

    if (counted)
        for (int w = tid; w < a.words; w += FA_BEH_THREADS) hist[w] = 0u;
    int e = 0, cnt = 0, t = 0;
    uint32_t n_steps = 0, n_eps = 0;
    const bool scanner = tid < n;
    if (scanner) {
        e = a.env_list[first + tid];
        senv[tid] = e;
        cnt = a.ep_count[e];
        t = a.ep_t[e];
    }
    __syncthreads();

    for (int s0 = 0; s0 < T; s0 += FA_BEH_TB) {
        const int tb = min(FA_BEH_TB, T - s0);
        if (scanner) {
            for (int k0 = 0; k0 < tb; k0 += 8) {
                uint8_t d[8];
#pragma unroll
                for (int q = 0; q < 8; ++q) d[q] = (k0 + q < tb) ? a.done[(size_t)(s0 + k0 + q) * E + e] : (uint8_t)0;
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    if (k0 + q >= tb) break;
                    uint32_t info = FA_BEH_CUT;
                    if (!(a.quota > 0 && cnt >= a.quota)) {
                        const int tc = min(t, MT - 1);
                        info = (uint32_t)tc;
                        ++n_steps;
                        if (d[q]) {
                            info |= FA_BEH_DONE;
                            if (counted) atomicAdd(&hist[FA_BEHAVIOUR_OFF_LEN_HIST + tc], 1u);
                            ++n_eps;
                            ++cnt;
                            t = 0;
                        } else {
                            ++t;
                        }
                    }
                    tinfo[(k0 + q) * FA_BEH_SLICE + tid] = info;
                }
            }
        }
        __syncthreads();
        if (counted) {
            const int total = tb * n * N;
            for (int idx = tid; idx < total; idx += FA_BEH_THREADS) {
                const int r = idx / N, i = idx - r * N;
                const int k = r / n, j = r - k * n;
                const uint32_t info = tinfo[k * FA_BEH_SLICE + j];
                if (info == FA_BEH_CUT) continue;
                const size_t sample = ((size_t)(s0 + k) * E + senv[j]) * N + i;
                const float *const row = a.obs + sample * FA_OBS_DIM;
                const float2 ax = *reinterpret_cast<const float2 *>(row);       // alive, x
                const float2 ya = *reinterpret_cast<const float2 *>(row + 2);   // y, angle
                const float next_alive = row[(size_t)E * N * FA_OBS_DIM];       // the same agent one step later
                const int64_t act = a.actions[sample];
                if (ax.x != 0.0f) {
                    const int team = i >= a.G ? 1 : 0;
                    const int bx = bin_of(ax.y, a.x0, a.sx, FA_BEHAVIOUR_BX), by = bin_of(ya.x, a.y0, a.sy, FA_BEHAVIOUR_BY);
                    const int bin = (team * FA_BEHAVIOUR_BY + by) * FA_BEHAVIOUR_BX + bx;
                    atomicAdd(&hist[off_occ + bin], 1u);
                    atomicAdd(&hist[off_alive + team * MT + (int)(info & 0xffffu)], 1u);
                    if (act == 7) atomicAdd(&hist[off_occ + maps + bin], 1u);
                    if (!(info & FA_BEH_DONE) && next_alive == 0.0f) atomicAdd(&hist[off_occ + 2 * maps + bin], 1u);
                }
            }
        }
        __syncthreads();
    }

    if (scanner) {
        a.ep_count[e] = cnt;
        a.ep_t[e] = t;
        if (counted) {
            atomicAdd(&hist[FA_BEHAVIOUR_OFF_STEPS], n_steps);
            atomicAdd(&hist[FA_BEHAVIOUR_OFF_EPISODES], n_eps);
        }
    }
    if (!counted) return; // the whole workgroup
    __syncthreads();
    unsigned long long *const rec = reinterpret_cast<unsigned long long *>(a.counts) + (size_t)cell * a.words;
    for (int w = tid; w < a.words; w += FA_BEH_THREADS) {
        const uint32_t v = hist[w];
        if (v) atomicAdd(&rec[w], (unsigned long long)v);
    }
}
} // namespace

static hipError_t fa_launch_behaviour(const FaBehaviourArgs &a, int n_slices, hipStream_t st) {
    const size_t lds = (size_t)(FA_BEH_TB * FA_BEH_SLICE + FA_BEH_SLICE + a.words) * sizeof(uint32_t);
    hipLaunchKernelGGL(fa_behaviour_kernel, dim3((unsigned)n_slices), dim3(FA_BEH_THREADS), lds, st, a);
    return hipGetLastError();
}

// ep_count, ep_t, the env list (E each) and the slice table
void fa_behaviour_regions(fa_env *env, FaSlab &slab) {
    FaBehaviour &bh = env->beh;
    const size_t E = (size_t)env->cfg.num_envs;
    bh.max_slices = (env->cfg.num_envs + FA_BEH_SLICE - 1) / FA_BEH_SLICE + FA_BEH_MAX_CELLS + 1;
    slab.region(bh.ep_count, E, true);
    slab.region(bh.ep_t, E, true);
    slab.region(bh.env_list, E);
    slab.region(bh.slices, (size_t)bh.max_slices * 4);
}

extern "C" {

int64_t fa_behaviour_cell_words(const fa_env *env) {
    if (int rc = fa_enter(env, "fa_behaviour_cell_words", false)) return rc;
    return FA_BEHAVIOUR_CELL_WORDS((int64_t)env->cfg.max_time_steps);
}

int fa_behaviour_begin(fa_env *env, const int32_t *env_cell, int32_t n_cells, int32_t episodes_per_env, uint64_t *counts,
                       void *stream) {
    FA_ENTER(env, "fa_behaviour_begin", false, env_cell, counts);
    if (n_cells < 1 || n_cells > FA_BEH_MAX_CELLS) return fail(FA_ERR_INVALID, "fa_behaviour_begin: n_cells must be 1..4096");
    if (episodes_per_env < 0) return fail(FA_ERR_INVALID, "fa_behaviour_begin: episodes_per_env must be >= 0 (0 = no quota)");
    if (env->cfg.max_time_steps > FA_BEH_MAX_MT)
        return fail(FA_ERR_INVALID, "fa_behaviour_begin: max_time_steps must be <= 1024 (a cell's record is kept in LDS)");
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
    FA_ENTER(env, "fa_behaviour_chunk", true);
    if (!env->beh.begun) return fail(FA_ERR_STATE, "fa_behaviour_chunk: no record begun (fa_behaviour_begin)");
    if (env->st.num_steps >= (1 << 24)) return fail(FA_ERR_INVALID, "fa_behaviour_chunk: num_steps must be < 2^24");
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
    FA_ENTER(env, "fa_behaviour_state", false);
    if (!env->beh.begun) return fail(FA_ERR_STATE, "fa_behaviour_state: no record begun (fa_behaviour_begin)");
    const size_t bytes = (size_t)env->cfg.num_envs * sizeof(int32_t);
    FA_HIP(hipDeviceSynchronize());
    if (ep_count_host) FA_HIP(hipMemcpy(ep_count_host, env->beh.ep_count, bytes, hipMemcpyDeviceToHost));
    if (ep_t_host) FA_HIP(hipMemcpy(ep_t_host, env->beh.ep_t, bytes, hipMemcpyDeviceToHost));
    return FA_OK;
}

} // extern "C"
