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

#include "fa_behaviour.h"
#include "fortattack.h"

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

hipError_t fa_launch_behaviour(const FaBehaviourArgs &a, int n_slices, hipStream_t st) {
    const size_t lds = (size_t)(FA_BEH_TB * FA_BEH_SLICE + FA_BEH_SLICE + a.words) * sizeof(uint32_t);
    hipLaunchKernelGGL(fa_behaviour_kernel, dim3((unsigned)n_slices), dim3(FA_BEH_THREADS), lds, st, a);
    return hipGetLastError();
}
