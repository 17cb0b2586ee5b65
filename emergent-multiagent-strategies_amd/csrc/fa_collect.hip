// fa_collect.hip -- PPO rollout-collector kernels (gfx950): GAE scan, advantage
// statistics, advantage normalisation.  All tensors are the caller's joint
// RolloutStorage buffers, (T[+1], E, N) float32, column c = e*N + i contiguous.
//
// These are HBM-streaming kernels: GAE reads r, V, m (12 B) and writes ret (4 B) per
// (t, e, i); the statistics read ret, V (8 B).  One lane per column, consecutive lanes
// on consecutive columns => every row access is a coalesced span.
#include "fa_env.h"
#include "fa_collect.h"

// Learner.wrap_horizon (learner.py:191-211) + RolloutStorage.compute_returns
// (storage.py:59-66) as one backward pass with per-env episode boundaries.
// `done[t*E + e]` != 0  <=>  the episode of env e ended at rollout step t, i.e. t+1 is one
// of that env's end_pts; index end_pt < T is never visited by the reference (the next
// segment starts at end_pt + 1, learner.py:211): its `returns` entry keeps its old value
// and the accumulator restarts at 0 for the segment below it.
// float32 throughout, operation order of storage.py:63-66; gamma and gamma*tau are
// rounded to float32 once (torch scalar * tensor).
// The one definition of a scan step, used by all four scans (and fa_gae_pivot):
//   delta_t = r + g32 * v_next * m_next - v   and   c_t = gt32 * m_next   depend on the inputs alone,
//   g_t = delta_t + c_t * gae                 is the recurrence; at an episode end the accumulator restarts at +0.0.
__device__ __forceinline__ float fa_gae_delta(float r, float v, float v_next, float m_next, float g32) {
    return r + g32 * v_next * m_next - v;
}
__device__ __forceinline__ float fa_gae_c(float m_next, float gt32) { return gt32 * m_next; }
__device__ __forceinline__ float fa_gae_step(float delta, float c, float gae) { return delta + c * gae; }

#define FA_GAE_CHUNK 16
struct FaGaeChunk { float r[FA_GAE_CHUNK], v[FA_GAE_CHUNK], m[FA_GAE_CHUNK]; uint8_t d[FA_GAE_CHUNK]; };
__global__ __launch_bounds__(64) void fa_gae_kernel(const float *__restrict__ rewards,
                                                    const float *__restrict__ value_preds,
                                                    const float *__restrict__ masks,
                                                    float *__restrict__ returns,
                                                    const uint8_t *__restrict__ done, int T, int E,
                                                    int N, float g32, float gt32) {
    const long long EN = (long long)E * N;
    const long long col = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (col >= EN) return;
    const int e = (int)(col / N);
    float gae = 0.0f;
    float v_next = value_preds[(long long)T * EN + col];
    float m_next = masks[(long long)T * EN + col];
    // The scan is a short dependent chain per step; the loads do not depend on it.  With one wave per
    // SIMD (24 576 columns = 384 waves) the kernel is a sequence of load round trips, so the chunks are
    // software-pipelined: chunk c+1's 4 x 16 loads are in flight while chunk c is scanned out of
    // registers.  Loads are unconditional and clamped (a short-circuit on the done flag becomes a
    // branch + vmcnt(0) per step and serialises the whole chunk).
    auto load = [&](FaGaeChunk &c, int t0) {
#pragma unroll
        for (int k = 0; k < FA_GAE_CHUNK; ++k) {
            const int t = t0 - k;
            const long long o = (long long)(t >= 0 ? t : 0) * EN + col;
            c.r[k] = rewards[o];
            c.v[k] = value_preds[o];
            c.m[k] = masks[o];
            c.d[k] = done[(long long)(t > 0 ? t - 1 : 0) * E + e];
        }
    };
    auto scan = [&](const FaGaeChunk &c, int t0) {
#pragma unroll
        for (int k = 0; k < FA_GAE_CHUNK; ++k) {
            const int t = t0 - k;
            if (t >= 0) {
                const float delta = fa_gae_delta(c.r[k], c.v[k], v_next, m_next, g32);
                const float g = fa_gae_step(delta, fa_gae_c(m_next, gt32), gae);
                if ((t > 0) & (c.d[k] != 0)) {
                    gae = 0.0f;
                } else {
                    gae = g;
                    returns[(long long)t * EN + col] = g + c.v[k];
                }
                v_next = c.v[k];
                m_next = c.m[k];
            }
        }
    };
    FaGaeChunk ca, cb;
    load(ca, T - 1);
    for (int t0 = T - 1; t0 >= 0; t0 -= 2 * FA_GAE_CHUNK) {
        load(cb, t0 - FA_GAE_CHUNK);
        scan(ca, t0);
        load(ca, t0 - 2 * FA_GAE_CHUNK);
        scan(cb, t0 - FA_GAE_CHUNK);
    }
}

// Cooperative form for small batches: at E*N = 24 576 columns the one-wave kernel above has 384
// waves, every wave can keep 63 vector-memory operations in flight (vmcnt), and Little's law pins
// it at ~3 TB/s.  Here a workgroup of four waves shares 64 columns: waves 1..3 stream rewards /
// value_preds / masks + done flags a 32-step chunk ahead into LDS (each with its own queue), wave 0
// scans the previous chunk out of LDS and stores the returns.  Same arithmetic, same order.
// (Two chunks in flight per loader: 3x slower through __syncthreads() in round 2 -- its fence drains
// vmcnt -- and still 18.8 us against 16.0 with raw barriers and statically named register sets in
// round 4 -- in that form the masks + done wave has 128 requests outstanding, twice what a wave can have in
// flight, and every barrier waits for it.)
#define FA_GAEC_CHUNK 32
__global__ __launch_bounds__(256) void fa_gae_coop_kernel(const float *__restrict__ rewards,
                                                          const float *__restrict__ value_preds,
                                                          const float *__restrict__ masks,
                                                          float *__restrict__ returns,
                                                          const uint8_t *__restrict__ done, int T, int E,
                                                          int N, float g32, float gt32) {
    __shared__ float s_r[2][FA_GAEC_CHUNK][64], s_v[2][FA_GAEC_CHUNK][64], s_m[2][FA_GAEC_CHUNK][64];
    __shared__ uint8_t s_d[2][FA_GAEC_CHUNK][64];
    const long long EN = (long long)E * N;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long colv = (long long)blockIdx.x * 64 + lane;
    const bool valid = colv < EN;
    const long long col = valid ? colv : EN - 1; // idle lanes shadow the last column, store nothing
    const int e = (int)(col / N);
    const int nc = (T + FA_GAEC_CHUNK - 1) / FA_GAEC_CHUNK;
    // chunk c holds steps t = T-1 - c*CHUNK - k, k = 0..CHUNK-1 (clamped loads below t = 0)
    auto load_chunk = [&](int c) {
        const int t0 = T - 1 - c * FA_GAEC_CHUNK, b = c & 1;
        if (wave == 3) {
            float x[FA_GAEC_CHUNK];
            uint8_t d[FA_GAEC_CHUNK];
#pragma unroll
            for (int k = 0; k < FA_GAEC_CHUNK; ++k) {
                const int t = t0 - k;
                x[k] = masks[(long long)(t >= 0 ? t : 0) * EN + col];
                d[k] = done[(long long)(t > 0 ? t - 1 : 0) * E + e];
            }
#pragma unroll
            for (int k = 0; k < FA_GAEC_CHUNK; ++k) { s_m[b][k][lane] = x[k]; s_d[b][k][lane] = d[k]; }
        } else {
            const float *src = wave == 1 ? rewards : value_preds;
            float x[FA_GAEC_CHUNK];
#pragma unroll
            for (int k = 0; k < FA_GAEC_CHUNK; ++k) {
                const int t = t0 - k;
                x[k] = src[(long long)(t >= 0 ? t : 0) * EN + col];
            }
            float(*dst)[64] = wave == 1 ? s_r[b] : s_v[b];
#pragma unroll
            for (int k = 0; k < FA_GAEC_CHUNK; ++k) dst[k][lane] = x[k];
        }
    };
    float gae = 0.0f, v_next = 0.0f, m_next = 0.0f;
    if (wave == 0) {
        v_next = value_preds[(long long)T * EN + col];
        m_next = masks[(long long)T * EN + col];
    } else {
        load_chunk(0);
    }
    __syncthreads();
    for (int c = 0; c < nc; ++c) {
        if (wave != 0) {
            if (c + 1 < nc) load_chunk(c + 1);
        } else {
            const int t0 = T - 1 - c * FA_GAEC_CHUNK, b = c & 1;
            // the chunk comes out of LDS in one batch (a read per scan step would put an LDS round
            // trip on every step of the chain)
            float r[FA_GAEC_CHUNK], v[FA_GAEC_CHUNK], m[FA_GAEC_CHUNK];
            uint8_t d[FA_GAEC_CHUNK];
#pragma unroll
            for (int k = 0; k < FA_GAEC_CHUNK; ++k) {
                r[k] = s_r[b][k][lane]; v[k] = s_v[b][k][lane]; m[k] = s_m[b][k][lane]; d[k] = s_d[b][k][lane];
            }
#pragma unroll
            for (int k = 0; k < FA_GAEC_CHUNK; ++k) {
                const int t = t0 - k;
                if (t >= 0) {
                    const float delta = fa_gae_delta(r[k], v[k], v_next, m_next, g32);
                    const float g = fa_gae_step(delta, fa_gae_c(m_next, gt32), gae);
                    if ((t > 0) & (d[k] != 0)) {
                        gae = 0.0f;
                    } else {
                        gae = g;
                        if (valid) returns[(long long)t * EN + col] = g + v[k];
                    }
                    v_next = v[k];
                    m_next = m[k];
                }
            }
        }
        __syncthreads();
    }
}


// ---- the collector tail in two launches: GAE + advantage moments, fold + normalisation --------------
// fa_gae_mom_kernel = a cooperative scan that also leaves the workgroup's one-pass advantage moments
// (ppo.py:121-123): S = sum(A - P), Q = sum((A - P)^2) per agent in fp64, with A = returns[t] - value_preds[t]
// taken in float32 from the value about to be stored -- the returns / value_preds re-read of
// fa_adv_onepass_vec_kernel and its launch disappear.  The entries at the episode ends are left stale by the
// scan (storage.py:59-66 never visits them) but belong to the statistics: their OLD returns (and value_preds)
// are gathered sparsely, FA_GAEC_GATHER per lane and chunk.
//
// Eight waves share 64 columns, split by ROLE so that the one serial chain of the kernel -- g = delta + c * gae,
// then the reset -- has a wave to itself (round 7; before, one wave carried the whole per-step work, 32 instructions
// a step with three exec-mask changes, and the kernel ran at that wave's pace: 20 us against 10 for its loads,
// barriers and stores):
//   waves 1..3  loaders, partitioned by TIME: each fetches rewards / value_preds / masks / done flags for its share
//               of the chunk's steps (plus the one row of overlap for v[t+1], m[t+1]), computes everything that does not
//               depend on the previous step -- delta_t = r + g32 * v_next * m_next - v, c_t = gt32 * m_next, the step's
//               flag (FA_GAES_*); the float32 expressions of fa_gae_kernel in the same order -- and leaves delta, c, the
//               flag and v in LDS.  One chunk in flight per loader, all workgroups walk the step axis together
//               (gae_scan_deep_prefetch.md).
//   wave 0      the scan: reads delta, c, flag of a chunk from LDS in one batch; per step a multiply, an add, a
//               select and the LDS write of g (over delta).  No global memory, no fp64.
//   waves 4, 5  the stores, one chunk behind the scan, even / odd steps: ret = g + v to returns for valid lanes and live
//               steps.  (A wave that stores should not also wait for bulk loads -- collector_tail_fusion.md -- so the
//               stores stay off the loaders.)
//   waves 6, 7  the fp64 moments, one chunk behind the scan, in the accumulation order the one-wave form had: wave 6 is its
//               accumulator pair 0 (even k, descending t; a chunk's first FA_GAEC_GATHER stale entries requested behind the
//               chunk and added at the top of the next, the rare remainder on the spot), wave 7 its pair 1 (odd k); the
//               per-agent fold adds pair 0 + pair 1 per lane as before.  (All of this on ONE post wave: 29.4 us -- the work
//               of a step is independent of the other steps, but at 8-9 cycles per instruction of such code a single wave
//               needs 150 ns for it.)
// A chunk passes through three trips: loaded in trip c, scanned in trip c + 1, posted in trip c + 2; every role runs
// fa_gaes_trips(nc) trips with one barrier each.  The workgroup barrier is a raw s_barrier behind an LDS wait, not
// __syncthreads(): loads, stores and gathers stay in flight across it.  Rows are addressed through buffer descriptors
// (scalar row offset + the lane's 32-bit byte offset).
// Pivot P_i: agent i's first GAE term of env 0, from the inputs alone, so that every workgroup and the
// fold agree on it without a grid-wide exchange (any sample-sized value does: it only keeps S*S/n from
// cancelling against Q).
#define FA_GAEC_GATHER 4
// the workgroup barrier between trips: LDS traffic complete, then s_barrier.  NOT __syncthreads(): its fence also
// waits for every global load and store in flight (vmcnt(0)) -- the loaders' next chunks, the store waves'
// stores, the gathers -- which is what pinned the first form of this kernel to one chunk in flight and a store drain per chunk.
#define FA_GAEC_BARRIER() asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory")
__device__ __forceinline__ float fa_gae_pivot(const float *__restrict__ rewards, const float *__restrict__ value_preds,
                                              const float *__restrict__ masks, int T, long long EN, int i, float g32) {
    const long long o = (long long)(T - 1) * EN + i, o1 = (long long)T * EN + i;
    const float vp = value_preds[o];
    const float delta = fa_gae_delta(rewards[o], vp, value_preds[o1], masks[o1], g32);
    return (delta + vp) - vp;
}
// The one-pass accumulation around a pivot, used by the moment waves and by the fa_adv_onepass*_kernel sweeps: the deviation
// of a float32 advantage (returns - value_preds, subtracted in float32 as the reference does) from the pivot, S += dd,
// Q = fma(dd, dd, Q), all in fp64.
__device__ __forceinline__ double fa_mom_dev(float adv, double piv) { return (double)adv - piv; }
__device__ __forceinline__ void fa_mom_add(double dd, double &S, double &Q) {
    S += dd;
    Q = __fma_rn(dd, dd, Q);
}

// The roles' shared arithmetic.  Loader l owns the steps k in [fa_gaes_first(l), fa_gaes_first(l + 1)) of every chunk.
#define FA_GAES_LOADERS 3
#define FA_GAES_THREADS (64 * (FA_GAES_LOADERS + 5)) // the scan, the loaders, two store waves, two moment waves
// a step's flag byte in LDS
#define FA_GAES_LIVE 0   // returns[t] is computed and stored, the advantage enters the moments
#define FA_GAES_STALE 1  // t > 0 && done[t-1]: the accumulator restarts, returns[t] keeps its old value, which enters the moments
#define FA_GAES_BELOW 2  // t < 0 (behind the last chunk's real steps): nothing
constexpr int fa_gaes_first(int l) { return (l * FA_GAEC_CHUNK + FA_GAES_LOADERS - 1) / FA_GAES_LOADERS; }
constexpr bool fa_gaes_one_owner_per_step() {
    for (int k = 0; k < FA_GAEC_CHUNK; ++k) {
        int owners = 0;
        for (int l = 0; l < FA_GAES_LOADERS; ++l) owners += (k >= fa_gaes_first(l) && k < fa_gaes_first(l + 1)) ? 1 : 0;
        if (owners != 1) return false;
    }
    return true;
}
// requests a loader has in flight: n rewards + n done flags + (n + 1) value_preds + (n + 1) masks
constexpr int fa_gaes_max_requests() {
    int most = 0;
    for (int l = 0; l < FA_GAES_LOADERS; ++l) {
        const int n = fa_gaes_first(l + 1) - fa_gaes_first(l);
        most = 4 * n + 2 > most ? 4 * n + 2 : most;
    }
    return most;
}
static_assert(fa_gaes_one_owner_per_step(), "every step of a chunk has exactly one loader");
static_assert(fa_gaes_max_requests() <= 63, "a wave has at most 63 vector-memory requests in flight (vmcnt)");
// trip j: chunk j is loaded, chunk j - 1 scanned, chunk j - 2 posted (-1: the role idles, but still meets the barrier)
__device__ __forceinline__ int fa_gaes_trips(int nc) { return nc + 2; }
__device__ __forceinline__ int fa_gaes_load_chunk(int j, int nc) { return j < nc ? j : -1; }
__device__ __forceinline__ int fa_gaes_scan_chunk(int j, int nc) { return (j >= 1 && j - 1 < nc) ? j - 1 : -1; }
__device__ __forceinline__ int fa_gaes_post_chunk(int j, int nc) { return (j >= 2 && j - 2 < nc) ? j - 2 : -1; }
template <int L> struct FaGaesLoader { static constexpr int first = fa_gaes_first(L), n = fa_gaes_first(L + 1) - fa_gaes_first(L); };
template <int P> struct FaGaesParity { static constexpr int value = P; };

__global__ __launch_bounds__(FA_GAES_THREADS) void fa_gae_mom_kernel(const float *__restrict__ rewards,
                                                                     const float *__restrict__ value_preds,
                                                                     const float *__restrict__ masks, float *__restrict__ returns,
                                                                     const uint8_t *__restrict__ done, int T, int E, int N, float g32,
                                                                     float gt32, double *__restrict__ partial) {
    // [stage][step][column], 4-byte elements (and a byte per flag).  A chunk's delta is overwritten by its g in place; c
    // lives from the load to the scan only: two stages.  70 KB + the fold's 2 KB: two workgroups per CU.
    __shared__ float s_g[3][FA_GAEC_CHUNK][64], s_v[3][FA_GAEC_CHUNK][64], s_c[2][FA_GAEC_CHUNK][64];
    __shared__ uint8_t s_f[3][FA_GAEC_CHUNK][64];
    __shared__ double s_sq[2][2][64];  // [accumulator pair][S, Q][column]
    const long long EN = (long long)E * N;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6); // wave: in a scalar register
    const long long colv = (long long)blockIdx.x * 64 + lane;
    const bool valid = colv < EN;
    const long long col = valid ? colv : EN - 1; // idle lanes shadow the last column, store nothing
    const int e = (int)(col / N);
    const int nc = (T + FA_GAEC_CHUNK - 1) / FA_GAEC_CHUNK;
    const int trips = fa_gaes_trips(nc);
    // chunk c holds steps t = T-1 - c*CHUNK - k, k = 0..CHUNK-1 (clamped loads below t = 0)
    // Rows are addressed through buffer descriptors: a wave-uniform row offset in a scalar register + the lane's
    // 32-bit byte offset.  (As 64-bit vector addresses the loads a loader keeps in flight cost it two registers each.)
    // Offsets fit 32 bits: (T + 1) * EN * 4 < 2^31 on this path.
    const unsigned rowb = (unsigned)EN * 4u;                                    // bytes per step of a (T, E, N) tensor
    const unsigned coff = (unsigned)col * 4u;
    auto rsrc = [&](const void *p, unsigned bytes) {
        return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(p), 0, (int)bytes, 0x00020000);
    };
    const __amdgpu_buffer_rsrc_t rs_rew = rsrc(rewards, (unsigned)T * rowb);
    const __amdgpu_buffer_rsrc_t rs_val = rsrc(value_preds, (unsigned)(T + 1) * rowb);
    const __amdgpu_buffer_rsrc_t rs_msk = rsrc(masks, (unsigned)(T + 1) * rowb);
    const __amdgpu_buffer_rsrc_t rs_ret = rsrc(returns, (unsigned)(T + 1) * rowb);
    const __amdgpu_buffer_rsrc_t rs_done = rsrc(done, (unsigned)T * (unsigned)E);
    auto ldf = [&](const __amdgpu_buffer_rsrc_t &rs, unsigned voff, unsigned soff) -> float {
        // (readfirstlane: the row offset IS uniform, but computed with a vector clamp it gets a waterfall loop per load)
        return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, (int)voff, __builtin_amdgcn_readfirstlane((int)soff), 0));
    };
    if (wave >= 1 && wave <= FA_GAES_LOADERS) {
        // ---- loaders (every role runs its own copy of the trip loop, each with its own barrier instruction: the counts match,
        // all from fa_gaes_trips)
        auto load_chunk = [&](auto who, int c) {
            constexpr int k0 = decltype(who)::first, n = decltype(who)::n;
            const int t0 = T - 1 - c * FA_GAEC_CHUNK - k0;  // the loader's first (latest) step
            float v[n + 1], m[n + 1], r[n];                  // v[i], m[i]: row t0 + 1 - i; r[i]: row t0 - i
            uint8_t d[n];
#pragma unroll
            for (int i = 0; i <= n; ++i) {
                const int t = t0 + 1 - i;
                const unsigned so = (unsigned)(t >= 0 ? t : 0) * rowb;
                v[i] = ldf(rs_val, coff, so);
                m[i] = ldf(rs_msk, coff, so);
                if (i < n) {
                    r[i] = ldf(rs_rew, coff, (unsigned)(t >= 1 ? t - 1 : 0) * rowb);
                    d[i] = __builtin_amdgcn_raw_buffer_load_b8(rs_done, e, __builtin_amdgcn_readfirstlane((int)((unsigned)(t >= 2 ? t - 2 : 0) * (unsigned)E)), 0);
                }
            }
            const int b3 = c % 3, b2 = c & 1;
#pragma unroll
            for (int i = 0; i < n; ++i) {
                const int t = t0 - i;
                s_g[b3][k0 + i][lane] = fa_gae_delta(r[i], v[i + 1], v[i], m[i], g32);   // v[i], m[i]: the step's v_next, m_next
                s_c[b2][k0 + i][lane] = fa_gae_c(m[i], gt32);
                s_v[b3][k0 + i][lane] = v[i + 1];
                s_f[b3][k0 + i][lane] = t < 0 ? FA_GAES_BELOW : (((t > 0) & (d[i] != 0)) ? FA_GAES_STALE : FA_GAES_LIVE);
            }
        };
        auto run = [&](auto who) {
            for (int j = 0; j < trips; ++j) {
                const int c = fa_gaes_load_chunk(j, nc);
                if (c >= 0) load_chunk(who, c);
                FA_GAEC_BARRIER();
            }
        };
        static_assert(FA_GAES_LOADERS == 3, "one branch per loader below");
        if (wave == 1) run(FaGaesLoader<0>());
        else if (wave == 2) run(FaGaesLoader<1>());
        else run(FaGaesLoader<2>());
    } else if (wave == 0) {
        // ---- the scanning wave: the recurrence and nothing else
        float gae = 0.0f;
        for (int j = 0; j < trips; ++j) {
            const int c = fa_gaes_scan_chunk(j, nc);
            if (c >= 0) {
                const int b3 = c % 3, b2 = c & 1;
                // the chunk comes out of LDS in one batch (a read per scan step would put an LDS round
                // trip on every step of the chain); steps below t = 0 in the last chunk run on clamped rows, behind every real one
                float dl[FA_GAEC_CHUNK], cc[FA_GAEC_CHUNK];
                uint8_t f[FA_GAEC_CHUNK];
#pragma unroll
                for (int k = 0; k < FA_GAEC_CHUNK; ++k) { dl[k] = s_g[b3][k][lane]; cc[k] = s_c[b2][k][lane]; f[k] = s_f[b3][k][lane]; }
#pragma unroll
                for (int k = 0; k < FA_GAEC_CHUNK; ++k) {
                    const float g = fa_gae_step(dl[k], cc[k], gae);
                    s_g[b3][k][lane] = g;
                    gae = f[k] != FA_GAES_LIVE ? 0.0f : g;   // a select: the reset is exactly +0.0
                }
            }
            FA_GAEC_BARRIER();
        }
    } else if (wave < FA_GAES_LOADERS + 3) {
        // ---- the store waves: steps k = 2 i + par of the chunk behind the scan
        const int par = wave - (FA_GAES_LOADERS + 1);
        for (int j = 0; j < trips; ++j) {
            const int c = fa_gaes_post_chunk(j, nc);
            if (c >= 0) {
                const int t0 = T - 1 - c * FA_GAEC_CHUNK - par, b3 = c % 3;
                float g[FA_GAEC_CHUNK / 2], v[FA_GAEC_CHUNK / 2];
                uint8_t f[FA_GAEC_CHUNK / 2];
#pragma unroll
                for (int i = 0; i < FA_GAEC_CHUNK / 2; ++i) {
                    g[i] = s_g[b3][2 * i + par][lane]; v[i] = s_v[b3][2 * i + par][lane]; f[i] = s_f[b3][2 * i + par][lane];
                }
#pragma unroll
                for (int i = 0; i < FA_GAEC_CHUNK / 2; ++i) {
                    const int t = t0 - 2 * i;   // f == 0 implies t >= 0
                    const float ret = g[i] + v[i];
                    if (valid & (f[i] == FA_GAES_LIVE)) __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, ret), rs_ret, (int)coff, __builtin_amdgcn_readfirstlane((int)((unsigned)t * rowb)), 0);
                }
            }
            FA_GAEC_BARRIER();
        }
    } else {
        // ---- the moment waves: accumulator pair `par` of the one-wave form, i.e. the steps k = 2 i + par in descending t; pair 0
        // also takes the stale entries.  A skipped step adds +0.0 to S and fma(0, 0, Q) to Q: neither changes a bit (the sums start at
        // +0.0 and never become -0.0), so the chain has no branch.
        auto run = [&](auto parity) {
            constexpr int par = decltype(parity)::value;
            double accS = 0.0, accQ = 0.0;
            const double piv = (double)fa_gae_pivot(rewards, value_preds, masks, T, EN, (int)(col % N), g32);
            auto add_stale = [&](float o, float v) {
                const double dd = fa_mom_dev(o - v, piv);
                fa_mom_add(dd, accS, accQ);
            };
            float go[FA_GAEC_GATHER], gv[FA_GAEC_GATHER]; // the previous chunk's requested stale entries: old returns, value_preds
            unsigned gmask = 0u;                            // ... which of them are real
#pragma unroll
            for (int j = 0; j < FA_GAEC_GATHER; ++j) { go[j] = 0.0f; gv[j] = 0.0f; }
            for (int j = 0; j < trips; ++j) {
                const int c = fa_gaes_post_chunk(j, nc);
                if (c >= 0) {
                    const int t0 = T - 1 - c * FA_GAEC_CHUNK, b3 = c % 3;
                    if (par == 0) {
#pragma unroll
                        for (int q = 0; q < FA_GAEC_GATHER; ++q)   // requested behind the previous chunk: a barrier's time to arrive
                            if ((gmask >> q) & 1u) add_stale(go[q], gv[q]);
                    }
                    float g[FA_GAEC_CHUNK / 2], v[FA_GAEC_CHUNK / 2];
                    uint8_t f[FA_GAEC_CHUNK];
#pragma unroll
                    for (int i = 0; i < FA_GAEC_CHUNK / 2; ++i) { g[i] = s_g[b3][2 * i + par][lane]; v[i] = s_v[b3][2 * i + par][lane]; }
#pragma unroll
                    for (int k = 0; k < FA_GAEC_CHUNK; ++k) f[k] = (par == 0 || (k & 1) == par) ? s_f[b3][k][lane] : 0;
#pragma unroll
                    for (int i = 0; i < FA_GAEC_CHUNK / 2; ++i) {
                        const float ret = g[i] + v[i];
                        const double d0 = fa_mom_dev(ret - v[i], piv);
                        const double dd = f[2 * i + par] == FA_GAES_LIVE ? d0 : 0.0;
                        fa_mom_add(dd, accS, accQ);
                    }
                    if (par == 0) {
                        // the chunk's stale entries (a few per cent of all): old returns and value_preds straight from memory.  The
                        // first FA_GAEC_GATHER per lane are only REQUESTED here and added at the top of the next chunk -- the raw barrier
                        // leaves them in flight, and waiting for them here would hold the whole workgroup's barrier back by a memory
                        // round trip per chunk -- the rest (rare) in a loop on the spot.
                        unsigned rem = 0u;
#pragma unroll
                        for (int k = 0; k < FA_GAEC_CHUNK; ++k) rem |= (f[k] == FA_GAES_STALE ? 1u : 0u) << k;
                        gmask = 0u;
#pragma unroll
                        for (int q = 0; q < FA_GAEC_GATHER; ++q) {
                            const int k = rem ? __builtin_ctz(rem) : 0;
                            gmask |= (rem ? 1u : 0u) << q;
                            rem &= rem - 1u;
                            const unsigned o = (unsigned)(t0 - k) * rowb + coff; // t0 - k >= 1 for a stale k, t0 >= 0 otherwise
                            go[q] = ldf(rs_ret, o, 0u);
                            gv[q] = ldf(rs_val, o, 0u);
                        }
                        while (__builtin_amdgcn_ballot_w64(rem != 0u) != 0ull) {
                            const bool has = rem != 0u;
                            const int k = has ? __builtin_ctz(rem) : 0;
                            rem &= rem - 1u;
                            const unsigned o = (unsigned)(t0 - k) * rowb + coff;
                            const float o_ = ldf(rs_ret, o, 0u), v_ = ldf(rs_val, o, 0u);
                            if (has) add_stale(o_, v_);
                        }
                    }
                }
                FA_GAEC_BARRIER();
            }
            if (par == 0) {
#pragma unroll
                for (int q = 0; q < FA_GAEC_GATHER; ++q)   // the last chunk's
                    if ((gmask >> q) & 1u) add_stale(go[q], gv[q]);
            }
            s_sq[par][0][lane] = valid ? accS : 0.0;
            s_sq[par][1][lane] = valid ? accQ : 0.0;
        };
        if (wave == FA_GAES_LOADERS + 3) run(FaGaesParity<0>());
        else run(FaGaesParity<1>());
    }
    {
        __syncthreads();
        // partial[block][agent] = {S, Q}: the lanes of an agent in ascending order
        if ((int)threadIdx.x < 2 * N) {
            const int i = threadIdx.x >> 1, cmp = threadIdx.x & 1;
            const int first = (int)(((long long)blockIdx.x * 64) % N); // agent of lane 0
            double acc = 0.0;
            for (int l = (i - first + N) % N; l < 64; l += N) acc += s_sq[0][cmp][l] + s_sq[1][cmp][l];
            partial[((long long)blockIdx.x * N + i) * 2 + cmp] = acc;
        }
    }
}

// One wave folds agent i's partials: lane l takes workgroups l, l + 64, ... in order (16-byte loads,
// issued together), then a fixed shuffle tree; every lane returns the same (mean, M2).  Used by the
// one-workgroup fold AND by every workgroup of the fused normalisation, so both produce the same bits.
#define FA_GAEM_FOLD 8 // partial workgroups per lane: nblocks <= 64 * FA_GAEM_FOLD
__device__ __forceinline__ void fa_gae_mom_fold(const double *__restrict__ partial, int nblocks, int N, int i, int lane,
                                                double n_rows, double piv, double &mean, double &m2) {
    const double2 *p2 = reinterpret_cast<const double2 *>(partial);
    double2 p[FA_GAEM_FOLD];
#pragma unroll
    for (int k = 0; k < FA_GAEM_FOLD; ++k) {
        const int b = lane + 64 * k;
        p[k] = p2[(long long)(b < nblocks ? b : 0) * N + i];
    }
    double s = 0.0, q = 0.0;
#pragma unroll
    for (int k = 0; k < FA_GAEM_FOLD; ++k) {
        const bool in = lane + 64 * k < nblocks;
        s += in ? p[k].x : 0.0;
        q += in ? p[k].y : 0.0;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { s += __shfl_down(s, off, 64); q += __shfl_down(q, off, 64); }
    s = __shfl(s, 0, 64);
    q = __shfl(q, 0, 64);
    mean = piv + s / n_rows;
    m2 = q - s * (s / n_rows);
}

// The pivot the partials were accumulated around.  piv_from_returns = 0: fa_gae_mom_kernel's, from the scan's inputs;
// 1: fa_adv_onepass[_vec]_kernel's (shapes beyond the fused scan), agent i's advantage in row 0 AFTER the scan.
__device__ __forceinline__ double fa_row0_pivot(const float *__restrict__ returns, const float *__restrict__ value_preds, int i) {
    return (double)(returns[i] - value_preds[i]);
}
__device__ __forceinline__ double fa_partials_pivot(int piv_from_returns, const float *__restrict__ rewards,
                                                    const float *__restrict__ value_preds, const float *__restrict__ masks,
                                                    const float *__restrict__ returns, int T, long long EN, int i, float g32) {
    return piv_from_returns ? fa_row0_pivot(returns, value_preds, i)
                            : (double)fa_gae_pivot(rewards, value_preds, masks, T, EN, i, g32);
}

// Chan-Golub-LeVeque merge of agent i's per-rank (n, mean, M2) triples in rank order: exact combination of two-pass
// statistics, the same bits on every rank and in every workgroup.  gathered: (W, N, 3).
__device__ __forceinline__ void fa_merge_ranks(const double *__restrict__ gathered, int W, int N, int i, double &n, double &mean,
                                               double &m2) {
    n = 0.0; mean = 0.0; m2 = 0.0;
    for (int r = 0; r < W; ++r) {
        const double *g = gathered + ((long long)r * N + i) * 3;
        const double nr = g[0], mr = g[1], m2r = g[2];
        if (nr <= 0.0) continue;
        const double nn = n + nr, delta = mr - mean;
        mean += delta * (nr / nn);
        m2 += m2r + delta * delta * (n * nr / nn);
        n = nn;
    }
}

// ppo.py:123: (A - mean) / (std + 1e-5), float32 arithmetic with float32 mean / std; A = returns - value_preds in float32.
__device__ __forceinline__ float fa_norm_den(double sd) { return (float)sd + 1e-5f; }
__device__ __forceinline__ float fa_norm_adv(float ret, float v, float mean, float den) { return (ret - v - mean) / den; }

// One workgroup folds the partials of the fused scan or of the one-pass sweep (piv_from_returns, see fa_partials_pivot).
__global__ void fa_gae_mom_final_kernel(const double *__restrict__ partial, int nblocks, int N,
                                        const float *__restrict__ rewards, const float *__restrict__ value_preds,
                                        const float *__restrict__ masks, const float *__restrict__ returns, int T, long long EN,
                                        float g32, double n_rows, double *__restrict__ moments_out,
                                        double *__restrict__ mean_out, double *__restrict__ std_out, int piv_from_returns) {
    const int i = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (i >= N) return;
    const double piv = fa_partials_pivot(piv_from_returns, rewards, value_preds, masks, returns, T, EN, i, g32);
    double mean, m2;
    fa_gae_mom_fold(partial, nblocks, N, i, lane, n_rows, piv, mean, m2);
    if (lane == 0) {
        if (moments_out) { moments_out[i * 3 + 0] = n_rows; moments_out[i * 3 + 1] = mean; moments_out[i * 3 + 2] = m2; }
        if (mean_out) mean_out[i] = mean;
        if (std_out) std_out[i] = sqrt(m2 / (n_rows - 1.0));
    }
}

// The fold and ppo.py:123 in one launch (one rank: nothing is exchanged between them): every workgroup
// folds the partials itself -- one wave per agent, 6 KB per agent out of L2 at config 2 -- and normalises its
// share of the advantages, 16 bytes per lane and trip, the first trip requested ahead of the fold.  The normalising expression
// is fa_adv_norm_kernel's (fa_norm_adv); workgroup 0 also leaves moments / mean / std.  `total` = T*E*N.
// The statistics come from one of three sources, named on the host by FaStatSource (fa_launch_gae_mom_norm).
__global__ __launch_bounds__(512) void fa_gae_mom_norm_kernel(const double *__restrict__ partial, int nblocks, int N,
                                                              const float *__restrict__ rewards,
                                                              const float *__restrict__ value_preds,
                                                              const float *__restrict__ masks,
                                                              const float *__restrict__ returns, int T, long long EN, float g32,
                                                              double n_rows, long long total, float *__restrict__ out,
                                                              double *__restrict__ moments_out, double *__restrict__ mean_out,
                                                              double *__restrict__ std_out, int piv_from_returns,
                                                              const double *__restrict__ gathered, int W) {
    // gathered != null (several ranks): no fold -- every workgroup merges the W ranks' (n, mean, M2) triples as fa_adv_merge_kernel
    // does (one lane per agent, fa_merge_ranks) and normalises with the result.
    // piv_from_returns: the partials are the one-pass sweep's; same {S, Q} layout, same fold (fa_partials_pivot)
    __shared__ float s_mean[FA_MAX_AGENTS_DEV], s_den[FA_MAX_AGENTS_DEV];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long stride = (long long)gridDim.x * blockDim.x;
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long quads = total / 4;
    const bool vec = (((uintptr_t)returns | (uintptr_t)value_preds | (uintptr_t)out) & 15) == 0;
    const float4 *r4 = reinterpret_cast<const float4 *>(returns), *v4 = reinterpret_cast<const float4 *>(value_preds);
    // the lane's first trip is requested before the fold: its round trip and the fold's run side by side
    float4 ra = make_float4(0.f, 0.f, 0.f, 0.f), va = ra, rb = ra, vb = ra;
    if (vec && gid < quads) {
        const long long q1 = gid + stride;
        ra = r4[gid]; va = v4[gid];
        rb = r4[q1 < quads ? q1 : gid]; vb = v4[q1 < quads ? q1 : gid];
    }
    if (gathered) {
        if ((int)threadIdx.x < N) {
            const int i = threadIdx.x;
            double n, mean, m2;
            fa_merge_ranks(gathered, W, N, i, n, mean, m2);
            const double sd = sqrt(m2 / (n - 1.0));
            s_mean[i] = (float)mean;
            s_den[i] = fa_norm_den(sd);
            if (blockIdx.x == 0) {
                if (mean_out) mean_out[i] = mean;
                if (std_out) std_out[i] = sd;
            }
        }
    } else
    for (int i = wave; i < N; i += 8) { // eight waves: one agent each up to 4v4, one round trip
        const double piv = fa_partials_pivot(piv_from_returns, rewards, value_preds, masks, returns, T, EN, i, g32);
        double mean, m2;
        fa_gae_mom_fold(partial, nblocks, N, i, lane, n_rows, piv, mean, m2);
        const double sd = sqrt(m2 / (n_rows - 1.0));
        if (lane == 0) {
            s_mean[i] = (float)mean;
            s_den[i] = fa_norm_den(sd);
            if (blockIdx.x == 0) {
                if (moments_out) { moments_out[i * 3 + 0] = n_rows; moments_out[i * 3 + 1] = mean; moments_out[i * 3 + 2] = m2; }
                if (mean_out) mean_out[i] = mean;
                if (std_out) std_out[i] = sd;
            }
        }
    }
    __syncthreads();
    if (vec) {
        float4 *o4 = reinterpret_cast<float4 *>(out);
        // write-through (sc1) 16-byte stores: nothing of `out` stays dirty in L2 for the kernel boundary behind this launch to
        // flush (29.4 against 30.1 us for the two launches, 177.4 against 178.4 behind the rollout; 16-byte sc1 stores cost what
        // plain ones do -- the 8-byte observation rows of the step kernel as sc1 stores: slower, 180.0 against 177.8)
        typedef int v4i __attribute__((ext_vector_type(4)));
        const bool small = total * 4 < (1LL << 31); // buffer offsets are 32 bits
        const __amdgpu_buffer_rsrc_t rs_out = __builtin_amdgcn_make_buffer_rsrc(out, 0, small ? (int)(total * 4) : 0, 0x00020000);
        auto st4 = [&](long long q, const float4 &v) {
            if (small) {
                v4i w = {__builtin_bit_cast(int, v.x), __builtin_bit_cast(int, v.y), __builtin_bit_cast(int, v.z), __builtin_bit_cast(int, v.w)};
                __builtin_amdgcn_raw_buffer_store_b128(w, rs_out, (int)(q * 16), 0, 16);
            } else {
                o4[q] = v;
            }
        };
        for (long long q0 = gid; q0 < quads; q0 += 2 * stride) {
            const long long q1 = q0 + stride;
            const bool two = q1 < quads;
            if (q0 != gid) {
                ra = r4[q0]; va = v4[q0];
                rb = r4[two ? q1 : q0]; vb = v4[two ? q1 : q0];
            }
            auto norm4 = [&](const float4 &r, const float4 &v, long long q) {
                int i = (int)((4 * q) % N);
                float4 o;
                o.x = fa_norm_adv(r.x, v.x, s_mean[i], s_den[i]); i = i + 1 == N ? 0 : i + 1;
                o.y = fa_norm_adv(r.y, v.y, s_mean[i], s_den[i]); i = i + 1 == N ? 0 : i + 1;
                o.z = fa_norm_adv(r.z, v.z, s_mean[i], s_den[i]); i = i + 1 == N ? 0 : i + 1;
                o.w = fa_norm_adv(r.w, v.w, s_mean[i], s_den[i]);
                return o;
            };
            st4(q0, norm4(ra, va, q0));
            if (two) st4(q1, norm4(rb, vb, q1));
        }
        for (long long k = quads * 4 + gid; k < total; k += stride) {
            const int i = (int)(k % N);
            out[k] = fa_norm_adv(returns[k], value_preds[k], s_mean[i], s_den[i]);
        }
    } else {
        for (long long k = gid; k < total; k += stride) {
            const int i = (int)(k % N);
            out[k] = fa_norm_adv(returns[k], value_preds[k], s_mean[i], s_den[i]);
        }
    }
}

// Four adjacent columns per lane: 16-byte loads (1 KiB per wave instruction instead of
// 256 B) and four independent scan chains per lane.  Same arithmetic per column as above.
#define FA_GAE4_CHUNK 16
__global__ __launch_bounds__(64) void fa_gae4_kernel(const float *__restrict__ rewards,
                                                     const float *__restrict__ value_preds,
                                                     const float *__restrict__ masks,
                                                     float *__restrict__ returns,
                                                     const uint8_t *__restrict__ done, int T, int E,
                                                     int N, float g32, float gt32) {
    const long long EN = (long long)E * N;
    const long long col = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (col >= EN) return;
    int e[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) e[q] = (int)((col + q) / N);
    float gae[4] = {0.f, 0.f, 0.f, 0.f};
    float4 v_next = *reinterpret_cast<const float4 *>(value_preds + (long long)T * EN + col);
    float4 m_next = *reinterpret_cast<const float4 *>(masks + (long long)T * EN + col);
    for (int t0 = T - 1; t0 >= 0; t0 -= FA_GAE4_CHUNK) {
        float4 r[FA_GAE4_CHUNK], v[FA_GAE4_CHUNK], m[FA_GAE4_CHUNK];
        unsigned skip[FA_GAE4_CHUNK];
#pragma unroll
        for (int k = 0; k < FA_GAE4_CHUNK; ++k) {
            const int t = t0 - k;
            const bool in = t >= 0;
            const long long o = (long long)(in ? t : 0) * EN + col;
            r[k] = *reinterpret_cast<const float4 *>(rewards + o);
            v[k] = *reinterpret_cast<const float4 *>(value_preds + o);
            m[k] = *reinterpret_cast<const float4 *>(masks + o);
            unsigned sk = 0;
            const uint8_t *d = done + (long long)(t > 0 ? t - 1 : 0) * E;
#pragma unroll
            for (int q = 0; q < 4; ++q) sk |= ((unsigned)(t > 0) & (unsigned)(d[e[q]] != 0)) << q;
            skip[k] = sk;
        }
#pragma unroll
        for (int k = 0; k < FA_GAE4_CHUNK; ++k) {
            const int t = t0 - k;
            if (t >= 0) {
                const float rr[4] = {r[k].x, r[k].y, r[k].z, r[k].w};
                const float vv[4] = {v[k].x, v[k].y, v[k].z, v[k].w};
                const float vn[4] = {v_next.x, v_next.y, v_next.z, v_next.w};
                const float mn[4] = {m_next.x, m_next.y, m_next.z, m_next.w};
                float out[4];
                float *ret = returns + (long long)t * EN + col;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float delta = fa_gae_delta(rr[q], vv[q], vn[q], mn[q], g32);
                    const float g = fa_gae_step(delta, fa_gae_c(mn[q], gt32), gae[q]);
                    const bool sk = (skip[k] >> q) & 1u;
                    gae[q] = sk ? 0.0f : g;
                    out[q] = g + vv[q];
                }
                if (skip[k] == 0u) {
                    *reinterpret_cast<float4 *>(ret) = make_float4(out[0], out[1], out[2], out[3]);
                } else {
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        if (!((skip[k] >> q) & 1u)) ret[q] = out[q];
                }
                v_next = v[k];
                m_next = m[k];
            }
        }
    }
}

// rlcore/algo/ppo.py:121-123 statistics.  A = returns[t] - value_preds[t] (float32
// subtraction as in the reference), accumulated in fp64.  Stage 1: per-workgroup
// partial sums per agent, fixed order; stage 2: one workgroup folds the partials in a
// fixed order => bitwise reproducible run to run.
// partial layout: [block][N][2] = {sum, sum_sq_dev}
template <int PASS>
__global__ __launch_bounds__(256) void fa_adv_partial_kernel(const float *__restrict__ returns,
                                                             const float *__restrict__ value_preds,
                                                             const double *__restrict__ mean, long long rows,
                                                             int N, double *__restrict__ partial) {
    __shared__ double red[4][FA_MAX_AGENTS_DEV];
    double acc[FA_MAX_AGENTS_DEV];
#pragma unroll
    for (int i = 0; i < FA_MAX_AGENTS_DEV; ++i) acc[i] = 0.0;
    double mu[FA_MAX_AGENTS_DEV];
#pragma unroll
    for (int i = 0; i < FA_MAX_AGENTS_DEV; ++i) mu[i] = (PASS == 1 && i < N) ? mean[i] : 0.0;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x; r < rows; r += stride) {
        const float *ret = returns + r * N, *vp = value_preds + r * N;
#pragma unroll
        for (int i = 0; i < FA_MAX_AGENTS_DEV; ++i) {
            if (i < N) {
                const double adv = (double)(ret[i] - vp[i]);
                if (PASS == 0) acc[i] += adv;
                else { const double d = adv - mu[i]; acc[i] += d * d; }
            }
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < FA_MAX_AGENTS_DEV; ++i) {
        double v = acc[i];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
        if (lane == 0) red[wave][i] = v;
    }
    __syncthreads();
    if (threadIdx.x < N) {
        const int i = threadIdx.x;
        partial[((long long)blockIdx.x * N + i)] = ((red[0][i] + red[1][i]) + red[2][i]) + red[3][i];
    }
}

// Same reduction for a compile-time even N with 16-byte loads: a lane takes two whole rows
// (2N floats = N/2 float4, 48 B at N = 6) per trip, so the agent of every loaded element is a
// compile-time constant and the wave reads one contiguous span.  (The row-per-lane kernel above
// issues N scalar loads with a 4N-byte lane stride and reaches only ~1.5 TB/s.)
template <int PASS, int TN>
__global__ __launch_bounds__(256) void fa_adv_partial_vec_kernel(const float *__restrict__ returns,
                                                                 const float *__restrict__ value_preds,
                                                                 const double *__restrict__ mean, long long row_pairs,
                                                                 double *__restrict__ partial) {
    constexpr int NV = TN / 2; // float4 per row pair
    __shared__ double red[4][TN];
    double acc[TN], mu[TN];
#pragma unroll
    for (int i = 0; i < TN; ++i) { acc[i] = 0.0; mu[i] = PASS == 1 ? mean[i] : 0.0; }
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < row_pairs; p += stride) {
        const float4 *r4 = reinterpret_cast<const float4 *>(returns + p * 2 * TN);
        const float4 *v4 = reinterpret_cast<const float4 *>(value_preds + p * 2 * TN);
        float4 rr[NV], vv[NV];
#pragma unroll
        for (int q = 0; q < NV; ++q) { rr[q] = r4[q]; vv[q] = v4[q]; }
#pragma unroll
        for (int q = 0; q < NV; ++q) {
            const float a4[4] = {rr[q].x - vv[q].x, rr[q].y - vv[q].y, rr[q].z - vv[q].z, rr[q].w - vv[q].w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int i = (4 * q + j) % TN; // folds to a constant after unrolling
                const double adv = (double)a4[j];
                if (PASS == 0) acc[i] += adv;
                else { const double d = adv - mu[i]; acc[i] += d * d; }
            }
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < TN; ++i) {
        double v = acc[i];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
        if (lane == 0) red[wave][i] = v;
    }
    __syncthreads();
    if (threadIdx.x < TN) {
        const int i = threadIdx.x;
        partial[((long long)blockIdx.x * TN + i)] = ((red[0][i] + red[1][i]) + red[2][i]) + red[3][i];
    }
}

// ---- advantage moments in ONE pass ---------------------------------------------------------------
// (n, mean, M2) per agent from a single sweep over returns / value_preds: every lane accumulates
// S = sum(A - P) and Q = sum((A - P)^2) in fp64 around a pivot P_i common to the whole grid -- agent
// i's advantage in row 0, an actual sample, so that S*S/n does not cancel against Q -- the workgroup
// folds its lanes into partial[block][i] = {S, Q}, and a one-workgroup kernel folds the workgroups in
// a fixed order: mean = P + S/n, M2 = Q - S*S/n.  Bitwise reproducible; relative error of M2 ~
// 1e-16 * (1 + ((P - mean)/std)^2) times the accumulation factor.  (Folding in the same launch by
// the last workgroup to finish -- ticket counter + device-scope fences -- measured 10x slower: an
// agent-scope release / acquire is an L2 write-back / invalidate on this multi-XCD part.)
__device__ __forceinline__ void fa_adv_onepass_finish(double (&acc_s)[FA_MAX_AGENTS_DEV], double (&acc_q)[FA_MAX_AGENTS_DEV],
                                                      int N, double *__restrict__ partial) {
    __shared__ double red[4][FA_MAX_AGENTS_DEV][2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < FA_MAX_AGENTS_DEV; ++i) {
        if (i < N) {
            double s = acc_s[i], q = acc_q[i];
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) { s += __shfl_down(s, off, 64); q += __shfl_down(q, off, 64); }
            if (lane == 0) { red[wave][i][0] = s; red[wave][i][1] = q; }
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < 2 * N) {
        const int i = threadIdx.x >> 1, c = threadIdx.x & 1;
        partial[((long long)blockIdx.x * N + i) * 2 + c] = ((red[0][i][c] + red[1][i][c]) + red[2][i][c]) + red[3][i][c];
    }
}

// (The workgroups' partials are folded by fa_gae_mom_final_kernel or fa_gae_mom_norm_kernel with the row-0 pivot.)
__global__ __launch_bounds__(256) void fa_adv_onepass_kernel(const float *__restrict__ returns,
                                                             const float *__restrict__ value_preds, long long rows, int N,
                                                             double *__restrict__ partial) {
    double acc_s[FA_MAX_AGENTS_DEV], acc_q[FA_MAX_AGENTS_DEV], piv[FA_MAX_AGENTS_DEV];
#pragma unroll
    for (int i = 0; i < FA_MAX_AGENTS_DEV; ++i) {
        acc_s[i] = 0.0; acc_q[i] = 0.0;
        piv[i] = i < N ? fa_row0_pivot(returns, value_preds, i) : 0.0;
    }
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x; r < rows; r += stride) {
        const float *ret = returns + r * N, *vp = value_preds + r * N;
#pragma unroll
        for (int i = 0; i < FA_MAX_AGENTS_DEV; ++i) {
            if (i < N) {
                const double d = fa_mom_dev(ret[i] - vp[i], piv[i]);
                fa_mom_add(d, acc_s[i], acc_q[i]);
            }
        }
    }
    fa_adv_onepass_finish(acc_s, acc_q, N, partial);
}

// compile-time even N with 16-byte loads: two whole rows per lane per trip (see fa_adv_partial_vec_kernel)
template <int TN>
__global__ __launch_bounds__(256) void fa_adv_onepass_vec_kernel(const float *__restrict__ returns,
                                                                 const float *__restrict__ value_preds, long long row_pairs,
                                                                 double *__restrict__ partial) {
    constexpr int NV = TN / 2;
    constexpr int UNR = 4; // row pairs in flight per lane
    double acc_s[FA_MAX_AGENTS_DEV], acc_q[FA_MAX_AGENTS_DEV], piv[FA_MAX_AGENTS_DEV];
#pragma unroll
    for (int i = 0; i < FA_MAX_AGENTS_DEV; ++i) {
        acc_s[i] = 0.0; acc_q[i] = 0.0;
        piv[i] = i < TN ? fa_row0_pivot(returns, value_preds, i) : 0.0;
    }
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long p0 = (long long)blockIdx.x * blockDim.x + threadIdx.x; p0 < row_pairs; p0 += stride * UNR) {
        float4 rr[UNR][NV], vv[UNR][NV];
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            const long long p = p0 + u * stride;
            const long long pc = p < row_pairs ? p : p0; // clamped: loaded, not accumulated
            const float4 *r4 = reinterpret_cast<const float4 *>(returns + pc * 2 * TN);
            const float4 *v4 = reinterpret_cast<const float4 *>(value_preds + pc * 2 * TN);
#pragma unroll
            for (int q = 0; q < NV; ++q) { rr[u][q] = r4[q]; vv[u][q] = v4[q]; }
        }
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            if (p0 + u * stride < row_pairs) {
#pragma unroll
                for (int q = 0; q < NV; ++q) {
                    const float a4[4] = {rr[u][q].x - vv[u][q].x, rr[u][q].y - vv[u][q].y, rr[u][q].z - vv[u][q].z,
                                         rr[u][q].w - vv[u][q].w};
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int i = (4 * q + j) % TN; // folds to a constant after unrolling
                        fa_mom_add(fa_mom_dev(a4[j], piv[i]), acc_s[i], acc_q[i]);
                    }
                }
            }
        }
    }
    fa_adv_onepass_finish(acc_s, acc_q, TN, partial);
}

// stats[i] = {n, sum, 0} (PASS 0) / stats[i][2] = ssd (PASS 1).  One wave per agent: lane l
// folds partials l, l+64, ... in order, then a fixed shuffle tree => reproducible.
template <int PASS>
__global__ void fa_adv_final_kernel(const double *__restrict__ partial, int nblocks, int N, double n_rows,
                                    double *__restrict__ stats, double *__restrict__ derived) {
    const int i = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (i >= N) return;
    double s = 0.0;
    for (int b = lane; b < nblocks; b += 64) s += partial[(long long)b * N + i];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
    if (lane == 0) {
        if (PASS == 0) {
            stats[i * 3 + 0] = n_rows; stats[i * 3 + 1] = s; stats[i * 3 + 2] = 0.0;
            if (derived) derived[i] = s / n_rows;                           // local mean
        } else {
            stats[i * 3 + 2] = s;
            if (derived) derived[i] = sqrt(s / (n_rows - 1.0));             // local unbiased std
        }
    }
}

// ppo.py:123: (A - mean) / (std + 1e-5), float32 arithmetic with float32 mean/std.
__global__ __launch_bounds__(256) void fa_adv_norm_kernel(const float *__restrict__ returns,
                                                          const float *__restrict__ value_preds,
                                                          const double *__restrict__ mean,
                                                          const double *__restrict__ std_, long long total,
                                                          int N, float *__restrict__ out) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x; k < total; k += stride) {
        const int i = (int)(k % N);
        out[k] = fa_norm_adv(returns[k], value_preds[k], (float)mean[i], fa_norm_den(std_[i]));
    }
}

// The merge of fa_merge_ranks alone: one collective instead of two.  gathered: (W, N, 3); one lane per agent.
__global__ void fa_adv_merge_kernel(const double *__restrict__ gathered, int W, int N,
                                    double *__restrict__ mean_out, double *__restrict__ std_out) {
    const int i = threadIdx.x;
    if (i >= N) return;
    double n, mean, m2;
    fa_merge_ranks(gathered, W, N, i, n, mean, m2);
    mean_out[i] = mean;
    std_out[i] = sqrt(m2 / (n - 1.0));
}

// (n, sum, ssd) -> (n, mean, M2) in place, one lane per agent
__global__ void fa_adv_moments_kernel(double *__restrict__ stats, int N) {
    const int i = threadIdx.x;
    if (i >= N) return;
    stats[i * 3 + 1] = stats[i * 3 + 1] / stats[i * 3 + 0];
}

hipError_t fa_launch_adv_merge(const double *gathered, int W, int N, double *mean_out, double *std_out,
                               hipStream_t st) {
    hipLaunchKernelGGL(fa_adv_merge_kernel, dim3(1), dim3(64), 0, st, gathered, W, N, mean_out, std_out);
    return hipGetLastError();
}
static hipError_t fa_launch_adv_moments_fix(double *stats, int N, hipStream_t st) {
    hipLaunchKernelGGL(fa_adv_moments_kernel, dim3(1), dim3(64), 0, st, stats, N);
    return hipGetLastError();
}

// ---- host side --------------------------------------------------------------------------------------
// The bound rollout storage as the tail's launchers see it, built once per call from the handle (tail_args below).
// gamma and gamma * tau are rounded to float32 once (torch scalar * tensor).  The kernels take these as plain parameters.
struct FaTailArgs {
    const float *rewards, *value_preds, *masks; // (T, E, N), (T + 1, E, N), (T + 1, E, N)
    float *returns;                             // (T + 1, E, N)
    const uint8_t *done;                        // (T, E)
    int T, E, N;
    float g32, gt32;
    long long rows() const { return (long long)T * E; }   // samples per agent
    long long total() const { return rows() * N; }
};

// Where fa_gae_mom_final_kernel / fa_gae_mom_norm_kernel take the per-agent statistics from.
enum FaStatSource {
    FA_STATS_SCAN_PARTIALS,  // fold of fa_gae_mom_kernel's {S, Q} partials; pivot = the agent's first GAE term of env 0
    FA_STATS_SWEEP_PARTIALS, // fold of fa_adv_onepass[_vec]_kernel's partials; pivot = the agent's advantage in row 0
    FA_STATS_GATHERED_RANKS, // rank-order merge of gathered (W, N, 3) {n, mean, M2} triples (fa_gae_mom_norm_kernel only)
};

// fa_gae_kernel / fa_gae_coop_kernel / fa_gae4_kernel by the number of columns
static hipError_t fa_launch_gae(const FaTailArgs &a, hipStream_t st) {
    const long long EN = (long long)a.E * a.N;
    // four columns per lane pay off only once there are enough columns to fill the chip with
    // 16-byte lanes; below that the one-column kernel has 4x the waves in flight
    const bool vec4 = (EN >= 4LL * 64 * 1024) && (EN % 4 == 0) && ((((uintptr_t)a.rewards | (uintptr_t)a.value_preds | (uintptr_t)a.masks |
                                          (uintptr_t)a.returns) & 15) == 0);
    const int grid = (int)(((vec4 ? EN / 4 : EN) + 63) / 64);   // 64 lanes of one column each, or of four
    if (vec4)
        hipLaunchKernelGGL(fa_gae4_kernel, dim3(grid), dim3(64), 0, st, a.rewards, a.value_preds, a.masks, a.returns, a.done, a.T, a.E,
                           a.N, a.g32, a.gt32);
    else if (EN <= 64LL * 2048)
        // few columns: four cooperating waves per 64 columns (see fa_gae_coop_kernel)
        hipLaunchKernelGGL(fa_gae_coop_kernel, dim3(grid), dim3(256), 0, st, a.rewards, a.value_preds, a.masks, a.returns, a.done,
                           a.T, a.E, a.N, a.g32, a.gt32);
    else
        hipLaunchKernelGGL(fa_gae_kernel, dim3(grid), dim3(64), 0, st, a.rewards, a.value_preds, a.masks, a.returns, a.done, a.T, a.E,
                           a.N, a.g32, a.gt32);
    return hipGetLastError();
}

// ---- GAE + moments (fa_gae_mom_kernel) and its two possible second launches ---------------------------
// Eligible up to 512 workgroups = 32 768 (env, agent) columns -- two workgroups per CU, which is what the kernel's 72 KB of
// LDS admit: beyond that the workgroups of a CU would run one after the other.  (The one-wave form of round 4 to 6, 53 KB,
// lost there with three per CU: 41 us against 34 for the separate kernels at 5v5 x 4096 and 3v3 x 8192; the role-split
// kernel was not measured beyond 512.)  At 3v3 x 4096 the fused tail takes 23.7 us against 33.7 for the separate kernels.  `partial`
// (partial_cap doubles) holds a {S, Q} pair per (workgroup, agent).  Returns the number of workgroups or 0.
static int fa_gae_mom_blocks(int T, int E, int N, long long partial_cap) {
    const long long EN = (long long)E * N;
    if (EN > 64LL * 512 || T < 1 || (long long)(T + 1) * EN * 4 >= (1LL << 31)) return 0;
    const long long nb = (EN + 63) / 64;
    if (nb > 64 * FA_GAEM_FOLD || nb * N * 2 > partial_cap) return 0;
    return (int)nb;
}
static hipError_t fa_launch_gae_mom(const FaTailArgs &a, double *partial, int nblocks, hipStream_t st) {
    hipLaunchKernelGGL(fa_gae_mom_kernel, dim3(nblocks), dim3(FA_GAES_THREADS), 0, st, a.rewards, a.value_preds, a.masks, a.returns,
                       a.done, a.T, a.E, a.N, a.g32, a.gt32, partial);
    return hipGetLastError();
}
// one workgroup folds `count` workgroups of partials (FA_STATS_SCAN_PARTIALS or FA_STATS_SWEEP_PARTIALS)
static hipError_t fa_launch_gae_mom_final(const FaTailArgs &a, FaStatSource src, const double *stats, int count, double *moments_out,
                                          double *mean_out, double *std_out, hipStream_t st) {
    hipLaunchKernelGGL(fa_gae_mom_final_kernel, dim3(1), dim3(64 * a.N), 0, st, stats, count, a.N, a.rewards, a.value_preds, a.masks,
                       a.returns, a.T, (long long)a.E * a.N, a.g32, (double)a.T * (double)a.E, moments_out, mean_out,
                       std_out, src == FA_STATS_SWEEP_PARTIALS ? 1 : 0);
    return hipGetLastError();
}
// statistics (fold of `count` workgroups of partials, or merge of `count` ranks) + normalisation in every workgroup
static hipError_t fa_launch_gae_mom_norm(const FaTailArgs &a, FaStatSource src, const double *stats, int count, float *out,
                                         double *moments_out, double *mean_out, double *std_out, hipStream_t st) {
    // a lane takes two 16-byte quads per trip; two workgroups of eight waves per CU (measured at config 2's 38 MB:
    // 128 / 256 / 512 / 1024 workgroups -> 31.6 / 29.7 / 30.0 / 31.6 us for the two launches, 512 the best behind the rollout)
    const long long want = (a.total() / 4 + 1023) / 1024;
    const int grid = (int)(want < 512 ? (want < 1 ? 1 : want) : 512);
    // several ranks: fa_adv_merge + fa_adv_normalize as ONE launch (every workgroup merges the gathered triples itself)
    const bool merge = src == FA_STATS_GATHERED_RANKS;
    hipLaunchKernelGGL(fa_gae_mom_norm_kernel, dim3(grid), dim3(512), 0, st, merge ? nullptr : stats, merge ? 0 : count, a.N, a.rewards,
                       a.value_preds, a.masks, a.returns, a.T, (long long)a.E * a.N, a.g32, (double)a.T * (double)a.E,
                       a.total(), out, merge ? nullptr : moments_out, mean_out, std_out, src == FA_STATS_SWEEP_PARTIALS ? 1 : 0,
                       merge ? stats : nullptr, merge ? count : 0);
    return hipGetLastError();
}

// The one-pass sweep: `partial` must hold nblocks * N * 2 doubles.  Its partials go to fa_launch_gae_mom_final or
// fa_launch_gae_mom_norm with FA_STATS_SWEEP_PARTIALS, whose fold takes at most 64 * FA_GAEM_FOLD workgroups.
static hipError_t fa_launch_adv_onepass(const FaTailArgs &a, double *partial, int nblocks, hipStream_t st) {
    const long long rows = a.rows();
    const bool vec = (rows % 2 == 0) && ((((uintptr_t)a.returns | (uintptr_t)a.value_preds) & 15) == 0);
    if (nblocks > 64 * FA_GAEM_FOLD) nblocks = 64 * FA_GAEM_FOLD;
    if (vec && a.N == 6)
        hipLaunchKernelGGL((fa_adv_onepass_vec_kernel<6>), dim3(nblocks), dim3(256), 0, st, a.returns, a.value_preds,
                           rows / 2, partial);
    else if (vec && a.N == 10)
        hipLaunchKernelGGL((fa_adv_onepass_vec_kernel<10>), dim3(nblocks), dim3(256), 0, st, a.returns, a.value_preds,
                           rows / 2, partial);
    else
        hipLaunchKernelGGL(fa_adv_onepass_kernel, dim3(nblocks), dim3(256), 0, st, a.returns, a.value_preds, rows, a.N,
                           partial);
    return hipGetLastError();
}

template <int PASS>
static void launch_adv_partial(const float *returns, const float *value_preds, const double *mean, long long rows,
                               int N, double *partial, int nblocks, hipStream_t st) {
    const bool vec = (rows % 2 == 0) && ((((uintptr_t)returns | (uintptr_t)value_preds) & 15) == 0);
    if (vec && N == 6)
        hipLaunchKernelGGL((fa_adv_partial_vec_kernel<PASS, 6>), dim3(nblocks), dim3(256), 0, st, returns, value_preds,
                           mean, rows / 2, partial);
    else if (vec && N == 10)
        hipLaunchKernelGGL((fa_adv_partial_vec_kernel<PASS, 10>), dim3(nblocks), dim3(256), 0, st, returns, value_preds,
                           mean, rows / 2, partial);
    else
        hipLaunchKernelGGL(fa_adv_partial_kernel<PASS>, dim3(nblocks), dim3(256), 0, st, returns, value_preds, mean,
                           rows, N, partial);
}

// the two-pass statistics: the reference formulation the one-pass code is tested against, kept apart from it (no FaTailArgs,
// no shared helpers)
static hipError_t fa_launch_adv_stats(int pass, const float *returns, const float *value_preds, const double *mean,
                                      long long rows, int N, double *partial, int nblocks, double *stats,
                                      double *derived, hipStream_t st) {
    if (pass == 0) {
        launch_adv_partial<0>(returns, value_preds, mean, rows, N, partial, nblocks, st);
        hipLaunchKernelGGL(fa_adv_final_kernel<0>, dim3(1), dim3(64 * N), 0, st, partial, nblocks, N,
                           (double)rows, stats, derived);
    } else {
        launch_adv_partial<1>(returns, value_preds, mean, rows, N, partial, nblocks, st);
        hipLaunchKernelGGL(fa_adv_final_kernel<1>, dim3(1), dim3(64 * N), 0, st, partial, nblocks, N,
                           (double)rows, stats, derived);
    }
    return hipGetLastError();
}

static hipError_t fa_launch_adv_norm(const FaTailArgs &a, const double *mean, const double *std_, float *out, hipStream_t st) {
    const long long total = a.total();
    long long want = (total + 255) / 256;
    const int grid = (int)(want < 2048 ? (want < 1 ? 1 : want) : 2048);
    hipLaunchKernelGGL(fa_adv_norm_kernel, dim3(grid), dim3(256), 0, st, a.returns, a.value_preds, mean, std_,
                       total, a.N, out);
    return hipGetLastError();
}

// ---- the exports (include/fortattack.h) --------------------------------------------------------------------
namespace {
// The bound storage as the launchers above take it; gamma, gamma * tau rounded to float32 once.
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

int fa_gae(fa_env *env, double gamma, double tau, void *stream) {
    FA_ENTER(env, "fa_gae", true);
    FA_HIP(fa_launch_gae(tail_args(env, gamma, tau), static_cast<hipStream_t>(stream)));
    return FA_OK;
}

int fa_gae_moments(fa_env *env, double gamma, double tau, double *moments_out, double *mean_out, double *std_out,
                   void *stream) {
    FA_ENTER(env, "fa_gae_moments", true);
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
    FA_ENTER(env, "fa_gae_normalize", true, adv_out);
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
    FA_ENTER(env, "fa_adv_moments_onepass", true);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const FaTailArgs a = tail_args(env);
    const int nblocks = tail_plan(env, a).sweep;
    FA_HIP(fa_launch_adv_onepass(a, env->adv_partial, nblocks, s));
    FA_HIP(fa_launch_gae_mom_final(a, FA_STATS_SWEEP_PARTIALS, env->adv_partial, nblocks, moments_out, mean_out,
                                   std_out, s));
    return FA_OK;
}

int fa_adv_stats(fa_env *env, int32_t pass, const double *mean, double *stats, void *stream) {
    FA_ENTER(env, "fa_adv_stats", true, stats);
    if (pass != 0 && pass != 1) return fail(FA_ERR_INVALID, "fa_adv_stats: pass must be 0 or 1");
    if (pass == 1 && !mean) return fail(FA_ERR_INVALID, "fa_adv_stats: pass 1 needs mean");
    const FaTailArgs a = tail_args(env);
    FA_HIP(fa_launch_adv_stats(pass, a.returns, a.value_preds, mean, a.rows(), a.N, env->adv_partial,
                               tail_plan(env, a).twopass, stats, nullptr, static_cast<hipStream_t>(stream)));
    return FA_OK;
}

int fa_adv_mean_std(fa_env *env, double *mean_out, double *std_out, void *stream) {
    FA_ENTER(env, "fa_adv_mean_std", true, mean_out, std_out);
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
    FA_ENTER(env, "fa_adv_moments", true, moments_out);
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
    FA_ENTER(env, "fa_adv_merge", false, gathered, mean_out, std_out);
    if (world < 1) return fail(FA_ERR_INVALID, "fa_adv_merge: world must be >= 1");
    FA_HIP(fa_launch_adv_merge(gathered, world, env->N, mean_out, std_out, static_cast<hipStream_t>(stream)));
    return FA_OK;
}

int fa_adv_merge_normalize(fa_env *env, const double *gathered, int32_t world, float *adv_out, double *mean_out, double *std_out,
                           void *stream) {
    FA_ENTER(env, "fa_adv_merge_normalize", false, gathered, adv_out);
    if (world < 1) return fail(FA_ERR_INVALID, "fa_adv_merge_normalize: world must be >= 1");
    // (this export has always looked at `world` before the storage: the storage check keeps its place)
    if (!env->bound) return fail(FA_ERR_STATE, "fa_adv_merge_normalize: no storage bound");
    FA_HIP(fa_launch_gae_mom_norm(tail_args(env), FA_STATS_GATHERED_RANKS, gathered, world, adv_out, nullptr, mean_out,
                                  std_out, static_cast<hipStream_t>(stream)));
    return FA_OK;
}

int fa_adv_normalize(fa_env *env, const double *mean, const double *std_, float *adv_out, void *stream) {
    FA_ENTER(env, "fa_adv_normalize", true, mean, std_, adv_out);
    FA_HIP(fa_launch_adv_norm(tail_args(env), mean, std_, adv_out, static_cast<hipStream_t>(stream)));
    return FA_OK;
}

} // extern "C"
