// fa_collect.h -- host interface of the collector tail (fa_collect.hip): GAE scan, advantage statistics, normalisation.
#pragma once
#include <cstdint>

#include <hip/hip_runtime.h>

// The bound rollout storage as the tail's launchers see it, built once per call from the handle (tail_args in fa_api.hip).
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
hipError_t fa_launch_gae(const FaTailArgs &a, hipStream_t st);
// workgroups of the fused scan for this shape, 0 where it does not serve; `partial_cap` doubles of partials are available
int fa_gae_mom_blocks(int T, int E, int N, long long partial_cap);
hipError_t fa_launch_gae_mom(const FaTailArgs &a, double *partial, int nblocks, hipStream_t st);
// the one-pass sweep over returns / value_preds: partial[nblocks][N] = {S, Q}; nblocks <= 512
hipError_t fa_launch_adv_onepass(const FaTailArgs &a, double *partial, int nblocks, hipStream_t st);
// one workgroup folds `count` workgroups of partials (FA_STATS_SCAN_PARTIALS or FA_STATS_SWEEP_PARTIALS)
hipError_t fa_launch_gae_mom_final(const FaTailArgs &a, FaStatSource src, const double *stats, int count, double *moments_out,
                                   double *mean_out, double *std_out, hipStream_t st);
// statistics (fold of `count` workgroups of partials, or merge of `count` ranks) + normalisation in every workgroup
hipError_t fa_launch_gae_mom_norm(const FaTailArgs &a, FaStatSource src, const double *stats, int count, float *out,
                                  double *moments_out, double *mean_out, double *std_out, hipStream_t st);
// the two-pass statistics: the reference formulation the one-pass code is tested against, kept apart from it (no FaTailArgs,
// no shared helpers)
hipError_t fa_launch_adv_stats(int pass, const float *returns, const float *value_preds, const double *mean,
                               long long rows, int N, double *partial, int nblocks, double *stats,
                               double *derived, hipStream_t st);
hipError_t fa_launch_adv_moments_fix(double *stats, int N, hipStream_t st);
hipError_t fa_launch_adv_merge(const double *gathered, int W, int N, double *mean_out, double *std_out, hipStream_t st);
hipError_t fa_launch_adv_norm(const FaTailArgs &a, const double *mean, const double *std_, float *out, hipStream_t st);
