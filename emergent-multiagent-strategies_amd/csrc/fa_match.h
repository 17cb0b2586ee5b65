// fa_match.h -- internal declarations of the match bookkeeping kernels (fa_match.hip): a fixed number of episodes per env,
// latched on the device, summed per match-up cell (include/fortattack.h: fa_match_begin / fa_match_latch / fa_match_table).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fa_device.h"

struct FaMatch {
    uint32_t *base_rc, *lat_rc;       // (E,3) result_count at fa_match_begin / of the env's quota of episodes
    uint32_t *base_alive, *lat_alive; // (E,N) alive_end likewise
    double *base_rew, *lat_rew;       // (E,N) ep_rew_sum likewise
    int32_t *cell, *latched;          // (E)   the env's match-up cell; 1 once its quota is latched
    int32_t *remaining, *overrun;     // device scalars: envs not yet latched; an env was seen beyond its quota
    int32_t n_cells, episodes_per_env, begun; // host side
};

#define FA_MATCH_THREADS 256 // workgroup of the table kernel: one per cell

hipError_t fa_launch_match_begin(const FaState &s, const FaMatch &m, const int32_t *env_cell, int E, int N, hipStream_t st);
hipError_t fa_launch_match_latch(const FaState &s, const FaMatch &m, int E, int N, hipStream_t st);
hipError_t fa_launch_match_table(const FaState &s, const FaMatch &m, int E, int N, double *raw, hipStream_t st);
