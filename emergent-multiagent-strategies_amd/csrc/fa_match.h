// fa_match.h -- what a handle keeps for the match bookkeeping (fa_match.hip): a fixed number of episodes per env, latched on
// the device, summed per match-up cell (include/fortattack.h: fa_match_begin / fa_match_latch / fa_match_table).
#pragma once
#include <stdint.h>

struct FaMatch {
    uint32_t *base_rc, *lat_rc;       // (E,3) result_count at fa_match_begin / of the env's quota of episodes
    uint32_t *base_alive, *lat_alive; // (E,N) alive_end likewise
    double *base_rew, *lat_rew;       // (E,N) ep_rew_sum likewise
    int32_t *cell, *latched;          // (E)   the env's match-up cell; 1 once its quota is latched
    int32_t *remaining, *overrun;     // device scalars: envs not yet latched; an env was seen beyond its quota
    int32_t n_cells, episodes_per_env, begun; // host side
};
