// fa_behaviour.h -- what a handle keeps for the behaviour-map pass (fa_behaviour.hip; include/fortattack.h:
// fa_behaviour_begin / fa_behaviour_chunk).
#pragma once
#include <stdint.h>

// the persistent per-env counters and the launch plan fa_behaviour_begin builds
struct FaBehaviour {
    int32_t *ep_count, *ep_t; // (E) episodes finished since begin; steps into the episode in flight
    int32_t *env_list;        // (E) the envs grouped by cell, ascending inside a cell; the envs of no cell last
    int32_t *slices;          // (max_slices, 4): cell (-1: counted nowhere), first entry of env_list, entries, 0
    int32_t max_slices;
    // host side, set by fa_behaviour_begin
    uint64_t *counts;
    int32_t n_cells, quota, n_slices, begun;
};
