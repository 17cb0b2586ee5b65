// fa_behaviour.h -- internal declarations of the behaviour-map pass (fa_behaviour.hip; include/fortattack.h:
// fa_behaviour_begin / fa_behaviour_chunk).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fa_device.h"

#define FA_BEH_THREADS 256
#define FA_BEH_SLICE 16  // envs of ONE cell per workgroup
#define FA_BEH_TB 64     // steps per block of the done scan / the sample sweep
#define FA_BEH_MAX_CELLS 4096
#define FA_BEH_MAX_MT 1024 // the largest record a workgroup keeps in LDS: (2 + 3 * 1024 + 6 * 32 * 40) * 4 = 43 016 bytes

// per handle: the persistent per-env counters and the launch plan fa_behaviour_begin builds
struct FaBehaviour {
    int32_t *ep_count, *ep_t; // (E) episodes finished since begin; steps into the episode in flight
    int32_t *env_list;        // (E) the envs grouped by cell, ascending inside a cell; the envs of no cell last
    int32_t *slices;          // (max_slices, 4): cell (-1: counted nowhere), first entry of env_list, entries, 0
    int32_t max_slices;
    // host side, set by fa_behaviour_begin
    uint64_t *counts;
    int32_t n_cells, quota, n_slices, begun;
};

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

inline int fa_behaviour_max_slices(int E) { return (E + FA_BEH_SLICE - 1) / FA_BEH_SLICE + FA_BEH_MAX_CELLS + 1; }
hipError_t fa_launch_behaviour(const FaBehaviourArgs &a, int n_slices, hipStream_t st);
