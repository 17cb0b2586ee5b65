// fa_collect.h -- what another translation unit launches of the collector tail (fa_collect.hip).
#pragma once
#include <hip/hip_runtime.h>

// rank-order merge of gathered (W, N, 3) {n, mean, M2} triples (fa_adv_merge; fa_adv_allreduce of fa_rccl.hip)
hipError_t fa_launch_adv_merge(const double *gathered, int W, int N, double *mean_out, double *std_out, hipStream_t st);
