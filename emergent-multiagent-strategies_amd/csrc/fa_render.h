// fa_render.h -- internal declarations of the batched frame renderer (fa_render.hip; include/fortattack.h: fa_render).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fa_device.h"

struct FaRenderArgs {
    FaState s;
    const int32_t *env_index; // (K) env of the handle shown by frame k
    uint8_t *rgb;             // (K, size, size, 3), row 0 = top
    const int64_t *actions;   // or null; element (e,i) at actions[e*as_e + i*as_i]
    int64_t as_e, as_i;
    const uint8_t *no_laser;  // (E) or null
    const float *team_attn;   // guards' (E,G,G) or null
    const float *opp_attn;    // guards' (E,G,A) or null
    int32_t K, size, E, G, A;
    int32_t viz_dead, attn_on; // attn_on: both maps given and viz_attn set
    // fortattack.py:368-600 constants, from FaDerived
    double agent_size, fort_dim, door_x, door_y, wall_xmin, wall_xmax, wall_ymin, wall_ymax, shoot_rad, half_win;
};

#define FA_RENDER_THREADS 256
#define FA_RENDER_QUADS 4 // 4-pixel spans per lane: a workgroup owns 256 * 4 spans = 4096 pixels of one frame

int fa_render_tiles(int size); // workgroups per frame
hipError_t fa_launch_render(const FaRenderArgs &a, hipStream_t st);
