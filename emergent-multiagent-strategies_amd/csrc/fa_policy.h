// fa_policy.h -- the tile constants of the fused MPNN policy kernel (fa_policy.hip) and the layout of
// its packed weight buffer (filled by emergent-multiagent-strategies_amd/mpnn_pack.py; documented for
// other hosts in include/fortattack.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fortattack.h"

#define FA_POLICY_ROWS 96     // (env, agent) rows per workgroup tile = three 32-row MFMA blocks
#define FA_POLICY_MAX_TEAM 8  // agents per team the attention loops are unrolled for

// Offsets (in floats) into one team's packed weight buffer, hidden_dim = 128 (mpnn.py:27-74).
// "packed (K x C)" = MFMA B-operand order: float4 index (cb * K/8 + t4) * 64 + lane holds
// W[k = (lane >> 5) * K/2 + 4 * t4 + q][col = 32 * cb + (lane & 31)], q = 0..3.
#define FA_POFF_WE 0        // encoder weight^T, plain [6][64]
#define FA_POFF_BE 384      // encoder bias [64]
#define FA_POFF_WOE 448     // oppEncoder weight^T, plain [6][64]
#define FA_POFF_BOE 832     // oppEncoder bias [64]
#define FA_POFF_AO 896      // packed (64 x 64):  norm_o * oppAttn.W_key W_query^T
#define FA_POFF_BO 4992     // packed (64 x 64):  oppAttn.W_val W_out
#define FA_POFF_AM 9088     // packed (128 x 128): norm * messages.W_query W_key^T
#define FA_POFF_W7 25472    // packed (256 x 128): [update.weight[:, :128]^T ; messages.W_val W_out update.weight[:, 128:]^T]
#define FA_POFF_BU 58240    // update bias [128]
#define FA_POFF_W8 58368    // packed (128 x 256): [policy_head.0.weight^T | value_head.0.weight^T]
#define FA_POFF_B8 91136    // [policy_head.0.bias | value_head.0.bias] [256]
#define FA_POFF_W9 91392    // packed (256 x 32): rows 0..127 x cols 0..7 = dist.linear.weight^T, rows 128..255 x col 8 = value_head.2.weight^T
#define FA_POFF_B9 99584    // [dist.linear.bias (8) | value_head.2.bias (1) | 0 ...] [32]
#define FA_POLICY_PLAIN_FLOATS 99616  // end of the float32 sections above (= the layout of the plain / gradient buffers)
// The same six dense matrices once more, for the bf16 matrix cores: every float32 weight split EXACTLY into three bf16 terms
// (hi = round-to-nearest at 8 significant bits, mid = the remainder rounded likewise, lo = the rest; fa_mfma.h gemm_cb3),
// in the B-operand order of v_mfma_f32_32x32x16_bf16: 16-byte index ((cb * K/16 + s) * 3 + term) * 64 + lane holds the eight
// bf16 W[k = (lane >> 5) * K/2 + 8 s + j][col = 32 cb + (lane & 31)], j = 0..7, of term 0 / 1 / 2 = hi / mid / lo.
// 1.5 floats of buffer per weight.  Written by fa_pack_weights (device) / mpnn_pack.pack_policy (host) next to the float32 form.
#define FA_POFF3_AO 99616   // (64 x 64)
#define FA_POFF3_BO 105760  // (64 x 64)
#define FA_POFF3_AM 111904  // (128 x 128)
#define FA_POFF3_W7 136480  // (256 x 128)
#define FA_POFF3_W8 185632  // (128 x 256)
#define FA_POFF3_W9 234784  // (256 x 32)
#define FA_POLICY_WEIGHT_FLOATS 247072

// The six dense sections as X(name, K, C).  The offsets above stay literals (include/fortattack.h documents them for other
// hosts); what follows checks that each is the previous one plus the previous section's size.
#define FA_DENSE_SECTIONS(X) X(AO, 64, 64) X(BO, 64, 64) X(AM, 128, 128) X(W7, 256, 128) X(W8, 128, 256) X(W9, 256, 32)
static_assert(FA_POFF_WE == 0 && FA_POFF_BE == FA_POFF_WE + 6 * 64 && FA_POFF_WOE == FA_POFF_BE + 64 && FA_POFF_BOE == FA_POFF_WOE + 6 * 64 &&
                  FA_POFF_AO == FA_POFF_BOE + 64 && FA_POFF_BO == FA_POFF_AO + 64 * 64 && FA_POFF_AM == FA_POFF_BO + 64 * 64 &&
                  FA_POFF_W7 == FA_POFF_AM + 128 * 128 && FA_POFF_BU == FA_POFF_W7 + 256 * 128 && FA_POFF_W8 == FA_POFF_BU + 128 &&
                  FA_POFF_B8 == FA_POFF_W8 + 128 * 256 && FA_POFF_W9 == FA_POFF_B8 + 256 && FA_POFF_B9 == FA_POFF_W9 + 256 * 32 &&
                  FA_POLICY_PLAIN_FLOATS == FA_POFF_B9 + 32,
              "FA_POFF_*: the float32 sections lie back to back");
// {offset, floats} of the dense sections in some pack, in order: back to back from `at` up to `end`?
constexpr bool fa_back_to_back(const int (*sec)[2], int n, int at, int end) {
    for (int i = 0; i < n; ++i) {
        if (sec[i][0] != at) return false;
        at += sec[i][1];
    }
    return at == end;
}
#define FA_X(n, K, C) {FA_POFF3_##n, (K) * (C) * 3 / 2},
constexpr int fa_poff3_sections[][2] = {FA_DENSE_SECTIONS(FA_X)};
#undef FA_X
static_assert(fa_back_to_back(fa_poff3_sections, 6, FA_POLICY_PLAIN_FLOATS, FA_POLICY_WEIGHT_FLOATS),
              "FA_POFF3_*: 1.5 floats per weight, back to back behind the float32 sections");
