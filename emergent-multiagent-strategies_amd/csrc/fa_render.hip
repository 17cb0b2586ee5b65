// fa_render.hip -- batched frame renderer: K frames of size x size x 3 uint8 straight from the handle's device state.
//
// The picture is the reference's pyglet scene (gym_fortattack/fortattack.py:368-600) as render.py::render_frame rasterises it
// with numpy, in the same painter's order: white background, black active region, fort disc, laser triangles (alpha 0.3),
// attention discs (fortattack.py:439-466), body and head discs, the reference agent's dot (:531-546), grey strips (:548-560),
// clip * 255 + 0.5 -> uint8.  The arithmetic is render_frame's operation for operation -- pixel centres and every geometry
// predicate in fp64 with the same expressions and comparison signs, colours as float32 blends img * (1 - a) + c * a with
// (1 - a) formed in double and rounded to float32 -- so a frame equals render_frame's byte for byte unless a pixel centre lies
// within a few ulp of an edge (the heading sin / cos are sincos_heading's, numpy's are glibc's).  Built with -ffp-contract=off
// like the rest of the library: nothing is fused.
//
// Shape: a workgroup owns 4096 consecutive pixels (1024 four-pixel spans, row-major) of ONE frame.  Its first wave, lane =
// agent, builds the frame's primitive list in LDS once -- compacted in painter's order with wave ballots, the trig lives here
// -- and after one barrier every lane evaluates its spans against the list in order (all lanes read the same primitive: LDS
// broadcasts); a wave skips a primitive whose Y extent misses the few rows its 64 spans lie in.  A lane owns 4 consecutive
// pixels of a row, so its 12 bytes leave as three dword stores where the address allows (two-byte stores where it is only
// even); the row tail of a size that is no multiple of 4 is written bytewise.  No allocation, no synchronisation: the
// launch is graph-capturable.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fa_env.h"
#include "fa_step_common.h" // sincos_heading

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

namespace {
enum { PR_DISC = 1, PR_TRI = 2 };

struct Prim {         // 136 bytes
    double d[12];     // disc: cx, cy, r^2.  triangle: per edge (q -> r) q0, q1, r1 - q1, r0 - q0
    double ylo, yhi;  // no pixel centre with Y outside [ylo, yhi] can pass the predicate (padded far beyond any rounding)
    float ca[3];      // c * alpha, the float32 product numpy forms
    float om;         // (float)(1.0 - alpha)
    int32_t type, pad;
};
#define FA_RENDER_PAD 1e-9 // world units; the predicates' rounding errors are ~1e-16

// fort + per agent (laser, attention disc, body, head) + the reference agent's dot
#define FA_RENDER_MAX_PRIMS (2 + 4 * FA_MAX_AGENTS_DEV)

__device__ __forceinline__ void set_colour(Prim &p, float r, float g, float b, double alpha) {
    const float af = (float)alpha;
    p.ca[0] = r * af;
    p.ca[1] = g * af;
    p.ca[2] = b * af;
    p.om = (float)(1.0 - alpha);
}

__device__ __forceinline__ void set_disc(Prim &p, double cx, double cy, double r) {
    p.type = PR_DISC;
    p.d[0] = cx;
    p.d[1] = cy;
    p.d[2] = r * r;
    p.ylo = cy - (fabs(r) + FA_RENDER_PAD);
    p.yhi = cy + (fabs(r) + FA_RENDER_PAD);
}

// side(q, r) of render_frame: (X - q0) * (r1 - q1) - (Y - q1) * (r0 - q0)
__device__ __forceinline__ void set_edge(double *d, double q0, double q1, double r0, double r1) {
    d[0] = q0;
    d[1] = q1;
    d[2] = r1 - q1;
    d[3] = r0 - q0;
}

__device__ __forceinline__ uint32_t to_u8(float v) {
    v = fminf(fmaxf(v, 0.0f), 1.0f);
    return (uint32_t)(v * 255.0f + 0.5f);
}

__global__ __launch_bounds__(FA_RENDER_THREADS) void fa_render_kernel(FaRenderArgs a, int tiles) {
    __shared__ Prim prims[FA_RENDER_MAX_PRIMS];
    __shared__ int nprim_s;
    const int frame = blockIdx.x / tiles, tile = blockIdx.x - frame * tiles;
    const int e = a.env_index[frame];
    if (e < 0 || e >= a.E) return; // the whole workgroup: nothing is read or written for this frame
    const int G = a.G, N = a.G + a.A;

    if (threadIdx.x < FA_WAVE) { // wave 0, lane = agent
        const int i = threadIdx.x;
        const bool valid = i < N;
        bool alive = false, shoot = false;
        double px = 0.0, py = 0.0, ang = 0.0;
        if (valid) {
            const size_t idx = (size_t)e * N + i;
            px = a.s.px[idx];
            py = a.s.py[idx];
            ang = a.s.ang[idx];
            alive = a.s.alive[idx] != 0;
            if (a.actions && !(a.no_laser && a.no_laser[e])) shoot = a.actions[(int64_t)e * a.as_e + (int64_t)i * a.as_i] == 7;
        }
        const bool drawn = valid && (alive || a.viz_dead);
        const bool laser = valid && alive && shoot;
        // attn_reference_agent (fortattack.py:441-444): the first agent that is alive or is the last guard
        const unsigned long long alive_m = __ballot(valid && alive);
        const int k = a.attn_on ? __builtin_ctzll(alive_m | (1ull << (G - 1))) : -1;
        const bool attn = a.attn_on && drawn && i != k;
        const unsigned long long laser_m = __ballot(laser), attn_m = __ballot(attn), drawn_m = __ballot(drawn);
        const unsigned long long below = (1ull << i) - 1ull;
        const int n_laser = __popcll(laser_m), n_attn = __popcll(attn_m), n_drawn = __popcll(drawn_m);
        const bool guard = i < G;
        const float cr = guard ? 0.0f : 1.0f, cg = guard ? 1.0f : 0.0f; // GUARD_RGB / ATTACKER_RGB

        if (i == 0) { // fort disc, fortattack.py:432
            Prim &p = prims[0];
            set_disc(p, a.door_x, a.door_y, a.fort_dim);
            set_colour(p, 0.0f, 1.0f, 1.0f, 1.0);
        }
        double sn = 0.0, cs = 1.0;
        if (drawn || laser) sincos_heading(ang, sn, cs);
        if (laser) { // core.py:373-382
            Prim &p = prims[1 + __popcll(laser_m & below)];
            double s2, c2, s3, c3;
            sincos_heading(ang + a.half_win, s2, c2);
            sincos_heading(ang - a.half_win, s3, c3);
            const double p1x = px + a.agent_size * cs, p1y = py + a.agent_size * sn;
            const double p2x = p1x + a.shoot_rad * c2, p2y = p1y + a.shoot_rad * s2;
            const double p3x = p1x + a.shoot_rad * c3, p3y = p1y + a.shoot_rad * s3;
            p.type = PR_TRI;
            set_edge(p.d + 0, p1x, p1y, p2x, p2y);
            set_edge(p.d + 4, p2x, p2y, p3x, p3y);
            set_edge(p.d + 8, p3x, p3y, p1x, p1y);
            p.ylo = fmin(p1y, fmin(p2y, p3y)) - FA_RENDER_PAD; // the three sides agree in sign only inside the triangle
            p.yhi = fmax(p1y, fmax(p2y, p3y)) + FA_RENDER_PAD;
            set_colour(p, cr, cg, 0.0f, 0.3);
        }
        if (attn) { // the weight the reference agent k (a guard) gives agent i
            Prim &p = prims[1 + n_laser + __popcll(attn_m & below)];
            const double w = guard ? (double)a.team_attn[((size_t)e * G + k) * G + i]
                                   : (double)a.opp_attn[((size_t)e * G + k) * a.A + (i - G)];
            set_disc(p, px, py, a.agent_size * (1.0 + w));
            set_colour(p, 1.0f, 1.0f, 0.0f, alive ? 0.9 : 0.3);
        }
        if (drawn) {
            const int at = 1 + n_laser + n_attn + 2 * __popcll(drawn_m & below);
            const double alpha = alive ? 1.0 : 0.35;
            set_disc(prims[at], px, py, a.agent_size);
            set_colour(prims[at], cr, cg, 0.0f, alpha);
            set_disc(prims[at + 1], px + 0.8 * a.agent_size * cs, py + 0.8 * a.agent_size * sn, 0.5 * a.agent_size);
            set_colour(prims[at + 1], cr, cg, 0.0f, alpha);
        }
        const bool dot = i == k && drawn; // fortattack.py:531-546
        if (dot) {
            Prim &p = prims[1 + n_laser + n_attn + 2 * n_drawn];
            set_disc(p, px, py, 0.5 * a.agent_size);
            set_colour(p, 0.5f * cr, 0.5f * cg, 0.5f * 0.0f, 1.0);
        }
        const unsigned long long dot_m = __ballot(dot);
        if (i == 0) nprim_s = 1 + n_laser + n_attn + 2 * n_drawn + (dot_m ? 1 : 0);
    }
    __syncthreads();

    const int nprim = __builtin_amdgcn_readfirstlane(nprim_s);
    const int size = a.size, qpr = (size + 3) >> 2, total = size * qpr;
    const double dsz = (double)size;
    uint8_t *const frame_out = a.rgb + (size_t)frame * size * size * 3;
#pragma unroll 1
    for (int it = 0; it < FA_RENDER_QUADS; ++it) {
        const int q = (tile * FA_RENDER_QUADS + it) * FA_RENDER_THREADS + (int)threadIdx.x;
        if (q >= total) break;
        const int row = q / qpr, col = (q - row * qpr) * 4;
        // the rows this wave's 64 spans lie in: a primitive whose Y extent misses them is skipped by the whole wave
        const int q_first = q - ((int)threadIdx.x & (FA_WAVE - 1)), q_last = min(q_first + FA_WAVE - 1, total - 1);
        const int row_top = __builtin_amdgcn_readfirstlane(q_first / qpr), row_bot = __builtin_amdgcn_readfirstlane(q_last / qpr);
        const double y_top = -(((double)row_top + 0.5) / dsz * 2.0 - 1.0), y_bot = -(((double)row_bot + 0.5) / dsz * 2.0 - 1.0);
        // pixel centres in world coordinates, camera bounds +-1 (fortattack.py:582-587); row 0 = top
        const double Y = -(((double)row + 0.5) / dsz * 2.0 - 1.0);
        const bool yin = Y >= a.wall_ymin && Y <= a.wall_ymax, yout = Y > a.wall_ymax || Y < a.wall_ymin;
        double X[4];
        bool inside[4];
        float img[4][3];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            X[j] = ((double)(col + j) + 0.5) / dsz * 2.0 - 1.0;
            inside[j] = X[j] >= a.wall_xmin && X[j] <= a.wall_xmax;
            const float v = (inside[j] && yin) ? 0.0f : 1.0f; // white, then the black active region
            img[j][0] = img[j][1] = img[j][2] = v;
        }
        for (int p = 0; p < nprim; ++p) {
            const Prim &P = prims[p];
            if (y_bot > P.yhi || y_top < P.ylo) continue;
            bool hit[4];
            if (__builtin_amdgcn_readfirstlane(P.type) == PR_DISC) {
                const double dy = Y - P.d[1], dy2 = dy * dy;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const double dx = X[j] - P.d[0];
                    hit[j] = dx * dx + dy2 <= P.d[2];
                }
            } else {
                const double y1 = (Y - P.d[1]) * P.d[3], y2 = (Y - P.d[5]) * P.d[7], y3 = (Y - P.d[9]) * P.d[11];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const double s1 = (X[j] - P.d[0]) * P.d[2] - y1;
                    const double s2 = (X[j] - P.d[4]) * P.d[6] - y2;
                    const double s3 = (X[j] - P.d[8]) * P.d[10] - y3;
                    hit[j] = (s1 >= 0.0 && s2 >= 0.0 && s3 >= 0.0) || (s1 <= 0.0 && s2 <= 0.0 && s3 <= 0.0);
                }
            }
            const float om = P.om, c0 = P.ca[0], c1 = P.ca[1], c2 = P.ca[2];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (hit[j]) {
                    img[j][0] = img[j][0] * om + c0;
                    img[j][1] = img[j][1] * om + c1;
                    img[j][2] = img[j][2] * om + c2;
                }
            }
        }
        uint32_t b[12];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool strip = inside[j] && yout; // fortattack.py:548-560
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) b[j * 3 + ch] = to_u8(strip ? 0.5f : img[j][ch]);
        }
        uint8_t *const out = frame_out + ((size_t)row * size + col) * 3;
        const uintptr_t addr = reinterpret_cast<uintptr_t>(out);
        if (col + 4 <= size && (addr & 3) == 0) {
            uint32_t *o = reinterpret_cast<uint32_t *>(out);
#pragma unroll
            for (int w = 0; w < 3; ++w) o[w] = b[4 * w] | (b[4 * w + 1] << 8) | (b[4 * w + 2] << 16) | (b[4 * w + 3] << 24);
        } else if (col + 4 <= size && (addr & 1) == 0) {
            uint16_t *o = reinterpret_cast<uint16_t *>(out);
#pragma unroll
            for (int w = 0; w < 6; ++w) o[w] = (uint16_t)(b[2 * w] | (b[2 * w + 1] << 8));
        } else {
            const int nb = (size - col < 4 ? size - col : 4) * 3;
#pragma unroll
            for (int w = 0; w < 12; ++w)
                if (w < nb) out[w] = (uint8_t)b[w];
        }
    }
}
} // namespace

static int fa_render_tiles(int size) { // workgroups per frame (fa_render checks K * tiles against the grid limit)
    const long long total = (long long)size * ((size + 3) >> 2);
    const int per_wg = FA_RENDER_THREADS * FA_RENDER_QUADS;
    return (int)((total + per_wg - 1) / per_wg);
}

static hipError_t fa_launch_render(const FaRenderArgs &a, hipStream_t st) {
    const int tiles = fa_render_tiles(a.size);
    hipLaunchKernelGGL(fa_render_kernel, dim3((unsigned)((long long)a.K * tiles)), dim3(FA_RENDER_THREADS), 0, st, a, tiles);
    return hipGetLastError();
}

extern "C" int fa_render(fa_env *env, const fa_render_io *io, void *stream) {
    FA_ENTER(env, "fa_render", false, io);
    if (!io->env_index || !io->rgb) return fail(FA_ERR_INVALID, "fa_render: env_index and rgb are required");
    if (io->num_frames < 1) return fail(FA_ERR_INVALID, "fa_render: num_frames must be >= 1");
    if (io->size < 8 || io->size > 2048) return fail(FA_ERR_INVALID, "fa_render: size must be 8..2048");
    if ((io->team_attn != nullptr) != (io->opp_attn != nullptr))
        return fail(FA_ERR_INVALID, "fa_render: team_attn and opp_attn go together (the guards' pair, or neither)");
    if ((long long)io->num_frames * fa_render_tiles(io->size) > 0x7fffffffLL)
        return fail(FA_ERR_INVALID, "fa_render: num_frames x size is more than one launch covers");
    FaRenderArgs a;
    std::memset(&a, 0, sizeof(a));
    a.s = env->s;
    a.env_index = io->env_index;
    a.rgb = io->rgb;
    a.actions = io->actions;
    a.as_e = io->act_stride_env;
    a.as_i = io->act_stride_agent;
    a.no_laser = io->no_laser;
    a.team_attn = io->team_attn;
    a.opp_attn = io->opp_attn;
    a.K = io->num_frames;
    a.size = io->size;
    a.E = env->cfg.num_envs;
    a.G = env->cfg.num_guards;
    a.A = env->cfg.num_attackers;
    a.viz_dead = io->viz_dead != 0;
    a.attn_on = io->team_attn && io->viz_attn != 0;
    const FaDerived &c = env->c;
    a.agent_size = c.agent_size;
    a.fort_dim = c.fort_dim;
    a.door_x = c.door_x;
    a.door_y = c.door_y;
    a.wall_xmin = c.wall_xmin;
    a.wall_xmax = c.wall_xmax;
    a.wall_ymin = c.wall_ymin;
    a.wall_ymax = c.wall_ymax;
    a.shoot_rad = c.shoot_rad;
    a.half_win = c.half_win;
    FA_HIP(fa_launch_render(a, static_cast<hipStream_t>(stream)));
    return FA_OK;
}
