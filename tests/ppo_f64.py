"""The float64 judge of the fused PPO gradient (csrc/fa_train.hip fa_ppo_grad) and its fixtures; shared by
tests/test_ppo_f64_cpu.py (fixture conditions, the judge against deliberately wrong references) and the GPU tests
(tests/test_gpu_ppo_grad_f64.py, tests/test_gpu_policy.py).  Everything here is built with CPU generators, so both see
the same bits; the GPU tests move the tensors.

The bar.  For every kernel-facing tensor (mpnn_pack.split_plain's layout) and every loss sum

    e_fused = max|got - g64| / S,   e_f32 = max|g32 - g64| / S,   S = max|g64| of that tensor
    e_fused <= factor * e_f32 + floor

where g64 / g32 are torch autograd through mpnn_pack.folded_ppo_reference in float64 / float32 on the same float32
inputs: the kernel may be `factor` times as far from the exact gradient as float32 autograd is, plus `floor` (16 ulp of
the tensor's largest entry).  An element whose float64 gradient is exactly zero (A_m of a team of one, A_o against one
opponent, the policy-head blocks of a value-only run, the structural zeros of W9, units that are dead on every row)
must come out exactly zero.

A float32 gradient is only defined away from the kinks of the function: a relu input, or a PPO clip boundary, within
float32 rounding of zero falls on either side depending on the summation order.  Envs are independent in the forward,
so make_case replaces exactly the envs whose FLOAT64 forward comes within KINK_MARGIN of a relu kink or LOSS_MARGIN of a
loss kink (never judged by a kernel output) by envs drawn from a follow-on seed, and reports the share it replaced."""
import functools
import math

import torch

from emergent_multiagent_strategies_amd import mpnn_pack as mp_
from emergent_multiagent_strategies_amd.mpnn import MPNN

CLIP = 0.2
KINK_MARGIN = 2e-6        # |relu input|, float64 (tests/test_gpu_policy.py has used this margin for its batches)
LOSS_MARGIN = 1e-4        # distance of a row from a clip boundary: 10 x the forward's observed 1e-5
MAX_REPLACED = 0.10
FLOOR = 1e-6              # tests/test_gpu_learner.py ERR_FLOOR: ~16 ulp of the tensor's largest entry
# docs/parity.md "fa_ppo_grad against float64": twice the largest e_fused / e_f32 of any tensor over every case below
# (2.16), rounded up to a power of two
FACTOR = 8.0
# The saturated fixtures have their own: 2 x 7.4 -> 16 and 2 x 11.6 -> 32.  Located from the kernel's operand records:
# the trunk's forward is as close to float64 as torch's float32 (4e-7 of max |h3|, both); from the SAME recorded h3 the
# heads + losses + way back to d[P | V] are 1.1e-5 / 1.4e-4 off where torch's float32 is 4.0e-6 / 3.1e-5.  The logits reach
# 25 / 320 there: an absolute error of a few ulp of the largest logit (1.9e-6 / 3.1e-5; the kernel's K = 128 chain of the
# W9 product leaves ~5, rocBLAS ~2; ~1.7 and ~1 at the ordinary fixtures' logits of 0.9) IS the relative error of every
# probability, and with it of the whole gradient.  That is the softmax's conditioning, not a defect of a stage.
FACTOR_BY_KIND = dict(saturated=16.0, underflow=32.0)
SUMS = ("vl", "al", "en", "mm")
BRANCH_R = (0.5, 0.79, 0.81, 1.0, 1.19, 1.21, 2.0)
BRANCH_D = (-0.5, -0.21, -0.19, 0.19, 0.21, 0.5)
ACTION_CELLS = ("in_range", "hi_adv_pos", "hi_adv_neg", "lo_adv_pos", "lo_adv_neg")
VALUE_CELLS = ("outside_l1", "outside_l2", "inside")

# ---- the case lists of the GPU tests (tests/test_ppo_f64_cpu.py checks every fixture's conditions) -----------------
# one case per tile count; ET = 32 // max(G, A) envs per tile; every second one ends in a ragged tile of one env
TILE_EDGE_COUNTS = (1, 2, 55, 56, 57, 63, 64, 65, 66, 67, 129, 201, 257)
TILE_CASES = (   # (G, A, team, tiles, ragged)                                      kernel build
    (3, 3, 0, 1, True), (2, 4, 1, 55, False), (3, 3, 1, 57, True), (4, 2, 0, 63, True), (1, 3, 1, 66, False),    # MT = 4
    (5, 5, 0, 2, True), (6, 3, 1, 56, False), (5, 5, 1, 64, False), (5, 5, 0, 129, False),                      # MT = 6
    (8, 8, 0, 65, True), (8, 1, 0, 67, True), (1, 8, 0, 201, True), (8, 8, 1, 257, False))                      # MT = 8
TERM_CASES = ((3, 3, 0, 197), (5, 5, 1, 118), (8, 8, 0, 79))          # (G, A, team, B): 20 tiles each, kind "branches"
MODE_CASES = ((3, 3, 1, 260), (5, 5, 0, 150))
GATHER_ROWS, GATHER_ALIVE = 900, 0.6
SATURATED_CASE, UNDERFLOW_CASE, ALL_DEAD_CASE = (5, 5, 0, 118, "saturated", 9, 0.7), (3, 3, 1, 95, "underflow", 9, 0.7), (3, 3, 0, 95, "all_dead", 13, 0.7)
# dist.linear.weight times this, on top of the fixture's 3: "saturated" reaches log-probabilities of -40 (probabilities of
# 5e-18: their entropy terms vanish below float32 resolution), "underflow" -400 (exp() is 0 in float32)
DIST_GAIN = dict(saturated=30.0, underflow=300.0)
LEGACY_CASES = ((3, 3, 0, 500, True), (3, 3, 1, 21, True), (3, 3, 0, 43, False), (5, 5, 1, 200, True), (2, 4, 0, 100, True),
                (4, 2, 1, 77, True), (8, 8, 0, 37, True), (7, 8, 1, 26, True), (1, 3, 0, 50, True))


def tile_envs(G, A):
    return 32 // max(G, A)


def tile_case_envs(G, A, tiles, ragged):
    ET = tile_envs(G, A)
    return ET * (tiles - 1) + 1 if ragged else ET * tiles


def all_gpu_fixtures():
    """(G, A, team, B, kind, seed, alive) of every fixture the GPU tests build."""
    out = [(G, A, team, tile_case_envs(G, A, tiles, ragged), "random", 100 + tiles, 0.7) for G, A, team, tiles, ragged in TILE_CASES]
    out += [(G, A, team, B, "branches", 9, 0.7) for G, A, team, B in TERM_CASES]
    for G, A, team, B in MODE_CASES:
        out += [(G, A, team, B, "random", 5, 0.7), (G, A, team, GATHER_ROWS, "random", 17, GATHER_ALIVE)]
    out += [SATURATED_CASE, UNDERFLOW_CASE, ALL_DEAD_CASE]
    out += [(G, A, team, B, "random", B, 0.7) for G, A, team, B, _ in LEGACY_CASES]
    return out


# ---- fixtures -----------------------------------------------------------------------------------------------------------
def _policy(G, A, team, seed, dist_gain):
    """tests/test_gpu_policy.py::_policies on the CPU: non-zero biases, larger logits than the 0.01-gain init gives."""
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        pols = [MPNN(num_agents=G, num_opp_agents=A, num_actions=8), MPNN(num_agents=A, num_opp_agents=G, num_actions=8)]
        for pol in pols:
            for p in pol.parameters():
                if p.dim() == 1:
                    p.data.uniform_(-0.3, 0.3)
            pol.dist.linear.weight.data.mul_(dist_gain)
    return pols[team]


def _draw(B, N, seed, alive):
    """One batch of today's distributions (tests/test_gpu_policy.py::_obs and the rows of its fa_ppo_grad tests)."""
    g = torch.Generator().manual_seed(seed)
    obs = torch.randn((B, N, 6), generator=g)
    obs[:, :, 0] = (torch.rand((B, N), generator=g) > 1.0 - alive).float()
    obs[:, :, 3] = obs[:, :, 3] * 3 + 4.7                            # headings are O(1..10)
    rnd = lambda: torch.randn((B, N, 1), generator=g)
    action = torch.randint(0, 8, (B, N, 1), generator=g)
    value_pred, ret, adv = rnd(), rnd(), rnd()
    old_logp = -torch.rand((B, N, 1), generator=g) * 2.5
    return dict(obs=obs.contiguous(), action=action, value_pred=value_pred, ret=ret, adv=adv, old_logp=old_logp)


@torch.no_grad()
def forward64(P, obs, own_sl, opp_sl):
    """mpnn_pack._forward in float64 with its relu inputs kept: -> (smallest |relu input| per env (B,), log-softmax
    (B, n, 8), value (B, n, 1))."""
    P = {k: v.detach().double() for k, v in P.items()}
    own, opp = obs[:, own_sl].double(), obs[:, opp_sl].double()
    n = own.shape[1]
    z = [own @ P["WE"] + P["BE"], opp @ P["WOE"] + P["BOE"]]
    h1, ho = torch.relu(z[0]), torch.relu(z[1])
    att = torch.softmax((h1 @ P["AO"]) @ ho.transpose(1, 2), dim=-1)
    h = torch.cat((h1, (att @ ho) @ P["BO"]), dim=2)
    diag = torch.zeros(n, n, dtype=torch.float64).fill_diagonal_(-float("inf"))
    for _ in range(3):
        mix = torch.softmax((h @ P["AM"]) @ h.transpose(1, 2) + diag, dim=-1) @ h if n > 1 else torch.zeros_like(h)
        z.append(torch.cat((h, mix), dim=2) @ P["W7"] + P["BU"])
        h = torch.relu(z[-1])
    z.append(h @ P["W8"] + P["B8"])
    out = torch.relu(z[-1]) @ P["W9"] + P["B9"]
    margin = torch.stack([t.abs().flatten(1).min(1).values for t in z]).min(0).values
    return margin, torch.log_softmax(out[..., :8], dim=-1), out[..., 8:9]


def _loss_rows(logp_all, value, rows, own_sl):
    """Float64, per own row (B, n): alive, ratio, adv, dv = value - value_pred, l1 - l2 of the clipped value loss."""
    alive = rows["obs"][:, own_sl, 0] > 0
    lp = logp_all.gather(-1, rows["action"][:, own_sl])[..., 0]
    ratio = torch.exp(lp - rows["old_logp"][:, own_sl, 0].double())
    adv = rows["adv"][:, own_sl, 0].double()
    vp, rt, v = rows["value_pred"][:, own_sl, 0].double(), rows["ret"][:, own_sl, 0].double(), value[..., 0]
    dv = v - vp
    vc = vp + dv.clamp(-CLIP, CLIP)
    return alive, ratio, adv, dv, (v - rt).pow(2) - (vc - rt).pow(2)


def loss_kink_margin(logp_all, value, rows, own_sl):
    """Per env: the smallest distance of an alive own row from a kink of the PPO losses (fa_train.hip:553-571) --
    |ratio - (1 +- clip)|, ||dv| - clip|, |l1 - l2| outside the clip, |adv|.  A dead row's loss terms are zero."""
    alive, ratio, adv, dv, dl = _loss_rows(logp_all, value, rows, own_sl)
    d = torch.minimum((ratio - (1 - CLIP)).abs(), (ratio - (1 + CLIP)).abs())
    d = torch.minimum(d, adv.abs())
    d = torch.minimum(d, (dv.abs() - CLIP).abs())
    d = torch.where(dv.abs() > CLIP, torch.minimum(d, dl.abs()), d)
    d = torch.where(alive, d, torch.full_like(d, float("inf")))
    return d.min(1).values


def branch_cells(logp_all, value, rows, own_sl):
    """Alive own rows per cell of the two clipped losses -> ({cell: count}, alive rows)."""
    alive, ratio, adv, dv, dl = _loss_rows(logp_all, value, rows, own_sl)
    hi, lo, pos = ratio >= 1 + CLIP, ratio <= 1 - CLIP, adv > 0
    outside = dv.abs() >= CLIP
    masks = dict(in_range=~hi & ~lo, hi_adv_pos=hi & pos, hi_adv_neg=hi & ~pos, lo_adv_pos=lo & pos, lo_adv_neg=lo & ~pos,
                 outside_l1=outside & (dl >= 0), outside_l2=outside & (dl < 0), inside=~outside)
    return {k: int((m & alive).sum()) for k, m in masks.items()}, int(alive.sum())


def _place_branches(rows, logp_all, value, own_sl, seed):
    """kind "branches": old_logp, adv, value_pred and ret of the own rows from the float64 forward, so that every cell
    of the clipped action loss (in range; ratio high / low x sign of adv) and of the clipped value loss (outside the
    clip with l1 >= l2, with l2 > l1; inside) holds a fixed share of the rows whatever the policy computes."""
    B, n = value.shape[:2]
    g = torch.Generator().manual_seed(seed)
    i = torch.arange(B * n).view(B, n)
    lp = logp_all.gather(-1, rows["action"][:, own_sl])[..., 0]
    r = torch.tensor(BRANCH_R, dtype=torch.float64)[i % len(BRANCH_R)]
    d = torch.tensor(BRANCH_D, dtype=torch.float64)[i % len(BRANCH_D)]
    mag = lambda: 0.5 + torch.rand((B, n), generator=g).double()
    sign = lambda k: 1.0 - 2.0 * (k % 2).double()
    # (the sign of adv runs with period 2 against r's period 7; the side of ret with period 12 against d's period 6.  ret
    #  lies 1.5 x as far above value as below: with equal distances sum(value - ret), the one non-zero entry of dB9 in a
    #  value-only run, would cancel to ~2 % of its terms and its float32 error be judged at 50 x its size)
    side = sign(i // len(BRANCH_D))
    own = dict(old_logp=lp - torch.log(r), adv=sign(i + 1) * mag(), value_pred=value[..., 0] - d,
               ret=value[..., 0] + side * mag() * (1.25 + 0.25 * side))
    for k, v in own.items():
        rows[k][:, own_sl, 0] = v.float()


@functools.lru_cache(maxsize=None)
def make_case(G, A, team, B, kind="random", seed=0, alive=0.7):
    """One team's minibatch for fa_ppo_grad as a dict of CPU tensors: the policy (`pol`, its kernel-facing float32
    matrices `P`), obs / action / value_pred / ret / adv / old_logp of all N agents, `replaced` (the share of envs the
    kink rejection replaced), `relu_margin` / `loss_margin` (what the fixture keeps, float64) and, kind "branches", `cells`."""
    assert kind in ("random", "branches", "saturated", "underflow", "all_dead")
    N = G + A
    own_sl, opp_sl = (slice(0, G), slice(G, N)) if team == 0 else (slice(G, N), slice(0, G))
    pol = _policy(G, A, team, 11 + team, 3.0 * DIST_GAIN.get(kind, 1.0))
    P = {k: v.detach().clone() for k, v in mp_.kernel_params(pol).items()}

    def draw(b, s):
        rows = _draw(b, N, s, alive)
        if kind == "all_dead":
            rows["obs"][:, own_sl, 0] = 0.0
        margin, logp_all, value = forward64(P, rows["obs"], own_sl, opp_sl)
        if kind == "branches":
            _place_branches(rows, logp_all, value, own_sl, s)
        return rows, margin, loss_kink_margin(logp_all, value, rows, own_sl)

    rows, relu_m, loss_m = draw(B, seed)
    bad = ((relu_m < KINK_MARGIN) | (loss_m < LOSS_MARGIN)).nonzero()[:, 0]
    replaced = int(bad.numel())
    for k in range(1, 200):
        if bad.numel() == 0:
            break
        fresh, fr, fl = draw(bad.numel(), seed + 1000 * k)
        for key in rows:
            rows[key][bad] = fresh[key]
        relu_m[bad], loss_m[bad] = fr, fl
        if kind == "branches":       # the placement cycles with the row index: redo it for the rows' final places
            margin, logp_all, value = forward64(P, rows["obs"], own_sl, opp_sl)
            _place_branches(rows, logp_all, value, own_sl, seed)
            relu_m, loss_m = margin, loss_kink_margin(logp_all, value, rows, own_sl)
        bad = ((relu_m < KINK_MARGIN) | (loss_m < LOSS_MARGIN)).nonzero()[:, 0]
        replaced += int(bad.numel())
    assert bad.numel() == 0, "no replacement off the kinks"
    case = dict(G=G, A=A, team=team, B=B, N=N, n=G if team == 0 else A, kind=kind, own_sl=own_sl, opp_sl=opp_sl, pol=pol, P=P,
                replaced=replaced / B, relu_margin=float(relu_m.min()), loss_margin=float(loss_m.min()), **rows)
    if kind == "branches":
        _, logp_all, value = forward64(P, rows["obs"], own_sl, opp_sl)
        case["cells"], case["alive_rows"] = branch_cells(logp_all, value, rows, own_sl)
    return case


def on_device(case, device):
    """The case with its tensors moved (the policy stays where it is)."""
    out = dict(case)
    out["P"] = {k: v.to(device) for k, v in case["P"].items()}
    for k in ("obs", "action", "value_pred", "ret", "adv", "old_logp"):
        out[k] = case[k].to(device).contiguous()
    return out


# ---- the reference ------------------------------------------------------------------------------------------------------
REAL_W9 = torch.zeros(256, 32, dtype=torch.bool)     # W9 is block diagonal: dist.linear.weight^T and value_head.2.weight^T
REAL_W9[:128, :8] = True
REAL_W9[128:, 8] = True


def finish(grads, sums):
    """Gradients of the kernel-facing matrices -> float64, W9 masked to the entries that are parameters (autograd treats
    W9 as dense), B9 cut to its nine real entries; the four loss sums as a float64 tensor."""
    out = {k: v.detach().double() for k, v in grads.items()}
    out["W9"] = out["W9"] * REAL_W9.to(out["W9"].device)
    out["B9"] = out["B9"][:9]
    return out, torch.stack([torch.as_tensor(s).detach().double().reshape(()) for s in sums])


def compose(vl, al, en, mm, c_v, c_e, clipped, normalize, deferred=False):
    """The loss the kernel differentiates (fa_train.hip:517-576, ppo.py:146-187): with normalize the masked terms are
    divided by the alive-mask mean (1 when nobody is alive); the unclipped value loss is a plain mean and is not.
    deferred: the library's normalize = 0 with its own mask mean -- the division is left to after the ranks' all-reduce,
    so the unclipped value loss goes out MULTIPLIED by the mask mean (learner.ppo_losses normalize=False: (vl * mask).mean())."""
    um = mm if float(mm) != 0.0 else 1.0
    if deferred:
        assert not normalize
        return c_v * vl * (1.0 if clipped else um) + al - c_e * en
    if not normalize:
        return c_v * vl + al - c_e * en
    return (c_v * vl + al - c_e * en) / um if clipped else c_v * vl + (al - c_e * en) / um


def reference(case, dtype, c_v, c_e, clipped, normalize, idx=None, adv=None, loss_fn=None, deferred=False):
    """torch autograd through mpnn_pack.folded_ppo_reference in `dtype` on the case's float32 inputs (rows idx of them;
    `adv` replaces the case's advantages) -> (gradients in split_plain's layout, (vl, al, en, mm)), float64 tensors on
    the case's device.  loss_fn: a stand-in for folded_ppo_reference (the CPU test's wrong variants)."""
    P = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in case["P"].items()}
    sel = (lambda t: t) if idx is None else (lambda t: t[idx])
    own = case["own_sl"]
    rows = [sel(case["action"])[:, own]] + [sel(t).to(dtype)[:, own] for t in
                                            (case["value_pred"], case["ret"], case["old_logp"], case["adv"] if adv is None else adv)]
    fn = loss_fn or mp_.folded_ppo_reference
    _, vl, al, en, mm = fn(P, sel(case["obs"]).to(dtype), own, case["opp_sl"], *rows, CLIP, c_v, c_e, clipped)
    compose(vl, al, en, mm, c_v, c_e, clipped, normalize, deferred).backward()
    return finish({k: torch.zeros_like(p) if p.grad is None else p.grad for k, p in P.items()}, (vl, al, en, mm))


def kernel_result(out, rows):
    """fa_ppo_grad's output buffer -> what reference() returns (the loss sums divided by the rows own-team rows)."""
    L = mp_.PLAIN_FLOATS
    return finish({k: v.clone() for k, v in mp_.split_plain(out).items()}, out[L:L + 4].double() / rows)


# ---- the judge ----------------------------------------------------------------------------------------------------------
def judge(got, g64, g32, factor=FACTOR, floor=FLOOR, tag=None, residue=()):
    """got / g64 / g32: (gradients, sums) as reference() returns them.  Asserts, for every tensor and every loss sum,
    e_fused <= factor * e_f32 + floor and exact zeros where float64 is exactly zero; -> {name: (e_fused, e_f32, ratio)}.
    tag: print the figures (one JUDGE line, what docs/parity.md's table was collected from) before asserting.
    residue: tensors whose float64-zero entries may hold a rounding residue here, bounded by floor x the largest entry
    over ALL tensors (docs/parity.md: A_o against one opponent in the tile kernel's builds for teams above four)."""
    largest = max(float(g64[0][k].abs().max()) for k in mp_.PLAIN_SHAPES)
    items = [(k, got[0][k], g64[0][k], g32[0][k]) for k in mp_.PLAIN_SHAPES]
    items += [(k, got[1][j], g64[1][j], g32[1][j]) for j, k in enumerate(SUMS)]
    table, bad = {}, []
    for k, a, w, b in items:
        a, w, b = a.double().reshape(-1), w.reshape(-1), b.double().reshape(-1)
        if not bool(torch.isfinite(a).all()):
            bad.append("%s: not finite" % k)
            continue
        zero = w == 0
        if k in residue and bool(zero.any()):
            table[k + ".residue"] = (float(a[zero].abs().max()) / largest if largest > 0 else 0.0, 0.0, 0.0)
            if not float(a[zero].abs().max()) <= floor * largest:
                bad.append("%s: residue %.2e where float64 is zero > %g x %.2e" % (k, float(a[zero].abs().max()), floor, largest))
        elif bool((a[zero] != 0).any()):
            bad.append("%s: %d entries are exactly zero in float64 and not here (largest %.2e)"
                       % (k, int((a[zero] != 0).sum()), float(a[zero].abs().max())))
        S = float(w.abs().max())
        if S == 0.0:
            table[k] = (0.0, 0.0, 0.0)
            continue
        e_fused, e_f32 = float((a - w).abs().max()) / S, float((b - w).abs().max()) / S
        table[k] = (e_fused, e_f32, e_fused / e_f32 if e_f32 > 0 else (math.inf if e_fused > 0 else 0.0))
        if not e_fused <= factor * e_f32 + floor:
            bad.append("%s: e_fused %.2e > %g x e_f32 %.2e + %g" % (k, e_fused, factor, e_f32, floor))
    if tag is not None:
        print("JUDGE %s %s" % (tag, " ".join("%s=%.2e/%.2e" % (k, v[0], v[1]) for k, v in table.items())))
    assert not bad, "; ".join(bad)
    return table
