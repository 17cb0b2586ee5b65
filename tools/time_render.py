"""Times of the batched frame renderer (csrc/fa_render.hip) at sizes a user would run -> one JSON line.

    python tools/time_render.py [--hbm-copy-gbs X] [--skip-crossplay]

* kernel: 5v5, E = 4096, frames of 350 and 128 pixels, K = 256 and 4096 frames per launch; a device-event pair around every
  launch, 3 warm-up launches, 25 timed ones: median / min / max, time per frame, output bytes per second (K * size^2 * 3 over
  the launch time).  --hbm-copy-gbs: the copy figure tools/ubench_hbm gave on the same visit (1 read + 1 write): the share
  is taken against half of it, the write stream of that copy.
* numpy: render.render_frame of one such frame on the host's CPU, the path the kernel replaces.
* crossplay: one chunk (100 steps, graph replay) of 5v5 x 4096 envs, 5 x 5 policies, with and without a 25-env recorder of 128
  pixels: two evaluators side by side, replayed alternately, 10 times each.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import emergent_multiagent_strategies_amd as fa  # noqa: E402


def _stats(ms):
    ms = sorted(ms)
    return dict(median_ms=round(ms[len(ms) // 2], 4), min_ms=round(ms[0], 4), max_ms=round(ms[-1], 4), launches=len(ms))


def _scene(eng, seed=0):
    """A reset world, random actions (a quarter shoot) and row-normalised attention: what a recorder draws."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    eng.reset()
    act = torch.randint(0, 8, (eng.E, eng.N), device="cuda", generator=g)
    act[torch.rand((eng.E, eng.N), device="cuda", generator=g) < 0.25] = 7
    team = torch.rand((eng.E, eng.G, eng.G), device="cuda", generator=g)
    opp = torch.rand((eng.E, eng.G, eng.A), device="cuda", generator=g)
    return act, (team / team.sum(-1, keepdim=True)).contiguous(), (opp / opp.sum(-1, keepdim=True)).contiguous()


def time_kernel(hbm_copy_gbs):
    G = A = 5
    E = 4096
    eng = fa.BatchedFortAttack(E, G, A, 100)
    act, team, opp = _scene(eng)
    rows = []
    for size in (350, 128):
        for K in (256, 4096):
            idx = (torch.arange(K, device="cuda", dtype=torch.int32) * (E // K)).contiguous()
            out = torch.empty((K, size, size, 3), dtype=torch.uint8, device="cuda")
            kw = dict(size=size, actions=act, attn=(team, opp), out=out)
            for _ in range(3):
                eng.render(idx, **kw)
            torch.cuda.synchronize()
            ms = []
            for _ in range(25):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                eng.render(idx, **kw)
                b.record()
                b.synchronize()
                ms.append(a.elapsed_time(b))
            st = _stats(ms)
            nbytes = K * size * size * 3
            row = dict(size=size, K=K, out_bytes=nbytes, us_per_frame=round(st["median_ms"] * 1e3 / K, 3),
                       out_GBps=round(nbytes / (st["median_ms"] * 1e-3) / 1e9, 1), **st)
            if hbm_copy_gbs:
                row["share_of_hbm_write"] = round(row["out_GBps"] / (hbm_copy_gbs / 2.0), 4)
            rows.append(row)
    # the numpy path on the host's CPU, one frame of the same scene
    s = eng.get_state()
    a_h, t_h, o_h = act.cpu().numpy(), team.cpu().numpy(), opp.cpu().numpy()
    cpu = {}
    for size in (350, 128):
        t0 = time.perf_counter()
        for e in range(3):
            fa.render.render_frame(s["pos_x"][e], s["pos_y"][e], s["ang"][e], s["alive"][e], G, shoot=a_h[e] == 7, size=size,
                                   attn_list=[[t_h[e], o_h[e]]])
        cpu["numpy_ms_per_frame_size%d" % size] = round((time.perf_counter() - t0) / 3 * 1e3, 3)
    eng.close()
    return rows, cpu


def time_crossplay():
    G = A = 5
    E, n = 4096, 5

    def policy(a, b, seed):
        torch.manual_seed(seed)
        pol = fa.MPNN(num_agents=a, num_opp_agents=b, num_actions=8).cuda().eval()
        for p in pol.parameters():
            p.requires_grad_(False)
        return pol

    guards, attackers = [policy(G, A, 10 + k) for k in range(n)], [policy(A, G, 20 + k) for k in range(n)]
    cps = {}
    for name in ("plain", "recorded"):
        eng = fa.BatchedFortAttack(E, G, A, 100, base_seed=1)
        cp = fa.CrossPlay(eng, guards, attackers, 3, sample_seed=2, use_graph=True)
        if name == "recorded":
            cp.recorder = fa.EpisodeRecorder(eng, cp.record_envs(1), cp.T, size=128)
        cp.begin()
        cps[name] = cp
    ms = {k: [] for k in cps}
    for rep in range(12):
        for name, cp in cps.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            cp._counter.add_(1)
            a.record()
            cp._graph.replay()
            b.record()
            b.synchronize()
            cp.eng.after_update()
            if rep >= 2:                                  # two warm-up replays each
                ms[name].append(a.elapsed_time(b))
    out = {"chunk_steps": cps["plain"].T, "recorded_envs": int(cps["recorded"].recorder.K), "record_size": 128}
    for name in cps:
        out[name] = _stats(ms[name])
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--hbm-copy-gbs", type=float, default=None)
    p.add_argument("--skip-crossplay", action="store_true")
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_render.py measures on the GPU: none found")
    rows, cpu = time_kernel(args.hbm_copy_gbs)
    out = dict(kernel=rows, cpu=cpu, hbm_copy_GBps=args.hbm_copy_gbs)
    if not args.skip_crossplay:
        out["crossplay"] = time_crossplay()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
