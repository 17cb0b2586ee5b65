"""Times of the behaviour pass (csrc/fa_behaviour.hip) at the size a user would run -> one JSON line.

    python tools/time_behaviour.py [--only plain|behaviour] [--reps N]

5v5 x 4096 envs, 5 x 5 policies, chunks of T = 100 steps, everything replayed from hipGraphs.

* kernel: the fa_behaviour_chunk launch alone, captured in a graph of its own, over the storage a played chunk left; a
  device-event pair around every replay, 5 warm-up replays, `--reps` timed ones (default 30): median / min / max.  Two
  records: without a quota (every row is swept: the most work a chunk can be) and with 3 episodes per env on the first chunk
  of a match.  fa_behaviour_begin before every replay (outside the event pair), so every replay does the same work.  The bytes
  are the ones the pass needs, from the shapes: T * E * N * (24 obs + 8 action) + T * E done; the rate is bytes over the
  median.
* crossplay: one chunk of two evaluators side by side, `plain` (behaviour=False) and `behaviour` (behaviour=True), replayed
  alternately, two warm-up replays and `--reps` timed ones each.  --only times one of them alone in its process: side by side, the
  chunk without the option measured 1.5 % slower than the same chunk alone in a process of its own (profiles/behaviour.md; the
  cause was not looked for), so figures of the two set-ups do not compare.  `--only plain` also runs on a checkout without
  the option (the parent of the commit that added it), for the comparison across commits: alternate the processes.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import emergent_multiagent_strategies_amd as fa  # noqa: E402

G = A = 5
E, POOL, T, MAXT, QUOTA = 4096, 5, 100, 100, 3


def _stats(ms):
    ms = sorted(ms)
    return dict(median_ms=round(ms[len(ms) // 2], 4), min_ms=round(ms[0], 4), max_ms=round(ms[-1], 4), launches=len(ms))


def _pools():
    def policy(a, b, seed):
        torch.manual_seed(seed)
        pol = fa.MPNN(num_agents=a, num_opp_agents=b, num_actions=8).cuda().eval()
        for p in pol.parameters():
            p.requires_grad_(False)
        return pol
    return [policy(G, A, 10 + k) for k in range(POOL)], [policy(A, G, 20 + k) for k in range(POOL)]


def _timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def time_kernel(cp, reps):
    """The launch alone, over the storage the evaluator's last chunk left."""
    eng = cp.eng
    cp._counter.add_(1)
    cp._graph.replay()                          # a played chunk in the storage (after_update cleared the last one)
    torch.cuda.synchronize()
    nbytes = T * E * eng.N * (24 + 8) + T * E
    out = dict(bytes=nbytes, slices_of=16)
    for name, quota in (("no_quota", 0), ("quota_%d" % QUOTA, QUOTA)):
        bm = fa.BehaviourMaps(eng, cp.cell, cp.n_cells, quota)
        bm.begin()
        bm.chunk()                              # the code object is loaded
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            bm.chunk()
        ms = []
        for rep in range(5 + reps):
            bm.begin()
            t = _timed(g.replay)
            if rep >= 5:
                ms.append(t)
        st = _stats(ms)
        counts = bm.counts()
        out[name] = dict(GBps=round(nbytes / (st["median_ms"] * 1e-3) / 1e9, 1), steps_counted=int(counts["steps"].sum()),
                         agent_steps_counted=int(counts["occ"].sum()), **st)
    return out


def time_crossplay(names, reps):
    guards, attackers = _pools()
    cps = {}
    for name in names:
        eng = fa.BatchedFortAttack(E, G, A, MAXT, base_seed=1)
        kw = dict(behaviour=True) if name == "behaviour" else {}
        cp = fa.CrossPlay(eng, guards, attackers, QUOTA, num_steps=T, sample_seed=2, use_graph=True, **kw)
        cp.begin()
        cps[name] = cp
    ms = {k: [] for k in cps}
    for rep in range(2 + reps):
        for name, cp in cps.items():
            cp._counter.add_(1)
            t = _timed(cp._graph.replay)
            cp.eng.after_update()
            if rep >= 2:                                  # two warm-up replays each
                ms[name].append(t)
    out = {"chunk_steps": T, "envs": E, "policies": [POOL, POOL]}
    for name in cps:
        out[name] = _stats(ms[name])
        out[name]["env_steps_per_s"] = round(T * E / (out[name]["median_ms"] * 1e-3))
    if "behaviour" in out and "plain" in out:
        out["behaviour_over_plain"] = round(out["behaviour"]["median_ms"] / out["plain"]["median_ms"], 4)
    return out, cps


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--only", choices=["plain", "behaviour"], default=None)
    p.add_argument("--reps", type=int, default=30)
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_behaviour.py measures on the GPU: none found")
    names = (args.only,) if args.only else ("plain", "behaviour")
    cross, cps = time_crossplay(names, args.reps)
    out = dict(crossplay=cross)
    if args.only != "plain":
        out["kernel"] = time_kernel(cps[names[0]], args.reps)
        k, c = out["kernel"]["no_quota"]["median_ms"], cross[names[0]]["median_ms"]
        out["kernel_share_of_chunk"] = round(k / c, 5)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
