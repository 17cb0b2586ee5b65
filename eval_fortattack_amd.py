#!/usr/bin/env python
"""Cross-play evaluation with the reference's flag names (test_fortattack_v2.py, test_fortattack_v2_gen_plot_data.py): every
guard checkpoint of a series against every attacker strategy, the whole matrix on one handle of --num-processes envs.

    python eval_fortattack_amd.py --guard-load-dir run1 --guard-ckpts 100 200 300 --attacker-load-dir attackers \\
        -l 220 650 1240 1600 2520 --num-eval-episodes 3 --num-processes 4096 --out-dir stats

Writes to --out-dir:
  crossplay.npz                               raw per-cell sums, the (guards, attackers, 8) table, both checkpoint lists
  stats_ensemble_strategies_ep<guard>.csv     per guard checkpoint: the K x 8 table rounded to two places
                                              (test_fortattack_v2.py:120-124)
  reward_data_ensemble.npy                    only with --num-eval-episodes 1: (guard ckpts, K x episodes, 1 + N), column 0
                                              the guard checkpoint, then every agent's episode return
                                              (test_fortattack_v2_gen_plot_data.py:55,117-118)
  video_g<guard>_a<attacker>_env<e>_ep<i>.gif only with --record: the first --record-episodes episodes of the first
                                              --record-per-cell envs of every match-up, --record-size pixels a side, drawn on
                                              the device with the guards' attention (test_fortattack.py --render --record
                                              --video-format gif); .npz (array ep0) with --video-format npz
  behaviour.npz                               only with --behaviour: the integer behaviour maps of every match-up (steps,
                                              episodes, len_hist, alive_t, occ, shots, deaths, each with a leading
                                              guards x attackers axis), summed on the device over the episodes that count
                                              for the match; `fingerprints` (guards, attackers, columns) and `columns`
  fingerprints.csv                            only with --behaviour: one row per match-up: guard, attacker, the fingerprint
                                              columns (behaviour.FINGERPRINT_COLUMNS)
  behaviour_g<guard>_a<attacker>.png          only with --behaviour: the match-up's occ / shots / deaths maps, guards above
                                              attackers

Differences from the reference scripts: --num-eval-episodes counts episodes PER ENV (every match-up is played by
num-processes / (guards x attackers) envs, so it gets that many times as many episodes); --guard-ckpts names the series
(default: every ep*.pt of --guard-load-dir, sorted by number); --num-guards/--num-attackers exist.
"""
import argparse
import os
import re


def get_args(argv=None):
    p = argparse.ArgumentParser(description="cross-play evaluation")
    p.add_argument("--num-guards", type=int, default=5)
    p.add_argument("--num-attackers", type=int, default=5)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--num-processes", type=int, default=4096, help="envs on the GPU (reference: 1)")
    p.add_argument("--num-env-steps", type=int, default=100, help="max steps per episode")
    p.add_argument("--num-eval-episodes", type=int, default=3, help="episodes per env")
    p.add_argument("--guard-load-dir", default="tmp")
    p.add_argument("--guard-ckpts", nargs="+", type=int, default=None, help="default: every ep*.pt of --guard-load-dir")
    p.add_argument("--attacker-load-dir", default="tmp")
    p.add_argument("-l", "--attacker-ckpts", nargs="+", type=int, default=[220, 650, 1240, 1600, 2520])
    p.add_argument("--deterministic", action="store_true", help="argmax actions (the reference samples)")
    p.add_argument("--no-graph", action="store_true", help="do not replay the chunk from a hipGraph")
    p.add_argument("--out-dir", default=None, help="default: --guard-load-dir")
    p.add_argument("--record", action="store_true", help="write one video per recorded episode of every match-up")
    p.add_argument("--video-format", choices=["gif", "npz"], default="gif")
    p.add_argument("--record-size", type=int, default=128, help="frame side in pixels")
    p.add_argument("--record-per-cell", type=int, default=1, help="envs recorded per match-up")
    p.add_argument("--record-episodes", type=int, default=1, help="episodes recorded per env (<= --num-eval-episodes)")
    p.add_argument("--behaviour", action="store_true",
                   help="write the behaviour maps and strategy fingerprints of every match-up (behaviour.npz, fingerprints.csv, PNGs)")
    args = p.parse_args(argv)
    if args.record and not 1 <= args.record_episodes <= args.num_eval_episodes:
        p.error("--record-episodes must be 1 .. --num-eval-episodes (%d)" % args.num_eval_episodes)
    if args.record and args.record_per_cell < 1:
        p.error("--record-per-cell must be >= 1")
    return args


def main():
    args = get_args()
    import numpy as np
    import torch
    import emergent_multiagent_strategies_amd as fa

    if args.guard_ckpts is None:            # gen_plot_data.py:48-50
        names = [re.match(r"ep(\d+)\.pt$", f) for f in os.listdir(args.guard_load_dir)]
        args.guard_ckpts = sorted(int(m.group(1)) for m in names if m)
    if not args.guard_ckpts:
        raise SystemExit("no guard checkpoints (ep*.pt) in %s" % args.guard_load_dir)
    guards = [os.path.join(args.guard_load_dir, "ep%d.pt" % c) for c in args.guard_ckpts]
    attackers = [os.path.join(args.attacker_load_dir, "ep%d.pt" % c) for c in args.attacker_ckpts]
    out_dir = args.out_dir or args.guard_load_dir
    os.makedirs(out_dir, exist_ok=True)
    E, N, K = args.num_processes, args.num_guards + args.num_attackers, len(attackers)
    eng = fa.BatchedFortAttack(E, args.num_guards, args.num_attackers, args.num_env_steps, base_seed=args.seed)
    cp = fa.CrossPlay(eng, guards, attackers, args.num_eval_episodes, deterministic=args.deterministic,
                      sample_seed=args.seed + 1, use_graph=not args.no_graph and args.num_env_steps >= 8,
                      behaviour=args.behaviour)
    per_episode = args.num_eval_episodes == 1
    if per_episode:     # each env's one episode return: reward x alive-before (obs[:, 0]), as test_fortattack_v2.py:90
        running = torch.zeros((E, N), dtype=torch.float64, device=eng.device)
        ret = torch.zeros_like(running)
        finished = torch.zeros(E, dtype=torch.bool, device=eng.device)

        def on_chunk(c):
            st = c.storage
            for s in range(c.T):
                running.add_(st.rewards[s, :, :, 0].double() * st.obs[s, :, :, 0].double())
                done = st.done[s] != 0
                first = done & ~finished
                ret[first] = running[first]
                finished.logical_or_(done)
                running[done] = 0.0
        cp.on_chunk = on_chunk
    if args.record:
        rec_envs = cp.record_envs(args.record_per_cell)
        cp.recorder = fa.EpisodeRecorder(eng, rec_envs, cp.T, size=args.record_size)
    cp.run()
    raw = cp.raw().cpu().numpy()
    table = cp.table()
    np.savez(os.path.join(out_dir, "crossplay.npz"), raw=raw, table=table, guard_ckpts=np.asarray(args.guard_ckpts),
             attacker_ckpts=np.asarray(args.attacker_ckpts))
    for k, ck in enumerate(args.guard_ckpts):
        np.savetxt(os.path.join(out_dir, "stats_ensemble_strategies_ep%d.csv" % ck), table[k].round(2), delimiter=",")
    if per_episode:
        cell = cp.cell.cpu().numpy()
        ret = ret.cpu().numpy()
        per_cell = min(int((cell == c).sum()) for c in range(cp.n_cells))   # the same number of episodes for every match-up
        data = np.zeros((len(guards), K * per_cell, 1 + N))
        for k, ck in enumerate(args.guard_ckpts):
            data[k, :, 0] = ck
            for i in range(K):
                data[k, i * per_cell:(i + 1) * per_cell, 1:] = ret[cell == k * K + i][:per_cell]
        np.save(os.path.join(out_dir, "reward_data_ensemble"), data)
    if args.record:
        cell = cp.cell.cpu().numpy()
        for e, episodes in zip(rec_envs, cp.recorder.episodes(args.record_episodes)):
            g, a = divmod(int(cell[e]), K)
            for i, frames in enumerate(episodes):
                path = os.path.join(out_dir, "video_g%d_a%d_env%d_ep%d.%s" % (args.guard_ckpts[g], args.attacker_ckpts[a], e, i,
                                                                              args.video_format))
                if args.video_format == "gif":
                    fa.record.write_gif(path, frames)
                else:
                    fa.record.write_npz(path, [frames])
    if args.behaviour:
        counts = cp.behaviour_counts()
        prints = cp.fingerprints()
        columns = list(fa.behaviour.FINGERPRINT_COLUMNS)
        np.savez(os.path.join(out_dir, "behaviour.npz"), fingerprints=prints, columns=np.asarray(columns),
                 guard_ckpts=np.asarray(args.guard_ckpts), attacker_ckpts=np.asarray(args.attacker_ckpts),
                 **{k: v.reshape((len(guards), K) + v.shape[1:]) for k, v in counts.items()})
        with open(os.path.join(out_dir, "fingerprints.csv"), "w") as f:
            f.write(",".join(["guard", "attacker"] + columns) + "\n")
            for g, gck in enumerate(args.guard_ckpts):
                for a, ack in enumerate(args.attacker_ckpts):
                    f.write(",".join(["%d" % gck, "%d" % ack] + ["%.6g" % v for v in prints[g, a]]) + "\n")
        for g, gck in enumerate(args.guard_ckpts):
            for a, ack in enumerate(args.attacker_ckpts):
                fa.behaviour.write_heatmaps(os.path.join(out_dir, "behaviour_g%d_a%d.png" % (gck, ack)),
                                            {k: v[g * K + a] for k, v in counts.items()})
    np.set_printoptions(suppress=True, precision=4)
    for k, ck in enumerate(args.guard_ckpts):
        print("guard checkpoint %d" % ck)
        print(table[k].round(2))
    eng.close()


if __name__ == "__main__":
    main()
