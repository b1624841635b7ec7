"""What collision-free sampling costs per ``predict_ret_best()`` (docs/NOTEBOOK.md section 32), on ORCA circle-crossing scenes
(episodes.py), at the shipped point (N = 3, K = 100 -> 15, H = 8, 2 steps) and cfg2 (N = 5, K = 20 -> 20, H = 12, 50 steps), seeded
random-init weights at the shipped width.  Three forecasters in ONE process, called alternately on the same frames:
  (a) rng_compat="device" on the staged route (precision given, self check off) - the route the flag takes, without the flag
  (b) collision_free_rounds=3 at threshold 0: nothing collides - the cost of asking (one flags launch, the slot table, one small download)
  (c) collision_free_rounds=3 at threshold 0.2: the reference's threshold - collision rate, rounds, fixed / colliding, latency
(a) is held on the staged route (``plan_route`` alone would chain it into one entry) so that the three differ in the denoise stage only:
all three encode, denoise and, at k < K, rank on the device from the resident positions.
Every figure is the median over the measured calls after warm-up; the three variants see the same frames in the same order and are
interleaved call by call, so clock and thermal drift hit them alike.  Run on the GPU box:
    python tools/reject_timing.py [--precision f16mx] [--calls 40] [--episodes 4]
--rule RULE measures the wall predicate instead (section 33), --padded the one-loop form on mixed-count batches (section 34), --repair
collision repair against the redraw loop (section 35), --repair --rule RULE collision repair with walls on that rule's frames (section 37),
--guide guided sampling against no flag, the repair, both and the redraw loop (section 38; with --rule RULE on that rule's frames, walls in),
--chain the constraints inside the one-entry chains (constraint_route="chain") against the staged route (section 41; with --rule RULE on that
rule's frames, walls in)."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from safe_interactive_crowdnav_amd import episodes as EP
from safe_interactive_crowdnav_amd.forecaster import HumanTrajectoryForecasterSim, write_configs
from safe_interactive_crowdnav_amd.weights import JMIDWeights, NetDims

POINTS = {"shipped": (3, 100, 15, 8, 2), "cfg2": (5, 20, 20, 12, 50)}      # N, K, k, H, steps


class St:
    def __init__(self, p):
        self.position = (float(p[0]), float(p[1]))


class Staged(HumanTrajectoryForecasterSim):
    """Variant (a): today's seeded forecaster held on the staged route (``plan_route`` would chain it): encode, denoise, rank."""

    def _predict_ret_best(self):
        import safe_interactive_crowdnav_amd.forecaster as FC
        keep = FC.plan_route
        FC.plan_route = lambda **kw: keep(**kw)._replace(run="staged")
        try:
            return super()._predict_ret_best()
        finally:
            FC.plan_route = keep


def walls_main(args, weights):
    """--rule: what the wall predicate costs per ``engine.denoise_reject`` call (docs/NOTEBOOK.md section 33), one scene per call at the
    two points, the pedestrians standing inside the rule's walls.  Four variants in ONE process, interleaved call by call on the same
    inputs and draw numbers:
      (a) jmid_denoise_reject_seeded at threshold 0.2                      (b) jmid_denoise_reject_walls_seeded with L = 0
      (c) ... with the rule's walls moved 1 km away: nothing hits          (d) ... with the rule's walls in place
    (b) must lie inside the spread of the repeated (a) calls (``b_inside_a_spread``): anything else means L = 0 is not the old path."""
    import torch

    from safe_interactive_crowdnav_amd import crowd_env
    from safe_interactive_crowdnav_amd.engine import JmidEngine
    walls = crowd_env.static_obstacles(args.rule)[0].reshape(-1, 4)
    if not len(walls):
        raise SystemExit(f"rule {args.rule!r} has no walls")
    away = walls + np.array([1000.0, 0.0, 1000.0, 0.0])
    geo, R = crowd_env.Geometry(), 3
    half_x = 0.5 * geo.rect_width - args.radius - 0.05
    out = {"rule": args.rule, "radius": args.radius, "walls": int(len(walls))}
    for point, (N, K, k, H, step) in POINTS.items():
        eng = JmidEngine(weights, joint=True, hist_len=6, step=step)
        eng.set_step(step, "ddim")
        g = torch.Generator().manual_seed(11)
        ctx = torch.randn([1, N, 256], generator=g).numpy()
        # the pedestrians stand in the room below the door band (y in -1.6 .. -1.0), clear of every wall of the straight-walled rules:
        # what hits is the forecast, not the present position
        p0 = ((torch.rand([1, N, 2], generator=g) * 2.0 - 1.0) * torch.tensor([max(half_x, 0.05), 0.3]) - torch.tensor([0.0, 1.3])).numpy()
        common = dict(seed=7, episode_ids=[0], K=K, T=H, dt=0.25, precision=args.precision, threshold=0.2, max_rounds=R)
        variants = {"a_no_walls_entry": {}, "b_L0": dict(walls=np.zeros((0, 4)), wall_radius=args.radius),
                    "c_walls_away": dict(walls=away, wall_radius=args.radius), "d_walls": dict(walls=walls, wall_radius=args.radius)}
        ms = {name: [] for name in variants}
        hit, reruns = [], []
        for i in range(args.warmup + args.calls):
            order = list(variants.items())
            order = order[i % 4:] + order[:i % 4]                           # alternate who goes first
            for name, kw in order:
                t0 = time.perf_counter()
                res = eng.denoise_reject(ctx, p0, draw0=i * (R + 1), **common, **kw)
                dt = 1e3 * (time.perf_counter() - t0)
                if i >= args.warmup:
                    ms[name].append(dt)
                    if name == "d_walls":
                        hit.append(int(res[4][0, 1]))
                        reruns.append(int(res[3][0, 2]))
        res = {name: {"median_ms": round(float(np.median(v)), 3), "p10_ms": round(float(np.percentile(v, 10)), 3),
                      "p90_ms": round(float(np.percentile(v, 90)), 3)} for name, v in ms.items()}
        a = res["a_no_walls_entry"]
        res["calls"] = len(ms["a_no_walls_entry"])
        res["b_minus_a_ms"] = round(res["b_L0"]["median_ms"] - a["median_ms"], 3)
        res["b_inside_a_spread"] = bool(a["p10_ms"] <= res["b_L0"]["median_ms"] <= a["p90_ms"])
        res["c_minus_a_ms"] = round(res["c_walls_away"]["median_ms"] - a["median_ms"], 3)
        res["d"] = {"minus_a_ms": round(res["d_walls"]["median_ms"] - a["median_ms"], 3),
                    "share_of_samples_hitting": round(float(np.sum(hit)) / (len(hit) * K), 5), "reruns_mean": round(float(np.mean(reruns)), 3)}
        res["workload"] = f"N={N}, K={K}, H={H}, {step} steps, {args.precision}, {args.rule}, one scene per call"
        out[point] = res
        print(point, json.dumps(res), flush=True)
        eng.close()
    return out


def padded_main(args, weights):
    """--padded: ``predict_batch(collision_free_rounds=3)`` on the naturally clustered, mixed-count scenes of
    tools/padded_batch_timing.py (docs/NOTEBOOK.md section 34): the grouped form - one rejection loop per in-cluster count - against
    ``collision_free_padded=True`` - ONE loop for the batch at A = the largest count.  Both in ONE process on the same scenes, seeds and
    draw numbers, alternating call by call; next to the medians the count histogram, the share of padded rows, what the loops did
    (samples colliding, fixed, rounds) and the distance between the two forecasts (a padded call's attention sums in another order)."""
    import torch

    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from padded_batch_timing import scenes
    from safe_interactive_crowdnav_amd.engine import JmidEngine
    from safe_interactive_crowdnav_amd.forecaster import predict_batch
    out = {"threshold": args.threshold, "rounds": 3}
    E = args.episodes
    for point, (N, K, k, H, step) in POINTS.items():
        eng = JmidEngine(weights, joint=True, hist_len=6, step=step)
        hum, rob = scenes(E, N)
        kw = dict(num_samples=K, num_ret_samples=k, horizon=H, time_step=0.25, precision=args.precision, noise="device", seed=7,
                  collision_free_rounds=3, collision_threshold=args.threshold)
        paths = {"grouped": {}, "padded": dict(collision_free_padded=True)}
        ms, res, stats = {name: [] for name in paths}, {}, {name: {} for name in paths}
        for i in range(args.warmup + args.calls):
            order = list(paths.items())
            order = order[i % 2:] + order[:i % 2]                           # alternate who goes first
            for name, how in order:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                res[name] = predict_batch(eng, hum, rob, list(range(E)), stats=stats[name], **how, **kw)      # (host arrays out: the call has synchronised)
                if i >= args.warmup:
                    ms[name].append(1e3 * (time.perf_counter() - t0))
        inc = res["grouped"][2]
        n_in = inc.sum(axis=1)
        r = {name: {"median_ms": round(float(np.median(v)), 3), "p10_ms": round(float(np.percentile(v, 10)), 3),
                    "p90_ms": round(float(np.percentile(v, 90)), 3)} for name, v in ms.items()}
        r["calls"] = len(ms["grouped"])
        r["counts"] = {int(a): int((n_in == a).sum()) for a in np.unique(n_in)}
        r["padded_rows"] = round(1.0 - float(n_in.sum()) / float(E * n_in.max()), 4)
        r["speedup"] = round(r["grouped"]["median_ms"] / r["padded"]["median_ms"], 3)
        for name in paths:
            ep = stats[name]["episodes"]
            r[name].update(samples_colliding=int(ep[:, 0].sum()), samples_fixed=int(ep[:, 1].sum()), rounds=int(ep[:, 2].max()),
                           episodes_rerun=int((ep[:, 2] > 0).sum()))
        d = np.linalg.norm(res["padded"][0][inc] - res["grouped"][0][inc], axis=-1)
        r["forecast_distance_m"] = {"mean": float(d.mean()), "max": float(d.max())} if k == K else None      # (k < K: the kept sets may differ)
        r["workload"] = f"E={E}, N={N}, K={K} -> {k}, H={H}, {step} steps, {args.precision}, naturally clustered scenes, threshold {args.threshold}"
        out[point] = r
        print(point, json.dumps(r), flush=True)
        eng.close()
    return out


def repair_main(args, weights):
    """--repair: what collision repair costs per ``predict_ret_best()`` against the redraw loop (docs/NOTEBOOK.md section 35), on the frames
    of the default mode.  Three forecasters in ONE process on the same frames, seeds and draw numbers, alternating call by call:
      (a) the staged route without a flag          (b) collision_free_rounds=3          (c) constraint_type="opt_softplus" alone
    (b) and (c) at ``--threshold``.  Next to the medians and their p10 - p90: what (b) fixed of what collided, and the share of the samples
    that (c) repaired and reverted, with its largest iteration count.  No gate: (c) is read against (a) and (b) of the same run."""
    out = {"threshold": args.threshold}
    for point, (N, K, k, H, step) in POINTS.items():
        sim = EP.simulate_circle_crossing(args.episodes, N, 6 + args.warmup + args.calls, seed=11)
        with tempfile.TemporaryDirectory() as td:
            env, yp = write_configs(td, joint=True, ctx_dim=256, N=N, K=K, k_ret=k, H=H, step=step, time_step=0.25)
            common = dict(weights=weights, precision=args.precision, self_check=False, rng_compat="device", seed=7, collision_threshold=args.threshold)
            variants = {"a_staged": Staged(env, yp, **common),
                        "b_rounds_3": HumanTrajectoryForecasterSim(env, yp, collision_free_rounds=3, **common),
                        "c_opt_softplus": HumanTrajectoryForecasterSim(env, yp, constraint_type="opt_softplus", **common)}
        ms = {name: [] for name in variants}
        redraw, fix, most = np.zeros(2, dtype=np.int64), np.zeros(3, dtype=np.int64), 0
        for e in range(args.episodes):
            for f in variants.values():
                f.prev_states, f.prev_robot_states = [[] for _ in range(N)], []
            for i in range(6 + args.warmup + args.calls):
                for f in variants.values():
                    f.update_state_hists(St(sim["robot_xy"][e, i]), [St(p) for p in sim["human_xy"][e, i]], float(sim["stamps"][i]))
                if i < 5:
                    continue
                order = list(variants.items())
                order = order[i % 3:] + order[:i % 3]                       # alternate who goes first
                for name, f in order:
                    t0 = time.perf_counter()
                    f.predict_ret_best()
                    dt = 1e3 * (time.perf_counter() - t0)
                    if i < 5 + args.warmup:
                        continue
                    ms[name].append(dt)
                    if name.startswith("b"):
                        redraw += np.array(f.rejection[1:3])
                    if name.startswith("c"):
                        fix += np.array(f.repair[:3])
                        most = max(most, f.repair[3])
        n = len(ms["a_staged"])
        res = {name: {"median_ms": round(float(np.median(v)), 3), "p10_ms": round(float(np.percentile(v, 10)), 3),
                      "p90_ms": round(float(np.percentile(v, 90)), 3)} for name, v in ms.items()}
        res["calls"] = n
        res["b_minus_a_ms"] = round(res["b_rounds_3"]["median_ms"] - res["a_staged"]["median_ms"], 3)
        res["c_minus_a_ms"] = round(res["c_opt_softplus"]["median_ms"] - res["a_staged"]["median_ms"], 3)
        res["b"] = {"samples_colliding": int(redraw[0]), "samples_fixed": int(redraw[1]), "share_colliding": round(float(redraw[0]) / (n * K), 5)}
        res["c"] = {"samples_colliding": int(fix[0]), "share_repaired": round(float(fix[1]) / (n * K), 5),
                    "share_reverted": round(float(fix[2]) / (n * K), 5), "max_iterations": int(most)}
        res["erange_fallbacks"] = sum(f.erange_fallbacks for f in variants.values())
        res["workload"] = f"N={N}, K={K} -> {k}, H={H}, {step} steps, {args.precision}, ORCA circle crossing, {args.episodes} episodes, threshold {args.threshold}"
        out[point] = res
        print(point, json.dumps(res), flush=True)
    return out


def repair_walls_main(args, weights):
    """--repair --rule RULE: what collision repair WITH WALLS costs per ``predict_ret_best()`` (docs/NOTEBOOK.md section 37), on the frames
    of ``crowd_env.simulate_hallway`` under that rule, with the rule's walls at ``--radius``.  Four forecasters in ONE process on the same
    frames, seeds and draw numbers, alternating call by call:
      (a) the staged route without a flag                        (b) collision_free_rounds=3 with the walls
      (c) constraint_type="opt_softplus" (it knows no wall)      (d) constraint_type="opt_softplus_walls"
    Next to the medians and their p10 - p90: what (b) found and fixed by cause, what (c) repaired, and for (d) the shares repaired and
    reverted split by cause (``metrics.repair_causes``).  No gate: (d) is read against (a), (b) and (c) of the same run."""
    from safe_interactive_crowdnav_amd import crowd_env
    walls = crowd_env.static_obstacles(args.rule)[0]
    if not len(walls):
        raise SystemExit(f"rule {args.rule!r} has no walls")
    out = {"rule": args.rule, "radius": args.radius, "walls": int(len(walls)), "threshold": args.threshold}
    for point, (N, K, k, H, step) in POINTS.items():
        sim = crowd_env.simulate_hallway(args.episodes, N, 6 + args.warmup + args.calls, seed=11, cfg=crowd_env.HallwayConfig(rule=args.rule))
        with tempfile.TemporaryDirectory() as td:
            env, yp = write_configs(td, joint=True, ctx_dim=256, N=N, K=K, k_ret=k, H=H, step=step, time_step=0.25)
            common = dict(weights=weights, precision=args.precision, self_check=False, rng_compat="device", seed=7, collision_threshold=args.threshold)
            obstacles = dict(static_obstacles=walls, wall_radius=args.radius)
            variants = {"a_staged": Staged(env, yp, **common),
                        "b_rounds_3_walls": HumanTrajectoryForecasterSim(env, yp, collision_free_rounds=3, **obstacles, **common),
                        "c_opt_softplus": HumanTrajectoryForecasterSim(env, yp, constraint_type="opt_softplus", **common),
                        "d_opt_softplus_walls": HumanTrajectoryForecasterSim(env, yp, constraint_type="opt_softplus_walls", **obstacles, **common)}
        ms = {name: [] for name in variants}
        redraw, fix, causes, most = np.zeros(4, dtype=np.int64), np.zeros(3, dtype=np.int64), {}, 0
        for e in range(args.episodes):
            for f in variants.values():
                f.prev_states, f.prev_robot_states = [[] for _ in range(N)], []
            for i in range(6 + args.warmup + args.calls):
                for f in variants.values():
                    f.update_state_hists(St(sim["robot_xy"][e, i]), [St(p) for p in sim["human_xy"][e, i]], float(sim["stamps"][i]))
                if i < 5:
                    continue
                order = list(variants.items())
                order = order[i % 4:] + order[:i % 4]                       # alternate who goes first
                for name, f in order:
                    t0 = time.perf_counter()
                    f.predict_ret_best()
                    dt = 1e3 * (time.perf_counter() - t0)
                    if i < 5 + args.warmup:
                        continue
                    ms[name].append(dt)
                    if name.startswith("b"):
                        redraw += np.array(f.rejection[1:5])
                    if name.startswith("c"):
                        fix += np.array(f.repair[:3])
                    if name.startswith("d"):
                        causes = {key: causes.get(key, 0) + v for key, v in f.repair_causes.items()}
                        most = max(most, f.repair[3])
        n = len(ms["a_staged"])
        res = {name: {"median_ms": round(float(np.median(v)), 3), "p10_ms": round(float(np.percentile(v, 10)), 3),
                      "p90_ms": round(float(np.percentile(v, 90)), 3)} for name, v in ms.items()}
        res["calls"] = n
        for name in ("b_rounds_3_walls", "c_opt_softplus", "d_opt_softplus_walls"):
            res[name[0] + "_minus_a_ms"] = round(res[name]["median_ms"] - res["a_staged"]["median_ms"], 3)
        res["d_minus_c_ms"] = round(res["d_opt_softplus_walls"]["median_ms"] - res["c_opt_softplus"]["median_ms"], 3)
        share = lambda v: round(float(v) / (n * K), 5)
        res["b"] = {"samples_flagged": int(redraw[0]), "samples_fixed": int(redraw[1]), "round0_pedestrians": int(redraw[2]), "round0_walls": int(redraw[3]),
                    "share_flagged": share(redraw[0]), "share_left_flagged": share(redraw[0] - redraw[1])}
        res["c"] = {"samples_colliding": int(fix[0]), "share_repaired": share(fix[1]), "share_reverted": share(fix[2])}
        res["d"] = dict(causes, max_iterations=int(most), share_candidates=share(causes["candidates"]), share_repaired=share(causes["repaired"]),
                        share_reverted=share(causes["reverted"]), share_walls_repaired=share(causes["walls_repaired"]),
                        share_walls_reverted=share(causes["walls"] - causes["walls_repaired"]),
                        share_pedestrians_repaired=share(causes["pedestrians_repaired"]),
                        share_pedestrians_reverted=share(causes["pedestrians"] - causes["pedestrians_repaired"]))
        res["erange_fallbacks"] = sum(f.erange_fallbacks for f in variants.values())
        res["workload"] = (f"N={N}, K={K} -> {k}, H={H}, {step} steps, {args.precision}, {args.rule} frames, {args.episodes} episodes, threshold "
                           f"{args.threshold}, wall radius {args.radius}")
        out[point] = res
        print(point, json.dumps(res), flush=True)
    return out


def guide_main(args, weights):
    """--guide: what guided sampling (``guidance=``) costs per ``predict_ret_best()`` and what it does to the share of colliding samples
    (docs/NOTEBOOK.md section 38).  The forecasters of ONE process on the same frames, seeds and draw numbers, alternating call by call:
      (a) the staged route without a flag      (b) constraint_type="opt_softplus"      (c) guidance (the defaults: scale 0.02 m x alpha_bar,
      n_inner 4)      (d) guidance + opt_softplus      (e) collision_free_rounds=3      (f) guidance with the alternative table: the last
      half of the steps at scale, nothing before.
    With --rule RULE the frames are that rule's hallway frames and (b), (c), (d), (e), (f) take its walls at --radius ("opt_softplus_walls").
    After every timed call the collision (and wall) statistics entries judge the set the call left resident: ``share_colliding`` is the
    share of samples that still fail at --threshold (for either cause with walls); behind a repair stage it is the repair's reverted share.
    No gate: everything is read against (a) of the same run."""
    from safe_interactive_crowdnav_amd import scene as SC
    walls = None
    if args.rule:
        from safe_interactive_crowdnav_amd import crowd_env
        walls = crowd_env.static_obstacles(args.rule)[0]
        if not len(walls):
            raise SystemExit(f"rule {args.rule!r} has no walls")
    out = {"threshold": args.threshold, "rule": args.rule, "radius": args.radius if walls is not None else None}
    for point, (N, K, k, H, step) in POINTS.items():
        frames = 6 + args.warmup + args.calls
        if walls is None:
            sim = EP.simulate_circle_crossing(args.episodes, N, frames, seed=11)
        else:
            sim = crowd_env.simulate_hallway(args.episodes, N, frames, seed=11, cfg=crowd_env.HallwayConfig(rule=args.rule))
        obstacles = {} if walls is None else dict(static_obstacles=walls, wall_radius=args.radius)
        repair = "opt_softplus" if walls is None else "opt_softplus_walls"
        gopt = {} if walls is None else {"walls": True}
        with tempfile.TemporaryDirectory() as td:
            env, yp = write_configs(td, joint=True, ctx_dim=256, N=N, K=K, k_ret=k, H=H, step=step, time_step=0.25)
            common = dict(weights=weights, precision=args.precision, self_check=False, rng_compat="device", seed=7, collision_threshold=args.threshold)
            variants = {"a_staged": Staged(env, yp, **common),
                        "b_" + repair: HumanTrajectoryForecasterSim(env, yp, constraint_type=repair, **obstacles, **common),
                        "c_guidance": HumanTrajectoryForecasterSim(env, yp, guidance=dict(gopt), **obstacles, **common),
                        "d_guidance_" + repair: HumanTrajectoryForecasterSim(env, yp, guidance=dict(gopt), constraint_type=repair, **obstacles, **common),
                        "e_rounds_3": HumanTrajectoryForecasterSim(env, yp, collision_free_rounds=3, **obstacles, **common),
                        "f_guidance_last_half": HumanTrajectoryForecasterSim(env, yp, guidance=dict(gopt, table="last_half"), **obstacles, **common)}
        ms = {name: [] for name in variants}
        bad = {name: 0 for name in variants}
        fix = {name: np.zeros(3, dtype=np.int64) for name in variants}
        guided = {name: np.zeros(2, dtype=np.int64) for name in variants}
        samples = 0
        for e in range(args.episodes):
            for f in variants.values():
                f.prev_states, f.prev_robot_states = [[] for _ in range(N)], []
            for i in range(frames):
                for f in variants.values():
                    f.update_state_hists(St(sim["robot_xy"][e, i]), [St(p) for p in sim["human_xy"][e, i]], float(sim["stamps"][i]))
                if i < 5:
                    continue
                a = variants["a_staged"]
                sb = SC.build_scene(*SC.frame_table(*a._snapshot(), a.time_step, a.num_hist_frames)[:2], a.time_step, H, a.num_hist_frames)
                dims = (1, len(sb.ids_in), K, H)
                order = list(variants.items())
                order = order[i % len(order):] + order[:i % len(order)]     # alternate who goes first
                for name, f in order:
                    t0 = time.perf_counter()
                    f.predict_ret_best()
                    dt = 1e3 * (time.perf_counter() - t0)
                    if i < 5 + args.warmup:
                        continue
                    ms[name].append(dt)
                    if dims[1] >= 1:      # the set the call left resident, judged by the statistics entries (not timed)
                        flagged = f.engine.collision_statistics(None, args.threshold, dims=dims, agents=False)[2][0, :, 3] > 0
                        if walls is not None:
                            flagged = flagged | (f.engine.wall_statistics(None, walls, args.radius, p0=sb.p0[None], dims=dims)[2][0, :, 1] > 0)
                        bad[name] += int(flagged.sum())
                    if f.repair is not None:
                        fix[name] += np.array(f.repair[:3])
                    if f.guide is not None:
                        guided[name] += np.array([int((f.guide[:, 0] > 0).sum()), int(f.guide[:, 1].sum())])
                if i >= 5 + args.warmup:
                    samples += K
        res = {name: {"median_ms": round(float(np.median(v)), 3), "p10_ms": round(float(np.percentile(v, 10)), 3),
                      "p90_ms": round(float(np.percentile(v, 90)), 3), "share_colliding": round(bad[name] / samples, 5)} for name, v in ms.items()}
        base = res["a_staged"]["median_ms"]
        for name, f in variants.items():
            res[name]["minus_a_ms"] = round(res[name]["median_ms"] - base, 3)
            if f.constraints.repair is not None:
                # the repair's own rows say what still fails (its reverted samples): at k = K the ranking reads a host copy and the
                # resident set stays as the denoise call left it
                res[name].update(share_repaired=round(float(fix[name][1]) / samples, 5), share_reverted=round(float(fix[name][2]) / samples, 5),
                                 share_colliding_before_repair=round(float(fix[name][0]) / samples, 5), share_colliding=round(float(fix[name][2]) / samples, 5))
            if guided[name][0]:
                res[name].update(share_guided=round(float(guided[name][0]) / samples, 5), iterations_per_guided_sample=round(float(guided[name][1]) / float(guided[name][0]), 3))
        res["calls"], res["samples"] = len(ms["a_staged"]), samples
        res["erange_fallbacks"] = sum(f.erange_fallbacks for f in variants.values())
        res["workload"] = (f"N={N}, K={K} -> {k}, H={H}, {step} steps, {args.precision}, " + ("ORCA circle crossing" if walls is None else f"{args.rule} frames, wall radius {args.radius}") +
                           f", {args.episodes} episodes, threshold {args.threshold}")
        out[point] = res
        print(point, json.dumps(res), flush=True)
    return out


def chain_main(args, weights):
    """--chain: the constraints inside the one-entry chains against the staged route (docs/NOTEBOOK.md section 41).  The forecasters of ONE
    process on the same frames, seeds and draw numbers, alternating call by call:
      (a) no flag: the plain chain, and the same held on the staged route
      (b) constraint_type (the repair), (c) guidance, (d) both - each staged (the default route) and as constraint_route="chain"
    With --rule RULE the frames are that rule's hallway frames and every constraint takes its walls at --radius.  No gate fixed in advance:
    a chain is read against the staged forecaster of the same constraints of the same run.  (The logs of section 41 also hold
    "*_chain_separate_launches" rows: the chain's repair phase was measured once with a repair kernel that evaluates the candidate gate
    itself against the separate predicate launches, which are what the chain runs; that kernel variant did not pay and is not in the tree.)"""
    walls = None
    if args.rule:
        from safe_interactive_crowdnav_amd import crowd_env
        walls = crowd_env.static_obstacles(args.rule)[0]
        if not len(walls):
            raise SystemExit(f"rule {args.rule!r} has no walls")
    out = {"threshold": args.threshold, "rule": args.rule, "radius": args.radius if walls is not None else None}
    for point, (N, K, k, H, step) in POINTS.items():
        frames = 6 + args.warmup + args.calls
        if walls is None:
            sim = EP.simulate_circle_crossing(args.episodes, N, frames, seed=11)
        else:
            sim = crowd_env.simulate_hallway(args.episodes, N, frames, seed=11, cfg=crowd_env.HallwayConfig(rule=args.rule))
        obstacles = {} if walls is None else dict(static_obstacles=walls, wall_radius=args.radius)
        repair = "opt_softplus" if walls is None else "opt_softplus_walls"
        gopt = {} if walls is None else {"walls": True}
        kinds = {"repair": dict(constraint_type=repair), "guidance": dict(guidance=dict(gopt)),
                 "both": dict(guidance=dict(gopt), constraint_type=repair)}
        with tempfile.TemporaryDirectory() as td:
            env, yp = write_configs(td, joint=True, ctx_dim=256, N=N, K=K, k_ret=k, H=H, step=step, time_step=0.25)
            common = dict(weights=weights, precision=args.precision, self_check=False, rng_compat="device", seed=7, collision_threshold=args.threshold)
            variants = {"a_chain": HumanTrajectoryForecasterSim(env, yp, **common), "a_staged": Staged(env, yp, **common)}
            for kind, kw in kinds.items():
                variants[kind + "_staged"] = HumanTrajectoryForecasterSim(env, yp, **kw, **obstacles, **common)
                variants[kind + "_chain"] = HumanTrajectoryForecasterSim(env, yp, constraint_route="chain", **kw, **obstacles, **common)
        ms = {name: [] for name in variants}
        fix = {name: np.zeros(3, dtype=np.int64) for name in variants}
        guided = {name: 0 for name in variants}
        for e in range(args.episodes):
            for f in variants.values():
                f.prev_states, f.prev_robot_states = [[] for _ in range(N)], []
            for i in range(frames):
                for f in variants.values():
                    f.update_state_hists(St(sim["robot_xy"][e, i]), [St(p) for p in sim["human_xy"][e, i]], float(sim["stamps"][i]))
                if i < 5:
                    continue
                order = list(variants.items())
                order = order[i % len(order):] + order[:i % len(order)]     # alternate who goes first
                for name, f in order:
                    t0 = time.perf_counter()
                    f.predict_ret_best()
                    dt = 1e3 * (time.perf_counter() - t0)
                    if i < 5 + args.warmup:
                        continue
                    ms[name].append(dt)
                    if f.repair is not None:
                        fix[name] += np.array(f.repair[:3])
                    if f.guide is not None:
                        guided[name] += int((f.guide[:, 0] > 0).sum())
        n = len(ms["a_chain"])
        res = {name: {"median_ms": round(float(np.median(v)), 3), "p10_ms": round(float(np.percentile(v, 10)), 3),
                      "p90_ms": round(float(np.percentile(v, 90)), 3)} for name, v in ms.items()}
        for name in variants:
            if fix[name][0]:
                res[name].update(share_candidates=round(float(fix[name][0]) / (n * K), 5), share_repaired=round(float(fix[name][1]) / (n * K), 5))
            if guided[name]:
                res[name]["share_guided"] = round(float(guided[name]) / (n * K), 5)
        res["calls"] = n
        res["a_staged_minus_chain_ms"] = round(res["a_staged"]["median_ms"] - res["a_chain"]["median_ms"], 3)
        for kind in kinds:
            res[kind + "_staged_minus_chain_ms"] = round(res[kind + "_staged"]["median_ms"] - res[kind + "_chain"]["median_ms"], 3)
            res[kind + "_chain_minus_plain_chain_ms"] = round(res[kind + "_chain"]["median_ms"] - res["a_chain"]["median_ms"], 3)
        res["erange_fallbacks"] = sum(f.erange_fallbacks for f in variants.values())
        res["workload"] = (f"N={N}, K={K} -> {k}, H={H}, {step} steps, {args.precision}, " + ("ORCA circle crossing" if walls is None else f"{args.rule} frames, wall radius {args.radius}") +
                           f", {args.episodes} episodes, threshold {args.threshold}")
        out[point] = res
        print(point, json.dumps(res), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precision", default="f16mx")
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--episodes", type=int, default=4)
    ap.add_argument("--rule", default=None, help="a hallway rule of crowd_env (hallway_static, rectangle, ...): measure the wall predicate instead; with --repair: "
                    "collision repair with walls on that rule's frames")
    ap.add_argument("--radius", type=float, default=0.3, help="with --rule: the wall radius in metres")
    ap.add_argument("--padded", action="store_true", help="predict_batch on mixed-count scenes: one loop per count against collision_free_padded")
    ap.add_argument("--repair", action="store_true", help="collision repair (constraint_type='opt_softplus') against collision_free_rounds=3 and no flag")
    ap.add_argument("--guide", action="store_true", help="guided sampling (guidance=) against no flag, the repair, both and collision_free_rounds=3; with --rule: with its walls")
    ap.add_argument("--chain", action="store_true", help="guidance and repair inside the one-entry chains (constraint_route='chain') against the staged route; "
                    "with --rule: with its walls")
    ap.add_argument("--threshold", type=float, default=0.2, help="with --padded / --repair / --guide / --chain: the collision threshold in metres")
    args = ap.parse_args()
    weights = JMIDWeights.from_seed(NetDims(ctx_dim=256), 5)
    if args.rule or args.padded or args.repair or args.guide or args.chain:
        if args.padded and "--episodes" not in sys.argv:
            args.episodes = 8
        if args.chain:
            out = chain_main(args, weights)
        elif args.guide:
            out = guide_main(args, weights)
        elif args.repair and args.rule:
            out = repair_walls_main(args, weights)
        else:
            out = repair_main(args, weights) if args.repair else padded_main(args, weights) if args.padded else walls_main(args, weights)
        try:
            import bench
            out["sustained_mfma"] = bench.sustained_mfma_tflops()
        except Exception:
            out["sustained_mfma"] = None
        print(json.dumps(out))
        return
    out = {}
    for point, (N, K, k, H, step) in POINTS.items():
        sim = EP.simulate_circle_crossing(args.episodes, N, 6 + args.warmup + args.calls, seed=11)
        with tempfile.TemporaryDirectory() as td:
            env, yp = write_configs(td, joint=True, ctx_dim=256, N=N, K=K, k_ret=k, H=H, step=step, time_step=0.25)
            common = dict(weights=weights, precision=args.precision, self_check=False, rng_compat="device", seed=7)
            variants = {"a_staged": Staged(env, yp, **common),
                        "b_threshold_0": HumanTrajectoryForecasterSim(env, yp, collision_free_rounds=3, collision_threshold=0.0, **common),
                        "c_threshold_0.2": HumanTrajectoryForecasterSim(env, yp, collision_free_rounds=3, collision_threshold=0.2, **common)}
        ms = {name: [] for name in variants}
        totals = {name: np.zeros(3, dtype=np.int64) for name in variants}
        rounds, calls_with_collision = [], 0
        for e in range(args.episodes):
            for f in variants.values():
                f.prev_states, f.prev_robot_states = [[] for _ in range(N)], []
            for i in range(6 + args.warmup + args.calls):
                for f in variants.values():
                    f.update_state_hists(St(sim["robot_xy"][e, i]), [St(p) for p in sim["human_xy"][e, i]], float(sim["stamps"][i]))
                if i < 5:
                    continue
                order = list(variants.items())
                order = order[i % 3:] + order[:i % 3]                       # alternate who goes first
                for name, f in order:
                    t0 = time.perf_counter()
                    f.predict_ret_best()
                    dt = 1e3 * (time.perf_counter() - t0)
                    if i >= 5 + args.warmup:
                        ms[name].append(dt)
                        if f.rejection is not None:
                            totals[name] += np.array([0, f.rejection[1], f.rejection[2]])
                            if name.startswith("c"):
                                rounds.append(f.rejection[0])
                                calls_with_collision += f.rejection[1] > 0
        n = len(ms["a_staged"])
        res = {name: {"median_ms": round(float(np.median(v)), 3), "p10_ms": round(float(np.percentile(v, 10)), 3),
                      "p90_ms": round(float(np.percentile(v, 90)), 3)} for name, v in ms.items()}
        res["calls"] = n
        res["b_minus_a_ms"] = round(res["b_threshold_0"]["median_ms"] - res["a_staged"]["median_ms"], 3)
        res["c_minus_a_ms"] = round(res["c_threshold_0.2"]["median_ms"] - res["a_staged"]["median_ms"], 3)
        res["c"] = {"samples": n * K, "samples_colliding": int(totals["c_threshold_0.2"][1]), "samples_fixed": int(totals["c_threshold_0.2"][2]),
                    "collision_rate": round(float(totals["c_threshold_0.2"][1]) / (n * K), 5), "calls_with_a_collision": int(calls_with_collision),
                    "rounds_mean": round(float(np.mean(rounds)), 3), "rounds_max": int(np.max(rounds))}
        res["erange_fallbacks"] = sum(f.erange_fallbacks for f in variants.values())
        res["workload"] = f"N={N}, K={K} -> {k}, H={H}, {step} steps, {args.precision}, ORCA circle crossing, {args.episodes} episodes"
        out[point] = res
        print(point, json.dumps(res), flush=True)
    try:      # the matrix rate this box sustains at its power cap, next to the figures (tools/mfma_peak.hip, as bench.py reports it)
        import bench
        out["sustained_mfma"] = bench.sustained_mfma_tflops()
    except Exception:
        out["sustained_mfma"] = None
    print(json.dumps(out))


if __name__ == "__main__":
    main()
