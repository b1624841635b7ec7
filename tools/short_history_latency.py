"""Latency of HumanTrajectoryForecasterSim(short_history=True).predict_ret_best() with L = 2 .. 5 shared history frames against the full
window (L = 6), in ONE process on one engine: what an MPC step pays during the first control steps of an episode.  Run on the GPU box.

    short_history_latency.py [--device-scene | --routes] [--reps R] [--warmup W] [cfg2 | shipped]

Per L a fresh forecaster is fed L frames (the engine is shared: forecaster.py caches it), called W times unmeasured and R times measured;
printed are the median and the 10th / 90th percentile of the wall time of a call and the medians of its parts.  L < 6 on the host scene
takes the staged path (encode(first_index) -> denoise -> topk: three library entries), L = 6 and --device-scene the one-entry chain.
--routes: per L, three forecasters side by side, their measured calls ALTERNATING (drift and the neighbours on the box hit them alike):
  host    short_history=True                                        the host frame table and scene, staged below L = 6
  frames  short_history=True, device_frames=True                    the host frame table, then engine.build_scene(first_frame=) + chain
  tracks  short_history=True, device_frames=True, track_presence=True   raw frames in: jmid_build_scene_stamped_var + ONE chain
and behind the L rows one more case, "absent": a full window in which the last of the N pedestrians is not seen on the two newest frames,
three forecasters with device_frames=True and track_presence=True, alternating as above:
  filter    coast_frames=0   today's route: his column is cut out on the host, jmid_build_scene_stamped_var on N - 1 tracks
  left_out  coast_frames=1   all N tracks to jmid_build_scene_stamped_coast; last seen 2 bins ago, he is left out on the device
  coasted   coast_frames=2   the same entry; he is coasted over 2 bins and forecast like everybody else"""
import os, sys, tempfile, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from safe_interactive_crowdnav_amd import forecaster as F
from safe_interactive_crowdnav_amd.weights import JMIDWeights, NetDims


class State:
    def __init__(self, p):
        self.position = (float(p[0]), float(p[1]))


PREC = os.environ.get("JMID_PREC", "f16mx")


def run(tag, N, K, k_ret, H, step, reps=30, warmup=3, device_scene=False):
    d = tempfile.mkdtemp()
    env, ypath = F.write_configs(d, joint=True, ctx_dim=256, N=N, K=K, k_ret=k_ret, H=H, step=step)
    w = JMIDWeights.from_seed(NetDims(ctx_dim=256), 0)
    rng = np.random.default_rng(0)
    p = rng.uniform(-1.0, 1.0, (N, 2)); v = rng.uniform(-0.5, 0.5, (N, 2))
    for L in (6, 5, 4, 3, 2, 6):          # the full window first and last: drift over the run shows as their difference
        f = F.HumanTrajectoryForecasterSim(env, ypath, weights=w, precision=PREC, short_history=True, device_scene=device_scene)
        for i in range(L):
            f.update_state_hists(State((0.0, -2.0 + 0.2 * i)), [State(p[j] + v[j] * 0.25 * i) for j in range(N)], 0.25 * i)
        for _ in range(max(warmup, 1)):
            f.predict_ret_best()
        ts, parts = [], []
        for _ in range(reps):
            t0 = time.perf_counter(); f.predict_ret_best(); ts.append(time.perf_counter() - t0)
            parts.append(dict(f.timings))
        ts = np.array(ts) * 1e3
        med = {k: float(np.median([q[k] for q in parts])) for k in ("scene_ms", "device_ms", "topk_ms", "assemble_ms")}
        print(f"RESULT {tag} device_scene={int(device_scene)} [{PREC}] L={L} reps={reps} warmup={warmup}: total_ms median {np.median(ts):.4f} "
              f"p10 {np.percentile(ts, 10):.4f} p90 {np.percentile(ts, 90):.4f}  " + "  ".join(f"{k} {x:.4f}" for k, x in med.items()), flush=True)


ROUTES = {"host": dict(), "frames": dict(device_frames=True), "tracks": dict(device_frames=True, track_presence=True)}


def run_routes(tag, N, K, k_ret, H, step, reps=30, warmup=3):
    d = tempfile.mkdtemp()
    env, ypath = F.write_configs(d, joint=True, ctx_dim=256, N=N, K=K, k_ret=k_ret, H=H, step=step)
    w = JMIDWeights.from_seed(NetDims(ctx_dim=256), 0)
    rng = np.random.default_rng(0)
    p = rng.uniform(-1.0, 1.0, (N, 2)); v = rng.uniform(-0.5, 0.5, (N, 2))
    for L in (6, 5, 4, 3, 2, 6):
        fs = {name: F.HumanTrajectoryForecasterSim(env, ypath, weights=w, precision=PREC, short_history=True, **kw) for name, kw in ROUTES.items()}
        for f in fs.values():
            for i in range(L):
                f.update_state_hists(State((0.0, -2.0 + 0.2 * i)), [State(p[j] + v[j] * 0.25 * i) for j in range(N)], 0.25 * i)
            for _ in range(max(warmup, 1)):
                f.predict_ret_best()
        ts = {name: [] for name in fs}
        for _ in range(reps):
            for name, f in fs.items():
                t0 = time.perf_counter(); f.predict_ret_best(); ts[name].append(time.perf_counter() - t0)
        for name in fs:
            t = np.array(ts[name]) * 1e3
            print(f"RESULT {tag} route={name} [{PREC}] L={L} reps={reps} warmup={warmup}: total_ms median {np.median(t):.4f} "
                  f"p10 {np.percentile(t, 10):.4f} p90 {np.percentile(t, 90):.4f}", flush=True)
    # one of N pedestrians not seen now
    fs = {name: F.HumanTrajectoryForecasterSim(env, ypath, weights=w, precision=PREC, short_history=True, device_frames=True, track_presence=True,
                                               coast_frames=c) for name, c in ABSENT.items()}
    for f in fs.values():
        for i in range(6):
            hum = [State(p[j] + v[j] * 0.25 * i) for j in range(N)]
            if i >= 4:
                hum[N - 1] = State((np.nan, np.nan))
            f.update_state_hists(State((0.0, -2.0 + 0.2 * i)), hum, 0.25 * i)
        for _ in range(max(warmup, 1)):
            f.predict_ret_best()
    ts = {name: [] for name in fs}
    for _ in range(reps):
        for name, f in fs.items():
            t0 = time.perf_counter(); f.predict_ret_best(); ts[name].append(time.perf_counter() - t0)
    for name in fs:
        t = np.array(ts[name]) * 1e3
        print(f"RESULT {tag} absent={name} [{PREC}] L=6 reps={reps} warmup={warmup}: total_ms median {np.median(t):.4f} "
              f"p10 {np.percentile(t, 10):.4f} p90 {np.percentile(t, 90):.4f}", flush=True)


ABSENT = {"filter": 0, "left_out": 1, "coasted": 2}


if __name__ == "__main__":
    opts = {}
    if "--routes" in sys.argv:
        sys.argv.remove("--routes")
        run = run_routes
    if "--device-scene" in sys.argv:
        sys.argv.remove("--device-scene")
        opts["device_scene"] = True
    for name in ("--reps", "--warmup"):
        if name in sys.argv:
            i = sys.argv.index(name)
            opts[name[2:]] = int(sys.argv[i + 1])
            del sys.argv[i:i + 2]
    which = sys.argv[1] if len(sys.argv) > 1 else ""
    if which in ("", "cfg2"):
        run("cfg2", 5, 20, 20, 12, 50, **opts)
    if which in ("", "shipped"):
        run("shipped", 3, 100, 15, 8, 2, **opts)
