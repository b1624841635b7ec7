"""End-to-end latency of HumanTrajectoryForecasterSim.predict_ret_best() (what one MPC step pays), split into
host preprocessing / encoder / denoise loop / selection + assembly.  Run on the GPU box.

    forecaster_latency.py [--device-scene | --device-frames] [--reps R] [--warmup W] [cfg2 | shipped [R]]

--device-scene builds the scene batch on the device (HumanTrajectoryForecasterSim(device_scene=True)), --device-frames the frame table
too and assembles the result there (device_frames=True); with a configuration name only that one runs and a "RESULT" line with the
medians of scene_ms, device_ms, assemble_ms and total_ms over the R calls after W warm-ups is printed."""
import os, sys, tempfile, time
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from safe_interactive_crowdnav_amd import forecaster as F
from safe_interactive_crowdnav_amd.weights import JMIDWeights, NetDims


class State:
    def __init__(self, p):
        self.position = (float(p[0]), float(p[1]))


PREC = os.environ.get("JMID_PREC", "f16x3")
DEVICE_SCENE = False
DEVICE_FRAMES = False


def run(tag, N, K, k_ret, H, step, reps=20, warmup=1):
    d = tempfile.mkdtemp()
    env, ypath = F.write_configs(d, joint=True, ctx_dim=256, N=N, K=K, k_ret=k_ret, H=H, step=step)
    kw = {"device_scene": True} if DEVICE_SCENE else {}
    if DEVICE_FRAMES:
        kw["device_frames"] = True
    f = F.HumanTrajectoryForecasterSim(env, ypath, weights=JMIDWeights.from_seed(NetDims(ctx_dim=256), 0), precision=PREC, **kw)
    rng = np.random.default_rng(0)
    p = rng.uniform(-1.5, 1.5, (N, 2)); v = rng.uniform(-0.5, 0.5, (N, 2))
    for i in range(8):
        f.update_state_hists(State((0.0, -2.0 + 0.2 * i)), [State(p[j] + v[j] * 0.25 * i) for j in range(N)], 0.25 * i)
    for _ in range(max(warmup, 1)):
        f.predict_ret_best()
    ts, parts = [], []
    for _ in range(reps):
        t0 = time.perf_counter(); f.predict_ret_best(); ts.append(time.perf_counter() - t0)
        parts.append(dict(f.timings))
    ts = np.array(ts) * 1e3
    med = {k: float(np.median([p[k] for p in parts])) for k in ("scene_ms", "device_ms", "assemble_ms", "total_ms")}
    print(f"RESULT {tag.split()[0]} device_scene={int(DEVICE_SCENE)} device_frames={int(DEVICE_FRAMES)} [{PREC}] reps={reps} warmup={warmup}: "
          + "  ".join(f"{k} {v:.4f}" for k, v in med.items()) + f"  total_ms p10 {np.percentile(ts, 10):.4f} p90 {np.percentile(ts, 90):.4f}", flush=True)
    print(f"{tag} [{PREC}]: predict_ret_best() median {np.median(ts):.3f} ms  min {ts.min():.3f}  max {ts.max():.3f}   last call: "
          + ", ".join(f"{k} {v:.3f}" for k, v in f.timings.items()), flush=True)
    return f


if __name__ == "__main__":
    if "--device-scene" in sys.argv:
        sys.argv.remove("--device-scene")
        DEVICE_SCENE = True
    if "--device-frames" in sys.argv:
        sys.argv.remove("--device-frames")
        DEVICE_FRAMES = True
    opts = {}
    for name in ("--reps", "--warmup"):
        if name in sys.argv:
            i = sys.argv.index(name)
            opts[name[2:]] = int(sys.argv[i + 1])
            del sys.argv[i:i + 2]
    if len(sys.argv) > 1 and sys.argv[1] == "cfg2":
        run("cfg2  N=5 K=20 H=12 50 steps", 5, 20, 20, 12, 50, **opts)
        raise SystemExit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "shipped" and opts:
        run("shipped N=3 K=100->15 H=8 2 steps", 3, 100, 15, 8, 2, **opts)
        raise SystemExit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "shipped":       # the shipped operating point only (under rocprofv3: tools/shipped_profile.sh)
        run("shipped N=3 K=100->15 H=8 2 steps", 3, 100, 15, 8, 2, reps=int(sys.argv[2]) if len(sys.argv) > 2 else 50)
        raise SystemExit(0)
    f = run("cfg2  N=5 K=20 H=12 50 steps", 5, 20, 20, 12, 50)
    run("shipped N=3 K=100->15 H=8 2 steps", 3, 100, 15, 8, 2)
    run("N=5 K=20 H=12 2 steps", 5, 20, 20, 12, 2)
    import cProfile, pstats
    pr = cProfile.Profile(); pr.enable()
    for _ in range(10):
        f.predict_ret_best()
    pr.disable()
    pstats.Stats(pr).sort_stats("cumulative").print_stats(18)
