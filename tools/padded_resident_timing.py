"""predict_batch() on naturally clustered scenes with the scene batch and the noise on the device: the grouped path
(device_frames=True, noise="device": one build + one jmid_forecast_scene_seeded per distinct in-cluster count) against
padded="resident" (ONE build, ONE jmid_forecast_scene_padded_seeded for the whole batch, A = the largest count).
Run on the GPU box:

    padded_resident_timing.py [--reps R] [--warmup W] [--episodes E] [--precision P] [cfg2 | shipped]

The two paths alternate inside one process; per configuration a "RESULT" line with the medians (p10, p90) of both over the R rounds
after W warm-up rounds, the count histogram of the batch and its share of padded rows, and the distance between the two results."""
import os, sys, time
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from safe_interactive_crowdnav_amd.engine import JmidEngine
from safe_interactive_crowdnav_amd.forecaster import predict_batch
from safe_interactive_crowdnav_amd.weights import JMIDWeights, NetDims
from padded_batch_timing import scenes


def run(tag, E, N, K, k_ret, H, step, precision, reps=20, warmup=3):
    eng = JmidEngine(JMIDWeights.from_seed(NetDims(ctx_dim=256), 0), joint=True, step=step)
    hum, rob = scenes(E, N)
    kw = dict(num_samples=K, num_ret_samples=k_ret, horizon=H, time_step=0.25, precision=precision, noise="device", seed=7)
    seeds = list(range(E))
    paths = {"grouped": dict(device_frames=True), "resident": dict(padded="resident")}
    out, ts = {}, {name: [] for name in paths}
    for r in range(warmup + reps):
        for name, how in paths.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out[name] = predict_batch(eng, hum, rob, seeds, **how, **kw)       # (host arrays out: the call has synchronised)
            if r >= warmup:
                ts[name].append(1e3 * (time.perf_counter() - t0))
    inc = out["grouped"][2]
    n_in = inc.sum(axis=1)
    hist = {int(a): int((n_in == a).sum()) for a in np.unique(n_in)}
    share = 1.0 - n_in.sum() / float(E * n_in.max())
    dist = float(np.linalg.norm(out["resident"][0][inc] - out["grouped"][0][inc], axis=-1).mean()) if k_ret == K else float("nan")
    g, p = np.array(ts["grouped"]), np.array(ts["resident"])
    print(f"RESULT {tag} [{precision}] E={E} N={N} K={K}->{k_ret} H={H} steps={step} reps={reps} warmup={warmup}: counts {hist} "
          f"padded_rows {share:.3f}  grouped_ms {np.median(g):.3f} (p10 {np.percentile(g, 10):.3f} p90 {np.percentile(g, 90):.3f})  "
          f"resident_ms {np.median(p):.3f} (p10 {np.percentile(p, 10):.3f} p90 {np.percentile(p, 90):.3f})  "
          f"speedup {np.median(g) / np.median(p):.3f}  mean |resident - grouped| {dist:.3e} m", flush=True)
    eng.close()


if __name__ == "__main__":
    opts = {}
    for name, key in (("--reps", "reps"), ("--warmup", "warmup")):
        if name in sys.argv:
            i = sys.argv.index(name)
            opts[key] = int(sys.argv[i + 1])
            del sys.argv[i:i + 2]
    E, precision = 8, "f16mx"
    if "--episodes" in sys.argv:
        i = sys.argv.index("--episodes"); E = int(sys.argv[i + 1]); del sys.argv[i:i + 2]
    if "--precision" in sys.argv:
        i = sys.argv.index("--precision"); precision = sys.argv[i + 1]; del sys.argv[i:i + 2]
    which = sys.argv[1] if len(sys.argv) > 1 else ""
    if which in ("", "cfg2"):
        run("cfg2", E, 5, 20, 20, 12, 50, precision, **opts)
    if which in ("", "shipped"):
        run("shipped", E, 3, 100, 15, 8, 2, precision, **opts)
