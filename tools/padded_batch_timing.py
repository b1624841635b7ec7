"""predict_batch() on naturally clustered scenes: the grouped path (one encode + denoise + top-k per distinct in-cluster count) against
padded=True (every episode in ONE jmid_predict_padded call, A = the largest count, padded agents masked as attention keys).
Run on the GPU box:

    padded_batch_timing.py [--reps R] [--warmup W] [--episodes E] [--precision P] [cfg2 | shipped]

The two paths alternate inside one process; per configuration a "RESULT" line with the medians (p10, p90) of both over the R rounds
after W warm-up rounds, the count histogram of the batch and its share of padded rows, and the distance between the two results."""
import os, sys, time
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from safe_interactive_crowdnav_amd.engine import JmidEngine
from safe_interactive_crowdnav_amd.forecaster import predict_batch
from safe_interactive_crowdnav_amd.weights import JMIDWeights, NetDims


def scenes(E, N, seed=17, F=6, dt=0.25):
    """tracks scattered over 10 m x 10 m, the robot at the lower edge: the reference's clustering keeps 1 .. N of them per episode"""
    rng = np.random.default_rng(seed)
    pos0 = rng.uniform(-5.0, 5.0, (E, N, 2))
    vel = rng.uniform(-1.0, 1.0, (E, N, 2))
    t = np.arange(F) * dt
    hum = pos0[:, None] + vel[:, None] * t[None, :, None, None] + 0.01 * rng.standard_normal((E, F, N, 2))
    rob = np.array([0.0, -3.0])[None, None] + 0.02 * rng.standard_normal((E, F, 2))
    return hum, rob


def run(tag, E, N, K, k_ret, H, step, precision, reps=20, warmup=3):
    eng = JmidEngine(JMIDWeights.from_seed(NetDims(ctx_dim=256), 0), joint=True, step=step)
    hum, rob = scenes(E, N)
    kw = dict(num_samples=K, num_ret_samples=k_ret, horizon=H, time_step=0.25, precision=precision)
    seeds = list(range(E))
    out, ts = {}, {False: [], True: []}
    for r in range(warmup + reps):
        for padded in (False, True):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out[padded] = predict_batch(eng, hum, rob, seeds, padded=padded, **kw)       # (host arrays out: the call has synchronised)
            if r >= warmup:
                ts[padded].append(1e3 * (time.perf_counter() - t0))
    n_in = out[False][2].sum(axis=1)
    hist = {int(a): int((n_in == a).sum()) for a in np.unique(n_in)}
    share = 1.0 - n_in.sum() / float(E * n_in.max())
    inc = out[False][2]
    dist = float(np.linalg.norm(out[True][0][inc] - out[False][0][inc], axis=-1).mean()) if k_ret == K else float("nan")
    g, p = np.array(ts[False]), np.array(ts[True])
    print(f"RESULT {tag} [{precision}] E={E} N={N} K={K}->{k_ret} H={H} steps={step} reps={reps} warmup={warmup}: counts {hist} "
          f"padded_rows {share:.3f}  grouped_ms {np.median(g):.3f} (p10 {np.percentile(g, 10):.3f} p90 {np.percentile(g, 90):.3f})  "
          f"padded_ms {np.median(p):.3f} (p10 {np.percentile(p, 10):.3f} p90 {np.percentile(p, 90):.3f})  "
          f"speedup {np.median(g) / np.median(p):.3f}  mean |padded - grouped| {dist:.3e} m", flush=True)
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
