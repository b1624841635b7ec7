"""DDPM sampling of a batch of episodes, end to end: host-drawn noise through the explicit entry against the seeded entry.

    seeded_ddpm_latency.py [--episodes E] [--reps R] [--precision P] [--only explicit|seeded]

cfg2 shape (A = 5, K = 20, T = 12, encoder_dim 256), DDPM, 100 steps.  "explicit" is today's path: x_T [E, K*A, T, 2] and z
[100, E, K*A, T, 2] drawn with torch's CPU generator, uploaded by jmid_denoise_ddpm, then the loop; "seeded" is jmid_denoise_seeded
(nothing drawn or uploaded).  Each variant runs on an engine of its own after one warm-up call; printed are the R end-to-end times,
their minimum, the host-draw share, and the device memory the process holds after the calls (hipMemGetInfo: the library's workspace
never shrinks, so that is its peak).  Run on the GPU box."""
import argparse, json, os, sys, time
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from safe_interactive_crowdnav_amd.engine import JmidEngine
from safe_interactive_crowdnav_amd.weights import JMIDWeights, NetDims

A, K, T, STEPS = 5, 20, 12, 100


def used_mib():
    free, total = torch.cuda.mem_get_info(0)
    return (total - free) / 2 ** 20


def run(variant, E, reps, precision):
    base = used_mib()
    eng = JmidEngine(JMIDWeights.from_seed(NetDims(ctx_dim=256), 0), joint=True, step=STEPS)
    eng.set_step(STEPS, "ddpm")
    g = torch.Generator().manual_seed(1)
    ctx = torch.randn([E, A, 256], generator=g).numpy()
    p0 = torch.randn([E, A, 2], generator=g).numpy()
    ids = np.arange(E)
    times, draws = [], []
    for r in range(reps + 1):                       # the first call is the warm-up (workspace allocation, kernel loading)
        t0 = time.perf_counter()
        if variant == "explicit":
            x_T = torch.randn([E, K * A, T, 2], generator=g)
            z = torch.randn([STEPS, E, K * A, T, 2], generator=g)
            t1 = time.perf_counter()
            _, pos = eng.denoise(x_T.numpy(), ctx, p0, precision=precision, want_vel=False, z=z.numpy())
        else:
            t1 = t0
            _, pos = eng.denoise(None, ctx, p0, precision=precision, want_vel=False, seed=1, episode_ids=ids, K=K, T=T)
        t2 = time.perf_counter()
        assert np.isfinite(pos).all()
        if r:
            times.append(1e3 * (t2 - t0))
            draws.append(1e3 * (t1 - t0))
    out = {"variant": variant, "E": E, "A": A, "K": K, "T": T, "steps": STEPS, "precision": precision, "reps": reps,
           "total_ms": [round(t, 2) for t in times], "min_ms": round(min(times), 2), "max_ms": round(max(times), 2),
           "host_draw_ms_min": round(min(draws), 2), "device_mib_after": round(used_mib() - base, 1),
           "noise_floats": (STEPS + 1) * E * K * A * T * 2}
    eng.close()
    print("RESULT " + json.dumps(out), flush=True)
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--episodes", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--precision", default="f16mx")
    ap.add_argument("--only", choices=["explicit", "seeded"])
    a = ap.parse_args()
    for v in ([a.only] if a.only else ["explicit", "seeded"]):
        run(v, a.episodes, a.reps, a.precision)
