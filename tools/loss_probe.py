"""One jmid_loss call of 256 scenes x A = 5 x T = 12 per arithmetic mode against jmid_net_eval on the same shape (E = 256, A = 5, K = 1,
T = 12): what the per-row fold, x_t and the reduction cost on top of the one net evaluation both are.  Run on the GPU box:

    loss_probe.py [--reps R] [--warmup W] [--episodes E]

Device memory (CUDA tensors in and out), the two calls alternating inside one process, wall time per call with a device synchronisation
(median, p10, p90 over R rounds after W warm-up rounds), then a second pass with the profiler classes "loss_prepare" and "loss_reduce"
enabled for the two kernels' own HIP-event durations.  One "RESULT" line per mode; "net_eval_spread" is the spread of the net_eval
timings themselves (p90 / p10), the floor under which a difference between the two calls says nothing.  Quote the numbers next to the
`sustained_peak` bench.py prints for the same box (the record is not box-normalised)."""
import os, sys, time
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from safe_interactive_crowdnav_amd.engine import JmidEngine
from safe_interactive_crowdnav_amd.weights import JMIDWeights, NetDims


def run(E, A, T, reps, warmup):
    eng = JmidEngine(JMIDWeights.from_seed(NetDims(ctx_dim=256), 0), joint=True, step=50)
    g = torch.Generator().manual_seed(3)
    x0 = torch.randn([E, A, T, 2], generator=g).cuda()
    e = torch.randn([E, A, T, 2], generator=g).cuda()
    ctx = torch.randn([E, A, 256], generator=g).cuda()
    t = np.random.default_rng(3).integers(1, 101, size=(E, A)).astype(np.int32)
    for precision in ("f32", "f16x3", "f16x2", "f16mx"):
        ts = {"loss": [], "net_eval": []}
        for r in range(warmup + reps):
            for name in ("net_eval", "loss"):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                if name == "loss":
                    out = eng.loss(x0, ctx, t, e=e, precision=precision)
                else:
                    eng.net_eval(x0, ctx, step_idx=0, precision=precision)
                torch.cuda.synchronize()
                if r >= warmup:
                    ts[name].append(1e3 * (time.perf_counter() - t0))
        eng.profile_reset()
        eng.profile_enable(["loss_prepare", "loss_reduce"])
        for _ in range(reps):
            eng.loss(x0, ctx, t, e=e, precision=precision)
        prof = eng.profile_get()
        eng.profile_disable()
        lo, ne = np.array(ts["loss"]), np.array(ts["net_eval"])
        print(f"RESULT loss_probe [{precision}] E={E} A={A} T={T} reps={reps} warmup={warmup}: loss {float(out.loss):.6f}  "
              f"loss_ms {np.median(lo):.3f} (p10 {np.percentile(lo, 10):.3f} p90 {np.percentile(lo, 90):.3f})  "
              f"net_eval_ms {np.median(ne):.3f} (p10 {np.percentile(ne, 10):.3f} p90 {np.percentile(ne, 90):.3f})  "
              f"ratio {np.median(lo) / np.median(ne):.3f}  net_eval_spread {np.percentile(ne, 90) / np.percentile(ne, 10):.3f}  "
              f"prepare_us {1e3 * prof['loss_prepare'][1] / max(1, prof['loss_prepare'][0]):.1f}  "
              f"reduce_us {1e3 * prof['loss_reduce'][1] / max(1, prof['loss_reduce'][0]):.1f}", flush=True)
    eng.close()


if __name__ == "__main__":
    opts = dict(reps=30, warmup=5, episodes=256)
    for name in list(opts):
        if "--" + name in sys.argv:
            i = sys.argv.index("--" + name)
            opts[name] = int(sys.argv[i + 1])
            del sys.argv[i:i + 2]
    run(opts["episodes"], 5, 12, opts["reps"], opts["warmup"])
