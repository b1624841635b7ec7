"""Duration of jmid_eval_statistics (HIP events on the handle's stream: profile class "eval_statistics") for the cfg3 batch, the
shipped shape and the kernel's limits, next to the jmid_denoise call of the same batch (wall clock around the synchronised call) and
to the host: metrics.eval_statistics_host and, where scipy is installed, the reference's two scipy routines restated as the loop
they are (a gaussian_kde per agent and step, evaluated at the ground truth and at its own points) for 16 episodes.
Figures of docs/NOTEBOOK.md section 14.  Run on the GPU box."""
import os, sys, time
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from safe_interactive_crowdnav_amd import metrics as M
from safe_interactive_crowdnav_amd.engine import JmidEngine
from safe_interactive_crowdnav_amd.weights import JMIDWeights, NetDims


def scenes(E, A, K, T, seed):
    g = torch.Generator().manual_seed(seed)
    walk = torch.cumsum(0.1 * torch.randn([E, K + 1, A, T, 2], generator=g), dim=3) + 3.0 * torch.randn([E, 1, A, 1, 2], generator=g)
    return walk[:, :K].contiguous(), walk[:, K].contiguous()


def stats_ms(eng, pos, gt, dims=None, reps=5):
    eng.eval_statistics(pos, gt, dims=dims)                  # warm: workspace, code object
    eng.profile_enable(["eval_statistics"])
    eng.profile_reset()
    wall = []
    for _ in range(reps):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        eng.eval_statistics(pos, gt, dims=dims)
        torch.cuda.synchronize(); wall.append((time.perf_counter() - t0) * 1e3)
    n, ms = eng.profile_get()["eval_statistics"]
    eng.profile_disable()
    return ms / n, float(np.median(wall))


def scipy_loop(pos, gt):
    from scipy.stats import gaussian_kde
    E, K, A, T, _ = pos.shape
    for e in range(E):
        for a in range(A):
            for t in range(T):
                p = pos[e, :, a, t].T
                np.clip(gaussian_kde(p).logpdf(gt[e, a, t]), -20, None)
                np.clip(gaussian_kde(p).logpdf(p), -20, None)


def main():
    eng = JmidEngine(JMIDWeights.from_seed(NetDims(ctx_dim=256), 0), joint=True, step=50)
    # cfg3: 256 episodes of 5 agents, 20 samples, 12 steps; the statistics of the positions the denoise call left on the device
    E, A, K, T = 256, 5, 20, 12
    g = torch.Generator().manual_seed(1)
    x_T = torch.randn([E, K * A, T, 2], generator=g).cuda()
    ctx = eng.encode(torch.randn([E * A, 6, 6], generator=g).cuda(), torch.randn([E * A, 2, 6, 6], generator=g).cuda(),
                     torch.rand([E * A, 2], generator=g).cuda()).view(E, A, 256)
    p0 = torch.randn([E, A, 2], generator=g).cuda()
    den = []
    for i in range(3):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        _, pos = eng.denoise(x_T, ctx, p0, dt=0.25, precision="f16mx", want_vel=False)
        torch.cuda.synchronize(); den.append((time.perf_counter() - t0) * 1e3)
    gt = pos[:, 0] + 0.05 * torch.randn([E, A, T, 2], generator=g).cuda()
    ev, wall = stats_ms(eng, pos, gt)
    ev0, wall0 = stats_ms(eng, None, gt, dims=(E, A, K, T))
    print(f"cfg3 E=256 A=5 K=20 T=12: jmid_denoise (f16mx, 50 steps) {min(den):.2f} ms | jmid_eval_statistics {ev * 1e3:.1f} us events, "
          f"{wall * 1e3:.1f} us wall (pos=NULL: {ev0 * 1e3:.1f} / {wall0 * 1e3:.1f} us) | ratio {min(den) / ev:.0f}", flush=True)
    assert ev < min(den), "the statistics must take less time than the denoise call they follow"
    a, s = eng.eval_statistics(pos, gt)
    torch.cuda.synchronize()
    print("  summary:", {k: round(v, 4) for k, v in M.summarise(a.cpu().numpy(), s.cpu().numpy()).items()}, flush=True)
    for tag, (E, A, K, T) in (("shipped E=256 A=3 K=100 T=8", (256, 3, 100, 8)), ("limits E=1 A=32 K=1024 T=24", (1, 32, 1024, 24)),
                              ("limits E=8 A=32 K=1024 T=24", (8, 32, 1024, 24))):
        pos, gt = scenes(E, A, K, T, 2)
        ev, wall = stats_ms(eng, pos.cuda(), gt.cuda(), reps=3)
        print(f"{tag}: jmid_eval_statistics {ev * 1e3:.1f} us events, {wall * 1e3:.1f} us wall", flush=True)
    # the host, 16 episodes of the cfg3 shape
    pos, gt = scenes(16, 5, 20, 12, 3)
    pos, gt = pos.numpy(), gt.numpy()
    t0 = time.perf_counter(); M.eval_statistics_host(pos, gt); t_host = time.perf_counter() - t0
    print(f"host, 16 episodes A=5 K=20 T=12: eval_statistics_host {t_host * 1e3:.1f} ms ({t_host / 80 * 1e3:.2f} ms per agent)", flush=True)
    try:
        t0 = time.perf_counter(); scipy_loop(pos.astype(np.float64), gt.astype(np.float64)); t_sp = time.perf_counter() - t0
        print(f"host, 16 episodes A=5 K=20 T=12: scipy gaussian_kde loop {t_sp * 1e3:.1f} ms ({t_sp / 80 * 1e3:.2f} ms per agent)", flush=True)
    except ImportError:
        print("scipy is not installed: no scipy loop", flush=True)
    assert eng.erange_count() == 0 and eng.timeout_count() == 0
    eng.close()


if __name__ == "__main__":
    main()
