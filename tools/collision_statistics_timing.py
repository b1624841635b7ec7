"""Duration of jmid_collision_statistics next to jmid_eval_statistics on the same positions in the same run (HIP events on the
handle's stream: both run under the profile class "eval_statistics"), device memory, warmed, the median of 25 calls: the cfg3 batch
(E = 256, A = 5, K = 20, T = 12) and the dense shape (A = 25, K = 64, T = 12; E = 256 and E = 1), and the kernel's limits.  Next to it
the host twin for 16 episodes of the cfg3 shape.  Figures of docs/NOTEBOOK.md section 16.  Run on the GPU box."""
import os, sys, time
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from safe_interactive_crowdnav_amd import metrics as M
from safe_interactive_crowdnav_amd.engine import JmidEngine
from safe_interactive_crowdnav_amd.weights import JMIDWeights, NetDims

REPS = 25


def scenes(E, A, K, T, seed):
    g = torch.Generator().manual_seed(seed)
    walk = torch.cumsum(0.1 * torch.randn([E, K + 1, A, T, 2], generator=g), dim=3) + 1.5 * torch.randn([E, 1, A, 1, 2], generator=g)
    return walk[:, :K].contiguous(), walk[:, K].contiguous()


def median_us(eng, call):
    call()                                                   # warm: workspace, code object
    call()
    eng.profile_enable(["eval_statistics"])
    ev, wall = [], []
    for _ in range(REPS):
        eng.profile_reset()
        torch.cuda.synchronize(); t0 = time.perf_counter()
        call()
        torch.cuda.synchronize(); wall.append((time.perf_counter() - t0) * 1e6)
        n, ms = eng.profile_get()["eval_statistics"]
        assert n == 1
        ev.append(ms * 1e3)
    eng.profile_disable()
    return float(np.median(ev)), float(np.min(ev)), float(np.max(ev)), float(np.median(wall))


def main():
    eng = JmidEngine(JMIDWeights.from_seed(NetDims(ctx_dim=32), 0), joint=True, step=2)
    for tag, (E, A, K, T) in (("cfg3", (256, 5, 20, 12)), ("dense", (256, 25, 64, 12)), ("dense, one episode", (1, 25, 64, 12)),
                              ("shipped", (256, 3, 100, 8)), ("limits", (1, 64, 1024, 24))):
        pos, gt = scenes(E, A, K, T, 2)
        pos, gt = pos.cuda(), gt.cuda()
        col = median_us(eng, lambda: eng.collision_statistics(pos))
        colp = median_us(eng, lambda: eng.collision_statistics(pos, pairs=True))
        line = (f"{tag} E={E} A={A} K={K} T={T}: jmid_collision_statistics {col[0]:.1f} us events (min {col[1]:.1f}, max {col[2]:.1f}; "
                f"{col[3]:.1f} us wall), with pair_out {colp[0]:.1f} us")
        evs = median_us(eng, lambda: eng.eval_statistics(pos, gt))
        line += f" | jmid_eval_statistics {evs[0]:.1f} us events (min {evs[1]:.1f}, max {evs[2]:.1f}; {evs[3]:.1f} us wall)"
        _, _, _, scene = eng.collision_statistics(pos)
        torch.cuda.synchronize()
        print(line, flush=True)
        print("  summary:", {k: round(v, 4) for k, v in M.summarise_collisions(scene.cpu().numpy()).items()}, flush=True)
    pos, _ = scenes(16, 5, 20, 12, 3)
    pos = pos.numpy()
    t0 = time.perf_counter(); M.collision_statistics_host(pos); t_host = time.perf_counter() - t0
    print(f"host, 16 episodes A=5 K=20 T=12: collision_statistics_host {t_host * 1e3:.2f} ms", flush=True)
    assert eng.erange_count() == 0 and eng.timeout_count() == 0
    eng.close()


if __name__ == "__main__":
    main()
