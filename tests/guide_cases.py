"""Inputs and helpers of the guided-sampling tests (tests/test_guide_host.py, tests/test_gpu_guide.py, tests/test_gpu_guided_*.py): the
random walks of tests/repair_cases.py and the corridors of tests/repair_wall_cases.py as VELOCITY blocks x [E, K*A, T, 2] - what the
denoise loop holds -, and fp64 helpers that judge a block by its integrated positions."""
import numpy as np

from .repair_cases import cluster_samples
from .repair_wall_cases import corridor

THRESHOLD = 0.2
RADIUS = 0.3
DT = 0.25


def same_bits(a, b) -> bool:
    a, b = (np.ascontiguousarray(v.detach().cpu().numpy() if hasattr(v, "detach") else v, dtype=np.float32) for v in (a, b))
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def velocities(pos: np.ndarray, p0: np.ndarray, dt: float = DT) -> np.ndarray:
    """pos [E, K, A, T, 2], p0 [E, A, 2] -> x [E, K*A, T, 2] float32: the steps of every path over dt, the first one from p0."""
    E, K, A, T, _ = pos.shape
    prev = np.concatenate([np.broadcast_to(p0[:, None, :, None], pos[:, :, :, :1].shape), pos[:, :, :, :-1]], axis=3)
    return np.ascontiguousarray(((pos - prev) / np.float32(dt)).astype(np.float32).reshape(E, K * A, T, 2))


def integrate64(x: np.ndarray, p0: np.ndarray, dt: float = DT) -> np.ndarray:
    """x [E, K*A, T, 2], p0 [E, A, 2] -> positions float64 [E, K, A, T, 2], the rule's "Integrate"."""
    E, KA, T, _ = x.shape
    A = p0.shape[1]
    v = np.asarray(x, dtype=np.float64).reshape(E, KA // A, A, T, 2)
    return np.asarray(p0, dtype=np.float64)[:, None, :, None, :] + float(np.float32(dt)) * np.cumsum(v, axis=3)


def min_segment_distance(pos: np.ndarray) -> np.ndarray:
    """pos [E, K, A, T, 2] float64 -> [E, K]: the smallest distance between two agents over every pair and segment (closest-point form);
    +inf with fewer than two agents or points."""
    E, K, A, T, _ = pos.shape
    out = np.full((E, K), np.inf)
    for i in range(A):
        for j in range(i + 1, A):
            rel = pos[:, :, i] - pos[:, :, j]
            a, b = rel[:, :, :-1], rel[:, :, 1:]
            ab = b - a
            den = (ab * ab).sum(-1)
            with np.errstate(divide="ignore", invalid="ignore"):
                u = np.where(den > 0, np.clip(-(a * ab).sum(-1) / den, 0.0, 1.0), 0.0)
            c = a + u[..., None] * ab
            d = np.sqrt((c * c).sum(-1))
            if d.shape[-1]:
                out = np.minimum(out, d.min(axis=-1))
    return out


def guide_cases():
    """name -> (x [E, K*A, T, 2], p0 [E, A, 2], keywords of guide_step): the shapes the device is held to the twin on."""
    def block(E, A, K, T, seed, **kw):
        pos, p0 = cluster_samples(E, A, T, K, seed, **kw)
        return velocities(pos, p0), p0

    return {"e2a3k4t8": (*block(2, 3, 4, 8, 21), {}),                                                    # the plain case
            "a1k2t4l2": (*block(1, 1, 2, 4, 2, start_std=0.15), dict(walls=corridor(2, 0.45), wall_radius=RADIUS)),      # wall only
            "a12k2t24": (*block(1, 12, 2, 24, 23, start_std=0.6, step_std=0.05), {}),                    # 288 points > 256 threads
            "e3a4k3t6": (*block(3, 4, 3, 6, 9, start_std=0.1), dict(n_agents=[4, 1, 2])),                               # padded
            "e3a4k3t6l3": (*block(3, 4, 3, 6, 7), dict(n_agents=[4, 1, 2], walls=corridor(3, 0.9), wall_radius=RADIUS)),
            "a64t24l64": (*block(1, 64, 1, 24, 1, start_std=4.0, step_std=0.05), dict(walls=corridor(64, 17.0, 20.0), wall_radius=RADIUS)),   # the LDS limit
            "t1": (*block(2, 3, 4, 1, 25), {}),                                                          # no pedestrian segment
            "t1l2": (*block(2, 3, 4, 1, 25), dict(walls=corridor(2, 0.45), wall_radius=RADIUS)),
            "n_inner1": (*block(2, 3, 4, 8, 21), dict(n_inner=1)),
            "e2a3k4t8l4": (*block(2, 3, 4, 8, 21), dict(walls=corridor(4, 0.8), wall_radius=RADIUS))}
