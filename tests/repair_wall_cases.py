"""Inputs of the tests of collision repair with walls (tests/test_repair_walls_host.py, tests/test_gpu_repair_walls.py), generated here:
the random walks of tests/repair_cases.py between wall segments laid so that some paths brush or cross them, and the constructed cases
of the rule (one agent brushing a wall, a pair colliding next to one, a step that crosses, a wall's tip, a wall of zero length, a present
position inside the radius).  float32 positions, float64 walls, fixed seeds."""
import numpy as np

from .repair_cases import cluster_samples

THRESHOLD = 0.2
RADIUS = 0.3
DT = 0.25


def corridor(L: int, half_width: float, half_length: float = 3.0) -> np.ndarray:
    """-> walls [L, 4]: the two sides y = -half_width and y = +half_width of a corridor along x, cut into L pieces in all (the lower side
    takes the odd one; L = 1: the upper side alone).  Neighbouring pieces share their end points, as the shipped obstacles do."""
    if L == 1:
        return np.array([[-half_length, half_width, half_length, half_width]])
    lo, hi = (L + 1) // 2, L // 2
    out = []
    for count, y in ((lo, -half_width), (hi, half_width)):
        x = np.linspace(-half_length, half_length, count + 1)
        out += [[x[i], y, x[i + 1], y] for i in range(count)]
    return np.asarray(out, dtype=np.float64)


def wall_cases():
    """name -> (pos [E, K, A, T, 2], p0 [E, A, 2], walls [L, 4]): what the device test compares with the twin; the host test holds every
    one of them to the stability condition under a perturbed exp."""
    return {"e2a3k5t3l2": (*cluster_samples(2, 3, 3, 5, 4, start_std=0.2), corridor(2, 1.3)),   # several samples, two steps, both sides
            "a1t2k1l1": (*cluster_samples(6, 1, 2, 1, 2, start_std=0.15), corridor(1, 0.45)),   # the smallest shape: one agent, one wall
            "k300": (*cluster_samples(1, 3, 8, 300, 11, start_std=0.2, step_std=0.03), corridor(4, 4.0)),     # more samples than threads
            "l64": (*cluster_samples(2, 3, 4, 4, 5), corridor(64, 0.8)),                     # the most walls
            "a64t24l64": (*cluster_samples(2, 64, 24, 1, 1, start_std=4.0, step_std=0.05), corridor(64, 17.0, 20.0)),      # the entry's limits
            "e5a3k4t4": (*cluster_samples(5, 3, 4, 4, 9, start_std=0.5), corridor(2, 1.5)),   # the partition case
            "e3a3k6t4": (*cluster_samples(3, 3, 4, 6, 7), corridor(3, 0.9))}                 # the padded case (counts 3, 1, 2)


def constructed():
    """name -> (pos [1, 1, A, 4, 2] float32, p0 [1, A, 2] float32 or None, walls [L, 4]): one sample each, against the wall y = 0,
    0 <= x <= 4 unless said otherwise, at RADIUS and THRESHOLD."""
    T, wall = 4, np.array([[0.0, 0.0, 4.0, 0.0]])
    x = 1.0 + 0.4 * np.arange(T)

    def path(xs, ys):
        return np.stack([np.broadcast_to(np.asarray(xs, dtype=np.float64), (T,)), np.broadcast_to(np.asarray(ys, dtype=np.float64), (T,))], axis=-1)

    def one(*paths):
        return np.stack(paths)[None, None].astype(np.float32)

    return {"brush": (one(path(x, 0.25)), None, wall),                                        # one agent walking along the wall, 5 cm too close
            "brush_p0": (one(path(x, 0.25)), np.float32([[[0.6, 0.5]]]), wall),
            "pair": (one(path(x, 0.33), path(x, 0.45)), None, wall),                          # a pair colliding next to the wall
            "cross": (one(path(1.0 + 0.1 * np.arange(T), [0.9, 0.6, 0.35, -0.05])), None, wall),      # the last step crosses
            "cross_back": (one(path(1.0 + 0.1 * np.arange(T), [0.9, 0.5, -0.1, 0.5])), None, wall),  # one point behind the wall
            "tip": (one(path(4.2, [0.9, 0.3, -0.3, -0.9])), None, wall),                      # walking past the wall's end
            "point": (one(path(x, 0.2)), None, np.array([[1.8, 0.0, 1.8, 0.0]])),             # a wall of zero length
            "p0_inside": (one(path(x, 0.5)), np.float32([[[0.6, 0.1]]]), wall)}               # the present position is too close: no repair
