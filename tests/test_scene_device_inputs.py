"""The inputs of tests/test_gpu_scene_device.py, pinned on the host.

The device scene kernel (csrc/scene.hpp) repeats scene.build_scenes_batched operation for operation, with one freedom: the cluster
means are summed in ascending node order on the device and by a BLAS product on the host, whose order is unspecified.  The two can
only choose different clusters when two clusters of DIFFERENT membership lie within rounding of the same distance from the robot
(rows of identical membership tie exactly and give the same mask either way).  Every input set of the GPU tests is therefore held
here to a margin of 1e-9 m - seven orders of magnitude above the rounding of a mean of at most 64 positions of magnitude < 100 m
(64 * 2^-53 * 100 m ~ 7e-13 m) - so that a bit-equal pass there cannot hide behind a coincidence.  A seed that violates the margin is
replaced HERE.
"""
import glob
import inspect
import os

import numpy as np
import pytest

from safe_interactive_crowdnav_amd import scene as SC
from tests.test_scene_golden import replay_histories

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
WRAPPER_CASES = sorted(os.path.basename(p) for p in glob.glob(os.path.join(GOLDEN, "wrapper_*.npz")))
MARGIN = 1e-9
F, DT = 6, 0.25


def wrapper_scene(case):
    """(fixture, human_xy [F, N, 2], robot_xy [F, 2], pose_now) of a reference capture: its histories through the host frame table."""
    z = np.load(os.path.join(GOLDEN, case))
    prev, rob = replay_histories(z)
    hum_xy, rob_xy, pose_now = SC.frame_table(prev, rob, float(z["time_step"]), int(z["past"]))
    return z, hum_xy, rob_xy, pose_now


def synthetic_positions(E, N, seed):
    """The positions scene.synthetic_episodes(E, N, seed) builds its batch from (the same draws in the same order)."""
    rng = np.random.default_rng(seed)
    pos0 = rng.uniform(-2.0, 2.0, (E, N, 2))
    vel = rng.uniform(-0.5, 0.5, (E, N, 2))
    t = np.arange(F + 1) * DT
    hum = pos0[:, None] + vel[:, None] * t[None, :, None, None]
    rob = np.array([0.0, -3.0])[None, None] + np.array([0.0, 0.2])[None, None] * t[None, :, None]
    rob = np.broadcast_to(rob, (E, F + 1, 2))
    return np.ascontiguousarray(hum[:, -F:]), np.ascontiguousarray(rob[:, -F:])


def random_positions(E, N, seed, half_width=6.0, robot=None):
    """E episodes of N pedestrians at U(-half_width, half_width)^2 walking at U(-1, 1)^2 m/s with 1 cm of jitter; the robot at
    U(-3, 3)^2 moving at 0.2 m/s, or at the fixed position ``robot``."""
    rng = np.random.default_rng(seed)
    pos0 = rng.uniform(-half_width, half_width, (E, N, 2))
    vel = rng.uniform(-1.0, 1.0, (E, N, 2))
    t = np.arange(F) * DT
    hum = pos0[:, None] + vel[:, None] * t[None, :, None, None] + 0.01 * rng.standard_normal((E, F, N, 2))
    start = rng.uniform(-3.0, 3.0, (E, 1, 2)) if robot is None else np.broadcast_to(np.asarray(robot, dtype=np.float64), (E, 1, 2))
    rob = start + np.array([0.0, 0.2])[None, None] * t[None, :, None]
    return np.ascontiguousarray(hum), np.ascontiguousarray(rob)


# name -> (human_xy [E, F, N, 2], robot_xy [E, F, 2], force_all_in_cluster): the batched sets of the GPU tests
def batched_sets():
    syn = synthetic_positions(64, 6, 11)
    return {
        "synthetic_natural": (*syn, False),
        "synthetic_forced": (*syn, True),
        "spread": (*random_positions(33, 12, 23), False),                        # clusters differ per episode, n_in ranges widely
        "one_human": (*random_positions(5, 1, 31, half_width=2.5), False),
        "all_lanes": (*random_positions(2, 63, 41), False),                      # N + 1 = 64 nodes: every lane of the wavefront
        "robot_far": (*random_positions(4, 5, 53, half_width=2.0, robot=(40.0, -35.0)), False),   # edge type 1 stays empty
    }


def cluster_margin(human_xy, robot_xy):
    """Per episode: by how much the chosen cluster's mean is nearer the robot than the nearest cluster of different membership
    (+inf when every pedestrian's cluster has the chosen one's membership) - the host twin's own operations."""
    pos = np.concatenate([robot_xy[:, :, None, :], human_xy], axis=2)
    last = pos[:, -1]
    near = np.sqrt(np.square(last[:, :, None] - last[:, None, :]).sum(-1)) < SC.ATTENTION_RADIUS
    means = (near.astype(np.float64) @ last) / near.sum(axis=2, keepdims=True)
    rdist = np.linalg.norm(means - last[:, :1], axis=2)[:, 1:]
    chosen = np.argmin(rdist, axis=1)
    out = np.full(len(last), np.inf)
    for e in range(len(last)):
        differs = (near[e, 1:] != near[e, chosen[e] + 1]).any(axis=1)
        if differs.any():
            out[e] = (rdist[e, differs] - rdist[e, chosen[e]]).min()
    return out


@pytest.mark.parametrize("case", WRAPPER_CASES)
def test_reference_fixtures_hold_the_cluster_margin(case):
    _, hum, rob, _ = wrapper_scene(case)
    assert hum.shape[0] == F
    m = cluster_margin(hum[None], rob[None])
    assert m[0] > MARGIN, f"{case}: the chosen cluster leads by {m[0]:.3e} m only"


def test_there_are_the_fourteen_reference_fixtures():
    other_widths = [c for c in WRAPPER_CASES if c.startswith(("wrapper_jmid_w64_", "wrapper_jmid_w128_"))]      # tests/width_cases.py: hidden 32 and 64
    assert len(WRAPPER_CASES) - len(other_widths) == 14 and len(other_widths) == 2 and "wrapper_jmid_entering.npz" in WRAPPER_CASES


def test_entering_fixture_is_the_threshold_case():
    """A pair of its 3-frame window lies 4.4e-16 m from the attention radius: one ulp of a contracted dx * dx + dy * dy decides an edge."""
    _, hum, rob, _ = wrapper_scene("wrapper_jmid_entering.npz")
    pos = np.concatenate([rob[:, None], hum], axis=1)[-3:]
    d = np.sqrt(np.square(pos[:, :, None] - pos[:, None, :]).sum(-1))
    assert np.abs(d - SC.ATTENTION_RADIUS).min() < 1e-15


@pytest.mark.parametrize("name", sorted(batched_sets()))
def test_batched_sets_hold_the_cluster_margin(name):
    hum, rob, force = batched_sets()[name]
    assert hum.shape[1] == F and hum.shape[2] + 1 <= 64
    if not force:
        m = cluster_margin(hum, rob)
        assert m.min() > MARGIN, f"{name}: episode {int(m.argmin())} leads by {m.min():.3e} m only"


def test_batched_sets_cover_what_they_are_for():
    sets = batched_sets()
    b = SC.build_scenes_batched(*sets["synthetic_forced"][:2], DT, force_all_in_cluster=True)
    syn = SC.synthetic_episodes(64, 6, 11)
    for key in ("x", "x_st", "nbr_sum", "edge_mask", "p0"):          # the positions ARE synthetic_episodes' own
        np.testing.assert_array_equal(b[key], syn[key])
    n_in = SC.build_scenes_batched(*sets["spread"][:2], DT)["in_cluster"].sum(axis=1)
    assert len(np.unique(n_in)) >= 4 and n_in.min() == 1 and n_in.max() >= 4
    assert sets["one_human"][0].shape[2] == 1 and sets["all_lanes"][0].shape[2] == 63
    far = SC.build_scenes_batched(*sets["robot_far"][:2], DT)
    assert not far["robot_in_cluster"].any() and not far["nbr_sum"][:, :, 1].any() and far["nbr_sum"][:, :, 0].any()
    nat = SC.build_scenes_batched(*sets["synthetic_natural"][:2], DT)
    assert nat["robot_in_cluster"].any() and nat["nbr_sum"][:, :, 1].any()


def test_device_scene_is_opt_in():
    from safe_interactive_crowdnav_amd import forecaster as FC
    assert FC.DEFAULTS["device_scene"] is False
    p = inspect.signature(FC.HumanTrajectoryForecasterSim.__init__).parameters["device_scene"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None          # None -> DEFAULTS
    q = inspect.signature(FC.predict_batch).parameters["device_scene"]
    assert q.kind is inspect.Parameter.KEYWORD_ONLY and q.default is False
