"""The NumPy twin of guided sampling (``metrics.guide_step_host``; include/jmid_hip.h states the rule, tests/test_gpu_guide.py holds the
kernel to the twin bit for bit): the properties of the rule on constructed inputs, and the refusals of the public keywords."""
import numpy as np
import pytest

from safe_interactive_crowdnav_amd import metrics, schedule
from safe_interactive_crowdnav_amd.forecaster import guidance_arguments, sampling_constraints
from tests.guide_cases import DT, THRESHOLD, integrate64, min_segment_distance, same_bits, velocities


def head_on():
    """Two agents walking into each other: A 2, T 4, dt 0.25, 1 m/s each, 0.6 m apart -> they meet in the middle of segment 0 -> 1."""
    p0 = np.array([[[-0.3, 0.0], [0.3, 0.01]]], dtype=np.float32)
    x = np.zeros((1, 2, 4, 2), dtype=np.float32)
    x[0, 0, :, 0], x[0, 1, :, 0] = 1.0, -1.0
    return x, p0


def test_zero_weight_and_far_apart_scenes_return_the_input_bits():
    x, p0 = head_on()
    out, rows = metrics.guide_step_host(x, p0, DT, THRESHOLD, weight=0.0)
    assert same_bits(out, x) and not rows.any()
    far = p0.copy()
    far[0, 1] = (50.0, 50.0)
    out, rows = metrics.guide_step_host(x, far, DT, THRESHOLD, weight=0.02)
    assert same_bits(out, x) and not rows.any()


def test_head_on_pair_is_pushed_apart():
    x, p0 = head_on()
    out, rows, (q0, q1) = metrics.guide_step_host(x, p0, 0.25, 0.2, weight=0.02, n_inner=4, return_positions=True)
    before, after = min_segment_distance(integrate64(x, p0, 0.25)), min_segment_distance(integrate64(out, p0, 0.25))
    print(f"head on: minimum segment distance {before[0, 0]:.6f} -> {after[0, 0]:.6f} m, rows {rows.tolist()}")
    assert before[0, 0] < 0.2 and after[0, 0] > before[0, 0]
    assert rows[0, 0, 0] == 1 and 1 <= rows[0, 0, 1] <= 4
    assert not same_bits(out, x)
    one = metrics.guide_step_host(x, p0, 0.25, 0.2, weight=0.02, n_inner=1)[1]
    assert one[0, 0].tolist() == [1.0, 1.0]


def test_write_back_integrates_to_the_final_positions():
    """x_out integrated in fp64 equals q_final within T fp32 ulps of the largest |x| * dt: one rounding per point, summed over <= T points."""
    rng = np.random.default_rng(3)
    E, A, K, T = 2, 3, 4, 8
    p0 = rng.normal(0.0, 0.2, size=(E, A, 2)).astype(np.float32)
    x = rng.normal(0.0, 0.6, size=(E, K * A, T, 2)).astype(np.float32)
    out, rows, (q0, q1) = metrics.guide_step_host(x, p0, DT, THRESHOLD, weight=0.02, n_inner=4, return_positions=True)
    assert rows[..., 0].sum() >= 1
    got = integrate64(out, p0, DT)
    bound = T * 2.0 ** -23 * float(np.abs(out).max()) * DT
    err = float(np.abs(got - q1).max())
    print(f"write-back: max |integrate(x_out) - q_final| = {err:.3e}, bound {bound:.3e}")
    assert err <= bound
    still = rows[..., 0] == 0
    assert same_bits(out.reshape(E, K, A, T, 2)[still], x.reshape(E, K, A, T, 2)[still])


def test_a_far_agent_keeps_its_bits():
    x2, p2 = head_on()
    rng = np.random.default_rng(5)
    x = np.concatenate([x2, rng.normal(0.0, 0.5, size=(1, 1, 4, 2)).astype(np.float32)], axis=1)
    p0 = np.concatenate([p2, np.array([[[40.0, -30.0]]], dtype=np.float32)], axis=1)
    out, rows = metrics.guide_step_host(x, p0, DT, THRESHOLD, weight=0.02)
    assert rows[0, 0, 0] == 1
    assert same_bits(out[0, 2], x[0, 2]) and not same_bits(out[0, :2], x[0, :2])


def test_padded_episode_equals_its_compacted_block():
    rng = np.random.default_rng(7)
    E, A, K, T = 3, 4, 3, 6
    counts = [4, 1, 2]
    p0 = rng.normal(0.0, 0.15, size=(E, A, 2)).astype(np.float32)
    x = rng.normal(0.0, 0.5, size=(E, K * A, T, 2)).astype(np.float32)
    xv = x.reshape(E, K, A, T, 2)
    for e, n in enumerate(counts):      # whatever the padded rows hold
        xv[e, :, n:] = np.nan
        p0[e, n:] = np.nan
    out, rows = metrics.guide_step_host(x, p0, DT, THRESHOLD, weight=0.02, n_agents=counts)
    ov = out.reshape(E, K, A, T, 2)
    assert rows[0, :, 0].sum() >= 1 and not rows[1].any()
    for e, n in enumerate(counts):
        alone, arow = metrics.guide_step_host(np.ascontiguousarray(xv[e:e + 1, :, :n]).reshape(1, K * n, T, 2), p0[e:e + 1, :n], DT, THRESHOLD,
                                              weight=0.02)
        assert same_bits(ov[e, :, :n], alone.reshape(K, n, T, 2)) and np.array_equal(rows[e], arow[0])
        assert same_bits(ov[e, :, n:], xv[e, :, n:])


def test_a_single_agent_moves_only_next_to_a_wall():
    p0 = np.array([[[0.0, 0.05]]], dtype=np.float32)
    x = np.zeros((1, 2, 4, 2), dtype=np.float32)      # K = 2 samples of one agent walking along a wall on the x axis
    x[0, :, :, 0] = 0.5
    walls = np.array([[-1.0, 0.0, 3.0, 0.0]])
    out, rows = metrics.guide_step_host(x, p0, DT, THRESHOLD, weight=0.02)
    assert same_bits(out, x) and not rows.any()
    out, rows = metrics.guide_step_host(x, p0, DT, THRESHOLD, weight=0.02, walls=walls, wall_radius=0.3)
    assert rows[..., 0].all() and not same_bits(out, x)
    assert (integrate64(out, p0, DT)[..., 1] > integrate64(x, p0, DT)[..., 1]).all()      # away from the wall
    # T = 1: no pedestrian segment - untouched without walls, the step from p0 against the walls with them
    x1, p1 = np.ascontiguousarray(head_on()[0][:, :, :1]), head_on()[1]
    x1[..., 1] = 0.2      # towards the wall: the step's far end is the closest point (a step parallel to it would weigh p0, which is fixed)
    out, rows = metrics.guide_step_host(x1, p1, DT, THRESHOLD, weight=0.02)
    assert same_bits(out, x1) and not rows.any()
    out, rows = metrics.guide_step_host(x1, p1, DT, THRESHOLD, weight=0.02, walls=np.array([[-1.0, 0.1, 1.0, 0.1]]), wall_radius=0.3)
    assert rows[0, 0, 0] == 1 and not same_bits(out, x1)


def test_a_sample_that_is_not_finite_is_untouched():
    x, p0 = head_on()
    x = np.concatenate([x, x], axis=1)      # K = 2
    x[0, 3, 2, 0] = np.nan
    out, rows = metrics.guide_step_host(x, p0, DT, THRESHOLD, weight=0.02)
    assert rows[0, 0, 0] == 1 and not rows[0, 1].any() and same_bits(out[0, 2:], x[0, 2:])


def test_twin_refusals():
    x, p0 = head_on()
    for kw in (dict(threshold=-1.0), dict(margin=np.nan), dict(tau=0.0), dict(weight=-0.1), dict(weight=np.inf), dict(n_inner=0),
               dict(n_inner=65), dict(wall_radius=0.3), dict(walls=np.zeros((1, 4))), dict(walls=np.full((1, 4), np.nan), wall_radius=0.1)):
        with pytest.raises(ValueError):
            metrics.guide_step_host(x, p0, DT, **kw)
    for dt in (0.0, np.inf):
        with pytest.raises(ValueError):
            metrics.guide_step_host(x, p0, dt)
    with pytest.raises(ValueError):
        metrics.guide_step_host(x, None, DT)


def test_guidance_weights():
    w = schedule.guidance_weights(0.02, step=5)
    sched = schedule.VarianceSchedule.linear()
    assert w.dtype == np.float64 and w.shape == (5,)
    assert np.array_equal(w, 0.02 * sched.alpha_bars[[80, 60, 40, 20, 0]].astype(np.float64))
    assert w[-1] == 0.02 and w[0] < 0.02 * 0.2 and (np.diff(w) > 0).all()
    assert schedule.guidance_weights(0.02, step=4, table="last_half").tolist() == [0.0, 0.0, 0.02, 0.02]
    assert schedule.guidance_weights(0.0, step=2).tolist() == [0.0, 0.0]
    with pytest.raises(ValueError):
        schedule.guidance_weights(-1.0)
    with pytest.raises(ValueError):
        schedule.guidance_weights(0.02, table="nope")


def test_keyword_refusals():
    """``guidance=`` on the forecaster, ``predict_batch`` and ``offline.generate``: what ``sampling_constraints`` refuses."""
    ok = sampling_constraints(None, 0.2, guidance={}, step=5)
    assert ok.guidance is not None and ok.guidance.n_inner == 4 and ok.guidance.threshold == 0.2 and len(ok.guidance.weights) == 5
    assert sampling_constraints(None, 0.2).guidance is None
    walls = np.array([[0.0, 0.0, 1.0, 0.0]])
    g = sampling_constraints(None, 0.2, static_obstacles=walls, wall_radius=0.3, guidance={"walls": True}, step=5).guidance
    assert g.walls.shape == (1, 4) and g.wall_radius == 0.3
    both = sampling_constraints(None, 0.2, constraint_type="opt_softplus", guidance={"scale": 0.01}, step=5)
    assert both.repair == {} and both.guidance.weights[-1] == 0.01
    for kw in (dict(guidance={"walls": True}),                                              # walls without static_obstacles / wall_radius
               dict(guidance={"walls": True}, static_obstacles=walls),
               dict(guidance={"nope": 1}), dict(guidance={"n_inner": 0}), dict(guidance={"n_inner": 65}), dict(guidance={"scale": -1.0}),
               dict(guidance={"tau": 0.0}), dict(guidance={"margin": -0.1}), dict(guidance={"weights": [0.1, -0.1, 0, 0, 0]}),
               dict(guidance={"weights": [0.1, 0.1]}),                                      # not one per step-table entry
               dict(guidance={"weights": [0.1] * 5, "scale": 0.02}),                        # both
               dict(guidance={}, rounds=3)):                                                # a rerun would have to be guided too
        with pytest.raises(ValueError):
            sampling_constraints(kw.pop("rounds", None), 0.2, step=5, **kw)
    with pytest.raises(ValueError):
        guidance_arguments({}, 0.2, step=5, sampling="ddpm")
