"""Collision repair without a GPU: the rule of include/jmid_hip.h (``jmid_repair_collisions``) through its NumPy twin
``metrics.repair_collisions_host`` - against a scalar loop that takes one agent and one pair at a time, on generated crossing crowds
(every colliding sample repaired, none at ``max_iter``, untouched samples bit for bit), on the degenerate inputs, under a perturbed
``exp`` - and the Python layer's routes and refusals."""
import itertools
import math

import numpy as np
import pytest

from safe_interactive_crowdnav_amd import metrics, offline
from safe_interactive_crowdnav_amd.forecaster import (HumanTrajectoryForecasterSim, plan_route, predict_batch, repair_arguments,
                                                      repair_totals, write_configs)
from safe_interactive_crowdnav_amd.weights import JMIDWeights, NetDims

from .repair_cases import SHAPES, THRESHOLD, cluster_samples, crossing_samples, gpu_cases
from .test_forecaster_route_table import BATCH, SINGLE

DEFAULTS = dict(margin=0.02, tau=0.005, step=0.02, max_iter=32)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def predicate_distance(ax, ay, bx, by):
    """``lineseg_dist`` as the predicate has it (csrc/collision_stats.hpp::cls_segment_dist), on Python floats."""
    if ax == bx and ay == by:
        return math.sqrt(ax * ax + ay * ay)
    ux, uy = bx - ax, by - ay
    n = math.sqrt(ux * ux + uy * uy)
    dx, dy = ux / n, uy / n
    h = max(ax * dx + ay * dy, (-bx) * dx + (-by) * dy, 0.0)
    return float(np.hypot(h, abs((-ax) * dy - (-ay) * dx)))


def scalar_repair(x32, threshold, margin, tau, step, max_iter):
    """The rule word for word on ONE joint sample x32 [A, T, 2] float32, one agent and one pair at a time, Python floats (fp64).
    -> (sample out float32, min_dist before, min_dist after, iterations, state)."""
    A, T, _ = x32.shape
    pairs = [(i, j) for i in range(A) for j in range(i + 1, A)]

    def min_dist(v):
        best = math.inf
        for i, j in pairs:
            for s in range(T - 1):
                d = predicate_distance(v[i][s][0] - v[j][s][0], v[i][s][1] - v[j][s][1], v[i][s + 1][0] - v[j][s + 1][0],
                                       v[i][s + 1][1] - v[j][s + 1][1])
                best = d if d < best or d != d else best
        return best

    x = [[[float(c) for c in p] for p in agent] for agent in x32]
    before = min_dist(x)
    if before != before:
        return x32.copy(), before, before, 0, metrics.REPAIR_NAN
    if A < 2 or not before < threshold:
        return x32.copy(), before, before, 0, metrics.REPAIR_UNTOUCHED
    m, stop = threshold + margin, threshold + margin * 0.5

    def segment(i, j, s):      # the closest-point form for the pair i < j
        ax, ay, bx, by = x[i][s][0] - x[j][s][0], x[i][s][1] - x[j][s][1], x[i][s + 1][0] - x[j][s + 1][0], x[i][s + 1][1] - x[j][s + 1][1]
        abx, aby = bx - ax, by - ay
        den = abx * abx + aby * aby
        u = min(max(-(ax * abx + ay * aby) / den, 0.0), 1.0) if den > 0.0 else 0.0
        cx, cy = ax + u * abx, ay + u * aby
        d = math.sqrt(cx * cx + cy * cy)
        nx, ny = (cx / d, cy / d) if d > 0.0 else (1.0, 0.0)
        z = (m - d) / tau
        e = float(np.exp(-abs(z)))
        return d, u, nx, ny, (1.0 / (1.0 + e) if z >= 0.0 else e / (1.0 + e))

    iters = 0
    for _ in range(max_iter):
        dmin = min(segment(i, j, s)[0] for i, j in pairs for s in range(T - 1))
        if dmin >= stop:
            break
        new = [[[0.0, 0.0] for _ in range(T)] for _ in range(A)]
        for a in range(A):
            for t in range(T):
                g = [0.0, 0.0]
                for b in range(A):                       # partners ascending
                    if b == a:
                        continue
                    i, j = min(a, b), max(a, b)
                    for s, far in ((t - 1, True), (t, False)):      # the segment that ends here, then the one that starts here
                        if not 0 <= s < T - 1:
                            continue
                        _, u, nx, ny, sg = segment(i, j, s)
                        w = sg * u if far else sg * (1.0 - u)
                        px, py = w * nx, w * ny
                        g = [g[0] - px, g[1] - py] if a == i else [g[0] + px, g[1] + py]
                new[a][t] = [x[a][t][0] - step * g[0], x[a][t][1] - step * g[1]]
        x = new
        iters += 1
    r32 = np.asarray(x, dtype=np.float64).astype(np.float32)
    after = min_dist([[[float(c) for c in p] for p in agent] for agent in r32])
    if after == after and not after < threshold:
        return r32, before, after, iters, metrics.REPAIR_REPAIRED
    return x32.copy(), before, before, iters, metrics.REPAIR_REVERTED


@pytest.mark.parametrize("A,T,K,seed", [(2, 2, 3, 3), (3, 3, 5, 1), (5, 12, 4, 2)])
def test_the_twin_equals_the_scalar_loop(A, T, K, seed):
    pos, _ = cluster_samples(1, A, T, K, seed)
    out, _, sample, episode = metrics.repair_collisions_host(pos, THRESHOLD)
    assert episode[0, 0] >= 1                              # (the case exercises the iteration)
    for k in range(K):
        want, before, after, iters, state = scalar_repair(pos[0, k], THRESHOLD, **DEFAULTS)
        assert (int(sample[0, k, 2]), int(sample[0, k, 3])) == (iters, state)
        assert sample[0, k, 0] == before and sample[0, k, 1] == after
        # the same operations in the same order: the same bits (both call the same exp)
        assert np.array_equal(bits(out[0, k]), bits(want))
    moved = sample[0, :, 3] == metrics.REPAIR_REPAIRED
    assert episode[0].tolist() == [int((sample[0, :, 3] > 0).sum()), int(moved.sum()), int(sample[0, :, 2].max())]


@pytest.fixture(scope="module")
def crossings():
    """The generated crowds and the twin's answer on each, computed once."""
    cases = []
    for E, A, T, K, seed, sigma, frame in SHAPES:
        pos, p0 = crossing_samples(E, A, T, K, seed, sigma, frame)
        cases.append((pos, p0, metrics.repair_collisions_host(pos, THRESHOLD)))
    return cases


def test_every_colliding_sample_of_the_crossings_is_repaired(crossings):
    total = 0
    for pos, _, (out, _, sample, episode) in crossings:
        _, _, before, _ = metrics.collision_statistics_host(pos, THRESHOLD)
        colliding = before[..., 3] > 0
        total += int(colliding.sum())
        state = sample[..., 3]
        assert np.array_equal(state == metrics.REPAIR_REPAIRED, colliding) and np.all(state[~colliding] == metrics.REPAIR_UNTOUCHED)
        _, _, after, scene = metrics.collision_statistics_host(out, THRESHOLD)
        assert not (after[..., 3] > 0).any() and np.all(scene[:, 0] == 0.0)
        assert np.array_equal(bits(out[~colliding]), bits(pos[~colliding]))             # untouched: bit for bit
        assert sample[..., 2].max() < DEFAULTS["max_iter"]                                # nobody reaches the cap
        assert np.array_equal(sample[..., 0], before[..., 0]) and np.array_equal(sample[..., 1], after[..., 0])
        assert np.array_equal(episode[:, 0], colliding.sum(axis=1)) and np.array_equal(episode[:, 1], colliding.sum(axis=1))
        # a repaired sample clears the threshold by about half the margin (the stop rule), and no point moves further than the steps allow
        assert after[..., 0][colliding].min() >= THRESHOLD + 0.25 * DEFAULTS["margin"] if colliding.any() else True
        assert np.abs(out.astype(np.float64) - pos).max() <= sample[..., 2].max() * DEFAULTS["step"] * (pos.shape[2] - 1) * 2
    assert total >= 40


@pytest.mark.parametrize("ulps", [-2, 2])
def test_two_ulps_of_exp_move_neither_a_state_nor_an_iteration_count(crossings, ulps):
    """What separates the kernel from the twin is the device's exp: 2 fp64 ulps of it must not show in any decision of the fixtures, nor
    in any bit of the fp32 output."""
    def exp(v):
        e = np.exp(v)
        for _ in range(abs(ulps)):
            e = np.nextafter(e, np.inf if ulps > 0 else -np.inf)
        return e
    for pos, _, (out, _, sample, episode) in crossings:
        out2, _, sample2, episode2 = metrics.repair_collisions_host(pos, THRESHOLD, exp=exp)
        assert np.array_equal(sample2[..., 2:], sample[..., 2:]) and np.array_equal(episode2, episode)
        assert np.array_equal(bits(out2), bits(out))
    for name, (pos, _) in gpu_cases().items():             # what the device test compares with the twin: the same condition
        out, _, sample, episode = metrics.repair_collisions_host(pos, THRESHOLD)
        out2, _, sample2, episode2 = metrics.repair_collisions_host(pos, THRESHOLD, exp=exp)
        assert episode[:, 1].sum() >= 1, name
        assert np.array_equal(sample2[..., 2:], sample[..., 2:]) and np.array_equal(episode2, episode), name
        assert np.array_equal(bits(out2), bits(out)), name


def test_velocities_of_repaired_samples():
    E, A, T, K, seed, sigma, frame = SHAPES[1]
    pos, p0 = crossing_samples(E, A, T, K, seed, sigma, frame)
    dt = 0.25
    vel = np.diff(np.concatenate([np.broadcast_to(p0[:, None, :, None], pos[:, :, :, :1].shape), pos], axis=3), axis=3) / np.float32(dt)
    vel = vel.astype(np.float32)
    out, vel_out, sample, _ = metrics.repair_collisions_host(pos, THRESHOLD, p0=p0, dt=dt, vel=vel)
    fixed = sample[..., 3] == metrics.REPAIR_REPAIRED
    assert fixed.any() and np.array_equal(bits(vel_out[~fixed]), bits(vel[~fixed]))
    prev = np.concatenate([np.broadcast_to(p0[:, None, :, None], out[:, :, :, :1].shape), out[:, :, :, :-1]], axis=3).astype(np.float64)
    want = ((out.astype(np.float64) - prev) / dt).astype(np.float32)
    assert np.array_equal(bits(vel_out[fixed]), bits(want[fixed]))
    with pytest.raises(ValueError, match="p0"):
        metrics.repair_collisions_host(pos, THRESHOLD, vel=vel)


def test_degenerate_inputs():
    T = 4
    far = np.stack([np.full(T, 9.0), np.arange(T) * 0.5], axis=-1)
    # k = 0: two agents at rest on one point (d = 0 on every segment: the (1, 0) normal); 1: a pair walking with one velocity (den = 0);
    # 2: a NaN coordinate; 3: far apart
    pos = np.zeros((1, 4, 3, T, 2), dtype=np.float32)
    pos[0, :, 2] = far
    pos[0, 0, 0] = pos[0, 0, 1] = (1.0, 1.0)
    pos[0, 1, 0] = np.stack([np.arange(T) * 0.25, np.zeros(T)], axis=-1)
    pos[0, 1, 1] = pos[0, 1, 0] + np.float32([0.0625, 0.03125])
    pos[0, 2, 0, 1, 0] = np.nan
    pos[0, 3, 0], pos[0, 3, 1] = far + 3.0, far - 3.0
    out, _, sample, episode = metrics.repair_collisions_host(pos, THRESHOLD)
    assert sample[0, :, 3].tolist() == [1, 1, 3, 0] and episode[0, :2].tolist() == [2, 2]
    assert np.array_equal(bits(out[0, 2:]), bits(pos[0, 2:])) and np.isnan(sample[0, 2, :2]).all()
    # coincident at rest: pushed apart along x only, symmetrically, agent 0 towards +x... the pair's i subtracts -sigma n: it moves to +x
    assert np.all(out[0, 0, 0, :, 0] > 1.0) and np.all(out[0, 0, 1, :, 0] < 1.0) and np.all(out[0, 0, :2, :, 1] == 1.0)
    assert np.array_equal(bits(out[0, :2, 2]), bits(pos[0, :2, 2]))                     # the bystander feels nothing (sigma underflows to 0)
    assert metrics.collision_statistics_host(out[:, :2], THRESHOLD)[2][..., 3].max() == 0
    for k in (0, 1):
        want, before, after, iters, state = scalar_repair(pos[0, k], THRESHOLD, **DEFAULTS)
        assert np.array_equal(bits(out[0, k]), bits(want)) and sample[0, k].tolist() == [before, after, iters, state]
    # A = 1: nothing to repair
    out1, _, sample1, episode1 = metrics.repair_collisions_host(pos[:, :, :1], THRESHOLD)
    assert np.array_equal(bits(out1[0, [0, 1, 3]]), bits(pos[0, [0, 1, 3], :1])) and np.all(sample1[0, [0, 1, 3], 3] == 0)
    assert np.all(np.isinf(sample1[0, [0, 1, 3], 0])) and episode1.tolist() == [[0, 0, 0]]
    # max_iter = 0: the identity plus the flags; a max_iter too small to finish: state 2 and the input bits back
    for cap in (0, 1):
        out0, _, sample0, episode0 = metrics.repair_collisions_host(pos, THRESHOLD, max_iter=cap)
        assert np.array_equal(bits(out0), bits(pos), ) and sample0[0, :, 3].tolist() == [2, 2, 3, 0]
        assert sample0[0, :2, 2].tolist() == [cap, cap] and episode0.tolist() == [[2, 0, cap]]
        assert np.array_equal(sample0[0, :2, 1], sample0[0, :2, 0])
    # threshold 0: nothing collides; a huge one: everything reverts, nothing is NaN
    assert np.all(metrics.repair_collisions_host(pos[:, [0, 1, 3]], 0.0)[2][..., 3] == 0)
    outb, _, sampleb, _ = metrics.repair_collisions_host(pos[:, [0, 1, 3]], 1e9)
    assert np.all(sampleb[..., 3] == 2) and np.all(sampleb[..., 2] == 32) and np.array_equal(bits(outb), bits(pos[:, [0, 1, 3]]))
    assert np.isfinite(sampleb).all()


def test_padded_counts_equal_the_compacted_episode():
    pos, p0 = cluster_samples(3, 3, 4, 6, 7)
    counts = np.array([3, 1, 2])
    padded = pos.copy()
    for e, n in enumerate(counts):
        padded[e, :, n:] = np.nan
    out, _, sample, episode = metrics.repair_collisions_host(padded, THRESHOLD, n_agents=counts)
    assert episode[:, 0].sum() >= 2 and episode[1].tolist() == [0, 0, 0]
    for e, n in enumerate(counts):
        alone = metrics.repair_collisions_host(np.ascontiguousarray(pos[e:e + 1, :, :n]), THRESHOLD)
        assert np.array_equal(bits(out[e, :, :n]), bits(alone[0][0])) and np.isnan(out[e, :, n:]).all()
        assert np.array_equal(sample[e], alone[2][0]) and np.array_equal(episode[e], alone[3][0])
    with pytest.raises(ValueError, match="n_agents"):
        metrics.repair_collisions_host(padded, THRESHOLD, n_agents=[3, 0, 2])


def test_route_table_is_unchanged_and_repair_is_staged():
    for kw, k, route in SINGLE:
        assert plan_route(k=k, K=10, A=3, H=12, repair=False, **kw) == route
        assert plan_route(k=k, K=10, A=3, H=12, repair=True, **kw) == (route.scene, "staged", route.rank)
    for kw, k, route in BATCH:
        assert plan_route(k=k, K=8, A=2, H=6, batch=True, repair=False, **kw) == route
        assert plan_route(k=k, K=8, A=2, H=6, batch=True, repair=True, **kw) == (route.scene, "staged", route.rank)
    flags = dict(k=(5, 20), A=(3, 40), device_topk=(True, False), device_scene=(False, True), device_frames=(False, True),
                 check=(False, True), short=(False, True), frames=(True, False), batch=(False, True), padded=(False, True),
                 resident=(False, True), tracks=(False, True), collision_free=(False, True))
    for values in itertools.product(*flags.values()):
        kw = dict(zip(flags, values), K=20, H=8)
        plain = plan_route(**kw)
        assert plan_route(**kw, repair=False) == plain
        assert plan_route(**kw, repair=True) == (plain.scene, "staged", plain.rank)
    assert plan_route(k=5, K=20, A=3, H=8, repair=True) == ("host", "staged", "device_resident")


def test_python_refusals(tmp_path):
    env, ypath = write_configs(str(tmp_path), joint=True, ctx_dim=32, N=3, K=6, k_ret=3, H=4, step=2)
    weights = JMIDWeights.from_seed(NetDims(ctx_dim=32), 1)
    walls = np.array([[[0.0, 0.0], [1.0, 0.0]]])
    with pytest.raises(ValueError, match="walls are not in the repair's objective"):
        HumanTrajectoryForecasterSim(env, ypath, weights=weights, rng_compat="device", collision_free_rounds=2, constraint_type="opt_softplus",
                                     static_obstacles=walls, wall_radius=0.3)
    with pytest.raises(ValueError, match="unknown constraint_type"):
        HumanTrajectoryForecasterSim(env, ypath, weights=weights, constraint_type="opt_relu")
    with pytest.raises(ValueError, match="without constraint_type"):
        HumanTrajectoryForecasterSim(env, ypath, weights=weights, repair_options={"tau": 0.01})
    for bad, word in (({"tau": 0.0}, "tau"), ({"step": -1.0}, "step"), ({"margin": float("nan")}, "margin"), ({"max_iter": 1025}, "max_iter"),
                      ({"rounds": 3}, "unknown repair_options")):
        with pytest.raises(ValueError, match=word):
            repair_arguments("opt_softplus", bad)
    assert repair_arguments(None) is None and repair_arguments("opt_softplus") == {} and repair_arguments("opt_softplus", {"tau": 0.01}) == {"tau": 0.01}
    ctx, p0 = np.zeros((3, 32), np.float32), np.zeros((3, 2), np.float32)
    with pytest.raises(ValueError, match="with_constraints=True"):
        offline.sample(None, 4, ctx, 5, True, constraint_type="opt_softplus", _integrate=(p0, 0.25))
    with pytest.raises(ValueError, match="positions"):
        offline.sample(None, 4, ctx, 5, True, constraint_type="opt_softplus", with_constraints=True)
    with pytest.raises(ValueError, match="walls are not"):
        offline.generate(None, ctx, p0, 0.25, 4, 5, True, with_constraints=True, constraint_type="opt_softplus", static_obstacles=walls, wall_radius=0.3)
    hum, rob = np.zeros((2, 6, 3, 2)), np.zeros((2, 6, 2))
    kw = dict(num_samples=6, num_ret_samples=3, horizon=4, time_step=0.25)
    with pytest.raises(ValueError, match="walls are not"):
        predict_batch(None, hum, rob, [0, 1], noise="device", collision_free_rounds=2, constraint_type="opt_softplus", static_obstacles=walls,
                      wall_radius=0.3, **kw)
    with pytest.raises(ValueError, match="unknown constraint_type"):
        predict_batch(None, hum, rob, [0, 1], constraint_type="softplus", **kw)
    assert repair_totals(np.array([[3, 2, 7], [0, 0, 0], [4, 4, 2]])) == (7, 6, 1, 7) and repair_totals(np.zeros((0, 3))) == (0, 0, 0, 0)
