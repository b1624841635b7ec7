"""Collision repair with walls without a GPU: the rule of include/jmid_hip.h (``jmid_repair_collisions_walls``) through its NumPy twin
``metrics.repair_collisions_host(walls=, wall_radius=)`` - against a scalar loop that takes one agent, one pair and one wall at a time,
against the twin without walls, on the constructed cases of the rule, under a perturbed ``exp`` - and the Python layer's new value."""
import math

import numpy as np
import pytest

from safe_interactive_crowdnav_amd import metrics, offline
from safe_interactive_crowdnav_amd.forecaster import (HumanTrajectoryForecasterSim, predict_batch, repair_arguments, wall_arguments,
                                                      write_configs)
from safe_interactive_crowdnav_amd.weights import JMIDWeights, NetDims

from .repair_cases import SHAPES, cluster_samples, crossing_samples
from .repair_wall_cases import DT, RADIUS, THRESHOLD, constructed, corridor, wall_cases
from .test_repair_host import DEFAULTS, bits, predicate_distance, scalar_repair


def wall_clearance(v32, p0, walls):
    """min_clear of ONE sample v32 [A, T, 2] float32 by the wall predicate's host twin (the predicate is not what this file pins)."""
    lead = None if p0 is None else np.asarray(p0, dtype=np.float32)[None]
    return float(metrics.wall_statistics_host(np.asarray(v32, dtype=np.float32)[None, None], walls, RADIUS, lead)[2][0, 0, 0])


def scalar_repair_walls(x32, p0, walls, threshold, radius, margin, tau, step, max_iter):
    """The rule word for word on ONE joint sample x32 [A, T, 2] float32 (p0 [A, 2] float32 or None), one agent, one pair and one wall at
    a time, Python floats (fp64).  -> (sample out float32, min_dist before, after, min_clear before, after, iterations, state)."""
    A, T, _ = x32.shape
    pairs = [(i, j) for i in range(A) for j in range(i + 1, A)]
    lead = None if p0 is None else [[float(c) for c in p] for p in p0]

    def min_dist(v):
        best = math.inf
        for i, j in pairs:
            for s in range(T - 1):
                d = predicate_distance(v[i][s][0] - v[j][s][0], v[i][s][1] - v[j][s][1], v[i][s + 1][0] - v[j][s + 1][0],
                                       v[i][s + 1][1] - v[j][s + 1][1])
                best = d if d < best or d != d else best
        return best

    x = [[[float(c) for c in p] for p in agent] for agent in x32]
    before, wbefore = min_dist(x), wall_clearance(x32, p0, walls)
    if before != before or wbefore != wbefore:
        return x32.copy(), before, before, wbefore, wbefore, 0, metrics.REPAIR_NAN
    if not ((A >= 2 and before < threshold) or wbefore - radius < 0):
        return x32.copy(), before, before, wbefore, wbefore, 0, metrics.REPAIR_UNTOUCHED
    m, stop, mw, wstop = threshold + margin, threshold + margin * 0.5, radius + margin, radius + margin * 0.5

    def sigmoid(z):
        e = float(np.exp(-abs(z)))
        return 1.0 / (1.0 + e) if z >= 0.0 else e / (1.0 + e)

    def closest(ax, ay, bx, by):       # the origin against the segment a -> b: (u, cx, cy, c . c)
        abx, aby = bx - ax, by - ay
        den = abx * abx + aby * aby
        u = min(max(-(ax * abx + ay * aby) / den, 0.0), 1.0) if den > 0.0 else 0.0
        cx, cy = ax + u * abx, ay + u * aby
        return u, cx, cy, cx * cx + cy * cy

    def segment(i, j, s):              # the pedestrian term's closest-point form for the pair i < j
        u, cx, cy, s2 = closest(x[i][s][0] - x[j][s][0], x[i][s][1] - x[j][s][1], x[i][s + 1][0] - x[j][s + 1][0], x[i][s + 1][1] - x[j][s + 1][1])
        d = math.sqrt(s2)
        nx, ny = (cx / d, cy / d) if d > 0.0 else (1.0, 0.0)
        return d, u, nx, ny, sigmoid((m - d) / tau)

    def point(a, i):                   # q[i] of agent a: p0 in front when it is given
        if lead is not None:
            return lead[a] if i == 0 else x[a][i - 1]
        return x[a][i]

    NP = T + (0 if lead is None else 1)

    def wall_segment(a, s, w):         # the wall term's form for the step q[s] -> q[s + 1]: (d, w_b0, w_b1, nx, ny, sigma)
        b0, b1 = point(a, s), point(a, s + 1)
        p00, p01 = (b0[0] - w[0], b0[1] - w[1]), (b0[0] - w[2], b0[1] - w[3])
        p10, p11 = (b1[0] - w[0], b1[1] - w[1]), (b1[0] - w[2], b1[1] - w[3])
        cands = []
        for k, (pa, pb) in enumerate(((p00, p01), (p10, p11), (p00, p10), (p01, p11))):
            u, cx, cy, s2 = closest(pa[0], pa[1], pb[0], pb[1])
            cands.append((s2, cx, cy, (1.0, 0.0) if k == 0 else (0.0, 1.0) if k == 1 else (1.0 - u, u)))
        best = cands[0]
        for c in cands[1:]:
            if c[0] < best[0]:         # the first one wins a tie
                best = c
        Wx, Wy, Bx, By = w[2] - w[0], w[3] - w[1], b1[0] - b0[0], b1[1] - b0[1]
        o1, o2 = Wx * p00[1] - Wy * p00[0], Wx * p10[1] - Wy * p10[0]
        o3, o4 = By * p00[0] - Bx * p00[1], By * p01[0] - Bx * p01[1]
        cross = ((o1 > 0 and o2 < 0) or (o1 < 0 and o2 > 0)) and ((o3 > 0 and o4 < 0) or (o3 < 0 and o4 > 0))
        if cross:
            best = cands[1]
        s2, cx, cy, (w0, w1) = best
        d = math.sqrt(s2)
        nx, ny = (cx / d, cy / d) if d > 0.0 else (1.0, 0.0)
        if cross:
            d, nx, ny = -d, -nx, -ny
        return d, w0, w1, nx, ny, sigmoid((mw - d) / tau)

    iters = 0
    for _ in range(max_iter):
        dmin = min([segment(i, j, s)[0] for i, j in pairs for s in range(T - 1)], default=math.inf)
        wmin = min([wall_segment(a, s, w)[0] for a in range(A) for s in range(NP - 1) for w in walls], default=math.inf)
        if dmin >= stop and wmin >= wstop:
            break
        new = [[[0.0, 0.0] for _ in range(T)] for _ in range(A)]
        for a in range(A):
            for t in range(T):
                g = [0.0, 0.0]
                for b in range(A):                       # the pedestrian partners first, ascending
                    if b == a:
                        continue
                    i, j = min(a, b), max(a, b)
                    for s, far in ((t - 1, True), (t, False)):
                        if not 0 <= s < T - 1:
                            continue
                        _, u, nx, ny, sg = segment(i, j, s)
                        w = sg * u if far else sg * (1.0 - u)
                        px, py = w * nx, w * ny
                        g = [g[0] - px, g[1] - py] if a == i else [g[0] + px, g[1] + py]
                q = t + NP - T                           # the point's index on its path
                for wall in walls:                       # then the walls ascending: the step that ends here, then the one that starts here
                    for s, far in ((q - 1, True), (q, False)):
                        if not 0 <= s < NP - 1:
                            continue
                        _, w0, w1, nx, ny, sg = wall_segment(a, s, wall)
                        w = sg * w1 if far else sg * w0
                        px, py = w * nx, w * ny
                        g = [g[0] - px, g[1] - py]
                new[a][t] = [x[a][t][0] - step * g[0], x[a][t][1] - step * g[1]]
        x = new
        iters += 1
    r32 = np.asarray(x, dtype=np.float64).astype(np.float32)
    after, wafter = min_dist([[[float(c) for c in p] for p in agent] for agent in r32]), wall_clearance(r32, p0, walls)
    if after == after and not after < threshold and wafter == wafter and not wafter - radius < 0:
        return r32, before, after, wbefore, wafter, iters, metrics.REPAIR_REPAIRED
    return x32.copy(), before, before, wbefore, wbefore, iters, metrics.REPAIR_REVERTED


def twin(pos, p0, walls, **kw):
    return metrics.repair_collisions_host(pos, THRESHOLD, p0=p0, dt=DT, walls=walls, wall_radius=RADIUS, **kw)


_TWIN = {}


def generated(name):
    """(pos, p0, walls, the twin's five outputs) of a generated case, the twin computed once."""
    if name not in _TWIN:
        pos, p0, walls = wall_cases()[name]
        _TWIN[name] = (pos, p0, walls, twin(pos, p0, walls))
    return _TWIN[name]


def assert_invariant(pos, p0, walls, out, sample, n_agents=None):
    """Every sample is either the input's bits or acceptable to both predicates' host twins."""
    fixed = sample[..., 3] == metrics.REPAIR_REPAIRED
    assert np.array_equal(bits(out[~fixed]), bits(pos[~fixed]))
    ped = metrics.collision_statistics_host(out, THRESHOLD, n_agents=n_agents)[2]
    hit = metrics.wall_statistics_host(out, walls, RADIUS, p0, n_agents=n_agents)[2]
    assert not (ped[..., 3][fixed] > 0).any() and not (hit[..., 1][fixed] > 0).any()
    assert not np.isnan(ped[..., 0][fixed]).any() and not np.isnan(hit[..., 0][fixed]).any()


@pytest.mark.parametrize("name,with_p0", [("e2a3k5t3l2", True), ("e2a3k5t3l2", False), ("a1t2k1l1", True), ("e3a3k6t4", True)])
def test_the_twin_equals_the_scalar_loop(name, with_p0):
    pos, p0, walls, _ = generated(name)
    p0 = p0 if with_p0 else None
    out, _, sample, episode, wall = twin(pos, p0, walls)
    assert episode[:, 1].sum() >= 1 and episode[:, 0].sum() > episode[:, 1].sum()       # (repaired and reverted samples both occur)
    for e in range(pos.shape[0]):
        for k in range(pos.shape[1]):
            want, before, after, wbefore, wafter, iters, state = scalar_repair_walls(pos[e, k], None if p0 is None else p0[e], walls.tolist(),
                                                                                     THRESHOLD, RADIUS, **DEFAULTS)
            assert (int(sample[e, k, 2]), int(sample[e, k, 3])) == (iters, state), (e, k)
            assert sample[e, k, :2].tolist() == [before, after] and wall[e, k].tolist() == [wbefore, wafter]
            assert np.array_equal(bits(out[e, k]), bits(want)), (e, k)       # the same operations in the same order: the same bits
        tried = sample[e, :, 3] == metrics.REPAIR_REPAIRED
        tried_all = tried | (sample[e, :, 3] == metrics.REPAIR_REVERTED)
        assert episode[e].tolist() == [int(tried_all.sum()), int(tried.sum()), int(sample[e, :, 2].max())]
    assert_invariant(pos, p0, walls, out, sample)


def test_no_walls_is_the_repair_without_walls():
    inputs = [cluster_samples(1, A, T, K, seed) for A, T, K, seed in ((2, 2, 3, 3), (3, 3, 5, 1), (5, 12, 4, 2))]
    inputs += [crossing_samples(E, A, T, K, seed, sigma, frame) for E, A, T, K, seed, sigma, frame in (SHAPES[0], SHAPES[3], SHAPES[4])]
    for n, (pos, p0) in enumerate(inputs):
        vel = np.full(pos.shape, 3.0, dtype=np.float32)
        plain = metrics.repair_collisions_host(pos, THRESHOLD, p0=p0, dt=DT, vel=vel)
        assert len(plain) == 4 and plain[3][:, 1].sum() >= 1
        empty = metrics.repair_collisions_host(pos, THRESHOLD, p0=p0, dt=DT, vel=vel, walls=np.zeros((0, 4)), wall_radius=RADIUS)
        assert len(empty) == 5 and np.all(np.isposinf(empty[4]))
        for a, b in zip(plain, empty):
            assert a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))
        if n < 3:                      # and both are the rule as it stood: the scalar loop of tests/test_repair_host.py
            for k in range(pos.shape[1]):
                want, before, after, iters, state = scalar_repair(pos[0, k], THRESHOLD, **DEFAULTS)
                assert np.array_equal(bits(empty[0][0, k]), bits(want)) and empty[2][0, k].tolist() == [before, after, iters, state]
    with pytest.raises(ValueError, match="wall_radius"):
        metrics.repair_collisions_host(pos, THRESHOLD, walls=np.zeros((0, 4)))
    with pytest.raises(ValueError, match="without walls"):
        metrics.repair_collisions_host(pos, THRESHOLD, wall_radius=RADIUS)
    # a wall far from everybody changes no position either (its terms underflow to nothing), and reports its clearance
    pos, p0 = inputs[1]
    far = twin(pos, p0, np.array([[-50.0, 40.0, 50.0, 40.0]]))
    plain = metrics.repair_collisions_host(pos, THRESHOLD, p0=p0, dt=DT)
    assert np.array_equal(bits(far[0]), bits(plain[0])) and np.array_equal(far[2], plain[2]) and np.all(far[4] > 30.0)


# the expected state of every constructed case (tests/repair_wall_cases.py), fixed after the twin was seen to reach it
EXPECTED = {"brush": 1, "brush_p0": 1, "pair": 1, "cross": 1, "cross_back": 1, "tip": 1, "point": 1, "p0_inside": 2}


@pytest.mark.parametrize("name", sorted(EXPECTED))
def test_constructed_cases(name):
    pos, p0, walls = constructed()[name]
    out, _, sample, episode, wall = twin(pos, p0, walls)
    assert int(sample[0, 0, 3]) == EXPECTED[name] and (wall[0, 0, 0] - RADIUS < 0) == (name != "pair")     # (the pair comes in clear of the wall)
    assert_invariant(pos, p0, walls, out, sample)
    want = scalar_repair_walls(pos[0, 0], None if p0 is None else p0[0], walls.tolist(), THRESHOLD, RADIUS, **DEFAULTS)
    assert np.array_equal(bits(out[0, 0]), bits(want[0])) and sample[0, 0].tolist() == [want[1], want[2], want[5], want[6]]
    assert wall[0, 0].tolist() == [want[3], want[4]]
    if EXPECTED[name] == 1:
        assert wall[0, 0, 1] >= RADIUS and sample[0, 0, 2] < DEFAULTS["max_iter"] and episode.tolist() == [[1, 1, int(sample[0, 0, 2])]]
        assert wall[0, 0, 1] == metrics.wall_statistics_host(out, walls, RADIUS, p0)[2][0, 0, 0]
    else:                              # the present position itself is inside the radius: nothing can be done, the input bits come back
        assert np.array_equal(bits(out), bits(pos)) and wall[0, 0, 1] == wall[0, 0, 0] and episode.tolist() == [[1, 0, DEFAULTS["max_iter"]]]
    if name == "pair":                 # both predicates hold now; the repair that knows no wall pushes a pedestrian into it
        assert sample[0, 0, 0] < THRESHOLD <= sample[0, 0, 1]
        blind = metrics.repair_collisions_host(pos, THRESHOLD)
        assert blind[2][0, 0, 3] == metrics.REPAIR_REPAIRED
        assert metrics.wall_statistics_host(pos, walls, RADIUS)[2][0, 0, 1] == 0 and metrics.wall_statistics_host(blind[0], walls, RADIUS)[2][0, 0, 1] >= 1
    if name in ("cross", "cross_back"):        # the crossing's distance is a cancellation: (almost) nothing before, the radius after
        assert wall[0, 0, 0] < 1e-12
    if name == "brush":                # a single agent IS a candidate with walls and is not without them
        assert metrics.repair_collisions_host(pos, THRESHOLD)[2][0, 0, 3] == metrics.REPAIR_UNTOUCHED
        assert np.all(out[0, 0, 0, :, 1] > pos[0, 0, 0, :, 1]) and np.array_equal(out[0, 0, 0, :, 0], pos[0, 0, 0, :, 0])


def test_nan_samples_and_the_cap():
    pos, p0, walls, _ = generated("e2a3k5t3l2")
    bad = pos.copy()
    bad[1, 4, 2, 1, 0] = np.nan
    out, _, sample, episode, wall = twin(bad, p0, walls)
    assert sample[1, 4, 3] == metrics.REPAIR_NAN and np.isnan(sample[1, 4, :2]).all() and np.isnan(wall[1, 4]).all()
    assert np.array_equal(bits(out[1, 4]), bits(bad[1, 4])) and sample[1, 4, 2] == 0
    # a NaN present position spoils the wall minimum alone: state 3 for every sample of the episode
    bad0 = p0.copy()
    bad0[0, 1, 1] = np.nan
    out, _, sample, episode, wall = twin(pos, bad0, walls)
    assert np.all(sample[0, :, 3] == metrics.REPAIR_NAN) and np.isnan(wall[0]).all() and not np.isnan(sample[0, :, 0]).any()
    assert np.array_equal(bits(out[0]), bits(pos[0])) and episode[0].tolist() == [0, 0, 0]
    for cap in (0, 1):                 # the identity plus the flags; a cap too small to finish
        out, _, sample, episode, wall = twin(pos, p0, walls, max_iter=cap)
        tried = sample[..., 3] > 0
        assert np.array_equal(bits(out), bits(pos)) and np.all(sample[..., 3][tried] == metrics.REPAIR_REVERTED) and tried.sum() == 9
        assert np.all(sample[..., 2][tried] == cap) and episode.tolist() == [[int(tried[0].sum()), 0, cap], [int(tried[1].sum()), 0, cap]]
        assert np.array_equal(wall[..., 0], wall[..., 1]) and np.array_equal(sample[..., 0], sample[..., 1])


def test_padded_counts_equal_the_compacted_episodes():
    pos, p0, walls, _ = generated("e3a3k6t4")
    counts = np.array([3, 1, 2])
    padded, lead = pos.copy(), p0.copy()
    for e, n in enumerate(counts):
        padded[e, :, n:], lead[e, n:] = np.nan, np.nan
    vel = np.full(pos.shape, 7.0, dtype=np.float32)
    out, vel_out, sample, episode, wall = twin(padded, lead, walls, n_agents=counts, vel=vel)
    assert episode[:, 1].min() >= 1                                         # the single agent of episode 1 is repaired too
    for e, n in enumerate(counts):
        alone = twin(np.ascontiguousarray(pos[e:e + 1, :, :n]), np.ascontiguousarray(p0[e:e + 1, :n]), walls,
                     vel=np.ascontiguousarray(vel[e:e + 1, :, :n]))
        assert np.array_equal(bits(out[e, :, :n]), bits(alone[0][0])) and np.isnan(out[e, :, n:]).all()
        assert np.array_equal(bits(vel_out[e, :, :n]), bits(alone[1][0])) and np.all(vel_out[e, :, n:] == 7.0)
        assert np.array_equal(sample[e], alone[2][0]) and np.array_equal(episode[e], alone[3][0]) and np.array_equal(wall[e], alone[4][0])
    assert_invariant(padded, lead, walls, out, sample, n_agents=counts)


def test_velocities_and_the_invariant_on_the_generated_cases():
    for name in wall_cases():
        pos, p0, walls, (out, _, sample, episode, wall) = generated(name)
        assert_invariant(pos, p0, walls, out, sample)
        causes = metrics.repair_causes(sample, wall, THRESHOLD, RADIUS)
        assert causes["candidates"] == episode[:, 0].sum() and causes["repaired"] == episode[:, 1].sum() >= 1, name
        assert causes["candidates"] == causes["pedestrians"] + causes["walls"] - causes["both"]
    pos, p0, walls, (out, _, sample, _, _) = generated("e5a3k4t4")
    prev = np.concatenate([np.broadcast_to(p0[:, None, :, None], pos[:, :, :, :1].shape), pos[:, :, :, :-1]], axis=3)
    vel = ((pos - prev) / np.float32(DT)).astype(np.float32)
    again = twin(pos, p0, walls, vel=vel)
    fixed = sample[..., 3] == metrics.REPAIR_REPAIRED
    assert np.array_equal(bits(again[0]), bits(out)) and np.array_equal(bits(again[1][~fixed]), bits(vel[~fixed]))
    prev = np.concatenate([np.broadcast_to(p0[:, None, :, None], out[:, :, :, :1].shape), out[:, :, :, :-1]], axis=3).astype(np.float64)
    assert np.array_equal(bits(again[1][fixed]), bits(((out.astype(np.float64) - prev) / DT).astype(np.float32)[fixed]))


@pytest.mark.parametrize("ulps", [-8, -2, 2, 8])
def test_ulps_of_exp_move_no_state_no_count_and_no_bit(ulps):
    """What separates the kernel from the twin is the device's exp: a few fp64 ulps of it must not show in any decision on the inputs
    the device test compares, nor in any bit of the fp32 output."""
    def exp(v):
        e = np.exp(v)
        for _ in range(abs(ulps)):
            e = np.nextafter(e, np.inf if ulps > 0 else -np.inf)
        return e
    cases = [(name,) + generated(name) for name in wall_cases()]
    cases += [(name, pos, p0, walls, twin(pos, p0, walls)) for name, (pos, p0, walls) in constructed().items()]
    for name, pos, p0, walls, (out, _, sample, episode, wall) in cases:
        out2, _, sample2, episode2, wall2 = twin(pos, p0, walls, exp=exp)
        assert np.array_equal(sample2[..., 2:], sample[..., 2:]) and np.array_equal(episode2, episode), name
        assert np.array_equal(bits(out2), bits(out)) and np.array_equal(wall2, wall), name


def test_python_surface(tmp_path):
    env, ypath = write_configs(str(tmp_path), joint=True, ctx_dim=32, N=3, K=6, k_ret=3, H=4, step=2)
    weights = JMIDWeights.from_seed(NetDims(ctx_dim=32), 1)
    walls = np.array([[[0.0, 0.0], [1.0, 0.0]]])
    with pytest.raises(ValueError, match="needs static_obstacles"):
        HumanTrajectoryForecasterSim(env, ypath, weights=weights, constraint_type="opt_softplus_walls")
    with pytest.raises(ValueError, match="wall_radius"):
        HumanTrajectoryForecasterSim(env, ypath, weights=weights, constraint_type="opt_softplus_walls", static_obstacles=walls)
    with pytest.raises(ValueError, match="unknown constraint_type"):
        HumanTrajectoryForecasterSim(env, ypath, weights=weights, constraint_type="opt_relu_walls", static_obstacles=walls, wall_radius=0.3)
    # the value without walls keeps its refusal, and now says where the walls are
    with pytest.raises(ValueError, match="walls are not in the repair's objective.*opt_softplus_walls"):
        repair_arguments("opt_softplus", None, walls, 0.3)
    with pytest.raises(ValueError, match="non-finite"):
        repair_arguments("opt_softplus_walls", None, np.array([[0.0, 0.0, np.inf, 0.0]]), 0.3)
    with pytest.raises(ValueError, match="wall_radius must be finite"):
        repair_arguments("opt_softplus_walls", None, walls, -0.1)
    with pytest.raises(ValueError, match="more than 64"):
        repair_arguments("opt_softplus_walls", None, corridor(65, 1.0), 0.3)
    fix = repair_arguments("opt_softplus_walls", {"tau": 0.01}, walls, 0.3)
    assert sorted(fix) == ["tau", "wall_radius", "walls"] and fix["wall_radius"] == 0.3 and fix["walls"].tolist() == [[0.0, 0.0, 1.0, 0.0]]
    assert repair_arguments("opt_softplus", {"tau": 0.01}) == {"tau": 0.01} and repair_arguments(None, None, walls, 0.3) is None
    # without a redraw loop the walls go to the repair alone; with one, to both
    assert wall_arguments(walls, 0.3, 0, True) == {} and sorted(wall_arguments(walls, 0.3, 2, True)) == ["wall_radius", "walls"]
    with pytest.raises(ValueError, match="needs collision-free sampling"):
        wall_arguments(walls, 0.3, 0)
    ctx, p0 = np.zeros((3, 32), np.float32), np.zeros((3, 2), np.float32)
    with pytest.raises(ValueError, match="with_constraints=True"):
        offline.sample(None, 4, ctx, 5, True, constraint_type="opt_softplus_walls", static_obstacles=walls, wall_radius=0.3, _integrate=(p0, 0.25))
    with pytest.raises(ValueError, match="needs static_obstacles"):
        offline.generate(None, ctx, p0, 0.25, 4, 5, True, with_constraints=True, constraint_type="opt_softplus_walls")
    hum, rob = np.zeros((2, 6, 3, 2)), np.zeros((2, 6, 2))
    kw = dict(num_samples=6, num_ret_samples=3, horizon=4, time_step=0.25)
    with pytest.raises(ValueError, match="needs static_obstacles"):
        predict_batch(None, hum, rob, [0, 1], constraint_type="opt_softplus_walls", **kw)
    with pytest.raises(ValueError, match="unknown constraint_type"):
        predict_batch(None, hum, rob, [0, 1], constraint_type="softplus_walls", static_obstacles=walls, wall_radius=0.3, **kw)
