"""The host side of collision-free sampling on padded batches: the host twins of the padded statistics (``metrics.collision_statistics_host``
/ ``metrics.wall_statistics_host`` with ``n_agents``) against their definition - the plain twin on every compacted episode -, the
refusals of ``predict_batch(collision_free_padded=True)``, and the engine entries that keyword issues (the recording stand-in of
tests/test_forecaster_routes.py).  No library, no device."""
import numpy as np
import pytest

from safe_interactive_crowdnav_amd import forecaster as FC, metrics
from tests.test_forecaster_routes import THREE_COUNTS_SEED, WEIGHTS, FakeEngine, batch_inputs

E, A, K, T = 5, 4, 6, 3
COUNTS = np.array([4, 1, 2, 3, 4])
THRESHOLD, RADIUS = 0.8, 0.3
WALLS = np.array([[0.5, -3.0, 0.5, 3.0], [-2.0, 1.0, 2.0, 1.2]])


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def positions(fill, real_bad=False):
    g = np.random.default_rng(3)
    pos = g.normal(size=(E, K, A, T, 2)).astype(np.float32)
    p0 = g.normal(size=(E, A, 2)).astype(np.float32)
    if real_bad:
        pos[0, 1, 2, 1, 0] = np.nan          # a REAL agent of a full episode
        pos[3, 4, 0, 2, 1] = np.inf          # ... and of a padded one
    for e, n in enumerate(COUNTS):
        pos[e, :, n:], p0[e, n:] = fill, fill
    return pos, p0


@pytest.mark.parametrize("real_bad", [False, True], ids=["finite", "real_nonfinite"])
@pytest.mark.parametrize("fill", [np.nan, np.inf, 1e30, 0.0], ids=["nan", "inf", "1e30", "zero"])
def test_collision_twin_is_the_plain_twin_on_every_compacted_episode(fill, real_bad):
    pos, _ = positions(fill, real_bad)
    pair, agent, sample, scene = metrics.collision_statistics_host(pos, THRESHOLD, n_agents=COUNTS)
    assert pair.shape == (E, K, A * (A - 1) // 2) and agent.shape == (E, K, A) and sample.shape == (E, K, 4) and scene.shape == (E, 5)
    for e, n in enumerate(COUNTS):
        pr, ag, sm, sc = metrics.collision_statistics_host(pos[e:e + 1, :, :n], THRESHOLD)
        i, j = np.triu_indices(n, 1)
        at_A = metrics.pair_index(i, j, A)
        assert (np.diff(at_A) > 0).all()                               # the (i, j) map is monotone: the tie rule carries over
        assert same_bits(pair[e][:, at_A], pr[0])
        rest = np.setdiff1d(np.arange(pair.shape[-1]), at_A)
        assert np.isnan(pair[e][:, rest]).all()                        # a pair with a padded agent
        assert same_bits(agent[e, :, :n], ag[0]) and not agent[e, :, n:].any()
        assert same_bits(sample[e][:, [0, 2, 3]], sm[0][:, [0, 2, 3]]) and same_bits(scene[e], sc[0])
        for s in range(K):                                             # closest_pair: the same pair, named at A
            c = int(sm[0, s, 1])
            assert sample[e, s, 1] == (-1 if c < 0 else at_A[c])
    # counts 1 and A
    assert np.isinf(sample[1, :, 0]).all() and (sample[1, :, 1:] == [-1, 0, 0]).all() and np.isnan(pair[1]).all()
    assert same_bits(pair[4], metrics.collision_statistics_host(pos[4:5], THRESHOLD)[0][0])
    # a non-finite REAL position is still NaN; a non-finite PADDED one is ignored
    if real_bad:
        assert np.isnan(sample[0, 1, 0]) and sample[0, 1, 1] == -1 and np.isnan(sample[3, 4, 0]) and np.isnan(scene[[0, 3], 2]).all()
    else:
        assert not np.isnan(sample[..., 0]).any() and not np.isnan(scene[[0, 2, 3, 4]]).any()
    # both outcomes occur among the real pairs
    real = np.isfinite(pair)
    assert (pair[real] < THRESHOLD).any() and (pair[real] >= THRESHOLD).any()
    # agent_collision_rate is over K * n_e
    assert np.allclose(scene[:, 1], agent.reshape(E, -1).sum(axis=1) / (K * COUNTS), rtol=0, atol=0)


@pytest.mark.parametrize("with_p0", [False, True], ids=["no_p0", "p0"])
@pytest.mark.parametrize("real_bad", [False, True], ids=["finite", "real_nonfinite"])
@pytest.mark.parametrize("fill", [np.nan, np.inf, 1e30], ids=["nan", "inf", "1e30"])
def test_wall_twin_is_the_plain_twin_on_every_compacted_episode(fill, real_bad, with_p0):
    pos, p0 = positions(fill, real_bad)
    if not with_p0:
        p0 = None
    dist, agent, sample, scene = metrics.wall_statistics_host(pos, WALLS, RADIUS, p0=p0, n_agents=COUNTS)
    assert dist.shape == (E, K, A, 2) and agent.shape == (E, K, A) and sample.shape == (E, K, 3) and scene.shape == (E, 5)
    for e, n in enumerate(COUNTS):
        d, ag, sm, sc = metrics.wall_statistics_host(pos[e:e + 1, :, :n], WALLS, RADIUS, p0=None if p0 is None else p0[e:e + 1, :n])
        assert same_bits(dist[e, :, :n], d[0]) and np.isnan(dist[e, :, n:]).all()
        assert same_bits(agent[e, :, :n], ag[0]) and not agent[e, :, n:].any()
        assert same_bits(sample[e], sm[0]) and same_bits(scene[e], sc[0])
    if real_bad:
        assert np.isnan(sample[0, 1, 0]) and np.isnan(sample[3, 4, 0])
    else:
        assert not np.isnan(sample).any() and not np.isnan(scene).any()
    real = np.isfinite(dist)
    assert (dist[real] < RADIUS).any() and (dist[real] >= RADIUS).any()
    assert np.allclose(scene[:, 1], agent.reshape(E, -1).sum(axis=1) / (K * COUNTS), rtol=0, atol=0)


def test_twins_refuse_bad_counts():
    pos, p0 = positions(np.nan)
    for bad in ([4, 0, 2, 3, 4], [4, 1, 2, 3, 5], [4, 1, 2]):
        with pytest.raises(ValueError, match="n_agents"):
            metrics.collision_statistics_host(pos, THRESHOLD, n_agents=bad)
        with pytest.raises(ValueError, match="n_agents"):
            metrics.wall_statistics_host(pos, WALLS, RADIUS, p0=p0, n_agents=bad)


# ------------------------------------------------------------------------------------------------------------- predict_batch
KW = dict(num_samples=8, num_ret_samples=3, horizon=6, time_step=0.25, precision="f16mx")


def test_predict_batch_refusals():
    hum, rob = batch_inputs(THREE_COUNTS_SEED)
    with pytest.raises(ValueError, match="collision_free_rounds"):
        FC.predict_batch(None, hum, rob, range(6), noise="device", collision_free_padded=True, **KW)
    with pytest.raises(ValueError, match="noise='device'"):
        FC.predict_batch(None, hum, rob, range(6), collision_free_rounds=2, collision_free_padded=True, **KW)
    for padded in (True, "resident"):
        with pytest.raises(ValueError, match="padded"):
            FC.predict_batch(None, hum, rob, range(6), noise="device", collision_free_rounds=2, collision_free_padded=True, padded=padded, **KW)


@pytest.mark.parametrize("kw,trace", [
    (dict(), "encode denoise_reject(padded)(nopos)[f16mx] topk(resident)(padded)"),
    (dict(device_topk=False), "encode denoise_reject(padded)[f16mx]"),
    (dict(num_ret_samples=8), "encode denoise_reject(padded)[f16mx]"),
    (dict(static_obstacles=WALLS, wall_radius=0.3), "encode denoise_reject(padded)(walls)(nopos)[f16mx] topk(resident)(padded)"),
    (dict(device_scene=True), "build_scene scene_arrays encode denoise_reject(padded)(nopos)[f16mx] topk(resident)(padded)"),
    (dict(device_frames=True), "build_scene build_scene scene_arrays encode denoise_reject(padded)(nopos)[f16mx] topk(resident)(padded)"),
])
def test_the_keyword_issues_one_encode_one_loop_one_ranking(kw, trace):
    hum, rob = batch_inputs(THREE_COUNTS_SEED)
    eng = FakeEngine(WEIGHTS)
    stats = {}
    args = dict(KW, noise="device", seed=5, collision_free_rounds=2, collision_free_padded=True, stats=stats)
    args.update(kw)
    fc, lw, inc = FC.predict_batch(eng, hum, rob, range(6), **args)
    counts = inc.sum(axis=1)
    assert len(set(counts.tolist())) == 3 and counts.min() >= 1, counts            # a three-count batch, nobody's cluster empty
    k = args["num_ret_samples"]
    assert fc.shape == (6, 6, k, 7, 2) and lw.shape == (6, 6, k) and fc.dtype == lw.dtype == np.float64
    assert " ".join(eng.trace) == trace
    assert stats["episodes"].shape == (6, 3) and stats["slots"].shape == (6, 8, 3) and stats["cause"].shape == (6, 2)
    # ... against one loop per count without it
    grouped = FakeEngine(WEIGHTS)
    FC.predict_batch(grouped, hum, rob, range(6), **dict(args, collision_free_padded=False))
    assert sum(t.startswith("denoise_reject") for t in grouped.trace) == 3 and not any("(padded)" in t for t in grouped.trace)


def test_an_empty_cluster_takes_the_count_groups():
    """A batch with an empty cluster has no padded form (a count must be at least 1): the keyword changes nothing about it - the same
    entries in the same order and the same outcome as without the keyword, whatever the count groups do with such a batch (on the host
    route they do not take one today: the group of count 0 has nothing to encode)."""
    hum, rob = batch_inputs(THREE_COUNTS_SEED)
    ff = np.zeros((6, 7), np.int32)
    ff[0, 1:] = 5                             # episode 0: every pedestrian has one frame - no ego row, an empty cluster
    assert FC.SC.build_scenes_batched(hum, rob, 0.25, horizon=6, first_frame=ff)["in_cluster"].sum(axis=1).tolist() == [0, 2, 4, 2, 2, 2]
    args = dict(KW, noise="device", seed=5, collision_free_rounds=2, first_frame=ff)

    def outcome(**kw):
        eng = FakeEngine(WEIGHTS)
        try:
            out = FC.predict_batch(eng, hum, rob, range(6), **args, **kw)
        except ValueError as err:
            out = str(err)
        return eng.trace, out

    with_kw, without = outcome(collision_free_padded=True), outcome()
    assert with_kw[0] == without[0] and with_kw[0] and not any("(padded)" in t for t in with_kw[0])
    assert type(with_kw[1]) is type(without[1])
    if isinstance(without[1], str):
        assert with_kw[1] == without[1]
    else:
        assert all(same_bits(x, y) for x, y in zip(with_kw[1], without[1]))
