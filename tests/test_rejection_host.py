"""Collision-free sampling without a GPU: the pairing twin (``metrics.fill_slots``) against a scalar loop, the route under the flag, the
refusals of the Python layer, and the reference's counts and sentence.  tests/test_gpu_rejection.py holds the device loop to the twin."""
import itertools

import numpy as np
import pytest

from safe_interactive_crowdnav_amd import metrics, offline
from safe_interactive_crowdnav_amd.forecaster import HumanTrajectoryForecasterSim, plan_route, predict_batch, write_configs
from safe_interactive_crowdnav_amd.weights import JMIDWeights, NetDims


def brute_force(table):
    """The rule of include/jmid_hip.h, one slot and one candidate at a time.  table [rounds + 1][K] bool."""
    K = len(table[0])
    holds = [(0, s) for s in range(K)]
    bad = [s for s in range(K) if not table[0][s]]
    n_bad0, fixed, last = len(bad), 0, 0
    for j in range(1, len(table)):
        if not bad:
            break
        last = j
        good = [c for c in range(K) if table[j][c]]
        while bad and good:              # the smallest bad slot takes the smallest acceptable candidate
            s, c = bad.pop(0), good.pop(0)
            holds[s] = (j, c)
            fixed += 1
    slots = np.array([[j, c, int(s in bad)] for s, (j, c) in enumerate(holds)], dtype=np.int32)
    return slots, np.array([n_bad0, fixed, last], dtype=np.int32)


def check(table):
    table = [np.asarray(r, dtype=bool) for r in table]
    slots, episode = metrics.fill_slots(table)
    want_slots, want_episode = brute_force(table)
    assert slots.dtype == np.int32 and episode.dtype == np.int32
    np.testing.assert_array_equal(slots, want_slots)
    np.testing.assert_array_equal(episode, want_episode)
    return slots, episode


@pytest.mark.parametrize("K", [1, 5, 300])
@pytest.mark.parametrize("rounds", [0, 1, 3, 6])
@pytest.mark.parametrize("p_ok", [0.1, 0.5, 0.9])
def test_fill_slots_equals_the_scalar_loop(K, rounds, p_ok):
    rng = np.random.default_rng(1000 * K + 10 * rounds + int(10 * p_ok))
    for _ in range(20):
        check(rng.random((rounds + 1, K)) < p_ok)


def test_fill_slots_named_cases():
    t, f = True, False
    # more acceptable candidates than bad slots: the smallest candidates are taken, the rest discarded
    slots, ep = check([[t, f, t, f, t], [f, t, t, t, t]])
    assert slots.tolist() == [[0, 0, 0], [1, 1, 0], [0, 2, 0], [1, 2, 0], [0, 4, 0]] and ep.tolist() == [2, 2, 1]
    # fewer: the smallest bad slots are filled, the others wait for the next round
    slots, ep = check([[f, f, f, t, f], [f, f, t, f, f], [t, f, f, f, t], [f, f, f, f, f]])
    assert slots.tolist() == [[1, 2, 0], [2, 0, 0], [2, 4, 0], [0, 3, 0], [0, 4, 1]] and ep.tolist() == [4, 3, 3]
    # a round with none acceptable changes nothing but the round counter
    slots, ep = check([[f, t], [f, f], [t, t]])
    assert slots.tolist() == [[2, 0, 0], [0, 1, 0]] and ep.tolist() == [1, 1, 2]
    # nothing bad at round 0: never rerun, whatever the later rows say
    slots, ep = check([[t, t, t], [f, f, f], [t, t, t]])
    assert slots.tolist() == [[0, 0, 0], [0, 1, 0], [0, 2, 0]] and ep.tolist() == [0, 0, 0]
    # max_rounds = 0: the flags and nothing else
    slots, ep = check([[f, t, f]])
    assert slots.tolist() == [[0, 0, 1], [0, 1, 0], [0, 2, 1]] and ep.tolist() == [2, 0, 0]
    # K = 1, the offline form: a sample is redrawn until it is acceptable
    slots, ep = check([[f], [f], [t], [f]])
    assert slots.tolist() == [[2, 0, 0]] and ep.tolist() == [1, 1, 2]
    # the callable form asks only for the rounds it needs
    asked = []

    def ask(j):
        asked.append(j)
        return [[f, t], [t, f]][j] if j < 2 else None

    slots, ep = metrics.fill_slots(ask)
    assert asked == [0, 1] and slots.tolist() == [[1, 0, 0], [0, 1, 0]] and ep.tolist() == [1, 1, 1]


def test_plan_route_under_the_flag():
    flags = dict(k=(5, 20), A=(3, 40), device_topk=(True, False), device_scene=(False, True), device_frames=(False, True),
                 check=(False, True), short=(False, True), frames=(True, False), batch=(False, True), padded=(False, True),
                 resident=(False, True), tracks=(False, True))
    n_chain = 0
    for values in itertools.product(*flags.values()):
        kw = dict(zip(flags, values), K=20, H=8)
        plain = plan_route(**kw)
        assert plan_route(**kw, collision_free=False) == plain              # every existing combination stays as it is
        got = plan_route(**kw, collision_free=True)
        assert got.run == "staged" and got.scene == plain.scene and got.rank == plain.rank
        n_chain += plain.run == "chain"
    assert n_chain > 0
    # the staged route with the ranking on the resident accepted set; the host twin beyond the top-k limits; nothing to rank at k == K
    assert plan_route(k=5, K=20, A=3, H=8, collision_free=True) == ("host", "staged", "device_resident")
    assert plan_route(k=5, K=20, A=3, H=8, device_frames=True, collision_free=True) == ("stamped", "staged", "device_resident")
    assert plan_route(k=5, K=20, A=40, H=8, collision_free=True).rank == "host"
    assert plan_route(k=20, K=20, A=3, H=8, collision_free=True).rank == "none"


def test_python_refusals(tmp_path):
    env, ypath = write_configs(str(tmp_path), joint=True, ctx_dim=32, N=3, K=6, k_ret=3, H=4, step=2)
    weights = JMIDWeights.from_seed(NetDims(ctx_dim=32), 1)
    for rng in ("cpu", "cuda", "auto"):      # a redraw is a draw number of the counter generator: rng_compat="device" only
        with pytest.raises(ValueError, match="rng_compat='device'"):
            HumanTrajectoryForecasterSim(env, ypath, weights=weights, rng_compat=rng, collision_free_rounds=2)
    with pytest.raises(ValueError, match="collision_free_rounds"):
        HumanTrajectoryForecasterSim(env, ypath, weights=weights, rng_compat="device", collision_free_rounds=65)
    ctx, p0 = np.zeros((3, 32), np.float32), np.zeros((3, 2), np.float32)
    ok = dict(bestof=True, sampling="ddim", step=2, seed=1, with_constraints=True, _integrate=(p0, 0.25))
    for bad, word in ((dict(sampling="ddpm"), "ddim"), (dict(_integrate=None), "positions"), (dict(seed=None), "seed"), (dict(bestof=False), "bestof")):
        with pytest.raises(ValueError, match=word):
            offline.sample(None, 4, ctx, 5, **dict(ok, **bad))
    with pytest.raises(ValueError, match="ddim"):
        offline.generate(None, ctx, p0, 0.25, 4, 5, True, sampling="ddpm", step=2, seed=1, with_constraints=True)
    hum, rob = np.zeros((2, 6, 3, 2)), np.zeros((2, 6, 2))
    kw = dict(num_samples=6, num_ret_samples=3, horizon=4, time_step=0.25, collision_free_rounds=2)
    for padded in (True, "resident"):
        with pytest.raises(ValueError, match="padded"):
            predict_batch(None, hum, rob, [0, 1], noise="device", padded=padded, **kw)
    with pytest.raises(ValueError, match="noise='device'"):
        predict_batch(None, hum, rob, [0, 1], **kw)


def test_rejection_totals_and_the_sentence(capsys):
    episodes = np.array([[3, 2, 2], [0, 0, 0], [5, 5, 1], [1, 0, 3]], dtype=np.int32)
    assert metrics.rejection_totals(episodes) == (3, 9, 7)
    assert metrics.rejection_totals(episodes[1:2]) == (0, 0, 0)
    assert metrics.rejection_totals(np.zeros((0, 3), np.int32)) == (0, 0, 0)
    agent, scene = np.ones((2, 3, 10)), np.ones((2, 6))
    plain = metrics.summarise(agent, scene)
    assert capsys.readouterr().out == "" and "rejection_fixed" not in plain
    out = metrics.summarise(agent, scene, rejection=metrics.rejection_totals(episodes))
    assert capsys.readouterr().out == "Rejection sampling fixed 7 samples out of 9 samples with collisions\n"       # MID/mid.py:1048
    assert (out["rejection_num_iter"], out["rejection_colliding"], out["rejection_fixed"]) == (3, 9, 7)
    assert {k: v for k, v in out.items() if not k.startswith("rejection_")} == plain
