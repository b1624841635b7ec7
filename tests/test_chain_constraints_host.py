"""Constraints in the one-entry chains, the part that needs no device: the route table with ``chain_constraints``, the validation of the
``engine.ChainConstraints`` value, and the refusals of the forecaster and ``predict_batch``."""
import itertools

import numpy as np
import pytest

from safe_interactive_crowdnav_amd.engine import ChainConstraints, ChainReport, Guidance, chain_constraint_arguments
from safe_interactive_crowdnav_amd.forecaster import (HumanTrajectoryForecasterSim, chain_constraints, constraint_route_arguments, plan_route,
                                                      predict_batch, sampling_constraints, write_configs)
from safe_interactive_crowdnav_amd.schedule import guidance_weights
from safe_interactive_crowdnav_amd.weights import JMIDWeights, NetDims

# the flag product tests/test_repair_host.py sweeps
FLAGS = dict(k=(5, 20), A=(3, 40), device_topk=(True, False), device_scene=(False, True), device_frames=(False, True),
             check=(False, True), short=(False, True), frames=(True, False), batch=(False, True), padded=(False, True),
             resident=(False, True), tracks=(False, True), collision_free=(False, True))
WALLS = np.array([[0.0, 0.0, 1.0, 0.0], [2.0, -1.0, 2.0, 1.0]])


def test_route_table_with_and_without_chain_constraints():
    chains = 0
    for values in itertools.product(*FLAGS.values()):
        kw = dict(zip(FLAGS, values), K=20, H=8)
        plain = plan_route(**kw)
        for repair, guidance in itertools.product((False, True), repeat=2):
            # False: every answer is today's
            assert plan_route(**kw, repair=repair, guidance=guidance, chain_constraints=False) == plan_route(**kw, repair=repair, guidance=guidance)
            # True: the run is the unconstrained call's, whatever the constraints; the scene and the ranking never move
            route = plan_route(**kw, repair=repair, guidance=guidance, chain_constraints=True)
            assert route == plain
            if kw["collision_free"] or kw["check"]:
                assert route.run == "staged"
            chains += route.run == "chain" and (repair or guidance)
    assert chains > 0
    assert plan_route(k=5, K=20, A=3, H=8, repair=True, guidance=True, chain_constraints=True) == ("host", "chain", "device_resident")
    assert plan_route(k=5, K=20, A=3, H=8, repair=True, guidance=True) == ("host", "staged", "device_resident")
    assert plan_route(k=5, K=20, A=3, H=8, repair=True, collision_free=True, chain_constraints=True).run == "staged"
    assert plan_route(k=5, K=20, A=3, H=8, guidance=True, check=True, chain_constraints=True).run == "staged"


def test_constraints_value_validation():
    w = guidance_weights(0.02, 2)
    guide = Guidance(0.2, weights=w)
    args = chain_constraint_arguments(ChainConstraints(0.2, guide, {}), 2)
    assert args[0] == 0.2 and np.array_equal(args[1], w) and args[2:6] == (4, 0.02, 0.005, 0) and args[6:12] == (1, 0.02, 0.005, 0.02, 32, 0)
    assert args[12] == 0 and args[13].shape == (0, 4) and args[14] == 0.0
    # each mechanism alone, and neither
    assert chain_constraint_arguments(ChainConstraints(0.2, guide, None), 2)[6] == 0
    off = chain_constraint_arguments(ChainConstraints(0.3, None, {"tau": 0.01, "max_iter": 7}), 2)
    assert off[1] is None and off[6:11] == (1, 0.02, 0.01, 0.02, 7)
    none = chain_constraint_arguments(ChainConstraints(0.2), 2)
    assert none[1] is None and none[6] == 0
    # walls: for the guidance, the repair, or both - the same ones
    gw = Guidance(0.2, weights=w, walls=WALLS.reshape(2, 2, 2), wall_radius=0.3)
    both = chain_constraint_arguments(ChainConstraints(0.2, gw, {"walls": WALLS, "wall_radius": 0.3}), 2)
    assert both[5] == 1 and both[11] == 1 and both[12] == 2 and np.array_equal(both[13], WALLS) and both[14] == 0.3
    only_repair = chain_constraint_arguments(ChainConstraints(0.2, guide, {"walls": WALLS, "wall_radius": 0.3}), 2)
    assert only_repair[5] == 0 and only_repair[11] == 1 and only_repair[12] == 2
    bad = [
        (ChainConstraints(0.2, Guidance(0.3, weights=w), None), "one threshold"),
        (ChainConstraints(-1.0), "threshold"),
        (ChainConstraints(float("nan")), "threshold"),
        (ChainConstraints(0.2, Guidance(0.2), None), "needs weights"),
        (ChainConstraints(0.2, Guidance(0.2, weights=[0.02] * 3), None), "one weight per step-table entry"),
        (ChainConstraints(0.2, Guidance(0.2, weights=w, walls=WALLS), None), "go together"),
        (ChainConstraints(0.2, None, {"walls": WALLS}), "go together"),
        (ChainConstraints(0.2, None, {"rounds": 3}), "unknown repair options"),
        (ChainConstraints(0.2, gw, {"walls": WALLS + 1.0, "wall_radius": 0.3}), "the same walls"),
        (ChainConstraints(0.2, gw, {"walls": WALLS, "wall_radius": 0.4}), "the same walls"),
        (ChainConstraints(0.2, None, {"walls": np.zeros((0, 4)), "wall_radius": 0.3}), "there are none"),
    ]
    for cons, word in bad:
        with pytest.raises(ValueError, match=word):
            chain_constraint_arguments(cons, 2)
    with pytest.raises(TypeError):
        chain_constraint_arguments({"threshold": 0.2}, 2)
    assert ChainReport() == (None, None, None, None)


def test_constraints_of_the_forecasters_keywords():
    assert chain_constraints(sampling_constraints()) is None
    limits = sampling_constraints(threshold=0.5, constraint_type="opt_softplus_walls", static_obstacles=WALLS, wall_radius=0.3,
                                  repair_options={"tau": 0.01}, guidance={"walls": True}, step=2)
    cons = chain_constraints(limits)
    assert cons.threshold == 0.5 and cons.guidance is limits.guidance and cons.repair is limits.repair
    args = chain_constraint_arguments(cons, 2)
    assert args[5] == 1 and args[11] == 1 and args[12] == 2 and args[8] == 0.01 and args[14] == 0.3
    assert not constraint_route_arguments("staged", 0) and not constraint_route_arguments("staged", 3) and constraint_route_arguments("chain", 0)


def test_refusals_without_a_device(tmp_path):
    env, ypath = write_configs(str(tmp_path), joint=True, ctx_dim=32, N=3, K=6, k_ret=3, H=4, step=2)
    weights = JMIDWeights.from_seed(NetDims(ctx_dim=32), 1)
    with pytest.raises(ValueError, match="collision_free_rounds"):
        HumanTrajectoryForecasterSim(env, ypath, weights=weights, rng_compat="device", collision_free_rounds=2, constraint_type="opt_softplus",
                                     constraint_route="chain")
    with pytest.raises(ValueError, match="constraint_route must be"):
        HumanTrajectoryForecasterSim(env, ypath, weights=weights, constraint_route="fused")
    # the default route keeps its refusals
    for flag in ("device_scene", "device_frames"):
        with pytest.raises(ValueError, match="no one-entry chain"):
            HumanTrajectoryForecasterSim(env, ypath, weights=weights, guidance={}, **{flag: True})
        with pytest.raises(ValueError, match="no one-entry chain"):
            HumanTrajectoryForecasterSim(env, ypath, weights=weights, guidance={}, constraint_route="staged", **{flag: True})
    with pytest.raises(ValueError, match="static_obstacles and wall_radius"):
        HumanTrajectoryForecasterSim(env, ypath, weights=weights, guidance={"walls": True}, constraint_route="chain", device_scene=True)
    hum, rob = np.zeros((2, 6, 3, 2)), np.zeros((2, 6, 2))
    kw = dict(num_samples=6, num_ret_samples=3, horizon=4, time_step=0.25)
    with pytest.raises(ValueError, match="collision_free_rounds"):
        predict_batch(None, hum, rob, [0, 1], noise="device", collision_free_rounds=2, constraint_type="opt_softplus", constraint_route="chain", **kw)
    with pytest.raises(ValueError, match="constraint_route must be"):
        predict_batch(None, hum, rob, [0, 1], constraint_route="one", **kw)
