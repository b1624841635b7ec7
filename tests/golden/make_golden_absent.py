#!/usr/bin/env python3
"""Generate tests/golden/absent_now_w32_n4.npz by RUNNING THE REFERENCE on a scene in which one node's data ends before the current frame
(build container only, as make_golden.py):

    python tests/golden/make_golden_absent.py

The reference's model side has no special case for such a node: ``Scene.present_nodes([t])`` does not list it (no ego row), its position at
t is NaN in the temporal scene graph (a NaN distance is not <= radius: MID/environment/scene_graph.py:165-181) and
``calculate_edge_scaling`` zeroes every edge that is not adjacent now (:203-225; the removal filter [1.0, 0.0] is the identity at the
current frame) - it is nobody's neighbour at t, although it IS a node of the temporal graph, adjacent to the others on the frames where
it was still seen.  So the batch the reference makes with the node in the Scene is the batch without it, which is what
``scene.build_scenes_batched(allow_absent=True)`` computes for a pedestrian with first_frame -1.

The Scene / Node objects are built as make_golden_short_history.py builds them (mid_sim_wrapper.py:358-411 with a first frame per track),
except that pedestrian 1's data holds the frames 1 .. F-3 only: he is last seen two frames ago, 1 m from pedestrian 0.  Stored, arrays only:
the inputs (human_xy [F, N, 2] / robot_xy [F, 2] with NaN wherever a node has no data, first_frame [N + 1] robot first with -1 for him,
last_frame [N + 1]), the batch tensors and the neighbour reductions of the PRESENT nodes (first_hist, x_t, x_st, nbr_sum, edge_mask, n_nbr,
node_ids), their constant-velocity rows (cv; NaN for him), the get_latent output (ctx) under JMIDWeights.from_seed (dims, wseed, checksum).

Nothing hinges on rounding: asserted here, smallest |pair distance - 3.0| over the last three frames among the nodes that have data there
(4.0e-02 when the file was written), one cluster membership among the present pedestrians.
"""
import os

import numpy as np

from make_golden import install_shims, make_forecaster, np32  # noqa: F401  (install_shims runs on import)
from make_golden_short_history import DT, F, H, MARGINS, check_margins, constant_velocity, reduce_batch, save, tracks  # noqa: E402

import pandas as pd  # noqa: E402
import torch  # noqa: E402

from sicnav_diffusion.JMID.MID.dataset.preprocessing import get_timesteps_data  # noqa: E402
from sicnav_diffusion.JMID.MID.environment import Node, Scene, derivative_of  # noqa: E402
from sicnav_diffusion.JMID.MID.models.encoders.model_utils import ModeKeys  # noqa: E402

# robot first: pedestrian 1 (node 2) is seen on frames 1 .. F-3, pedestrian 2 from frame 2 on
SPEC = dict(last=[[0.3, -1.6], [0.0, 0.0], [0.9, 0.5], [-1.2, 0.4], [0.5, 1.3]],
            vel=[[0.0, 0.2], [0.3, 0.1], [-0.2, 0.3], [-0.1, 0.25], [0.2, -0.3]],
            curve=[[0.0, 0.0], [0.2, -0.1], [0.1, 0.1], [0.1, 0.15], [-0.3, 0.2]],
            first=[0, 0, 1, 2, 0], last_frame=[F - 1, F - 1, F - 3, F - 1, F - 1])


def build_scene(f, pos, first, last):
    """make_golden_short_history.build_scene with a last frame per track: every node is in the Scene, present on first .. last."""
    env = f.mid_env
    cols = pd.MultiIndex.from_product([["position", "velocity", "acceleration"], ["x", "y"]])
    scene = Scene(timesteps=F, dt=DT, name="posvel_tracker/pos", aug_func=None)
    for j in range(pos.shape[1]):
        x, y = pos[first[j]:last[j] + 1, j, 0], pos[first[j]:last[j] + 1, j, 1]
        vx, vy = derivative_of(x, scene.dt), derivative_of(y, scene.dt)
        ax, ay = derivative_of(vx, scene.dt), derivative_of(vy, scene.dt)
        data = pd.DataFrame({("position", "x"): x, ("position", "y"): y, ("velocity", "x"): vx, ("velocity", "y"): vy,
                             ("acceleration", "x"): ax, ("acceleration", "y"): ay}, columns=cols)
        node = Node(node_type=env.NodeType.JRDB_ROBOT if j == 0 else env.NodeType.PEDESTRIAN, node_id=str(j - 1), data=data,
                    aux_data={"pos_x_mean": 0.0, "pos_y_mean": 0.0})
        node.first_timestep = int(first[j])
        scene.nodes.append(node)
    env.scenes = [scene]
    return scene


def main():
    ctx_dim, wseed = 32, 95
    f, w = make_forecaster(True, ctx_dim, 4, 6, 3, H, 50, wseed, past=F, time_step=DT)
    f.mid_model.model.eval()
    first, last = np.asarray(SPEC["first"], np.int32), np.asarray(SPEC["last_frame"], np.int32)
    pos = tracks(SPEC["last"], SPEC["vel"], SPEC["curve"], first)
    gone = last < F - 1
    assert gone.tolist() == [False, False, True, False, False]
    d_seen = np.sqrt(np.square(pos[last[2], 2] - pos[last[2], 1]).sum())           # where he was last seen: well inside the radius of pedestrian 0
    assert d_seen < 1.5, d_seen
    pos[np.arange(F)[:, None] > last[None, :]] = np.nan
    in_mask = check_margins(pos[:, ~gone], first[~gone])                           # (the present nodes: one cluster, clear of the radius)
    assert in_mask.all()
    with np.errstate(invalid="ignore"):                                            # ... and his pairs on the frames where he has data
        d = np.sqrt(np.square(pos[F - 3:, 2:3] - pos[F - 3:]).sum(-1))
    assert np.nanmin(np.abs(d[:, [0, 1, 3, 4]] - 3.0)) > 1e-9
    scene = build_scene(f, pos, first, last)
    hyp = f.mid_model.hyperparams
    batch, nodes, _ = get_timesteps_data(env=f.mid_env, scene=scene, t=np.arange(F - 1, F), node_type="PEDESTRIAN", state=hyp["state"],
                                         pred_state=hyp["pred_state"], edge_types=f.mid_env.get_edge_types(), min_ht=1, max_ht=F - 1,
                                         min_ft=0, max_ft=0, hyperparams=hyp)
    ids = [int(n.id) for n in nodes]
    assert ids == [0, 2, 3], ids                                                   # present_nodes([t]) does not list him
    with torch.no_grad():
        ctx = f.mid_model.model.encoder.get_latent(ModeKeys.PREDICT, batch, "PEDESTRIAN")
    out = reduce_batch(batch)
    first_frame = np.where(gone, -1, first).astype(np.int32)
    assert (out["first_hist"] == first_frame[1:][ids]).all() and (out["n_nbr"][:, 0] == 2).all()      # nobody's neighbour at t
    assert np.isfinite(out["nbr_sum"]).all() and np.isfinite(np32(ctx)).all()
    cv = constant_velocity(np.where(np.isnan(pos), 0.0, pos)[:, ~gone], first[~gone])
    cv_all = np.full((pos.shape[1] - 1, H, 2), np.nan)
    cv_all[~gone[1:]] = cv
    save("absent_now_w32_n4.npz", ctx_dim=ctx_dim, wseed=wseed, wsum=w.checksum(), joint=1, time_step=DT, past=F, H=H, human_xy=pos[:, 1:],
         robot_xy=pos[:, 0], first_frame=first_frame, last_frame=last, node_ids=np.asarray(ids), ctx=np32(ctx), cv=cv_all,
         robot_in_cluster=bool(in_mask[0]), **out)
    print(f"smallest |pair distance - 3.0| among the present nodes: {min(MARGINS):.3e}; he was last seen {d_seen:.2f} m from pedestrian 0")


if __name__ == "__main__":
    main()
