#!/usr/bin/env python3
"""Generate tests/golden/shorthist_*.npz by RUNNING THE REFERENCE on tracks seen for fewer than hist_len frames (build container only, as
make_golden.py):

    python tests/golden/make_golden_short_history.py

The reference's simulator wrapper refuses such scenes, its model does not: every batch row carries a first_history_index
(MID/dataset/preprocessing.py:468) and the three LSTMs run on the slice from there on (MID/models/encoders/model_utils.py:77-105).  So the
Scene / Node objects are built here the way mid_sim_wrapper.py:358-411 builds them - positions, derivative_of over the track's own span,
node.first_timestep per track; a one-frame track is kept (the wrapper skips it, the dataset loader keeps it as a graph node) - and the
reference's get_timesteps_data is called with min_ht=1, max_ht=F-1, min_ft=0, max_ft=0.  Stored per case, arrays only: the inputs (human_xy
and robot_xy [F, N, 2] / [F, 2] with NaN in front of a track's first frame, first_frame [N + 1] robot first), the batch tensors (first_hist,
x_t, x_st), the summed neighbour histories and clamped edge values as encode_edge forms them (nbr_sum, edge_mask, n_nbr), the ego track ids
(node_ids), every pedestrian's constant-velocity row by the arithmetic of mid_sim_wrapper.py:413-429 (cv), and the get_latent output (ctx)
under the synthetic weights of JMIDWeights.from_seed (dims, wseed and checksum stored).

  shorthist_mixed_w32_n4 / _w256_n4   robot full, pedestrians first seen at frames [0, 2, 4, 3], one cluster; pedestrians 1 and 3 are both
                                      present on the last three frames and within the radius of each other on the last one only
  shorthist_start_n3                  the whole scene has L = 2 frames (keys l2_*) and L = 3 frames (keys l3_*): the episode start;
                                      *_human_raw / *_robot_raw are the L frames as pushed
  shorthist_oneframe_n4               pedestrian 1 has a single frame next to three longer tracks: no ego row, still a neighbour
  shorthist_loss_jmid_w32_e2a3t6      DiffusionTraj.get_loss (generator pattern of make_golden_loss.py, explicit t) on the contexts
                                      get_latent makes of two such scenes: rows with first_history_index [0, 1, 4] and [4, 0, 1]

Nothing hinges on rounding; the margins are asserted here and were, when the files were written (all scenes):
  smallest |pair distance - 3.0| over the last three frames            7.4e-02   (asserted > 1e-9)
  every pedestrian is within 3 m of every other at the last frame: all clusters have the same membership, whichever is chosen
  (the cluster choice compares distances of DIFFERENT memberships only; asserted: one membership)
"""
import os

import numpy as np

from make_golden import install_shims, make_forecaster, np32  # noqa: F401  (install_shims runs on import)

import pandas as pd  # noqa: E402
import torch  # noqa: E402

from sicnav_diffusion.JMID.MID.dataset.preprocessing import generate_mask, get_timesteps_data  # noqa: E402
from sicnav_diffusion.JMID.MID.environment import Node, Scene, derivative_of  # noqa: E402
from sicnav_diffusion.JMID.MID.models.encoders.model_utils import ModeKeys  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
F, DT, H = 6, 0.25, 6
RADIUS = 3.0
MARGINS = []


def tracks(last, vel, curve, first_frame):
    """Positions [F, n, 2] of n nodes: last + vel * tau + curve * tau^2 at tau = (t - (F-1)) * DT, NaN in front of first_frame."""
    tau = (np.arange(F) - (F - 1))[:, None, None] * DT
    p = np.asarray(last, float)[None] + np.asarray(vel, float)[None] * tau + np.asarray(curve, float)[None] * tau ** 2
    p[np.arange(F)[:, None] < np.asarray(first_frame)[None, :]] = np.nan
    return p


def check_margins(pos, first_frame):
    """pos [F, N+1, 2] robot first.  Every pair distance on the last three frames stays clear of the radius; one cluster membership."""
    with np.errstate(invalid="ignore"):
        d = np.sqrt(np.square(pos[F - 3:, :, None] - pos[F - 3:, None, :]).sum(-1))
    m = np.nanmin(np.abs(d - RADIUS))
    assert m > 1e-9, m
    near = d[-1] < RADIUS
    assert all((near[j] == near[1]).all() for j in range(1, pos.shape[1])), "the pedestrians' clusters differ"
    MARGINS.append(float(m))
    return near[1]                      # the chosen cluster's row (robot first)


def build_scene(f, pos, first_frame, in_mask):
    """mid_sim_wrapper.py:358-411 with a first frame per track (and without its skip of one-frame tracks)."""
    env = f.mid_env
    cols = pd.MultiIndex.from_product([["position", "velocity", "acceleration"], ["x", "y"]])
    scene = Scene(timesteps=F, dt=DT, name="posvel_tracker/pos", aug_func=None)
    for j in np.nonzero(in_mask)[0]:
        x, y = pos[first_frame[j]:, j, 0], pos[first_frame[j]:, j, 1]
        vx, vy = derivative_of(x, scene.dt), derivative_of(y, scene.dt)
        ax, ay = derivative_of(vx, scene.dt), derivative_of(vy, scene.dt)
        data = pd.DataFrame({("position", "x"): x, ("position", "y"): y, ("velocity", "x"): vx, ("velocity", "y"): vy,
                             ("acceleration", "x"): ax, ("acceleration", "y"): ay}, columns=cols)
        node = Node(node_type=env.NodeType.JRDB_ROBOT if j == 0 else env.NodeType.PEDESTRIAN, node_id=str(j - 1), data=data,
                    aux_data={"pos_x_mean": 0.0, "pos_y_mean": 0.0})
        node.first_timestep = int(first_frame[j])
        scene.nodes.append(node)
    env.scenes = [scene]
    return scene


def reference_batch(f, pos, first_frame):
    in_mask = check_margins(pos, first_frame)
    scene = build_scene(f, pos, first_frame, in_mask)
    hyp = f.mid_model.hyperparams
    out = get_timesteps_data(env=f.mid_env, scene=scene, t=np.arange(F - 1, F), node_type="PEDESTRIAN", state=hyp["state"],
                             pred_state=hyp["pred_state"], edge_types=f.mid_env.get_edge_types(), min_ht=1, max_ht=F - 1, min_ft=0,
                             max_ft=0, hyperparams=hyp)
    batch, nodes, _ = out
    return batch, [int(n.id) for n in nodes], in_mask


def constant_velocity(pos, first_frame):
    """mid_sim_wrapper.py:413-429 for every pedestrian, over its own span."""
    N = pos.shape[1] - 1
    cv = np.zeros((N, H, 2))
    for i in range(N):
        for c in range(2):
            x = pos[first_frame[i + 1]:, i + 1, c]
            v = derivative_of(x, DT)
            cv[i, :, c] = x[-1] + np.cumsum(np.tile(v[-1] * DT, H))
    return cv


def reduce_batch(batch):
    """What the existing wrapper fixtures store of a batch: the tensors and the neighbour reductions of encode_edge."""
    first_hist, x_t, _y, x_st_t, _yst, nbr, nbr_edge, _r, _m, _p = batch
    A, Th = x_t.shape[0], x_t.shape[1]
    keys = [k for k in nbr.keys() if str(k[0]) == "PEDESTRIAN"]
    assert [str(k[1]) for k in keys] == ["PEDESTRIAN", "JRDB_ROBOT"], keys
    nbr_sum = np.zeros((A, 2, Th, 6), np.float32)
    edge_mask = np.zeros((A, 2), np.float32)
    n_nbr = np.zeros((A, 2), np.int64)
    for e, key in enumerate(keys):
        for a in range(A):
            lst = nbr[key][a]
            n_nbr[a, e] = len(lst)
            if len(lst):
                nbr_sum[a, e] = torch.stack(lst, 0).sum(0).numpy()
            edge_mask[a, e] = float(torch.clamp(torch.sum(nbr_edge[key][a], dim=0, keepdim=True), max=1.0))
    return dict(first_hist=np.asarray(first_hist).astype(np.int32), x_t=np32(x_t), x_st=np32(x_st_t), nbr_sum=nbr_sum, edge_mask=edge_mask,
                n_nbr=n_nbr)


def scene_case(f, pos, first_frame):
    first_frame = np.asarray(first_frame, np.int32)
    batch, ids, in_mask = reference_batch(f, pos, first_frame)
    with torch.no_grad():
        ctx = f.mid_model.model.encoder.get_latent(ModeKeys.PREDICT, batch, "PEDESTRIAN")
    out = reduce_batch(batch)
    assert (out["first_hist"] == first_frame[1:][ids]).all()
    assert np.isfinite(out["nbr_sum"]).all() and np.isfinite(np32(ctx)).all()
    out.update(human_xy=pos[:, 1:], robot_xy=pos[:, 0], first_frame=first_frame, node_ids=np.asarray(ids), ctx=np32(ctx),
               cv=constant_velocity(pos, first_frame), robot_in_cluster=bool(in_mask[0]))
    return out


def save(name, **arrays):
    path = os.path.join(HERE, name)
    np.savez_compressed(path, **arrays)
    print(f"wrote {name}: {os.path.getsize(path) / 1024:.1f} KB")


def meta(weights, ctx_dim, wseed):
    return dict(ctx_dim=ctx_dim, wseed=wseed, wsum=weights.checksum(), joint=1, time_step=DT, past=F, H=H)


# robot first in every list
MIXED = dict(last=[[0.3, -1.6], [0.0, 0.0], [-1.45, 0.35], [0.4, 1.1], [1.42, 0.1]],
             vel=[[0.0, 0.2], [0.3, 0.1], [-0.1, 0.25], [0.2, -0.3], [-1.6, 0.0]],
             curve=[[0.0, 0.0], [0.2, -0.1], [0.1, 0.15], [-0.3, 0.2], [0.0, 0.1]], first=[0, 0, 2, 4, 3])
START = dict(last=[[0.2, -1.4], [0.1, 0.2], [-0.9, 0.6], [0.8, 0.9]], vel=[[0.0, 0.2], [0.35, 0.05], [-0.2, 0.3], [0.1, -0.4]],
             curve=[[0.0, 0.0], [0.3, -0.2], [0.15, 0.1], [-0.25, 0.3]])
ONEFRAME = dict(last=[[-0.4, -1.2], [0.0, 0.1], [1.0, 0.5], [-1.1, 0.7], [0.3, 1.3]],
                vel=[[0.1, 0.2], [0.25, 0.1], [-0.3, 0.2], [0.2, 0.2], [-0.15, -0.35]],
                curve=[[0.0, 0.0], [0.1, 0.2], [0.2, -0.1], [-0.2, 0.1], [0.1, 0.1]], first=[0, 0, 5, 1, 2])
LOSS_A = dict(last=[[0.1, -1.5], [0.0, 0.0], [1.1, 0.4], [-0.8, 0.9]], vel=[[0.0, 0.2], [0.3, -0.1], [-0.2, 0.2], [0.15, 0.3]],
              curve=[[0.0, 0.0], [0.2, 0.1], [-0.1, 0.2], [0.3, -0.2]], first=[0, 0, 1, 4])
LOSS_B = dict(last=[[-0.3, -1.3], [0.5, 0.2], [-0.7, -0.1], [0.2, 1.2]], vel=[[0.1, 0.15], [-0.25, 0.2], [0.3, 0.1], [-0.1, -0.3]],
              curve=[[0.0, 0.0], [-0.2, 0.1], [0.1, -0.3], [0.2, 0.2]], first=[0, 4, 0, 1])


def positions(spec, first=None):
    first = spec["first"] if first is None else first
    return tracks(spec["last"], spec["vel"], spec["curve"], first), first


def gen_scenes():
    for ctx_dim, wseed in ((32, 91), (256, 92)):
        f, w = make_forecaster(True, ctx_dim, 4, 6, 3, H, 50, wseed, past=F, time_step=DT)
        f.mid_model.model.eval()
        pos, first = positions(MIXED)
        case = scene_case(f, pos, first)
        d = np.sqrt(np.square(pos[3:, 2] - pos[3:, 4]).sum(-1))          # pedestrians 1 and 3 over the last three frames
        assert (d[:2] > RADIUS).all() and d[2] <= RADIUS, d
        save(f"shorthist_mixed_w{ctx_dim}_n4.npz", **meta(w, ctx_dim, wseed), **case)
        if ctx_dim != 32:
            continue
        out = {}
        for L in (2, 3):
            pos, first = positions(START, [F - L] * 4)
            case = scene_case(f, pos, first)
            case.update(human_raw=pos[F - L:, 1:], robot_raw=pos[F - L:, 0])
            out.update({f"l{L}_{k}": v for k, v in case.items()})
        save("shorthist_start_n3.npz", **meta(w, 32, wseed), **out)
        pos, first = positions(ONEFRAME)
        case = scene_case(f, pos, first)
        assert list(case["node_ids"]) == [0, 2, 3]
        save("shorthist_oneframe_n4.npz", **meta(w, 32, wseed), **case)


def gen_loss():
    ctx_dim, wseed, dseed, E, A, T = 32, 93, 811, 2, 3, H
    f, w = make_forecaster(True, ctx_dim, 3, 6, 3, H, 50, wseed, past=F, time_step=DT)
    model = f.mid_model.model
    model.eval()
    parts = []
    for spec in (LOSS_A, LOSS_B):
        pos, first = positions(spec)
        batch, ids, _ = reference_batch(f, pos, np.asarray(first))
        assert ids == [0, 1, 2]
        parts.append(batch)
    g = torch.Generator().manual_seed(dseed)
    y = torch.randn([E * A, T, 2], generator=g)
    nbr = {k: parts[0][5][k] + parts[1][5][k] for k in parts[0][5]}
    nbr_edge = {k: parts[0][6][k] + parts[1][6][k] for k in parts[0][6]}
    batch = (torch.cat([parts[0][0], parts[1][0]]), torch.cat([parts[0][1], parts[1][1]]), y, torch.cat([parts[0][3], parts[1][3]]), y,
             nbr, nbr_edge, None, None, None)
    t = np.array([[100, 37, 37], [5, 62, 1]])
    seen = {}
    vp = model.vel_predictor
    hook = vp.net.register_forward_hook(lambda m, a, kw, out: seen.update(e_theta=out.detach().clone()), with_kwargs=True)
    cuda, torch.Tensor.cuda = torch.Tensor.cuda, lambda self, *a, **k: self
    try:
        with torch.no_grad():
            ctx = model.encode(ModeKeys.PREDICT, batch, "PEDESTRIAN")
            attn_mask, loss_mask = generate_mask([None, None, y], E, T)
            torch.manual_seed(dseed)
            loss = vp.get_loss(y, ctx, batch_size=E, attn_mask=attn_mask, loss_mask=loss_mask, t=t.reshape(-1).tolist())
            torch.manual_seed(dseed)
            e = torch.randn_like(y)
    finally:
        torch.Tensor.cuda = cuda
        hook.remove()
    e_theta = seen["e_theta"].reshape(E, A, T, 2)
    assert torch.isfinite(e_theta).all() and torch.isfinite(loss)
    red = reduce_batch(batch)
    assert sorted(set(red["first_hist"].tolist())) == [0, 1, 4]
    save("shorthist_loss_jmid_w32_e2a3t6.npz", ctx_dim=ctx_dim, A=A, T=T, joint=1, wseed=wseed, dseed=dseed, wsum=w.checksum(),
         x0=np32(y).reshape(E, A, T, 2), ctx=np32(ctx).reshape(E, A, ctx_dim), t=t.astype(np.int32), e=np32(e).reshape(E, A, T, 2),
         e_theta=np32(e_theta), loss=np.float32(float(loss)), n_agents=np.full(E, A, np.int32), **red)
    print(f"loss {float(loss):.6f}")


if __name__ == "__main__":
    gen_scenes()
    gen_loss()
    print(f"smallest |pair distance - {RADIUS}| over all scenes: {min(MARGINS):.3e}")
