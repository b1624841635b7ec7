"""What tests/test_gpu_chain_constraints.py and tests/test_gpu_chain_constraints_forecaster.py share: the fixtures of the constrained
one-entry chains (``jmid_predict_constrained``, ``jmid_predict_scene_constrained``, ``jmid_forecast_scene_constrained``) and THE REFERENCE
they are compared with - the staged composition made from the engine's existing methods: the gathered rows of the scene -> ``encode`` ->
``denoise`` (guided when asked for) -> ``repair_collisions(None, ...)`` on the resident set -> ``topk(None, ...)`` -> the host assembly.

Seeded w32 nets, a 2-step DDIM table, THR = 1.0 m (the threshold at which tests/test_gpu_guided_forecaster.py sees the guidance fire)."""
import functools

import numpy as np
import torch

from safe_interactive_crowdnav_amd import scene as SC
from safe_interactive_crowdnav_amd.engine import ChainConstraints, Guidance, JmidEngine
from safe_interactive_crowdnav_amd.schedule import guidance_weights
from safe_interactive_crowdnav_amd.weights import JMIDWeights, NetDims

THR, DT, F, STEP, WSEED = 1.0, 0.25, 6, 2, 5
WALLS = np.array([[-1.5, 0.2, 1.5, 0.2], [0.4, -2.0, 0.4, 2.0]])      # L = 2: through the middle of every fixture here
RADIUS = 0.3
MODES = ("guide", "repair", "both", "both_walls")
_ENGINES = {}


def fresh_engine():
    return JmidEngine(JMIDWeights.from_seed(NetDims(ctx_dim=32), WSEED), joint=True, hist_len=F, step=STEP)


def engine_for():
    if "e" not in _ENGINES:
        _ENGINES["e"] = fresh_engine()
    return _ENGINES["e"]


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def constraints(mode, threshold=THR, weights=None):
    """The ``ChainConstraints`` of a mode: guidance only, repair only, both, both with the L = 2 walls."""
    w = guidance_weights(0.02, STEP) if weights is None else np.asarray(weights, dtype=np.float64)
    walls = dict(walls=WALLS, wall_radius=RADIUS) if mode == "both_walls" else {}
    guide = Guidance(threshold, weights=w, **walls) if mode != "repair" else None
    repair = dict(walls) if mode != "guide" else None
    return ChainConstraints(threshold, guide, repair)


def host_inputs(E, A, K, T, seed):
    """The five host arrays of ``predict``: pedestrians a few decimetres apart, so that THR = 1.0 m sees collisions."""
    g = torch.Generator().manual_seed(seed)
    x_st = torch.randn([E * A, F, 6], generator=g).numpy()
    nbr = torch.randn([E * A, 2, F, 6], generator=g).numpy()
    em = torch.rand([E * A, 2], generator=g).numpy()
    x_T = torch.randn([E, K * A, T, 2], generator=g).numpy()
    p0 = (0.6 * torch.randn([E, A, 2], generator=g)).numpy()
    return x_st, nbr, em, x_T, p0


def staged(eng, ctx, p0, dims, k, precision, cons, x_T=None, seeded=None, n_agents=None):
    """The staged composition behind ``encode``: ctx [E, A, ctx_dim], p0 [E, A, 2] -> (rows, logw or None, report dict).  The positions
    stay on the device between the stages, as in the forecaster's staged run; they come back only when k == K."""
    E, A, K, T = dims
    seeded = seeded or {}
    pad = {} if n_agents is None else {"n_agents": n_agents}
    report = dict(guide=None, sample=None, episode=None, wall=None)
    want_pos = k == K and cons.repair is None
    if cons.guidance is not None:
        _, pos, report["guide"] = eng.denoise(x_T, ctx, p0, dt=DT, precision=precision, want_vel=False, want_pos=want_pos, guidance=cons.guidance,
                                              want_guide=True, **seeded, **pad)
    elif seeded and n_agents is not None:
        pos = eng.denoise_padded_seeded(ctx, p0, n_agents, seeded["seed"], seeded["episode_ids"], K, T, dt=DT, precision=precision, want_vel=False,
                                        want_pos=want_pos)[1]
    else:
        pos = eng.denoise(x_T, ctx, p0, dt=DT, precision=precision, want_vel=False, want_pos=want_pos, **seeded, **pad)[1]
    if cons.repair is not None:
        out = eng.repair_collisions(None, threshold=cons.threshold, dims=dims, p0=p0, dt=DT, want_pos=k == K, **pad, **cons.repair)
        pos, report["sample"], report["episode"] = out[0], out[2], out[3]
        if len(out) > 4:
            report["wall"] = out[4]
    if k == K:
        return pos, None, report
    sel, lw = eng.topk(None, k, dims=dims, **pad)
    return sel, lw, report


def staged_predict(eng, inputs, k, precision, cons, n_agents=None):
    """``predict(constraints=)`` / ``predict_padded(constraints=)`` as the staged composition on the caller's arrays."""
    x_st, nbr, em, x_T, p0 = inputs
    E, A, T = p0.shape[0], p0.shape[1], x_T.shape[2]
    ctx = eng.encode(x_st, nbr, em).reshape(E, A, -1)
    return staged(eng, ctx, p0, (E, A, x_T.shape[1] // A, T), k, precision, cons, x_T=x_T, n_agents=n_agents)


def staged_scene(eng, built, pose, K, T, k, precision, cons, x_T=None, seeded=None, padded=False, forecast=False):
    """``predict_scene*`` / ``forecast_scene*`` with ``constraints=`` as the staged composition on the rows ``scene_arrays`` reads back from
    the resident scene (``built``: what ``build_scene`` returned; ``pose`` [E, N, 2]: the present positions the assembly prepends)."""
    arr, inc, n = eng.scene_arrays(), built["in_cluster"], built["n_in"]
    E, A = inc.shape[0], int(n.max())
    first = arr["first_index"].any()
    if padded:
        take = lambda key: SC.pad_agents(arr[key], inc, A)
    else:
        assert (n == A).all()
        take = lambda key: np.ascontiguousarray(arr[key][inc].reshape((E, A) + arr[key].shape[2:]))
    ctx = eng.encode(take("x_st").reshape(E * A, F, 6), take("nbr_sum").reshape(E * A, 2, F, 6), take("edge_mask").reshape(E * A, 2),
                     first_index=take("first_index").reshape(-1) if first else None).reshape(E, A, -1)
    counts = n.astype(np.int32) if padded else None
    rows, lw, report = staged(eng, ctx, take("p0"), (E, A, K, T), k, precision, cons, x_T=x_T, seeded=seeded, n_agents=counts)
    if not forecast:
        return rows, lw, report
    fc, flw = SC.assemble_forecasts(inc, rows, lw, built["cv"], pose, k, K, **({"n_agents": counts} if padded else {}))
    return fc, flw, report


def same_report(got, want):
    """The ``ChainReport`` of a constrained chain against the staged composition's report dict, bit for bit; -> the list of fields that differ."""
    bad = []
    for key in ("guide", "sample", "episode", "wall"):
        a, b = getattr(got, key), want[key]
        if (a is None) != (b is None) or (a is not None and not same_bits(a, b)):
            bad.append(key)
    return bad


def crowd(E, N, seed, half_width=1.2):
    """E episodes of N pedestrians close to each other and to the robot, walking at U(-1, 1)^2 m/s: human_xy [E, F, N, 2], robot_xy [E, F, 2]."""
    rng = np.random.default_rng(seed)
    pos0 = rng.uniform(-half_width, half_width, (E, N, 2))
    vel = rng.uniform(-1.0, 1.0, (E, N, 2))
    t = np.arange(F) * DT
    hum = pos0[:, None] + vel[:, None] * t[None, :, None, None] + 0.01 * rng.standard_normal((E, F, N, 2))
    rob = np.array([0.0, -1.0])[None, None] + np.array([0.0, 0.2])[None, None] * t[None, :, None]
    return np.ascontiguousarray(hum), np.ascontiguousarray(np.broadcast_to(rob, (E, F, 2)))


@functools.lru_cache(maxsize=None)
def mixed_crowd():
    """A batch whose clusters the build chooses itself, with windows per node (``first_frame``): (hum, rob, first_frame [E, N + 1]).  Spread
    wide enough that the in-cluster counts differ (asserted where it is used)."""
    E, N = 3, 4
    rng = np.random.default_rng(33)
    pos0 = rng.uniform(-3.5, 3.5, (E, N, 2))
    vel = rng.uniform(-1.0, 1.0, (E, N, 2))
    t = np.arange(F) * DT
    hum = pos0[:, None] + vel[:, None] * t[None, :, None, None] + 0.01 * rng.standard_normal((E, F, N, 2))
    rob = np.array([0.0, -1.0])[None, None] + np.array([0.0, 0.2])[None, None] * t[None, :, None]
    ff = np.zeros((E, N + 1), dtype=np.int32)
    ff[0, 2], ff[1, 1], ff[2, 3], ff[2, 4] = 3, 4, 2, 1      # short windows: 3, 2, 4 and 5 of the 6 frames
    return np.ascontiguousarray(hum), np.ascontiguousarray(np.broadcast_to(rob, (E, F, 2))), ff
