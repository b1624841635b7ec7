"""Collision repair with walls on the device (csrc/repair.hpp, repair_sample_kernel<true>; jmid_repair_collisions_walls) against its NumPy
twin (``metrics.repair_collisions_host(walls=, wall_radius=)``; tests/test_repair_walls_host.py pins the twin itself and the stability of
these inputs under the one operation that differs, exp): states, iteration counts, episode rows, positions and velocities equal the twin's
bits, the distance columns within one fp32 unit in the last place (what tests/test_gpu_repair.py and tests/test_gpu_wall_statistics.py allow
for the same columns); then the raw C entry, the resident set, and the Python layer against the staged composition by hand."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from safe_interactive_crowdnav_amd import _lib, crowd_env, metrics, offline
from safe_interactive_crowdnav_amd import scene as SC
from safe_interactive_crowdnav_amd.engine import JmidError
from safe_interactive_crowdnav_amd.forecaster import predict_batch, rank_samples, repair_totals
from tests.repair_cases import gpu_cases
from tests.repair_wall_cases import DT as DTV, RADIUS, THRESHOLD, constructed, wall_cases
from tests.test_gpu_collision_statistics import assert_within_one_ulp
from tests.test_gpu_noise import GOLDEN, engine_for, make_forecaster, same_bits
from tests.test_gpu_rejection import SEED, to_np
from tests.test_gpu_rejection_walls import inputs as wall_inputs, wall_from
from tests.test_gpu_repair import ulps
from tests.test_scene_device_inputs import DT, random_positions

HALLWAY = np.ascontiguousarray(np.asarray(crowd_env.static_obstacles("hallway_static")[0], dtype=np.float64).reshape(-1, 4))
_TWIN = {}


def case(name):
    """(pos, p0, vel, walls, the twin's five outputs), the twin computed once per input."""
    if name not in _TWIN:
        pos, p0, walls = wall_cases()[name]
        if name == "e2a3k5t3l2":     # a sample that cannot be judged rides along: state 3, untouched
            pos = pos.copy()
            pos[1, 4, 2, 1, 0] = np.nan
        prev = np.concatenate([np.broadcast_to(p0[:, None, :, None], pos[:, :, :, :1].shape), pos[:, :, :, :-1]], axis=3)
        vel = ((pos - prev) / np.float32(DTV)).astype(np.float32)
        _TWIN[name] = (pos, p0, vel, walls, metrics.repair_collisions_host(pos, THRESHOLD, p0=p0, dt=DTV, vel=vel, walls=walls, wall_radius=RADIUS))
    return _TWIN[name]


def assert_equals_the_twin(got, want, pos, vel, what):
    out, vel_out, sample, episode, wall = (to_np(a) for a in got)
    w_out, w_vel, w_sample, w_episode, w_wall = want
    state = sample[..., 3]
    print(f"{what}: states {np.bincount(state.astype(int).ravel(), minlength=4).tolist()}, episodes {episode.tolist()}")
    assert np.array_equal(state, w_sample[..., 3]) and np.array_equal(sample[..., 2], w_sample[..., 2]), what
    assert np.array_equal(episode, w_episode), what
    assert same_bits(out, w_out) and same_bits(vel_out, w_vel), what                   # positions and velocities: the twin's bits
    fixed = state == metrics.REPAIR_REPAIRED
    assert same_bits(out[~fixed], pos[~fixed]) and same_bits(vel_out[~fixed], vel[~fixed]), what
    finite = np.isfinite(w_sample[..., :2])
    assert np.array_equal(np.isnan(sample[..., :2]), np.isnan(w_sample[..., :2])) and np.array_equal(np.isinf(sample[..., :2]), np.isinf(w_sample[..., :2]))
    if finite.any():
        assert ulps(sample[..., :2][finite], w_sample[..., :2][finite].astype(np.float32)) <= 1, what
    assert_within_one_ulp(np.ascontiguousarray(wall), w_wall, what + " min_clear")


@pytest.mark.parametrize("name,device", [("e2a3k5t3l2", False), ("e2a3k5t3l2", True), ("a1t2k1l1", False), ("a1t2k1l1", True), ("k300", False),
                                         ("k300", True), ("l64", False), ("l64", True), ("a64t24l64", False)])
def test_equals_the_twin(name, device):
    eng = engine_for()
    pos, p0, vel, walls, want = case(name)
    assert want[3][:, 1].sum() >= 1
    args = [torch.from_numpy(a).cuda() for a in (pos, p0, vel)] if device else [pos, p0, vel]
    got = eng.repair_collisions(args[0], THRESHOLD, p0=args[1], dt=DTV, vel=args[2], walls=walls, wall_radius=RADIUS)
    assert_equals_the_twin(got, want, pos, vel, name)
    out, vel_out, sample, _, wall = (to_np(a) for a in got)
    fixed = sample[..., 3] == metrics.REPAIR_REPAIRED
    # the two statistics entries on the device's own output: every repaired sample is clean, and reports the clearances it has
    after = eng.collision_statistics(out, THRESHOLD, agents=False)[2]
    hits = eng.wall_statistics(out, walls, RADIUS, p0=p0)[2]
    assert not (after[..., 3][fixed] > 0).any() and not (hits[..., 1][fixed] > 0).any()
    assert same_bits(after[..., 0][fixed], sample[..., 1][fixed]) and same_bits(hits[..., 0][fixed], wall[..., 1][fixed])
    prev = np.concatenate([np.broadcast_to(p0[:, None, :, None], out[:, :, :, :1].shape), out[:, :, :, :-1]], axis=3).astype(np.float64)
    assert same_bits(vel_out[fixed], ((out.astype(np.float64) - prev) / DTV).astype(np.float32)[fixed])


def test_constructed_cases_on_the_device():
    eng = engine_for()
    for name, (pos, p0, walls) in constructed().items():
        want = metrics.repair_collisions_host(pos, THRESHOLD, p0=p0, dt=DTV, walls=walls, wall_radius=RADIUS)
        got = eng.repair_collisions(pos, THRESHOLD, p0=p0, dt=DTV, walls=walls, wall_radius=RADIUS)
        print(f"{name}: state {int(got[2][0, 0, 3])} after {int(got[2][0, 0, 2])} iterations, clearance {got[4][0, 0].tolist()}")
        assert same_bits(got[0], want[0]) and np.array_equal(got[2][..., 2:], want[2][..., 2:]) and np.array_equal(got[3], want[3]), name
        assert_within_one_ulp(got[4], want[4], name + " min_clear")


def raw(eng, name, pos, p0, **kw):
    """One call of a raw entry on host memory -> (rc, message, pos_out, sample, episode, wall)."""
    E, K, A, T, _ = pos.shape
    ptr = lambda a: C.c_void_p(a.ctypes.data) if a is not None else None
    out, sample, episode, wall = np.empty_like(pos), np.empty((E, K, 4), np.float32), np.empty((E, 3), np.int32), np.empty((E, K, 2), np.float32)
    a = dict(dict(pos=pos, p0=p0, threshold=THRESHOLD, margin=0.02, tau=0.005, step=0.02, max_iter=32, pos_out=out, vel_out=None,
                  sample_out=sample, wall_out=wall, walls=None, L=0, wall_radius=RADIUS, T=T, n_agents=None), **kw)
    head = (eng._h, E, A, K, a["T"], ptr(a["n_agents"]), ptr(a["pos"]), ptr(a["p0"]), DTV, a["threshold"], a["margin"], a["tau"], a["step"], a["max_iter"])
    tail = (ptr(a["pos_out"]), ptr(a["vel_out"]), ptr(a["sample_out"]), ptr(a.get("episode_out", episode)))
    if name == "jmid_repair_collisions":
        rc = eng._lib.jmid_repair_collisions(*head, *tail, _lib.MEM_HOST)
    else:
        rc = eng._lib.jmid_repair_collisions_walls(*head, a["L"], ptr(a["walls"]), a["wall_radius"], *tail, ptr(a["wall_out"]), _lib.MEM_HOST)
    return rc, eng._lib.jmid_last_error(eng._h).decode(), out, sample, episode, wall


def test_the_raw_entry_and_no_walls():
    eng = engine_for()
    pos, p0, vel, walls, want = case("e2a3k5t3l2")
    rc, _, out, sample, episode, wall = raw(eng, "walls", pos, p0, walls=walls, L=len(walls))
    assert rc == 0 and same_bits(out, want[0]) and np.array_equal(sample[..., 2:], want[2][..., 2:]) and np.array_equal(episode, want[3])
    assert_within_one_ulp(wall, want[4], "raw min_clear")
    # L = 0 IS jmid_repair_collisions, bit for bit, on that entry's own inputs; wall_out is +inf
    for name in ("e2a3k5t3", "k300", "a64t2k1"):
        pos, p0 = gpu_cases()[name]
        old, new = raw(eng, "jmid_repair_collisions", pos, p0), raw(eng, "walls", pos, p0, L=0)
        assert old[0] == 0 and new[0] == 0 and old[4][:, 1].sum() >= 1
        for a, b in zip(old[2:5], new[2:5]):
            assert same_bits(a, b), name
        assert np.all(np.isposinf(new[5]))
        plain = eng.repair_collisions(pos, THRESHOLD, p0=p0, dt=DTV, vel=np.zeros_like(pos))
        empty = eng.repair_collisions(pos, THRESHOLD, p0=p0, dt=DTV, vel=np.zeros_like(pos), walls=np.zeros((0, 4)), wall_radius=RADIUS)
        assert len(plain) == 4 and len(empty) == 5 and all(same_bits(a, b) for a, b in zip(plain, empty)) and np.all(np.isposinf(empty[4]))


def test_refusals_of_the_raw_entry():
    eng = engine_for()
    pos, p0, vel, walls, _ = case("e2a3k5t3l2")
    L = len(walls)
    assert raw(eng, "walls", pos, p0, walls=walls, L=L)[0] == 0 and raw(eng, "walls", pos, p0, walls=walls, L=L, vel_out=vel.copy())[0] == 0
    assert raw(eng, "walls", pos, None, walls=walls, L=L)[0] == 0                      # without p0: T - 1 steps per agent
    bad = walls.copy()
    bad[1, 2] = np.nan
    for word, kw in (("0 <= L <= 64", dict(L=65)), ("0 <= L <= 64", dict(L=-1)), ("null walls", dict(walls=None)), ("wall_radius", dict(wall_radius=-0.1)),
                     ("wall_radius", dict(wall_radius=float("inf"))), ("non-finite", dict(walls=bad)), ("threshold", dict(threshold=float("nan"))),
                     ("tau", dict(tau=0.0)), ("max_iter", dict(max_iter=1025)), ("p0", dict(p0=None, vel_out=vel.copy())),
                     ("every output is NULL", dict(pos_out=None, sample_out=None, wall_out=None, episode_out=None)), ("T", dict(T=1)),
                     ("n_agents", dict(n_agents=np.array([3, 4], np.int32)))):
        args = dict(dict(walls=walls, L=L), **kw)
        rc, msg = raw(eng, "walls", pos, args.pop("p0", p0), **args)[:2]
        assert rc == _lib.EINVAL and "jmid_repair_collisions_walls" in msg and word in msg, (word, rc, msg)
    assert raw(eng, "walls", pos, p0, walls=walls, L=L, pos_out=None, sample_out=None, episode_out=None)[0] == 0      # wall_out alone is an output
    with pytest.raises(ValueError, match="wall_radius"):
        eng.repair_collisions(pos, THRESHOLD, walls=walls)
    with pytest.raises(ValueError, match="without walls"):
        eng.repair_collisions(pos, THRESHOLD, wall_radius=RADIUS)


def test_padded_counts_equal_the_compacted_episodes():
    eng = engine_for()
    pos, p0, walls = wall_cases()["e3a3k6t4"]
    counts = np.array([3, 1, 2], dtype=np.int32)
    padded, lead, vel = pos.copy(), p0.copy(), np.full(pos.shape, 7.0, dtype=np.float32)
    for e, n in enumerate(counts):
        padded[e, :, n:], lead[e, n:] = np.nan, np.nan
    kw = dict(dt=DTV, walls=walls, wall_radius=RADIUS)
    got = eng.repair_collisions(padded, THRESHOLD, p0=lead, vel=vel, n_agents=counts, **kw)
    assert got[3][:, 1].min() >= 1                                                      # the single agent of episode 1 is repaired too
    for e, n in enumerate(counts):
        alone = eng.repair_collisions(np.ascontiguousarray(pos[e:e + 1, :, :n]), THRESHOLD, p0=np.ascontiguousarray(p0[e:e + 1, :n]),
                                      vel=np.ascontiguousarray(vel[e:e + 1, :, :n]), **kw)
        assert same_bits(got[0][e, :, :n], alone[0][0]) and same_bits(got[0][e, :, n:], padded[e, :, n:])
        assert same_bits(got[1][e, :, :n], alone[1][0]) and same_bits(got[1][e, :, n:], vel[e, :, n:])
        assert same_bits(got[2][e], alone[2][0]) and same_bits(got[3][e], alone[3][0]) and same_bits(got[4][e], alone[4][0])
    want = metrics.repair_collisions_host(padded, THRESHOLD, p0=lead, vel=vel, n_agents=counts, **kw)
    assert_equals_the_twin(got, want, padded, vel, "padded (3, 1, 2)")
    assert not (eng.wall_statistics(got[0], walls, RADIUS, p0=lead, n_agents=counts)[2][..., 1][got[2][..., 3] == 1] > 0).any()


def test_partition_invariance():
    eng = engine_for()
    pos, p0, walls = wall_cases()["e5a3k4t4"]
    kw = dict(dt=DTV, walls=walls, wall_radius=RADIUS)
    whole = eng.repair_collisions(pos, THRESHOLD, p0=p0, vel=np.zeros_like(pos), **kw)
    assert (whole[3][:, 1] > 0).sum() >= 3
    for part in ([0, 1], [2, 3, 4], [0], [1], [2], [3], [4]):
        got = eng.repair_collisions(pos[part], THRESHOLD, p0=p0[part], vel=np.zeros_like(pos[part]), **kw)
        for g, w in zip(got, whole):
            assert same_bits(g, w[part]), part


@pytest.mark.parametrize("after", ["denoise", "denoise_reject_walls"])
def test_the_resident_set_is_repaired_in_place(after):
    eng = engine_for()
    eng.set_step(2, "ddim")
    E, A, K, T, k = 4, 3, 5, 3, 2
    ctx, p0 = wall_inputs(E, A)
    seeded = dict(seed=SEED, episode_ids=[7, 0, 4294967295, 12], K=K, T=T)
    walls = wall_from(eng.denoise(None, ctx, p0, **seeded)[1], p0)
    kw = dict(dt=DTV, walls=walls, wall_radius=RADIUS)

    def draw():
        if after == "denoise":
            return eng.denoise(None, ctx, p0, **seeded)[:2]
        return eng.denoise_reject(ctx, p0, threshold=THRESHOLD, max_rounds=1, walls=walls, wall_radius=RADIUS, **seeded)[:2]

    vel, pos = draw()
    want = eng.repair_collisions(pos, THRESHOLD, p0=p0, vel=vel, **kw)                  # (given positions: the resident set is not touched)
    for a, b in zip(eng.wall_statistics(None, walls, RADIUS, p0=p0, dims=(E, A, K, T)), eng.wall_statistics(pos, walls, RADIUS, p0=p0)):
        assert same_bits(a, b)
    assert want[3][:, 0].sum() >= 1, "nothing is flagged"
    print(f"after {after}: episodes {want[3].tolist()}, causes {metrics.repair_causes(want[2], want[4], THRESHOLD, RADIUS)}")
    got = eng.repair_collisions(None, THRESHOLD, p0=p0, dims=(E, A, K, T), want_pos=True, **kw)
    assert same_bits(got[0], want[0]) and got[1] is None and all(same_bits(a, b) for a, b in zip(got[2:], want[2:]))
    for a, b in zip(eng.topk(None, k, dims=(E, A, K, T)), eng.topk(want[0], k)):
        assert same_bits(a, b)
    for a, b in zip(eng.wall_statistics(None, walls, RADIUS, p0=p0, dims=(E, A, K, T)), eng.wall_statistics(want[0], walls, RADIUS, p0=p0)):
        assert same_bits(a, b)
    # a second repair of the repaired set finds only what the first one reverted, and changes nothing
    again = eng.repair_collisions(None, THRESHOLD, p0=p0, dims=(E, A, K, T), want_pos=True, **kw)
    assert same_bits(again[0], want[0]) and np.array_equal(again[3][:, 0], want[3][:, 0] - want[3][:, 1]) and not again[3][:, 1].any()
    eng.denoise(None, ctx, None, want_pos=False, **seeded)
    with pytest.raises(JmidError) as err:
        eng.repair_collisions(None, THRESHOLD, p0=p0, dims=(E, A, K, T), **kw)
    assert err.value.code == _lib.EINVAL


def by_hand(f, thr, radius, rounds=0):
    """The staged composition of one ``predict_ret_best()`` with ``constraint_type="opt_softplus_walls"`` from the engine's entries."""
    F, H, K, k = f.num_hist_frames, f.predict_horizon, f.num_samples, f.num_ret_samples
    hum_xy, rob_xy, pose_now = SC.frame_table(*f._snapshot(), f.time_step, F)
    sb = SC.build_scene(hum_xy, rob_xy, f.time_step, H, F)
    A = len(sb.ids_in)
    ctx = f.engine.encode(sb.x_st, sb.nbr_sum, sb.edge_mask)
    loop = dict(walls=HALLWAY, wall_radius=radius) if rounds else {}
    _, pos, _, loop_episode, *_ = f.engine.denoise_reject(ctx[None], sb.p0[None], f.noise_seed, [f.episode_id], K, H, dt=f.time_step, precision="f32",
                                                          threshold=thr, max_rounds=rounds, draw0=0, **loop)
    pos, _, sample, episode, wall = f.engine.repair_collisions(pos, thr, p0=sb.p0[None], dt=f.time_step, walls=HALLWAY, wall_radius=radius)
    rows, logw = rank_samples(f.engine, "device" if k < K else "none", pos, k, (1, A, K, H))
    inc = np.zeros(f.num_hums, dtype=bool)
    inc[sb.ids_in] = True
    result = SC.assemble_forecasts(inc, rows[0], None if logw is None else logw[0], sb.cv_forecasts, pose_now, k, K)
    return result, episode, metrics.repair_causes(sample, wall, thr, radius), loop_episode


def test_forecaster_with_the_new_value(tmp_path):
    z = np.load(os.path.join(GOLDEN, "wrapper_jmid_topk.npz"))
    radius, thr = 0.05, THRESHOLD
    kw = dict(rng_compat="device", seed=17, precision="f32", collision_threshold=thr, static_obstacles=HALLWAY.reshape(-1, 2, 2), wall_radius=radius)
    f = make_forecaster(z, tmp_path / "a", constraint_type="opt_softplus_walls", **kw)
    assert f.repair is None and f.repair_causes is None and f._walls == {}
    fc, lw = f.predict_ret_best()
    (want_fc, want_lw), episode, causes, _ = by_hand(f, thr, radius)
    print(f"hallway_static at radius {radius}: repair {f.repair}, causes {f.repair_causes}")
    assert same_bits(fc, want_fc) and same_bits(lw, want_lw) and f.repair == repair_totals(episode) and f.repair_causes == causes
    assert f.repair[0] >= 1 and causes["walls"] >= 1 and f.repair[2] == f.repair[0] - f.repair[1]
    # the redraw loop first (both predicates), the repair on whatever it left flagged for either cause
    both = make_forecaster(z, tmp_path / "b", constraint_type="opt_softplus_walls", collision_free_rounds=1, **kw)
    assert sorted(both._walls) == ["wall_radius", "walls"]
    fc, lw = both.predict_ret_best()
    (want_fc, want_lw), episode, causes, _ = by_hand(both, thr, radius, rounds=1)
    print(f"R = 1 + repair: rejection {both.rejection}, repair {both.repair}")
    assert same_bits(fc, want_fc) and same_bits(lw, want_lw) and both.repair == repair_totals(episode) and both.repair_causes == causes
    assert both.repair[0] == both.rejection[1] - both.rejection[2]
    # off unless asked for: the forecaster without a constraint type gives the plain bits, walls or no walls in the loop
    plain = make_forecaster(z, tmp_path / "c", rng_compat="device", seed=17, precision="f32").predict_ret_best()
    off = make_forecaster(z, tmp_path / "d", rng_compat="device", seed=17, precision="f32", collision_threshold=thr).predict_ret_best()
    assert same_bits(plain[0], off[0]) and same_bits(plain[1], off[1])


def test_predict_batch_with_the_new_value():
    E, N, K, k, H = 6, 6, 16, 5, 8
    hum, rob = random_positions(E, N, 67, half_width=2.5)           # in-cluster counts (1, 4, 4, 2, 4, 3)
    eng = engine_for()
    eng.set_step(2, "ddim")
    gids = [1000 + 7 * e for e in range(E)]
    radius = 0.05
    kw = dict(num_samples=K, num_ret_samples=k, horizon=H, time_step=DT, precision="f32", collision_threshold=0.3, noise="device", seed=2024,
              constraint_type="opt_softplus_walls", static_obstacles=HALLWAY, wall_radius=radius)
    for extra in (dict(), dict(collision_free_rounds=1), dict(collision_free_rounds=1, collision_free_padded=True)):
        stats = {}
        fc, lw, inc = predict_batch(eng, hum, rob, gids, stats=stats, **kw, **extra)
        counts = inc.sum(axis=1)
        print(f"{extra}: counts {counts.tolist()}, repair {stats['repair'].tolist()}, causes {stats['repair_causes']}")
        assert len(np.unique(counts)) >= 2 and counts.min() >= 1 and counts.max() <= 4, counts
        assert stats["repair"].shape == (E, 3) and stats["repair"][:, 0].sum() >= 1 and stats["repair_causes"]["walls"] >= 1
        assert stats["repair_causes"]["candidates"] == stats["repair"][:, 0].sum() and stats["repair_causes"]["repaired"] == stats["repair"][:, 1].sum()
        if extra:                                    # the repair takes what the loop left flagged, for either cause
            assert np.array_equal(stats["repair"][:, 0], stats["episodes"][:, 0] - stats["episodes"][:, 1])
        if extra.get("collision_free_padded"):
            continue                                 # (a padded call's attention rounds differently per batch: no bitwise rule)
        for e in (0, E - 1):
            one = {}
            fc1, lw1, _ = predict_batch(eng, hum[e:e + 1], rob[e:e + 1], gids[e:e + 1], stats=one, **kw, **extra)
            assert same_bits(fc1[0], fc[e]) and same_bits(lw1[0], lw[e]) and same_bits(one["repair"][0], stats["repair"][e])
        if not extra:                                # the composition by hand of one episode: build, encode, denoise, repair, rank, assemble
            e = int(np.argmax(counts))
            b = SC.build_scenes_batched(hum[e:e + 1], rob[e:e + 1], DT, horizon=H)
            rows, A = np.nonzero(b["in_cluster"][0])[0], int(counts[e])
            p0 = np.ascontiguousarray(b["p0"][0, rows])[None]
            ctx = eng.encode(b["x_st"][0, rows], b["nbr_sum"][0, rows], b["edge_mask"][0, rows]).reshape(1, A, -1)
            _, pos = eng.denoise(None, ctx, p0, dt=DT, precision="f32", want_vel=False, seed=2024, episode_ids=np.asarray(gids[e:e + 1]), K=K, T=H)
            pos, _, _, episode, _ = eng.repair_collisions(pos, 0.3, p0=p0, dt=DT, walls=HALLWAY, wall_radius=radius)
            sel, logw = eng.topk(pos, k)
            want = SC.assemble_forecasts(b["in_cluster"], sel, logw, b["cv"], hum[e:e + 1, -1], k, K)
            assert same_bits(want[0][0], fc[e]) and same_bits(want[1][0], lw[e]) and same_bits(episode[0], stats["repair"][e])


def test_offline_generate_with_the_new_value():
    eng = engine_for()
    B, T, n = 3, 4, 8
    ctx, p0 = wall_inputs(1, B)
    ctx, p0 = ctx[0], (p0[0] * 0.5 + np.float32([0.3, 0.0])).astype(np.float32)        # inside the hallway
    call = dict(sampling="ddim", step=2, seed=SEED)
    radius = 0.05
    plain = offline.generate(eng, ctx, p0, 0.25, T, n, True, **call)
    lead = np.ascontiguousarray(np.broadcast_to(p0[None], (n, B, 2)))
    want, _, sample, episode, wall = eng.repair_collisions(plain[0].reshape(n, 1, B, T, 2), THRESHOLD, p0=lead, dt=0.25, walls=HALLWAY, wall_radius=radius)
    pos, steps, num_iter, flagged, fixed = offline.generate(eng, ctx, p0, 0.25, T, n, True, with_constraints=True, constraint_type="opt_softplus_walls",
                                                            collision_threshold=THRESHOLD, static_obstacles=HALLWAY, wall_radius=radius, **call)
    print(f"num_iter {num_iter}, {flagged} flagged, {fixed} repaired, causes {metrics.repair_causes(sample, wall, THRESHOLD, radius)}")
    assert same_bits(pos, want.reshape(n, B, T, 2)) and steps == plain[1]
    assert (num_iter, flagged, fixed) == (int(episode[:, 2].max()), int(episode[:, 0].sum()), int(episode[:, 1].sum())) and flagged >= 1
    with pytest.raises(ValueError, match="walls are not in the repair's objective"):
        offline.generate(eng, ctx, p0, 0.25, T, n, True, with_constraints=True, constraint_type="opt_softplus", static_obstacles=HALLWAY,
                         wall_radius=radius, **call)
    eng.set_step(2, "ddim")
