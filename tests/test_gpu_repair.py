"""Collision repair on the device (csrc/repair.hpp; jmid_repair_collisions) against its NumPy twin (``metrics.repair_collisions_host``;
tests/test_repair_host.py pins the twin itself and the stability of these inputs under the one operation that differs, exp): states,
iteration counts and episode rows equal, positions and velocities within one fp32 unit in the last place; then the properties of the
rule on the device's own output, the resident set, and the Python layer against the staged composition by hand."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from safe_interactive_crowdnav_amd import _lib, metrics, offline
from safe_interactive_crowdnav_amd import scene as SC
from safe_interactive_crowdnav_amd.engine import JmidError
from safe_interactive_crowdnav_amd.forecaster import predict_batch, rank_samples, repair_totals
from tests.repair_cases import THRESHOLD, gpu_cases
from tests.test_gpu_noise import GOLDEN, engine_for, make_forecaster, same_bits
from tests.test_gpu_rejection import SEED, inputs, mixed_threshold, to_np
from tests.test_scene_device_inputs import DT, random_positions

DTV = 0.25
_TWIN = {}


def case(name):
    """(pos, p0, vel, the twin's four outputs), the twin computed once per input."""
    if name not in _TWIN:
        pos, p0 = gpu_cases()[name]
        if name == "e2a3k5t3":       # a sample that cannot be judged rides along: state 3, untouched
            pos = pos.copy()
            pos[1, 4, 2, 1, 0] = np.nan
        prev = np.concatenate([np.broadcast_to(p0[:, None, :, None], pos[:, :, :, :1].shape), pos[:, :, :, :-1]], axis=3)
        vel = ((pos - prev) / np.float32(DTV)).astype(np.float32)
        _TWIN[name] = (pos, p0, vel, metrics.repair_collisions_host(pos, THRESHOLD, p0=p0, dt=DTV, vel=vel))
    return _TWIN[name]


def ulps(a, b):
    a, b = (np.ascontiguousarray(to_np(v), dtype=np.float32).view(np.int32).astype(np.int64) for v in (a, b))
    return int(np.abs(a - b).max())


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("name", ["e2a3k5t3", "a2t2k1", "k300", "a64t2k1", "a64t24k1"])
def test_equals_the_twin(name, device):
    eng = engine_for()
    pos, p0, vel, (want, want_vel, want_sample, want_episode) = case(name)
    assert want_episode[:, 1].sum() >= 1
    args = [torch.from_numpy(a).cuda() for a in (pos, p0, vel)] if device else [pos, p0, vel]
    out, vel_out, sample, episode = eng.repair_collisions(args[0], THRESHOLD, p0=args[1], dt=DTV, vel=args[2])
    out, vel_out, sample, episode = (to_np(a) for a in (out, vel_out, sample, episode))
    state = sample[..., 3]
    print(f"{name}: states {np.bincount(state.astype(int).ravel(), minlength=4).tolist()}, episodes {episode.tolist()}, positions "
          f"{ulps(out, want)} ulp, velocities {ulps(np.nan_to_num(vel_out), np.nan_to_num(want_vel))} ulp from the twin")
    assert np.array_equal(state, want_sample[..., 3]) and np.array_equal(sample[..., 2], want_sample[..., 2])
    assert np.array_equal(episode, want_episode)
    finite = ~np.isnan(want_sample[..., 0])
    assert np.array_equal(np.isnan(sample[..., :2]), np.isnan(want_sample[..., :2]))
    assert ulps(sample[..., :2][finite], want_sample[..., :2][finite].astype(np.float32)) <= 1
    fixed = state == metrics.REPAIR_REPAIRED
    assert ulps(out[fixed], want[fixed]) <= 1 and ulps(vel_out[fixed], want_vel[fixed]) <= 1
    # untouched, reverted and NaN samples: the input bits, positions and velocities
    assert same_bits(out[~fixed], pos[~fixed]) and same_bits(vel_out[~fixed], vel[~fixed])
    # the statistics entry on the device's own output: every repaired sample is clean
    after = eng.collision_statistics(out, THRESHOLD, agents=False)[2]
    assert not (after[..., 3][fixed] > 0).any() and same_bits(after[..., 0][fixed], sample[..., 1][fixed])
    # the velocities of a repaired sample are those of ITS positions
    prev = np.concatenate([np.broadcast_to(p0[:, None, :, None], out[:, :, :, :1].shape), out[:, :, :, :-1]], axis=3).astype(np.float64)
    assert same_bits(vel_out[fixed], ((out.astype(np.float64) - prev) / DTV).astype(np.float32)[fixed])


def test_thresholds_zero_and_huge_and_the_cap():
    eng = engine_for()
    pos, p0, vel, _ = case("e2a3k5t3")
    out, _, sample, episode = eng.repair_collisions(pos, 0.0)
    assert same_bits(out, pos) and not episode.any() and sample[..., 3].tolist() == [[0] * 5, [0, 0, 0, 0, 3]]
    out, vel_out, sample, episode = eng.repair_collisions(pos, 1e9, p0=p0, dt=DTV, vel=vel)
    assert same_bits(out, pos) and same_bits(vel_out, vel)
    assert sample[..., 3].tolist() == [[2] * 5, [2, 2, 2, 2, 3]] and episode.tolist() == [[5, 0, 32], [4, 0, 32]]
    assert np.isfinite(sample[sample[..., 3] == 2]).all()
    for cap in (0, 1):       # the identity plus the flags; a cap too small to finish: reverted, the input bits
        out, _, sample, episode = eng.repair_collisions(pos, THRESHOLD, max_iter=cap)
        want = metrics.repair_collisions_host(pos, THRESHOLD, max_iter=cap)
        assert same_bits(out, pos) and np.array_equal(sample[..., 2:], want[2][..., 2:]) and np.array_equal(episode, want[3])
        assert episode[:, 1].sum() == 0 and episode[0].tolist() == [2, 0, cap]


def test_padded_counts_equal_the_compacted_episodes():
    eng = engine_for()
    pos, p0 = gpu_cases()["e3a3k6t4"]
    counts = np.array([3, 1, 2], dtype=np.int32)
    padded, vel = pos.copy(), np.full(pos.shape, 7.0, dtype=np.float32)
    for e, n in enumerate(counts):
        padded[e, :, n:] = np.nan
    out, vel_out, sample, episode = eng.repair_collisions(padded, THRESHOLD, p0=p0, dt=DTV, vel=vel, n_agents=counts)
    assert episode[:, 1].sum() >= 2 and episode[1].tolist() == [0, 0, 0]
    for e, n in enumerate(counts):
        alone = eng.repair_collisions(np.ascontiguousarray(pos[e:e + 1, :, :n]), THRESHOLD, p0=np.ascontiguousarray(p0[e:e + 1, :n]), dt=DTV,
                                      vel=np.ascontiguousarray(vel[e:e + 1, :, :n]))
        assert same_bits(out[e, :, :n], alone[0][0]) and same_bits(out[e, :, n:], padded[e, :, n:])
        assert same_bits(vel_out[e, :, :n], alone[1][0]) and same_bits(vel_out[e, :, n:], vel[e, :, n:])
        assert same_bits(sample[e], alone[2][0]) and same_bits(episode[e], alone[3][0])
    want = metrics.repair_collisions_host(padded, THRESHOLD, n_agents=counts)
    assert np.array_equal(sample[..., 2:], want[2][..., 2:]) and np.array_equal(episode, want[3])
    assert same_bits(eng.collision_statistics(out, THRESHOLD, n_agents=counts)[3][:, 0], np.zeros(3, np.float32))


def test_partition_invariance():
    eng = engine_for()
    pos, p0 = gpu_cases()["e5a3k4t4"]
    whole = eng.repair_collisions(pos, THRESHOLD, p0=p0, dt=DTV, vel=np.zeros_like(pos))
    assert (whole[3][:, 1] > 0).sum() >= 3
    for part in ([0, 1], [2, 3, 4], [0], [1], [2], [3], [4]):
        got = eng.repair_collisions(pos[part], THRESHOLD, p0=p0[part], dt=DTV, vel=np.zeros_like(pos[part]))
        for g, w in zip(got, whole):
            assert same_bits(g, w[part]), part


@pytest.mark.parametrize("after", ["denoise", "denoise_reject"])
def test_the_resident_set_is_repaired_in_place(after):
    eng = engine_for()
    eng.set_step(2, "ddim")
    E, A, K, T, k = 4, 3, 5, 3, 2
    ctx, p0 = inputs(E, A)
    ids = [7, 0, 4294967295, 12]
    seeded = dict(seed=SEED, episode_ids=ids, K=K, T=T)

    def draw(thr):
        if after == "denoise":
            return eng.denoise(None, ctx, p0, **seeded)[:2]
        return eng.denoise_reject(ctx, p0, threshold=thr, max_rounds=1, **seeded)[:2]

    thr = mixed_threshold(eng.collision_statistics(draw(0.0)[1], 1.0)[2][..., 0])
    vel, pos = draw(thr)
    want = eng.repair_collisions(pos, thr, p0=p0, dt=DTV, vel=vel)          # (given positions: the resident set is not touched)
    for a, b in zip(eng.collision_statistics(None, thr, dims=(E, A, K, T)), eng.collision_statistics(pos, thr)):
        assert same_bits(a, b)
    assert want[3][:, 0].sum() >= 1, "nothing collides at this threshold"
    print(f"after {after}: threshold {thr:.4f}, episodes {want[3].tolist()}")
    got = eng.repair_collisions(None, thr, dims=(E, A, K, T), want_pos=True)
    assert same_bits(got[0], want[0]) and got[1] is None and same_bits(got[2], want[2]) and same_bits(got[3], want[3])
    for a, b in zip(eng.topk(None, k, dims=(E, A, K, T)), eng.topk(want[0], k)):
        assert same_bits(a, b)
    for a, b in zip(eng.collision_statistics(None, thr, dims=(E, A, K, T)), eng.collision_statistics(want[0], thr)):
        assert same_bits(a, b)
    # a second repair of the repaired set finds only what the first one reverted, and changes nothing
    again = eng.repair_collisions(None, thr, dims=(E, A, K, T), want_pos=True)
    assert same_bits(again[0], want[0]) and np.array_equal(again[3][:, 0], want[3][:, 0] - want[3][:, 1]) and not again[3][:, 1].any()
    # the forgetting rules are those of the other pos = NULL consumers
    eng.denoise(None, ctx, None, want_pos=False, **seeded)
    with pytest.raises(JmidError) as err:
        eng.repair_collisions(None, thr, dims=(E, A, K, T))
    assert err.value.code == _lib.EINVAL


def by_hand(f, thr, x_T=None, rounds=0):
    """The staged composition of one ``predict_ret_best()`` with ``constraint_type="opt_softplus"`` from the engine's entries."""
    F, H, K, k = f.num_hist_frames, f.predict_horizon, f.num_samples, f.num_ret_samples
    hum_xy, rob_xy, pose_now = SC.frame_table(*f._snapshot(), f.time_step, F)
    sb = SC.build_scene(hum_xy, rob_xy, f.time_step, H, F)
    A = len(sb.ids_in)
    ctx = f.engine.encode(sb.x_st, sb.nbr_sum, sb.edge_mask)
    if x_T is not None:
        _, pos = f.engine.denoise(x_T, ctx[None], sb.p0[None], dt=f.time_step, precision="f32")
    else:
        _, pos, _, _ = f.engine.denoise_reject(ctx[None], sb.p0[None], f.noise_seed, [f.episode_id], K, H, dt=f.time_step, precision="f32",
                                               threshold=thr, max_rounds=rounds, draw0=0)
    raw = pos
    pos, _, _, episode = f.engine.repair_collisions(pos, thr)
    rows, logw = rank_samples(f.engine, "device" if k < K else "none", pos, k, (1, A, K, H))
    inc = np.zeros(f.num_hums, dtype=bool)
    inc[sb.ids_in] = True
    return SC.assemble_forecasts(inc, rows[0], None if logw is None else logw[0], sb.cv_forecasts, pose_now, k, K), episode, raw


def test_forecaster_with_constraint_type(tmp_path):
    z = np.load(os.path.join(GOLDEN, "wrapper_jmid_topk.npz"))
    K, H = int(z["K"]), int(z["H"])
    # the reference's torch RNG contract: the repair needs no noise of its own
    plain = make_forecaster(z, tmp_path / "plain", rng_compat="cpu", precision="f32")
    torch.manual_seed(5)
    base = plain.predict_ret_best()
    probe = make_forecaster(z, tmp_path / "probe", rng_compat="cpu", precision="f32")
    A = len(SC.build_scene(*SC.frame_table(*probe._snapshot(), probe.time_step, probe.num_hist_frames)[:2], probe.time_step, H,
                           probe.num_hist_frames).ids_in)
    torch.manual_seed(5)
    x_T = probe._draw_x_T(A)
    thr = mixed_threshold(probe.engine.collision_statistics(by_hand(probe, 0.0, x_T)[2], 1.0)[2][..., 0])
    (want_fc, want_lw), episode, _ = by_hand(probe, thr, x_T)
    f = make_forecaster(z, tmp_path / "a", rng_compat="cpu", precision="f32", constraint_type="opt_softplus", collision_threshold=thr)
    assert f.repair is None
    torch.manual_seed(5)
    fc, lw = f.predict_ret_best()
    print(f"torch contract: threshold {thr:.4f}, repair {f.repair}")
    assert same_bits(fc, want_fc) and same_bits(lw, want_lw) and f.repair == repair_totals(episode) and f.repair[0] >= 1
    assert f.repair[2] == f.repair[0] - f.repair[1]
    # off unless asked for: the plain forecaster's bits
    off = make_forecaster(z, tmp_path / "off", rng_compat="cpu", precision="f32", collision_threshold=thr)
    torch.manual_seed(5)
    again = off.predict_ret_best()
    assert same_bits(again[0], base[0]) and same_bits(again[1], base[1]) and off.repair is None
    # the redraw loop first, the repair on whatever is still flagged: R = 1 + repair against the two entries by hand
    kw = dict(rng_compat="device", seed=17, precision="f32", collision_free_rounds=1, collision_threshold=thr)
    both = make_forecaster(z, tmp_path / "b", constraint_type="opt_softplus", **kw)
    fc, lw = both.predict_ret_best()
    (want_fc, want_lw), episode, _ = by_hand(both, thr, rounds=1)
    print(f"R = 1 + repair: rejection {both.rejection}, repair {both.repair}")
    assert same_bits(fc, want_fc) and same_bits(lw, want_lw) and both.repair == repair_totals(episode)
    assert both.repair[0] == both.rejection[1] - both.rejection[2]           # the repair's candidates: what the loop left flagged


def test_predict_batch_with_constraint_type():
    E, N, K, k, H = 6, 6, 16, 5, 8
    hum, rob = random_positions(E, N, 67, half_width=5.0)
    eng = engine_for()
    eng.set_step(2, "ddim")
    gids = [1000 + 7 * e for e in range(E)]
    kw = dict(num_samples=K, num_ret_samples=k, horizon=H, time_step=DT, precision="f32", collision_threshold=0.5)
    for extra in (dict(noise="device", seed=2024), dict(), dict(noise="device", seed=2024, collision_free_rounds=1),
                  dict(noise="device", seed=2024, collision_free_rounds=1, collision_free_padded=True)):
        stats = {}
        fc, lw, inc = predict_batch(eng, hum, rob, gids, stats=stats, constraint_type="opt_softplus", **kw, **extra)
        counts = inc.sum(axis=1)
        assert len(np.unique(counts)) >= 2, counts
        print(f"{extra}: counts {counts.tolist()}, repair {stats['repair'].tolist()}")
        assert stats["repair"].shape == (E, 3) and stats["repair"][:, 0].sum() >= 1
        if extra.get("collision_free_rounds"):       # the repair takes what the loop left flagged
            assert np.array_equal(stats["repair"][:, 0], stats["episodes"][:, 0] - stats["episodes"][:, 1])
        if extra.get("collision_free_padded"):
            continue                                 # (a padded call's attention rounds differently per batch: no bitwise rule)
        for e in (0, E - 1):
            one = {}
            fc1, lw1, _ = predict_batch(eng, hum[e:e + 1], rob[e:e + 1], gids[e:e + 1], stats=one, constraint_type="opt_softplus", **kw, **extra)
            assert same_bits(fc1[0], fc[e]) and same_bits(lw1[0], lw[e]) and same_bits(one["repair"][0], stats["repair"][e])
    off = predict_batch(eng, hum, rob, gids, noise="device", seed=2024, **kw)
    plain = predict_batch(eng, hum, rob, gids, noise="device", seed=2024, **{a: b for a, b in kw.items() if a != "collision_threshold"})
    assert same_bits(off[0], plain[0]) and same_bits(off[1], plain[1])


def test_offline_generate_with_opt_softplus():
    eng = engine_for()
    B, T, n = 3, 4, 6
    ctx, p0 = inputs(1, B)
    ctx, p0 = ctx[0], p0[0] * 2.0
    call = dict(sampling="ddim", step=2, seed=SEED)
    plain = offline.generate(eng, ctx, p0, 0.25, T, n, True, **call)
    thr = mixed_threshold(eng.collision_statistics(plain[0].reshape(n, 1, B, T, 2), 1.0)[2][..., 0])
    want, _, _, episode = eng.repair_collisions(plain[0].reshape(n, 1, B, T, 2), thr)
    pos, steps, num_iter, colliding, fixed = offline.generate(eng, ctx, p0, 0.25, T, n, True, with_constraints=True, constraint_type="opt_softplus",
                                                              collision_threshold=thr, **call)
    print(f"threshold {thr:.4f}: num_iter {num_iter}, {colliding} colliding, {fixed} repaired")
    assert same_bits(pos, want.reshape(n, B, T, 2)) and steps == plain[1]
    assert (num_iter, colliding, fixed) == (int(episode[:, 2].max()), int(episode[:, 0].sum()), int(episode[:, 1].sum())) and colliding >= 1
    # the torch contract and the DDPM sampler take it too (no seed): the count of colliding samples is that of the plain samples
    torch.manual_seed(3)
    raw = offline.generate(eng, ctx, p0, 0.25, T, n, True, sampling="ddpm", step=2)
    torch.manual_seed(3)
    got = offline.generate(eng, ctx, p0, 0.25, T, n, True, sampling="ddpm", step=2, with_constraints=True, constraint_type="opt_softplus",
                           collision_threshold=thr)
    assert got[3] == int((eng.collision_statistics(raw[0].reshape(n, 1, B, T, 2), thr)[2][..., 3] > 0).sum())
    eng.set_step(2, "ddim")


def test_refusals_of_the_raw_entry():
    eng = engine_for()
    E, A, K, T = 2, 3, 5, 3
    pos, p0, vel, _ = case("e2a3k5t3")
    out, sample = np.empty_like(pos), np.empty((E, K, 4), np.float32)
    vel = vel.copy()
    ptr = lambda a: C.c_void_p(a.ctypes.data) if a is not None else None

    def call(pos=pos, p0=p0, threshold=0.2, margin=0.02, tau=0.005, step=0.02, max_iter=32, pos_out=out, vel_out=None, sample_out=sample, T=T):
        rc = eng._lib.jmid_repair_collisions(eng._h, E, A, K, T, None, ptr(pos), ptr(p0), 0.25, threshold, margin, tau, step, max_iter,
                                             ptr(pos_out), ptr(vel_out), ptr(sample_out), None, _lib.MEM_HOST)
        return rc, eng._lib.jmid_last_error(eng._h).decode()

    assert call()[0] == 0 and call(vel_out=vel)[0] == 0
    for name, kw in (("threshold", dict(threshold=float("inf"))), ("margin", dict(margin=-0.01)), ("tau", dict(tau=0.0)), ("step", dict(step=0.0)),
                     ("max_iter", dict(max_iter=1025)), ("p0", dict(p0=None, vel_out=vel)), ("every output is NULL", dict(pos_out=None, sample_out=None)),
                     ("T", dict(T=1))):
        rc, msg = call(**kw)
        assert rc == _lib.EINVAL and "jmid_repair_collisions" in msg and name in msg, (name, rc, msg)
    eng.encode(*[np.zeros(s, np.float32) for s in ((1, 6, 6), (1, 2, 6, 6), (1, 2))])      # (a host-mode entry of the arena: nothing is resident)
    rc, msg = call(pos=None)
    assert rc == _lib.EINVAL and "pos = NULL" in msg
