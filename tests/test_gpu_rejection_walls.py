"""Collision-free sampling with walls on the device (jmid_denoise_reject_walls_seeded) against a Python loop over entries that exist
next to it - ``engine.noise(draw=)``, ``engine.denoise(x_T)``, ``engine.collision_statistics``, ``engine.wall_statistics`` - and the host
pairing twin (``metrics.fill_slots``), whose callers AND the two predicates.  As in tests/test_gpu_rejection.py the oracle issues the
calls the library issues (it reruns exactly the episodes with bad slots, ascending, as ONE call per round), so every comparison is bit
for bit.  The weights are those of the checkpoint fixture ckpt_ref_jmid_w32.

The wall of a case is placed from the case's own round-0 samples: a long vertical segment right of everybody, at the midpoint of the
widest gap in the central half of "the largest x a sample reaches" plus the radius, so that about half the samples hit it and every
|clearance - radius| is half that gap (asserted: 10-90 % hit, margin >= 1e-6 m)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from safe_interactive_crowdnav_amd import _lib, metrics, offline
from safe_interactive_crowdnav_amd import scene as SC
from safe_interactive_crowdnav_amd.engine import JmidEngine
from safe_interactive_crowdnav_amd.forecaster import predict_batch, rank_samples
from safe_interactive_crowdnav_amd.weights import JMIDWeights, NetDims
from tests.test_gpu_noise import GOLDEN, make_forecaster, same_bits
from tests.test_gpu_rejection import SEED, mixed_threshold, to_np
from tests.test_scene_device_inputs import DT, random_positions

RADIUS = 0.3
MARGIN = 1e-6
NAMES = ("vel", "pos", "slots", "episodes", "cause")


@pytest.fixture(scope="module")
def eng():
    ev = np.load(os.path.join(GOLDEN, "ckpt_ref_jmid_w32_eval.npz"))
    weights = JMIDWeights.from_seed(NetDims(ctx_dim=32), int(ev["wseed"]))
    assert weights.checksum() == str(ev["wsum"])                       # the weights of tests/golden/ckpt_ref_jmid_w32.pt.xz
    e = JmidEngine(weights, joint=True, hist_len=6, step=2)
    yield e
    e.close()


def inputs(E, A, seed=0, device=False):
    """ctx and p0 of E episodes; every episode's p0 is shifted so that its right-most agent stands at x = 0 (the network's velocities do
    not depend on p0): one wall then splits the samples of every episode."""
    g = torch.Generator().manual_seed(seed)
    ctx = torch.randn([E, A, 32], generator=g)
    p0 = 0.6 * torch.randn([E, A, 2], generator=g)
    p0[:, :, 0] -= p0[:, :, 0].max(dim=1, keepdim=True).values
    if device:
        return ctx.cuda(), p0.cuda()
    return ctx.numpy(), p0.numpy()


def reach(pos, p0):
    """[E, K]: the largest x any agent of the sample reaches, its present position included."""
    pos, p0 = to_np(pos), to_np(p0)
    return np.maximum(pos[..., 0].max(axis=(2, 3)), p0[:, None, :, 0].max(axis=2))


def wall_from(pos, p0):
    """The case's wall [1, 4] from its round-0 samples, and the share of them that hits it."""
    x = reach(pos, p0)
    gap = mixed_threshold(x)
    walls = np.array([[gap + RADIUS, -100.0, gap + RADIUS, 100.0]], dtype=np.float64)
    sample = metrics.wall_statistics_host(to_np(pos), walls, RADIUS, p0=to_np(p0))[2]
    share = float((sample[..., 1] > 0).mean())
    margin = float(np.abs(sample[..., 0] - RADIUS).min())
    print(f"wall at x = {gap + RADIUS:.4f}: {share:.2f} of the round-0 samples hit, closest |clearance - radius| {margin:.3e}")
    assert 0.1 <= share <= 0.9 and margin >= MARGIN
    return walls


class Oracle:
    """The loop at ``max_rounds`` = ``rounds`` from the entries next to it, every round's candidates kept: a smaller ``max_rounds`` is a
    prefix of it.  walls None: the pedestrian predicate alone."""

    def __init__(self, eng, ctx, p0, ids, K, T, precision, threshold, walls, radius, rounds, draw0=0, dt=0.25):
        self.E, self.A, self.K, self.T = int(ctx.shape[0]), int(ctx.shape[1]), K, T
        self.ids = np.asarray(ids, dtype=np.uint32)
        dev = isinstance(ctx, torch.Tensor)
        self.ok = [[] for _ in range(self.E)]          # episode -> round -> bool [K]
        self.cand = [[] for _ in range(self.E)]        # episode -> round -> (vel [K, A, T, 2], pos)
        self.rerun = []                                # round j >= 1 -> the episodes it reran
        for j in range(rounds + 1):
            rows = [e for e in range(self.E) if j == 0 or metrics.fill_slots(self.ok[e])[0][:, 2].any()]
            if not rows:
                break
            x_T = eng.noise(SEED, self.ids[rows], K * self.A, T, draw=draw0 + j, device=dev)
            vel, pos = eng.denoise(x_T, ctx[rows], p0[rows], dt=dt, precision=precision)
            ped = to_np(eng.collision_statistics(pos, threshold, agents=False)[2])
            ok_ped = (ped[..., 3] == 0) & ~np.isnan(ped[..., 0])
            if walls is None:
                ok_wall = np.ones_like(ok_ped)
            else:
                wall = to_np(eng.wall_statistics(pos, walls, radius, p0=p0[rows])[2])
                ok_wall = (wall[..., 1] == 0) & ~np.isnan(wall[..., 0])
            vel, pos = to_np(vel), to_np(pos)
            if j == 0:
                self.pos0, self.min_dist0 = pos.copy(), ped[..., 0].copy()
                self.cause = np.stack([(~ok_ped).sum(axis=1), (~ok_wall).sum(axis=1)], axis=1).astype(np.int32)
            else:
                self.rerun.append(rows)
            for b, e in enumerate(rows):
                self.ok[e].append(ok_ped[b] & ok_wall[b])
                self.cand[e].append((vel[b], pos[b]))

    def result(self, max_rounds):
        E, K, A, T = self.E, self.K, self.A, self.T
        vel, pos = np.empty((E, K, A, T, 2), np.float32), np.empty((E, K, A, T, 2), np.float32)
        slots, episodes = np.empty((E, K, 3), np.int32), np.empty((E, 3), np.int32)
        for e in range(E):
            slots[e], episodes[e] = metrics.fill_slots(self.ok[e][:max_rounds + 1])
            for s in range(K):
                vel[e, s], pos[e, s] = (a[slots[e, s, 1]] for a in self.cand[e][slots[e, s, 0]])
        return vel, pos, slots, episodes, self.cause


def assert_equals(got, want, what=""):
    assert len(got) == len(want)
    for name, g, w in zip(NAMES, got, want):
        assert same_bits(g, w), f"{what}: {name} differs from the oracle"


def case(eng, E, A, K, T, ids, precision, device=False, draw0=0):
    """-> ctx, p0, the pedestrian threshold in the middle of the round-0 clearances, the wall of the round-0 samples."""
    ctx, p0 = inputs(E, A, device=device)
    probe = Oracle(eng, ctx, p0, ids, K, T, precision, 1.0, None, None, 0, draw0)
    return ctx, p0, mixed_threshold(probe.min_dist0), wall_from(probe.pos0, p0)


# ------------------------------------------------------------------------------------------------ 1. L = 0 is the entry without walls
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("precision", ["f32", "f16mx"])
def test_no_walls_is_the_entry_without_walls(eng, precision, device):
    eng.set_step(2, "ddim")
    E, A, K, T, ids = 4, 3, 5, 3, [7, 0, 4294967295, 12]
    ctx, p0 = inputs(E, A, device=device)
    thr = mixed_threshold(Oracle(eng, ctx, p0, ids, K, T, precision, 1.0, None, None, 0).min_dist0)
    for draw0, m in ((0, 0), (0, 3), (5, 2)):
        call = dict(seed=SEED, episode_ids=ids, K=K, T=T, precision=precision, threshold=thr, max_rounds=m, draw0=draw0)
        old = eng.denoise_reject(ctx, p0, **call)
        assert len(old) == 4
        for walls in (np.zeros((0, 4)), np.zeros((0, 2, 2))):
            new = eng.denoise_reject(ctx, p0, walls=walls, wall_radius=RADIUS, **call)
            assert len(new) == 5
            for name, a, b in zip(NAMES, new, old):
                assert same_bits(a, b), (name, draw0, m)
            cause = to_np(new[4])
            assert cause.dtype == np.int32 and not cause[:, 1].any() and (cause[:, 0] == to_np(old[3])[:, 0]).all()
    assert to_np(old[3])[:, 0].sum() >= 1              # (the threshold splits the samples: something was redrawn)


# ------------------------------------------------------------------------------------------------ 2. equality with the oracle
@pytest.mark.parametrize("draw0", [0, 5])
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("precision", ["f32", "f16mx"])
def test_equals_the_oracle(eng, precision, device, draw0):
    eng.set_step(2, "ddim")
    E, A, K, T, ids = 4, 3, 5, 3, [7, 0, 4294967295, 12]
    ctx, p0, thr, walls = case(eng, E, A, K, T, ids, precision, device, draw0)
    call = dict(seed=SEED, episode_ids=ids, K=K, T=T, precision=precision, draw0=draw0, walls=walls, wall_radius=RADIUS)
    # the wall alone (threshold 0: no pedestrian ever collides), then both predicates
    for threshold in (0.0, thr):
        orc = Oracle(eng, ctx, p0, ids, K, T, precision, threshold, walls, RADIUS, 3, draw0)
        e3, e0 = orc.result(3)[3], orc.result(0)[3]
        print(f"threshold {threshold:.4f}: cause {orc.cause.tolist()}, episodes at 3 rounds {e3.tolist()}, reruns {orc.rerun}")
        assert orc.cause[:, 1].sum() >= 1 and (threshold == 0.0) == (orc.cause[:, 0].sum() == 0)
        assert (np.maximum(orc.cause[:, 0], orc.cause[:, 1]) <= e0[:, 0]).all() and (e0[:, 0] <= orc.cause.sum(axis=1)).all()
        assert e3[:, 1].sum() >= 1, "no slot is fixed at max_rounds = 3: the case shows nothing"
        for m in (0, 1, 3):
            got = eng.denoise_reject(ctx, p0, threshold=threshold, max_rounds=m, **call)
            assert_equals(got, orc.result(m), f"threshold {threshold}, {m} rounds")
    # a radius no path keeps: every sample hits in every round - the plain call's bits, every flag 1, rounds == max_rounds
    plain = Oracle(eng, ctx, p0, ids, K, T, precision, 0.0, None, None, 0, draw0).result(0)
    for m in (0, 2):
        got = eng.denoise_reject(ctx, p0, threshold=0.0, max_rounds=m, **dict(call, wall_radius=1e6))
        assert same_bits(got[0], plain[0]) and same_bits(got[1], plain[1])
        assert to_np(got[2])[..., 2].all() and (to_np(got[3]) == [K, 0, m]).all() and (to_np(got[4]) == [0, K]).all()


@pytest.mark.parametrize("precision", ["f32", "f16mx"])
def test_many_samples(eng, precision):
    """K = 300 gives every thread of the scan two samples."""
    eng.set_step(2, "ddim")
    E, A, K, T, ids = 2, 2, 300, 2, [10, 11]
    ctx, p0, thr, walls = case(eng, E, A, K, T, ids, precision)
    orc = Oracle(eng, ctx, p0, ids, K, T, precision, thr, walls, RADIUS, 2)
    got = eng.denoise_reject(ctx, p0, seed=SEED, episode_ids=ids, K=K, T=T, precision=precision, threshold=thr, max_rounds=2, walls=walls,
                             wall_radius=RADIUS)
    print(f"K = 300: cause {to_np(got[4]).tolist()}, episodes {to_np(got[3]).tolist()}")
    assert_equals(got, orc.result(2), "K = 300")
    assert orc.cause.sum(axis=0).min() >= 1            # (both predicates reject something)


# ------------------------------------------------------------------------------------------------ 3. partition invariance
@pytest.mark.parametrize("precision", ["f32", "f16mx"])
def test_partition_invariance(eng, precision):
    """Every episode's rows of all five outputs: the same bits in the batch of six, as 3 + 3 and as 1 + 5 (head_dim 16)."""
    eng.set_step(2, "ddim")
    E, A, K, T = 6, 2, 3, 4
    ids = np.array([9, 3, 4000000000, 0, 17, 5], dtype=np.uint32)
    ctx, p0, thr, walls = case(eng, E, A, K, T, ids, precision)
    call = dict(seed=SEED, K=K, T=T, precision=precision, threshold=thr, max_rounds=3, walls=walls, wall_radius=RADIUS)
    whole = eng.denoise_reject(ctx, p0, episode_ids=ids, **call)
    print(f"threshold {thr:.4f}: cause {whole[4].tolist()}, episodes {whole[3].tolist()}")
    assert whole[3][:, 1].sum() >= 1 and whole[4][:, 1].sum() >= 1
    for part in ([0, 1, 2], [3, 4, 5], [0], [1, 2, 3, 4, 5]):
        got = eng.denoise_reject(ctx[part], p0[part], episode_ids=ids[part], **call)
        for name, g, w in zip(NAMES, got, whole):
            assert same_bits(g, w[part]), (name, part)


def test_captured_loop_gives_the_same_bits(eng):
    """The "graph" knob (diagnostics flavour): the reruns of one episode are calls of one shape, captured and replayed.  The same bits
    with the knob on and off, the wall kernel next to them."""
    eng.set_step(2, "ddim")
    ctx, p0 = inputs(1, 3)
    walls = np.array([[0.5, -100.0, 0.5, 100.0]])
    call = dict(seed=SEED, episode_ids=[21], K=5, T=3, threshold=0.0, max_rounds=3, walls=walls, wall_radius=1e6)    # (every round reruns)
    off = eng.denoise_reject(ctx, p0, **call)
    assert (off[3] == [5, 0, 3]).all() and (off[4] == [0, 5]).all()
    eng.set_tuning("graph", 1)
    try:
        before = eng.graph_replays()
        for _ in range(2):
            on = eng.denoise_reject(ctx, p0, **call)
            for a, b in zip(on, off):
                assert same_bits(a, b)
        assert eng.graph_replays() > before
    finally:
        eng.set_tuning("graph", 0)


# ------------------------------------------------------------------------------------------------ 4. the resident accepted set
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_accepted_set_is_what_the_wall_statistics_see(eng, device):
    eng.set_step(2, "ddim")
    E, A, K, T, ids = 4, 3, 5, 3, [7, 0, 4294967295, 12]
    ctx, p0, thr, walls = case(eng, E, A, K, T, ids, "f32", device)
    _, pos, slots, episodes, _ = eng.denoise_reject(ctx, p0, seed=SEED, episode_ids=ids, K=K, T=T, threshold=thr, max_rounds=3, walls=walls,
                                                    wall_radius=RADIUS)
    assert to_np(episodes)[:, 1].sum() >= 1          # (the accepted set differs from the last rerun's output)
    resident = eng.wall_statistics(None, walls, RADIUS, p0=p0, dims=(E, A, K, T))
    for a, b in zip(resident, eng.wall_statistics(pos, walls, RADIUS, p0=p0)):
        assert same_bits(a, b)
    # a slot is flagged exactly when its accepted sample fails one of the two predicates
    ped = to_np(eng.collision_statistics(None, thr, dims=(E, A, K, T))[2])
    wall = to_np(resident[2])
    bad = ~((ped[..., 3] == 0) & ~np.isnan(ped[..., 0]) & (wall[..., 1] == 0) & ~np.isnan(wall[..., 0]))
    np.testing.assert_array_equal(to_np(slots)[..., 2], bad.astype(np.int32))


# ------------------------------------------------------------------------------------------------ 5. refusals through the raw ABI
def test_refusals_of_the_raw_entry(eng):
    eng.set_step(2, "ddim")
    E, A, K, T = 2, 2, 3, 3
    ctx, p0 = inputs(E, A)
    ids = np.array([1, 2], dtype=np.uint32)
    vel, pos = np.empty((E, K, A, T, 2), np.float32), np.empty((E, K, A, T, 2), np.float32)
    ok_walls = np.array([[5.0, -1.0, 5.0, 1.0], [6.0, 0.0, 6.0, 0.0]])
    ptr = lambda a: C.c_void_p(a.ctypes.data)

    def call(T=T, p0=p0, threshold=0.2, max_rounds=1, L=2, walls=ok_walls, radius=RADIUS):
        rc = eng._lib.jmid_denoise_reject_walls_seeded(eng._h, E, A, K, T, SEED, ptr(ids), 0, ptr(ctx), ptr(p0) if p0 is not None else None, 0.25,
                                                       _lib.PREC_F32, threshold, max_rounds, L, ptr(walls) if walls is not None else None,
                                                       radius, ptr(vel), ptr(pos), None, None, None, _lib.MEM_HOST)
        return rc, eng._lib.jmid_last_error(eng._h).decode()

    assert call()[0] == 0 and call(L=0, walls=None)[0] == 0
    bad_walls = ok_walls.copy()
    bad_walls[1, 3] = np.inf
    for name, kw in (("p0", dict(p0=None)), ("T", dict(T=1)), ("max_rounds", dict(max_rounds=65)), ("threshold", dict(threshold=float("nan"))),
                     ("radius", dict(radius=-0.1)), ("radius", dict(radius=float("nan"))), ("64", dict(L=65)), ("walls", dict(walls=None)),
                     ("non-finite", dict(walls=bad_walls))):
        rc, msg = call(**kw)
        assert rc == _lib.EINVAL and "jmid_denoise_reject_walls_seeded" in msg and name in msg, (name, rc, msg)
    eng.set_step(10, "ddpm")
    try:
        rc, msg = call()
        assert rc == _lib.EINVAL and "DDIM" in msg
    finally:
        eng.set_step(2, "ddim")


# ------------------------------------------------------------------------------------------------ 6. end to end
def clear_of(rows, p0, walls, radius):
    """rows [k, A, H, 2] returned samples, p0 [A, 2] -> [k] bool: the sample's clearance by the host twin is at least the radius."""
    sample = metrics.wall_statistics_host(rows[None], walls, radius, p0=p0[None])[2][0]
    return sample[:, 0] - radius >= 0


def by_hand(f, thr, walls, R, draw0):
    """The staged composition of one ``predict_ret_best()`` with walls from the engine's entries."""
    F, H, K, k = f.num_hist_frames, f.predict_horizon, f.num_samples, f.num_ret_samples
    hum_xy, rob_xy, pose_now = SC.frame_table(*f._snapshot(), f.time_step, F)
    sb = SC.build_scene(hum_xy, rob_xy, f.time_step, H, F)
    A = len(sb.ids_in)
    ctx = f.engine.encode(sb.x_st, sb.nbr_sum, sb.edge_mask)
    kw = {} if walls is None else dict(walls=walls, wall_radius=RADIUS)
    out = f.engine.denoise_reject(ctx[None], sb.p0[None], f.noise_seed, [f.episode_id], K, H, dt=f.time_step, precision="f32", threshold=thr,
                                  max_rounds=R, draw0=draw0, **kw)
    rows, logw = rank_samples(f.engine, "device_resident" if k < K else "none", out[1], k, (1, A, K, H))
    inc = np.zeros(f.num_hums, dtype=bool)
    inc[sb.ids_in] = True
    return SC.assemble_forecasts(inc, rows[0], None if logw is None else logw[0], sb.cv_forecasts, pose_now, k, K), out, sb


def test_offline_generate_with_walls(eng):
    """The offline form: sample i is episode i with K = 1, the context shared - the oracle's positions and the reference's three counts,
    a sample counting when it fails either predicate."""
    B, T, n = 3, 4, 12
    ctx, p0 = inputs(1, B)
    ctx, p0 = ctx[0], p0[0]
    eng.set_step(2, "ddim")
    ctx_e, p0_e = np.ascontiguousarray(np.broadcast_to(ctx, (n, B, 32))), np.ascontiguousarray(np.broadcast_to(p0, (n, B, 2)))
    probe = Oracle(eng, ctx_e, p0_e, np.arange(n), 1, T, "f32", 1.0, None, None, 0)
    # (the n samples of the offline form are the K of one scene: the wall from their reach, as everywhere above)
    walls = wall_from(probe.pos0.reshape(1, n, B, T, 2), p0[None])
    orc = Oracle(eng, ctx_e, p0_e, np.arange(n), 1, T, "f32", 0.0, walls, RADIUS, 3)
    _, want, _, episodes, cause = orc.result(3)
    pos, steps, num_iter, colliding, fixed = offline.generate(eng, ctx, p0, 0.25, T, n, True, sampling="ddim", step=2, seed=SEED,
                                                              with_constraints=True, collision_threshold=0.0, max_rounds=3,
                                                              static_obstacles=walls, wall_radius=RADIUS)
    print(f"num_iter {num_iter}, {colliding} samples hit, {fixed} fixed")
    assert same_bits(pos, want.reshape(n, B, T, 2)) and steps == n * 3
    assert (num_iter, colliding, fixed) == metrics.rejection_totals(episodes) and colliding == cause[:, 1].sum() >= 1 and fixed >= 1


def test_forecaster_with_walls(tmp_path):
    z = np.load(os.path.join(GOLDEN, "wrapper_jmid_topk.npz"))
    kw = dict(rng_compat="device", seed=17, precision="f32")
    probe = make_forecaster(z, tmp_path / "probe", **kw)
    _, out0, sb = by_hand(probe, 0.0, None, 0, 0)
    walls = wall_from(out0[1], sb.p0[None])
    f = make_forecaster(z, tmp_path / "a", collision_free_rounds=2, collision_threshold=0.0, static_obstacles=walls.reshape(-1, 2, 2),
                        wall_radius=RADIUS, **kw)
    assert f.rejection is None
    fc, lw = f.predict_ret_best()
    (want_fc, want_lw), (_, pos, slots, episodes, cause), sb = by_hand(f, 0.0, walls, 2, 0)
    assert same_bits(fc, want_fc) and same_bits(lw, want_lw)
    assert f.rejection == metrics.rejection_totals(episodes, cause) and len(f.rejection) == 5
    print(f"rejection {f.rejection}, flags {slots[0, :, 2].tolist()}")
    assert f.rejection[4] >= 1 and f.rejection[3] == 0 and f.rejection[2] >= 1      # walls only: some sample hit, and was fixed
    # every returned sample that comes from an unflagged slot keeps its distance from the wall
    ret = np.ascontiguousarray(fc[sb.ids_in][:, :, 1:].transpose(1, 0, 2, 3)).astype(np.float32)       # [k, A, H, 2]
    clear = clear_of(ret, sb.p0, walls, RADIUS)
    for j in range(ret.shape[0]):
        slot = [s for s in range(pos.shape[1]) if same_bits(pos[0, s], ret[j])]
        assert slot, "a returned sample is not in the accepted set"
        assert clear[j] or slots[0, slot[0], 2] == 1, (j, slot)
    assert clear.any()
    # without the keywords: the forecaster without walls, five counts become three
    g = make_forecaster(z, tmp_path / "b", collision_free_rounds=2, collision_threshold=0.0, **kw)
    g.predict_ret_best()
    assert len(g.rejection) == 3


@pytest.mark.parametrize("device_frames", [False, True], ids=["host_scene", "device_frames"])
def test_predict_batch_with_walls(eng, device_frames):
    E, N, K, k, H = 6, 6, 16, 5, 8
    hum, rob = random_positions(E, N, 67, half_width=5.0)
    eng.set_step(2, "ddim")
    gids = [1000 + 7 * e for e in range(E)]
    kw = dict(num_samples=K, num_ret_samples=k, horizon=H, time_step=DT, precision="f32", device_frames=device_frames, noise="device",
              seed=2024, collision_free_rounds=2, collision_threshold=0.2)
    stats, plain = {}, {}
    fc0, lw0, inc0 = predict_batch(eng, hum, rob, gids, stats=plain, **kw)
    # the wall: a long vertical segment that about half of the samples returned for the first episode with a cluster reach
    first = int(np.argmax(inc0.any(axis=1)))
    gap = mixed_threshold(fc0[first, inc0[first]][..., 0].max(axis=(0, 2)))
    walls = np.array([[[gap + RADIUS, -100.0], [gap + RADIUS, 100.0]]])
    fc, lw, inc = predict_batch(eng, hum, rob, gids, stats=stats, static_obstacles=walls, wall_radius=RADIUS, **kw)
    np.testing.assert_array_equal(inc, inc0)
    print(f"wall at x = {gap + RADIUS:.4f} (episode {first}), counts {inc.sum(axis=1).tolist()}, episodes {stats['episodes'].tolist()}, "
          f"cause {stats['cause'].tolist()}")
    assert stats["cause"].shape == (E, 2) and "cause" not in plain
    np.testing.assert_array_equal(stats["cause"][:, 0], plain["episodes"][:, 0])          # round 0 is the same draw: the same pedestrian count
    assert stats["cause"][:, 1].sum() >= 1 and not same_bits(fc, fc0)
    # an episode without a flagged slot returns only samples that keep their distance from every wall
    checked = 0
    for e in range(E):
        if stats["slots"][e, :, 2].any() or not inc[e].any():
            continue
        ret = np.ascontiguousarray(fc[e, inc[e]][:, :, 1:].transpose(1, 0, 2, 3)).astype(np.float32)
        assert clear_of(ret, hum[e, -1, inc[e]].astype(np.float32), walls, RADIUS).all(), e
        checked += stats["cause"][e, 1] > 0
    assert checked >= 1, "no episode was cleared of its wall hits: the case shows nothing"
    for e in (0, E - 1):
        one = {}
        fc1, lw1, _ = predict_batch(eng, hum[e:e + 1], rob[e:e + 1], gids[e:e + 1], stats=one, static_obstacles=walls, wall_radius=RADIUS, **kw)
        assert same_bits(fc1[0], fc[e]) and same_bits(lw1[0], lw[e]), f"episode {e}: the forecasts depend on the batch"
        assert same_bits(one["cause"][0], stats["cause"][e]) and same_bits(one["slots"][0], stats["slots"][e])
