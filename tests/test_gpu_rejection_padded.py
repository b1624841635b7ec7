"""Collision-free sampling of a padded batch on the device (jmid_denoise_reject_padded_seeded) against a Python loop over the entries
next to it - ``engine.noise(n_agents=, draw=)``, ``engine.denoise(x_T, n_agents=)``, ``engine.collision_statistics(n_agents=)``,
``engine.wall_statistics(n_agents=)`` - and the host pairing twin (``metrics.fill_slots``).  As in tests/test_gpu_rejection.py the oracle
issues the calls the library issues: it reruns exactly the episodes with bad slots, ascending, with THEIR counts, as ONE padded call per
round at the call's A.  Every comparison is bit for bit and no margin is needed."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from safe_interactive_crowdnav_amd import _lib, metrics
from safe_interactive_crowdnav_amd import scene as SC
from safe_interactive_crowdnav_amd.forecaster import predict_batch
from tests.test_gpu_noise import engine_for, same_bits
from tests.test_gpu_rejection import SEED, SPREAD, mixed_threshold, to_np
from tests.test_scene_device_inputs import DT, random_positions

NAMES = ("vel", "pos", "slots", "episodes", "cause")
RADIUS = 0.3
MARGIN = 1e-6
# the main shape, and the shape whose key tiles are wholly padded (S = K A T = 192 keys, 4 of every 24 real in the second episode)
MAIN = (4, 3, (3, 1, 2, 3), 5, 3, [7, 0, 4294967295, 12])
TILES = (2, 6, (6, 1), 4, 8, [3, 9])
# the input seeds of the mixed-threshold and of the walls case.  Their preconditions (asserted below) are conditions on the ORACLE and
# can only be evaluated on a GPU.  Seeds tried, 0 .. 7, each for both nets, both precisions, both memory modes and both draw0.  Mixed
# case: 0 fails at draw0 = 0 (the rerun lists never hold the two-agent episode: one count per list), 1 and 6 fail (no slot is ever
# fixed), 2, 3, 4, 5 and 7 meet them.  Walls case: 0 fails (the one-agent episode hits no wall at round 0), 1 .. 7 meet them.
INPUT_SEED = 2
WALL_SEED = 2
PLAIN_SEED = 0       # the other cases (their own assertions say what they need: something is rerun, something is fixed)


def inputs(E, A, counts, seed=INPUT_SEED, device=False, fill=np.nan, align=False):
    """ctx [E, A, 32] and p0 [E, A, 2]; the episodes differ in how close their agents start (tests/test_gpu_rejection.py), the padded
    agents' rows hold ``fill``.  align: every episode's right-most REAL agent stands at x = 0, so that one wall splits every episode."""
    g = torch.Generator().manual_seed(seed)
    ctx = torch.randn([E, A, 32], generator=g)
    p0 = torch.randn([E, A, 2], generator=g) * torch.tensor(SPREAD[:E])[:, None, None]
    for e, n in enumerate(counts):
        if align:
            p0[e, :, 0] -= p0[e, :n, 0].max()
        ctx[e, n:], p0[e, n:] = fill, fill
    if device:
        return ctx.cuda(), p0.cuda()
    return ctx.numpy(), p0.numpy()


class Oracle:
    """The padded loop at ``max_rounds`` = ``rounds`` from the entries next to it, every round's candidates kept: a smaller
    ``max_rounds`` is a prefix of it.  walls None: the pedestrian predicate alone."""

    def __init__(self, eng, ctx, p0, counts, ids, K, T, precision, threshold, rounds, draw0=0, walls=None, radius=None, dt=0.25):
        self.E, self.A, self.K, self.T = int(ctx.shape[0]), int(ctx.shape[1]), K, T
        self.n = np.asarray(counts, dtype=np.int32)
        self.ids = np.asarray(ids, dtype=np.uint32)
        dev = isinstance(ctx, torch.Tensor)
        self.ok = [[] for _ in range(self.E)]          # episode -> round -> bool [K]
        self.cand = [[] for _ in range(self.E)]        # episode -> round -> (vel [K, A, T, 2], pos)
        self.rerun = []                                # round j >= 1 -> the episodes it reran
        for j in range(rounds + 1):
            rows = [e for e in range(self.E) if j == 0 or metrics.fill_slots(self.ok[e])[0][:, 2].any()]
            if not rows:
                break
            n = self.n[rows]
            x_T = eng.noise(SEED, self.ids[rows], K * self.A, T, draw=draw0 + j, device=dev, n_agents=n, A=self.A)
            vel, pos = eng.denoise(x_T, ctx[rows], p0[rows], dt=dt, precision=precision, n_agents=n)
            ped = to_np(eng.collision_statistics(pos, threshold, agents=False, n_agents=n)[2])
            ok_ped = (ped[..., 3] == 0) & ~np.isnan(ped[..., 0])
            if walls is None:
                ok_wall = np.ones_like(ok_ped)
            else:
                wall = to_np(eng.wall_statistics(pos, walls, radius, p0=p0[rows], n_agents=n)[2])
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
    assert len(got) == len(want) == 5
    for name, g, w in zip(NAMES, got, want):
        assert same_bits(g, w), f"{what}: {name} differs from the oracle"


def clearance_threshold(orc):
    """``mixed_threshold`` on the oracle's round-0 clearances (an episode with one agent has none: its min_dist is +inf)."""
    return mixed_threshold(orc.min_dist0[orc.n >= 2])


def wall_from(orc, p0):
    """The case's wall [1, 4] from the oracle's round-0 samples, as tests/test_gpu_rejection_walls.py places it: a long vertical segment
    at the midpoint of the widest gap in the central half of "the largest x a real agent of the sample reaches", plus the radius."""
    pos, p0 = orc.pos0, to_np(p0)
    x = np.stack([np.maximum(pos[e, :, :n, :, 0].max(axis=(1, 2)), p0[e, :n, 0].max()) for e, n in enumerate(orc.n)])
    gap = mixed_threshold(x)
    walls = np.array([[gap + RADIUS, -100.0, gap + RADIUS, 100.0]], dtype=np.float64)
    sample = metrics.wall_statistics_host(pos, walls, RADIUS, p0=p0, n_agents=orc.n)[2]
    share, margin = float((sample[..., 1] > 0).mean()), float(np.abs(sample[..., 0] - RADIUS).min())
    print(f"wall at x = {gap + RADIUS:.4f}: {share:.2f} of the round-0 samples hit, closest |clearance - radius| {margin:.3e}")
    assert 0.1 <= share <= 0.9 and margin >= MARGIN
    return walls


# ------------------------------------------------------------------------------------------------ 1. equality with the oracle
@pytest.mark.parametrize("draw0", [0, 5])
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("precision", ["f32", "f16mx"])
@pytest.mark.parametrize("joint", [True, False], ids=["jmid", "imid"])
def test_equals_the_oracle(joint, precision, device, draw0):
    eng = engine_for(joint)
    e0 = eng.erange_count()
    eng.set_step(2, "ddim")
    E, A, counts, K, T, ids = MAIN
    ctx, p0 = inputs(E, A, counts, device=device)
    call = dict(seed=SEED, episode_ids=ids, K=K, T=T, precision=precision, draw0=draw0, n_agents=counts)
    orc = lambda thr, m: Oracle(eng, ctx, p0, counts, ids, K, T, precision, thr, m, draw0)
    # threshold 0: nothing ever collides - no rerun; max_rounds = 0 at draw0 = 0 is jmid_denoise_padded_seeded (equality 2)
    for m in (0, 3):
        got = eng.denoise_reject(ctx, p0, threshold=0.0, max_rounds=m, **call)
        assert_equals(got, orc(0.0, m).result(m), f"threshold 0, {m} rounds")
        assert not to_np(got[3]).any() and not to_np(got[2])[..., 2].any() and not to_np(got[4]).any()
        assert np.isnan(to_np(got[1])[1, :, 1:]).all() and np.isfinite(to_np(got[1])[1, :, 0]).all()
        if draw0 == 0:
            v0, q0 = eng.denoise_padded_seeded(ctx, p0, counts, SEED, ids, K, T, precision=precision)
            assert same_bits(got[0], v0) and same_bits(got[1], q0)
    # threshold 1e9: every slot of every episode with two agents or more stays flagged; the one-agent episode is never rerun
    plain = orc(1e9, 0).result(0)
    many = np.asarray(counts) >= 2
    for m in (0, 2):
        got = eng.denoise_reject(ctx, p0, threshold=1e9, max_rounds=m, **call)
        assert_equals(got, orc(1e9, m).result(m), f"threshold 1e9, {m} rounds")
        assert same_bits(got[0], plain[0]) and same_bits(got[1], plain[1])
        slots, episodes = to_np(got[2]), to_np(got[3])
        assert slots[many][..., 2].all() and (episodes[many] == [K, 0, m]).all()
        assert not slots[~many][..., 2].any() and not episodes[~many].any()
    # a threshold in the middle of the oracle's own round-0 clearances
    thr = clearance_threshold(orc(1.0, 0))
    o3 = orc(thr, 3)
    _, _, _, e3, _ = o3.result(3)
    print(f"threshold {thr:.4f}: episodes at 3 rounds {e3.tolist()}, reruns {o3.rerun}")
    # the preconditions, on the oracle alone
    assert o3.rerun and (e3[:, 2] > 0).any(), "no episode is rerun: choose another INPUT_SEED"
    assert (e3[:, 2] == 0).any(), "every episode is rerun: choose another INPUT_SEED"
    assert e3[:, 1].sum() >= 1, "no slot is fixed at max_rounds = 3: choose another INPUT_SEED"
    assert any(len({counts[e] for e in rows}) >= 2 for rows in o3.rerun), "no rerun list holds two different counts: choose another INPUT_SEED"
    # (equality 3: a slot fixed in round j holds a candidate of the oracle's ONE padded call on the gathered rows and counts of round j)
    for m in (0, 1, 3):
        assert_equals(eng.denoise_reject(ctx, p0, threshold=thr, max_rounds=m, **call), o3.result(m), f"threshold {thr}, {m} rounds")
    assert eng.erange_count() == e0


@pytest.mark.parametrize("precision", ["f32", "f16mx"])
@pytest.mark.parametrize("joint", [True, False], ids=["jmid", "imid"])
def test_wholly_padded_key_tiles(joint, precision):
    """(6, 1) agents at T = 8: most 32-key tiles of the second episode hold no real key, and a rerun may hold that episode alone."""
    eng = engine_for(joint)
    eng.set_step(2, "ddim")
    E, A, counts, K, T, ids = TILES
    ctx, p0 = inputs(E, A, counts, seed=PLAIN_SEED, align=True)
    probe = Oracle(eng, ctx, p0, counts, ids, K, T, precision, 1.0, 0)
    thr, walls = mixed_threshold(probe.min_dist0[0]), wall_from(probe, p0)
    for w in (None, walls):
        orc = Oracle(eng, ctx, p0, counts, ids, K, T, precision, thr, 3, 0, w, None if w is None else RADIUS)
        got = eng.denoise_reject(ctx, p0, seed=SEED, episode_ids=ids, K=K, T=T, precision=precision, threshold=thr, max_rounds=3, n_agents=counts,
                                 walls=w, wall_radius=None if w is None else RADIUS)
        print(f"walls {w is not None}: cause {orc.cause.tolist()}, episodes {to_np(got[3]).tolist()}, reruns {orc.rerun}")
        assert_equals(got, orc.result(3), f"walls {w is not None}")
        assert orc.rerun                                   # (something was rerun)


# ------------------------------------------------------------------------------------------------ 2. walls
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("precision", ["f32", "f16mx"])
def test_walls(precision, device):
    """Both predicates.  The one-agent episode can only fail on walls: it is rerun for that cause alone, and cause_out says so."""
    eng = engine_for()
    e0 = eng.erange_count()
    eng.set_step(2, "ddim")
    E, A, counts, K, T, ids = MAIN
    ctx, p0 = inputs(E, A, counts, seed=WALL_SEED, device=device, align=True)
    probe = Oracle(eng, ctx, p0, counts, ids, K, T, precision, 1.0, 0)
    thr, walls = clearance_threshold(probe), wall_from(probe, p0)
    call = dict(seed=SEED, episode_ids=ids, K=K, T=T, precision=precision, n_agents=counts, walls=walls, wall_radius=RADIUS)
    for threshold in (0.0, thr):
        orc = Oracle(eng, ctx, p0, counts, ids, K, T, precision, threshold, 3, 0, walls, RADIUS)
        e3 = orc.result(3)[3]
        print(f"threshold {threshold:.4f}: cause {orc.cause.tolist()}, episodes at 3 rounds {e3.tolist()}, reruns {orc.rerun}")
        assert orc.cause[1, 0] == 0 and orc.cause[1, 1] >= 1, "the one-agent episode hits no wall at round 0: choose another WALL_SEED"
        assert e3[1, 2] >= 1 and any(1 in rows for rows in orc.rerun)
        assert (threshold == 0.0) == (orc.cause[:, 0].sum() == 0)
        for m in (0, 1, 3):
            got = eng.denoise_reject(ctx, p0, threshold=threshold, max_rounds=m, **call)
            assert_equals(got, orc.result(m), f"threshold {threshold}, {m} rounds")
            assert (to_np(got[4])[1] == orc.cause[1]).all()
    assert eng.erange_count() == e0


# ------------------------------------------------------------------------------------------------ 3. the stated equalities
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("precision", ["f32", "f16mx"])
@pytest.mark.parametrize("joint", [True, False], ids=["jmid", "imid"])
def test_every_count_equal_to_A_is_the_walls_entry(joint, precision, device):
    """Equality 1: all five outputs, bit for bit, with and without walls."""
    eng = engine_for(joint)
    eng.set_step(2, "ddim")
    E, A, _, K, T, ids = MAIN
    full = (A,) * E
    ctx, p0 = inputs(E, A, full, seed=PLAIN_SEED, device=device, align=True)
    probe = Oracle(eng, ctx, p0, full, ids, K, T, precision, 1.0, 0)
    thr, walls = clearance_threshold(probe), wall_from(probe, p0)
    for draw0, m, w in ((0, 3, walls), (5, 2, walls), (0, 3, np.zeros((0, 4)))):
        call = dict(seed=SEED, episode_ids=ids, K=K, T=T, precision=precision, threshold=thr, max_rounds=m, draw0=draw0, walls=w, wall_radius=RADIUS)
        old, new = eng.denoise_reject(ctx, p0, **call), eng.denoise_reject(ctx, p0, n_agents=full, **call)
        for name, a, b in zip(NAMES, new, old):
            assert same_bits(a, b), (name, draw0, m)
    assert to_np(old[3])[:, 0].sum() >= 1                  # (something was redrawn)


@pytest.mark.parametrize("precision", ["f32", "f16mx"])
def test_an_episode_does_not_depend_on_its_batch_mates(precision):
    """Equality 4: every episode's rows of all five outputs are the same bits in the whole batch, in a 2 + 2 split and alone, at the
    call's A (head_dim 16) - also when the part's largest count is smaller than A."""
    eng = engine_for()
    eng.set_step(2, "ddim")
    E, A, counts, K, T, ids = MAIN
    counts, ids = np.asarray(counts, dtype=np.int32), np.asarray(ids, dtype=np.uint32)
    ctx, p0 = inputs(E, A, counts, seed=WALL_SEED, align=True)
    probe = Oracle(eng, ctx, p0, counts, ids, K, T, precision, 1.0, 0)
    thr, walls = clearance_threshold(probe), wall_from(probe, p0)
    call = dict(seed=SEED, K=K, T=T, precision=precision, threshold=thr, max_rounds=3, walls=walls, wall_radius=RADIUS)
    whole = eng.denoise_reject(ctx, p0, episode_ids=ids, n_agents=counts, **call)
    assert whole[3][:, 1].sum() >= 1                       # (something was fixed)
    for part in ([0, 1], [2, 3], [1, 2], [0], [1], [2], [3]):
        got = eng.denoise_reject(ctx[part], p0[part], episode_ids=ids[part], n_agents=counts[part], **call)
        for name, g, w in zip(NAMES, got, whole):
            assert same_bits(g, w[part]), (name, part)


# ------------------------------------------------------------------------------------------------ 4. the resident accepted set
def test_accepted_set_is_resident():
    eng = engine_for()
    eng.set_step(2, "ddim")
    E, A, counts, K, T, ids = MAIN
    ctx, p0 = inputs(E, A, counts, seed=PLAIN_SEED)
    thr = clearance_threshold(Oracle(eng, ctx, p0, counts, ids, K, T, "f32", 1.0, 0))
    _, pos, _, episodes, _ = eng.denoise_reject(ctx, p0, seed=SEED, episode_ids=ids, K=K, T=T, threshold=thr, max_rounds=3, n_agents=counts)
    assert episodes[:, 1].sum() >= 1                       # (the accepted set differs from the last rerun's output)
    dims = (E, A, K, T)
    for a, b in zip(eng.topk(None, 2, dims=dims, n_agents=counts), eng.topk(pos, 2, n_agents=counts)):
        assert same_bits(a, b)
    for a, b in zip(eng.collision_statistics(None, thr, dims=dims, n_agents=counts), eng.collision_statistics(pos, thr, n_agents=counts)):
        assert same_bits(a, b)
    walls = np.array([[0.0, -5.0, 0.0, 5.0]])
    for a, b in zip(eng.wall_statistics(None, walls, RADIUS, p0=p0, dims=dims, n_agents=counts),
                    eng.wall_statistics(pos, walls, RADIUS, p0=p0, n_agents=counts)):
        assert same_bits(a, b)


# ------------------------------------------------------------------------------------------------ 5. refusals through the raw ABI
def test_refusals_of_the_raw_entry():
    eng = engine_for()
    eng.set_step(2, "ddim")
    E, A, K, T = 2, 2, 3, 3
    ctx, p0 = inputs(E, A, (2, 1))
    ids = np.array([1, 2], dtype=np.uint32)
    vel, pos = np.empty((E, K, A, T, 2), np.float32), np.empty((E, K, A, T, 2), np.float32)
    ptr = lambda a: None if a is None else C.c_void_p(a.ctypes.data)

    def call(n=(2, 1), T=T, p0=p0, draw0=0, threshold=0.2, max_rounds=1, L=0, walls=None, radius=0.0):
        na = None if n is None else np.asarray(n, dtype=np.int32)
        rc = eng._lib.jmid_denoise_reject_padded_seeded(eng._h, E, A, K, T, ptr(na), SEED, ptr(ids), draw0, ptr(ctx), ptr(p0), 0.25, _lib.PREC_F32,
                                                        threshold, max_rounds, L, ptr(walls), radius, ptr(vel), ptr(pos), None, None, None,
                                                        _lib.MEM_HOST)
        return rc, eng._lib.jmid_last_error(eng._h).decode()

    assert call()[0] == 0
    for name, kw in (("p0", dict(p0=None)), ("T", dict(T=1)), ("max_rounds", dict(max_rounds=65)), ("draw0", dict(draw0=-1)),
                     ("threshold", dict(threshold=float("nan"))), ("radius", dict(radius=-1.0)), ("walls", dict(L=1)),
                     ("n_agents", dict(n=None)), ("n_agents", dict(n=(0, 1))), ("n_agents", dict(n=(2, 3)))):
        rc, msg = call(**kw)
        assert rc == _lib.EINVAL and "jmid_denoise_reject_padded_seeded" in msg and name in msg, (name, rc, msg)
    eng.set_step(10, "ddpm")
    try:
        rc, msg = call()
        assert rc == _lib.EINVAL and "DDIM" in msg
    finally:
        eng.set_step(2, "ddim")


# ------------------------------------------------------------------------------------------------ 6. predict_batch
def by_hand(eng, hum, rob, gids, K, k, H, thr, R, walls=None, radius=None):
    """``predict_batch(collision_free_padded=True)`` from the entries next to it: the host scene, padded inputs, one encode, the ORACLE's
    loop, ``topk(n_agents=)`` on its accepted set, ``assemble_forecasts(n_agents=)``."""
    E, F = hum.shape[0], hum.shape[1]
    b = SC.build_scenes_batched(hum, rob, DT, horizon=H)
    inc = b["in_cluster"]
    n_in = inc.sum(axis=1).astype(np.int32)
    A = int(n_in.max())
    p0 = SC.pad_agents(b["p0"], inc, A)
    ctx = eng.encode(SC.pad_agents(b["x_st"], inc, A).reshape(E * A, F, 6), SC.pad_agents(b["nbr_sum"], inc, A).reshape(E * A, 2, F, 6),
                     SC.pad_agents(b["edge_mask"], inc, A).reshape(E * A, 2)).reshape(E, A, -1)
    orc = Oracle(eng, ctx, p0, n_in, gids, K, H, "f32", thr, R, 0, walls, radius, dt=DT)
    _, pos, slots, episodes, cause = orc.result(R)
    sel, lw = eng.topk(pos, k, n_agents=n_in)
    return SC.assemble_forecasts(inc, sel, lw, b["cv"], hum[:, -1], k, K, n_agents=n_in), slots, episodes, cause, n_in, orc


@pytest.mark.parametrize("with_walls", [False, True], ids=["no_walls", "walls"])
def test_predict_batch_collision_free_padded_equals_the_oracle(with_walls):
    E, N, K, k, H = 6, 6, 16, 5, 8
    hum, rob = random_positions(E, N, 67, half_width=5.0)
    eng = engine_for()
    eng.set_step(2, "ddim")
    gids = [1000 + 7 * e for e in range(E)]
    walls = np.array([[[-6.0, 0.3], [6.0, 0.1]]]) if with_walls else None
    wk = dict(static_obstacles=walls, wall_radius=RADIUS) if with_walls else {}
    stats = {}
    fc, lw, inc = predict_batch(eng, hum, rob, gids, num_samples=K, num_ret_samples=k, horizon=H, time_step=DT, precision="f32", noise="device",
                                seed=SEED, collision_free_rounds=2, collision_threshold=0.5, collision_free_padded=True, stats=stats, **wk)
    (want_fc, want_lw), slots, episodes, cause, n_in, orc = by_hand(eng, hum, rob, gids, K, k, H, 0.5, 2, walls, RADIUS if with_walls else None)
    print(f"counts {n_in.tolist()}, episodes {episodes.tolist()}, cause {cause.tolist()}, reruns {orc.rerun}")
    assert len(np.unique(n_in)) >= 2 and n_in.min() >= 1, n_in
    assert episodes[:, 0].sum() >= 1                       # (some joint sample is redrawn; otherwise the test would show nothing)
    assert same_bits(fc, want_fc) and same_bits(lw, want_lw) and (inc.sum(axis=1) == n_in).all()
    assert same_bits(stats["slots"], slots) and same_bits(stats["episodes"], episodes) and same_bits(stats["cause"], cause)
    assert with_walls == bool(cause[:, 1].any())


@pytest.mark.parametrize("device_frames", [False, True], ids=["host_scene", "device_frames"])
def test_predict_batch_collision_free_padded_equal_counts_is_the_grouped_path(device_frames):
    """Every cluster the same size (the robot in the middle of a tight crowd): the padded loop is the grouped one, bit for bit."""
    E, N, K, k, H = 3, 4, 8, 3, 6
    hum, rob = random_positions(E, N, 5, half_width=1.0, robot=(0.0, 0.0))
    eng = engine_for()
    eng.set_step(2, "ddim")
    gids = [11, 5, 4000000000]
    kw = dict(num_samples=K, num_ret_samples=k, horizon=H, time_step=DT, precision="f32", noise="device", seed=SEED, device_frames=device_frames,
              collision_free_rounds=2, collision_threshold=0.4, static_obstacles=np.array([[-3.0, 0.5, 3.0, 0.5]]), wall_radius=RADIUS)
    one, two = {}, {}
    grouped = predict_batch(eng, hum, rob, gids, stats=one, **kw)
    padded = predict_batch(eng, hum, rob, gids, stats=two, collision_free_padded=True, **kw)
    counts = grouped[2].sum(axis=1)
    print(f"counts {counts.tolist()}, episodes {one['episodes'].tolist()}, cause {one['cause'].tolist()}")
    assert len(np.unique(counts)) == 1 and counts[0] >= 2, counts
    assert one["episodes"][:, 0].sum() >= 1                # (something is redrawn)
    for a, b in zip(padded, grouped):
        assert same_bits(a, b)
    for key in ("episodes", "slots", "cause"):
        assert same_bits(one[key], two[key]), key
