"""The collision and wall statistics of a padded batch on the device (jmid_collision_statistics_padded, jmid_wall_statistics_padded)
against the equality that defines them: every value of episode e is bit for bit what the plain entry gives for that episode's compacted
[1, K, n_e, T, 2] block, pair (i, j) at its pdist index at A.  The plain entries are the reference, so no margin is needed."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from safe_interactive_crowdnav_amd import _lib, metrics
from safe_interactive_crowdnav_amd.engine import JmidError
from tests.test_gpu_noise import engine_for, same_bits
from tests.test_gpu_rejection import to_np

E, A, K, T = 4, 4, 5, 3
COUNTS = np.array([4, 1, 2, 3], dtype=np.int32)
THRESHOLD, RADIUS = 0.8, 0.3
WALLS = np.array([[0.5, -3.0, 0.5, 3.0], [-2.0, 1.0, 2.0, 1.2]], dtype=np.float64)


def padded_positions(fill, real_nan=False, seed=11):
    """pos [E, K, A, T, 2] and p0 [E, A, 2] with ``fill`` in the padded agents' rows; real_nan: one REAL position is NaN too."""
    g = np.random.default_rng(seed)
    pos = g.normal(size=(E, K, A, T, 2)).astype(np.float32)
    p0 = g.normal(size=(E, A, 2)).astype(np.float32)
    if real_nan:
        pos[0, 2, 1, 1, 0] = np.nan          # episode 0 (4 agents), sample 2, agent 1
        pos[3, 0, 2, 0, 1] = np.inf          # episode 3 (3 agents), sample 0, its last real agent
    for e, n in enumerate(COUNTS):
        pos[e, :, n:], p0[e, n:] = fill, fill
    return pos, p0


def scattered_collision(eng, pos, pairs=True):
    """The plain entry on every compacted episode, scattered to the shapes at A."""
    pair = np.full((E, K, A * (A - 1) // 2), np.nan, dtype=np.float32)
    agent = np.zeros((E, K, A), dtype=np.uint8)
    sample, scene = np.empty((E, K, 4), np.float32), np.empty((E, 5), np.float32)
    for e, n in enumerate(COUNTS):
        pr, ag, sm, sc = (to_np(a) for a in eng.collision_statistics(np.ascontiguousarray(pos[e:e + 1, :, :n]), THRESHOLD, pairs=True))
        i, j = np.triu_indices(n, 1)
        at_A = metrics.pair_index(i, j, A)
        pair[e][:, at_A] = pr[0]
        agent[e, :, :n], sample[e], scene[e] = ag[0], sm[0], sc[0]
        has = sm[0, :, 1] >= 0
        sample[e, has, 1] = at_A[sm[0, has, 1].astype(np.int64)].astype(np.float32)
    return pair, agent, sample, scene


def scattered_walls(eng, pos, p0):
    L = WALLS.shape[0]
    dist = np.full((E, K, A, L), np.nan, dtype=np.float32)
    agent = np.zeros((E, K, A), dtype=np.uint8)
    sample, scene = np.empty((E, K, 3), np.float32), np.empty((E, 5), np.float32)
    for e, n in enumerate(COUNTS):
        d, ag, sm, sc = (to_np(a) for a in eng.wall_statistics(np.ascontiguousarray(pos[e:e + 1, :, :n]), WALLS, RADIUS,
                                                              p0=None if p0 is None else np.ascontiguousarray(p0[e:e + 1, :n])))
        dist[e, :, :n], agent[e, :, :n], sample[e], scene[e] = d[0], ag[0], sm[0], sc[0]
    return dist, agent, sample, scene


@pytest.mark.parametrize("real_nan", [False, True], ids=["finite", "real_nan"])
@pytest.mark.parametrize("fill", [np.nan, 1e30], ids=["nan_rows", "1e30_rows"])
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_collision_statistics_equal_the_plain_entry_on_compacted_episodes(device, fill, real_nan):
    eng = engine_for()
    e0 = eng.erange_count()
    pos, _ = padded_positions(fill, real_nan)
    # both outcomes occur among the real pairs (on the host twin), and the one-agent episode has none
    hp, ha, hs, _ = metrics.collision_statistics_host(pos, THRESHOLD, n_agents=COUNTS)
    real = ~np.isnan(hp) if not real_nan else np.isfinite(hp)
    assert (hp[real] < THRESHOLD).any() and (hp[real] >= THRESHOLD).any()
    assert np.isinf(hs[1, :, 0]).all() and (hs[1, :, 1] == -1).all() and not ha[1].any()
    want = scattered_collision(eng, pos)
    got = eng.collision_statistics(torch.from_numpy(pos).cuda() if device else pos, THRESHOLD, pairs=True, n_agents=COUNTS)
    assert all(isinstance(g, torch.Tensor) == device for g in got)
    for name, g, w in zip(("pair", "agent", "sample", "scene"), got, want):
        assert same_bits(g, w), f"{name} differs from the plain entry on the compacted episodes"
    # ... which is also the host twin, to fp32 rounding of the fp64 values (integers and indices exactly)
    assert np.array_equal(to_np(got[1]), ha) and np.array_equal(to_np(got[2])[..., 1:], hs[..., 1:].astype(np.float32))
    if real_nan:
        s = to_np(got[2])
        assert np.isnan(s[0, 2, 0]) and s[0, 2, 1] == -1 and np.isnan(s[3, 0, 0])
    # without pair_out and agent_out the rest is the same
    part = eng.collision_statistics(pos, THRESHOLD, pairs=False, agents=False, n_agents=COUNTS)
    assert part[0] is None and part[1] is None and same_bits(part[2], want[2]) and same_bits(part[3], want[3])
    assert eng.erange_count() == e0          # (no call of this test ended with JMID_ERANGE)


@pytest.mark.parametrize("with_p0", [False, True], ids=["no_p0", "p0"])
@pytest.mark.parametrize("fill", [np.nan, 1e30], ids=["nan_rows", "1e30_rows"])
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_wall_statistics_equal_the_plain_entry_on_compacted_episodes(device, fill, with_p0):
    eng = engine_for()
    e0 = eng.erange_count()
    pos, p0 = padded_positions(fill)
    if not with_p0:
        p0 = None
    hd, ha, hs, _ = metrics.wall_statistics_host(pos, WALLS, RADIUS, p0=p0, n_agents=COUNTS)
    assert (hd[~np.isnan(hd)] < RADIUS).any() and (hd[~np.isnan(hd)] >= RADIUS).any()
    want = scattered_walls(eng, pos, p0)
    cuda = lambda a: None if a is None else torch.from_numpy(a).cuda()
    got = eng.wall_statistics(cuda(pos) if device else pos, WALLS, RADIUS, p0=cuda(p0) if device else p0, n_agents=COUNTS)
    for name, g, w in zip(("dist", "agent", "sample", "scene"), got, want):
        assert same_bits(g, w), f"{name} differs from the plain entry on the compacted episodes"
    assert np.array_equal(to_np(got[1]), ha) and np.array_equal(to_np(got[2])[..., 1:], hs[..., 1:].astype(np.float32))
    assert eng.erange_count() == e0          # (no call of this test ended with JMID_ERANGE)


def test_every_count_equal_to_A_is_the_plain_entry():
    eng = engine_for()
    g = np.random.default_rng(5)
    pos, p0 = g.normal(size=(3, K, A, T, 2)).astype(np.float32), g.normal(size=(3, A, 2)).astype(np.float32)
    for a, b in zip(eng.collision_statistics(pos, THRESHOLD, pairs=True, n_agents=[A] * 3), eng.collision_statistics(pos, THRESHOLD, pairs=True)):
        assert same_bits(a, b)
    for a, b in zip(eng.wall_statistics(pos, WALLS, RADIUS, p0=p0, n_agents=[A] * 3), eng.wall_statistics(pos, WALLS, RADIUS, p0=p0)):
        assert same_bits(a, b)


@pytest.mark.parametrize("joint", [True, False], ids=["jmid", "imid"])
def test_resident_positions_of_a_padded_denoise(joint):
    """pos = NULL after engine.denoise(n_agents=): the positions that call left resident (NaN in their padded rows)."""
    eng = engine_for(joint)
    e0 = eng.erange_count()
    eng.set_step(2, "ddim")
    g = torch.Generator().manual_seed(2)
    ctx, p0 = torch.randn([E, A, 32], generator=g).numpy(), torch.randn([E, A, 2], generator=g).numpy()
    x_T = eng.noise(77, [1, 2, 3, 4], K * A, T, n_agents=COUNTS)
    _, pos = eng.denoise(x_T, ctx, p0, n_agents=COUNTS)
    assert np.isnan(pos[1, :, 1:]).all() and np.isfinite(pos[1, :, :1]).all()
    res_c = eng.collision_statistics(None, THRESHOLD, dims=(E, A, K, T), pairs=True, n_agents=COUNTS)
    res_w = eng.wall_statistics(None, WALLS, RADIUS, p0=p0, dims=(E, A, K, T), n_agents=COUNTS)
    for a, b in zip(res_c, eng.collision_statistics(pos, THRESHOLD, pairs=True, n_agents=COUNTS)):
        assert same_bits(a, b)
    for a, b in zip(res_w, eng.wall_statistics(pos, WALLS, RADIUS, p0=p0, n_agents=COUNTS)):
        assert same_bits(a, b)
    # the plain entry on the same positions is what the padded one is for: a NaN row decides every min_dist
    assert np.isnan(eng.collision_statistics(pos, THRESHOLD)[2][1:, :, 0]).all()
    assert not np.isnan(to_np(res_c[2])[..., 0]).any()
    assert eng.erange_count() == e0          # (no call of this test ended with JMID_ERANGE)


def test_refusals():
    eng = engine_for()
    pos, p0 = padded_positions(np.nan)
    for bad in ([4, 0, 2, 3], [4, 1, 2, 5]):
        with pytest.raises(JmidError) as err:
            eng.collision_statistics(pos, THRESHOLD, n_agents=bad)
        assert err.value.code == _lib.EINVAL and "jmid_collision_statistics_padded" in str(err.value)
        with pytest.raises(JmidError) as err:
            eng.wall_statistics(pos, WALLS, RADIUS, p0=p0, n_agents=bad)
        assert err.value.code == _lib.EINVAL and "jmid_wall_statistics_padded" in str(err.value)
