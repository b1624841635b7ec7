"""The host twin of the device noise generator (safe-interactive-crowdnav_amd/noise.py; csrc/noise.hpp): Philox4x32-10 known answers,
the (seed, episode id, draw, element) addressing, the moments of the Box-Muller normals, and the binding's refusal of x_T together
with seed.  tests/test_gpu_noise.py holds the device kernel to this module bit for bit."""
import numpy as np
import pytest

from safe_interactive_crowdnav_amd import noise as NZ
from safe_interactive_crowdnav_amd.engine import JmidEngine, seeded_noise_args

KNOWN = [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
]


@pytest.mark.parametrize("counter,key,want", KNOWN)
def test_philox4x32_10_known_answers(counter, key, want):
    got = NZ.philox4x32_10(np.array(counter, dtype=np.uint32), np.array(key, dtype=np.uint32))
    assert got.dtype == np.uint32 and got.shape == (4,)
    assert " ".join(f"{int(v):08x}" for v in got) == want


def test_known_answers_vectorised():
    got = NZ.philox4x32_10(np.array([c for c, _, _ in KNOWN], dtype=np.uint32), np.array([k for _, k, _ in KNOWN], dtype=np.uint32))
    assert [" ".join(f"{int(v):08x}" for v in row) for row in got] == [w for _, _, w in KNOWN]


def test_words_are_the_philox_blocks_of_the_address():
    """counter = (q, episode id, draw, 0), key = (seed low, seed high); element idx takes word idx % 4 of block idx // 4."""
    seed, ids, rows, T, draw = (1 << 40) + 9, [5, 0, 4294967295], 7, 5, 3
    w = NZ.words(seed, ids, rows, T, draw)
    assert w.shape == (3, rows, T, 2) and w.dtype == np.uint32
    flat = w.reshape(3, -1)
    key = np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint32)
    for e, eid in enumerate(ids):
        for idx in (0, 1, 5, 34, 69):
            blk = NZ.philox4x32_10(np.array([idx // 4, eid, draw, 0], dtype=np.uint32), key)
            assert flat[e, idx] == blk[idx % 4]


@pytest.mark.parametrize("fn", [NZ.words, NZ.normal])
def test_an_episode_does_not_depend_on_its_batch(fn):
    def same(a, b):
        return a.shape == b.shape and a.tobytes() == b.tobytes()

    full = fn(3, [10, 11, 12, 13, 14], 6, 4, 2)
    assert same(full[2:3], fn(3, [12], 6, 4, 2))                       # E
    assert same(full[[4, 0, 2]], fn(3, [14, 10, 12], 6, 4, 2))         # order
    assert same(full[1:2], fn(3, [99, 11, 7], 6, 4, 2)[1:2])           # the other ids of the call
    assert same(full[:2], fn(3, np.array([10, 11], dtype=np.int64), 6, 4, 2))


@pytest.mark.parametrize("fn", [NZ.words, NZ.normal])
def test_seed_draw_and_id_all_enter(fn):
    base = fn(0, [7], 8, 4, 0)
    assert not np.array_equal(base, fn(1, [7], 8, 4, 0))
    assert not np.array_equal(base, fn(1 << 40, [7], 8, 4, 0))          # a seed with only high bits set
    assert not np.array_equal(fn(1, [7], 8, 4, 0), fn((1 << 32) + 1, [7], 8, 4, 0))
    assert not np.array_equal(base, fn(0, [7], 8, 4, 1))                # draws
    assert not np.array_equal(base, fn(0, [8], 8, 4, 0))                # ids
    assert not np.array_equal(fn(0, [7], 8, 4, 1), fn(0, [8], 8, 4, 0))


def test_partial_last_block():
    """rows = 3, T = 1: 6 values, 2 mod 4 - the second block is half used, and it is the prefix of the longer tensor's."""
    w = NZ.words(5, [1, 2], 3, 1, 2)
    assert w.shape == (2, 3, 1, 2)
    long = NZ.words(5, [1, 2], 4, 1, 2)
    assert np.array_equal(w.reshape(2, 6), long.reshape(2, 8)[:, :6])
    z, zl = NZ.normal(5, [1, 2], 3, 1, 2), NZ.normal(5, [1, 2], 4, 1, 2)
    assert z.dtype == np.float32 and z.shape == (2, 3, 1, 2)
    assert z.reshape(2, 6).tobytes() == np.ascontiguousarray(zl.reshape(2, 8)[:, :6]).tobytes()
    # the shape is a view of the flat index: [rows, T, 2] row-major
    assert np.array_equal(NZ.words(5, [1], 2, 6, 0).ravel(), NZ.words(5, [1], 12, 1, 0).ravel())


def test_moments_of_the_normals():
    """2^16 values, seed 1234, id 7, draw 0: every bound is five standard errors of the statistic under N(0, 1) (Var z^2 = 2, Var z^4 = 96)."""
    z = NZ.normal(1234, [7], 1 << 14, 2, 0).ravel().astype(np.float64)
    n = z.size
    assert n == 1 << 16
    mean, std, m4, zmax = z.mean(), z.std(), (z ** 4).mean(), np.abs(z).max()
    print(f"mean {mean:.4f} std {std:.4f} fourth moment {m4:.3f} max |z| {zmax:.3f}")
    assert abs(mean) < 5 / np.sqrt(n)
    assert abs(std - 1) < 5 / np.sqrt(2 * n)
    assert abs(m4 - 3) < 5 * np.sqrt(96 / n)
    assert zmax <= 6.67


def test_the_extreme_words_stay_inside_the_bound():
    """u1 = 2^-32 (a = 0) is the largest radius: sqrt(64 ln 2) = 6.66; a = 2^32 - 1 gives u1 = 1, radius 0 - no log(0), no overflow."""
    pairs = np.array([[0, 0], [0, 1 << 30], [0xFFFFFFFF, 123]], dtype=np.float64)
    u1 = (pairs[:, 0] + 1.0) * 2.0 ** -32
    r = np.sqrt(-2.0 * np.log(u1))
    assert np.isfinite(r).all() and r.max() <= 6.67 and r[2] == 0.0


def test_bad_arguments():
    for bad in (dict(rows=0), dict(T=0), dict(draw=-1), dict(seed=-1), dict(seed=1 << 64), dict(episode_ids=[-1]),
                dict(episode_ids=[1 << 32]), dict(episode_ids=[])):
        kw = dict(seed=0, episode_ids=[0], rows=2, T=2, draw=0)
        kw.update(bad)
        with pytest.raises(ValueError):
            NZ.words(**kw)


def test_the_binding_rejects_x_T_together_with_seed():
    x = np.zeros((1, 4, 3, 2), np.float32)
    ctx = np.zeros((1, 2, 32), np.float32)
    with pytest.raises(ValueError, match="mutually exclusive"):
        seeded_noise_args(x, 1, [0])
    eng = object.__new__(JmidEngine)          # no handle: the refusal comes before the library is touched
    for call in (lambda: eng.denoise(x, ctx, seed=1, episode_ids=[0], K=2, T=3),
                 lambda: eng.predict_scene(x, 2, seed=1, episode_ids=[0], K=2, T=3),
                 lambda: eng.forecast_scene(x, 2, seed=1, episode_ids=[0], K=2, T=3)):
        with pytest.raises(ValueError, match="mutually exclusive"):
            call()
    with pytest.raises(ValueError):
        seeded_noise_args(None, None, None)             # neither
    with pytest.raises(ValueError):
        seeded_noise_args(None, 1, None)                # a seed without ids
    with pytest.raises(ValueError):
        seeded_noise_args(x, None, [0])                 # ids without a seed
    with pytest.raises(ValueError):
        seeded_noise_args(None, 1, [0, 1], E=3)         # one id per episode
    assert seeded_noise_args(x, None, None) is None
    seed, ids = seeded_noise_args(None, (1 << 40) + 9, [5, 0, 4294967295], E=3)
    assert seed == (1 << 40) + 9 and ids.dtype == np.uint32 and ids.tolist() == [5, 0, 4294967295]
