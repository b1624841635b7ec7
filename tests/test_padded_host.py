"""Host side of the padded scene batches: the packing helpers of scene.py, the NumPy twin of the device's key-mask words, what the
fixtures tests/golden/padded_*.npz cover, and the refusals of predict_batch(padded=True) that need no device."""
import glob
import os

import numpy as np
import pytest

from safe_interactive_crowdnav_amd import scene as SC

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = sorted(os.path.basename(p) for p in glob.glob(os.path.join(GOLDEN, "padded_*.npz")))


def brute_words(n_agents, A, K, T):
    S = K * A * T
    out = np.zeros((len(n_agents), (S + 31) // 32), np.uint32)
    for e, n in enumerate(n_agents):
        for s in range(K):
            for a in range(int(n)):
                for t in range(T):
                    j = (s * A + a) * T + t
                    out[e, j // 32] |= np.uint32(1) << np.uint32(j % 32)
    return out


@pytest.mark.parametrize("A,K,T,n", [(4, 8, 12, [4, 1, 3]), (3, 5, 6, [2, 3, 1]), (1, 3, 5, [1]), (7, 2, 24, [1, 7, 4, 6]), (2, 1, 1, [1, 2])])
def test_key_mask_words_are_the_valid_keys(A, K, T, n):
    w = SC.key_mask_words(np.array(n), A, K, T)
    assert w.dtype == np.uint32
    np.testing.assert_array_equal(w, brute_words(n, A, K, T))
    S = K * A * T
    if S % 32:      # bits at or past S are 0
        assert not (w[:, -1] >> np.uint32(S % 32)).any()
    assert (w[:, 0] & 1).all()      # key 0 of an episode is always valid


def test_fixtures_hold_the_word_kinds_the_kernels_branch_on():
    assert len(CASES) == 4
    full = np.uint32(0xFFFFFFFF)
    for case in CASES:
        z = np.load(os.path.join(GOLDEN, case))
        A, K, T, n = int(z["A"]), int(z["K"]), int(z["T"]), z["n_agents"]
        w = SC.key_mask_words(n, A, K, T)
        partial = (w != 0) & (w != full)
        assert (w == full).any() and partial.any(), case
        assert float(z["compact_err"]) <= 1e-5            # the reference's masked branch against its own compact evaluation
        assert (n == A).any() and (n < A).any()
        real = np.arange(A)[None, :] < n[:, None]
        assert not z["ctx"][~real].any()
        if "e3a4k8t12" in case:
            # S = 384, 12 tiles: episode 1 (one agent of four: 12 valid keys in every 48) has the all-zero words 2, 5, 8, 11
            assert w.shape == (3, 12) and list(np.nonzero(w[1] == 0)[0]) == [2, 5, 8, 11]
            assert (w[0] == full).all() and w[2, 0] == full
        else:
            # S = 90: the last tile is cut by S in every episode.  (A T = 18 < 32: every 32-key tile holds a real agent's keys, so
            # this shape cannot have an all-zero word - the first fixture is the one that has them.)
            assert w.shape == (3, 3) and (w[:, 2] >> np.uint32(90 - 64) == 0).all() and w[1, 2] == np.uint32((1 << 26) - 1)
            assert not (w == 0).any()


def test_pad_and_unpad_round_trip():
    rng = np.random.default_rng(0)
    E, N, K, H = 5, 6, 4, 3
    inc = rng.random((E, N)) < 0.5
    inc[:, 0] = True
    n = inc.sum(axis=1)
    A = int(n.max())
    arr = rng.standard_normal((E, N, 2, 3)).astype(np.float32)
    p = SC.pad_agents(arr, inc, A)
    assert p.shape == (E, A, 2, 3)
    for e in range(E):
        np.testing.assert_array_equal(p[e, :n[e]], arr[e, inc[e]])
        assert not p[e, n[e]:].any()
    per = [rng.standard_normal((K * int(n[e]), H, 2)).astype(np.float32) for e in range(E)]
    x = SC.pad_samples(per, n, A, K)
    assert x.shape == (E, K * A, H, 2)
    for e in range(E):
        for s in range(K):
            for a in range(A):
                want = per[e][s * n[e] + a] if a < n[e] else 0.0
                np.testing.assert_array_equal(x[e, s * A + a], want)
        np.testing.assert_array_equal(SC.unpad_samples(x.reshape(E, K, A, H, 2), n, e).reshape(K * n[e], H, 2), per[e])


def test_predict_batch_names_what_padded_does_not_combine_with():
    from safe_interactive_crowdnav_amd.forecaster import predict_batch
    hum, rob = np.zeros((2, 6, 3, 2)), np.zeros((2, 6, 2))
    kw = dict(num_samples=4, num_ret_samples=4, horizon=4, time_step=0.25, padded=True)
    for bad in (dict(device_scene=True), dict(device_frames=True), dict(noise="device")):
        with pytest.raises(ValueError, match="padded=True"):
            predict_batch(None, hum, rob, [0, 1], **kw, **bad)
