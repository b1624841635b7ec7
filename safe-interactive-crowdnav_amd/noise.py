"""Host twin of ``csrc/noise.hpp``: the seeded noise of the device sampler, restated in vectorised NumPy.

A draw is a pure function of (seed, episode id, draw number, element): Philox4x32-10 (Salmon et al., SC'11) with

    key     = (seed & 0xffffffff, seed >> 32)
    counter = (q, episode_id, draw, 0)        q = idx // 4, idx the row-major index inside the episode's [rows, T, 2] tensor

whose four output words give the elements 4q .. 4q + 3 (the last block of an episode may be partly used).  ``draw`` 0 is x_T,
``draw`` i + 1 the z of step-table entry i.  Normals are Box-Muller per word pair (a, b) in float64, rounded once to float32:
u1 = (a + 1) 2^-32, u2 = b 2^-32, r = sqrt(-2 ln u1), (r cos(2 pi u2), r sin(2 pi u2)); |z| <= 6.67.

This generator is statistically, not seed-, compatible with the reference (which draws from torch's generators): the parity
gates stay defined on identical x_T through the explicit-noise entry points.
"""
from __future__ import annotations

import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)
TWO_PI = 6.283185307179586


def philox4x32_10(counter, key) -> np.ndarray:
    """counter [..., 4], key [..., 2] (broadcast against each other) uint32 -> the block's four words [..., 4] uint32."""
    c = np.asarray(counter, dtype=np.uint64) & _MASK
    k = np.asarray(key, dtype=np.uint64) & _MASK
    shape = np.broadcast_shapes(c.shape[:-1], k.shape[:-1])
    c0, c1, c2, c3 = (np.broadcast_to(c[..., i], shape) for i in range(4))
    k0, k1 = (np.broadcast_to(k[..., i], shape) for i in range(2))
    for r in range(10):
        p0, p1 = M0 * c0, M1 * c2                     # 32 x 32 -> 64 bit products: exact in uint64
        rk0 = (k0 + np.uint64((r * W0) & 0xFFFFFFFF)) & _MASK
        rk1 = (k1 + np.uint64((r * W1) & 0xFFFFFFFF)) & _MASK
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ rk0, p1 & _MASK, (p0 >> _S32) ^ c3 ^ rk1, p0 & _MASK
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def _ids(episode_ids) -> np.ndarray:
    ids = np.atleast_1d(np.asarray(episode_ids))
    if ids.ndim != 1 or ids.size < 1:
        raise ValueError("episode_ids must hold one id per episode")
    if np.any(ids.astype(np.int64) < 0) or np.any(ids.astype(np.uint64) > 0xFFFFFFFF):
        raise ValueError("episode ids are uint32")
    return ids.astype(np.uint32)


def words(seed: int, episode_ids, rows: int, T: int, draw: int = 0) -> np.ndarray:
    """The raw Philox words behind ``normal``: uint32 [E, rows, T, 2]."""
    seed, rows, T, draw = int(seed), int(rows), int(T), int(draw)
    if rows < 1 or T < 1 or draw < 0 or not 0 <= seed < 1 << 64:
        raise ValueError("rows, T >= 1, draw >= 0 and a 64-bit seed")
    ids = _ids(episode_ids)
    n = rows * T * 2
    nq = (n + 3) // 4
    ctr = np.zeros((ids.size, nq, 4), dtype=np.uint64)
    ctr[..., 0] = np.arange(nq, dtype=np.uint64)[None]
    ctr[..., 1] = ids.astype(np.uint64)[:, None]
    ctr[..., 2] = draw
    key = np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64)
    w = philox4x32_10(ctr, key).reshape(ids.size, nq * 4)[:, :n]
    return np.ascontiguousarray(w).reshape(ids.size, rows, T, 2)


def normal(seed: int, episode_ids, rows: int, T: int, draw: int = 0) -> np.ndarray:
    """Standard normals float32 [E, rows, T, 2]: what ``jmid_noise_fill`` writes for the same arguments."""
    ids = _ids(episode_ids)
    n = int(rows) * int(T) * 2
    nq = (n + 3) // 4
    w = np.zeros((ids.size, nq * 4), dtype=np.uint32)
    w[:, :n] = words(seed, ids, rows, T, draw).reshape(ids.size, n)
    pairs = w.reshape(ids.size, nq * 2, 2).astype(np.float64)
    u1 = (pairs[..., 0] + 1.0) * 2.0 ** -32
    u2 = pairs[..., 1] * 2.0 ** -32
    r = np.sqrt(-2.0 * np.log(u1))
    th = TWO_PI * u2
    z = np.stack([r * np.cos(th), r * np.sin(th)], axis=-1).astype(np.float32)
    return np.ascontiguousarray(z.reshape(ids.size, nq * 4)[:, :n]).reshape(ids.size, int(rows), int(T), 2)


def fill_padded(seed: int, episode_ids, n_agents, A: int, K: int, T: int, draw: int = 0) -> np.ndarray:
    """The draw of a padded batch, float32 [E, K * A, T, 2]: what ``jmid_noise_fill_padded`` writes for the same arguments.

    Episode e draws exactly what it draws alone at its own count - ``normal(seed, [id_e], K * n_e, T, draw)``, n_e = n_agents[e] - and
    row ``s * n_e + a`` of that compact tensor lands in padded row ``s * A + a``; the padded rows (a >= n_e) are NaN."""
    ids = _ids(episode_ids)
    n = np.atleast_1d(np.asarray(n_agents)).astype(np.int64)
    A, K, T = int(A), int(K), int(T)
    if n.shape != ids.shape or A < 1 or K < 1 or np.any(n < 1) or np.any(n > A):
        raise ValueError("one count per episode, 1 <= n_agents[e] <= A, and K >= 1")
    out = np.full((ids.size, K, A, T, 2), np.nan, dtype=np.float32)
    for e in range(ids.size):
        ne = int(n[e])
        out[e, :, :ne] = normal(seed, ids[e:e + 1], K * ne, T, draw).reshape(K, ne, T, 2)
    return out.reshape(ids.size, K * A, T, 2)
