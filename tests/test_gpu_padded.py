"""Padded scene batches (the *_padded entries of include/jmid_hip.h): episodes of different agent counts in ONE call of the uniform
shape [E, K A, T] with A the largest count, the tokens of padded agents masked as attention keys.

The fixtures tests/golden/padded_*.npz come from the reference's masked branch (tests/golden/make_golden_padded.py):
  E=3, A=4, K=8, T=12, n=[4,1,3]: S = 384, 12 key tiles; all-zero, all-ones and partial mask words
  E=3, A=3, K=5, T=6,  n=[2,3,1]: S = 90, the last key tile is also cut by S
at encoder_dim 32 (head_dim 16: the generic attention kernels) and 256 (head_dim 128: the LDS-DMA kernel).
mean ADE as tests/test_gpu_parity.py defines it; gate 1e-4."""
import ctypes as C
import functools
import glob
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import tests.test_gpu_parity as P      # the engines of that file (one per width and flavour), its ade() and tolerances
from oracle import jmid_oracle as O
from safe_interactive_crowdnav_amd import scene as SC
from safe_interactive_crowdnav_amd.engine import JmidEngine, JmidError
from safe_interactive_crowdnav_amd.kde import most_likely_samples
from safe_interactive_crowdnav_amd.weights import JMIDWeights, NetDims

GOLDEN = P.GOLDEN
CASES = sorted(os.path.basename(p) for p in glob.glob(os.path.join(GOLDEN, "padded_*.npz")))
WIDE_FIRST = "padded_w256_e3a4k8t12.npz"
PRECISIONS, ADE_GATE, ade = P.PRECISIONS, P.ADE_GATE, P.ade


def load(case, flavour="diag"):
    z = np.load(os.path.join(GOLDEN, case))
    eng, w = P.get_engine(int(z["ctx_dim"]), int(z["wseed"]), True, flavour)
    assert w.checksum() == str(z["wsum"])
    eng.set_step(int(z["step"]))
    return z, eng, w, (int(z["A"]), int(z["K"]), int(z["T"])), z["n_agents"]


def real_rows(arr, n, e, A, K):
    """[E, K*A, ...] or [E, K, A, ...] -> episode e's real agents [K, n[e], ...]"""
    a = np.asarray(arr)[e]
    return a.reshape((K, A) + a.shape[-2:])[:, :int(n[e])]


def padded_rows_mask(n, A, K):
    return np.broadcast_to((np.arange(A)[None, :] >= np.asarray(n)[:, None])[:, None, :], (len(n), K, A))


def p0_of(z):
    g = torch.Generator().manual_seed(int(z["dseed"]) + 1)
    return torch.randn([len(z["n_agents"]), int(z["A"]), 2], generator=g).numpy()


@functools.lru_cache(maxsize=None)
def oracle_compact(case):
    """oracle.jmid_oracle on every episode compacted to A = n[e]: velocities [K, n[e], T, 2] per episode, computed once per fixture"""
    z, _, w, (A, K, T), n = load(case)
    out = []
    with torch.no_grad():
        for e in range(len(n)):
            xc = torch.from_numpy(np.ascontiguousarray(real_rows(z["x"], n, e, A, K))).reshape(K * int(n[e]), T, 2)
            cc = torch.from_numpy(z["ctx"][e, :int(n[e])])
            out.append(O.denoise(w.tensors, cc, xc, sample=K, step=int(z["step"]), joint=True).numpy().reshape(K, int(n[e]), T, 2))
    return out


def compact_denoise(eng, z, e, A, K, T, n, precision):
    """episode e alone through today's denoise at A = n[e]"""
    ne = int(n[e])
    xc = np.ascontiguousarray(real_rows(z["x"], n, e, A, K)).reshape(1, K * ne, T, 2)
    vel, _ = eng.denoise(xc, np.ascontiguousarray(z["ctx"][e:e + 1, :ne]), precision=precision, want_pos=False)
    return vel[0]


def check_compact_bounds(tag, eng, z, padded, case, precision):
    """Per episode e of `padded` (e -> its real rows [K, n[e], T, 2] out of a padded call): padded vs oracle <= 1e-4, and padded vs
    compact <= 2 x (compact vs oracle) - both are roundings of the same sum, each about one such distance from the truth."""
    (A, K, T), n = (int(z["A"]), int(z["K"]), int(z["T"])), z["n_agents"]
    orc = oracle_compact(case)
    for e, pe in padded.items():
        ce = compact_denoise(eng, z, e, A, K, T, n, precision)
        d_po, d_pc, d_co = ade(pe, orc[e]), ade(pe, ce), ade(ce, orc[e])
        print(f"{tag} {case} [{precision}] episode {e} (n = {int(n[e])}): padded-oracle {d_po:.3e}  padded-compact {d_pc:.3e}  compact-oracle {d_co:.3e}")
        assert np.isfinite(pe).all()
        assert d_po <= ADE_GATE, d_po
        assert d_pc <= 2.0 * d_co, (d_pc, d_co)


@pytest.mark.parametrize("flavour", ["diag", "prod"])
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("case", CASES)
def test_padded_net_eval_and_denoise_match_the_reference_masked_branch(case, precision, flavour):
    z, eng, _, (A, K, T), n = load(case, flavour)
    e_all = eng.net_eval(z["x"], z["ctx"], step_idx=0, precision=precision, n_agents=n)
    vel, _ = eng.denoise(z["x"], z["ctx"], precision=precision, want_pos=False, n_agents=n)
    for e in range(len(n)):
        d_e = ade(real_rows(e_all, n, e, A, K), real_rows(z["e"], n, e, A, K))
        d_v = ade(real_rows(vel, n, e, A, K), real_rows(z["vel"], n, e, A, K))
        print(f"{case} [{precision}, {flavour}] episode {e}: e_theta {d_e:.3e}  vel {d_v:.3e}")
        assert d_e <= P.E_THETA_TOL[precision], d_e
        assert d_v <= ADE_GATE, d_v
    pad = padded_rows_mask(n, A, K)
    assert np.isnan(vel[pad]).all() and np.isfinite(vel[~pad]).all()
    assert np.isnan(e_all.reshape(len(n), K, A, T, 2)[pad]).all()


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("case", CASES)
def test_padded_call_equals_each_episode_run_alone(case, precision):
    z, eng, _, (A, K, T), n = load(case)
    vel, _ = eng.denoise(z["x"], z["ctx"], precision=precision, want_pos=False, n_agents=n)
    check_compact_bounds("compact", eng, z, {e: real_rows(vel, n, e, A, K) for e in range(len(n))}, case, precision)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("case", CASES)
def test_full_episodes_keep_the_plain_calls_bits(case, precision):
    """Same E, A, K, T, same chunk plan, same split-KV factor: an episode without padding runs the plain kernels' arithmetic."""
    z, eng, _, (A, K, T), n = load(case)
    p0 = p0_of(z)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(z["x"].shape, generator=g).numpy()
    ctx = torch.randn(z["ctx"].shape, generator=g).numpy()
    plain = eng.denoise(x, ctx, p0, precision=precision)
    full = eng.denoise(x, ctx, p0, precision=precision, n_agents=np.full(len(n), A))
    np.testing.assert_array_equal(full[0], plain[0])
    np.testing.assert_array_equal(full[1], plain[1])
    np.testing.assert_array_equal(eng.net_eval(x, ctx, precision=precision, n_agents=np.full(len(n), A)), eng.net_eval(x, ctx, precision=precision))
    mixed = eng.denoise(x, ctx, p0, precision=precision, n_agents=n)
    for e in np.nonzero(n == A)[0]:
        np.testing.assert_array_equal(mixed[0][e], plain[0][e])
        np.testing.assert_array_equal(mixed[1][e], plain[1][e])
    assert (n == A).any()


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("case", CASES)
def test_padding_rows_are_never_read(case, precision, device):
    z, eng, _, (A, K, T), n = load(case)
    pad = padded_rows_mask(n, A, K)
    p0 = p0_of(z)
    outs = []
    for fill in (0.0, 3.0e4, np.nan):
        x = z["x"].reshape(len(n), K, A, T, 2).copy()
        ctx, p = z["ctx"].copy(), p0.copy()
        g = np.random.default_rng(1)
        x[pad] = fill * (g.standard_normal(x[pad].shape) if np.isfinite(fill) else 1.0)
        ctx[pad[:, 0]] = fill
        p[pad[:, 0]] = fill
        args = [x.reshape(z["x"].shape).astype(np.float32), ctx, p]
        keep = [a.copy() for a in args]
        if device:
            args = [torch.from_numpy(a).cuda() for a in args]
        vel, pos = eng.denoise(*args, dt=0.25, precision=precision, n_agents=n)      # (raises on any status but 0, JMID_ERANGE included)
        e_out = eng.net_eval(args[0], args[1], precision=precision, n_agents=n)
        if device:
            torch.cuda.synchronize()
            for a, k in zip(args, keep):      # the caller's arrays are inputs: not a byte of them changes
                np.testing.assert_array_equal(a.cpu().numpy(), k)
            vel, pos, e_out = vel.cpu().numpy(), pos.cpu().numpy(), e_out.cpu().numpy()
        e_out = e_out.reshape(vel.shape)
        for o in (vel, pos, e_out):
            assert np.isnan(o[pad]).all() and np.isfinite(o[~pad]).all()
        outs.append((vel[~pad], pos[~pad], e_out[~pad]))
    for o in outs[1:]:
        for a, b in zip(o, outs[0]):
            np.testing.assert_array_equal(a, b)


def split_starts(S, nsplit):
    """first key tile of every split: the kernel's own formula (attn_f16x3.hpp, kt_begin)"""
    nt = (S + 31) // 32
    return [s * nt // nsplit for s in range(nsplit + 1)]


@pytest.mark.parametrize("nsplit", [3, 12])
@pytest.mark.parametrize("precision", P.SPLIT_MODES)
def test_split_kv_ranges_that_start_on_or_consist_of_masked_tiles(precision, nsplit):
    """head_dim 128, forced split-KV factor: with 3 splits the third starts on an all-zero word of episode 1 (tile 8), with 12 every
    split is one tile and four of episode 1's are entirely masked - a wave's first COMPUTED tile is not its first tile, and a split
    may hand (m, l) = (-inf, 0) to the merge.  The one-scene shape E = 1, n = [1] crosses the merge inside the out-projection's
    one-launch GEMM + LayerNorm in f16mx."""
    z, eng, _, (A, K, T), n = load(WIDE_FIRST)
    S = K * A * T
    words = SC.key_mask_words(n, A, K, T)
    starts = split_starts(S, nsplit)
    assert starts[:nsplit] == ([0, 4, 8] if nsplit == 3 else list(range(12)))
    assert any(words[1, s] == 0 for s in starts[1:nsplit])                                                  # a split starts on a zero word
    assert (nsplit == 3) or any((words[1, a:b] == 0).all() for a, b in zip(starts[:-1], starts[1:]))       # a split is entirely masked
    eng.set_tuning("attn_nsplit", nsplit)
    try:
        vel, _ = eng.denoise(z["x"], z["ctx"], precision=precision, want_pos=False, n_agents=n)
        one, _ = eng.denoise(z["x"][1:2], z["ctx"][1:2], precision=precision, want_pos=False, n_agents=n[1:2])
    finally:
        eng.set_tuning("attn_nsplit", 0)
    check_compact_bounds(f"nsplit={nsplit}", eng, z, {e: real_rows(vel, n, e, A, K) for e in range(len(n))}, WIDE_FIRST, precision)
    check_compact_bounds(f"nsplit={nsplit} one scene", eng, z, {1: real_rows(one, n[1:2], 0, A, K)}, WIDE_FIRST, precision)


def test_topk_padded_ranks_each_episode_over_its_real_agents():
    eng, _ = P.get_engine(32, 77, True)
    g = torch.Generator().manual_seed(23)
    E, K, A, H, k = 3, 30, 4, 8, 7
    n = np.array([4, 1, 3], np.int32)
    pos = (torch.cumsum(0.004 * torch.randn([E, K, A, H, 2], generator=g), dim=3) + torch.randn([E, 1, A, 1, 2], generator=g)).numpy()
    pad = padded_rows_mask(n, A, K)
    pos[pad] = np.nan
    for p in (pos, torch.from_numpy(pos).cuda()):
        sel, lw = eng.topk(p, k, n_agents=n)
        if torch.is_tensor(sel):
            torch.cuda.synchronize()
            sel, lw = sel.cpu().numpy(), lw.cpu().numpy()
        for e in range(E):
            top, lw_h = most_likely_samples(np.ascontiguousarray(pos[e][:, :n[e]]), k)      # the reference's arithmetic on the compact episode
            np.testing.assert_array_equal(sel[e, :n[e]], top)
            np.testing.assert_allclose(lw[e, :n[e]], lw_h, rtol=0, atol=5e-5)
            assert np.isnan(sel[e, n[e]:]).all() and np.isnan(lw[e, n[e]:]).all()
    # the plain entry's result does not move: a batch without padding through both
    full = np.where(np.isnan(pos), 0.25, pos).astype(np.float32)
    a, b = eng.topk(full, k), eng.topk(full, k, n_agents=np.full(E, A))
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1], b[1])


def test_topk_padded_with_the_whitened_points_in_global_memory():
    """A = 18, K = 256: the K x 2 A whitened points of an (episode, horizon step) do not fit in LDS next to the [d, d] algebra, so every
    workgroup keeps them in its slice of the global workspace - which must not depend on the episode's own count (slices by 2 n_e
    would overlap between episodes of different counts, whose workgroups run side by side).  K well above 2 A and below 512: the
    regime in which tests/test_gpu_kde.py holds choice and order against the host twin."""
    eng, _ = P.get_engine(32, 77, True)
    g = torch.Generator().manual_seed(29)
    E, K, A, H, k = 3, 256, 18, 4, 7
    n = np.array([18, 3, 11], np.int32)
    pos = (torch.cumsum(0.003 * torch.randn([E, K, A, H, 2], generator=g), dim=3) + torch.randn([E, 1, A, 1, 2], generator=g)).numpy()
    pos[padded_rows_mask(n, A, K)] = np.nan
    sel, lw = eng.topk(pos, k, n_agents=n)
    for e in range(E):
        top, lw_h = most_likely_samples(np.ascontiguousarray(pos[e][:, :n[e]]), k)
        np.testing.assert_array_equal(sel[e, :n[e]], top)
        np.testing.assert_allclose(lw[e, :n[e]], lw_h, rtol=0, atol=2e-4)
        assert np.isnan(sel[e, n[e]:]).all() and np.isnan(lw[e, n[e]:]).all()


@pytest.mark.parametrize("precision", ["f32", "f16mx"])
def test_topk_of_the_preceding_padded_denoise(precision):
    z, eng, _, (A, K, T), n = load("padded_w32_e3a4k8t12.npz")
    p0 = p0_of(z)
    _, pos = eng.denoise(z["x"], z["ctx"], p0, dt=0.01, precision=precision, want_vel=False, n_agents=n)
    a = eng.topk(pos, 3, n_agents=n)
    eng.denoise(z["x"], z["ctx"], p0, dt=0.01, precision=precision, want_vel=False, want_pos=False, n_agents=n)
    b = eng.topk(None, 3, dims=(len(n), A, K, T), n_agents=n)
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1], b[1])
    assert np.isnan(a[0][1, 1:]).all() and np.isfinite(a[0][1, :1]).all()


@pytest.mark.parametrize("joint", [True, False])
def test_graph_replay_and_imid_take_other_counts_of_the_same_shape(joint):
    """The mask words and the zeroed rows are written outside the captured loop, on memory the loop reads: a replay with other
    counts gives that call's result.  iMID: no mask, the same zero-in / NaN-out contract."""
    z = np.load(os.path.join(GOLDEN, "padded_w32_e3a4k8t12.npz"))
    w = JMIDWeights.from_seed(NetDims(ctx_dim=32), 5)
    eng = JmidEngine(w, joint=joint, step=4)
    A, K = int(z["A"]), int(z["K"])
    counts = [np.array([4, 1, 3]), np.array([2, 4, 1]), np.array([1, 1, 4])]
    eager = [eng.denoise(z["x"], z["ctx"], precision="f32", want_pos=False, n_agents=n)[0] for n in counts]
    eng.set_tuning("graph", 1)
    r0 = eng.graph_replays()
    for _ in range(2):
        for n, ref in zip(counts, eager):
            vel, _ = eng.denoise(z["x"], z["ctx"], precision="f32", want_pos=False, n_agents=n)
            np.testing.assert_array_equal(vel, ref)
            assert np.isnan(vel[padded_rows_mask(n, A, K)]).all()
    assert eng.graph_replays() > r0
    eng.close()


def natural_clusters(E=24, F=6, N=6, dt=0.25):
    """the generator of tests/test_gpu_forecaster.py's ragged-batch test"""
    rng = np.random.default_rng(17)
    pos0 = rng.uniform(-5.0, 5.0, (E, N, 2))
    vel = rng.uniform(-1.0, 1.0, (E, N, 2))
    t = np.arange(F) * dt
    hum = pos0[:, None] + vel[:, None] * t[None, :, None, None] + 0.01 * rng.standard_normal((E, F, N, 2))
    rob = np.array([0.0, -3.0])[None, None] + 0.02 * rng.standard_normal((E, F, 2))
    return hum, rob


@pytest.mark.parametrize("ctx_dim,precision,k_ret", [(32, "f32", 16), (256, "f16mx", 16), (32, "f16x3", 5)])
def test_predict_batch_padded_against_the_grouped_path(ctx_dim, precision, k_ret):
    from safe_interactive_crowdnav_amd.forecaster import predict_batch
    K, H, dt = 16, 8, 0.25
    hum, rob = natural_clusters()
    E, F, N, _ = hum.shape
    eng = JmidEngine(JMIDWeights.from_seed(NetDims(ctx_dim=ctx_dim), 5), joint=True, step=2)
    w = JMIDWeights.from_seed(NetDims(ctx_dim=ctx_dim), 5)
    seeds = [1000 + e for e in range(E)]
    kw = dict(num_samples=K, num_ret_samples=k_ret, horizon=H, time_step=dt, precision=precision)
    torch.manual_seed(99)
    state0 = torch.get_rng_state()
    fc_g, lw_g, inc_g = predict_batch(eng, hum, rob, seeds, **kw)
    state_g = torch.get_rng_state()
    fc_p, lw_p, inc_p = predict_batch(eng, hum, rob, seeds, padded=True, **kw)
    state_p = torch.get_rng_state()
    sizes = inc_g.sum(axis=1)
    assert len(np.unique(sizes)) >= 3 and sizes.min() >= 1
    np.testing.assert_array_equal(inc_p, inc_g)
    assert torch.equal(state_g, state0) and torch.equal(state_p, state_g)
    np.testing.assert_array_equal(fc_p[~inc_g], fc_g[~inc_g])          # constant-velocity rows: host arithmetic
    assert np.isfinite(fc_p).all() and np.isfinite(lw_p).all()
    if k_ret < K:
        # ranked (at this time step the joint likelihoods of the samples tie to rounding, so WHICH samples are kept is not comparable
        # between two roundings of the futures): the kept forecasts are k distinct ones of the K futures of the same padded call, bit
        # for bit, the same ones for every agent of an episode, with one normalised weight row per episode
        all_p, _, _ = predict_batch(eng, hum, rob, seeds, padded=True, **dict(kw, num_ret_samples=K))
        for e in range(E):
            rows = np.nonzero(inc_g[e])[0]
            idx = [np.nonzero((all_p[e, rows] == fc_p[e, rows][:, q:q + 1]).all(axis=(0, 2, 3)))[0] for q in range(k_ret)]
            assert all(i.size == 1 for i in idx) and len({int(i[0]) for i in idx}) == k_ret, idx
            assert (lw_p[e] == lw_p[e, :1]).all() and abs(np.exp(lw_p[e, 0]).sum() - 1.0) <= 1e-5
            assert (np.diff(lw_p[e, 0]) >= 0).all()
        eng.close()
        return
    # all K futures, no ranking: against the oracle on every compact episode, the bound of the compact-equivalence check
    b = SC.build_scenes_batched(hum, rob, dt, horizon=H)
    with torch.no_grad():
        for e in range(E):
            rows = np.nonzero(inc_g[e])[0]
            x_T = torch.randn([K * rows.size, H, 2], generator=torch.Generator().manual_seed(seeds[e]))
            ctx = O.encode_context(w.tensors, torch.from_numpy(b["x_st"][e, rows]), torch.from_numpy(b["nbr_sum"][e, rows]),
                                   torch.from_numpy(b["edge_mask"][e, rows]))
            pos = O.integrate(O.denoise(w.tensors, ctx, x_T, sample=K, step=2, joint=True)[None], torch.from_numpy(b["p0"][e, rows])[None], dt)[0]
            ref = pos.numpy().transpose(1, 0, 2, 3)                    # [n, K, H, 2]
            d_po, d_go = ade(fc_p[e, rows][:, :, 1:], ref), ade(fc_g[e, rows][:, :, 1:], ref)
            d_pg = ade(fc_p[e, rows][:, :, 1:], fc_g[e, rows][:, :, 1:])
            print(f"predict_batch [{ctx_dim}, {precision}] episode {e} (n = {rows.size}): padded-oracle {d_po:.3e}  padded-grouped {d_pg:.3e}  "
                  f"grouped-oracle {d_go:.3e}")
            assert d_po <= ADE_GATE and d_pg <= 2.0 * d_go, (e, d_po, d_pg, d_go)      # per episode, as the compact-equivalence check
    eng.close()


def test_padded_entries_refuse_bad_counts_and_unsupported_forms():
    from safe_interactive_crowdnav_amd.forecaster import predict_batch
    z, eng, _, (A, K, T), n = load("padded_w32_e3a3k5t6.npz")
    for bad in ([0, 3, 1], [2, A + 1, 1], [-1, 1, 1]):
        with pytest.raises(JmidError) as ei:
            eng.denoise(z["x"], z["ctx"], precision="f32", n_agents=np.array(bad))
        assert ei.value.code == -1
        with pytest.raises(JmidError) as ei:
            eng.net_eval(z["x"], z["ctx"], precision="f32", n_agents=np.array(bad))
        assert ei.value.code == -1
        with pytest.raises(JmidError) as ei:
            eng.topk(np.zeros((3, K, A, T, 2), np.float32), 2, n_agents=np.array(bad))
        assert ei.value.code == -1
    lib, h = eng._lib, eng._h
    x, ctx = np.ascontiguousarray(z["x"]), np.ascontiguousarray(z["ctx"])
    out = np.empty((3, K, A, T, 2), np.float32)
    xp, cp, op = (C.c_void_p(a.ctypes.data) for a in (x, ctx, out))
    assert lib.jmid_denoise_padded(h, 3, A, K, T, None, xp, cp, None, 0.25, 0, op, None, 0) == -1
    assert lib.jmid_net_eval_padded(h, 3, A, K, T, None, 0, xp, cp, 0, op, 0) == -1
    assert lib.jmid_topk_padded(h, 3, A, K, T, 2, None, op, None, op, op, 0) == -1
    assert lib.jmid_predict_padded(h, 3, A, K, T, K, None, xp, xp, xp, xp, xp, 0.25, 0, None, None, None, op) == -1
    with pytest.raises(ValueError):
        eng.denoise(None, z["ctx"], precision="f32", seed=1, episode_ids=[0, 1, 2], K=K, T=T, n_agents=n)
    # DDPM has no padded form
    eng.set_step(int(z["step"]), sampling="ddpm")
    try:
        with pytest.raises(JmidError) as ei:
            eng.denoise(z["x"], z["ctx"], precision="f32", n_agents=n)
        assert ei.value.code == -1
    finally:
        eng.set_step(int(z["step"]))
    # the A/B attention knobs have no masked kernel (head_dim 128)
    zw, engw, _, _, nw = load(WIDE_FIRST)
    engw.set_tuning("attn_sm", 2)
    try:
        with pytest.raises(JmidError) as ei:
            engw.denoise(zw["x"], zw["ctx"], precision="f16mx", n_agents=nw)
        assert ei.value.code == -1
    finally:
        engw.set_tuning("attn_sm", 0)
    # "attn_pf" = 2 (one-step fragment reads) has no masked form in the two-term modes; f16x3's one kernel does not depend on it
    engw.set_tuning("attn_pf", 2)
    try:
        with pytest.raises(JmidError) as ei:
            engw.denoise(zw["x"], zw["ctx"], precision="f16x2", n_agents=nw)
        assert ei.value.code == -1
        vel, _ = engw.denoise(zw["x"], zw["ctx"], precision="f16x3", want_pos=False, n_agents=nw)
    finally:
        engw.set_tuning("attn_pf", 0)
    np.testing.assert_array_equal(vel, engw.denoise(zw["x"], zw["ctx"], precision="f16x3", want_pos=False, n_agents=nw)[0])
    # mixed counts in the scene-resident entry stay JMID_EINVAL; predict_batch says what padded=True does not combine with
    hum, rob = natural_clusters(E=6)
    eng2 = JmidEngine(JMIDWeights.from_seed(NetDims(ctx_dim=32), 5), joint=True, step=2)
    b = eng2.build_scene(hum, rob, 0.25, horizon=8)
    assert len(np.unique(b["n_in"])) > 1
    with pytest.raises(JmidError) as ei:
        eng2.predict_scene(np.zeros((6, 16 * int(b["n_in"].max()), 8, 2), np.float32), 16, dt=0.25, precision="f32")
    assert ei.value.code == -1
    kw = dict(num_samples=16, num_ret_samples=16, horizon=8, time_step=0.25, padded=True)
    for bad in (dict(device_scene=True), dict(device_frames=True), dict(noise="device")):
        with pytest.raises(ValueError, match="padded"):
            predict_batch(eng2, hum, rob, list(range(6)), **kw, **bad)
    eng2.close()
