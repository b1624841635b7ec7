"""Padded chains on the resident scene (include/jmid_hip.h: jmid_noise_fill_padded, jmid_denoise_padded_seeded,
jmid_predict_scene_padded / jmid_forecast_scene_padded and their seeded forms) and ``predict_batch(padded="resident")``: a scene batch of
MIXED in-cluster counts in one call, the counts read where the build kernel wrote them, every episode drawing the noise it draws alone.

Shapes: seeded weights NetDims(ctx_dim=32), step 2, K = 16, H = 8, dt = 0.25; the episodes of tests/test_gpu_padded.py's natural_clusters.
Six of them show two different counts only, so E = 8 - the smallest batch of that generator with three (asserted in ``batch``)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import tests.test_gpu_parity as P      # ade() and the project's ADE gate
from oracle import jmid_oracle as O
from safe_interactive_crowdnav_amd import _lib, noise as NZ, scene as SC
from safe_interactive_crowdnav_amd.engine import JmidEngine, JmidError
from safe_interactive_crowdnav_amd.forecaster import predict_batch
from safe_interactive_crowdnav_amd.weights import JMIDWeights, NetDims

K, H, DT, F, STEP, WSEED = 16, 8, 0.25, 6, 2, 5
ADE_GATE, ade = P.ADE_GATE, P.ade
_ENGINES = {}


def weights():
    return JMIDWeights.from_seed(NetDims(ctx_dim=32), WSEED)


def fresh_engine():
    return JmidEngine(weights(), joint=True, hist_len=F, step=STEP)


def engine_for():
    if "e" not in _ENGINES:
        _ENGINES["e"] = fresh_engine()
    return _ENGINES["e"]


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype
    assert np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def natural_clusters(E=24, F=6, N=6, dt=0.25):
    """the generator of tests/test_gpu_padded.py (and of tests/test_gpu_forecaster.py's ragged-batch test)"""
    rng = np.random.default_rng(17)
    pos0 = rng.uniform(-5.0, 5.0, (E, N, 2))
    vel = rng.uniform(-1.0, 1.0, (E, N, 2))
    t = np.arange(F) * dt
    hum = pos0[:, None] + vel[:, None] * t[None, :, None, None] + 0.01 * rng.standard_normal((E, F, N, 2))
    rob = np.array([0.0, -3.0])[None, None] + 0.02 * rng.standard_normal((E, F, 2))
    return hum, rob


@functools.lru_cache(maxsize=None)
def batch():
    """-> (hum, rob, the host twin's scene batch, counts).  E = 8: no smaller batch of the generator has three different counts."""
    for E in range(1, 8):
        n = SC.build_scenes_batched(*natural_clusters(E), DT, horizon=H)["in_cluster"].sum(axis=1)
        assert len(np.unique(n)) < 3 or n.min() < 1, (E, n)
    hum, rob = natural_clusters(8)
    b = SC.build_scenes_batched(hum, rob, DT, horizon=H)
    n = b["in_cluster"].sum(axis=1)
    assert n.tolist() == [3, 2, 2, 3, 3, 2, 1, 3]          # three different counts, none empty
    return hum, rob, b, n


def padded_x_T(n, A, fill=np.nan):
    """torch noise per episode, [K * n_e, H, 2] from its own seed, scattered; ``fill`` in the padded rows (never read)"""
    x = SC.pad_samples([torch.randn([K * int(ne), H, 2], generator=torch.Generator().manual_seed(100 + e)).numpy() for e, ne in enumerate(n)],
                       n, A, K)
    pad = np.broadcast_to((np.arange(A)[None, :] >= np.asarray(n)[:, None])[:, None, :], (len(n), K, A))
    x.reshape(len(n), K, A, H, 2)[pad] = fill
    return x, pad


# ------------------------------------------------------------------------------------------------ 1. the noise
# (counts, A, K, T, ids, draw, seed): the twin test's case (n_e = 1: 30 elements, a block in two rows, a half-used last block) and one of
# several workgroups per episode with an id and a seed in the high bits
NOISE_CASES = [
    ([1, 3, 2], 3, 5, 3, [7, 0, 41], 0, 0x1234_5678_9ABC),
    ([4, 1, 3], 4, 64, 12, [5, 4294967295, 0], 3, (1 << 40) + 9),
]


@pytest.mark.parametrize("case", NOISE_CASES, ids=["a3k5t3", "a4k64t12"])
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_padded_noise_equals_the_twin_and_every_episodes_own_draw(case, device):
    """The rule of tests/test_gpu_noise.py::test_normals_equal_the_host_twin against ``noise.fill_padded``; against the device's own
    per-episode draw there is nothing to round differently: the same bits."""
    n, A, Kc, T, ids, draw, seed = case
    eng = engine_for()
    got = eng.noise(seed, ids, Kc * A, T, draw=draw, device=device, n_agents=n)
    got = got.cpu().numpy() if device else got
    want = NZ.fill_padded(seed, ids, n, A, Kc, T, draw)
    assert got.shape == want.shape == (len(n), Kc * A, T, 2) and got.dtype == np.float32
    real = ~np.isnan(want)
    assert np.array_equal(np.isnan(got), ~real)
    g, w = got[real], want[real]
    differ = int((g.view(np.uint32) != w.view(np.uint32)).sum())
    ulp = np.spacing(np.maximum(np.abs(g), np.abs(w)))
    worst = float((np.abs(g.astype(np.float64) - w.astype(np.float64)) / ulp).max())
    print(f"{g.size} values: {differ} not bit-identical, worst difference {worst:.2f} ulp, max |z| {np.abs(g).max():.3f}")
    assert np.abs(g).max() <= 6.67
    assert worst <= 1.0
    assert differ * (1 << 16) <= g.size
    gv = got.reshape(len(n), Kc, A, T, 2)
    for e, ne in enumerate(n):
        same_bits(np.ascontiguousarray(gv[e, :, :ne]).reshape(Kc * ne, T, 2), eng.noise(seed, ids[e:e + 1], Kc * ne, T, draw=draw)[0])


@pytest.mark.parametrize("precision", ["f32", "f16mx"])
def test_denoise_padded_seeded_equals_the_padded_call_fed_the_padded_draw(precision):
    eng = engine_for()
    n, A, ids = np.array([3, 1, 2], np.int32), 3, [11, 3, 7]
    g = torch.Generator().manual_seed(3)
    ctx, p0 = torch.randn([3, A, 32], generator=g).numpy(), torch.randn([3, A, 2], generator=g).numpy()
    x_T = eng.noise(9, ids, K * A, H, n_agents=n)
    want = eng.denoise(x_T, ctx, p0, dt=DT, precision=precision, n_agents=n)
    got = eng.denoise_padded_seeded(ctx, p0, n, 9, ids, K, H, dt=DT, precision=precision)
    same_bits(got[0], want[0])
    same_bits(got[1], want[1])
    assert np.isnan(got[1][1, :, 1:]).all() and np.isfinite(got[1][1, :, :1]).all()
    dev = eng.denoise_padded_seeded(torch.from_numpy(ctx).cuda(), torch.from_numpy(p0).cuda(), n, 9, ids, K, H, dt=DT, precision=precision)
    torch.cuda.synchronize()
    same_bits(dev[1].cpu().numpy(), want[1])
    # DDIM only, exactly like jmid_denoise_padded
    eng.set_step(STEP, sampling="ddpm")
    try:
        with pytest.raises(JmidError) as ei:
            eng.denoise_padded_seeded(ctx, p0, n, 9, ids, K, H, dt=DT, precision=precision)
        assert ei.value.code == -1
    finally:
        eng.set_step(STEP)


# ------------------------------------------------------------------------------------------------ 2. the chains
@functools.lru_cache(maxsize=None)
def chain(precision, k):
    """The mixed batch through jmid_predict_scene_padded and jmid_forecast_scene_padded (explicit x_T, NaN in its padded rows) and
    through jmid_predict_padded fed the gathered rows of jmid_scene_get - computed once per (precision, k)."""
    hum, rob, _, n = batch()
    eng = engine_for()
    b = eng.build_scene(hum, rob, DT, horizon=H)
    np.testing.assert_array_equal(b["n_in"], n)
    arr, inc, A, E = eng.scene_arrays(), b["in_cluster"], int(n.max()), len(n)
    x_T, pad = padded_x_T(n, A)
    rows, lw = eng.predict_scene_padded(x_T, k, dt=DT, precision=precision)
    fc, fclw = eng.forecast_scene_padded(x_T, k, dt=DT, precision=precision)
    host = eng.predict_padded(SC.pad_agents(arr["x_st"], inc, A).reshape(E * A, F, 6), SC.pad_agents(arr["nbr_sum"], inc, A).reshape(E * A, 2, F, 6),
                              SC.pad_agents(arr["edge_mask"], inc, A).reshape(E * A, 2), x_T, SC.pad_agents(arr["p0"], inc, A), k, n,
                              dt=DT, precision=precision)
    return dict(b=b, n=n, A=A, pad=pad, x_T=x_T, rows=rows, lw=lw, fc=fc, fclw=fclw, host=host, pose=hum[:, -1])


CHAINS = [("f32", K), ("f32", 5), ("f16mx", K), ("f16mx", 5)]


@pytest.mark.parametrize("precision,k", CHAINS)
def test_predict_scene_padded_has_the_bits_of_predict_padded_on_the_gathered_rows(precision, k):
    c = chain(precision, k)
    same_bits(c["rows"], c["host"][0])
    if k < K:
        same_bits(c["lw"], c["host"][1])
        real = np.arange(c["A"])[None, :] < c["n"][:, None]
        assert np.isnan(c["rows"][~real]).all() and np.isnan(c["lw"][~real]).all()
        assert np.isfinite(c["rows"][real]).all() and np.isfinite(c["lw"][real]).all()
    else:
        assert c["lw"] is None
        assert np.isnan(c["rows"][c["pad"]]).all() and np.isfinite(c["rows"][~c["pad"]]).all()


@pytest.mark.parametrize("precision,k", CHAINS)
def test_forecast_scene_padded_is_the_host_assembly_of_the_padded_rows(precision, k):
    c = chain(precision, k)
    b, inc = c["b"], c["b"]["in_cluster"]
    want_fc, want_lw = SC.assemble_forecasts(inc, c["rows"], c["lw"], b["cv"], c["pose"], k, K, n_agents=c["n"])
    same_bits(c["fc"], want_fc)
    same_bits(c["fclw"], want_lw)
    assert np.isfinite(c["fc"]).all() and np.isfinite(c["fclw"]).all()
    assert (~inc).any()
    same_bits(c["fc"][~inc][:, :, 1:], np.repeat(b["cv"][~inc][:, None], k, axis=1))
    same_bits(c["fc"][:, :, :, 0], np.repeat(c["pose"][:, :, None], k, axis=2))


@pytest.mark.parametrize("precision", ["f32", "f16mx"])
def test_a_batch_of_equal_counts_has_the_bits_of_the_plain_scene_entries(precision):
    hum, rob, _, n = batch()
    eps = np.nonzero(n == 2)[0]
    eng = engine_for()
    b = eng.build_scene(hum[eps], rob[eps], DT, horizon=H)
    assert b["n_in"].tolist() == [2] * len(eps) and len(eps) == 3
    x_T, _ = padded_x_T(n[eps], 2)
    ids = [4, 9, 2]
    for k in (K, 5):
        same_bits(eng.forecast_scene_padded(x_T, k, dt=DT, precision=precision)[0], eng.forecast_scene(x_T, k, dt=DT, precision=precision)[0])
        got = eng.forecast_scene_padded(None, k, dt=DT, precision=precision, seed=5, episode_ids=ids, K=K, T=H)
        want = eng.forecast_scene(None, k, dt=DT, precision=precision, seed=5, episode_ids=ids, K=K, T=H)
        same_bits(got[0], want[0])
        same_bits(got[1], want[1])
        got, want = eng.predict_scene_padded(x_T, k, dt=DT, precision=precision), eng.predict_scene(x_T, k, dt=DT, precision=precision)
        same_bits(got[0], want[0])
        if k < K:
            same_bits(got[1], want[1])


@pytest.mark.parametrize("precision,k", [("f32", K), ("f16mx", 5)])
def test_the_seeded_chains_equal_the_explicit_ones_fed_the_padded_draw(precision, k):
    hum, rob, _, n = batch()
    eng = engine_for()
    ids = np.arange(40, 48)
    eng.build_scene(hum, rob, DT, horizon=H)
    A = int(n.max())
    x_T = eng.noise(77, ids, K * A, H, draw=0, n_agents=n)
    assert np.isnan(x_T).any()                                    # the padded rows of the draw: never read
    want_fc = eng.forecast_scene_padded(x_T, k, dt=DT, precision=precision)
    got = eng.forecast_scene_padded(None, k, dt=DT, precision=precision, seed=77, episode_ids=ids, K=K, T=H)
    same_bits(got[0], want_fc[0])
    same_bits(got[1], want_fc[1])
    want = eng.predict_scene_padded(x_T, k, dt=DT, precision=precision)
    got = eng.predict_scene_padded(None, k, dt=DT, precision=precision, seed=77, episode_ids=ids, K=K, T=H)
    same_bits(got[0], want[0])
    if k < K:
        same_bits(got[1], want[1])
    other = eng.forecast_scene_padded(None, k, dt=DT, precision=precision, seed=77, episode_ids=ids[::-1].copy(), K=K, T=H)
    assert not np.array_equal(other[0], want_fc[0])                # the ids are part of the address


def test_padded_rows_hold_nothing_of_the_previous_call():
    """Counts [3, 1, 2], then [1, 3, 2] on the same handle: the rows that were real in the first call are padding in the second (and the
    other way round) - the second result is the one of a handle that never saw the first."""
    hum, rob, _, n = batch()
    first, second = [0, 6, 1], [6, 0, 1]
    assert n[first].tolist() == [3, 1, 2] and n[second].tolist() == [1, 3, 2]
    used, clean = fresh_engine(), fresh_engine()
    try:
        x1, _ = padded_x_T(n[first], 3, fill=7.0)
        x2, pad2 = padded_x_T(n[second], 3)
        used.build_scene(hum[first], rob[first], DT, horizon=H)
        used.forecast_scene_padded(x1, 5, dt=DT, precision="f32")
        used.predict_scene_padded(x1, K, dt=DT, precision="f32")
        out = []
        for eng in (used, clean):
            eng.build_scene(hum[second], rob[second], DT, horizon=H)
            out.append((eng.forecast_scene_padded(x2, 5, dt=DT, precision="f32"), eng.predict_scene_padded(x2, K, dt=DT, precision="f32")[0],
                        eng.predict_scene_padded(None, 5, dt=DT, precision="f32", seed=3, episode_ids=[0, 1, 2], K=K, T=H)))
        (fa, pa, sa), (fb, pb, sb) = out
        same_bits(fa[0], fb[0])
        same_bits(fa[1], fb[1])
        same_bits(pa, pb)
        same_bits(sa[0], sb[0])
        same_bits(sa[1], sb[1])
        assert np.isnan(pa[pad2]).all() and np.isfinite(pa[~pad2]).all() and np.isfinite(fa[0]).all()
    finally:
        used.close()
        clean.close()


# ------------------------------------------------------------------------------------------------ 3. predict_batch
def oracle_positions(w, ctx, x_T, p0):
    """oracle/ on one compact episode: ctx [n, 2 H], x_T [K n, H, 2], p0 [n, 2] -> positions [n, K, H, 2]"""
    with torch.no_grad():
        vel = O.denoise(w.tensors, torch.from_numpy(ctx), torch.from_numpy(x_T), sample=K, step=STEP, joint=True)
        return O.integrate(vel[None], torch.from_numpy(p0)[None], DT)[0].numpy().transpose(1, 0, 2, 3)


def check_resident_against_grouped(eng, hum, rob, b, precision, k, short, oracle_ctx):
    """``padded="resident"`` against the grouped device path, both with device noise - the checks of
    tests/test_gpu_padded.py::test_predict_batch_padded_against_the_grouped_path, plus bit equality wherever nothing is rounded differently."""
    E = hum.shape[0]
    gids, seed = [1000 + e for e in range(E)], 31
    kw = dict(num_samples=K, num_ret_samples=k, horizon=H, time_step=DT, precision=precision, noise="device", seed=seed, short_history=short)
    fc_g, lw_g, inc_g = predict_batch(eng, hum, rob, gids, device_frames=True, **kw)
    fc_p, lw_p, inc_p = predict_batch(eng, hum, rob, gids, padded="resident", **kw)
    n, w = inc_g.sum(axis=1), weights()
    A = int(n.max())
    assert len(np.unique(n)) >= 3 and n.min() >= 1
    np.testing.assert_array_equal(inc_p, inc_g)
    same_bits(fc_p[~inc_g], fc_g[~inc_g])                          # constant-velocity rows
    assert np.isfinite(fc_p).all() and np.isfinite(lw_p).all()
    full = np.nonzero(n == A)[0]
    assert full.size >= 1
    same_bits(fc_p[full], fc_g[full])                              # an episode without padding: the grouped call's bits
    same_bits(lw_p[full], lw_g[full])
    all_p = fc_p if k == K else predict_batch(eng, hum, rob, gids, padded="resident", **dict(kw, num_ret_samples=K))[0]
    for e in np.nonzero(n < A)[0]:
        rows = np.nonzero(inc_g[e])[0]
        if k < K:
            # ranked: the kept forecasts are k distinct ones of the K futures of the same padded call, bit for bit, the same ones for every
            # agent of the episode, with one normalised weight row per episode in ascending order
            idx = [np.nonzero((all_p[e, rows] == fc_p[e, rows][:, q:q + 1]).all(axis=(0, 2, 3)))[0] for q in range(k)]
            assert all(i.size == 1 for i in idx) and len({int(i[0]) for i in idx}) == k, idx
            assert (lw_p[e] == lw_p[e, :1]).all() and abs(np.exp(lw_p[e, 0]).sum() - 1.0) <= 1e-5
            assert (np.diff(lw_p[e, 0]) >= 0).all()
            continue
        x_T = eng.noise(seed, [gids[e]], K * rows.size, H)[0]      # the draw of the episode alone: what both paths gave it
        ref = oracle_positions(w, oracle_ctx(e, rows), x_T, b["p0"][e, rows])
        d_po, d_go = ade(fc_p[e, rows][:, :, 1:], ref), ade(fc_g[e, rows][:, :, 1:], ref)
        d_pg = ade(fc_p[e, rows][:, :, 1:], fc_g[e, rows][:, :, 1:])
        print(f"padded=resident [{precision}, short={short}] episode {e} (n = {rows.size}): padded-oracle {d_po:.3e}  padded-grouped {d_pg:.3e}  "
              f"grouped-oracle {d_go:.3e}")
        assert d_po <= ADE_GATE and d_pg <= 2.0 * d_go, (e, d_po, d_pg, d_go)


@pytest.mark.parametrize("precision,k", [("f32", K), ("f16mx", K), ("f16x3", 5)])
def test_predict_batch_resident_padded_against_the_count_groups(precision, k):
    hum, rob, b, _ = batch()
    w = weights()

    def ctx(e, rows):
        with torch.no_grad():
            return O.encode_context(w.tensors, torch.from_numpy(b["x_st"][e, rows]), torch.from_numpy(b["nbr_sum"][e, rows]),
                                    torch.from_numpy(b["edge_mask"][e, rows])).numpy()
    check_resident_against_grouped(engine_for(), hum, rob, b, precision, k, False, ctx)


@pytest.mark.parametrize("precision,k", [("f32", K), ("f16mx", 5)])
def test_predict_batch_resident_padded_takes_short_windows(precision, k):
    """Windows of L = 3 frames through jmid_build_scene_var: the padded short-history form jmid_predict_padded cannot have.  oracle/
    restates the encoder for full-length rows only, so its context here is jmid_encode_var's on the compact rows (rows are independent:
    the same bits on both paths); the denoise loop and the integrator are the oracle's."""
    hum, rob, _, _ = batch()
    hum, rob = hum[:, -3:], rob[:, -3:]
    parts = [SC.pad_short_window(hum[e], rob[e], F) for e in range(hum.shape[0])]
    hp, rp, ff = (np.stack([p[i] for p in parts]) for i in range(3))
    assert (ff == F - 3).all()
    b = SC.build_scenes_batched(hp, rp, DT, horizon=H, first_frame=ff)
    eng = engine_for()

    def ctx(e, rows):
        return eng.encode(b["x_st"][e, rows], b["nbr_sum"][e, rows], b["edge_mask"][e, rows], first_index=b["first_index"][e, rows])
    check_resident_against_grouped(eng, hum, rob, b, precision, k, True, ctx)


# ------------------------------------------------------------------------------------------------ 4. refusals, the captured loop
def test_refusals_leave_the_scene_resident():
    hum, rob, _, n = batch()
    eng = fresh_engine()
    lib, h = eng._lib, eng._h
    ptr = lambda a: C.c_void_p(a.ctypes.data)
    E, N, A = len(n), hum.shape[2], int(n.max())
    x_T = np.zeros((E, K * (A + 1), H, 2), np.float32)
    ids = np.arange(E, dtype=np.uint32)
    pos, fc, lw = np.empty((E, K, A + 1, H, 2), np.float32), np.empty((E, N, K, H + 1, 2)), np.empty((E, N, K))

    def calls(E, A):
        return [lib.jmid_predict_scene_padded(h, E, A, K, H, K, ptr(x_T), DT, _lib.PREC_F32, None, None, None, ptr(pos)),
                lib.jmid_forecast_scene_padded(h, E, A, K, H, K, ptr(x_T), DT, _lib.PREC_F32, None, ptr(fc), ptr(lw)),
                lib.jmid_predict_scene_padded_seeded(h, E, A, K, H, K, 5, ptr(ids), DT, _lib.PREC_F32, None, None, None, ptr(pos)),
                lib.jmid_forecast_scene_padded_seeded(h, E, A, K, H, K, 5, ptr(ids), DT, _lib.PREC_F32, None, ptr(fc), ptr(lw))]

    try:
        assert calls(E, A) == [-1] * 4 and b"jmid_build_scene" in lib.jmid_last_error(h)          # no resident scene
        eng.build_scene(hum, rob, DT, horizon=H)
        resident = eng.scene_arrays()
        good = eng.forecast_scene_padded(None, K, dt=DT, precision="f32", seed=5, episode_ids=ids, K=K, T=H)

        def survived():
            now = eng.scene_arrays()
            for key in resident:
                same_bits(now[key], resident[key])
            again = eng.forecast_scene_padded(None, K, dt=DT, precision="f32", seed=5, episode_ids=ids, K=K, T=H)
            same_bits(again[0], good[0])

        for bad_A in (A - 1, A + 1):                                                                # not the largest count
            assert calls(E, bad_A) == [-1] * 4 and b"largest" in lib.jmid_last_error(h)
            survived()
        assert calls(E - 1, A) == [-1] * 4                                                          # another E
        assert lib.jmid_predict_scene_padded(h, E, A, K, H, K, None, DT, _lib.PREC_F32, None, None, None, ptr(pos)) == -1
        assert lib.jmid_forecast_scene_padded_seeded(h, E, A, K, H, K, 5, None, DT, _lib.PREC_F32, None, ptr(fc), ptr(lw)) == -1
        survived()
        eng.set_step(STEP, sampling="ddpm")                                                         # a DDPM table on the handle
        try:
            assert calls(E, A) == [-1] * 4 and b"DDIM" in lib.jmid_last_error(h)
        finally:
            eng.set_step(STEP)
        survived()
        # an empty cluster: one-frame tracks are no ego rows
        ff = np.zeros((2, N + 1), np.int32)
        ff[1, 1:] = F - 1
        b = eng.build_scene(hum[:2], rob[:2], DT, horizon=H, first_frame=ff)
        assert b["n_in"].tolist() == [int(n[0]), 0]
        var_scene = eng.scene_arrays()
        assert calls(2, int(n[0])) == [-1] * 4 and b"no in-cluster" in lib.jmid_last_error(h)
        now = eng.scene_arrays()
        for key in var_scene:
            same_bits(now[key], var_scene[key])
        # mixed counts in the plain entry stay refused
        eng.build_scene(hum, rob, DT, horizon=H)
        with pytest.raises(JmidError) as ei:
            eng.predict_scene(np.zeros((E, K * A, H, 2), np.float32), K, dt=DT, precision="f32")
        assert ei.value.code == -1
        # the noise entry
        out = np.empty((3, K * 3, H, 2), np.float32)
        cnt = np.array([3, 1, 2], np.int32)
        fill = lambda **kw: lib.jmid_noise_fill_padded(h, 5, *[kw.get(key, v) for key, v in (("E", 3), ("A", 3), ("K", K), ("T", H))],
                                                       kw.get("n", ptr(cnt)), kw.get("ids", ptr(ids)), kw.get("draw", 0), kw.get("out", ptr(out)),
                                                       _lib.MEM_HOST)
        assert fill() == 0
        for bad in (dict(E=0), dict(A=0), dict(K=0), dict(T=0), dict(draw=-1), dict(n=None), dict(ids=None), dict(out=None), dict(A=2),
                    dict(n=ptr(np.array([3, 0, 2], np.int32)))):
            assert fill(**bad) == -1, bad
    finally:
        eng.close()


def test_graph_replays_take_other_resident_counts_of_the_same_shape():
    """As tests/test_gpu_padded.py::test_graph_replay_and_imid_take_other_counts_of_the_same_shape: the counts reach the captured loop
    through the mask words and the zeroed rows, written outside it - here from the counts the build kernel left on the device."""
    hum, rob, _, n = batch()
    scenes = [[0, 6, 1], [6, 0, 1], [5, 2, 3]]
    assert [n[s].tolist() for s in scenes] == [[3, 1, 2], [1, 3, 2], [2, 2, 3]]
    eng = fresh_engine()
    try:
        def run(s):
            eng.build_scene(hum[s], rob[s], DT, horizon=H)
            return eng.predict_scene_padded(None, K, dt=DT, precision="f32", seed=13, episode_ids=s, K=K, T=H)[0]
        eager = [run(s) for s in scenes]
        eng.set_tuning("graph", 1)
        r0 = eng.graph_replays()
        for _ in range(2):
            for s, ref in zip(scenes, eager):
                same_bits(run(s), ref)
        assert eng.graph_replays() > r0
    finally:
        eng.close()
