"""Constraints in the one-entry chains (include/jmid_hip.h: jmid_predict_constrained, jmid_predict_scene_constrained,
jmid_forecast_scene_constrained; ``constraints=`` of the engine's chained methods): guided sampling inside the chain's denoise stage, the
repair between that stage and the ranking, the reports in the one download.

THE RULE is a composition, so every comparison is bit-equality against the staged composition made from the engine's existing methods
(tests/chain_constraint_cases.py).  Every non-trivial case also asserts that the equality is not vacuous: the staged route reports a guided
sample and a repair candidate where the mode has the mechanism, and the constrained result differs from the unconstrained chain."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import tests.chain_constraint_cases as CC
from safe_interactive_crowdnav_amd import _lib
from safe_interactive_crowdnav_amd.engine import ChainConstraints, ChainReport, JmidError, kde_bandwidths
from safe_interactive_crowdnav_amd.schedule import guidance_weights

THR, DT, same_bits = CC.THR, CC.DT, CC.same_bits
PRECISIONS = ["f32", "f16mx"]


def not_vacuous(mode, want, got_rows, plain_rows):
    """The three assertions that go with every equality: the staged route saw the mechanisms fire, and the constraints changed a bit."""
    report = want[2]
    if mode != "repair":
        assert report["guide"][..., 0].sum() >= 1, "no sample was guided: choose another seed"
    if mode != "guide":
        assert report["episode"][:, 0].sum() >= 1, "no repair candidate: choose another seed"
    assert not same_bits(got_rows, plain_rows), "the constrained chain equals the unconstrained one"


def check(mode, got, want, plain):
    assert len(got) == 3 and isinstance(got[2], ChainReport)
    assert same_bits(got[0], want[0])
    assert (got[1] is None and want[1] is None) or same_bits(got[1], want[1])
    assert CC.same_report(got[2], want[2]) == []
    not_vacuous(mode, want, got[0], plain[0])


# ------------------------------------------------------------------------------------------------ 1. host arrays
HOST = dict(E=2, A=3, K=4, T=8, seed=11)


@functools.lru_cache(maxsize=None)
def host_inputs():
    return CC.host_inputs(HOST["E"], HOST["A"], HOST["K"], HOST["T"], HOST["seed"])


@pytest.mark.parametrize("mode", CC.MODES)
@pytest.mark.parametrize("k", [2, 4])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_predict_constrained_is_the_staged_composition(precision, k, mode):
    eng, inp, cons = CC.engine_for(), host_inputs(), CC.constraints(mode)
    plain = eng.predict(*inp, k, dt=DT, precision=precision)
    got = eng.predict(*inp, k, dt=DT, precision=precision, constraints=cons)
    want = CC.staged_predict(eng, inp, k, precision, cons)
    print(f"{precision} k={k} {mode}: guide {None if want[2]['guide'] is None else want[2]['guide'][..., 0].sum()}, "
          f"episode {None if want[2]['episode'] is None else want[2]['episode'].tolist()}")
    check(mode, got, want, plain)
    assert same_bits(eng.predict(*inp, k, dt=DT, precision=precision)[0], plain[0])      # the unconstrained chain is what it was


PADDED = dict(E=3, A=4, K=3, T=6, counts=(4, 1, 2), seed=23)


@functools.lru_cache(maxsize=None)
def padded_inputs():
    x_st, nbr, em, x_T, p0 = CC.host_inputs(PADDED["E"], PADDED["A"], PADDED["K"], PADDED["T"], PADDED["seed"])
    p0[1, 0] = (0.35, 0.1)      # the single agent of episode 1 starts next to both walls
    return x_st, nbr, em, x_T, p0


@pytest.mark.parametrize("mode", ["both", "both_walls"])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_predict_padded_constrained(precision, mode):
    eng, inp, cons, n = CC.engine_for(), padded_inputs(), CC.constraints(mode), np.array(PADDED["counts"], np.int32)
    k, K, A = 2, PADDED["K"], PADDED["A"]
    plain = eng.predict_padded(*inp, k, n, dt=DT, precision=precision)
    got = eng.predict_padded(*inp, k, n, dt=DT, precision=precision, constraints=cons)
    want = CC.staged_predict(eng, inp, k, precision, cons, n_agents=n)
    check(mode, got, want, plain)
    real = np.arange(A)[None, :] < n[:, None]
    assert np.isnan(got[0][~real]).all() and np.isnan(got[1][~real]).all() and np.isfinite(got[0][real]).all()
    # the single-agent episode iterates only with walls
    touched = got[2].guide[1, :, 1].sum() + (got[2].sample[1, :, 3] != 0).sum()
    print(f"{precision} {mode}: episode 1 (one agent) guide iterations + repair states {touched}, episode rows {got[2].episode.tolist()}")
    assert (touched >= 1) == (mode == "both_walls")
    if mode == "both_walls":
        assert got[2].wall is not None and np.isfinite(got[2].wall).all()
    # all K samples: pos_out is the repaired set
    allk = eng.predict_padded(*inp, K, n, dt=DT, precision=precision, constraints=cons)
    want = CC.staged_predict(eng, inp, K, precision, cons, n_agents=n)
    assert same_bits(allk[0], want[0]) and allk[1] is None and CC.same_report(allk[2], want[2]) == []


# ------------------------------------------------------------------------------------------------ 2. the resident scene
SCENE = dict(E=2, N=3, K=4, H=8, seed=7, ids=(5, 9))


@functools.lru_cache(maxsize=None)
def scene_x_T():
    return CC.host_inputs(SCENE["E"], SCENE["N"], SCENE["K"], SCENE["H"], 31)[3]


def build_forced(eng):
    hum, rob = CC.crowd(SCENE["E"], SCENE["N"], SCENE["seed"])
    b = eng.build_scene(hum, rob, DT, horizon=SCENE["H"], force_all_in_cluster=True)
    assert b["n_in"].tolist() == [SCENE["N"]] * SCENE["E"]
    return b, hum[:, -1]


@pytest.mark.parametrize("mode", CC.MODES)
@pytest.mark.parametrize("seeded", [False, True], ids=["x_T", "seeded"])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_scene_chains_constrained(precision, seeded, mode):
    eng, cons, K, H = CC.engine_for(), CC.constraints(mode), SCENE["K"], SCENE["H"]
    b, pose = build_forced(eng)
    nz = dict(seed=77, episode_ids=list(SCENE["ids"]), K=K, T=H) if seeded else {}
    x_T = None if seeded else scene_x_T()
    for k in (2, K):
        plain = eng.predict_scene(x_T, k, dt=DT, precision=precision, **nz)
        got = eng.predict_scene(x_T, k, dt=DT, precision=precision, constraints=cons, **nz)
        want = CC.staged_scene(eng, b, pose, K, H, k, precision, cons, x_T=x_T, seeded=nz)
        check(mode, got, want, plain)
    plain = eng.forecast_scene(x_T, 2, dt=DT, precision=precision, **nz)
    got = eng.forecast_scene(x_T, 2, dt=DT, precision=precision, constraints=cons, **nz)
    want = CC.staged_scene(eng, b, pose, K, H, 2, precision, cons, x_T=x_T, seeded=nz, forecast=True)
    check(mode, got, want, plain)
    assert same_bits(eng.forecast_scene(x_T, 2, dt=DT, precision=precision, **nz)[0], plain[0])


@pytest.mark.parametrize("mode", CC.MODES)
@pytest.mark.parametrize("precision", PRECISIONS)
def test_padded_seeded_scene_chains_on_short_windows(precision, mode):
    eng, cons, K, H = CC.engine_for(), CC.constraints(mode), 4, 8
    hum, rob, ff = CC.mixed_crowd()
    b = eng.build_scene(hum, rob, DT, horizon=H, first_frame=ff)
    n = b["n_in"]
    assert len(np.unique(n)) > 1 and n.min() >= 1 and eng.scene_arrays()["first_index"].any(), n
    nz = dict(seed=3, episode_ids=[4, 40, 400], K=K, T=H)
    for k in (2, K):
        plain = eng.predict_scene_padded(None, k, dt=DT, precision=precision, **nz)
        got = eng.predict_scene_padded(None, k, dt=DT, precision=precision, constraints=cons, **nz)
        want = CC.staged_scene(eng, b, hum[:, -1], K, H, k, precision, cons, seeded=nz, padded=True)
        check(mode, got, want, plain)
    plain = eng.forecast_scene_padded(None, 2, dt=DT, precision=precision, **nz)
    got = eng.forecast_scene_padded(None, 2, dt=DT, precision=precision, constraints=cons, **nz)
    want = CC.staged_scene(eng, b, hum[:, -1], K, H, 2, precision, cons, seeded=nz, padded=True, forecast=True)
    check(mode, got, want, plain)
    assert np.isfinite(got[0]).all()
    # the explicit form of the padded chain
    x_T = eng.noise(3, nz["episode_ids"], K * int(n.max()), H, n_agents=n)
    again = eng.forecast_scene_padded(x_T, 2, dt=DT, precision=precision, constraints=cons)
    assert same_bits(again[0], got[0]) and same_bits(again[1], got[1]) and CC.same_report(again[2], want[2]) == []


# ------------------------------------------------------------------------------------------------ 3. constraints that change nothing
@pytest.mark.parametrize("precision", PRECISIONS)
def test_constraints_that_cannot_fire_leave_the_unconstrained_bits(precision):
    eng, inp = CC.engine_for(), host_inputs()
    E, K = HOST["E"], HOST["K"]
    plain = {k: eng.predict(*inp, k, dt=DT, precision=precision) for k in (2, K)}
    zero_table = ChainConstraints(THR, CC.constraints("guide", weights=[0.0, 0.0]).guidance, None)
    for name, cons in (("threshold 0", CC.constraints("both", threshold=0.0)), ("zero table", zero_table)):
        for k in (2, K):
            got = eng.predict(*inp, k, dt=DT, precision=precision, constraints=cons)
            assert same_bits(got[0], plain[k][0]) and (got[1] is None or same_bits(got[1], plain[k][1])), name
            assert not got[2].guide.any(), name
            if got[2].sample is not None:
                assert not got[2].sample[..., 3].any() and not got[2].episode.any(), name
    # the raw entry with everything off: zeros in every report row (state 0 everywhere)
    rows = raw_predict(eng, inp, 2, precision, guide_weights=None, repair=0)
    assert rows["rc"] == 0 and same_bits(rows["sel"], plain[2][0]) and same_bits(rows["logw"], plain[2][1])
    assert not rows["guide"].any() and not rows["sample"].any() and not rows["episode"].any() and not rows["wall"].any()
    # one agent without walls: nothing to push apart
    one = CC.host_inputs(E, 1, K, HOST["T"], 5)
    base = eng.predict(*one, 2, dt=DT, precision=precision)
    got = eng.predict(*one, 2, dt=DT, precision=precision, constraints=CC.constraints("both"))
    assert same_bits(got[0], base[0]) and same_bits(got[1], base[1])
    assert not got[2].guide.any() and not got[2].sample[..., 3].any() and not got[2].episode.any()


# ------------------------------------------------------------------------------------------------ 4. batch mates, chunks
@pytest.mark.parametrize("precision", PRECISIONS)
def test_an_episode_does_not_depend_on_its_batch_mates(precision):
    eng, cons = CC.engine_for(), CC.constraints("both")
    E, A, K, T, k = 4, 3, 4, 8, 2
    inp = CC.host_inputs(E, A, K, T, 41)
    part = lambda lo, hi: tuple(a[lo * A:hi * A] if i < 3 else a[lo:hi] for i, a in enumerate(inp))
    whole = eng.predict(*inp, k, dt=DT, precision=precision, constraints=cons)
    assert whole[2].guide[..., 0].sum() >= 1 and whole[2].episode[:, 0].sum() >= 1
    for lo, hi in ((0, 2), (2, 4)):
        half = eng.predict(*part(lo, hi), k, dt=DT, precision=precision, constraints=cons)
        assert same_bits(half[0], whole[0][lo:hi]) and same_bits(half[1], whole[1][lo:hi])
        assert all(same_bits(a, b[lo:hi]) for a, b in zip(half[2], whole[2]) if a is not None)
    try:
        for chunk in (1, 2, 3):
            eng.set_chunk_episodes(chunk)
            got = eng.predict(*inp, k, dt=DT, precision=precision, constraints=cons)
            assert same_bits(got[0], whole[0]) and same_bits(got[1], whole[1]), chunk
            assert all(same_bits(a, b) for a, b in zip(got[2], whole[2]) if a is not None), chunk
    finally:
        eng.set_chunk_episodes(0)


@pytest.mark.parametrize("mode", ["repair", "both", "both_walls"])
def test_a_nan_episode_is_state_3_as_on_the_staged_route(mode):
    eng, cons, K = CC.engine_for(), CC.constraints(mode), HOST["K"]
    poisoned = tuple(a.copy() for a in host_inputs())
    poisoned[3][1, 2, 3, 0] = np.nan      # one value of episode 1's noise: its joint samples attend to each other, the whole episode is NaN
    got = eng.predict(*poisoned, K, dt=DT, precision="f32", constraints=cons)
    want = CC.staged_predict(eng, poisoned, K, "f32", cons)
    states = got[2].sample[..., 3]
    assert (states[1] == 3).all() and (states[0] != 3).all() and np.isnan(got[2].sample[1, :, :2]).all(), states
    assert same_bits(got[0], want[0]) and CC.same_report(got[2], want[2]) == []
    assert np.isnan(got[0][1]).all() and np.isfinite(got[0][0]).all()


def test_profile_class_counts_one_guide_launch_per_positive_weight_and_chunk():
    eng, inp = CC.engine_for(), host_inputs()
    assert (guidance_weights(0.02, CC.STEP) > 0).all()
    eng.profile_reset()
    eng.profile_enable(["guide"])
    try:
        eng.set_chunk_episodes(1)
        eng.predict(*inp, 2, dt=DT, constraints=CC.constraints("both"))                            # 2 entries x 2 chunks
        eng.predict(*inp, 2, dt=DT, constraints=CC.constraints("guide", weights=[0.0, 0.02]))      # 1 entry x 2 chunks
        eng.predict(*inp, 2, dt=DT, constraints=CC.constraints("repair"))                          # none
        n, _ = eng.profile_get()["guide"]
    finally:
        eng.profile_disable()
        eng.set_chunk_episodes(0)
    assert n == 6


def test_graph_replays_advance_as_on_the_unconstrained_chain_and_never_when_guided():
    inp, calls = host_inputs(), 4

    def replays(cons):
        eng = CC.fresh_engine()
        try:
            want = eng.predict(*inp, 2, dt=DT, constraints=cons)
            eng.set_tuning("graph", 1)
            n0 = eng.graph_replays()
            for _ in range(calls):
                got = eng.predict(*inp, 2, dt=DT, constraints=cons)
                assert same_bits(got[0], want[0]) and same_bits(got[1], want[1])
            return eng.graph_replays() - n0
        finally:
            eng.close()
    plain = replays(None)
    assert plain >= 1
    assert replays(CC.constraints("repair")) == plain
    assert replays(CC.constraints("guide")) == 0 and replays(CC.constraints("both")) == 0


# ------------------------------------------------------------------------------------------------ 5. the raw entries
def ptr(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


GOOD = dict(threshold=THR, guide_weights=guidance_weights(0.02, CC.STEP), n_inner=4, guide_margin=0.02, guide_tau=0.005, guide_walls=0, repair=1,
            margin=0.02, tau=0.005, step=0.02, max_iter=32, repair_walls=0, L=0, walls=None, wall_radius=0.0)


def constraint_args(over):
    c = {**GOOD, **over}
    return (c["threshold"], ptr(c["guide_weights"]), c["n_inner"], c["guide_margin"], c["guide_tau"], c["guide_walls"], c["repair"], c["margin"],
            c["tau"], c["step"], c["max_iter"], c["repair_walls"], c["L"], ptr(c["walls"]), c["wall_radius"]), c


def raw_predict(eng, inp, k, precision="f32", dims=None, null=(), **over):
    """jmid_predict_constrained through ctypes: the status and every output array."""
    x_st, nbr, em, x_T, p0 = (np.ascontiguousarray(a, np.float32) for a in inp)
    E, A, K, T = dims or (p0.shape[0], p0.shape[1], x_T.shape[1] // p0.shape[1], x_T.shape[2])
    out = dict(sel=np.zeros((E, A, max(k, 1), T, 2), np.float32), logw=np.zeros((E, A, max(k, 1)), np.float32), pos=np.zeros((E, K, A, T, 2), np.float32),
               guide=np.ones((E, K, 2), np.float32), sample=np.ones((E, K, 4), np.float32), episode=np.ones((E, 3), np.int32),
               wall=np.ones((E, K, 2), np.float32))
    bw = np.ascontiguousarray(kde_bandwidths(T).numpy())
    args, keep = constraint_args(over)
    ins = dict(x_st=x_st, nbr=nbr, em=em, x_T=x_T, p0=p0)
    out["rc"] = eng._lib.jmid_predict_constrained(eng._h, E, A, K, T, k, None, *[None if key in null else ptr(a) for key, a in ins.items()], DT,
                                                  _lib.PRECISIONS[precision], ptr(bw), *args, ptr(out["sel"]), ptr(out["logw"]), ptr(out["pos"]),
                                                  ptr(out["guide"]), ptr(out["sample"]), ptr(out["episode"]), ptr(out["wall"]))
    return out


def test_raw_entries_refuse_what_their_namesakes_and_the_staged_entries_refuse():
    eng, inp = CC.fresh_engine(), host_inputs()
    try:
        good = raw_predict(eng, inp, 2)
        want = eng.predict(*inp, 2, dt=DT, constraints=CC.constraints("both"))
        assert good["rc"] == 0 and same_bits(good["sel"], want[0]) and same_bits(good["guide"], want[2].guide)
        assert same_bits(good["sample"], want[2].sample) and same_bits(good["episode"], want[2].episode)
        assert np.isinf(good["wall"]).all()      # a repair without walls: jmid_repair_collisions_walls' L = 0
        nan_wall = CC.WALLS.copy()
        nan_wall[1, 2] = np.nan
        bad = [dict(guide_walls=1), dict(repair_walls=1), dict(guide_walls=1, L=2, walls=None), dict(repair_walls=1, L=2, walls=nan_wall),
               dict(L=65), dict(L=-1), dict(guide_weights=np.array([0.02, -1.0])), dict(guide_weights=np.array([np.inf, 0.0])),
               dict(n_inner=0), dict(n_inner=65), dict(guide_tau=0.0), dict(guide_margin=-1.0), dict(threshold=-0.1), dict(threshold=np.nan),
               dict(tau=0.0), dict(step=0.0), dict(margin=np.inf), dict(max_iter=-1), dict(max_iter=1025),
               dict(repair_walls=1, L=2, walls=CC.WALLS, wall_radius=-1.0), dict(guide_walls=1, L=2, walls=CC.WALLS, wall_radius=np.nan)]
        for over in bad:
            assert raw_predict(eng, inp, 2, **over)["rc"] == _lib.EINVAL, over
        # what jmid_predict refuses
        for kw in (dict(k=0), dict(k=5), dict(null=("p0",)), dict(null=("x_T",)), dict(dims=(0, 3, 4, 8))):
            k = kw.pop("k", 2)
            assert raw_predict(eng, inp, k, **kw)["rc"] == _lib.EINVAL, kw
        # T = 1 has no pedestrian segment: the repair entries refuse it, the guided ones do not
        short = CC.host_inputs(2, 3, 4, 1, 3)
        assert raw_predict(eng, short, 2)["rc"] == _lib.EINVAL and raw_predict(eng, short, 2, repair=0)["rc"] == 0
        # the scene entries without a resident scene; a seeded call without ids
        E, A, K, T = HOST["E"], HOST["A"], HOST["K"], HOST["T"]
        args, _keep = constraint_args({})
        fc, lw = np.zeros((E, A, 2, T + 1, 2)), np.zeros((E, A, 2))
        sel, slw = np.zeros((E, A, 2, T, 2), np.float32), np.zeros((E, A, 2), np.float32)
        ids, bw = np.array([1, 2], np.uint32), np.ascontiguousarray(kde_bandwidths(T).numpy())
        scene = lambda ids_ptr: eng._lib.jmid_predict_scene_constrained(eng._h, E, A, K, T, 2, 0, None, 5, ids_ptr, DT, 0, ptr(bw), *args, ptr(sel), ptr(slw),
                                                                        None, None, None, None, None)
        forecast = lambda: eng._lib.jmid_forecast_scene_constrained(eng._h, E, A, K, T, 2, 0, None, 5, ptr(ids), DT, 0, ptr(bw), *args, ptr(fc), ptr(lw),
                                                                    None, None, None, None)
        assert scene(ptr(ids)) == _lib.EINVAL and forecast() == _lib.EINVAL
        hum, rob = CC.crowd(E, A, SCENE["seed"])
        eng.build_scene(hum, rob, DT, force_all_in_cluster=True)                # (no horizon: no cv)
        assert scene(ptr(ids)) == 0 and scene(None) == _lib.EINVAL and forecast() == _lib.EINVAL
        assert eng._lib.jmid_predict_scene_constrained(None, E, A, K, T, 2, 0, None, 5, ptr(ids), DT, 0, ptr(bw), *args, ptr(sel), ptr(slw), None, None,
                                                       None, None, None) == _lib.EINVAL
        # a DDPM table
        eng.set_step(CC.STEP, "ddpm")
        assert raw_predict(eng, inp, 2)["rc"] == _lib.EINVAL
        eng.set_step(CC.STEP, "ddim")
        # nothing of a refused call stays: the good call again, bit for bit
        again = raw_predict(eng, inp, 2)
        assert again["rc"] == 0 and all(same_bits(again[key], good[key]) for key in good if key != "rc")
        # and the Python surface turns a refusal of the library into JmidError
        with pytest.raises(JmidError):
            eng.predict(*inp, 2, dt=DT, constraints=ChainConstraints(THR, None, {"tau": 0.0}))
    finally:
        eng.close()
