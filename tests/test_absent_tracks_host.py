"""Pedestrians who are not seen now, host twins: left out of the scene (scene.build_scenes_batched(allow_absent=True)) or coasted to the
anchor frame (scene.frame_table_tracks(max_coast=)).  Pinned to today's functions by exact invariants - bytes, not tolerances: the new
arithmetic is selections plus one fp64 multiply-add.  No GPU."""
import os

import numpy as np
import pytest

from safe_interactive_crowdnav_amd import scene as SC

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

F, DT, W = 6, 0.25, 25
STEPS = np.array([0.0, 0.05, 0.12, 0.25, 0.26, 0.6, 1.3])     # duplicate stamps, jitter, empty bins, a stale frame
TRIALS = 300
KEYS = ("x", "x_st", "nbr_sum", "edge_mask", "p0", "cv")


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def episode(rng, R=None, N=None):
    """Raw frames without a human NaN, as tests/test_track_windows_host.py makes them: some in a permuted push order, some with a NaN
    robot frame or a NaN stamp (dropped frames)."""
    R = int(rng.integers(1, 12)) if R is None else R
    N = int(rng.integers(1, 5)) if N is None else N
    stamps = 3.0 + np.cumsum(rng.choice(STEPS, R))
    hum = rng.uniform(-4.0, 4.0, (R, N, 2))
    rob = rng.uniform(-4.0, 4.0, (R, 2))
    if rng.random() < 0.3:
        p = rng.permutation(R)
        stamps, hum, rob = stamps[p], hum[p], rob[p]
    if rng.random() < 0.3:
        rob[rng.integers(R), rng.integers(2)] = np.nan
    if rng.random() < 0.1:
        stamps[rng.integers(R)] = np.nan
    return stamps, hum, rob


def kept_sorted(stamps, rob):
    """Indices of the kept frames in stable sort order by stamp: the last one is the anchor."""
    kept = np.nonzero(~(np.isnan(stamps) | np.isnan(rob).any(axis=1)))[0]
    return kept[np.argsort(stamps[kept], kind="stable")]


def holed(rng, stamps, hum, rob, p=0.4):
    out = hum.copy()
    miss = rng.random(hum.shape[:2]) < p
    out[miss, int(rng.integers(2))] = np.nan
    return out


# ------------------------------------------------------------------------------------------------ the track table
def test_max_coast_none_and_nobody_absent_are_todays_bytes():
    rng = np.random.default_rng(3101)
    with_holes = 0
    for _ in range(TRIALS):
        stamps, hum, rob = episode(rng)
        hum = holed(rng, stamps, hum, rob)
        today = SC._track_table(stamps, hum, rob, DT, F)
        again = SC._track_table(stamps, hum, rob, DT, F, None)
        assert len(again) == 5 and all(same(a, b) for a, b in zip(today[:4], again[:4])) and today[4] == again[4]
        # nobody absent: the anchor frame sees everybody
        order = kept_sorted(stamps, rob)
        if len(order):
            hum[order[-1]] = rng.uniform(-4.0, 4.0, hum.shape[1:])
        today = SC._track_table(stamps, hum, rob, DT, F)
        for c in (0, 2, F - 2):
            got = SC._track_table(stamps, hum, rob, DT, F, c)
            assert len(got) == 6 and all(same(a, b) for a, b in zip(today[:4], got[:4]) if len(order) or a is not today[2]) and today[4] == got[4]
            assert got[5].dtype == np.int32 and (got[5] == (0 if len(order) else -1)).all()
            assert len(order) or np.isnan(got[2]).all()              # no kept frame: nobody is seen in an anchor frame
        with_holes += int(np.isnan(hum).any())
    assert with_holes > TRIALS // 2


def test_a_coasted_column_is_todays_table_fed_the_coasted_values():
    rng = np.random.default_rng(3102)
    coasted = left_out = still = stepped = 0
    for _ in range(TRIALS):
        stamps, hum, rob = episode(rng)
        R, N = hum.shape[:2]
        hum = holed(rng, stamps, hum, rob, 0.5)
        order = kept_sorted(stamps, rob)
        c = int(rng.integers(0, F - 1))
        today = SC._track_table(stamps, hum, rob, DT, F)
        h, r, p, ff, n_grid, coast = SC._track_table(stamps, hum, rob, DT, F, c)
        assert n_grid == today[4] and same(r, today[1]) and ff[0] == today[3][0]
        if not len(order):
            assert (coast == -1).all() and np.isnan(p).all() and np.isnan(h).all()
            continue
        anchor = order[-1]
        ns = np.trunc(stamps * 100.0)
        bins = (ns[anchor] - ns[order]).astype(np.int64) // W
        for j in range(N):
            if today[3][1 + j] >= 0:                   # seen in the anchor frame: everything as today
                assert coast[j] == 0 and same(h[:, j], today[0][:, j]) and ff[1 + j] == today[3][1 + j] and same(p[j], today[2][j])
                continue
            seen = ~np.isnan(hum[order, j]).any(axis=1)
            b_new = int(bins[seen].min()) if seen.any() else None
            if b_new is None or b_new > c or b_new > n_grid - 1:
                assert coast[j] == -1 and ff[1 + j] == -1 and np.isnan(h[:, j]).all() and np.isnan(p[j]).all()
                left_out += 1
                continue
            assert coast[j] == b_new and same(p[j], h[F - 1, j]) and np.isfinite(h[ff[1 + j]:, j]).all() and np.isnan(h[:ff[1 + j], j]).all()
            # today's table on the same raw frames + his coasted values as observations: in the anchor frame, and in one synthetic frame
            # per bin 1 .. b_new-1 (the oldest stamp of its bin, nobody else seen in it)
            fed_h, fed_r, fed_s = hum.copy(), rob, stamps
            fed_h[anchor, j] = h[F - 1, j]
            for b in range(1, b_new):
                row = np.full((1, N, 2), np.nan)
                row[0, j] = h[F - 1 - b, j]
                fed_h = np.concatenate([row, fed_h])
                fed_r = np.concatenate([[[0.5, -0.5]], fed_r])
                fed_s = np.concatenate([[(ns[anchor] - b * W - (W - 1) + 0.25) / 100.0], fed_s])
            want = SC._track_table(fed_s, fed_h, fed_r, DT, F)
            assert want[4] == n_grid and same(want[0][:, j], h[:, j]) and want[3][1 + j] == ff[1 + j]
            # the definition, read off the column
            y_new = h[F - 1 - b_new, j]
            step = y_new - h[F - 2 - b_new, j] if F - 2 - b_new >= ff[1 + j] else np.zeros(2)
            for b in range(b_new):
                assert same(h[F - 1 - b, j], y_new + float(b_new - b) * step)
            coasted += 1
            still += int(b_new > 0 and not step.any())
            stepped += int(b_new > 0 and step.any())
        # every column of a pedestrian seen in the anchor frame was compared above; the robot's too
    assert coasted > 40 and left_out > 40 and still > 3 and stepped > 10


def test_frame_table_tracks_and_the_batched_form_with_max_coast():
    rng = np.random.default_rng(3103)
    E, R, N = 40, 9, 3
    st, hu, ro = np.empty((E, R)), np.empty((E, R, N, 2)), np.empty((E, R, 2))
    n_frames = rng.integers(1, R + 1, E)
    for e in range(E):
        st[e], hu[e], ro[e] = episode(rng, R, N)
        hu[e][rng.random((R, N)) < 0.3] = np.nan
    today = SC.frame_table_tracks_batched(st, hu, ro, n_frames, DT, F)
    assert "coast" not in today
    out = SC.frame_table_tracks_batched(st, hu, ro, n_frames, DT, F, max_coast=2)
    assert out["coast"].dtype == np.int32 and out["coast"].shape == (E, N) and same(out["n_grid"], today["n_grid"]) and same(out["robot_xy"], today["robot_xy"])
    assert ((out["coast"] == -1) == (out["first_frame"][:, 1:] == -1)).all() and (out["coast"] <= 2).all()
    assert ((today["first_frame"][:, 1:] >= 0) <= (out["coast"] == 0)).all()
    assert ((today["first_frame"][:, 1:] == -1) & (out["coast"] >= 0)).sum() > 3 and (out["coast"] > 0).any()      # coasted ones among them
    for e in range(E):
        n = int(n_frames[e])
        args = (st[e, :n], hu[e, :n], ro[e, :n], DT, F)
        if out["n_grid"][e] < 2:
            with pytest.raises(SC.HistoryTooShortError):
                SC.frame_table_tracks(*args, max_coast=2)
            continue
        got = SC.frame_table_tracks(*args, max_coast=2)
        assert len(got) == 6 and len(SC.frame_table_tracks(*args)) == 5
        for key, v in zip(("human_xy", "robot_xy", "pose_now", "first_frame", "n_grid", "coast"), got):
            assert same(np.asarray(v, dtype=out[key].dtype), out[key][e]), key
    for bad in (-1, F - 1, 1.5):
        with pytest.raises(ValueError):
            SC.frame_table_tracks_batched(st, hu, ro, n_frames, DT, F, max_coast=bad)


def test_one_observation_stands_still_and_two_give_the_step():
    stamps = 10.0 + DT * np.arange(6)
    rng = np.random.default_rng(3104)
    hum, rob = rng.uniform(-3, 3, (6, 3, 2)), rng.uniform(-3, 3, (6, 2))
    hum[:4, 0] = np.nan
    hum[5, 0] = np.nan                  # seen once, at bin 1
    hum[4:, 1] = np.nan
    hum[2, 1] = np.nan                  # b_new = 2, a hole right behind it: the step comes from the interpolated row
    h, r, p, ff, n_grid, coast = SC.frame_table_tracks(stamps, hum, rob, DT, F, max_coast=2)
    assert coast.tolist() == [1, 2, 0] and ff.tolist() == [0, 4, 0, 0]
    assert same(h[4:, 0], np.stack([hum[4, 0], hum[4, 0] + 1.0 * np.zeros(2)])) and same(p[0], h[5, 0])
    mid = (hum[3, 1] - hum[1, 1]) / (3.0 - 1.0) * (2.0 - 1.0) + hum[1, 1]
    step = hum[3, 1] - mid
    assert same(h[2, 1], mid) and same(h[4, 1], hum[3, 1] + 1.0 * step) and same(h[5, 1], hum[3, 1] + 2.0 * step) and same(p[1], h[5, 1])
    assert same(h[:, 2], hum[:, 2]) and same(p[2], hum[5, 2])
    left = SC.frame_table_tracks(stamps, hum, rob, DT, F, max_coast=1)
    assert left[5].tolist() == [1, -1, 0] and left[3].tolist() == [0, 4, -1, 0] and np.isnan(left[0][:, 1]).all() and np.isnan(left[2][1]).all()
    assert same(left[0][:, [0, 2]], h[:, [0, 2]])


# ------------------------------------------------------------------------------------------------ the scene
def scene_episode(rng, N, spread):
    hum = rng.uniform(-spread, spread, (1, 1, N, 2)) + 0.1 * np.cumsum(rng.standard_normal((1, F, N, 2)), axis=1)
    rob = rng.uniform(-spread, spread, (1, 1, 2)) + 0.1 * np.cumsum(rng.standard_normal((1, F, 2)), axis=1)
    ff = np.zeros((1, N + 1), dtype=np.int32)
    ff[0, 1:] = rng.choice([0, 0, 0, 2, F - 2, F - 1], N)
    ff[0, 0] = rng.choice([0, 0, 1])
    ff = np.maximum(ff, ff[:, :1])
    return hum, rob, ff


def test_left_out_is_the_episode_with_the_column_removed():
    rng = np.random.default_rng(3105)
    chosen_left = member_left = outside_left = forced = 0
    for trial in range(TRIALS):
        N = int(rng.integers(2, 6))
        hum, rob, ff = scene_episode(rng, N, rng.choice([1.0, 3.0, 5.0]))
        force = trial % 10 == 0
        full = SC.build_scenes_batched(hum, rob, DT, force_all_in_cluster=force, horizon=4, first_frame=ff)
        again = SC.build_scenes_batched(hum, rob, DT, force_all_in_cluster=force, horizon=4, first_frame=ff, allow_absent=True)
        assert set(full) == set(again) and all(same(full[key], again[key]) for key in full)        # no -1: the bits of allow_absent=False
        out = rng.random(N) < 0.4
        if out.all():
            out[rng.integers(N)] = False
        if not out.any():
            out[rng.integers(N)] = True
        # whose cluster today's build chooses, and who is in it
        last = np.concatenate([rob[0, -1:], hum[0, -1]])
        near = np.sqrt(np.square(last[:, None] - last[None]).sum(-1)) < 3.0
        means = (near @ last) / near.sum(1, keepdims=True)
        chosen = int(np.argmin(np.linalg.norm(means - last[0], axis=1)[1:]))
        chosen_left += int(out[chosen])
        member_left += int((near[1 + chosen, 1:] & out & (np.arange(N) != chosen)).any() and not out[chosen])
        outside_left += int((~near[1 + chosen, 1:] & out).any())
        forced += int(force)
        ffa = ff.copy()
        ffa[0, 1:][out] = -1
        poison = hum.copy()
        poison[:, :, out] = 1e9 * rng.standard_normal((1, F, int(out.sum()), 2))     # his positions are never read
        got = SC.build_scenes_batched(poison, rob, DT, force_all_in_cluster=force, horizon=4, first_frame=ffa, allow_absent=True)
        want = SC.build_scenes_batched(hum[:, :, ~out], rob, DT, force_all_in_cluster=force, horizon=4, first_frame=ffa[:, np.r_[True, ~out]])
        for key in KEYS + ("in_cluster", "first_index"):
            assert same(got[key][:, ~out], want[key]), key
        assert same(got["robot_in_cluster"], want["robot_in_cluster"])
        for key in KEYS:
            assert np.isnan(got[key][:, out]).all() and got[key].dtype == want[key].dtype, key
        assert not got["in_cluster"][:, out].any() and (got["first_index"][:, out] == -1).all()
        # one scene: in neither list
        sb = SC.build_scene(poison[0], rob[0], DT, 4, F, force_all_in_cluster=force, first_frame=ffa[0], allow_absent=True)
        assert sb.ids_in.tolist() == np.nonzero(got["in_cluster"][0])[0].tolist()
        assert sorted(sb.ids_in.tolist() + sb.ids_out.tolist()) == np.nonzero(~out)[0].tolist() and sorted(sb.cv_forecasts) == sb.ids_out.tolist()
        with pytest.raises(ValueError):
            SC.build_scenes_batched(poison, rob, DT, horizon=4, first_frame=ffa)
        with pytest.raises(ValueError):
            SC.build_scene(poison[0], rob[0], DT, 4, F, first_frame=ffa[0])
    assert chosen_left > 30 and member_left > 30 and outside_left > 30 and forced == TRIALS // 10


def test_left_out_refusals():
    rng = np.random.default_rng(3106)
    hum, rob, ff = scene_episode(rng, 3, 1.0)
    hum, rob, ff = np.repeat(hum, 2, axis=0), np.repeat(rob, 2, axis=0), np.repeat(ff, 2, axis=0)
    ff[1, 1:] = -1
    with pytest.raises(ValueError, match="episode 1"):                       # nobody left
        SC.build_scenes_batched(hum, rob, DT, first_frame=ff, allow_absent=True)
    ff[1, 1] = 0
    SC.build_scenes_batched(hum, rob, DT, first_frame=ff, allow_absent=True)
    for e, j, v in ((0, 0, -1), (1, 2, -2), (0, 3, F)):                        # the robot, below -1, beyond the window
        bad = ff.copy()
        bad[e, j] = v
        with pytest.raises(ValueError):
            SC.build_scenes_batched(hum, rob, DT, first_frame=bad, allow_absent=True)


# ------------------------------------------------------------------------------------------------ the reference's model side
def test_left_out_is_what_the_reference_makes_of_a_node_whose_data_ends_before_now():
    """tests/golden/absent_now_w32_n4.npz (make_golden_absent.py): the reference's own Scene / Node / get_timesteps_data on a scene in which
    pedestrian 1 was last seen two frames ago, 1.2 m from pedestrian 0.  He is in the Scene, and a node of its temporal graph."""
    z = np.load(os.path.join(GOLDEN, "absent_now_w32_n4.npz"))
    dt, Hz, Fz = float(z["time_step"]), int(z["H"]), int(z["past"])
    ff, ids = z["first_frame"], z["node_ids"]
    assert ff.tolist() == [0, 0, -1, 2, 0] and ids.tolist() == [0, 2, 3] and z["last_frame"].tolist() == [5, 5, 3, 5, 5]
    assert np.isfinite(z["human_xy"][1:4, 1]).all() and np.isnan(z["human_xy"][4:, 1]).all()
    b = SC.build_scenes_batched(z["human_xy"][None], z["robot_xy"][None], dt, horizon=Hz, first_frame=ff[None], allow_absent=True)
    assert np.nonzero(b["in_cluster"][0])[0].tolist() == ids.tolist() and bool(b["robot_in_cluster"][0]) == bool(z["robot_in_cluster"])
    assert same(b["first_index"][0, ids], z["first_hist"])
    for r, (i, fi) in enumerate(zip(ids, z["first_hist"])):
        assert same(b["x_st"][0, i, fi:], z["x_st"][r, fi:]) and same(b["x"][0, i, fi:], z["x_t"][r, fi:])
        assert np.isnan(b["x_st"][0, i, :fi]).all() and np.isnan(z["x_st"][r, :fi]).all()
    assert np.isfinite(z["nbr_sum"]).all() and same(b["nbr_sum"][0, ids], z["nbr_sum"]) and same(b["edge_mask"][0, ids], z["edge_mask"])
    assert same(b["p0"][0, ids], z["x_t"][:, -1, 0:2]) and same(b["cv"][0], z["cv"]) and np.isnan(b["cv"][0, 1]).all()
    assert (z["n_nbr"][:, 0] == 2).all()                     # the reference counts two pedestrian neighbours per ego: not him
    sb = SC.build_scene(z["human_xy"], z["robot_xy"], dt, Hz, Fz, first_frame=ff, allow_absent=True)
    assert sb.ids_in.tolist() == ids.tolist() and sb.ids_out.tolist() == [] and same(sb.nbr_sum, z["nbr_sum"]) and same(sb.x_st[0], z["x_st"][0])
