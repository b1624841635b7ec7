"""Per-track history windows from raw stamped frames, host twin (scene.frame_table_tracks): pinned to the existing frame table
(scene.frame_table_frames) and to pad_short_window's layout by exact invariants - bytes, not tolerances.  No GPU."""
import numpy as np
import pytest

from safe_interactive_crowdnav_amd import scene as SC

F, DT = 6, 0.25
STEPS = np.array([0.0, 0.05, 0.12, 0.25, 0.26, 0.6, 1.3])     # duplicate stamps, jitter, empty bins, a stale frame
TRIALS = 300


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def episode(rng, R=None, N=None):
    """Raw frames without a human NaN: (stamps [R], human_xy [R, N, 2], robot_xy [R, 2]); some in a permuted push order, some with a
    NaN robot frame or a NaN stamp (dropped frames)."""
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


def tracks_or_none(stamps, hum, rob):
    try:
        return SC.frame_table_tracks(stamps, hum, rob, DT, F)
    except SC.HistoryTooShortError:
        return None


def test_without_human_nan_is_the_frame_table_right_aligned():
    rng = np.random.default_rng(2901)
    built = short = 0
    for _ in range(TRIALS):
        stamps, hum, rob = episode(rng)
        try:
            h0, r0, p0 = SC.frame_table_frames(stamps, hum, rob, DT, F)
        except SC.HistoryTooShortError:          # no kept frame at all
            with pytest.raises(SC.HistoryTooShortError):
                SC.frame_table_tracks(stamps, hum, rob, DT, F)
            continue
        if len(h0) < 2:                          # item 7: one grid frame is too short, as today
            with pytest.raises(SC.HistoryTooShortError) as ei:
                SC.frame_table_tracks(stamps, hum, rob, DT, F)
            assert ei.value.n_grid == len(h0)
            short += 1
            continue
        h, r, p, ff, n_grid = SC.frame_table_tracks(stamps, hum, rob, DT, F)
        assert n_grid == len(h0) and h.shape == (F,) + hum.shape[1:] and r.shape == (F, 2)
        assert same(h[F - n_grid:], h0) and same(r[F - n_grid:], r0) and same(p, p0)
        assert np.isnan(h[:F - n_grid]).all() and np.isnan(r[:F - n_grid]).all()
        assert ff.dtype == np.int32 and (ff == F - n_grid).all()
        # ... which is pad_short_window's layout and first_frame
        hp, rp, fp = SC.pad_short_window(h0, r0, F)
        assert same(h, hp) and same(r, rp) and same(ff, fp)
        built += 1
    assert built > TRIALS // 2 and short > 0


def test_holes_in_one_track_leave_the_others_alone():
    rng = np.random.default_rng(2902)
    checked = late = interpolated = 0
    for _ in range(TRIALS):
        stamps, hum, rob = episode(rng)
        R, N = hum.shape[:2]
        order = kept_sorted(stamps, rob)
        if not len(order):
            continue
        anchor = order[-1]
        j = int(rng.integers(N))
        holes = rng.random(R) < 0.45
        holes[anchor] = False                                      # anchor seen
        holed = hum.copy()
        holed[holes, j, int(rng.integers(2))] = np.nan             # one NaN coordinate is "not seen"
        full, got = tracks_or_none(stamps, hum, rob), tracks_or_none(stamps, holed, rob)
        assert (full is None) == (got is None)
        if got is None:
            continue
        h, r, p, ff, n_grid = got
        # every other column and the robot: the table without holes
        others = np.arange(N) != j
        assert n_grid == full[4] and same(r, full[1]) and same(h[:, others], full[0][:, others])
        assert same(ff[np.r_[True, others]], full[3][np.r_[True, others]])
        assert same(p, holed[-1])
        # column j from its first frame on: the existing table run on only the frames where j is seen
        seen = ~holes
        hs, _, _ = SC.frame_table_frames(stamps[seen], hum[seen], rob[seen], DT, F)
        f = int(ff[1 + j])
        assert f == F - len(hs) and f >= F - n_grid
        assert same(h[f:, j], hs[:, j]) and np.isnan(h[:f, j]).all()
        checked += 1
        late += f > F - n_grid
        interpolated += int(not same(h[f:, j], full[0][f:, j]))
    assert checked > TRIALS // 2 and late > 20 and interpolated > 20


def test_a_late_pedestrian_keeps_everybody_elses_history():
    """The motivating case: a pedestrian unseen on the 3 oldest of 6 frames.  The wrapper's table has 3 rows for everybody."""
    stamps = 10.0 + DT * np.arange(6)
    rng = np.random.default_rng(2903)
    hum, rob = rng.uniform(-3, 3, (6, 3, 2)), rng.uniform(-3, 3, (6, 2))
    hum[:3, 1] = np.nan
    assert len(SC.frame_table_frames(stamps, hum, rob, DT, F)[0]) == 3
    h, r, p, ff, n_grid = SC.frame_table_tracks(stamps, hum, rob, DT, F)
    assert n_grid == 6 and ff.tolist() == [0, 0, 3, 0]
    assert same(h, hum) and same(r, rob) and same(p, hum[-1])


def test_result_feeds_the_scene_builder():
    stamps = 10.0 + DT * np.arange(6)
    rng = np.random.default_rng(2904)
    hum, rob = rng.uniform(-1, 1, (6, 4, 2)), rng.uniform(-1, 1, (6, 2))
    hum[:3, 1] = np.nan                 # late
    hum[:5, 2] = np.nan                 # seen in the anchor frame only: a node, no ego row
    hum[2, 3] = np.nan                  # a hole: interpolated
    h, r, _, ff, n_grid = SC.frame_table_tracks(stamps, hum, rob, DT, F)
    assert n_grid == 6 and ff.tolist() == [0, 0, 3, 5, 0]
    assert same(h[2, 3], (hum[3, 3] - hum[1, 3]) / (3.0 - 1.0) * (2.0 - 1.0) + hum[1, 3])
    b = SC.build_scenes_batched(h[None], r[None], DT, horizon=4, first_frame=ff[None])
    assert b["in_cluster"][0].tolist() == [True, True, False, True]          # everybody within 3 m; the one-frame pedestrian is no ego row
    assert b["first_index"][0].tolist() == [0, 3, 5, 0]
    assert np.isfinite(b["nbr_sum"]).all() and np.isfinite(b["x_st"][0, 0]).all() and np.isfinite(b["x_st"][0, 3]).all()
    assert np.isnan(b["x_st"][0, 1, :3]).all() and np.isfinite(b["x_st"][0, 1, 3:]).all()
    assert same(b["cv"][0, 2], np.repeat(hum[5, 2][None], 4, axis=0))         # its constant-velocity row: the position repeated
    sb = SC.build_scene(h, r, DT, 4, F, first_frame=ff)
    assert sb.ids_in.tolist() == [0, 1, 3] and sb.ids_out.tolist() == [2]


def test_refusals_and_the_batched_form():
    rng = np.random.default_rng(2905)
    E, R, N = 40, 9, 3
    st, hu, ro = np.empty((E, R)), np.empty((E, R, N, 2)), np.empty((E, R, 2))
    n_frames = rng.integers(1, R + 1, E)
    for e in range(E):
        st[e], hu[e], ro[e] = episode(rng, R, N)
        hu[e][rng.random((R, N)) < 0.25] = np.nan
    out = SC.frame_table_tracks_batched(st, hu, ro, n_frames, DT, F)
    assert out["first_frame"].dtype == np.int32 and out["n_grid"].dtype == np.int32
    absent = too_short = built = 0
    for e in range(E):
        n = int(n_frames[e])
        args = (st[e, :n], hu[e, :n], ro[e, :n], DT, F)
        order = kept_sorted(st[e, :n], ro[e, :n])
        assert same(out["pose_now"][e], hu[e, n - 1])
        if out["n_grid"][e] < 2:                               # item 7
            with pytest.raises(SC.HistoryTooShortError) as ei:
                SC.frame_table_tracks(*args)
            assert ei.value.n_grid == out["n_grid"][e] and (len(order) == 0) == (out["n_grid"][e] == 0)
            too_short += 1
            continue
        h, r, p, ff, n_grid = SC.frame_table_tracks(*args)
        assert n_grid == out["n_grid"][e]
        assert same(h, out["human_xy"][e]) and same(r, out["robot_xy"][e]) and same(p, out["pose_now"][e]) and same(ff, out["first_frame"][e])
        # item 6: absent now <=> not seen in the anchor frame; its first_frame is -1 and its column NaN
        gone = np.isnan(hu[e, order[-1]]).any(axis=1)
        assert ((ff[1:] == -1) == gone).all() and np.isnan(h[:, gone]).all() and np.isfinite(h[F - 1][~gone]).all()
        assert ff[0] == F - n_grid and (ff[1:][~gone] >= ff[0]).all() and (ff[1:][~gone] <= F - 1).all()
        absent += int(gone.any())
        built += 1
    assert absent > 3 and too_short > 3 and built > 10
    with pytest.raises(ValueError):
        SC.frame_table_tracks_batched(st, hu, ro, np.zeros(E, dtype=int), DT, F)
    err = SC.TrackAbsentError(2, 1)
    assert isinstance(err, ValueError) and (err.episode, err.track) == (2, 1)


def test_histories_with_a_missing_pedestrian_are_frames():
    """The forecaster's lists with NaN positions and a duplicated stamp are frames for the per-track table, and not for the joined one."""
    stamps = [1.0, 1.25, 1.25, 1.5]
    prev = [[[0.1 * r, 0.2, t] for r, t in enumerate(stamps)], [[np.nan if r < 2 else 1.0, 0.0, t] for r, t in enumerate(stamps)]]
    rob = [[0.0, 0.0, 0.5]] + [[1.0, 1.0, t] for t in stamps]
    assert SC.histories_as_frames(prev, rob) is None
    st, hum, rb = SC.histories_as_frames(prev, rob, joined=False)
    assert st.tolist() == stamps and hum.shape == (4, 2, 2) and rb.shape == (4, 2) and np.isnan(hum[:2, 1, 0]).all()
