"""Short histories on the host: scene.build_scene / build_scenes_batched with ``first_frame`` against the reference's own batch tensors for
tracks seen for fewer than hist_len frames (tests/golden/shorthist_*.npz, written by tests/golden/make_golden_short_history.py), bit for bit;
``first_frame`` all zero against today's builders; ``pad_short_window``; and the argument check of ``JmidEngine.encode(first_index=)``."""
import glob
import os

import numpy as np
import pytest

from safe_interactive_crowdnav_amd import scene as SC
from safe_interactive_crowdnav_amd.engine import JmidEngine

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
F, DT, H = 6, 0.25, 6


def shorthist_cases():
    """name -> dict of arrays, one per reference scene (the two cases of shorthist_start_n3 split)."""
    out = {}
    for name in ("mixed_w32_n4", "mixed_w256_n4", "oneframe_n4"):
        z = np.load(os.path.join(GOLDEN, f"shorthist_{name}.npz"))
        out[name] = {k: z[k] for k in z.files}
    z = np.load(os.path.join(GOLDEN, "shorthist_start_n3.npz"))
    for L in (2, 3):
        d = {k: z[k] for k in z.files if not k.startswith(("l2_", "l3_"))}
        d.update({k[3:]: z[k] for k in z.files if k.startswith(f"l{L}_")})
        out[f"start_l{L}_n3"] = d
    return out


CASES = shorthist_cases()


def mixed_batch():
    """E = 3, N = 4: a full-history episode next to two short ones (the mixed and the one-frame fixtures) -> human_xy [3, F, 4, 2],
    robot_xy [3, F, 2], first_frame [3, 5].  The batch of tests/test_gpu_short_history.py; held to the cluster margin below."""
    from tests.test_scene_device_inputs import random_positions
    h0, r0 = random_positions(1, 4, 97, half_width=1.2, robot=(0.2, -1.4))
    m, o = CASES["mixed_w32_n4"], CASES["oneframe_n4"]
    hum = np.stack([h0[0], m["human_xy"], o["human_xy"]])
    rob = np.stack([r0[0], m["robot_xy"], o["robot_xy"]])
    ff = np.stack([np.zeros(5, np.int32), m["first_frame"], o["first_frame"]]).astype(np.int32)
    return hum, rob, ff


def test_mixed_batch_holds_the_cluster_margin():
    from tests.test_scene_device_inputs import MARGIN, cluster_margin
    hum, rob, ff = mixed_batch()
    assert cluster_margin(hum, rob).min() > MARGIN         # (the last frame is present for everybody: no NaN enters)
    pos = np.concatenate([rob[:, :, None], hum], axis=2)[:, -3:]
    with np.errstate(invalid="ignore"):
        d = np.sqrt(np.square(pos[:, :, :, None] - pos[:, :, None, :]).sum(-1))
    assert np.nanmin(np.abs(d - SC.ATTENTION_RADIUS)) > MARGIN
    b = SC.build_scenes_batched(hum, rob, DT, horizon=H, first_frame=ff)
    assert list(b["in_cluster"].sum(axis=1)) == [3, 4, 3]
    for e in (1, 2):                                       # per episode the single-scene builder's bits
        one = SC.build_scenes_batched(hum[e:e + 1], rob[e:e + 1], DT, horizon=H, first_frame=ff[e:e + 1])
        for key in ("x", "x_st", "nbr_sum", "edge_mask", "p0", "cv"):
            same_bits(one[key][0], b[key][e])


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def same_bits(a, b):
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    np.testing.assert_array_equal(bits(a), bits(b))


def check_rows_against_reference(z, ids_in, first_index, x, x_st, nbr_sum, edge_mask, p0):
    np.testing.assert_array_equal(ids_in, z["node_ids"])
    np.testing.assert_array_equal(first_index, z["first_hist"])
    assert first_index.dtype == np.int32
    for r, fi in enumerate(z["first_hist"]):
        same_bits(x_st[r, fi:], z["x_st"][r, fi:])
        same_bits(x[r, fi:], z["x_t"][r, fi:])
        assert np.isnan(x_st[r, :fi]).all() and np.isnan(x[r, :fi]).all()
        assert np.isnan(z["x_st"][r, :fi]).all()          # (the reference pads its own history with NaN)
    assert np.isfinite(nbr_sum).all()
    same_bits(nbr_sum, z["nbr_sum"])                      # all F frames, the ones in front of the ego's own first frame included
    same_bits(edge_mask, z["edge_mask"])
    same_bits(p0, z["x_t"][:, -1, 0:2])


@pytest.mark.parametrize("name", sorted(CASES))
def test_host_twin_matches_the_reference_batch(name):
    z = CASES[name]
    sb = SC.build_scene(z["human_xy"], z["robot_xy"], DT, H, F, first_frame=z["first_frame"])
    check_rows_against_reference(z, sb.ids_in, sb.first_index, sb.x, sb.x_st, sb.nbr_sum, sb.edge_mask, sb.p0)
    assert sb.robot_in_cluster == bool(z["robot_in_cluster"])
    N = z["human_xy"].shape[1]
    assert sorted(list(sb.ids_in) + list(sb.ids_out)) == list(range(N))
    for i in sb.ids_out:                                   # (here: the one-frame pedestrian - its position repeated)
        same_bits(sb.cv_forecasts[int(i)], z["cv"][int(i)])
    # the batched builder: every pedestrian has a row, the ego rows are the reference's
    b = SC.build_scenes_batched(z["human_xy"][None], z["robot_xy"][None], DT, horizon=H, first_frame=z["first_frame"][None])
    rows = np.nonzero(b["in_cluster"][0])[0]
    check_rows_against_reference(z, rows, b["first_index"][0, rows], b["x"][0, rows], b["x_st"][0, rows], b["nbr_sum"][0, rows],
                                 b["edge_mask"][0, rows], b["p0"][0, rows])
    same_bits(b["cv"][0], z["cv"])
    np.testing.assert_array_equal(b["first_index"][0], z["first_frame"][1:])


def test_one_frame_pedestrian_is_a_neighbour_but_no_ego_row():
    z = CASES["oneframe_n4"]
    assert list(z["first_frame"]) == [0, 0, 5, 1, 2]
    sb = SC.build_scene(z["human_xy"], z["robot_xy"], DT, H, F, first_frame=z["first_frame"])
    assert list(sb.ids_in) == [0, 2, 3] and list(sb.ids_out) == [1]
    assert (z["n_nbr"][:, 0] == 3).all()                   # ... and the reference counts it among every ego's pedestrian neighbours
    np.testing.assert_array_equal(sb.cv_forecasts[1], np.repeat(z["human_xy"][-1, 1][None], H, axis=0))
    # without it the neighbour sums differ: it does contribute
    keep = [0, 2, 3]
    sb3 = SC.build_scene(z["human_xy"][:, keep], z["robot_xy"], DT, H, F, first_frame=z["first_frame"][[0, 1, 3, 4]])
    assert not np.array_equal(sb3.nbr_sum[:, 0], sb.nbr_sum[:, 0])


def test_mixed_fixture_has_a_pair_connected_on_the_last_frame_only():
    z = CASES["mixed_w32_n4"]
    d = np.sqrt(np.square(z["human_xy"][3:, 1] - z["human_xy"][3:, 3]).sum(-1))
    assert (d[:2] > SC.ATTENTION_RADIUS).all() and d[2] <= SC.ATTENTION_RADIUS


def wrapper_inputs():
    from tests.test_scene_golden import CASES as WRAPPER, replay_histories
    for case in WRAPPER:
        z = np.load(os.path.join(GOLDEN, case))
        prev, rob = replay_histories(z)
        hum_xy, rob_xy, _ = SC.frame_table(prev, rob, float(z["time_step"]), int(z["past"]))
        yield case, z, hum_xy, rob_xy


def test_all_zero_first_frame_is_todays_builder_bit_for_bit():
    n = 0
    for case, z, hum, rob in wrapper_inputs():
        dt, Hc, past = float(z["time_step"]), int(z["H"]), int(z["past"])
        N = hum.shape[1]
        zero = np.zeros(N + 1, dtype=np.int32)
        a = SC.build_scene(hum, rob, dt, Hc, past)
        for b in (SC.build_scene(hum, rob, dt, Hc, past, first_frame=None), SC.build_scene(hum, rob, dt, Hc, past, first_frame=zero)):
            np.testing.assert_array_equal(a.ids_in, b.ids_in)
            np.testing.assert_array_equal(a.ids_out, b.ids_out)
            for key in ("x", "x_st", "nbr_sum", "edge_mask", "p0"):
                same_bits(getattr(a, key), getattr(b, key))
            assert a.robot_in_cluster == b.robot_in_cluster and sorted(a.cv_forecasts) == sorted(b.cv_forecasts)
            for i in a.cv_forecasts:
                same_bits(a.cv_forecasts[i], b.cv_forecasts[i])
            assert (b.first_index == 0).all() and len(b.first_index) == len(b.ids_in)
        ba = SC.build_scenes_batched(hum[None], rob[None], dt, horizon=Hc)
        bz = SC.build_scenes_batched(hum[None], rob[None], dt, horizon=Hc, first_frame=zero[None])
        assert sorted(ba) == sorted(bz)
        for key in ba:
            if ba[key].dtype.kind == "f":
                same_bits(ba[key], bz[key])
            else:
                np.testing.assert_array_equal(ba[key], bz[key])
        n += 1
    assert n >= 5


@pytest.mark.parametrize("L", [2, 3])
def test_pad_short_window_reproduces_the_episode_start_fixture(L):
    z = CASES[f"start_l{L}_n3"]
    hum, rob, ff = SC.pad_short_window(z["human_raw"], z["robot_raw"], F)
    assert hum.shape == (F, 3, 2) and rob.shape == (F, 2) and ff.dtype == np.int32 and list(ff) == [F - L] * 4
    assert np.isnan(hum[:F - L]).all() and np.isnan(rob[:F - L]).all()
    same_bits(hum[F - L:], z["human_raw"])
    np.testing.assert_array_equal(ff, z["first_frame"])
    sb = SC.build_scene(hum, rob, DT, H, F, first_frame=ff)
    check_rows_against_reference(z, sb.ids_in, sb.first_index, sb.x, sb.x_st, sb.nbr_sum, sb.edge_mask, sb.p0)
    # whatever stands in front of first_frame is never read
    junk = SC.build_scene(np.where(np.isnan(hum), 1e30, hum), np.where(np.isnan(rob), -7.0, rob), DT, H, F, first_frame=ff)
    same_bits(junk.nbr_sum, sb.nbr_sum)
    same_bits(junk.x_st[:, F - L:], sb.x_st[:, F - L:])
    # a full window passes through
    full_h, full_r, ff0 = SC.pad_short_window(np.zeros((8, 3, 2)), np.zeros((8, 2)), F)
    assert full_h.shape == (F, 3, 2) and full_r.shape == (F, 2) and (ff0 == 0).all()


def test_first_frame_refusals():
    z = CASES["mixed_w32_n4"]
    hum, rob = z["human_xy"], z["robot_xy"]
    for bad in ([0, 0, 2, 4, 6], [0, -1, 2, 4, 3], [5, 0, 2, 4, 3], [0, 0, 2, 4]):
        with pytest.raises(ValueError):
            SC.build_scene(hum, rob, DT, H, F, first_frame=np.asarray(bad))
    # a one-frame robot is a neighbour like any other when everybody is forced into the cluster
    sb = SC.build_scene(hum, rob, DT, H, F, force_all_in_cluster=True, first_frame=np.asarray([5, 0, 2, 4, 3]))
    assert list(sb.ids_in) == [0, 1, 2, 3] and np.isfinite(sb.nbr_sum).all()


def test_encode_refuses_a_first_index_outside_its_range_before_any_device_call():
    """engine.encode's argument check needs no device: the handle is never touched (an engine without one, as on a CPU-only box)."""
    eng = JmidEngine.__new__(JmidEngine)
    eng.hist_len, eng._h = F, None
    x_st, nbr, em = np.zeros((3, F, 6), np.float32), np.zeros((3, 2, F, 6), np.float32), np.zeros((3, 2), np.float32)
    for bad in ([0, F - 1, 0], [0, -1, 2], [0, 1], [0.0, 1.0, 2.0]):
        with pytest.raises(ValueError):
            eng.encode(x_st, nbr, em, first_index=np.asarray(bad))
    assert eng._first_index(np.array([0, F - 2, 3]), 3).dtype == np.int32
