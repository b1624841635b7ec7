"""``guidance=`` on the drop-in class, ``predict_batch`` and ``offline.generate``: the outputs equal the engine-level guided call fed the
same scene, the repair of ``constraint_type="opt_softplus"`` runs on the guided set, both RNG contracts work, and nothing changes unless
the keyword is given."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from safe_interactive_crowdnav_amd import offline
from safe_interactive_crowdnav_amd import scene as SC
from safe_interactive_crowdnav_amd.forecaster import guidance_arguments, predict_batch, rank_samples, repair_totals
from tests.test_gpu_noise import GOLDEN, engine_for, make_forecaster, same_bits
from tests.test_scene_device_inputs import DT, random_positions

THR = 1.0      # metres: wide enough that the guidance fires on every fixture here (asserted below)
GUIDE = {"scale": 0.02, "n_inner": 4}


def by_hand(f, x_T=None, repair=False):
    """One ``predict_ret_best()`` with ``guidance=GUIDE`` from the engine's entries: encode -> guided denoise (-> repair) -> rank."""
    F, H, K, k = f.num_hist_frames, f.predict_horizon, f.num_samples, f.num_ret_samples
    hum_xy, rob_xy, pose_now = SC.frame_table(*f._snapshot(), f.time_step, F)
    sb = SC.build_scene(hum_xy, rob_xy, f.time_step, H, F)
    A = len(sb.ids_in)
    ctx = f.engine.encode(sb.x_st, sb.nbr_sum, sb.edge_mask)
    g = guidance_arguments(GUIDE, THR, step=f.step_size)
    seeded = {} if x_T is not None else dict(seed=f.noise_seed, episode_ids=[f.episode_id], K=K, T=H)
    _, pos, guide = f.engine.denoise(x_T, ctx[None], sb.p0[None], dt=f.time_step, precision="f32", guidance=g, want_guide=True, **seeded)
    episode = None
    if repair:
        pos, _, _, episode = f.engine.repair_collisions(pos, THR)
    rows, logw = rank_samples(f.engine, "device" if k < K else "none", pos, k, (1, A, K, H))
    inc = np.zeros(f.num_hums, dtype=bool)
    inc[sb.ids_in] = True
    return SC.assemble_forecasts(inc, rows[0], None if logw is None else logw[0], sb.cv_forecasts, pose_now, k, K), guide, episode, A


def test_forecaster_with_guidance(tmp_path):
    z = np.load(os.path.join(GOLDEN, "wrapper_jmid_topk.npz"))
    # the reference's torch RNG contract
    plain = make_forecaster(z, tmp_path / "plain", rng_compat="cpu", precision="f32", collision_threshold=THR)
    torch.manual_seed(5)
    base = plain.predict_ret_best()
    probe = make_forecaster(z, tmp_path / "probe", rng_compat="cpu", precision="f32")
    F, H = probe.num_hist_frames, probe.predict_horizon
    A = len(SC.build_scene(*SC.frame_table(*probe._snapshot(), probe.time_step, F)[:2], probe.time_step, H, F).ids_in)
    torch.manual_seed(5)
    x_T = probe._draw_x_T(A)
    (want_fc, want_lw), want_guide, _, _ = by_hand(probe, x_T)
    f = make_forecaster(z, tmp_path / "a", rng_compat="cpu", precision="f32", guidance=GUIDE, collision_threshold=THR)
    assert f.guide is None and f.constraints.guidance is not None
    torch.manual_seed(5)
    fc, lw = f.predict_ret_best()
    print(f"torch contract: {int(f.guide[:, 0].astype(bool).sum())} of {f.guide.shape[0]} samples guided, {int(f.guide[:, 1].sum())} iterations")
    assert same_bits(fc, want_fc) and same_bits(lw, want_lw) and np.array_equal(f.guide, want_guide[0]) and f.guide[:, 0].sum() >= 1
    assert not same_bits(fc, base[0])
    # the device contract, and with constraint_type the repair runs on the guided set
    kw = dict(rng_compat="device", seed=17, precision="f32", collision_threshold=THR, guidance=GUIDE)
    d = make_forecaster(z, tmp_path / "d", **kw)
    fc, lw = d.predict_ret_best()
    (want_fc, want_lw), want_guide, _, _ = by_hand(d)
    assert same_bits(fc, want_fc) and same_bits(lw, want_lw) and np.array_equal(d.guide, want_guide[0])
    both = make_forecaster(z, tmp_path / "b", constraint_type="opt_softplus", **kw)
    fc, lw = both.predict_ret_best()
    (want_fc, want_lw), want_guide, episode, _ = by_hand(both, repair=True)
    print(f"guidance + repair: guided {int(both.guide[:, 0].sum())}, repair {both.repair}")
    assert same_bits(fc, want_fc) and same_bits(lw, want_lw) and both.repair == repair_totals(episode) and np.array_equal(both.guide, want_guide[0])
    alone = make_forecaster(z, tmp_path / "r", constraint_type="opt_softplus", **{a: b for a, b in kw.items() if a != "guidance"})
    alone.predict_ret_best()
    print(f"repair alone: {alone.repair}")
    # the first-call self check of an opt-in mode carries the same guidance in both runs
    mx = make_forecaster(z, tmp_path / "mx", **{**kw, "precision": "f16mx"}, self_check=True)
    mx.predict_ret_best()
    assert mx.guide is not None and np.isfinite(mx.self_check_delta)
    # refusals: a rerun would have to be guided too; the one-entry chains; walls without obstacles
    for bad in (dict(collision_free_rounds=2), dict(device_scene=True), dict(device_frames=True), dict(guidance={"walls": True})):
        with pytest.raises(ValueError):
            make_forecaster(z, tmp_path / "bad", **{**kw, **bad})


def test_predict_batch_with_guidance():
    E, N, K, k, H = 6, 6, 16, 5, 8
    hum, rob = random_positions(E, N, 67, half_width=5.0)
    eng = engine_for()
    eng.set_step(2, "ddim")
    gids = [1000 + 7 * e for e in range(E)]
    kw = dict(num_samples=K, num_ret_samples=k, horizon=H, time_step=DT, precision="f32", collision_threshold=THR)
    plain = predict_batch(eng, hum, rob, gids, noise="device", seed=2024, **kw)
    for extra in (dict(noise="device", seed=2024), dict(), dict(noise="device", seed=2024, constraint_type="opt_softplus")):
        stats = {}
        fc, lw, inc = predict_batch(eng, hum, rob, gids, stats=stats, guidance=GUIDE, **kw, **extra)
        print(f"{extra}: counts {inc.sum(axis=1).tolist()}, guided samples {stats['guide'][..., 0].sum(axis=1).tolist()}")
        assert stats["guide"].shape == (E, K, 2) and stats["guide"][..., 0].sum() >= 1
        for e in (0, E - 1):      # an episode's rows do not depend on its batch mates
            one = {}
            fc1, lw1, _ = predict_batch(eng, hum[e:e + 1], rob[e:e + 1], gids[e:e + 1], stats=one, guidance=GUIDE, **kw, **extra)
            assert same_bits(fc1[0], fc[e]) and same_bits(lw1[0], lw[e]) and same_bits(one["guide"][0], stats["guide"][e])
        if extra == dict(noise="device", seed=2024):
            assert not same_bits(fc, plain[0])
            # the engine-level guided call of one count group
            counts = inc.sum(axis=1)
            eps = np.nonzero(counts == counts.max())[0]
            b = SC.build_scenes_batched(hum, rob, DT, horizon=H)
            rows = np.stack([np.nonzero(inc[e])[0] for e in eps])
            A, n = int(counts.max()), len(eps) * int(counts.max())
            ctx = eng.encode(b["x_st"][eps[:, None], rows].reshape(n, 6, 6), b["nbr_sum"][eps[:, None], rows].reshape(n, 2, 6, 6),
                             b["edge_mask"][eps[:, None], rows].reshape(n, 2)).reshape(len(eps), A, -1)
            p0 = np.ascontiguousarray(b["p0"][eps[:, None], rows])
            _, pos, guide = eng.denoise(None, ctx, p0, dt=DT, precision="f32", seed=2024, episode_ids=np.asarray(gids)[eps], K=K, T=H,
                                        guidance=guidance_arguments(GUIDE, THR, step=2), want_guide=True)
            sel, logw = rank_samples(eng, "device", pos, k, (len(eps), A, K, H))
            want = SC.assemble_forecasts(inc[eps], sel, logw, b["cv"][eps], hum[eps, -1], k, K)
            assert same_bits(fc[eps], want[0]) and same_bits(lw[eps], want[1]) and same_bits(stats["guide"][eps], guide)
    # off unless asked for
    off = predict_batch(eng, hum, rob, gids, noise="device", seed=2024, **kw)
    assert same_bits(off[0], plain[0]) and same_bits(off[1], plain[1])
    for bad in (dict(collision_free_rounds=1, noise="device"), dict(padded=True), dict(padded="resident"), dict(device_frames=True),
                dict(device_scene=True)):
        with pytest.raises(ValueError):
            predict_batch(eng, hum, rob, gids, guidance=GUIDE, **kw, **bad)
    try:
        eng.set_step(2, "ddpm")
        with pytest.raises(ValueError):
            predict_batch(eng, hum, rob, gids, guidance=GUIDE, **kw)
    finally:
        eng.set_step(2, "ddim")


def test_offline_generate_with_guidance():
    eng = engine_for()
    B, T, n = 3, 4, 6
    g = torch.Generator().manual_seed(3)
    ctx, p0 = torch.randn([B, 32], generator=g).numpy(), (0.05 * torch.randn([B, 2], generator=g)).numpy()
    try:
        kw = dict(sampling="ddim", step=2, precision="f32", seed=9)
        plain = offline.generate(eng, ctx, p0, DT, T, n, True, **kw)
        pos, steps, a, b, c = offline.generate(eng, ctx, p0, DT, T, n, True, with_constraints=True, collision_threshold=THR, guidance=GUIDE, **kw)
        print(f"offline: {b} of {n} samples guided, at most {a} iterations")
        assert b >= 1 and a >= 1 and c == 0 and steps == plain[1] and not same_bits(pos, plain[0])
        _, want, _ = eng.denoise(None, np.broadcast_to(ctx[None], (n, B, 32)).copy(), np.broadcast_to(p0[None], (n, B, 2)).copy(), dt=DT,
                                 precision="f32", seed=9, episode_ids=np.arange(n, dtype=np.uint32), K=1, T=T,
                                 guidance=guidance_arguments(GUIDE, THR, step=2), want_guide=True)
        assert same_bits(pos, want.reshape(n, B, T, 2))
        for bad in (dict(with_constraints=False), dict(with_constraints=True, sampling="ddpm")):
            with pytest.raises(ValueError):
                offline.generate(eng, ctx, p0, DT, T, n, True, collision_threshold=THR, guidance=GUIDE, **{**kw, **bad})
    finally:
        eng.set_step(2, "ddim")
