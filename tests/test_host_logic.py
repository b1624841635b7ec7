"""Host-side logic that needs no GPU: KDE top-k, weight container round trip, DDIM step table."""
import glob
import os

import numpy as np
import pytest
import torch

from safe_interactive_crowdnav_amd.kde import most_likely_samples
from safe_interactive_crowdnav_amd.schedule import VarianceSchedule, ddim_steps
from safe_interactive_crowdnav_amd.weights import JMIDWeights, NetDims, all_shapes

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.mark.parametrize("case", sorted(os.path.basename(p) for p in glob.glob(os.path.join(GOLDEN, "kde_*.npz"))))
def test_kde_topk_matches_reference(case):
    z = np.load(os.path.join(GOLDEN, case))
    top, lw = most_likely_samples(z["forecasts"], int(z["k_ret"]))
    np.testing.assert_array_equal(top, z["top"])
    np.testing.assert_allclose(lw, z["logw"], rtol=1e-5, atol=1e-5)


def test_schedule_matches_reference_buffers():
    z = np.load(os.path.join(GOLDEN, "schedule.npz"))
    s = VarianceSchedule.linear()
    np.testing.assert_array_equal(s.betas, z["betas"])
    # exp / log / sqrt of a torch CPU tensor go through MKL, whose vector code path depends on the CPU: the buffers derived
    # from them are bit-equal on the CPU the fixture was made on and within a few ulp on others (2 / 1 / 4 seen)
    np.testing.assert_array_max_ulp(s.alpha_bars, z["alpha_bars"], maxulp=4)
    np.testing.assert_array_max_ulp(s.sigmas_inflex, z["sigmas_inflex"], maxulp=4)
    np.testing.assert_array_max_ulp(s.sigmas_flex, z["sigmas_flex"], maxulp=4)


def test_ddpm_table_flexibility():
    """get_sigmas (diffusion.py:59-64): sigma = flex * sigmas_flex[t] + (1 - flex) * sigmas_inflex[t]."""
    from safe_interactive_crowdnav_amd.schedule import ddpm_steps
    s = VarianceSchedule.linear()
    t0, t1, th = ddpm_steps(s, 10, 0.0), ddpm_steps(s, 10, 1.0), ddpm_steps(s, 10, 0.5)
    assert [x.t for x in t0] == list(range(100, 0, -10)) and all(x.noise for x in t0)
    assert [x.sigma for x in t0] == [s.sigmas_inflex[x.t] for x in t0]
    assert [x.sigma for x in t1] == [s.sigmas_flex[x.t] for x in t1]
    assert all(min(a.sigma, b.sigma) <= h.sigma <= max(a.sigma, b.sigma) for a, b, h in zip(t0, t1, th))
    assert not ddpm_steps(s, 100)[-1].noise            # t == 1: z = 0 (diffusion.py:571)
    with pytest.raises(ValueError):
        ddpm_steps(s, 10, 1.5)


def test_ddim_table():
    s = VarianceSchedule.linear()
    tab = ddim_steps(s, 50)
    assert [x.t for x in tab] == list(range(100, 0, -2))
    assert tab[-1].n_x == np.float32(1.0) and tab[-1].n_e == np.float32(0.0)   # abar_0 = 1: last step returns x0
    assert [x.t for x in ddim_steps(s, 2)] == [100, 50]
    with pytest.raises(ValueError):
        ddim_steps(s, 30)   # stride 3 does not divide 100 (reference would wrap around)


def test_weight_container_roundtrip(tmp_path):
    dims = NetDims(ctx_dim=32)
    w = JMIDWeights.from_seed(dims, 3)
    assert list(w.tensors) == list(all_shapes(dims))
    assert w.checksum() == JMIDWeights.from_seed(dims, 3).checksum() != JMIDWeights.from_seed(dims, 4).checksum()
    p = str(tmp_path / "w.npz")
    w.save(p)
    w2 = JMIDWeights.load(p)
    assert w2.dims == dims and w2.checksum() == w.checksum()
    n_live = sum(int(np.prod(s)) for k, s in all_shapes(NetDims()).items() if "/" not in k)
    assert n_live == 6_940_432    # live parameter count of the net
    with pytest.raises(KeyError):
        JMIDWeights(dims, {})


def test_reference_state_import():
    """from_reference_state accepts the checkpoint's own key layout (vel_predictor.net.* + ModuleDict)."""
    dims = NetDims(ctx_dim=32)
    w = JMIDWeights.from_seed(dims, 1)
    net_state = {"vel_predictor.net." + k: v for k, v in w.net_state_dict().items()}
    net_state["vel_predictor.net.layer.linear1.weight"] = torch.zeros(1)   # the unused template copy is ignored
    mods = {}
    for name, sd in w.encoder_state_dicts().items():
        if "edge_influence" in name:
            m = torch.nn.Module()
            m.w1 = torch.nn.Linear(16, 16, bias=False)
            m.w2 = torch.nn.Linear(16, 16, bias=False)
            m.v = torch.nn.Linear(16, 1, bias=False)
        else:
            m = torch.nn.LSTM(sd["weight_ih_l0"].shape[1], 16, batch_first=True)
        m.load_state_dict(sd)
        mods[name] = m
    w2 = JMIDWeights.from_reference_state(dims, net_state, mods)
    assert w2.checksum() == w.checksum()


def test_mpc_glue_matches_caller_arithmetic():
    """same arithmetic as SICNavAcados.predict (sicnav_acados.py:1644-1667), written there with
    einops and per-human loops."""
    import einops
    from safe_interactive_crowdnav_amd.mpc_glue import mpc_forecast_inputs

    rng = np.random.default_rng(0)
    N, k, H, horiz, dt = 3, 15, 8, 5, 0.25
    top = rng.standard_normal((N, k, H + 1, 2))
    w = np.log(rng.dirichlet(np.ones(k)))[None].repeat(N, axis=0)
    out = mpc_forecast_inputs(top, w, horiz, dt, joint=True)
    forecasts = top[:, :, 1:, :]
    np.testing.assert_array_equal(out.samples_by_stage,
                                  einops.rearrange(forecasts, "h s t d -> t (h s) d")[: horiz + 1, :, :])
    np.testing.assert_array_equal(out.init_weights, w[0, :])
    for h in range(N):
        assert out.goal_xy[h, 0] == pytest.approx(np.mean(forecasts[h, :, 0, 0]))
        assert out.goal_xy[h, 1] == pytest.approx(np.mean(forecasts[h, :, 0, 1]))
        assert out.v_pref[h] == pytest.approx(np.max(np.linalg.norm(np.diff(forecasts[h], axis=1), axis=2) / dt))
    assert mpc_forecast_inputs(top, w, horiz, dt, joint=False).init_weights.shape == (N, k)


@pytest.mark.parametrize("case", ["mpc_glue_joint.npz", "mpc_glue_indep_outdoor.npz", "mpc_glue_exact_horizon.npz"])
def test_mpc_glue_matches_reference_capture(case, golden_dir):
    """SURVEY 8f row f1 pinned by captures of the reference's own lines (tests/golden/make_golden_mpc.py executes
    sicnav_acados.py:1639-1682 and :1388-1413 against recording stand-ins): forecast slicing, initial weights, the
    't (h s) d' stage layout, goal point / preferred speed / heading per human, and the per-stage Acados parameter
    vectors p_0 .. p_horiz, bit for bit."""
    import os
    from safe_interactive_crowdnav_amd.mpc_glue import human_headings, mpc_forecast_inputs, stage_parameter_blocks

    z = np.load(os.path.join(golden_dir, case))
    horiz, joint, outdoor = int(z["horiz"]), bool(z["joint"]), bool(z["outdoor"])
    out = mpc_forecast_inputs(z["top_k_forecasts"], z["top_k_weights"], horiz, float(z["time_step"]), joint=joint)
    np.testing.assert_array_equal(out.forecasts, z["forecasts"])
    np.testing.assert_array_equal(out.init_weights, z["forecasts_init_weights"])
    np.testing.assert_array_equal(out.samples_by_stage, z["forecasts_reshaped"])
    np.testing.assert_array_equal(out.goal_xy[:, 0], z["gx"])
    np.testing.assert_array_equal(out.goal_xy[:, 1], z["gy"])
    np.testing.assert_array_equal(out.v_pref, z["v_pref"])
    np.testing.assert_array_equal(human_headings(z["human_pxpyvxvy"][:, 2], z["human_pxpyvxvy"][:, 3]), z["theta"])
    p = stage_parameter_blocks(out.samples_by_stage, z["goal_states"], z["goal_actions"], z["Q_diag"], z["R_diag"],
                               z["term_Q_diag"], horiz, static_obs=z["static_obs"] if outdoor else None)
    assert p.shape == z["p_stages"].shape and p.dtype == np.float64
    np.testing.assert_array_equal(p, z["p_stages"])
    with pytest.raises(IndexError):          # the reference indexes MID_samples[horiz] and fails the same way
        stage_parameter_blocks(out.samples_by_stage[:horiz], z["goal_states"], z["goal_actions"], z["Q_diag"],
                               z["R_diag"], z["term_Q_diag"], horiz)


def test_install_aliases_the_reference_module(monkeypatch):
    """``install()``: the reference's caller line (sicnav_acados.py:24) resolves to this package's class without an edit -
    with the reference tree importable (its own parent packages) and without it (stand-in parents)."""
    import importlib
    import sys
    import safe_interactive_crowdnav_amd as P
    from safe_interactive_crowdnav_amd import forecaster as FC

    saved = dict(FC.DEFAULTS)
    for with_reference in (False, True):
        if with_reference and not os.path.isdir("/root/reference/sicnav_diffusion"):
            continue
        for name in [n for n in sys.modules if n == "sicnav_diffusion" or n.startswith("sicnav_diffusion.")]:
            monkeypatch.delitem(sys.modules, name)
        if with_reference:
            monkeypatch.syspath_prepend("/root/reference")
            importlib.invalidate_caches()
        try:
            assert FC.DEFAULTS["precision"] == "f16mx" and FC.DEFAULTS["self_check"] is True      # what bench.py quotes is what a drop-in user runs
            mod = P.install(precision="f16x3", self_check=False)
            stood_in = list(P._STAND_INS)
            assert mod is FC and FC.DEFAULTS["precision"] == "f16x3" and FC.DEFAULTS["self_check"] is False
            ns = {}
            exec("from sicnav_diffusion.JMID.mid_sim_wrapper import HumanTrajectoryForecasterSim", ns)     # the caller's line
            assert ns["HumanTrajectoryForecasterSim"] is FC.HumanTrajectoryForecasterSim
            import sicnav_diffusion.JMID.mid_sim_wrapper as W
            assert W is FC and hasattr(W, "get_most_likely_samples") and hasattr(W, "ForecasterSimSuper")
            with pytest.raises(TypeError):
                P.install(no_such_default=1)
        finally:
            P.uninstall()
            FC.DEFAULTS.clear()
            FC.DEFAULTS.update(saved)
        assert sys.modules.get("sicnav_diffusion.JMID.mid_sim_wrapper") is not FC
        # stand-in parents (registered when the reference tree is not importable) are gone again: the real packages stay
        # importable afterwards
        assert not P._STAND_INS and not any(n in sys.modules for n in stood_in)
        if with_reference:
            assert not stood_in


def test_install_does_not_mask_a_reference_package_that_fails_to_import(tmp_path, monkeypatch):
    """A reference tree that IS on sys.path but whose package __init__ raises (a missing dependency) must surface as that error:
    install() only substitutes a stand-in for "this package does not exist"."""
    import importlib
    import sys
    import safe_interactive_crowdnav_amd as P
    from safe_interactive_crowdnav_amd import forecaster as FC
    (tmp_path / "sicnav_diffusion").mkdir()
    (tmp_path / "sicnav_diffusion" / "__init__.py").write_text("import a_dependency_that_is_not_installed_here\n")
    for name in [n for n in sys.modules if n == "sicnav_diffusion" or n.startswith("sicnav_diffusion.")]:
        monkeypatch.delitem(sys.modules, name)
    monkeypatch.syspath_prepend(str(tmp_path))
    importlib.invalidate_caches()
    saved = dict(FC.DEFAULTS)
    try:
        with pytest.raises(ModuleNotFoundError, match="a_dependency_that_is_not_installed_here"):
            P.install()
    finally:
        P.uninstall()
        FC.DEFAULTS.clear()
        FC.DEFAULTS.update(saved)
    assert "sicnav_diffusion" not in sys.modules


def test_chunk_plan_never_holds_an_empty_chunk():
    """run_network's chunk plan (csrc/jmid_planner.hip::plan_chunks, through the diagnostics entry point; host logic only): the
    sizes add up to E, no chunk is empty - round 4's balanced plan rounded E chunks of ONE episode (K*A*T > 32768 tokens per
    episode) up to E + 1 for odd E, and a zero-episode chunk is a grid-0 launch - and, unforced with two lanes, the count is even
    whenever that is possible."""
    import ctypes as C
    import __graft_entry__ as graft
    from safe_interactive_crowdnav_amd import _lib
    from safe_interactive_crowdnav_amd.build import LIB_DIAG
    graft.build()
    lib = _lib.load_library(LIB_DIAG)
    buf = (C.c_int * 8192)()

    def plan(E, tokens, lanes=2, forced=0, net=_lib.NET_JMID):
        n = lib.jmid_dbg_plan_chunks(net, 4, lanes, forced, E, tokens, buf, len(buf))
        assert 0 < n <= len(buf), n
        return list(buf[:n])

    for tokens in (1200, 19200, 38400, 128 * 25 * 12, 65536, 70000):       # cfg2, cfg4, and shapes whose automatic chunk is 1 episode
        for E in (1, 2, 3, 4, 5, 7, 9, 51, 52, 101, 255, 256, 257, 511, 512, 4096):
            for lanes in (1, 2, 3):
                for net in (_lib.NET_JMID, _lib.NET_IMID):
                    sizes = plan(E, tokens, lanes=lanes, net=net)
                    assert sum(sizes) == E and min(sizes) >= 1, (tokens, E, lanes, sizes[:8])
                    if lanes >= 2 and E >= 2 and len(sizes) < E:
                        assert len(sizes) % 2 == 0 and max(sizes) - min(sizes) <= 1, (tokens, E, sizes[:8])
            for forced in (1, 2, 51):
                sizes = plan(E, tokens, forced=forced)
                assert sum(sizes) == E and min(sizes) >= 1 and max(sizes) <= forced
    assert plan(256, 1200) == [43] * 4 + [42] * 2
    assert plan(3, 38400) == [1, 1, 1] and plan(5, 70000) == [1] * 5       # the advisor's case: c == 1, odd E

    # a small batch by arithmetic mode: at most 2 560 tokens stay ONE chunk in F16MX (the LayerNorms ride in its GEMM launches, which only
    # run while nothing else of the handle is in flight); every other mode, and anything larger, runs as two halves side by side
    def plan_mode(E, tokens, prec, lanes=2):
        n = lib.jmid_dbg_plan_chunks_mode(_lib.NET_JMID, 4, lanes, 0, E, tokens, prec, buf, len(buf))
        assert 0 < n <= len(buf), n
        return list(buf[:n])

    assert plan_mode(2, 1200, _lib.PREC_F16MX) == [2] and plan_mode(2, 1280, _lib.PREC_F16MX) == [2]
    assert plan_mode(2, 1281, _lib.PREC_F16MX) == [1, 1] and plan_mode(3, 1200, _lib.PREC_F16MX) == [2, 1]
    assert plan_mode(4, 600, _lib.PREC_F16MX) == [4] and plan_mode(4, 1200, _lib.PREC_F16MX) == [2, 2]
    for prec in (_lib.PREC_F32, _lib.PREC_F16X3, _lib.PREC_F16X2):
        assert plan_mode(2, 1200, prec) == [1, 1] and plan_mode(4, 600, prec) == [2, 2]
    assert plan_mode(2, 1200, _lib.PREC_F16MX, lanes=1) == [2] and plan_mode(256, 1200, _lib.PREC_F16MX) == [43] * 4 + [42] * 2
    for E in (1, 2, 3, 5, 51, 256):                      # the mode-less entry point = a mode without the rule
        assert plan(E, 1200) == plan_mode(E, 1200, _lib.PREC_F16X3)


# ---- the launch plan of a split-fp16 GEMM (csrc/launch_plan.hpp::plan_gemm through jmid_dbg_gemm_plan; host logic only) ----
GEMM_PLAN_TABLE = os.path.join(GOLDEN, "gemm_plan_table.txt")
GEMM_PLAN_KNOBS = ("gemm_h_variant", "gemm_small", "ln_rows", "small_lnx", "small_lnx2", "cus", "vt_stage", "csl_swap", "h1_stage", "gemm_pn",
                   "small_qk", "small_pn", "gemm_ng")
GEMM_PLAN_DEFAULTS = {**dict.fromkeys(GEMM_PLAN_KNOBS, 0), "cus": 256}
EPI_BIAS, EPI_BIAS_RELU, EPI_CSL = 0, 1, 2
OUT_F32, OUT_SPLIT, OUT_QKV, OUT_LNX = 0, 1, 2, 4
GS_NONE, GS_SMALL_64x64, GS_SMALL_64x128, GS_SMALL_64x128_TWO, GS_SMALL_64x64_TWO, GS_64, GS_128, GS_256x128, GS_256x256, GS_128x256, \
    GS_256x256_NS3, GS_REG_64, GS_REG_128 = range(13)
GS_SMALL = (GS_SMALL_64x64, GS_SMALL_64x128, GS_SMALL_64x128_TWO, GS_SMALL_64x64_TWO)


def gemm_plan_grid():
    """(mode, epi, out, N, K, small_now, one_chunk, knobs) x the token counts: modes x3 / x2 / mx; the (epilogue, output) pairs of the
    net, each on the layers that use it, at d_model 512 and at width 32 (d_ff = 2 d, d_mid = d / 2, d_low = d / 4); the default knobs
    and every forced gemm_h_variant, gemm_small, ln_rows; small_now 0 / 1 / 2.  Token counts from 64 to 262 144, with the points around
    every threshold of the rules, for every N of the net: 256 and 512 small tiles of 64 x 64 / 64 x 128 (N = 1536: 640, 1344, 2688
    rows; 1024: 1024, 2048, 4096; 512: 2048; 256: 4096, 8192, 16384; 128: 8192, 16384, 32768), 256 tiles of 128 x 128 (2688, 3968, 8064,
    16256, 32640), of 256 x 128 (5376, 7936, 16128, 32512, 65280) and of 256 x 256 (10752, 16128), the 7168 / 12288 rows of the 256 x 256
    rule, 2048 / 2560 / 4096 tokens (32, 40 and 64 row tiles of the one-launch GEMM + LayerNorm)."""
    Ms = {64, 100, 1200, 2400, 3600, 4800, 100000, 131072, 262144}
    for base in (640, 1024, 1344, 2048, 2560, 2688, 3968, 4096, 5376, 7168, 7936, 8064, 8192, 10752, 12288, 16128, 16256, 16384, 32512, 32640,
                 32768, 65280, 65536):
        Ms |= {base - 64, base - 1, base, base + 1, base + 64}
    Ms = sorted(Ms)
    cases = []
    for d in (512, 32):
        layers = [(EPI_BIAS, OUT_QKV, 3 * d, d), (EPI_BIAS, OUT_F32, 3 * d, d), (EPI_BIAS, OUT_F32, d, d), (EPI_BIAS, OUT_F32, d, 2 * d),
                  (EPI_BIAS_RELU, OUT_SPLIT, 2 * d, d), (EPI_CSL, OUT_SPLIT, d // 2, d), (EPI_CSL, OUT_F32, d // 4, d // 2)]
        if d == 512:
            layers += [(EPI_BIAS, OUT_LNX, d, d), (EPI_BIAS, OUT_LNX, d, 2 * d)]
        knob_sets = [{}] + [{"gemm_h_variant": v} for v in range(1, 9)] + [{"gemm_small": v} for v in (1, 2)] + [{"ln_rows": v} for v in (64, 128)]
        for mode in (0, 1, 2):
            for epi, out, N, K in layers:
                if out == OUT_LNX and mode != 2:        # (asked for in F16MX only: residual_path)
                    continue
                for small_now in (0, 1, 2):
                    for one_chunk in ((0, 1) if out == OUT_LNX else (1,)):
                        for ks in knob_sets:
                            cases.append((mode, epi, out, N, K, small_now, one_chunk, GEMM_PLAN_DEFAULTS | ks))
    return Ms, cases


def gemm_plan_rows(lib):
    """The plans of the whole grid as the lines of the table.  A plan row is one cell 'shape family . flags . group_tiles'
    (hexadecimal) per token count, equal neighbours folded as cell*count; every distinct row is written once, followed by the
    cases that have it: 'mode epi out N K | ... : small_now.one_chunk:forced knobs ...' (v = gemm_h_variant, s = gemm_small, r = ln_rows,
    - = defaults, * = all thirteen knob sets).  The row tiles of the two GEMM + LayerNorm generations depend on the token count and
    "ln_rows" only: three rows of their own."""
    import ctypes as C
    Ms, cases = gemm_plan_grid()
    out8 = (C.c_int * 8)()

    def fold(cells):
        runs = []
        for c in cells:
            if runs and runs[-1][0] == c:
                runs[-1][1] += 1
            else:
                runs.append([c, 1])
        return " ".join(f"{c}*{n}" for c, n in runs)

    short = {"gemm_h_variant": "v", "gemm_small": "s", "ln_rows": "r"}
    plans, groups, ln_rows, knob_codes = [], {}, {}, []
    for mode, epi, out, N, K, small_now, one_chunk, knobs in cases:
        kv = (C.c_int * len(GEMM_PLAN_KNOBS))(*[knobs[k] for k in GEMM_PLAN_KNOBS])
        cells = []
        for M in Ms:
            assert lib.jmid_dbg_gemm_plan(mode, epi, out, M, N, K, small_now, one_chunk, kv, out8) == 0
            family, shape, flags, gt, bm, bn, rows1, rows2 = out8[:8]
            plans.append(((mode, epi, out, M, N, K, small_now, one_chunk, knobs), (family, shape, flags, gt, bm, bn)))
            fam = family if shape != GS_NONE else "-"        # (no launch, no kernel family)
            cells.append(f"{shape:x}{fam}.{flags:x}.{gt:x}")
            assert ln_rows.setdefault((knobs["ln_rows"], M), (rows1, rows2)) == (rows1, rows2)
        code = "".join(f"{short[k]}{v}" for k, v in knobs.items() if v != GEMM_PLAN_DEFAULTS[k]) or "-"
        if code not in knob_codes:
            knob_codes.append(code)
        groups.setdefault(fold(cells), {}).setdefault((mode, epi, out, N, K), {}).setdefault((small_now, one_chunk), []).append(code)
    lines = ["# M: " + " ".join(str(m) for m in Ms)]
    for r in (0, 64, 128):
        lines.append(f"ln_rows={r} : " + fold([f"{ln_rows[(r, M)][0] // 64}{ln_rows[(r, M)][1] // 64}" for M in Ms]))
    for row, layers in groups.items():
        lines.append("row " + row)
        by_facts = {}
        for layer, facts in layers.items():
            text = " ".join(f"{s}.{c}:" + ("*" if codes == knob_codes else ",".join(codes)) for (s, c), codes in facts.items())
            by_facts.setdefault(text, []).append(" ".join(map(str, layer)))
        for text, same in by_facts.items():
            lines.append("  " + " | ".join(same) + " : " + text)
    return lines, plans


def test_gemm_plans_at_d_model_192_mix_the_modes_and_cut_the_last_column_tile():
    """What the rows (96, 6) and (96, 12) of tests/width_cases.py are there for, read from csrc/launch_plan.hpp: in an F16MX call in_proj
    (N = 576), out_proj and linear2 (N = 192) run F16X2's kernels and linear1 (N = 384) F16MX's own; no GEMM of the layer takes a small
    launch (K % 128 != 0); and a batch of 16 800 rows takes the 128 x 128 shape with a partial last column tile at N = 576 and 192 - the
    shapes tests/test_gpu_kernels.py and tests/test_gpu_parity.py run on the device."""
    import ctypes as C

    import __graft_entry__ as graft
    from safe_interactive_crowdnav_amd import _lib
    from safe_interactive_crowdnav_amd.build import LIB_DIAG
    graft.build()
    lib = _lib.load_library(LIB_DIAG)
    kv = (C.c_int * len(GEMM_PLAN_KNOBS))(*[GEMM_PLAN_DEFAULTS[k] for k in GEMM_PLAN_KNOBS])
    out8 = (C.c_int * 8)()
    X3, X2, MX = 0, 1, 2
    d = 192
    layers = {"in_proj": (EPI_BIAS, OUT_QKV, 3 * d, d), "out_proj": (EPI_BIAS, OUT_F32, d, d), "linear1": (EPI_BIAS_RELU, OUT_SPLIT, 2 * d, d),
              "linear2": (EPI_BIAS, OUT_F32, d, 2 * d)}
    for mode in (X3, X2, MX):
        for name, (epi, out, N, K) in layers.items():
            for M in (1, 315, 384, 16800):
                assert lib.jmid_dbg_gemm_plan(mode, epi, out, M, N, K, 1, 1, kv, out8) == 0
                family, shape, _, _, bm, bn = out8[:6]
                assert family == (mode if mode != MX or name == "linear1" else X2), (mode, name, M, family)
                assert shape not in GS_SMALL and shape != GS_NONE, (mode, name, M, shape)
                if M == 16800:
                    assert (shape, bm, bn) == (GS_128, 128, 128), (mode, name, shape)
                    assert (N % bn != 0) == (name != "linear1")
    # the one-launch GEMM + LayerNorm is not asked for off d_model 512 (residual_path), and would not fit: K % 128 != 0
    assert lib.jmid_dbg_gemm_plan(MX, EPI_BIAS, OUT_LNX, 315, d, d, 1, 1, kv, out8) == 0 and out8[1] == GS_NONE


def test_gemm_launch_plans_are_the_ones_the_launchers_used_to_pick():
    """csrc/launch_plan.hpp::plan_gemm reproduces, on the whole grid, what the per-launch rules it replaced decided (tests/golden/
    gemm_plan_table.txt: dumped from those rules, cut unchanged out of the launchers into functions that return the shape, before
    they were unified) - and never returns a shape that is not built for the mode and epilogue, or a small shape whose tiles do not
    fit the chip."""
    import __graft_entry__ as graft
    from safe_interactive_crowdnav_amd import _lib
    from safe_interactive_crowdnav_amd.build import LIB_DIAG
    graft.build()
    lines, plans = gemm_plan_rows(_lib.load_library(LIB_DIAG))
    want = open(GEMM_PLAN_TABLE).read().splitlines()
    assert len(lines) == len(want) > 50 and len(plans) > 200000
    for got, exp in zip(lines, want):
        assert got == exp
    seen = set()
    for (mode, epi, out, M, N, K, small_now, one_chunk, knobs), (family, shape, flags, gt, bm, bn) in plans:
        seen.add(shape)
        tiles = -(-M // bm) * -(-N // bn)
        assert family in (0, 1, 2) and (family == mode or (mode == 2 and family == 1))
        if family == 2:
            assert K % 64 == 0 and N % 128 == 0 and shape not in (GS_REG_64, GS_REG_128)
        else:
            assert shape not in (GS_128x256, GS_256x256_NS3)
        assert (shape == GS_NONE) <= (out == OUT_LNX)
        if out == OUT_LNX:
            assert shape in (GS_NONE, GS_SMALL_64x64, GS_SMALL_64x64_TWO)
        if epi == EPI_CSL:
            assert shape not in (GS_256x256, GS_128x256, GS_256x256_NS3) and not (family == 2 and out == OUT_F32 and shape == GS_256x128)
        if shape in (GS_256x256, GS_128x256, GS_256x256_NS3):
            assert N % 256 == 0
        if shape in GS_SMALL:
            assert small_now and knobs["gemm_small"] != 1 and knobs["gemm_h_variant"] == 0 and K % 128 == 0 and N % bn == 0 and bm == 64
            two = shape in (GS_SMALL_64x128_TWO, GS_SMALL_64x64_TWO)
            assert tiles <= (512 if two else 256) and (not two or family != 0)      # one workgroup per CU, or two (not F16X3)
            assert gt >= 1 and (N // bn) % gt == 0
            if out == OUT_LNX:
                assert small_now == 1 and one_chunk == 1 and family == 2 and -(-M // 64) <= 64
    assert seen == set(range(13))        # every shape of the enum is reached on the grid


def test_module_level_get_most_likely_samples_has_the_reference_signature():
    """mid_sim_wrapper.get_most_likely_samples(forecasts, mid_model, num_ret_samples) -> torch tensors [A, k, H, 2], [A, k]."""
    from safe_interactive_crowdnav_amd.forecaster import get_most_likely_samples, topk_fits_device
    z = np.load(os.path.join(GOLDEN, sorted(glob.glob(os.path.join(GOLDEN, "kde_*.npz")))[0]))
    top, lw = get_most_likely_samples(torch.from_numpy(z["forecasts"]), object(), int(z["k_ret"]))
    assert isinstance(top, torch.Tensor) and isinstance(lw, torch.Tensor)
    np.testing.assert_array_equal(top.numpy(), z["top"])
    np.testing.assert_allclose(lw.numpy(), z["logw"], rtol=1e-5, atol=1e-5)
    # the device kernel's size limits (include/jmid_hip.h): beyond them the class falls back to the host twin
    assert topk_fits_device(32, 1024, 24) and not topk_fits_device(33, 100, 8) and not topk_fits_device(5, 1025, 8) \
        and not topk_fits_device(5, 100, 25)


def test_rank_cpu_shares_are_disjoint_and_numa_local():
    """bench.rank_cpu_share (the per-rank CPU placement of a multi-rank launch): contiguous disjoint shares of the allowed cores; with
    NUMA information the ranks whose GPUs hang off one node split THAT node's cores; degenerate inputs never give an empty share."""
    import bench
    allowed = list(range(256))
    sh = [bench.rank_cpu_share(allowed, r, 8) for r in range(8)]
    assert all(len(x) == 32 for x in sh) and sorted(sum(sh, [])) == allowed
    numa = [0, 0, 0, 0, 1, 1, 1, 1]
    nodes = {0: list(range(0, 64)) + list(range(128, 192)), 1: list(range(64, 128)) + list(range(192, 256))}
    sh = [bench.rank_cpu_share(allowed, r, 8, numa, nodes) for r in range(8)]
    assert sorted(sum(sh, [])) == allowed and all(set(sh[r]) <= set(nodes[numa[r]]) for r in range(8))
    # a cpuset smaller than the node list (a container): only allowed cores are handed out
    sh = [bench.rank_cpu_share(list(range(0, 16)), r, 8, numa, nodes) for r in range(8)]
    assert all(len(x) >= 1 and set(x) <= set(range(16)) for x in sh)
    assert bench.rank_cpu_share([3, 4], 5, 8) == [3, 4]                      # fewer cores than ranks: everybody gets them all
    assert bench.rank_cpu_share(allowed, 2, 3, [None, None, None], {}) == allowed[171:256]
    assert bench._cpulist("0-3,8,10-11\n") == [0, 1, 2, 3, 8, 10, 11]


def test_compact_bench_line_always_fits_and_always_parses():
    """bench.compact_line never asserts and never loses the contract keys, however long the notes of the long result are (the driver
    parses this one stdout line; round 4's 20 KB line was not parsed)."""
    import json
    import bench
    full = {"metric": "m", "value": 1.0, "unit": "traj/s", "n_gpus": 1, "steps": 1, "warmup": 0, "ms_per_step": 1.0, "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None, "dtype": "x" * 3000, "data": "synthetic",
            "config": {"workload_short": "w" * 3000, "episodes_per_gpu": 1, "total_episodes": 1, "humans": 5, "samples": 20, "horizon": 12,
                       "denoise_steps": 50, "net": "jmid", "precision": "f16mx", "lanes": 2, "dist_backend": None},
            "cpu_baseline": {"value": 1.0, "unit": "traj/s", "cores": 1, "kind": "port", "processes": 1, "threads_per_process": 1,
                             "hardware_threads": 1, "host_physical_cores": 1, "sample_short": "s" * 3000, "cores_short": "c" * 3000},
            "modes": {m: {"value": 1.0, "ms_per_step": 1.0} for m in ("f16mx", "f16x2", "f16x3")}}
    line = bench.compact_line(full, "/tmp/detail.json")
    assert len(line) <= bench.COMPACT_LIMIT
    j = json.loads(line)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline"):
        assert k in j, k


# ---- the layouts of a chained call's I/O block and of the scene workspace (csrc/jmid_abi.hip::chain_io, scene_arrays through
# jmid_dbg_chain_layout; host logic only) ----
L_SCENE, L_FORECAST, L_SEEDED, L_PADDED, L_FIRST, L_BW, L_POS, L_CV = (1 << i for i in range(8))
CHAIN_ARRAYS = ("x_st", "nbr_sum", "edge_mask", "x_T", "p0", "bw", "ctx", "flag", "forecasts", "logw_d", "sel", "logw", "pos", "first_index")
SCENE_ARRAYS = ("human_xy", "robot_xy", "pose_now", "x", "x_st", "nbr_sum", "edge_mask", "p0", "n_in", "in_cluster", "robot_in", "cv", "first_index")
LAYOUT_ALIGN = 256


def _check_block(arrays, total):
    """arrays {name: (offset, bytes)} of the arrays present: every offset on the rounding rule, no two overlap, the size is the last end"""
    spans = sorted(arrays.values())
    assert all(o % LAYOUT_ALIGN == 0 and b > 0 for o, b in spans), arrays
    assert all(o0 + b0 <= o1 for (o0, b0), (o1, _) in zip(spans, spans[1:])), arrays
    up = lambda v: -(-v // LAYOUT_ALIGN) * LAYOUT_ALIGN
    assert total == up(spans[-1][0] + spans[-1][1]), (arrays, total)


def _contiguous(arrays, names, start):
    """the arrays `names` that are present lie one behind the other from `start`, each rounded up -> the end"""
    for n in names:
        if n in arrays:
            assert arrays[n][0] == start, (n, arrays, start)
            start += -(-arrays[n][1] // LAYOUT_ALIGN) * LAYOUT_ALIGN
    return start


@pytest.mark.parametrize("dims", [(1, 1, 2, 1, 1), (3, 5, 20, 12, 7)], ids=["e1a1k2t1n1", "e3a5k20t12n7"])
def test_chain_and_scene_layouts(dims):
    """Every mode combination of the chained entries at two shapes (hist_len 6, ctx_dim 32): 256-byte offsets, no overlap, the upload
    arrays the contiguous prefix in their order, the download arrays one contiguous range (ending behind the assembled arrays of a
    forecast), the bytes of include/jmid_hip.h's shapes, the size = the last end, the pinned block = upload + download at the same inner
    offsets; the combinations no entry makes are refused.  The scene workspace likewise, the grid block its first bytes."""
    import ctypes as C
    import itertools
    import __graft_entry__ as graft
    from safe_interactive_crowdnav_amd import _lib
    from safe_interactive_crowdnav_amd.build import LIB_DIAG
    graft.build()
    lib = _lib.load_library(LIB_DIAG)
    E, A, K, T, N = dims
    Th, ctx_dim = 6, 32
    n_chain, n_scene = 2 * len(CHAIN_ARRAYS) + 5, 2 * len(SCENE_ARRAYS) + 4

    def layout(k, flags):
        dev, pin, scn = (C.c_int64 * n_chain)(), (C.c_int64 * n_chain)(), (C.c_int64 * n_scene)()
        rc = lib.jmid_dbg_chain_layout(Th, ctx_dim, E, A, K, T, k, N, flags, dev, pin, scn)
        if rc:
            return None

        def block(words, names):
            arrays = {n: (words[2 * i], words[2 * i + 1]) for i, n in enumerate(names)}
            assert all((o == -1) == (b == 0) for o, b in arrays.values()), arrays
            return {n: v for n, v in arrays.items() if v[1]}, list(words[2 * len(names):])
        return block(dev, CHAIN_ARRAYS), block(pin, CHAIN_ARRAYS), block(scn, SCENE_ARRAYS)

    n_valid = 0
    for scene, forecast, seeded, padded, first, (k, bw) in itertools.product(*[(False, True)] * 5, ((1, True), (1, False), (K, False))):
        rank = k < K
        for pos in ((False, True) if rank and not forecast else (not forecast,)):
            flags = (scene * L_SCENE | forecast * L_FORECAST | seeded * L_SEEDED | padded * L_PADDED | first * L_FIRST | bw * L_BW | pos * L_POS
                     | forecast * L_CV)
            got = layout(k, flags)
            if not scene and (forecast or seeded or first):
                assert got is None, "forecast, seeded noise and first_index exist in scene mode only"
                continue
            assert got is not None, (dims, k, flags)
            n_valid += 1
            (dev, (up_off, up_bytes, down_off, down_bytes, total)), (pin, (p_up_off, p_up_bytes, p_down_off, p_down_bytes, p_total)), _ = got
            EA, f4 = E * A, 4
            want = {"x_st": EA * Th * 6 * f4, "nbr_sum": EA * 2 * Th * 6 * f4, "edge_mask": EA * 2 * f4, "x_T": E * K * A * T * 2 * f4, "p0": EA * 2 * f4,
                    "ctx": EA * ctx_dim * f4, "flag": 4}
            if rank and bw:
                want["bw"] = T * f4
            if forecast:
                want.update(forecasts=E * N * k * (T + 1) * 2 * 8, logw_d=E * N * k * 8)
            if rank:
                want.update(sel=EA * k * T * 2 * f4, logw=EA * k * f4)
            if pos:
                want["pos"] = E * K * A * T * 2 * f4
            if first:
                want["first_index"] = EA * 4
            assert {n: b for n, (_, b) in dev.items()} == want, (dims, k, flags)
            _check_block(dev, total)
            # the upload block: the prefix, in the stated order; ctx behind it; then the download block
            upload, download = ("x_st", "nbr_sum", "edge_mask", "x_T", "p0", "bw"), ("flag", "forecasts", "logw_d", "sel", "logw", "pos")
            assert up_off == 0 and _contiguous(dev, upload, 0) == up_bytes == dev["ctx"][0]
            assert _contiguous(dev, ("ctx",), up_bytes) == down_off
            end = _contiguous(dev, download, down_off)
            if forecast:      # the one copy ends behind the assembled arrays; sel / logw stay on the device
                assert down_off + down_bytes == _contiguous(dev, download[:3], down_off) <= end
            else:
                assert down_off + down_bytes == end
            assert _contiguous(dev, ("first_index",), end) == total
            # the pinned block: exactly upload + download, the same inner offsets
            moved = [n for n in upload + (download[:3] if forecast else download) if n in dev]
            assert sorted(pin) == sorted(moved) and all(pin[n][1] == dev[n][1] for n in moved)
            _check_block(pin, p_total)
            assert (p_up_off, p_up_bytes, p_down_off, p_down_bytes, p_total) == (0, up_bytes, up_bytes, down_bytes, up_bytes + down_bytes)
            for n in moved:
                inner = (dev[n][0] - up_off, pin[n][0] - p_up_off) if n in upload else (dev[n][0] - down_off, pin[n][0] - p_down_off)
                assert inner[0] == inner[1], n
    # per (k, bw, pos): 5 calls that rank or return pos, 3 forecasts.  Host arrays: {uniform, padded} x 5; scene: {x_T, seeded} x {uniform,
    # padded} x {no first_index, first_index} x (5 + 3)
    assert n_valid == 2 * 5 + 8 * (5 + 3)
    # the calls no entry makes
    assert layout(K, L_SCENE) is None and layout(K, 0) is None                      # k == K needs pos_out
    assert layout(1, L_SCENE | L_FORECAST) is None                                  # a forecast needs the scene's cv
    assert layout(1, L_SCENE | L_FORECAST | L_CV | L_POS) is None                   # ... and downloads no pos
    assert layout(K + 1, L_POS) is None and layout(0, L_POS) is None

    # the scene workspace, with and without cv and first_index
    for cv, first in itertools.product((False, True), repeat=2):
        _, _, (scn, (grid_bytes, down_off, down_bytes, total)) = layout(K, L_SCENE | L_POS | cv * L_CV | first * L_FIRST)
        rows = E * N
        want = {"human_xy": E * Th * N * 2 * 8, "robot_xy": E * Th * 2 * 8, "pose_now": rows * 2 * 8, "x": rows * Th * 6 * 4, "x_st": rows * Th * 6 * 4,
                "nbr_sum": rows * 2 * Th * 6 * 4, "edge_mask": rows * 2 * 4, "p0": rows * 2 * 4, "n_in": E * 4, "in_cluster": rows, "robot_in": E}
        if cv:
            want["cv"] = rows * T * 2 * 8
        if first:
            want["first_index"] = rows * 4
        assert {n: b for n, (_, b) in scn.items()} == want
        _check_block(scn, total)
        assert _contiguous(scn, SCENE_ARRAYS[:3], 0) == grid_bytes                  # its first bytes: the grid block's three arrays
        assert _contiguous(scn, SCENE_ARRAYS[3:8], grid_bytes) == down_off
        end = _contiguous(scn, SCENE_ARRAYS[8:12], down_off)
        assert down_off + down_bytes == end and _contiguous(scn, SCENE_ARRAYS[12:], end) == total
