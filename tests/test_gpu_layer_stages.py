"""Every stage of one transformer encoder layer, as a denoise step launches it, against float64 - element by element, in every mode.

``JmidEngine.dbg_layer`` (jmid_dbg_layer) runs layer ``layer`` launch for launch as a step of a one-chunk call of the case's shape
runs it and copies every stage out as two planes.  Each stage is compared with the float64 reference of tests/layer_reference.py fed
the DEVICE's output of the stage before it - errors never compound - under that file's componentwise bound: every element of every
real row (only the query rows of padded agents are left out: garbage by design, NaN at the ABI).  Beside it the project's looser
convention, TOL[precision] max(1, max|ref|) against the plain float64 reference.  A line per stage gives the worst err / bound and
where it sits (row mod 128, column mod 64): a failure points at a tile position.

tests/test_layer_bounds_host.py shows that the bounds hold for an emulated correct kernel and catch nine emulated wrong ones."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import layer_reference as R  # noqa: E402
import width_cases as WC  # noqa: E402
from safe_interactive_crowdnav_amd.engine import JmidEngine  # noqa: E402
from safe_interactive_crowdnav_amd.weights import JMIDWeights, NetDims  # noqa: E402

MODES = ["f32", "f16x3", "f16x2", "f16mx"]
SPLIT = ["f16x3", "f16x2", "f16mx"]
TOL = {"f32": 2e-5, "f16x3": 4e-5, "f16x2": 2e-3, "f16mx": 2e-3}      # tests/test_gpu_kernels.py
TOL_MX_LN = 6e-3                                                      # ... its F16MX GEMM + LayerNorm tests
# GemmShape (csrc/launch_plan.hpp) and ResidualPath (csrc/jmid_planner.hip) words of the plan
GS_SMALL = (1, 2, 3, 4)
GS_LARGE = tuple(range(5, 13))      # GS_64 ... GS_REG_128
GS_SMALL_64x128_TWO, GS_SMALL_64x64_TWO, GS_256x256 = 3, 4, 8
RB_GEMM_LN2, RB_GEMM_LN, RB_LNX_SMALL, RB_GEMM_ADD_LN = 0, 1, 2, 3

_ENGINES = {}


def get_engine(d, joint, nhead=4):
    key = (d, nhead, joint)
    if key not in _ENGINES:
        w = JMIDWeights.from_seed(NetDims(ctx_dim=d // 2, nhead=nhead), 5)
        _ENGINES[key] = (JmidEngine(w, joint=joint, step=5), w)
    return _ENGINES[key]


def worst(err, bound, rows):
    r = (err / bound)[rows]
    i = np.unravel_index(int(np.argmax(r)), r.shape)
    row = int(np.flatnonzero(rows)[i[0]]) if rows.dtype == bool else int(i[0])
    return float(r[i]), row, int(i[1])


def check_layer(d, joint, shape, n_agents, precision, layer, last, expect=None, nhead=4, X=None, report=None):
    """One jmid_dbg_layer call, every stage present against its reference.  Returns (plan, stages).  X: another input than the case's
    layer_input; report: a dict that receives (ref, bound) of the attention stage ("attention") and of stage 3 ("norm1")."""
    eng, w = get_engine(d, joint, nhead)
    assert eng.dims.nhead == nhead and eng.dims.d_model == d
    E, A, K, T = shape
    M = E * A * K * T
    nseq, S = (E, K * A * T) if joint else (E * K * A, T)
    if X is None:
        X = R.layer_input(shape, n_agents, d)
    stages, plan = eng.dbg_layer(X, layer, shape, precision, n_agents=n_agents, last=last)
    tag = f"{'jmid' if joint else 'imid'} {shape} n={n_agents} d={d}{'' if nhead == 4 else f' nhead={nhead}'} [{precision}] layer {layer}{' (last)' if last else ''}"
    print(f"{tag} plan: {plan}")
    assert plan["range_flag"] == 0
    spec = R.stage_specs(precision, joint, plan, last)
    lw = R.layer_weights(w.tensors, layer)
    real = R.real_rows(n_agents, E, A, K, T)
    every = np.ones(M, bool)
    assert int((~real).sum()) == (0 if n_agents is None else sum((A - n) * K * T for n in n_agents))
    valid = R.key_valid(n_agents, E, A, K, T) if joint else np.ones((nseq, S), bool)
    assert plan["masked"] == int(n_agents is not None and joint)
    hd = d // eng.dims.nhead
    merged = lambda s: stages[s][0].astype(np.float64) + stages[s][1].astype(np.float64)
    tol = lambda s: TOL_MX_LN if precision == "f16mx" and s in (3, 5) and d == 512 else TOL[precision]
    failures = []

    def judge(s, ref, bound, plain, rows):
        got = merged(s)
        assert np.isfinite(got[rows]).all(), (tag, s)
        ratio, row, col = worst(np.abs(got - ref), bound, rows)
        plain_err = float(np.abs(got - plain)[rows].max())
        plain_tol = tol(s) * max(1.0, float(np.abs(plain[rows]).max()))
        print(f"{tag} stage {s}: worst err/bound {ratio:.4f} at row {row} (mod 128: {row % 128}) col {col} (mod 64: {col % 64}); "
              f"|err| vs plain float64 {plain_err:.3e} (allowed {plain_tol:.3e})")
        if not ratio <= 1.0:
            failures.append((s, "bound", ratio, row % 128, col % 64))
        if not plain_err <= plain_tol:
            failures.append((s, "TOL", plain_err, plain_tol))

    # stage 0: the split itself
    x_rep = "f32" if precision == "f32" else spec["x_rep"]
    assert (np.abs(merged(0) - X) <= R.out_term(X.astype(np.float64), x_rep)).all(), (tag, "stage 0")
    # stage 1
    ref, bound, plain = R.qkv_stage(*stages[0], lw["in_w"], lw["in_b"], spec["in_proj"], spec["qkv_reps"], R.LOG2E / np.sqrt(hd))
    judge(1, ref, bound, plain, every)
    # stage 2 (absent when the out-projection's launch merges the split-KV partials: stage 3 is then judged from stage 1)
    att = R.attention_stage(*stages[1], nseq, S, eng.dims.nhead, valid, spec["logits"], spec["p_rep"], spec["v_lo"], spec["attn_out"],
                            plan["attn_nsplit"])
    if stages[2] is not None:
        assert not plan["merge"]
        judge(2, *att, real)
        r3 = R.ln_stage(*stages[0], *stages[2], lw["out_w"], lw["out_b"], lw["n1_g"], lw["n1_b"], spec["out_proj"], spec["x_rep"])
    else:
        assert plan["merge"] and plan["out_proj_path"] == RB_LNX_SMALL
        r3 = R.ln_stage(*stages[0], att[0], np.zeros_like(att[0]), lw["out_w"], lw["out_b"], lw["n1_g"], lw["n1_b"], spec["out_proj"],
                        spec["x_rep"], A_err=att[1], A_plain=att[2])
    judge(3, *r3, real)
    if report is not None:
        report.update(attention=att[:2], norm1=r3[:2])
    judge(4, *R.gemm_stage(*stages[3], lw["l1_w"], lw["l1_b"], spec["linear1"], True, spec["h1_rep"]), real)
    judge(5, *R.ln_stage(*stages[3], *stages[4], lw["l2_w"], lw["l2_b"], lw["n2_g"], lw["n2_b"], spec["linear2"], spec["x_last_rep"]), real)
    assert not failures, (tag, failures)
    seen = dict(plan, in_proj_vt_bits=plan["in_proj_flags"] & 3, linear1_h1_bit=plan["linear1_flags"] & 16)      # (launch_plan.hpp gemm_flags)
    for key, want in (expect or {}).items():
        ok = seen[key] in want if isinstance(want, (tuple, list)) else seen[key] == want
        assert ok, (tag, key, seen[key], want)
    return plan, stages


def both_layers(d, joint, shape, n_agents, precision, expect=None, nhead=4):
    eng, _ = get_engine(d, joint, nhead)
    check_layer(d, joint, shape, n_agents, precision, 1, False, expect, nhead)
    return check_layer(d, joint, shape, n_agents, precision, eng.dims.tf_layer - 1, True, expect, nhead)


# (E, A, K, T), n_agents, also at d_model 64
JMID_SHAPES = [((1, 1, 1, 1), None, True),             # M = S = 1
               ((2, 2, 3, 4), None, True),             # S = 24: one partial key tile, fewer than 64 rows
               ((3, 3, 5, 7), None, True),             # S = 105, S % 4 != 0: v_transpose_kernel; M = 315
               ((1, 5, 20, 12), None, False),          # one scene: small-launch GEMMs, OUT_LNX, 1200 = 9 x 128 + 48
               ((1, 3, 100, 8), None, False),          # M = 2400: two workgroups per CU
               ((3, 4, 8, 12), [4, 1, 3], True),       # S = 384: all-ones, all-zero and partial mask words
               ((3, 3, 5, 6), [2, 3, 1], True),        # S = 90: the last key tile cut by both S and the mask
               ((1, 4, 8, 12), [1], False)]            # one padded scene through OUT_LNX
OLD_D = tuple(sorted((WC.d_model(c) for c, _ in WC.OLD_NETS), reverse=True))      # d_model of the suite's two nhead = 4 networks
JMID_CASES = [(s, n, d) for s, n, small in JMID_SHAPES for d in (OLD_D if small else OLD_D[:1])]


GM_X3, GM_X2, GM_MX = 0, 1, 2      # GemmMode (csrc/launch_plan.hpp)


def expectation(shape, n_agents, d, precision, nhead=4):
    """which kernel the case is there for: the facts of csrc/launch_plan.hpp / csrc/jmid_planner.hip each row of tests/width_cases.py exists
    for - a planner change that silently stops exercising a path fails the test"""
    if precision == "f32":
        return {}
    e = {}
    S = shape[1] * shape[2] * shape[3]
    head = d // nhead
    mx = precision == "f16mx"
    e["vt_direct"] = int(S % 4 == 0)
    e["attn_dma"] = int(head == 128)                                    # plan_attn: the LDS-DMA kernel is head 128's
    if d == 512:
        if not (shape == (1, 3, 100, 8) and precision == "f16x3"):      # (F16X3 has no two-workgroups-per-CU small shape)
            e["in_proj_shape"] = GS_SMALL
        if mx:
            # byte_lo_plane and residual_path look at d_model alone: the byte plane and the one-launch GEMM + LayerNorm beside either
            # attention kernel; the bf8 K images are the LDS-DMA kernel's (plan_step: k8 needs head 128)
            e.update(k8=int(head == 128), q8l=int(head == 128), byte_lo=1, out_proj_path=RB_LNX_SMALL, linear2_path=RB_LNX_SMALL)
        else:
            e.update(out_proj_path=RB_GEMM_ADD_LN, linear2_path=RB_GEMM_ADD_LN)
    else:
        # residual_path: no row-complete kernel and no OUT_LNX launch off d_model 512 (GLN_BN); byte_lo_plane: none either
        e.update(byte_lo=0, out_proj_path=RB_GEMM_ADD_LN, linear2_path=RB_GEMM_ADD_LN, merge=0)
    if head != 128:
        e.update(k8=0, q8l=0, attn_nsplit=1, merge=0)                   # plan_call: only head 128's launches split the key range
    if d == 1024 and mx:
        e.update(k8=1, q8l=1)                                           # head 128 through nhead 8: the bf8 images without the byte plane
    if d == 192:
        # plan_gemm: F16MX needs N % 128 == 0 (in_proj 576, out_proj / linear2 192: F16X2's kernels; linear1 384: its own) - one step
        # mixes the two; small_gemm_shape refuses K % 128 != 0 for every GEMM of the layer
        word = {"f16x3": GM_X3, "f16x2": GM_X2, "f16mx": GM_MX}[precision]
        narrow = GM_X2 if mx else word
        e.update(in_proj_mode=narrow, out_proj_mode=narrow, linear2_mode=narrow, linear1_mode=word, in_proj_shape=GS_LARGE, linear1_shape=GS_LARGE)
    if shape == (1, 3, 100, 8) and precision in ("f16x2", "f16mx"):
        e["in_proj_shape"] = GS_SMALL_64x128_TWO
        if precision == "f16mx":
            e["out_proj_gemm_shape"] = GS_SMALL_64x64_TWO
    if shape == (1, 5, 20, 12) and precision == "f16mx" and d == 512 and head == 128:
        e["merge"] = 1                                                  # small_cmb_fits: the merge rides in the OUT_LNX launch behind the LDS-DMA kernel only
    return e


@pytest.mark.parametrize("precision", MODES)
@pytest.mark.parametrize("shape,n_agents,d", JMID_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_jmid_layer_stages_stay_inside_their_bounds(shape, n_agents, d, precision):
    both_layers(d, True, shape, n_agents, precision, expectation(shape, n_agents, d, precision))


# ---- the rows of tests/width_cases.py the suite did not run before: (E, A, K, T), n_agents, only at d_model >= 512
NEW_SHAPES = [((1, 1, 1, 1), None, False),
              ((3, 3, 5, 7), None, False),             # S = 105, S % 4 != 0; M = 315: more than one row tile, the last one partial
              ((3, 4, 8, 12), [4, 1, 3], False),       # all-ones, all-zero and partial mask words
              ((1, 5, 20, 12), None, True)]            # one scene: the small launches / OUT_LNX / the merge - or, at d_model 1024, none of them planned
NEW_CASES = [(net, s, n) for net in WC.NEW_NETS for s, n, wide in NEW_SHAPES if not wide or WC.d_model(net[0]) >= 512]


@pytest.mark.parametrize("precision", MODES)
@pytest.mark.parametrize("net,shape,n_agents", NEW_CASES, ids=lambda v: WC.net_id(v) if isinstance(v, tuple) and len(v) == 2 else str(v).replace(" ", ""))
def test_jmid_layer_stages_at_every_accepted_width_and_head_size(net, shape, n_agents, precision):
    d, nhead = WC.d_model(net[0]), net[1]
    both_layers(d, True, shape, n_agents, precision, expectation(shape, n_agents, d, precision, nhead), nhead)


@pytest.mark.parametrize("precision", MODES)
@pytest.mark.parametrize("pack", [1, 0])
@pytest.mark.parametrize("net", [(64, 4), (128, 4), (256, 8)], ids=WC.net_id)
def test_imid_layer_stages_at_head_sizes_32_and_64(net, pack, precision):
    """attn_f32_kernel / attn_f32_packed_kernel<32 | 64> on S = T = 6"""
    assert net in WC.NEW_NETS
    d, nhead = WC.d_model(net[0]), net[1]
    eng, _ = get_engine(d, False, nhead)
    try:
        eng.set_tuning("attn_pack", pack)
        both_layers(d, False, (2, 3, 4, 6), None, precision, {"masked": 0, "k8": 0, "attn_pack": pack}, nhead)
    finally:
        eng.set_tuning("attn_pack", 1)


@pytest.mark.parametrize("precision", MODES)
@pytest.mark.parametrize("pack", [1, 0])
@pytest.mark.parametrize("d", list(OLD_D))
def test_imid_layer_stages_stay_inside_their_bounds(d, pack, precision):
    """S = T = 6: the exact-fp32 attention kernel on short sequences, several per wave (attn_pack) or one"""
    eng, _ = get_engine(d, False)
    try:
        eng.set_tuning("attn_pack", pack)
        both_layers(d, False, (2, 3, 4, 6), None, precision, {"masked": 0, "k8": 0, "attn_pack": pack})
    finally:
        eng.set_tuning("attn_pack", 1)


# knob sets on the one-scene case: each is one more call of the same shape, so the batch kernels meet ragged tiles without a large batch
KNOBS = [({"small_lnx": 2}, ["f16mx"], {"out_proj_path": RB_GEMM_ADD_LN, "linear2_path": RB_GEMM_ADD_LN, "merge": 0}),
         ({"ln_fuse": 1, "ln_rows": 64}, SPLIT, {"out_proj_ln_rows": 64}),
         ({"ln_fuse": 1, "ln_rows": 128}, SPLIT, {"out_proj_ln_rows": 128}),
         ({"gemm_small": 1}, SPLIT, {"in_proj_shape": (5, 6, 7, 8), "linear1_shape": (5, 6, 7, 8)}),
         ({"attn_nsplit": 3, "small_cmb": 0}, SPLIT, {"attn_nsplit": 3}),
         ({"attn_nsplit": 3, "small_cmb": 2}, SPLIT, {"attn_nsplit": 3, "merge": 0}),
         ({"no_vt_direct": 1}, SPLIT, {"vt_direct": 0}),
         # (these two knobs belong to the 256 x 256 kernels a batch runs: alone they must leave the one scene's small launches as they
         #  are - asserted -, and forced onto the one scene, 1200 = 4 x 256 + 176 rows, they select the staged or the direct epilogues)
         ({"vt_stage": 2}, SPLIT, {"in_proj_shape": GS_SMALL, "linear1_shape": GS_SMALL}),
         ({"h1_stage": 2}, ["f16mx"], {"in_proj_shape": GS_SMALL, "linear1_shape": GS_SMALL, "out_proj_path": RB_LNX_SMALL}),
         ({"gemm_h_variant": 6}, SPLIT, {"in_proj_shape": GS_256x256, "linear1_shape": GS_256x256, "in_proj_vt_bits": 3}),
         ({"gemm_h_variant": 6, "vt_stage": 2}, SPLIT, {"in_proj_shape": GS_256x256, "in_proj_vt_bits": 0}),
         ({"gemm_h_variant": 6, "h1_stage": 2}, ["f16mx"], {"linear1_shape": GS_256x256, "linear1_h1_bit": 0}),
         ({"attn_h_variant": 1}, SPLIT, {"attn_dma": 0, "k8": 0}),
         ({"attn_mx": 2}, ["f16mx"], {"k8": 0, "q8l": 0})]
KNOB_CASES = [(k, p, e) for k, modes, e in KNOBS for p in modes]


def with_knobs(knobs, fn):
    eng, _ = get_engine(512, True)
    try:
        for name, value in knobs.items():
            eng.set_tuning(name, value)
        return fn()
    finally:
        for name in knobs:
            eng.set_tuning(name, 0)


@pytest.mark.parametrize("knobs,precision,expect", KNOB_CASES, ids=[",".join(f"{n}={v}" for n, v in k.items()) + "-" + p for k, p, _ in KNOB_CASES])
def test_one_scene_under_kernel_variant_knobs(knobs, precision, expect):
    e = dict(expect)
    if "ln_fuse" in knobs:
        e["out_proj_path"] = e["linear2_path"] = RB_GEMM_LN2 if precision == "f16mx" else RB_GEMM_LN
    with_knobs(knobs, lambda: both_layers(512, True, (1, 5, 20, 12), None, precision, e))


@pytest.mark.parametrize("precision", SPLIT)
@pytest.mark.parametrize("nsplit", [3, 12])
def test_masked_scenes_with_a_forced_split_kv_factor(nsplit, precision):
    """S = 384 = 12 key tiles: split ranges of four tiles and of one - a range may consist of all-zero mask words only"""
    with_knobs({"attn_nsplit": nsplit}, lambda: both_layers(512, True, (3, 4, 8, 12), [4, 1, 3], precision, {"attn_nsplit": nsplit, "masked": 1}))
