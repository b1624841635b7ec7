"""The reference-maximum paths of the attention softmax on loud inputs, without a GPU (tests/softmax_cases.py has the table):

* an emulated CORRECT kernel under each rule - "thr14" (the LDS-DMA kernel), "lazy8" (the register-staged kernels, and the DMA kernel under
  "attn_sm" = 2), "strict" (the exact-fp32 kernel) - stays inside the unchanged bound of layer_reference.attention_stage with P up to 2^14
  and 2^8: printed per case are the worst err / bound among movers and non-movers and the median / 99th percentile of bound / max|ref|;
* ``softmax_paths`` (float64) and the emulator's own record of moves agree on every decisive row, and every case meets its predicates on the
  emulated planes - and on float64 Q / K of every network and both layers the GPU test runs, so the table is pinned before a device sees it;
* eight emulated WRONG slow paths each leave the bound: six on the table's cases; the two that differ from the correct kernel only where
  every logit of a range's first tile, or of a whole row, lies below -126 (the guards of attn_f16x3.hpp:738-741 and :893) on hand-made
  stage-1 planes that get there, which rows of |c| <= 16 among 32 - 96 ordinary keys never do."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import layer_reference as R  # noqa: E402
import softmax_cases as SC  # noqa: E402
import test_layer_bounds_host as H  # noqa: E402
from safe_interactive_crowdnav_amd.weights import JMIDWeights, NetDims  # noqa: E402

MODES = H.MODES
# one scene at (256, 4): attn_pick_nsplit(10 q-tiles x 4 heads, 1200) = 6 (attn_f16x3.hpp:1005; the GPU test reads it from the plan)
SCENE_NSPLIT = 6


def runs():
    """(id, case, d_model, precision, knobs, nsplit): d_model 512 and 64 at nhead 4, the shapes of a case as test_layer_bounds_host.py runs them"""
    out = []
    for p in MODES:
        for d in (512, 64):
            out.append((f"stair-d{d}-{p}", "stair", d, p, {}, 1))
            for ns in ((1, 3, 12) if d == 512 and p != "f32" else (1,)):
                out.append((f"masked-d{d}-{p}-ns{ns}", "masked", d, p, {}, ns))
        out.append((f"scene-d512-{p}", "scene", 512, p, {}, SCENE_NSPLIT))
    for knobs, modes, _ in SC.SCENE_KNOBS:
        if "small_cmb" in knobs and knobs["small_cmb"]:
            continue      # (who merges is the device's business: the emulation has one merge)
        for p in modes:
            out.append((f"scene-d512-{p}-" + ",".join(f"{k}={v}" for k, v in knobs.items()), "scene", 512, p, knobs, knobs.get("attn_nsplit", SCENE_NSPLIT)))
    return out


RUNS = runs()
_L, _S1 = {}, {}


def emulated(run):
    """(Layer, path model on its stage-1 planes, rule, ranges) of a run - made once"""
    rid, name, d, precision, knobs, nsplit = run
    if rid not in _L:
        c = SC.CASES[name]
        E, A, K, T = c["shape"]
        over = {}
        if knobs.get("attn_h_variant") == 1:
            over = dict(attn_dma=0, k8=0, q8l=0)
        if knobs.get("attn_mx") == 2:
            over = dict(k8=0, q8l=0)
        plan = dict(H.host_plan(precision, True, d, E * A * K * T, c["n_agents"] is not None), attn_nsplit=nsplit, **over)
        rule = SC.launch_rule(precision, plan, knobs)
        ranges = SC.launch_ranges(precision, plan, K * A * T)
        X = SC.loud_input(c["shape"], c["n_agents"], d, c["loud"])
        key1 = (name, d, precision, plan["k8"], plan["q8l"])      # what stage 1 depends on: runs that differ in rule, ranges or P share it
        L = H.Layer(c["shape"], c["n_agents"], True, d, 4, precision, X=X, rule=rule, ranges=ranges, plan=over, upto=2, stage1=_S1.get(key1))
        _S1[key1] = (L.st[0], L.st[1], L.kern)
        q, k = SC.head_planes(L.st[1], L.nseq, L.S, 4)
        _L[rid] = (L, SC.softmax_paths(q, k, L.valid, rule, ranges), rule, ranges)
    return _L[rid]


@pytest.mark.parametrize("run", RUNS, ids=[r[0] for r in RUNS])
def test_an_emulated_correct_kernel_of_each_rule_stays_inside_the_attention_bound(run):
    L, P, rule, ranges = emulated(run)
    r = np.zeros((L.M, L.d))
    r[L.real] = L.ratio(2, L.st[2])
    assert np.isfinite(r).all()
    movers, others = SC.worst_by_path(r, P, L.hd, L.real)
    ref, bound = L.reference(2)
    rel = (bound / np.abs(ref[L.real]).max())[L.real]
    print(f"emulated {run[0]} [{rule}, {len(ranges)} range(s)] attention worst err/bound: movers {movers:.4f}, non-movers {others:.4f}; "
          f"bound / max|ref| median {np.median(rel):.2e}, 99th percentile {np.percentile(rel, 99):.2e}")
    assert max(movers, others) <= 1.0


@pytest.mark.parametrize("run", RUNS, ids=[r[0] for r in RUNS])
def test_the_path_model_agrees_with_the_emulator_and_the_case_meets_its_predicates(run):
    L, P, rule, ranges = emulated(run)
    sure = P["decisive"] & P["computed"] & ~P["first"]
    assert (P["moved"] == L.record["moved"])[sure].all(), "softmax_paths and the emulator disagree on a decisive row"
    assert not L.record["moved"][~P["computed"]].any()
    counts = SC.predicate_counts(P, L.real.reshape(L.nseq, L.S))
    names = SC.case_predicates(run[1], ranges)
    print(f"emulated {run[0]} [{rule}, {len(ranges)} range(s)] predicates {names}: " + ", ".join(f"{k}={v:.3g}" for k, v in counts.items()))
    assert not SC.failed_predicates(names, counts, rule)


def net_rules(head):
    """(rule, split factors) a network's launches of a case can take on the device"""
    return [("thr14", (1, 2, 3, 6, 12)), ("lazy8", (1, 6)), ("strict", (1,))] if head == 128 else [("lazy8", (1,)), ("strict", (1,))]


@pytest.mark.parametrize("name", list(SC.CASES))
def test_every_network_and_layer_meets_the_predicates_on_float64_planes(name):
    """Q, K = X W^T + b in float64, every network of the case, layer 1 and the last layer, every rule its kernels follow and every split
    factor a plan may name: the minimums hold with the device's roundings still to come (only decisive rows count)."""
    c = SC.CASES[name]
    E, A, K, T = c["shape"]
    S = K * A * T
    valid = R.key_valid(c["n_agents"], E, A, K, T)
    judged = R.real_rows(c["n_agents"], E, A, K, T).reshape(E, S)
    bad = []
    for ctx, nhead in SC.NETS[name]:
        dims = NetDims(ctx_dim=ctx, nhead=nhead)
        d = dims.d_model
        tensors = JMIDWeights.from_seed(dims, 5).tensors
        X = SC.loud_input(c["shape"], c["n_agents"], d, c["loud"]).astype(np.float64)
        for layer in (1, dims.tf_layer - 1):
            lw = R.layer_weights(tensors, layer)
            qkv = X @ lw["in_w"].T + lw["in_b"]
            q, k = SC.head_planes((qkv, np.zeros_like(qkv)), E, S, nhead)
            for rule, factors in net_rules(d // nhead):
                for ns in factors:
                    if ns > 1 and (name == "stair" or (name == "masked" and (rule != "thr14" or ns == 6))):
                        continue      # (S = 105 never splits; the masked form is the thr14 kernel's, split in 2, 3 or 12)
                    ranges = SC.key_ranges(S, ns)
                    counts = SC.predicate_counts(SC.softmax_paths(q, k, valid, rule, ranges), judged)
                    failed = SC.failed_predicates(SC.case_predicates(name, ranges), counts, rule)
                    if failed:
                        bad.append(((ctx, nhead), layer, rule, ns, failed))
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ wrong slow paths
TABLE_FAULTS = ("no_o_rescale", "no_l_rescale", "move_whole_wave", "half_sum", "stale_p", "merge_true_max")
GUARD_FAULTS = ("first_rescale", "masked_range_zero")
assert set(TABLE_FAULTS + GUARD_FAULTS) == set(H.SLOW_PATH_FAULTS)
LAZY8_FAULTS = ("no_o_rescale", "no_l_rescale")      # lazy8 has one pass and no threshold: the rescale is all that can go wrong in it


@pytest.mark.parametrize("precision", SC.SPLIT_MODES)
@pytest.mark.parametrize("fault", TABLE_FAULTS)
def test_an_emulated_wrong_slow_path_leaves_the_bound(fault, precision):
    targets = [] if fault == "merge_true_max" else [f"stair-d512-{precision}"]
    targets.append(f"scene-d512-{precision}")
    if fault in LAZY8_FAULTS:
        targets.append(f"stair-d64-{precision}")
    for rid in targets:
        L, P, rule, ranges = emulated(next(r for r in RUNS if r[0] == rid))
        with np.errstate(all="ignore"):
            r = L.ratio(2, L.attention(fault=fault))
        worst = float(np.where(np.isfinite(r), r, np.inf).max())
        print(f"{fault} {rid} [{rule}]: worst err/bound {worst:.3g}")
        assert worst > 1.0, (fault, rid, worst)


def guard_planes(precision, masked):
    """Hand-made stage-1 planes for the two guards of the thr14 kernel that the table's inputs never reach (they matter only where EVERY
    logit of a range's first computed tile, or of a whole row, lies below -126; rows of |c| <= 16 among ordinary keys do not get there):
    d_model 512, four heads, S = 64.  The 32 keys of tile 0 are -3.5 u_h + noise and every even query is +3.5 u_h + noise (u_h standard
    normal per head): those logits are -12.25 |u_h|^2 log2(e) / sqrt(128) = -200 +- 30 log2 units.  Odd queries and the keys of tile 1 are
    ordinary.  masked: tile 1 is padded agents' keys and the launch splits in two - the second range is fully masked and an even row's
    every valid logit lies below -126; not masked: one range, the first computed tile is the one below -128 and tile 1 lies 200 above it."""
    d, nhead, hd, S = 512, 4, 128, 64
    spec = R.stage_specs(precision, True, H.host_plan(precision, True, d, S, masked), last=False)
    qscale = R.LOG2E / np.sqrt(hd)
    rng = np.random.default_rng(4242)
    u = rng.standard_normal((1, nhead, hd))
    q, k, v = (rng.standard_normal((S, nhead, hd)) for _ in range(3))
    q[0::2] = 3.5 * u + 0.3 * q[0::2]
    k[:32] = -3.5 * u + 0.3 * k[:32]
    logits = np.einsum("ihc,jhc->hij", q[0::2], k[:32]) * qscale
    assert logits.max() < -130.0, logits.max()
    flat = lambda a: a.reshape(S, d).astype(np.float32)
    Q, K, V = (H.store(flat(a), rep) for a, rep in zip((q * qscale, k, v), spec["qkv_reps"]))
    read = tuple(np.concatenate([Q[i] / np.float32(qscale), K[i], V[i]], 1) for i in (0, 1))
    valid = np.ones((1, S), bool)
    valid[0, 32:] = not masked
    return spec, dict(Q=Q, K=K, V=V), read, valid, ([(0, 1), (1, 2)] if masked else [(0, 2)])


@pytest.mark.parametrize("precision", SC.SPLIT_MODES)
@pytest.mark.parametrize("fault", GUARD_FAULTS)
def test_the_first_tile_and_empty_range_guards_are_needed(fault, precision):
    """attn_f16x3.hpp:741 (no rescale from the placeholder 0 in a range's first computed tile: 2^-delta = inf on O = 0) and :893 (a range
    that computed no tile is (-inf, 0) to the merge, not (0, 0): the placeholder would become M and every weight 2^(m_i - 0) underflow):
    on planes that reach them the correct emulation stays inside the bound and the kernel without the guard leaves it."""
    spec, kern, read, valid, ranges = guard_planes(precision, masked=fault == "masked_range_zero")
    ref, bound, _ = R.attention_stage(*read, 1, 64, 4, valid, spec["logits"], spec["p_rep"], spec["v_lo"], spec["attn_out"], len(ranges))
    worst = {}
    for name, f in (("correct", None), (fault, fault)):
        with np.errstate(all="ignore"):
            hi, lo = H.emu_attention(kern, read, 1, 64, 4, valid, spec, rule="thr14", ranges=ranges, fault=f)
            r = np.abs(hi.astype(np.float64) + lo.astype(np.float64) - ref) / bound
        worst[name] = float(np.where(np.isfinite(r), r, np.inf).max())
    print(f"{fault} on hand-made planes [{precision}]: worst err/bound correct {worst['correct']:.4f}, without the guard {worst[fault]:.3g}")
    assert worst["correct"] <= 1.0 and worst[fault] > 1.0, worst
