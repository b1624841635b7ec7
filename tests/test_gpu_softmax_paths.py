"""The reference-maximum paths of the attention softmax on the device: the cases of tests/softmax_cases.py through ``JmidEngine.dbg_layer`` -
the production operand path (OUT_QKV epilogue with the bf8 images and V^T, the mask words, split-KV and both merges) - on inputs loud enough
that the maximum MOVES: in tiles after the first, twice, in the ragged last tile, in part of a wave and in all of it, behind zero mask
words, in later split ranges, with an excess that wipes O and l.

Every stage still passes its unchanged bound and the TOL line (test_gpu_layer_stages.check_layer, every real row); the attention stage is
reported split into movers and non-movers by ``softmax_paths`` on the DEVICE's stage-1 planes, and the case's predicates are asserted on
those planes: a run in which the branch was not taken is a failed test, not a pass.  The plan says which kernel ran (expectation()), and the
rule follows from the plan: "thr14" with P as a truncated pair (F16X3), as one plane on fp16 logits (F16X2; F16MX under "attn_mx" = 2) and on
bf8 logits (F16MX), masked and not, merged by attn_combine_kernel and inside OUT_LNX; "lazy8" at heads 16, 32, 64 and - by knob - 128;
"strict" in F32.  tests/test_softmax_paths_host.py holds the emulation these figures stand next to."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import layer_reference as R  # noqa: E402
import softmax_cases as SC  # noqa: E402
import width_cases as WC  # noqa: E402
import test_gpu_layer_stages as LS  # noqa: E402

MODES = LS.MODES


def run_case(name, net, precision, expect, knobs=None):
    c = SC.CASES[name]
    shape, n_agents = c["shape"], c["n_agents"]
    E, A, K, T = shape
    S, nseq = K * A * T, E
    d, nhead = WC.d_model(net[0]), net[1]
    hd = d // nhead
    eng, _ = LS.get_engine(d, True, nhead)
    X = SC.loud_input(shape, n_agents, d, c["loud"])
    real = R.real_rows(n_agents, E, A, K, T)
    valid = R.key_valid(n_agents, E, A, K, T)
    failures = []
    for layer, last in ((1, False), (eng.dims.tf_layer - 1, True)):
        report = {}
        plan, stages = LS.check_layer(d, True, shape, n_agents, precision, layer, last, expect, nhead, X=X, report=report)
        rule = SC.launch_rule(precision, plan, knobs)
        ranges = SC.launch_ranges(precision, plan, S)
        if precision != "f32":
            assert plan["attn_dma"] == int(hd == 128 and (knobs or {}).get("attn_h_variant", 0) != 1)
        q, k = SC.head_planes(stages[1], nseq, S, nhead)
        P = SC.softmax_paths(q, k, valid, rule, ranges)
        tag = f"{name} w{net[0]}h{nhead} [{precision}] layer {layer} {knobs or ''} [{rule}, {len(ranges)} range(s), merge {plan['merge']}, masked {plan['masked']}, k8 {plan['k8']}]"
        if stages[2] is not None:
            ref, bound = report["attention"]
            got = stages[2][0].astype(np.float64) + stages[2][1].astype(np.float64)
            movers, others = SC.worst_by_path(np.abs(got - ref) / bound, P, hd, real)
            print(f"{tag} attention worst err/bound: movers {movers:.4f}, non-movers {others:.4f}")
        else:      # the merge rode in the out-projection's launch: stage 3 by rows, a row a mover when one of its heads moved
            ref, bound = report["norm1"]
            got = stages[3][0].astype(np.float64) + stages[3][1].astype(np.float64)
            row_moves = SC.mover_mask(P, hd).any(1)
            ratio = np.where(real[:, None], np.abs(got - ref) / bound, 0.0)
            print(f"{tag} norm1 (attention merged in its launch) worst err/bound: rows with a mover {ratio[row_moves].max():.4f}, without {ratio[~row_moves].max():.4f}")
        counts = SC.predicate_counts(P, real.reshape(nseq, S))
        names = SC.case_predicates(name, ranges)
        print(f"{tag} predicates {names}: " + ", ".join(f"{k_}={v:.3g}" for k_, v in counts.items()))
        failures += [(layer, f) for f in SC.failed_predicates(names, counts, rule)]
    assert not failures, failures


@pytest.mark.parametrize("precision", MODES)
@pytest.mark.parametrize("name,net", [(n, net) for n in SC.CASES for net in SC.NETS[n]], ids=lambda v: v if isinstance(v, str) else WC.net_id(v))
def test_the_reference_maximum_moves_and_every_stage_stays_inside_its_bound(name, net, precision):
    c = SC.CASES[name]
    d, nhead = WC.d_model(net[0]), net[1]
    run_case(name, net, precision, LS.expectation(c["shape"], c["n_agents"], d, precision, nhead))


KNOB_RUNS = [("scene", k, p, e) for k, modes, e in SC.SCENE_KNOBS for p in modes] + [("masked", k, p, e) for k, modes, e in SC.MASKED_KNOBS for p in modes]


@pytest.mark.parametrize("name,knobs,precision,expect", KNOB_RUNS, ids=[n + "-" + ",".join(f"{a}={b}" for a, b in k.items()) + "-" + p for n, k, p, _ in KNOB_RUNS])
def test_the_reference_maximum_moves_under_kernel_variant_knobs(name, knobs, precision, expect):
    """on the shipped width (256, 4): a forced split-KV factor with either merge, lazy8 at head 128 in the register-staged kernel and in the
    LDS-DMA kernel, thr14 on fp16 logits in F16MX; the masked form split in three (a range opens on a zero word) and in twelve"""
    LS.with_knobs(knobs, lambda: run_case(name, (256, 4), precision, expect, knobs))
