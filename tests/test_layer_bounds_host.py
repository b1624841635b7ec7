"""The bounds of tests/layer_reference.py are neither impossible nor toothless (no GPU needed): a correct kernel, emulated in numpy
with the roundings the mode performs - operands rounded as the mode stores them, fp32 accumulation in k16 blocks,
outputs rounded to their planes -, stays inside every bound, and nine emulated WRONG kernels each push at least one element of a real
row over it, at every shape of tests/test_gpu_layer_stages.py where the fault can be expressed.

Inputs as on the device: X standard normal with row scales a fixed permutation of linspace(0.25, 4, M), the engine's seeded weights
of layer 1; the X rows of padded agents are 6 x a real row of the same episode, so a padded key that gets through carries softmax
weight of order 1."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import layer_reference as R  # noqa: E402
import width_cases as WC  # noqa: E402
from safe_interactive_crowdnav_amd.weights import JMIDWeights, NetDims

MODES = ["f32", "f16x3", "f16x2", "f16mx"]
# (E, A, K, T), n_agents, also at d_model 64, joint
SHAPES = [((1, 1, 1, 1), None, True, True), ((2, 2, 3, 4), None, True, True), ((3, 3, 5, 7), None, True, True),
          ((1, 5, 20, 12), None, False, True), ((1, 3, 100, 8), None, False, True), ((3, 4, 8, 12), [4, 1, 3], True, True),
          ((3, 3, 5, 6), [2, 3, 1], True, True), ((1, 4, 8, 12), [1], False, True), ((2, 3, 4, 6), None, True, False)]
OLD_D = tuple(sorted((WC.d_model(c) for c, _ in WC.OLD_NETS), reverse=True))      # d_model of the suite's two nhead = 4 networks
CASES = [(s, n, j, d, 4) for s, n, small, j in SHAPES for d in (OLD_D if small else OLD_D[:1])]
# rows of tests/width_cases.py with another head size (32, 64, and 64 at d_model 512), at the one shape with a partial row tile and S % 4 != 0
HEAD_NETS = [(96, 6), (128, 4), (256, 8)]
HEAD_CASES = [(((3, 3, 5, 7)), None, True, WC.d_model(c), h) for c, h in HEAD_NETS]
HEAD64_CASES = [c for c in HEAD_CASES if c[3] // c[4] == 64]
assert all(n in WC.NETS for n in HEAD_NETS) and len(HEAD64_CASES) == 2
_W = {}


def weights(d):
    if d not in _W:
        _W[d] = R.layer_weights(JMIDWeights.from_seed(NetDims(ctx_dim=d // 2), 5).tensors, 1)
    return _W[d]


make_x = R.layer_input


def host_plan(precision, joint, d, M, masked, nhead=4):
    """What launch_plan.hpp decides for the arithmetic of the layer's GEMMs (plan_gemm: F16MX where K % 64 == 0 and N % 128 == 0) and
    jmid_planner.hip plan_step for the images and planes - the words of jmid_dbg_layer's plan that layer_reference.stage_specs reads."""
    ff = 2 * d
    code = {"f32": -1, "f16x3": 0, "f16x2": 1, "f16mx": 2}[precision]
    mode = lambda N, K: 1 if code == 2 and not (K % 64 == 0 and N % 128 == 0) else code
    hd128 = d // nhead == 128
    k8 = int(joint and precision == "f16mx" and hd128)
    return dict(in_proj_mode=mode(3 * d, d), linear1_mode=mode(ff, d), out_proj_mode=mode(d, d), linear2_mode=mode(d, ff),
                k8=k8, q8l=k8, byte_lo=int(precision == "f16mx" and d == 512), attn_dma=int(hd128), masked=int(masked and joint))


# ------------------------------------------------------------------------------------------------ emulated kernels
def emu_gemm(A_hi, A_lo, W, b, arith, drop_k32_row=None):
    """fp32 result of A . W^T + b as the mode's K loop forms it: one fp32 accumulator, every MFMA's contribution (a k16 block of one
    operand pair; the fp8 term a k64 block) rounded to fp32 as it is added.  drop_k32_row: that row loses its last k32 block."""
    A_hi, A_lo = np.array(A_hi, np.float32), np.array(A_lo, np.float32)
    K = A_hi.shape[1]
    if drop_k32_row is not None:
        A_hi[drop_k32_row, K - 32:] = 0
        A_lo[drop_k32_row, K - 32:] = 0
    W32 = W.astype(np.float32)
    if arith == "f32":
        pairs, scale, w8, a8 = [(A_hi + A_lo, W32)], np.float32(1), None, None
    else:
        Wh, Wl = R.split16(W32 * np.float32(R.KW))
        scale = np.float32(1 / R.KW)
        pairs = {"x3": [(A_hi, Wh), (A_hi, Wl), (A_lo, Wh)], "x2": [(A_hi, Wh), (A_hi, Wl)], "mx": [(A_hi, Wh)]}[arith]
        w8, a8 = (R.bf8(Wl), R.bf8(A_hi)) if arith == "mx" else (None, None)
    acc = np.zeros((A_hi.shape[0], W.shape[0]), np.float32)
    for k0 in range(0, K, 16):
        for a, w in pairs:
            acc = acc + a[:, k0:k0 + 16] @ w[:, k0:k0 + 16].T            # (fp32 throughout: the block's own sum rounds as well)
        if w8 is not None and (k0 + 16) % 64 == 0:
            acc = acc + a8[:, k0 - 48:k0 + 16] @ w8[:, k0 - 48:k0 + 16].T
    return acc * scale + b.astype(np.float32)


def store(v, rep):
    """fp32 values -> the planes of a representation, as read back"""
    v = np.asarray(v, np.float32)
    if rep == "f32":
        return v, np.zeros_like(v)
    hi, lo = R.split16(v)
    if rep == "hi":
        lo = np.zeros_like(v)
    elif rep == "hi_bf8":
        lo = R.bf8(lo)
    return hi, lo


def emu_qkv(X, W, b, spec, qscale, joint_split, **mut):
    """stage 1: (planes as read back, the planes the attention kernel holds: Q pre-scaled, and the bf8 image of K_hi)"""
    acc = emu_gemm(X[0], X[1], W, b, spec["in_proj"], mut.get("drop_k32_row"))
    d = acc.shape[1] // 3
    q, k, v = acc[:, :d], acc[:, d:2 * d], acc[:, 2 * d:]
    if not joint_split:
        z = np.zeros_like(acc)
        return (acc, z), None
    qs = q * np.float32(qscale)
    if "double_scale_head" in mut:
        h, hd = mut["double_scale_head"]
        qs[:, h * hd:(h + 1) * hd] *= np.float32(qscale)
    Q, Kp, V = store(qs, spec["qkv_reps"][0]), store(k, spec["qkv_reps"][1]), store(v, spec["qkv_reps"][2])
    read_hi = np.concatenate([Q[0] / np.float32(qscale), Kp[0], V[0]], 1)
    read_lo = np.concatenate([Q[1] / np.float32(qscale), Kp[1], V[1]], 1)
    return (read_hi, read_lo), dict(Q=Q, K=Kp, V=V)


def emu_lazy_tile(rule, spec, s, m, l, o, vh, vl, first, fault):
    """One key tile under a lazy rule: s [S, keys] fp32 logits (thr14: already minus m - the accumulator started there), the state
    m, l [S, 1], o [S, hd] -> (m, l, o, moved [S, 1]).  first: the range's first computed tile."""
    f32 = np.float32

    def form(x):
        with np.errstate(over="ignore"):
            p = np.exp2(x).astype(f32)
            if spec["p_rep"] == "p1":      # the packed fp16 P, and the row sum of exactly those values (dot2_ones)
                ph = R.f16(p)
                return p, ph, None, ph.sum(1, keepdims=True, dtype=f32)
            if spec["p_rep"] == "split":
                ph = R.f16_rtz(p)
                return p, ph, R.f16_rtz(p - ph), p.sum(1, keepdims=True, dtype=f32)
            return p, p, None, p.sum(1, keepdims=True, dtype=f32)

    def pv(o, ph, pl):
        o = o + ph @ vh
        if pl is not None:
            o = o + pl @ vh
        if spec["v_lo"] and spec["p_rep"] != "f32":
            o = o + ph @ vl
        return o

    with np.errstate(all="ignore"):
        tmax = s.max(1, keepdims=True)
        if rule == "lazy8":
            m_new = np.where(tmax > m + f32(8), tmax, m).astype(f32)
            alpha = np.exp2(m - m_new).astype(f32)
            moved = (m_new != m) & (not first)
            p, ph, pl, _ = form(s - m_new)
            psum = p.sum(1, keepdims=True, dtype=f32)      # (:209, :776-783: the fp32 row sum, also where P enters P . V as one fp16 plane)
            l = (l if fault == "no_l_rescale" else l * alpha) + psum
            o = pv(o if fault == "no_o_rescale" else o * alpha, ph, pl)
            return m_new, l, o, moved
        trip = np.ones_like(m, bool)
        if not first:
            p, ph, pl, psum = form(s)
            tested = psum
            if fault == "half_sum":        # lane half 0 holds keys frag_row(r, 0) = (r & 3) + 8 (r >> 2): its sum alone
                mine = (np.arange(s.shape[1]) % 8) < 4
                tested = (p if pl is not None or spec["p_rep"] == "f32" else ph)[:, mine].sum(1, keepdims=True, dtype=f32)
            trip = ~(tested <= f32(16384.0))
        if first or trip.any():
            delta = np.where(trip, tmax, f32(0)).astype(f32)
            if fault == "move_whole_wave" and not first:      # delta = tmax for every row of a wave (32 queries) one of whose rows tripped
                for w0 in range(0, len(trip), 32):
                    if trip[w0:w0 + 32].any():
                        delta[w0:w0 + 32] = tmax[w0:w0 + 32]
            if not first or fault == "first_rescale":
                alpha = np.exp2(-delta).astype(f32)
                if fault != "no_o_rescale":
                    o = o * alpha
                if fault != "no_l_rescale":
                    l = l * alpha
            m = (m + delta).astype(f32)
            if first or fault != "stale_p":
                _, ph, pl, psum = form(s - delta)
        return m, l + psum, pv(o, ph, pl), trip & (not first)


SLOW_PATH_FAULTS = ("no_o_rescale", "no_l_rescale", "move_whole_wave", "half_sum", "stale_p", "first_rescale", "merge_true_max",
                    "masked_range_zero")


def emu_attention(kern, read, nseq, S, nhead, valid, spec, nsplit=1, admit=None, drop_range=None, shift_last_v=False, rule="strict",
                  ranges=None, record=None, fault=None):
    """stage 2 in fp32: 32-key tiles, online softmax in log2 units on the pre-scaled Q, P rounded as the mode stores it, O and l summed
    tile by tile, split-KV ranges merged.  admit = (first query, last query, seq, key): those queries see that masked key;
    drop_range: the keys of one split-KV range never arrive; shift_last_v: V^T of the last key is read one column on.
    rule: how the reference maximum moves (tests/softmax_cases.py) - "strict" m = max(m, tile maximum); "lazy8" attn_f16x3.hpp:203 only
    past m + 8; "thr14" attn_f16x3.hpp:694-754: the logits accumulate onto -m, P is formed optimistically, the row sum of the P actually used
    (the packed fp16 sum in "p1") says which rows move, O and l of those take 2^-delta, P is formed again; a range's first computed
    tile sets m from the placeholder 0 without a rescale; a zero mask word is skipped.  ranges: [begin tile, end tile) per split-KV
    range (default: the nsplit equal parts this file always used).  record: a dict that receives "moved" [nseq, nhead, S, tiles] and
    "first".  fault: one of SLOW_PATH_FAULTS, a wrong slow path / merge."""
    assert rule in ("strict", "lazy8", "thr14") and (fault is None or fault in SLOW_PATH_FAULTS)
    lazy = rule != "strict"
    ntile = (S + 31) // 32
    if record is not None:
        record["moved"] = np.zeros((nseq, nhead, S, ntile), bool)
        record["first"] = np.zeros((nseq, nhead, S, ntile), bool)
    f32 = np.float32
    M = nseq * S
    if kern is None:           # fp32 Q, K, V (F32; iMID)
        d = read[0].shape[1] // 3
        hd = d // nhead
        qf = read[0][:, :d] * f32(1 / np.sqrt(hd) * R.LOG2E)
        Q, K, V = (qf, 0 * qf), (read[0][:, d:2 * d], 0 * qf), (read[0][:, 2 * d:], 0 * qf)
    else:
        Q, K, V = kern["Q"], kern["K"], kern["V"]
        d = Q[0].shape[1]
        hd = d // nhead
    k8h = R.bf8(K[0]) if spec["logits"] == "bf8" else None
    q8h = R.bf8(Q[0]) if spec["logits"] == "bf8" else None
    out = np.zeros((M, d), f32)
    head = lambda a, n, h: a[n * S:(n + 1) * S, h * hd:(h + 1) * hd]
    for n in range(nseq):
        for h in range(nhead):
            qh, ql, kh, kl = (np.ascontiguousarray(head(a, n, h), f32) for a in (Q[0], Q[1], K[0], K[1]))
            vh, vl = np.ascontiguousarray(head(V[0], n, h), f32), np.ascontiguousarray(head(V[1], n, h), f32)
            if shift_last_v:
                vh, vl = vh.copy(), vl.copy()
                vh[S - 1], vl[S - 1] = np.roll(vh[S - 1], -1), np.roll(vl[S - 1], -1)
            ok = np.broadcast_to(valid[n][None, :], (S, S)).copy()
            if admit is not None and admit[2] == n:
                ok[admit[0]:admit[1], admit[3]] = True
            bounds = np.linspace(0, (S + 31) // 32, nsplit + 1).astype(int) * 32
            spans = [(bounds[sp], bounds[sp + 1]) for sp in range(nsplit)] if ranges is None else [(32 * a, 32 * b) for a, b in ranges]
            parts, tops = [], []
            for sp, (k_lo, k_hi) in enumerate(spans):
                m = np.full((S, 1), 0.0 if rule == "thr14" else -np.inf, f32)
                l = np.zeros((S, 1), f32)
                o = np.zeros((S, hd), f32)
                seen = False
                true_max = np.full((S, 1), -np.inf, f32)
                for k0 in range(k_lo, min(k_hi, S), 32):
                    if drop_range is not None and drop_range == sp:
                        continue
                    ks = slice(k0, min(k0 + 32, S))
                    if lazy and not ok[:, ks].any():          # a zero mask word: the tile is skipped whole
                        continue
                    s = np.zeros((S, ks.stop - k0), f32) if rule != "thr14" else np.repeat(-m, ks.stop - k0, 1)
                    for c0 in range(0, hd, 16):
                        cs = slice(c0, c0 + 16)
                        s = s + qh[:, cs] @ kh[ks, cs].T
                        if spec["logits"] == "f16":
                            s = s + ql[:, cs] @ kh[ks, cs].T
                            s = s + qh[:, cs] @ kl[ks, cs].T
                    if spec["logits"] == "bf8":
                        for c0 in range(0, hd, 64):
                            cs = slice(c0, c0 + 64)
                            s = s + ql[:, cs] @ head(k8h, n, h)[ks, cs].T
                            s = s + head(q8h, n, h)[:, cs] @ kl[ks, cs].T
                    s = np.where(ok[:, ks], s, f32(-np.inf))
                    if lazy:
                        true_max = np.maximum(true_max, s.max(1, keepdims=True) + (m if rule == "thr14" else f32(0)))
                        first = not seen
                        m, l, o, moved = emu_lazy_tile(rule, spec, s, m, l, o, vh[ks], vl[ks], first, fault)
                        seen = True
                        if record is not None:
                            record["moved"][n, h, :, k0 // 32] = moved[:, 0]
                            record["first"][n, h, :, k0 // 32] = first
                        continue
                    m_new = np.maximum(m, s.max(1, keepdims=True))
                    if record is not None:
                        record["moved"][n, h, :, k0 // 32] = (np.isfinite(m) & (m_new > m))[:, 0]
                    safe = np.where(np.isfinite(m_new), m_new, f32(0))
                    alpha = np.where(np.isfinite(m), np.exp2(m - safe), f32(0)).astype(f32)
                    p = np.exp2(s - safe).astype(f32)
                    if spec["p_rep"] == "p1":
                        ph, pl = R.f16(p), None
                        psum = ph.sum(1, keepdims=True, dtype=f32)
                    elif spec["p_rep"] == "split":
                        ph = R.f16_rtz(p)
                        pl = R.f16_rtz(p - ph)
                        psum = p.sum(1, keepdims=True, dtype=f32)
                    else:
                        ph, pl = p, None
                        psum = p.sum(1, keepdims=True, dtype=f32)
                    l = l * alpha + psum
                    o = o * alpha
                    o = o + ph @ vh[ks]
                    if pl is not None:
                        o = o + pl @ vh[ks]
                    if spec["v_lo"] and spec["p_rep"] != "f32":
                        o = o + ph @ vl[ks]
                    m = m_new
                if lazy and not seen:      # the range computed no tile: (-inf, 0) to the merge, attn_f16x3.hpp:893
                    m = np.full((S, 1), 0.0 if fault == "masked_range_zero" else -np.inf, f32)
                parts.append((m, l, o))
                tops.append(true_max)
            if len(parts) == 1:
                m, l, o = parts[0]
            else:
                mm = np.max([p_[0] for p_ in parts], 0)
                ws = [np.where(np.isfinite(p_[0]), np.exp2(p_[0] - mm), f32(0)).astype(f32) for p_ in parts]
                if fault == "merge_true_max":      # the weights from the ranges' true maxima: O_i and l_i stand on the lazy m_i
                    with np.errstate(invalid="ignore"):
                        ws = [np.where(np.isfinite(t_), np.exp2(t_ - np.max(tops, 0)), f32(0)).astype(f32) for t_ in tops]
                l = sum(w * p_[1] for w, p_ in zip(ws, parts))
                o = sum(w * p_[2] for w, p_ in zip(ws, parts))
            out[n * S:(n + 1) * S, h * hd:(h + 1) * hd] = o * (f32(1) / l)
    return store(out, spec["attn_out"])


def emu_ln(X, A, W, b, gamma, beta, arith, rep, skip_mean_col=None, **mut):
    """X <- LayerNorm(X + A . W^T + b) in fp32 as add_ln_kernel does it (two-pass variance)."""
    f32 = np.float32
    y = emu_gemm(A[0], A[1], W, b, arith, mut.get("drop_k32_row"))
    v = (np.asarray(X[0], f32) + np.asarray(X[1], f32)) + y
    d = v.shape[1]
    s = v.sum(1, keepdims=True, dtype=f32)
    if skip_mean_col is not None:
        s = s - v[:, skip_mean_col:skip_mean_col + 1]
    mean = s / f32(d)
    t = v - mean
    rstd = (f32(1) / np.sqrt((t * t).sum(1, keepdims=True, dtype=f32) / f32(d) + f32(R.EPS))).astype(f32)
    return store(t * rstd * gamma.astype(f32) + beta.astype(f32), rep)


def emu_linear1(X, W, b, arith, rep, no_relu_cols=None, **mut):
    acc = emu_gemm(X[0], X[1], W, b, arith, mut.get("drop_k32_row"))
    out = np.maximum(acc, 0)
    if no_relu_cols is not None:
        out[:, no_relu_cols] = acc[:, no_relu_cols]
    return store(out, rep)


# ------------------------------------------------------------------------------------------------ one layer, stage by stage
class Layer:
    """The emulated correct layer of one case and mode, every stage fed the emulated output of the stage before it, with the reference
    and bound of every stage - made once, shared by the correct-kernel test and the mutations."""

    def __init__(self, shape, n_agents, joint, d, nhead, precision, X=None, rule="strict", ranges=None, plan=None, upto=5, stage1=None):
        """X: another input than the case's layer_input; rule, ranges: emu_attention's; plan: words of host_plan to replace (a knob);
        upto = 2: the stages after attention are not made (tests/test_softmax_paths_host.py judges attention alone); stage1: (st[0],
        st[1], kern) of another Layer with the same input, mode and Q / K / V representations - the in_proj emulation is not repeated"""
        E, A, K, T = shape
        self.shape, self.n_agents, self.joint, self.d, self.precision = shape, n_agents, joint, d, precision
        self.M, self.nhead, self.hd = E * A * K * T, nhead, d // nhead
        self.nseq, self.S = (E, K * A * T) if joint else (E * K * A, T)
        self.w = weights(d)
        self.real = R.real_rows(n_agents, E, A, K, T)
        self.valid = R.key_valid(n_agents, E, A, K, T) if joint else np.ones((self.nseq, self.S), bool)
        self.plan = dict(host_plan(precision, joint, d, self.M, n_agents is not None, nhead), **(plan or {}))
        self.rule, self.ranges, self.record = rule, ranges, {}
        self.spec = R.stage_specs(precision, joint, self.plan, last=False)
        self.qscale = R.LOG2E / np.sqrt(self.hd)
        self.split_joint = joint and precision != "f32"
        self.nsplit = 3 if (joint and precision != "f32" and self.hd == 128 and self.S >= 192) else 1
        if ranges is not None:
            self.nsplit = len(ranges)
        w, sp = self.w, self.spec
        self.st = {0: store(make_x(shape, n_agents, d) if X is None else X, "f32" if precision == "f32" else sp["x_rep"])}
        if stage1 is not None:
            self.st[0], self.st[1], self.kern = stage1
        else:
            self.st[1], self.kern = self.qkv()
        self.st[2] = self.attention(record=self.record)
        self.ref = {}
        if upto <= 2:
            return
        self.st[3] = emu_ln(self.st[0], self.st[2], w["out_w"], w["out_b"], w["n1_g"], w["n1_b"], sp["out_proj"], sp["x_rep"])
        self.st[4] = emu_linear1(self.st[3], w["l1_w"], w["l1_b"], sp["linear1"], sp["h1_rep"])
        self.st[5] = emu_ln(self.st[3], self.st[4], w["l2_w"], w["l2_b"], w["n2_g"], w["n2_b"], sp["linear2"], sp["x_last_rep"])
        # ... and norm2 as the encoder's last layer runs it (no_lo_out: one plane where nothing reads the other)
        self.last_rep = R.stage_specs(precision, joint, self.plan, last=True)["x_last_rep"]
        self.st["5 last"] = emu_ln(self.st[3], self.st[4], w["l2_w"], w["l2_b"], w["n2_g"], w["n2_b"], sp["linear2"], self.last_rep)
        self.ref = {}

    def qkv(self, **mut):
        return emu_qkv(self.st[0], self.w["in_w"], self.w["in_b"], self.spec, self.qscale, self.split_joint, **mut)

    def attention(self, kern=None, read=None, **mut):
        return emu_attention(self.kern if kern is None else kern, self.st[1] if read is None else read, self.nseq, self.S, self.nhead,
                             self.valid, self.spec, nsplit=mut.pop("nsplit", self.nsplit), rule=self.rule, ranges=self.ranges, **mut)

    def reference(self, s):
        """(ref, bound) of stage s from the emulated planes of the stage(s) before it"""
        if s not in self.ref:
            w, sp, st = self.w, self.spec, self.st
            if s == 1:
                r = R.qkv_stage(*st[0], w["in_w"], w["in_b"], sp["in_proj"], sp["qkv_reps"], self.qscale)
            elif s == 2:
                r = R.attention_stage(*st[1], self.nseq, self.S, self.nhead, self.valid, sp["logits"], sp["p_rep"], sp["v_lo"], sp["attn_out"],
                                      self.nsplit)
            elif s == 3:
                r = R.ln_stage(*st[0], *st[2], w["out_w"], w["out_b"], w["n1_g"], w["n1_b"], sp["out_proj"], sp["x_rep"])
            elif s == 4:
                r = R.gemm_stage(*st[3], w["l1_w"], w["l1_b"], sp["linear1"], True, sp["h1_rep"])
            else:
                r = R.ln_stage(*st[3], *st[4], w["l2_w"], w["l2_b"], w["n2_g"], w["n2_b"], sp["linear2"],
                               self.last_rep if s == "5 last" else sp["x_last_rep"])
            self.ref[s] = r[:2]
        return self.ref[s]

    def ratio(self, s, planes):
        ref, bound = self.reference(s)
        got = planes[0].astype(np.float64) + planes[1].astype(np.float64)
        return (np.abs(got - ref) / bound)[self.real]


_LAYERS = {}


def layer(case, precision):
    key = (str(case), precision)
    if key not in _LAYERS:
        _LAYERS[key] = Layer(*case, precision)
    return _LAYERS[key]


def case_id(c):
    (E, A, K, T), n, joint, d, nhead = c
    return f"{'jmid' if joint else 'imid'}-{E}x{A}x{K}x{T}-{'pad' if n else 'full'}-d{d}" + ("" if nhead == 4 else f"-h{nhead}")


@pytest.mark.parametrize("case,precision", [(c, p) for p in MODES for c in CASES + HEAD_CASES], ids=lambda v: v if isinstance(v, str) else case_id(v))
def test_an_emulated_correct_kernel_stays_inside_every_bound(case, precision):
    L = layer(case, precision)
    worst = {}
    for s in (1, 2, 3, 4, 5, "5 last"):
        r = L.ratio(s, L.st[s])
        assert np.isfinite(r).all()
        worst[s] = float(r.max())
    print(f"emulated {case_id(case)} [{precision}] worst err/bound per stage: " + ", ".join(f"{s}: {v:.4f}" for s, v in worst.items()))
    assert max(worst.values()) <= 1.0, worst


# ------------------------------------------------------------------------------------------------ mutations
def over(L, s, planes):
    r = L.ratio(s, planes)
    return float(r.max())


class NotDetectable(float):
    """the worst err / bound of a fault the bounds cannot be asked to catch: printed, not asserted"""


def mut_lost_k32(L):
    """one row of a ragged last tile loses its last k32 block (in_proj, and linear2 with K = d_ff)"""
    row = int(np.flatnonzero(L.real)[-1])
    a = over(L, 1, L.qkv(drop_k32_row=row)[0])
    w, sp = L.w, L.spec
    b = over(L, 5, emu_ln(L.st[3], L.st[4], w["l2_w"], w["l2_b"], w["n2_g"], w["n2_b"], sp["linear2"], sp["x_last_rep"], drop_k32_row=row))
    return min(a, b)


def mut_padded_key(L):
    """one 128-row query block admits one padded key"""
    if L.n_agents is None or not L.joint or L.valid.all():
        return None
    n = int(np.flatnonzero(~L.valid.all(1))[0])
    key = int(np.flatnonzero(~L.valid[n])[0])
    return over(L, 2, L.attention(admit=(0, min(128, L.S), n, key)))


def mut_dropped_range(L):
    """one split-KV range is dropped"""
    if L.nsplit == 1:
        return None
    return over(L, 2, L.attention(drop_range=L.nsplit - 1))


def mut_shifted_vt(L):
    """V^T of the last key shifted by one column when S % 4 != 0"""
    if L.S % 4 == 0 or not L.joint:
        return None
    return over(L, 2, L.attention(shift_last_v=True))


def mut_mean_column(L):
    """one column (the last) left out of the rows' mean"""
    w, sp = L.w, L.spec
    return over(L, 3, emu_ln(L.st[0], L.st[2], w["out_w"], w["out_b"], w["n1_g"], w["n1_b"], sp["out_proj"], sp["x_rep"],
                             skip_mean_col=L.d - 1))


def mut_no_relu(L):
    """ReLU not applied in the last 64-column tile"""
    w, sp = L.w, L.spec
    return over(L, 4, emu_linear1(L.st[3], w["l1_w"], w["l1_b"], sp["linear1"], sp["h1_rep"], no_relu_cols=slice(2 * L.d - 64, 2 * L.d)))


def mut_double_scale(L):
    """Q's scale applied twice in one head"""
    if not L.split_joint:
        return None
    return over(L, 1, L.qkv(double_scale_head=(L.nhead - 1, L.hd))[0])


def mut_zero_lo(L):
    """output lo plane zeroed in one tile (the residual stream after norm1).  Detected where that plane is an fp16 plane (F16X3, F16X2,
    F16MX at d_model 64).  Where it is the byte plane (F16MX at d_model 512) the fault is expressible but NOT reliably detectable: the
    plane is worth 2^-12 of the value, less than the 2^-13 |A| |W| of the mode's bf8 correction terms that the bound has to allow -
    below what a float64 comparison of one stage can see.  There the ratio is printed and nothing is asserted (NotDetectable); bit
    equality with the unfused pair (tests/test_gpu_kernels.py) is what holds that plane.  F32 has no lo plane."""
    if L.spec["x_rep"] == "f32":
        return None
    hi, lo = L.st[3]
    lo = lo.copy()
    rows = np.flatnonzero(L.real)[:64]
    lo[rows[:, None], np.arange(min(64, L.d))[None, :]] = 0
    r = over(L, 3, (hi, lo))
    return r if L.spec["x_rep"] == "pair" else NotDetectable(r)


def mut_swapped_rows(L):
    """rows m and m + 64 swapped"""
    rows = np.flatnonzero(L.real)
    if len(rows) < 2:
        return None
    m, m2 = (int(rows[0]), int(rows[0]) + 64) if L.M > 64 and L.real[int(rows[0]) + 64] else (int(rows[0]), int(rows[1]))
    hi, lo = (a.copy() for a in L.st[4])
    for a in (hi, lo):
        a[[m, m2]] = a[[m2, m]]
    return over(L, 4, (hi, lo))


MUTATIONS = [mut_lost_k32, mut_padded_key, mut_dropped_range, mut_shifted_vt, mut_mean_column, mut_no_relu, mut_double_scale, mut_zero_lo,
             mut_swapped_rows]


@pytest.mark.parametrize("precision", MODES)
@pytest.mark.parametrize("mutation", MUTATIONS, ids=lambda f: f.__name__[4:])
def test_an_emulated_wrong_kernel_leaves_its_bound(mutation, precision):
    """at every shape where the fault is expressible (None: it is not - no mask, no split, S % 4 == 0, no lo plane, one row)"""
    seen = 0
    for case in CASES:
        r = mutation(layer(case, precision))
        if r is None:
            continue
        print(f"{mutation.__name__[4:]} {case_id(case)} [{precision}]: worst err/bound {r:.3g}" + (" (not asserted)" if isinstance(r, NotDetectable) else ""))
        if isinstance(r, NotDetectable):
            continue
        seen += 1
        assert r > 1.0, (mutation.__name__, case_id(case), precision, r)
    # (F32 has no pre-scaled Q planes, no lo plane and no split-KV launch)
    if not (precision == "f32" and mutation in (mut_double_scale, mut_zero_lo, mut_dropped_range)):
        assert seen > 0, "the mutation was never expressible"


# (no padded scene and no split-KV launch among the head-64 cases: head 64's launches never split - plan_call - and the masked shapes
#  are the GPU test's)
HEAD64_MUTATIONS = [m for m in MUTATIONS if m not in (mut_padded_key, mut_dropped_range)]


@pytest.mark.parametrize("precision", MODES)
@pytest.mark.parametrize("mutation", HEAD64_MUTATIONS, ids=lambda f: f.__name__[4:])
def test_an_emulated_wrong_kernel_leaves_its_bound_at_head_size_64(mutation, precision):
    """the same faults at head 64 (d_model 256 with four heads, d_model 512 with eight): the bounds bite there before a device result
    is judged by them"""
    seen = 0
    for case in HEAD64_CASES:
        r = mutation(layer(case, precision))
        if r is None:
            continue
        print(f"{mutation.__name__[4:]} {case_id(case)} [{precision}]: worst err/bound {r:.3g}" + (" (not asserted)" if isinstance(r, NotDetectable) else ""))
        if isinstance(r, NotDetectable):
            continue
        seen += 1
        assert r > 1.0, (mutation.__name__, case_id(case), precision, r)
    if not (precision == "f32" and mutation in (mut_double_scale, mut_zero_lo)):
        assert seen > 0, "the mutation was never expressible"
