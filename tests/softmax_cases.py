"""The inputs, the path model and the predicates of the attention softmax's reference-maximum tests (tests/test_softmax_paths_host.py,
tests/test_gpu_softmax_paths.py): the one table both take their lists from.

Three rules move the reference maximum m of the online softmax (paths relative to safe-interactive-crowdnav_amd/csrc):

* ``thr14``  attn_f16x3.hpp attn_f16x3_dma_kernel, SM = 1 (:694-754): P = 2^(s - m) is formed optimistically; only when a row's tile sum
  exceeds ATT_SM_THR = 2^14 (or is not finite) m moves to the tile maximum, O and l are rescaled and P is formed again.  A wave's first
  COMPUTED tile (masked form: the first non-zero mask word of its key range) sets m without a rescale.
* ``lazy8``  attn_f16x3_kernel<16 | 32 | 64 | 128> (:192-213) and the DMA kernel under "attn_sm" = 2: m moves when the tile maximum exceeds
  it by more than ATT_LAZY_TAU = 8.
* ``strict`` attn_f32.hpp:119: m = max(m, tile maximum).

The seeded weights give logits of 2.7 log2 units standard deviation: m almost never moves after the first tile.  ``loud_input`` makes a
few token rows loud, so that their K rows sit far above (for about half of the queries) or far below the reference maximum, and
``softmax_paths`` says in float64 which (sequence, head, query row, tile) takes which branch - the predicates below are conditions a case
must meet on the planes it actually ran on, device or emulated, before its result counts as a test of that branch."""
import warnings

import numpy as np

import layer_reference as R
import width_cases as WC

RULES = ("thr14", "lazy8", "strict")
THR14 = 2.0 ** 14          # ATT_SM_THR
TAU8 = 8.0                 # ATT_LAZY_TAU
WIPE = 126.0               # 2^-delta leaves the normal fp32 range: O and l are wiped by the rescale
DEAD_P = 2.0 ** -24        # every P of a tile below half the fp16 subnormal step: the tile adds nothing
# strict's rule has no band of its own: a "small" move is one neither lazy rule would have made at its threshold (excess <= 8)
SMALL_EXCESS = {"thr14": (14.0, 20.0), "lazy8": (8.0, 12.0), "strict": (0.0, 8.0)}
HIGH_P = {"thr14": (2.0 ** 9, 2.0 ** 14), "lazy8": (2.0 ** 4, 2.0 ** 8)}
STRICT_EPS = 2.0 ** -10    # strict: |tile max - m| above the fp32 logits' own rounding (|s| < 2^10, 2^-24 relative, sqrt(hd) terms)


# ------------------------------------------------------------------------------------------------ inputs
LOUD_SEED = 77000


def loud_input(shape, n_agents, d, loud, seed=LOUD_SEED):
    """layer_reference.layer_input with the rows of loud = [(row, c), ...] replaced by c x a standard-normal row (fixed seed).  The rows
    must be real agents' rows - valid as keys, judged as queries - and |c| <= 16 (max |Q|K|V| 36 at d_model 512, 51 in the masked case,
    whose padded rows are 6 x a real row: far inside fp16, and check_layer asserts range_flag == 0 on the device).
    An entry (row, c, "u") takes c x ONE standard-normal row u shared by all such entries of the case: the logit of an aligned query on
    an aligned key is c_q c_k g_h with one g_h per head, so 32 consecutive aligned queries all see an aligned key of the right sign
    above their reference maximum - random directions never make all rows of a wave move in one tile (each row's sign is a coin)."""
    X = R.layer_input(shape, n_agents, d).copy()
    E, A, K, T = shape
    real = R.real_rows(n_agents, E, A, K, T)
    rng = np.random.default_rng(seed + d)
    u = rng.standard_normal(d)
    for row, c, *shared in loud:
        assert real[row] and 0 < abs(c) <= 16, (row, c)
        X[row] = (c * (u if shared else rng.standard_normal(d))).astype(np.float32)
    return X


# ------------------------------------------------------------------------------------------------ the launch's key ranges
def key_ranges(S, nsplit):
    """[begin tile, end tile) of every split-KV range: attn_f16x3.hpp:525-527 kt_begin = split * ntiles / nsplit (integer division)"""
    nt = (S + 31) // 32
    return [(sp * nt // nsplit, (sp + 1) * nt // nsplit) for sp in range(nsplit)]


def launch_rule(precision, plan, knobs=None):
    """which rule the launch a plan describes follows - from the plan's own words (and the one knob the plan does not report)"""
    if precision == "f32":
        return "strict"
    if plan["attn_dma"] and (knobs or {}).get("attn_sm", 0) != 2:
        return "thr14"
    return "lazy8"


def launch_ranges(precision, plan, S):
    """only the LDS-DMA kernel splits the key range (launch_attn_f16x3: the register-staged kernels take no split argument)"""
    return key_ranges(S, plan["attn_nsplit"] if precision != "f32" and plan["attn_dma"] else 1)


def mask_words(valid, S):
    """[nseq, ntiles] the key-mask words (bit j of word t: key 32 t + j valid; keys past S are 0) - launch_mask_words"""
    nseq = valid.shape[0]
    nt = (S + 31) // 32
    pad = np.zeros((nseq, nt * 32), bool)
    pad[:, :S] = valid
    return (pad.reshape(nseq, nt, 32).astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(-1)


def head_planes(stage1, nseq, S, nhead):
    """(q, k) [nseq, nhead, S, hd] float64 from stage 1 of dbg_layer (hi + lo; Q as read back: unscaled)"""
    full = np.asarray(stage1[0], np.float64) + np.asarray(stage1[1], np.float64)
    d = full.shape[1] // 3
    hd = d // nhead
    cut = lambda a: a.reshape(nseq, S, nhead, hd).transpose(0, 2, 1, 3)
    return cut(full[:, :d]), cut(full[:, d:2 * d])


# ------------------------------------------------------------------------------------------------ the path model
def softmax_paths(q, k, valid, rule, ranges):
    """float64 model of a rule on q, k [nseq, nhead, S, hd] (logits in log2 units: q . k log2(e) / sqrt(hd)), valid [nseq, S], over the
    launch's key-tile ranges.  Arrays [nseq, nhead, S, ntiles]:
      computed  the tile is computed for that row (its mask word is not zero)
      first     it is the first computed tile of its range
      moved     the row's reference maximum moved there (never in a first tile: that one SETS it)
      excess    tile maximum - m before the tile (NaN where not computed or first)
      pmax      the largest P of the tile as the kernel forms it (after a move: 1)
      decisive  the branch does not hang on the logits' rounding: the tile sum outside [2^13.5, 2^14.5] (thr14), the excess outside
                [7.5, 8.5] (lazy8); once a row was not decisive the rest of its range is not either (its m is unknown)
    and  words [nseq, ntiles], range_of [ntiles], m_range [nseq, nhead, S, nranges] (the lazy m_i a range hands to the merge; -inf: it
    computed no tile), m_sure (every tile of that range was decisive for the row)."""
    assert rule in RULES
    nseq, nhead, S, hd = q.shape
    nt = (S + 31) // 32
    words = mask_words(valid, S)
    shape = (nseq, nhead, S, nt)
    out = dict(computed=np.zeros(shape, bool), first=np.zeros(shape, bool), moved=np.zeros(shape, bool), decisive=np.zeros(shape, bool),
               excess=np.full(shape, np.nan), pmax=np.full(shape, np.nan), words=words, range_of=np.full(nt, -1),
               m_range=np.full((nseq, nhead, S, len(ranges)), -np.inf), m_sure=np.ones((nseq, nhead, S, len(ranges)), bool), rule=rule, ranges=list(ranges))
    scale = R.LOG2E / np.sqrt(hd)
    for n in range(nseq):
        s_all = np.where(valid[n][None, None, :], (q[n] @ k[n].swapaxes(-1, -2)) * scale, -np.inf)      # [nhead, S, S]
        for ri, (t0, t1) in enumerate(ranges):
            m = np.full((nhead, S), -np.inf)
            sure = np.ones((nhead, S), bool)
            seen = False
            for t in range(t0, t1):
                out["range_of"][t] = ri
                if words[n, t] == 0:
                    continue
                s = s_all[:, :, 32 * t:min(32 * t + 32, S)]
                tmax = s.max(-1)
                out["computed"][n, :, :, t] = True
                if not seen:
                    seen = True
                    out["first"][n, :, :, t] = True
                    out["decisive"][n, :, :, t] = True
                    out["pmax"][n, :, :, t] = 1.0
                    m = tmax
                    continue
                excess = tmax - m
                if rule == "thr14":
                    lsum = np.log2(np.exp2(np.minimum(s - m[..., None], 1000.0)).sum(-1))
                    move = lsum > 14.0
                    sure &= np.abs(lsum - 14.0) > 0.5
                elif rule == "lazy8":
                    move = excess > TAU8
                    sure &= np.abs(excess - TAU8) > 0.5
                else:
                    move = excess > 0.0
                    sure &= np.abs(excess) > STRICT_EPS
                out["moved"][n, :, :, t] = move
                out["excess"][n, :, :, t] = excess
                out["decisive"][n, :, :, t] = sure
                m = np.where(move, tmax, m)
                out["pmax"][n, :, :, t] = np.exp2(np.minimum(tmax - m, 1000.0))
            out["m_range"][n, :, :, ri] = m
            out["m_sure"][n, :, :, ri] = sure
    return out


# ------------------------------------------------------------------------------------------------ predicates
def predicate_counts(P, judged):
    """every predicate's count on a path model; judged [nseq, S] bool: the query rows of real agents.  Only decisive rows count."""
    rule = P["rule"]
    nseq, nhead, S, nt = P["moved"].shape
    J = np.broadcast_to(judged[:, None, :, None], P["moved"].shape)
    later = P["computed"] & ~P["first"] & P["decisive"]
    mv = P["moved"] & later & J
    stay = ~P["moved"] & later & J
    pairs = int(judged.sum()) * nhead
    c = {"pairs": pairs, "movers": int(mv.any(-1).sum())}
    c["moves"] = c["movers"] / max(pairs, 1)
    c["last_partial"] = int(mv[..., nt - 1].sum()) if S % 32 else 0
    c["staircase"] = int((mv.sum(-1) >= 2).sum())
    lo, hi = SMALL_EXCESS[rule]
    ex = np.where(mv, P["excess"], np.nan)
    with np.errstate(invalid="ignore"):
        c["small_excess"] = int(((ex > lo) & (ex <= hi)).sum())
        c["wipe"] = int((ex > WIPE).sum())
        c["max_excess"] = float(np.nanmax(ex)) if mv.any() else 0.0
        if rule in HIGH_P:
            c["high_P_stay"] = int((stay & (P["pmax"] >= HIGH_P[rule][0]) & (P["pmax"] < HIGH_P[rule][1])).any(-1).sum())
        c["dead_tile"] = int((stay & (P["pmax"] < DEAD_P)).sum())
    # waves: 32 consecutive queries of a sequence (attn_f16x3.hpp: q = (qt * 4 + wid) * 32 + l31), every row the kernel runs
    full = S // 32
    c["mixed_wave"] = c["full_wave"] = 0
    if full:
        ok = (P["computed"] & ~P["first"] & P["decisive"])[:, :, :full * 32].reshape(nseq, nhead, full, 32, nt)
        m_ = (P["moved"] & P["computed"] & ~P["first"] & P["decisive"])[:, :, :full * 32].reshape(nseq, nhead, full, 32, nt)
        s_ = ok & ~m_
        c["mixed_wave"] = int((m_.any(3) & s_.any(3)).sum())
        c["full_wave"] = int(m_.all(3).sum())
    # masked form: a move in a tile whose word is neither zero nor all ones; a range whose first words are zero and that moves later
    last_full = (1 << (S - 32 * (nt - 1))) - 1
    all_ones = np.full(nt, 0xFFFFFFFF, np.uint64)
    all_ones[nt - 1] = last_full
    partial = (P["words"] != 0) & (P["words"] != all_ones[None, :])
    c["masked_move"] = int((mv & partial[:, None, None, :]).sum())
    c["zero_lead_move"] = c["zero_lead_ranges"] = 0
    for ri, (t0, t1) in enumerate(P["ranges"]):
        if t1 > t0:
            lead = P["words"][:, t0] == 0
            c["zero_lead_ranges"] += int((lead & ((P["words"][:, t0:t1] != 0).sum(1) >= 2)).sum())      # (a tile after the first computed one)
            c["zero_lead_move"] += int(mv[lead][..., t0:t1].sum())
    in_later_range = (P["range_of"] > 0)[None, None, None, :]
    c["split_move"] = int((mv & in_later_range).sum())
    mr = np.where(np.isfinite(P["m_range"]) & P["m_sure"], P["m_range"], np.nan)      # (a range whose m_i hangs on rounding is left out)
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)      # (a row none of whose ranges counts: NaN, no gap)
        gap =np.nanmax(mr, -1) - np.nanmin(mr, -1) if mr.shape[-1] > 1 else np.zeros(mr.shape[:-1])
    c["merge_gap"] = int(((gap > WIPE) & judged[:, None, :]).sum())
    return c


# what each predicate asks of the counts (minimums: conditions, not measurements)
MINIMUM = {"moves": ("moves", 0.05), "last_partial": ("last_partial", 8), "staircase": ("staircase", 4), "small_excess": ("small_excess", 1),
           "wipe": ("wipe", 1), "high_P_stay": ("high_P_stay", 4), "dead_tile": ("dead_tile", 8), "mixed_wave": ("mixed_wave", 1),
           "full_wave": ("full_wave", 1), "masked_move": ("masked_move", 1), "zero_lead_move": ("zero_lead_move", 1), "zero_lead_ranges": ("zero_lead_ranges", 1),
           "split_move": ("split_move", 1), "merge_gap": ("merge_gap", 1)}


def failed_predicates(names, counts, rule):
    bad = []
    for name in names:
        if name == "high_P_stay" and rule not in HIGH_P:
            continue
        key, least = MINIMUM[name]
        if not counts[key] >= least:
            bad.append((name, counts[key], least))
    return bad


# ------------------------------------------------------------------------------------------------ the cases
# loud keys of ascending c in tiles 0, 1, 2 and in the 9-key last tile of sequence 0; sequence 1: the loudest key in tile 0 (dead tiles
# behind it) and two blocks of c = 16 rows in tiles 2 and 3 - a c = 16 query on a c = 16 key is a logit of standard deviation 120, the
# only way to an excess above 126; sequence 2: wave 0 aligned (c = 6 ... 8 on the shared row), one loud key in the middle and the aligned
# keys +-16 in the last tile (one of the two signs lies above every aligned query's maximum in a head, whatever the sign of its g_h)
_WAVE = lambda row0: [(row0 + i, round(6 + 2 * i / 31, 2), "u") for i in range(32)]
STAIR = dict(shape=(3, 3, 5, 7), n_agents=None,
             loud=[(20, 2), (40, 6), (50, 7), (70, 10), (80, 11), (100, 16), (102, 16),
                   (108, 16), (169, 16), (170, 16), (171, 16), (202, 16), (203, 16), (204, 16),
                   (280, 10), (308, 16, "u"), (311, -16, "u")] + _WAVE(210),
             predicates=("moves", "last_partial", "staircase", "small_excess", "wipe", "high_P_stay", "dead_tile", "mixed_wave", "full_wave"))
# six ranges of 6 - 7 tiles (three under the knob): loud keys in the first (200; 620 ...) and last (380; 790 ...) tile of a range and
# across ranges; the c = 16 blocks for ranges whose m_i lie more than 126 apart; wave 12 aligned, the first tile of a range under both splits
SCENE = dict(shape=(1, 5, 20, 12), n_agents=None,
             loud=[(10, 12), (45, 4), (200, 8), (340, 7), (380, 12), (700, 10), (1190, 16),
                   (620, 16), (621, 16), (622, 16), (790, 16), (791, 16), (792, 16),
                   (450, 16, "u"), (460, -16, "u")] + _WAVE(384),
             predicates=("moves", "staircase", "split_move", "merge_gap", "mixed_wave", "full_wave"))
# loud REAL rows; sequence 1 (one real agent: every non-zero word is partial, every third word zero) has one behind the zero word that
# opens the third of three ranges
MASKED = dict(shape=(3, 4, 8, 12), n_agents=[4, 1, 3],
              loud=[(40, 6), (100, 16), (101, 16), (200, 12), (300, 16), (301, 16),
                    (384 + 5, 8), (384 + 200, 14), (384 + 340, 14), (768 + 100, 8), (768 + 340, 14)],
              predicates=("moves", "masked_move"))
CASES = {"stair": STAIR, "scene": SCENE, "masked": MASKED}
NETS = {"stair": list(WC.NETS), "scene": [(256, 4), (256, 8), (512, 8)], "masked": [(256, 4), (32, 4), (256, 8)]}
assert all(n in WC.NETS for nets in NETS.values() for n in nets)
# knob sets at (256, 4): (knobs, modes, plan facts, further predicates)
SPLIT_MODES = ["f16x3", "f16x2", "f16mx"]
SCENE_KNOBS = [({"attn_nsplit": 3, "small_cmb": 0}, SPLIT_MODES, {"attn_nsplit": 3}),
               ({"attn_nsplit": 3, "small_cmb": 2}, SPLIT_MODES, {"attn_nsplit": 3, "merge": 0}),
               ({"attn_h_variant": 1}, SPLIT_MODES, {"attn_dma": 0, "k8": 0}),
               ({"attn_sm": 2}, SPLIT_MODES, {"attn_dma": 1}),
               ({"attn_mx": 2}, ["f16mx"], {"k8": 0, "q8l": 0, "attn_dma": 1})]
MASKED_KNOBS = [({"attn_nsplit": 3}, SPLIT_MODES, {"attn_nsplit": 3, "masked": 1}),
                ({"attn_nsplit": 12}, SPLIT_MODES, {"attn_nsplit": 12, "masked": 1})]


def case_predicates(name, ranges):
    """the predicates a run of a case is there for: the split ones only where the launch split the key range.  Ranges of one tile each
    (S = 384 under "attn_nsplit" = 12) have no tile after their first: no rule can move there, and what such a launch tests is the merge
    of twelve lazy m_i, some of them -inf - merge_gap alone."""
    names = list(CASES[name]["predicates"])
    if len(ranges) == 1:
        return [p for p in names if p not in ("split_move", "merge_gap")]
    if max(t1 - t0 for t0, t1 in ranges) <= 1:
        return ["merge_gap"]
    if name == "masked":
        names += ["split_move"]
        if len(ranges) == 3:      # four tiles each: the third range of the one-agent sequence opens on a zero word (every third word is zero).
            names += ["zero_lead_ranges", "zero_lead_move"]      # Asserted, not assumed: a change of the range arithmetic fails here
    return names


# ------------------------------------------------------------------------------------------------ reporting
def mover_mask(P, hd):
    """[M, d] bool: the output elements of the (row, head) pairs whose reference maximum moved in a tile after their range's first"""
    mv = (P["moved"] & P["computed"] & ~P["first"]).any(-1)               # [nseq, nhead, S]
    nseq, nhead, S = mv.shape
    return np.repeat(mv.transpose(0, 2, 1).reshape(nseq * S, nhead), hd, axis=1)


def worst_by_path(ratio, P, hd, rows):
    """(worst err / bound among movers, among non-movers) over the judged rows"""
    mask = mover_mask(P, hd)
    r = np.where(rows[:, None], ratio, 0.0)
    return float(np.where(mask, r, 0.0).max()), float(np.where(~mask, r, 0.0).max())
