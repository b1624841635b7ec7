"""The networks the GPU tests create: the one place in tests/ where widths are named.

jmid_create accepts ctx_dim = 32 k in [32, 512], any nhead whose head size is 16, 32, 64 or 128, and hist_len up to 16
(include/jmid_hip.h).  Every row below is a (ctx_dim, nhead) the width-parametrised tests run; d_model = 2 ctx_dim,
head = d_model / nhead, LSTM hidden = ctx_dim / 2 (weights.NetDims).  A row whose ``refused`` is a string is one the library says no
to where the handle is made: the tests pin the refusal instead of running it.
"""
from collections import namedtuple

Row = namedtuple("Row", "ctx_dim nhead why refused")

ROWS = [
    Row(32, 4, "d_model 64, head 16, hidden 16: the reduced width of the suite", None),
    Row(64, 4, "d_model 128, head 32: N = 64 concat3, the generic encoder loop; a width the reference can build", None),
    Row(96, 6, "d_model 192, head 32, hidden 48: N and K no multiples of 128, F16MX and F16X2 GEMMs in one step, a three-wave encoder", None),
    Row(96, 12, "d_model 192, head 16: head 16 at a width other than 64", None),
    Row(128, 4, "d_model 256, head 64; a width the reference can build", None),
    Row(256, 4, "d_model 512, head 128, hidden 128: the shipped width", None),
    Row(256, 8, "d_model 512, head 64: fused LayerNorm, the one-launch GEMM + LayerNorm, the split-KV merge beside the non-DMA attention kernel", None),
    Row(512, 8, "d_model 1024, head 128, hidden 256: the unfolded tail, the encoder at its LDS and thread limit", None),
]

RUN = [r for r in ROWS if r.refused is None]
NETS = [(r.ctx_dim, r.nhead) for r in RUN]                       # every accepted row
OLD_NETS = [(32, 4), (256, 4)]                                   # the two the suite ran before the table
NEW_NETS = [n for n in NETS if n not in OLD_NETS]
CTX_DIMS = sorted({r.ctx_dim for r in RUN})                      # where nhead does not matter (encoder, hyper rows, tail)
OLD_CTX_DIMS = [c for c, _ in OLD_NETS]
REFERENCE_NETS = [n for n in NETS if n[1] == 4]                  # the reference's nhead is 4: rows it can make fixtures for
ORACLE_ONLY_NETS = [n for n in NEW_NETS if n[1] != 4]
HIDDEN = sorted({c // 2 for c in CTX_DIMS})                      # 16 and 128 are register variants of the encoder, the rest the generic loop


def nhead_of(ctx_dim):
    """the first head count the table has for a width: for the tests of code that does not read it (encoder, hyper rows, tail)"""
    return next(h for c, h in NETS if c == ctx_dim)


TAIL_MAX_D, TAIL_MAX_MID, TAIL_MAX_LOW = 512, 256, 128      # csrc/tail_fold.hpp kTailMaxD / kTailMaxMid / kTailMaxLow


def tail_folds(ctx_dim):
    """does a split-fp16 call fold the tail at this width (csrc/jmid_planner.hip plan_step: p.tail_fold, without the knob)?"""
    d, dmid, dlow = 2 * ctx_dim, ctx_dim, ctx_dim // 2
    return d % 8 == 0 and d <= TAIL_MAX_D and dmid <= TAIL_MAX_MID and dlow <= TAIL_MAX_LOW


def per_trajectory(ctx_dim):
    """is there a per-trajectory output kernel at this width (plan_step: out_tpw needs d <= 512, csrc/elementwise.hpp:266)?"""
    return 2 * ctx_dim <= 512


def d_model(ctx_dim):
    return 2 * ctx_dim


def head(ctx_dim, nhead):
    return 2 * ctx_dim // nhead


def net_id(net):
    return f"w{net[0]}h{net[1]}"
