"""The context encoder (csrc/encoder.hpp: three LSTMs + additive attention, one workgroup per row) against float64, element by element,
at every LSTM hidden size of tests/width_cases.py: 16 and 128 run the register variants encoder_kernel<16> / <128>, 32, 48, 64 and 256
the generic loop encoder_kernel<0> (256: 1024 threads, gates[4 * ENC_MAX_H] exactly full; 48: 192 threads, three waves), and at
hist_len 2, 8 and 16 = ENC_MAX_TH.

The tolerance is measured against the reference, not the device: the distance of the float32 CPU oracle from the float64 one on the
case's own inputs, times 8 (the device's tanhf / expf are not torch's and its sums run in another order over up to 16 recurrent
steps), and never looser than the 5e-6 of tests/test_gpu_parity.py::test_context_encoder_matches_reference_golden."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import tests.width_cases as WC
from oracle import jmid_oracle as O
from safe_interactive_crowdnav_amd.engine import JmidEngine
from safe_interactive_crowdnav_amd.weights import JMIDWeights, NetDims

N_ROWS = 9
EDGE_MASKS = [[1, 1], [1, 0], [0, 1], [0, 0], [.5, .25]]      # [0, 0]: a softmax over two equal scores of zero vectors
HIST = [2, 8, 16]
FACTOR, ATOL_MAX = 8.0, 5e-6
_W = {}


def weights(ctx_dim):
    if ctx_dim not in _W:
        w = JMIDWeights.from_seed(NetDims(ctx_dim=ctx_dim, nhead=WC.nhead_of(ctx_dim)), 5)
        _W[ctx_dim] = (w, O.to_dtype(w.tensors, torch.float64))
    return _W[ctx_dim]


def inputs(ctx_dim, Th):
    """x_st ~ 2 N(0, 1), nbr_sum ~ 3 N(0, 1): the gates reach saturation"""
    g = torch.Generator().manual_seed(1000 * ctx_dim + Th)
    x_st = 2.0 * torch.randn([N_ROWS, Th, 6], generator=g)
    nbr = 3.0 * torch.randn([N_ROWS, 2, Th, 6], generator=g)
    em = torch.tensor([EDGE_MASKS[r % len(EDGE_MASKS)] for r in range(N_ROWS)], dtype=torch.float32)
    fi = torch.randint(0, Th - 1, [N_ROWS], generator=g).numpy().astype(np.int32)      # 0 .. Th - 2
    return x_st, nbr, em, fi


def reference(w, x_st, nbr, em, fi, dtype):
    """rows of the oracle in ``dtype``; fi: every row on its own slice of the window"""
    with torch.no_grad():
        if fi is None:
            return O.encode_context(w, x_st.to(dtype), nbr.to(dtype), em.to(dtype)).numpy()
        return np.concatenate([O.encode_context(w, x_st[r:r + 1, f:].to(dtype), nbr[r:r + 1, :, f:].to(dtype), em[r:r + 1].to(dtype)).numpy()
                               for r, f in enumerate(fi)])


@pytest.mark.parametrize("Th", HIST)
@pytest.mark.parametrize("ctx_dim", WC.CTX_DIMS)
def test_context_encoder_matches_float64(ctx_dim, Th):
    w, w64 = weights(ctx_dim)
    x_st, nbr, em, fi = inputs(ctx_dim, Th)
    eng = JmidEngine(w, joint=True, hist_len=Th, step=2)
    try:
        for label, first in (("full window", None), ("first_index", fi)):
            xs, nb = x_st.clone(), nbr.clone()
            if first is not None:
                for r, f in enumerate(first):
                    xs[r, :f] = float("nan")
                    nb[r, :, :f] = float("nan")
            ref = reference(w64, x_st, nbr, em, first, torch.float64)
            o32 = reference(w.tensors, x_st, nbr, em, first, torch.float32)
            dist = float(np.abs(o32.astype(np.float64) - ref).max())
            tol = min(FACTOR * dist, ATOL_MAX)
            ctx = eng.encode(xs.numpy(), nb.numpy(), em.numpy(), first_index=first)
            assert ctx.shape == (N_ROWS, ctx_dim) and ctx.dtype == np.float32 and np.isfinite(ctx).all()
            err = np.abs(ctx.astype(np.float64) - ref)
            i = np.unravel_index(int(err.argmax()), err.shape)
            print(f"encoder hidden {ctx_dim // 2} hist_len {Th} {label}: device max |err| {err.max():.3e} at row {i[0]} col {i[1]}; "
                  f"float32 oracle {dist:.3e}, allowed {tol:.3e}; max |ctx| {np.abs(ref).max():.3f}")
            assert err.max() <= tol, (ctx_dim, Th, label, float(err.max()), tol)
            # the [0, 0] rows: no edge encoding, the history encoding alone
            zero = [r for r in range(N_ROWS) if EDGE_MASKS[r % len(EDGE_MASKS)] == [0, 0]]
            assert zero and not ctx[zero, :ctx_dim // 2].any()
    finally:
        eng.close()
