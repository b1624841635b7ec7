"""Host side of the denoising loss (jmid_loss; DiffusionTraj.get_loss, MID/models/diffusion.py:448-476): the twin of the device
reduction, the mask derivation of offline.get_loss, the per-timestep schedule and the per-timestep diagnostic.  No GPU.

The fixtures tests/golden/loss_*.npz come from the reference's own get_loss (tests/golden/make_golden_loss.py)."""
import glob
import os

import numpy as np
import pytest
import torch

from safe_interactive_crowdnav_amd import metrics, offline
from safe_interactive_crowdnav_amd.schedule import VarianceSchedule, loss_tables

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = sorted(os.path.basename(p) for p in glob.glob(os.path.join(GOLDEN, "loss_*.npz")))
EXPECTED = ["loss_imid_w32_e3a3t6.npz", "loss_jmid_w256_e2a25t12.npz", "loss_jmid_w256_e3a4t12.npz", "loss_jmid_w32_e2a2t4_full.npz",
            "loss_jmid_w32_e3a3t6.npz"]


def test_every_fixture_is_present_and_covers_its_timesteps():
    assert CASES == EXPECTED
    for case in CASES:
        z = np.load(os.path.join(GOLDEN, case))
        n = z["n_agents"] if "n_agents" in z.files else np.full(z["t"].shape[0], z["t"].shape[1])
        real = np.arange(z["t"].shape[1])[None, :] < n[:, None]
        t = z["t"]
        assert t.min() >= 1 and t.max() <= 100 and 1 in t[real] and 100 in t[real]
        assert float(z["compact_err"]) <= 1e-5
    z = np.load(os.path.join(GOLDEN, "loss_jmid_w256_e3a4t12.npz"))      # a scene with a repeated and a distinct timestep
    assert len(set(z["t"][0].tolist())) in (2, 3)


@pytest.mark.parametrize("case", EXPECTED)
def test_loss_host_reproduces_the_reference_loss(case):
    """fp32 difference and square, fp64 sums, against the reference's fp32 torch.mean: 1e-6 relative (the fp32 vs fp64 mean gap of the
    fixtures, measured when they were made, is <= 8e-8)."""
    z = np.load(os.path.join(GOLDEN, case))
    n = z["n_agents"] if "n_agents" in z.files else None
    loss, count, rows = metrics.loss_host(z["e_theta"], z["e"], n)
    E, A, T, _ = z["e"].shape
    n_real = int(n.sum()) if n is not None else E * A
    rel = abs(loss - float(z["loss"])) / float(z["loss"])
    print(f"{case}: loss_host {loss:.9f}  reference {float(z['loss']):.9f}  rel {rel:.2e}  (fixture's own fp64 gap {float(z['loss_rel']):.2e})")
    assert count == n_real * T * 2
    assert rel <= 1e-6, rel
    assert float(z["loss_rel"]) <= 8e-8
    real = np.ones((E, A), bool) if n is None else np.arange(A)[None, :] < n[:, None]
    assert np.isnan(rows[~real]).all() and np.isfinite(rows[real]).all()
    # the rows are the fp64 sums of the fp32 squares
    d = (z["e_theta"] - z["e"]).astype(np.float32)
    want = (d * d).astype(np.float32).astype(np.float64).reshape(E, A, -1).sum(-1)
    np.testing.assert_allclose(rows[real], want[real], rtol=1e-14, atol=0)
    # NaN in the padded rows of e_theta (what the device returns) changes nothing
    if n is not None and (~real).any():
        et = z["e_theta"].copy()
        et[~real] = np.nan
        again = metrics.loss_host(et, z["e"], n)
        assert again[0] == loss and again[1] == count


def test_loss_host_refuses_bad_arguments():
    e = np.zeros((2, 3, 4, 2), np.float32)
    with pytest.raises(ValueError):
        metrics.loss_host(e, e[:, :2])
    with pytest.raises(ValueError):
        metrics.loss_host(e, e, n_agents=[0, 3])
    with pytest.raises(ValueError):
        metrics.loss_host(e, e, n_agents=[3])


@pytest.mark.parametrize("case", [c for c in EXPECTED if "jmid" in c])
def test_mask_derivation_yields_the_fixture_counts(case):
    z = np.load(os.path.join(GOLDEN, case))
    n = z["n_agents"]
    E, A, T, _ = z["x0"].shape
    y = z["x0"].copy()
    y[np.arange(A)[None, :] >= n[:, None]] = np.nan
    got = offline.agent_counts_from_futures(y.reshape(E * A, T, 2), E)
    assert got.dtype == np.int32
    np.testing.assert_array_equal(got, n)
    np.testing.assert_array_equal(offline.agent_counts_from_futures(torch.from_numpy(y.reshape(E * A, T, 2)), E), n)


def test_mask_derivation_refuses_what_the_two_reference_masks_disagree_on():
    E, A, T = 2, 3, 4
    y = np.random.default_rng(0).standard_normal((E, A, T, 2)).astype(np.float32)
    np.testing.assert_array_equal(offline.agent_counts_from_futures(y.reshape(E * A, T, 2), E), [3, 3])
    bad = y.copy()
    bad[0, 1] = np.nan              # a NaN row in front of a real one
    with pytest.raises(ValueError, match="two masks disagree"):
        offline.agent_counts_from_futures(bad.reshape(E * A, T, 2), E)
    bad = y.copy()
    bad[1, 2, 3, 0] = np.nan        # a partly-NaN row
    with pytest.raises(ValueError, match="two masks disagree"):
        offline.agent_counts_from_futures(bad.reshape(E * A, T, 2), E)
    bad = y.copy()
    bad[1] = np.nan                 # a scene without agents
    with pytest.raises(ValueError, match="no real agent"):
        offline.agent_counts_from_futures(bad.reshape(E * A, T, 2), E)
    with pytest.raises(ValueError):
        offline.agent_counts_from_futures(y.reshape(E * A, T, 2), 4)
    ok = y.copy()
    ok[0, 2] = np.nan
    ok[1, 1:] = np.nan
    np.testing.assert_array_equal(offline.agent_counts_from_futures(ok.reshape(E * A, T, 2), E), [2, 1])


def test_loss_tables_are_the_square_roots_of_the_reference_schedule_bit_for_bit():
    z = np.load(os.path.join(GOLDEN, "schedule.npz"))
    beta, c0, c1 = loss_tables(VarianceSchedule.linear())
    ab = torch.from_numpy(z["alpha_bars"])
    assert beta.dtype == c0.dtype == c1.dtype == np.float32 and beta.shape == c0.shape == c1.shape == (101,)
    np.testing.assert_array_equal(beta.view(np.uint32), z["betas"].view(np.uint32))
    np.testing.assert_array_equal(c0.view(np.uint32), torch.sqrt(ab).numpy().view(np.uint32))
    np.testing.assert_array_equal(c1.view(np.uint32), torch.sqrt(1 - ab).numpy().view(np.uint32))
    assert beta[0] == 0 and c0[0] == 1 and c1[0] == 0          # the padding entry


def test_loss_by_timestep_hand_case():
    T = 2
    rows = np.array([[4.0, 8.0, 100.0], [12.0, 2.0, 6.0]])
    t = np.array([[5, 7, 9], [5, 5, 7]])
    got = metrics.loss_by_timestep(rows, t, T)
    assert got == {5: (4.0 + 12.0 + 2.0) / (3 * 4), 7: (8.0 + 6.0) / (2 * 4), 9: 100.0 / 4}
    # padded rows (NaN, any t) are left out
    rows[0, 2] = np.nan
    got = metrics.loss_by_timestep(rows, t, T, n_agents=[2, 3])
    assert got == {5: 18.0 / 12, 7: 14.0 / 8}
    with pytest.raises(ValueError):
        metrics.loss_by_timestep(rows, t[:, :2], T)
