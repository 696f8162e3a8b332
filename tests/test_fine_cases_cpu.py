"""CPU: the conditions of the cases in tests/helpers/fine_cases.py that tests/test_fine_grained_gpu.py relies on — checked here, where no kernel runs."""
import numpy as np
import pytest
import torch

from helpers import fine_cases as F, ppo_hparam_cases as H


@pytest.mark.parametrize("n", F.LOSS_ROWS)
def test_the_banded_minibatch_meets_its_conditions_and_has_a_bound(n):
    """no row of the n-row minibatch on a kink under sets A and B, the clip shares inside their windows; one positive bound per output gradient."""
    b = F.hparam_batch(n)
    for hset in ("A", "B"):
        _, g64, margins, shares = F.loss_and_row_grads(b, H.hparams(hset), F.LOSS_NU, torch.float64)
        assert F.banded_conditions_hold(margins, shares), (n, hset, margins, shares)
        assert all(g64[k].shape == (n,) and np.abs(g64[k]).max() > 0 for k in F.ROW_GRAD_KEYS)
    assert set(F.ROW_GRAD_F32_DEV[n]) == set(F.ROW_GRAD_KEYS) and all(v > 0 for v in F.ROW_GRAD_F32_DEV[n].values())


@pytest.mark.parametrize("n", [300, 1000])
def test_the_row_gradient_table_is_what_the_helper_measures(n):
    """the stored max |float32 oracle - float64 oracle| against a fresh measurement: the same order of magnitude on any CPU (float32 sums of
    another torch build may differ in the last places, which moves the maximum by a fraction of itself)."""
    dev, _ = F.row_grad_dev(n)
    for k in F.ROW_GRAD_KEYS:
        assert 0.5 * F.ROW_GRAD_F32_DEV[n][k] <= dev[k] <= 2.0 * F.ROW_GRAD_F32_DEV[n][k], (n, k, dev[k], F.ROW_GRAD_F32_DEV[n][k])


@pytest.mark.parametrize("per_step", [False, True])
def test_the_is_weights_case_walks_past_every_first_trip_without_overflow(per_step):
    lengths = F.IS_LENGTHS
    assert len(lengths) > 16 and sum(lengths) > 1024 and max(lengths) > 64      # waves over episodes, threads over rows, lanes over steps
    assert {65, 129, 64, 128, 1} <= set(lengths)                                # one live lane in the last trip; whole trips; a single step
    r64, r32, bounds = F.is_weights_oracles(per_step)
    assert 0.1 < r64["prod"].min() and r64["prod"].max() < 2.0
    assert r64["w"].shape == (sum(lengths),) and all(0 < v < 1e-5 for v in bounds.values()), bounds
