"""GPU: the segment of the wave-quad update kernel (ppo_train_halves.hip) between the norm granule's store and Adam — the hop in whose shadow work is
moved in front of barrier (S6): today the request of the clip threshold; tried and dropped, Adam's beta scaling of the moments and a rolling granule
poll (profiles/update_norm_hop.md).  What such a move can break is a value that is missing or applied twice on one instantiation, or work done for
a step whose Adam never ran — a target-KL stop, the last step of a launch.  Everything is compared bit for bit: between the production, the
phase-timer and the in-kernel-gather instantiations, with four and with two workgroups per network, and between a launch that stops on its KL
and one that was told to run exactly the epochs in front of the stop."""
import numpy as np
import pytest
import torch

from helpers.update_stream import SHAPES, stream_bytes
from test_update_stream_gpu import _assert_same, _make, _same_bits

pytestmark = pytest.mark.gpu

PROF, TWO_PARTS = 1, 32      # hp._pad bits: the instantiation with the phase timers; two workgroups per network instead of four


class _Launcher:
    """an agent at a shape of helpers/update_stream.py with `epochs` permutations (and optionally another batch size); run() restores the initial
    state and makes ONE update call with the epochs / target KL it is given."""

    def __init__(self, name, epochs, batch_size=None, lp_shift=0.0):
        O, A, AS, disc, T, N, B, _ = SHAPES[name]
        self.agent, _, _ = _make(name, lp_shift=lp_shift)
        self.agent.n_epochs = epochs
        if batch_size is not None:
            self.agent.batch_size = B = batch_size
        self.n, self.B, self.E = T * N, B, epochs
        rng = np.random.RandomState(77 + self.n + B)
        self.job = self.agent._train_begin(np.stack([rng.permutation(self.n) for _ in range(epochs)]).astype(np.int32))
        pol, ws = self.agent.policy, self.agent._train_ws
        self.state0 = [t.clone() for t in (pol.params, pol.exp_avg, pol.exp_avg_sq, ws["t"])]
        self.need = stream_bytes(O, AS, self.n, B, epochs)
        self.steps_per_epoch = -(-self.n // B)

    def run(self, mode, pad=0, epochs=None, target_kl=None):
        from icrl_amd import _lib
        from icrl_amd.structs import PpoHyperT, p
        pol, ws, b, job = self.agent.policy, self.agent._train_ws, _lib.byref, self.job
        for dst, src in zip((pol.params, pol.exp_avg, pol.exp_avg_sq, ws["t"]), self.state0):
            dst.copy_(src)
        ws["stats"].zero_()
        hp = PpoHyperT.from_buffer_copy(job["hp"])
        hp._pad |= pad
        hp.n_epochs = self.E if epochs is None else epochs
        hp.use_target_kl, hp.target_kl = (0, 0.0) if target_kl is None else (1, float(target_kl))
        head = (b(job["ps"]), p(pol.exp_avg), p(pol.exp_avg_sq), p(ws["t"]), b(job["bs"]), p(job["perms"]), p(ws["nu"]), b(hp), p(ws["stats"]), p(ws["sync"]))
        if mode == "gather":
            _lib.check(_lib.lib().icrl_ppo_lag_train(*head, _lib.current_stream()), "icrl_ppo_lag_train")
        else:
            sws = torch.zeros(self.need, dtype=torch.uint8, device="cuda")
            _lib.check(_lib.lib().icrl_ppo_lag_train_stream(*head, p(sws), self.need, _lib.current_stream()), "icrl_ppo_lag_train_stream")
        torch.cuda.synchronize()
        words = _lib.last_route(_lib.FAMILY_UPDATE)
        assert words[4] == (1 if mode == "stream" else 0) and words[1] == (2 if pad & TWO_PARTS else 4)
        state = [t.clone() for t in (pol.params, pol.exp_avg, pol.exp_avg_sq, ws["t"], ws["stats"])]
        assert float(state[4][11]) == 0.0, "inter-workgroup exchange timed out"
        return state


_launchers = {}


def _launcher(*key):      # (one agent per configuration, shared by the tests below; run() restores its state)
    if key not in _launchers:
        _launchers[key] = _Launcher(*key)
    return _launchers[key]


def _instantiations_agree(c, pad, what, **kw):
    ref = c.run("stream", pad, **kw)
    assert not bool(ref[4][12:32].any())      # the production instantiation carries no timers
    assert not _same_bits(ref[:3], c.state0[:3])      # (it did train)
    prof = c.run("stream", pad | PROF, **kw)
    assert bool((prof[4][12:26] > 0).all())      # the phases were timed: the other instantiation ran
    _assert_same(prof, ref, f"{what}, phase timers")
    _assert_same(c.run("gather", pad, **kw), ref, f"{what}, in-kernel gather")
    _assert_same(c.run("gather", pad | PROF, **kw), ref, f"{what}, in-kernel gather with phase timers")
    return ref


@pytest.mark.parametrize("parts", [4, 2])
@pytest.mark.parametrize("name", ["hc-b64", "hc-b40", "hc-35", "lgw-b64"])
def test_instantiations_agree_after_three_epochs(name, parts):
    """production, phase-timer and in-kernel-gather instantiations: identical parameters, moments, step counter and statistics after 3 epochs (6, 12, 3
    and 6 optimiser steps; hc-35: one ragged 35-row minibatch per epoch; hc-b40: a ragged chunk in every step and a ragged 8-row last minibatch)."""
    c = _launcher(name, 3)
    ref = _instantiations_agree(c, TWO_PARTS if parts == 2 else 0, f"{name}, {parts} parts")
    assert int(ref[4][0]) == 3 and int(ref[4][1]) == 3 * c.steps_per_epoch and int(ref[3][0]) == int(c.state0[3][0]) + 3 * c.steps_per_epoch


@pytest.mark.parametrize("parts", [4, 2])
def test_a_single_optimiser_step(parts):
    """one epoch, rows = batch (128): the launch is one optimiser step — one pass through (S6) and one Adam, then the write-back."""
    c = _launcher("hc-b64", 1, 128)
    assert c.steps_per_epoch == 1
    ref = _instantiations_agree(c, TWO_PARTS if parts == 2 else 0, f"one step, {parts} parts")
    assert int(ref[4][1]) == 1 and int(ref[3][0]) == int(c.state0[3][0]) + 1


@pytest.mark.parametrize("name,parts,mode", [("hc-b40", 4, "stream"), ("hc-b40", 2, "stream"), ("lgw-b64", 4, "stream"), ("hc-35", 4, "gather")])
def test_target_kl_stop_behind_epoch_0(name, parts, mode):
    """old log-probs 0.05 above the policy's: the mean KL of epoch 0 is ~0.05, far above 1.5 x 1e-4, so the launch stops behind epoch 0 of 3.  It leaves
    what a launch of ONE epoch without a target leaves: the same steps ran, and nothing was done to a moment for a step that did not."""
    c = _launcher(name, 3, None, 0.05)
    pad = TWO_PARTS if parts == 2 else 0
    got = c.run(mode, pad, target_kl=1e-4)
    assert int(got[4][0]) == 0 and int(got[4][1]) == c.steps_per_epoch and float(got[4][11]) == 0.0
    assert float(got[4][32]) > 1.5e-4 and not bool(got[4][33:].any())      # epoch 0's KL was logged, epochs 1 and 2 never ran
    want = c.run(mode, pad, epochs=1)
    assert int(want[4][1]) == c.steps_per_epoch
    _assert_same([g[:33] if i == 4 else g for i, g in enumerate(got)][:4], want[:4], f"{name}, stop behind epoch 0")
    assert _same_bits([got[4][1:12], got[4][32:33]], [want[4][1:12], want[4][32:33]])      # (stats[0]: the stop epoch against "none")


@pytest.mark.parametrize("parts", [4, 2])
def test_target_kl_stop_behind_epoch_1(parts):
    """the target is taken from the run's own log: between the KLs of epoch 0 and epoch 1 of a launch without a target (the policy moves away from the
    rollout's, so the KL of epoch 1 is the larger one; old log-probs 0.01 above the policy's keep the logged mean of old - new log-prob, which at a
    noise of 0.05 per row can fall below zero, positive).  The launch then runs epochs 0 and 1 of 3 and equals a two-epoch launch without a target."""
    c = _launcher("hc-b40", 3, None, 0.01)
    pad = TWO_PARTS if parts == 2 else 0
    free = c.run("stream", pad)
    kl0, kl1 = float(free[4][32]), float(free[4][33])
    print(f"hc-b40, {parts} parts: logged KL of epochs 0, 1, 2 = {kl0:.3e}, {kl1:.3e}, {float(free[4][34]):.3e}")
    assert kl1 > kl0 > 0
    target = np.float32(0.5 * (kl0 + kl1) / 1.5)
    assert kl0 <= float(np.float32(1.5) * target) < kl1      # (the kernel's own comparison, in float32)
    got = c.run("stream", pad, target_kl=target)
    assert int(got[4][0]) == 1 and int(got[4][1]) == 2 * c.steps_per_epoch and float(got[4][11]) == 0.0
    assert _same_bits([got[4][32:34]], [free[4][32:34]]) and float(got[4][34]) == 0.0
    want = c.run("stream", pad, epochs=2)
    _assert_same(got[:4], want[:4], "stop behind epoch 1")
    assert _same_bits([got[4][1:12], got[4][32:34]], [want[4][1:12], want[4][32:34]])
    _assert_same(c.run("gather", pad, target_kl=target), got, "stop behind epoch 1, in-kernel gather")
