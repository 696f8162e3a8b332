"""GPU: the phase-timer instantiation of the wave-quad update kernel (hp._pad & 1) is the same computation as the production one.  The phase tables
of profiles/update_lds_batch.md are read from that instantiation; they are only worth something if it leaves the very parameters, moments, step
counter and statistics the production kernel leaves — through the in-kernel gather and through the minibatch stream, at the shapes where ragged,
multi-chunk, sub-chunk and discrete-action paths run (tests/helpers/update_stream.py)."""
import pytest
import torch

from test_update_stream_gpu import _assert_same, _case, _same_bits

pytestmark = pytest.mark.gpu

PROF = 1      # hp._pad bit: the instantiation with the phase timers


@pytest.mark.parametrize("mode", ["gather", "stream"])
@pytest.mark.parametrize("name", ["hc-b64", "hc-b40", "hc-b160", "hc-35", "lgw-b64"])
def test_phase_timer_build_is_the_same_computation(name, mode):
    c = _case(name)
    ref, words, _ = c.run(mode)
    assert words[4] == (1 if mode == "stream" else 0) and words[0] == 5
    assert not bool(ref[4][12:32].any())      # the production instantiation carries no timers
    got, words, _ = c.run(mode, PROF)
    assert words[4] == (1 if mode == "stream" else 0) and words[0] == 5
    assert bool((got[4][12:26] > 0).all())      # the seven phases of the policy and the reward-critic workgroup were timed: the other instantiation ran
    _assert_same(got, ref, f"{name}, {mode}, phase timers")
    assert not _same_bits(got[:1], c.state0[:1])      # (and it did train)
