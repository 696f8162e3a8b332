"""GPU: the pre-gathered minibatch stream of the update (icrl_ppo_lag_train_stream).  The pre-pass's records against a numpy gather (exact),
its statistics table against float64 numpy, then the whole update in both forms from the same state: bit-identical parameters, moments,
step counter and statistics — the stream changes where the rows come from, not one value or the order of one sum."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from helpers import routes
from helpers.update_stream import PLANES, SHAPES, minibatch_stats, records, stream_bytes

pytestmark = pytest.mark.gpu


def _make(name, target_kl=None, lp_shift=0.0):
    """an agent at the shape, its rollout buffer filled with distinct values whose old log-probs and values are the policy's own (ratios start
    near 1 as after a rollout; lp_shift: the old log-probs that much above them, i.e. an approximate KL of that size), a permutation per epoch; returns (agent, buffer planes as numpy, perms)."""
    from icrl_amd import spaces
    from icrl_amd.ppo_lag import PPOLagrangian
    from icrl_amd.vec_env import HipSynthVecEnv, VecCostWrapper, VecNormalizeWithCost
    O, A, AS, disc, T, N, B, E = SHAPES[name]
    rng = np.random.RandomState(1000 + O + T * N + B)
    senv = HipSynthVecEnv(N, "hc", 0)
    if disc or (O, A) != (18, 6):      # (any other shape: the env's spaces overridden, as nothing steps it here)
        senv.observation_space = spaces.Box(-np.inf, np.inf, (O,), np.float64)
        senv.action_space = spaces.Discrete(A) if disc else spaces.Box(-1.0, 1.0, (A,), np.float32)
    agent = PPOLagrangian("TwoCriticsMlpPolicy", VecNormalizeWithCost(VecCostWrapper(senv)), n_steps=T, seed=0, batch_size=B, n_epochs=E, target_kl=target_kl)
    n = T * N
    obs = rng.randn(T, N, O).astype(np.float32)
    act = rng.randint(0, A, (T, N, 1)).astype(np.float32) if disc else np.clip(rng.randn(T, N, A), -1, 1).astype(np.float32)
    v_r, v_c, lp, _ = agent.policy.evaluate_actions(obs.reshape(n, O), act.reshape(n, AS))
    buf = dict(observations=obs, actions=act, log_probs=lp.cpu().numpy().reshape(T, N) + 0.05 * rng.randn(T, N).astype(np.float32) + np.float32(lp_shift),
               reward_values=v_r.cpu().numpy().reshape(T, N), cost_values=v_c.cpu().numpy().reshape(T, N),
               reward_advantages=rng.randn(T, N).astype(np.float32) * 2, cost_advantages=rng.rand(T, N).astype(np.float32),
               reward_returns=rng.randn(T, N).astype(np.float32), cost_returns=rng.rand(T, N).astype(np.float32))
    rb = agent.rollout_buffer
    for k, v in buf.items():
        getattr(rb, k).copy_(torch.as_tensor(np.asarray(v, np.float32)).reshape(getattr(rb, k).shape))
    rb.full = True
    perms = np.stack([rng.permutation(n) for _ in range(E)]).astype(np.int32)
    return agent, buf, perms


class _Case:
    """one agent, its job descriptors and initial state; run(mode) restores the state and makes ONE update call."""

    def __init__(self, name, target_kl=None, lp_shift=0.0):
        self.name = name
        self.agent, self.buf, self.perms = _make(name, target_kl, lp_shift)
        self.job = self.agent._train_begin(self.perms)
        pol, ws = self.agent.policy, self.agent._train_ws
        self.state0 = [t.clone() for t in (pol.params, pol.exp_avg, pol.exp_avg_sq, ws["t"])]
        O, A, AS, disc, T, N, B, E = SHAPES[name]
        self.need = stream_bytes(O, AS, T * N, B, E)

    def run(self, mode, pad=0):
        """mode: "gather" icrl_ppo_lag_train | "stream" | "short" (a workspace one byte too small) | "null"; returns (state, route words, workspace)"""
        from icrl_amd import _lib
        from icrl_amd.structs import PpoHyperT, p
        pol, ws, b, job = self.agent.policy, self.agent._train_ws, _lib.byref, self.job
        for dst, src in zip((pol.params, pol.exp_avg, pol.exp_avg_sq, ws["t"]), self.state0):
            dst.copy_(src)
        hp = PpoHyperT.from_buffer_copy(job["hp"]); hp._pad |= pad
        head = (b(job["ps"]), p(pol.exp_avg), p(pol.exp_avg_sq), p(ws["t"]), b(job["bs"]), p(job["perms"]), p(ws["nu"]), b(hp), p(ws["stats"]), p(ws["sync"]))
        sws = None
        if mode == "gather":
            _lib.check(_lib.lib().icrl_ppo_lag_train(*head, _lib.current_stream()), "icrl_ppo_lag_train")
        else:
            size = {"stream": self.need, "short": self.need - 1, "null": 0}[mode]
            sws = torch.full((max(size, 16),), 0xA5, dtype=torch.uint8, device="cuda") if mode != "null" else None
            _lib.check(_lib.lib().icrl_ppo_lag_train_stream(*head, p(sws) if sws is not None else None, size, _lib.current_stream()), "icrl_ppo_lag_train_stream")
        torch.cuda.synchronize()
        words = _lib.last_route(_lib.FAMILY_UPDATE)
        state = [t.clone() for t in (pol.params, pol.exp_avg, pol.exp_avg_sq, ws["t"], ws["stats"])]
        assert float(state[4][11]) == 0.0, "inter-workgroup exchange timed out"
        return state, words, sws


def _same_bits(a, b):
    return all(torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y) for x, y in zip(a, b))


def _assert_same(a, b, what):
    for k, x, y in zip(("params", "exp_avg", "exp_avg_sq", "adam_step", "stats"), a, b):
        if k == "stats":      # [0..11] and the per-epoch KLs ([12..31]: phase timers, diagnostic builds only)
            x, y = torch.cat([x[:12], x[32:]]), torch.cat([y[:12], y[32:]])
        assert _same_bits([x], [y]), f"{what}: {k} differs in {int((x != y).sum())} of {x.numel()} entries"
    assert not bool(torch.isnan(a[0]).any())


_cases = {}


def _case(name):      # (one agent per shape, shared by the tests below; its state is restored in front of every call)
    if name not in _cases:
        _cases[name] = _Case(name)
    return _cases[name]


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_prepass_against_numpy(name):
    """every record the pre-pass wrote = the numpy gather of the planes (exact: copies), ragged rows = the chunk's first row, the chunk behind
    the last = the plan's zero entry.  The statistics table against float64 numpy: means to 2e-6 + 2e-5 relative (a tree sum of <= 160 floats of
    magnitude ~2: <= 8 eps sum|x| / n ~ 8e-7), 1 / (std + 1e-8) to 1e-5 relative (the same sums through s_rr - s_r mean, then v_sqrt / v_rcp at
    1 ulp each: ~1e-6); bit for bit they are the in-kernel values, which test_stream_against_gather_bit_for_bit shows through the update."""
    O, A, AS, disc, T, N, B, E = SHAPES[name]
    c = _case(name)
    _, words, sws = c.run("stream")
    assert words[4] == 1 and words[0] == 5
    want = records(c.buf, c.perms, T, N, B, E)
    n_rec = want.size
    got = sws[:4 * n_rec].view(torch.float32).cpu().numpy().reshape(want.shape)
    assert np.array_equal(got, want), f"{int((got != want).sum())} of {want.size} record words differ"
    n_steps = E * (-(-T * N // B))
    off = (4 * n_rec + 255) // 256 * 256
    table = sws[off:off + 16 * (n_steps + 2)].view(torch.float32).cpu().numpy().reshape(n_steps + 2, 4)
    ref = minibatch_stats(c.buf, c.perms, T, N, B, E)
    assert np.allclose(table[:n_steps, 0], ref[:, 0], rtol=2e-5, atol=2e-6) and np.allclose(table[:n_steps, 2], ref[:, 2], rtol=2e-5, atol=2e-6)
    assert np.allclose(table[:n_steps, 1], ref[:, 1], rtol=1e-5, atol=0)
    assert np.array_equal(table[n_steps:], [[0, 1, 0, 0]] * 2) and not table[:, 3].any()


@pytest.mark.parametrize("parts", [4, 2])
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_stream_against_gather_bit_for_bit(name, parts):
    """the same update through icrl_ppo_lag_train and icrl_ppo_lag_train_stream, four and two workgroups per network (hp._pad & 32)."""
    c = _case(name)
    pad = 32 if parts == 2 else 0
    ref, words, _ = c.run("gather", pad)
    assert (words[0], words[1], words[2], words[4]) == (5 if parts == 4 else 4, parts, 1, 0)
    got, words, _ = c.run("stream", pad)
    assert words[4] == 1 and words[0] == (5 if parts == 4 else 4) and words[1] == parts
    E = SHAPES[name][7]
    assert int(got[4][1]) == E * (-(-SHAPES[name][4] * SHAPES[name][5] // SHAPES[name][6])) and int(got[4][0]) == E      # every step ran
    _assert_same(got, ref, f"{name}, {parts} parts")
    assert not _same_bits(got[:1], c.state0[:1])      # (and it did train)


@pytest.mark.parametrize("name", ["hc-b40", "lgw-b64"])
def test_target_kl_stop_in_epoch_0(name):
    """a target KL the first epoch exceeds (old log-probs 0.05 above the policy's: mean KL ~0.05 against 0.01): both forms stop behind epoch 0
    with identical state."""
    c = _Case(name, target_kl=0.01, lp_shift=0.05)
    ref, _, _ = c.run("gather")
    got, words, _ = c.run("stream")
    assert words[4] == 1
    assert int(got[4][0]) == 0 and int(got[4][1]) == -(-SHAPES[name][4] * SHAPES[name][5] // SHAPES[name][6])      # early_stop_epoch 0, one epoch of steps
    _assert_same(got, ref, name)


@pytest.mark.parametrize("mode", ["short", "null"])
def test_fallback_without_room(mode):
    """a workspace one byte too small, or none: the in-kernel gather (route word [4] == 0), same results; the workspace is not touched."""
    c = _case("hc-b40")
    ref, _, _ = c.run("gather")
    got, words, sws = c.run(mode)
    assert words[4] == 0 and words[0] == 5
    _assert_same(got, ref, mode)
    if sws is not None:
        assert bool((sws == 0xA5).all())


_CHILD = ("import sys; sys.path[:0] = [%r, %r]\n"
          "import test_update_stream_gpu as t\nt._python_default(%d)\nprint('CHILD OK')\n")


def _python_default(expect):
    import hashlib
    from icrl_amd import _lib
    agent, _, perms = _make("hc-b64")
    agent.train(perms=perms)
    assert _lib.last_route(_lib.FAMILY_UPDATE)[4] == expect and _lib.last_route(_lib.FAMILY_UPDATE)[0] == 5
    assert ("stream" in agent._train_ws) == bool(expect)
    agent.train(perms=perms[::-1].copy())      # (the workspace is re-used)
    assert _lib.last_route(_lib.FAMILY_UPDATE)[4] == expect
    digest = hashlib.sha256(agent.policy.params.cpu().numpy().tobytes() + agent.policy.exp_avg_sq.cpu().numpy().tobytes()).hexdigest()
    print("PARAMS", digest)
    return digest


def test_python_default_and_switch():
    """PPOLagrangian.train() streams by default; ICRL_UPDATE_STREAM=0 (read once per process: a child) keeps the in-kernel gather; same parameters."""
    mine = _python_default(1)
    here = os.path.dirname(os.path.abspath(__file__))
    out = subprocess.run([sys.executable, "-c", _CHILD % (os.path.dirname(here), here, 0)], env=dict(os.environ, ICRL_UPDATE_STREAM="0"),
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "CHILD OK" in out.stdout, (out.stdout[-2000:], out.stderr[-2000:])
    assert f"PARAMS {mine}" in out.stdout
