"""CPU: the dense Two Bridges envs (DD2B / CDD2B / DDCDD2B / C2B / CC2B) and PointTrack.

tests/golden/g24_bridge_env.npz holds what the REFERENCE's own classes (custom_envs/envs/two_bridges.py, envs/point.py under gym's
TimeLimit) returned on a noise and on scripted action sequences per class, and the rows of its `bridges()` cost on CDD2B / CC2B
(tools/gen_bridges_golden.py); tests/helpers/bridge_env.BridgeVecEnv is the numpy definition the GPU tests run over.

Bounds (same float32 actions on both sides; derived in DESIGN §21, none fitted).  k is the index of a step within its episode.
  discrete   positions, dones and the constant rewards (-2, -1, 12) bit for bit: every operation is a correctly rounded add, multiply,
             rint or divide.  The dense reward 10 / sqrt(d2): the reference takes d2 ** (1/2) through libm's pow (glibc documents 1 ulp),
             an implementation may take a correctly rounded sqrt (device: 1 ulp budgeted): the two roots differ by <= 2 ulp, a relative
             2 * 2^-52; the quotient rounds once on either side, 2 * 2^-53 more: relative 3 * 2^-52, asserted as 4 * 2^-52.
  continuous ori bit for bit (one correctly rounded add per step).  x, y: per step cos / sin of two libraries differ by <= 3 ulp(1)
             (device 2, host 1) times |a0| <= 2: 6 * 2^-52; the product rounds on either side, <= ulp(2) = 2^-51; the sum at |x| < 32
             rounds on either side, <= 2^-48; together 24 * 2^-52 < 2^-47, so k * 2^-47 after k steps (a rejected move keeps the old
             error).  Rewards: -2, -1, 250 equal; the dense reward c / dist with c <= 200 and dist >= 1 outside the goal branch has
             |d reward| <= c |d dist| <= 200 * 2 k 2^-47 from the position, plus the relative 4 * 2^-52 of the root, the quotient and the
             factor 20 on a value <= 200: (400 k + 25) * 2^-47.
  PointTrack the Point envs' bounds: ori bit for bit, x / y k * 2^-46, reward 4 k * 2^-46 (no denominator here; the
             track bonus is a decision).
  decisions  (dones, rejections, branches) equal: the fixture records that no decision operand of a continuous or PointTrack sequence
             sits within 1e-9 of its threshold (asserted first), many orders above the position bounds.
"""
import numpy as np
import pytest

from helpers import bridge_env

KINDS = ("point_track", "dd2b", "cdd2b", "ddcdd2b", "c2b", "cc2b")
IDS = {"PointTrack-v0": "point_track", "DD2B-v0": "dd2b", "CDD2B-v0": "cdd2b", "DDCDD2B-v0": "ddcdd2b", "C2B-v0": "c2b", "CC2B-v0": "cc2b"}
SEQS = {k: ("noise", "front", "turn", "ring") if k == "point_track" else ("noise", "script") for k in KINDS}
STEPS = {k: 320 if k == "point_track" else 420 for k in KINDS}
U52, U47, U46 = 2.0 ** -52, 2.0 ** -47, 2.0 ** -46
MARGIN = 1e-9


def episode_step(dones):
    """k[t, n]: the index (1-based) of step t within its episode, from the recorded dones."""
    S, N = dones.shape
    k = np.zeros((S, N), np.int64)
    run = np.zeros(N, np.int64)
    for t in range(S):
        run += 1
        k[t] = run
        run[dones[t]] = 0
    return k


def compare_with_golden(g, kind, seq, obs, rew, done):
    """obs [S, N, O] (after auto-reset), rew, done of some implementation against the recorded reference -> worst fractions of the bounds."""
    p = f"{kind}/{seq}/"
    robs, rrew, rdone = g[p + "obs"], g[p + "rewards"], g[p + "dones"]
    assert obs.shape == robs.shape and rew.shape == rrew.shape
    assert np.array_equal(done, rdone), (kind, seq, np.argwhere(done != rdone)[:4])
    if kind in bridge_env.DISCRETE or seq == "front":
        assert np.array_equal(obs, robs), (kind, seq, np.argwhere(obs != robs)[:4])
        if seq == "front":
            assert np.array_equal(rew, rrew)
            return 0.0, 0.0
        const = np.isin(rrew, (-2.0, -1.0, 12.0))
        assert np.array_equal(rew[const], rrew[const]) and np.isin(rew, (-2.0, -1.0, 12.0)).sum() == const.sum(), (kind, seq)
        er = np.abs(rew - rrew) / (4.0 * U52 * np.abs(rrew))
        assert er.max() <= 1.0, (kind, seq, "dense reward", er.max())
        return 0.0, float(er.max())
    assert float(g[p + "margin"]) >= MARGIN, "a decision operand of the reference sits on a threshold: decisions are not comparable"
    k = episode_step(rdone).astype(np.float64)
    assert np.array_equal(obs[..., 2], robs[..., 2]), (kind, seq, "ori")
    if kind == "point_track":
        assert np.array_equal(obs[..., 3:6], robs[..., 3:6]) and np.array_equal(obs[..., 8], robs[..., 8])
        assert np.array_equal(obs[..., 6:8], obs[..., 0:2])
        ex = np.abs(obs[..., 0:2] - robs[..., 0:2]) / (k[..., None] * U46)
        er = np.abs(rew - rrew) / (4.0 * k * U46)
    else:
        const = np.isin(rrew, (-2.0, -1.0, 250.0))
        assert np.array_equal(rew[const], rrew[const]) and np.isin(rew, (-2.0, -1.0, 250.0)).sum() == const.sum(), (kind, seq)
        ex = np.abs(obs[..., 0:2] - robs[..., 0:2]) / (k[..., None] * U47)
        er = np.abs(rew - rrew) / ((400.0 * k + 25.0) * U47)
    assert ex.max() <= 1.0, (kind, seq, "x / y", ex.max())
    assert er.max() <= 1.0, (kind, seq, "reward", er.max())
    return float(ex.max()), float(er.max())


@pytest.mark.parametrize("kind", KINDS)
def test_helper_env_vs_reference_recording(golden, kind):
    g = golden("g24_bridge_env")
    O, A, max_steps = bridge_env.DIMS[kind]
    for seq in SEQS[kind]:
        acts = g[f"{kind}/{seq}/actions"]
        assert acts.dtype == np.float32 and acts.shape == (STEPS[kind], 3, A)
        env = bridge_env.BridgeVecEnv(3, kind)
        start = np.zeros((3, O))
        if kind == "ddcdd2b":
            start[:, :2] = (3.0, 5.0)
        assert np.array_equal(env.reset(), start)
        obs, rew, done = (np.stack(v) for v in zip(*(env.step(acts[t]) for t in range(acts.shape[0]))))
        compare_with_golden(g, kind, seq, obs, rew, done)
        # only the time limit ends an episode, and the row of an end holds the start position
        assert np.array_equal(np.argwhere(done)[:, 0], np.repeat(np.arange(max_steps - 1, STEPS[kind], max_steps), 3))
        assert np.array_equal(obs[done], np.tile(start[0], (int(done.sum()), 1)))


def test_recorded_sequences_cover_the_field(golden):
    """what the generator asserted, from the recorded arrays: rejections, both bridges, the goal, the x 20 region, the left half."""
    g = golden("g24_bridge_env")
    for kind in ("dd2b", "cdd2b", "ddcdd2b", "c2b", "cc2b"):
        raw = np.concatenate([g[f"{kind}/{s}/raw_obs"].reshape(-1, bridge_env.DIMS[kind][0]) for s in SEQS[kind]])
        rew = np.concatenate([g[f"{kind}/{s}/rewards"].reshape(-1) for s in SEQS[kind]])
        cont = kind in bridge_env.CONTINUOUS
        x, y = raw[:, 0], raw[:, 1]
        assert (rew == -2.0).any() and (rew == -1.0).any() and (rew == (250.0 if cont else 12.0)).any(), kind
        on_lower = ((x > 4) & (x < 8) & (y > 5) & (y < 6)).any()
        assert on_lower == (kind in ("dd2b", "c2b")), kind                  # the constraint closes the lower bridge
        assert ((x > 4) & (x < 8) & (y > 14) & (y < 15)).any(), kind        # the upper one is open to all
        in_water = (x > 4) & (x < 8) & (((y > 0) & (y < 5)) | ((y > 6) & (y < 14)) | ((y > 15) & (y < 20)))
        assert not in_water.any() and x.min() >= 0 and y.min() >= 0 and max(x.max(), y.max()) <= 20, kind
        dense = ~np.isin(rew, (-2.0, -1.0, 12.0, 250.0))
        assert dense.sum() > 50 and (rew[dense] > 0).all() and (x[dense] > 4).all(), kind
        if cont:
            assert (rew[dense] > 10.0).any() and (rew[dense & (y >= 6)] <= 10.0).all(), kind      # 20 x where y < 6, dist >= 1
    r = g["point_track/ring/rewards"]
    assert (r > 1.0).any() and (r < 1.0).any() and (g["point_track/front/rewards"] == 0.0).sum() + (g["point_track/front/rewards"] == 1.0).sum() == r.size


@pytest.mark.parametrize("env_id,kind", [("CDD2B-v0", "cdd2b"), ("CC2B-v0", "cc2b")])
def test_bridges_cost_vs_reference_rows(golden, env_id, kind):
    from icrl_amd.true_constraint_net import BridgesCost
    g = golden("g24_bridge_env")
    cost = BridgesCost(env_id)
    for seq in SEQS[kind]:
        p = f"{kind}/{seq}/"
        prev, acts, want = g[p + "prev_obs"], g[p + "actions"], g[p + "bridges_cost"]
        S, N = want.shape
        got = cost(prev.reshape(S * N, -1), acts.reshape(S * N, -1))
        assert got.shape == (S * N,) and got.dtype == np.int64 and np.array_equal(got, want.reshape(-1)), (env_id, seq)
        assert 0 < want.sum() < S * N
        got3 = cost(prev, acts)                                   # [batch, n_envs, .] in -> [batch, n_envs] out, as the reference
        assert got3.shape == (S, N) and np.array_equal(got3, want)
        if kind == "cdd2b":
            assert np.array_equal(cost(prev.reshape(S * N, -1), acts.reshape(S * N)), want.reshape(-1))      # a flat index vector
    if kind == "cc2b":
        # the continuous quirk (ref: true_constraint_net.py:92-95): only where the move ENDS counts.  From (3.2, 4.6) heading 1 rad by
        # 2 the move enters the constraint rectangle at x = 4 (y ~ 5.85) and ends above it: the env rejects the move, the cost is 0
        ob, ac = np.array([[3.2, 4.6, 0.0]]), np.array([[2.0, 1.0]], np.float32)
        x, y = 3.2 + np.cos(1.0) * 2.0, 4.6 + np.sin(1.0) * 2.0
        assert 4 < x < 8 and y > 6                                # ends in the water above the bridge, through the constraint
        assert cost(ob, ac).tolist() == [0]
        e = bridge_env.BridgeVecEnv(1, "cc2b")
        e.s[0] = ob[0]
        assert e.step(ac)[1][0] == -2.0
        assert cost(np.array([[3.5, 5.5, 0.0]]), np.array([[1.0, 0.0]], np.float32)).tolist() == [1]      # ends inside
        assert cost(np.array([[3.0, 5.0, 0.0]]), np.array([[1.0, 0.0]], np.float32)).tolist() == [1]      # ends on the corner (4, 5) exactly
    torch = pytest.importorskip("torch")
    p = f"{kind}/noise/"
    got = cost(torch.as_tensor(g[p + "prev_obs"]), torch.as_tensor(g[p + "actions"]))      # tensors are converted
    assert isinstance(got, np.ndarray) and np.array_equal(got, g[p + "bridges_cost"])


def test_true_cost_resolver(capsys):
    from icrl_amd import true_constraint_net as T
    assert T.get_true_cost_function("CDD2B-v0") is T.null_cost        # unchanged: the null cost, announced
    assert "Cost function for CDD2B-v0 is not implemented yet" in capsys.readouterr().out
    for env_id, cont in (("CDD2B-v0", False), ("CC2B-v0", True)):
        c = T.true_cost_for(env_id)
        assert isinstance(c, T.BridgesCost) and c.continuous is cont and not isinstance(c, T.AnalyticCost)
        assert env_id not in T.TRUE_COSTS
    assert capsys.readouterr().out == ""
    wall = T.true_cost_for("HCWithPosTest-v0")
    assert isinstance(wall, T.AnalyticCost) and wall.name == "wall_behind" and wall.lo == -3
    assert T.true_cost_for("DD2B-v0") is T.null_cost and T.true_cost_for("C2B-v0") is T.null_cost
    with pytest.raises(ValueError, match="BridgesCost"):
        T.BridgesCost("DD2B-v0")


def test_env_tables():
    from icrl_amd import envs
    for env_id, kind in IDS.items():
        assert envs.ENV_IDS[env_id] == (kind, False, False)      # none ends an episode early
        with pytest.raises(ValueError, match="device-resident"):
            envs.register(env_id, "m:a")
    for env_id in ("TwoBridges-v0", "D2B-v0", "PointBridge-v0", "CDD3B-v0"):      # not served
        assert env_id not in envs.ENV_IDS


def test_vec_env_tables_and_spaces():
    torch = pytest.importorskip("torch")
    from icrl_amd import spaces, vec_env
    for kind in KINDS:
        O, A, ms = bridge_env.DIMS[kind]
        assert vec_env.KINDS[kind] == (O, A, ms, bridge_env.FORMS[kind])
        B = vec_env.dynamics_matrix(kind)
        assert B.shape == (O, A) and not B.any()
    assert [vec_env.KINDS[k][3] for k in ("hc", "ant", "lgw", "clgw", "point_circle", "point_null_test")] == [0, 1, 2, 3, 4, 8]
    assert {k: vec_env.DISCRETE_ACTIONS[k] for k in bridge_env.DISCRETE} == {"dd2b": 4, "cdd2b": 4, "ddcdd2b": 4}
    for env_id, kind in IDS.items():
        O, A, ms = bridge_env.DIMS[kind]
        env = vec_env.HipSynthVecEnv.make(env_id, 3, device="cpu")      # (construction allocates only: no kernel is launched)
        assert (env.obs_dim, env.act_dim, env.max_steps, env.reward_form) == (O, A, ms, bridge_env.FORMS[kind])
        assert env.wall_terminate is False and env.broken is False
        assert env.B.shape == (O, A) and not env.B.any() and env.s.dtype == torch.float64
        a, o = env.action_space, env.observation_space
        h = bridge_env.BridgeVecEnv(3, kind)
        if kind in bridge_env.DISCRETE:
            assert isinstance(a, spaces.Discrete) and a.n == 4 and h.action_low is None
            assert o.shape == (2,) and o.dtype == np.float32 and (o.low == 0).all() and (o.high == 20).all()
        elif kind in bridge_env.CONTINUOUS:
            assert a.shape == (2,) and a.dtype == np.float32 and (a.low == -2).all() and (a.high == 2).all()
            assert o.shape == (3,) and o.dtype == np.float32 and (o.low == 0).all() and o.high.tolist() == [20.0, 20.0, np.inf]
            assert np.array_equal(h.action_low, a.low) and np.array_equal(h.action_high, a.high)
        else:
            assert a.shape == (2,) and a.dtype == np.float32 and (a.low == np.float32(-0.25)).all() and (a.high == np.float32(0.25)).all()
            assert o.shape == (9,) and o.dtype == np.float64 and np.isinf(o.low).all() and np.isinf(o.high).all()
            assert np.array_equal(h.action_low, a.low) and np.array_equal(h.action_high, a.high)
