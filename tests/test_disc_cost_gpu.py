"""GPU: discriminator costs (gail_utils.DiscriminatorCost / icrl_cost_disc_t, the cost of `cpg --load_gail`) inside the fused rollout
launches — the rows entry point against icrl_disc_reward bit for bit, every launch form against the per-step launches bit for bit, the
per-step cost against icrl_disc_reward on the step's own state, the fused path against the per-step loop over the same object, the
host-env chain, and cpg end to end on the two reference-trained discriminators."""
import ctypes
import types

import numpy as np
import pytest
import torch

import tests.helpers.host_envs  # noqa: F401  (registers the Host* ids)
from helpers import disc_cost_cases as cases, routes
from helpers.disc_cost_cases import BUF_KEYS

pytestmark = pytest.mark.gpu
_WIDE_POLICY = dict(policy_kwargs=dict(net_arch=[dict(pi=[128, 96], vf=[80, 128], cvf=[128, 128])]))


def _sub(g, prefix):
    return {k[len(prefix):]: g[k] for k in g.files if k.startswith(prefix)}


def _forward(desc, obs, acs):
    from icrl_amd import _lib
    from icrl_amd.structs import p
    out = torch.full((obs.shape[0],), -1.0, device="cuda")
    _lib.check(_lib.lib().icrl_cost_mlp_forward(_lib.byref(desc), p(obs), p(acs), obs.shape[0], p(out), _lib.current_stream()), "icrl_cost_mlp_forward")
    return out


# ---- 0. the numpy form against the oracle (a discriminator's parameters live on the device from construction: no CPU test can hold it) ----
def test_numpy_in_gives_the_reference_closures_array(golden):
    from icrl_amd.gail_utils import DiscriminatorCost, GailDiscriminator
    from oracle import gail as o_gail
    g = golden("g12_gail")
    disc = GailDiscriminator(18, 6, [20], None, lambda x: 0.0, None, None, False, clip_obs=20, eps=1e-5)
    disc.load_state_dict(_sub(g, "d1/"))
    od = o_gail.make_disc(18, 6, [20])
    od.load_state_dict(_sub(g, "d1/"))
    cost = DiscriminatorCost(disc)
    got = cost(g["probe_obs"], g["probe_acs"])
    assert isinstance(got, np.ndarray) and got.dtype == np.float32
    want = o_gail.disc_reward(od, g["probe_obs"], g["probe_acs"], apply_log=False)
    assert got.shape == np.asarray(want).shape and np.allclose(got, want, rtol=2e-5, atol=2e-6), np.abs(got - want).max()
    assert np.array_equal(got, disc.reward_function(g["probe_obs"], g["probe_acs"], apply_log=False).cpu().numpy())      # the parent's closure
    dev = cost(torch.as_tensor(g["probe_obs"], device="cuda"), torch.as_tensor(g["probe_acs"], device="cuda"))
    assert torch.is_tensor(dev) and dev.is_cuda and dev.dtype == torch.float32 and np.array_equal(dev.cpu().numpy(), got)
    s = cost.struct()
    assert s.n_hidden == -2 and (s.obs_dim, s.acs_dim, s.in_dim) == (18, 6, 24) and s.net == ctypes.addressof(s._inner)


# ---- 1. rows: icrl_cost_mlp_forward with the descriptor is icrl_disc_reward(apply_log = 0), bit for bit ----------------------------------
def _row_disc(shape):
    return {"hc": lambda: cases.fresh(18, 6, [20], 1), "ant": lambda: cases.fresh(113, 8, [40, 40], 2), "point": cases.load_point,
            "wide": lambda: cases.fresh(18, 6, [128, 128], 4)}[shape]()


@pytest.mark.parametrize("shape", ["hc", "ant", "point", "wide"])
@pytest.mark.parametrize("N", [1, 63, 257])
def test_rows_with_the_descriptor_equal_disc_reward(N, shape):
    from icrl_amd.gail_utils import DiscriminatorCost
    disc = _row_disc(shape)
    rng = np.random.RandomState(N)
    obs = torch.as_tensor(rng.randn(N, disc.obs_dim) * 2.0, device="cuda")
    acs = torch.as_tensor((rng.randn(N, disc.acs_dim) * 0.7).astype(np.float32), device="cuda")
    got, want = _forward(DiscriminatorCost(disc).struct(), obs, acs), cases.disc_reward(disc, obs, acs)
    assert torch.equal(got, want), (got - want).abs().max().item()
    d = got.cpu().numpy()
    assert np.all((d >= 0) & (d <= 1)) and (N == 1 or d.std() > 0)
    cost = _forward(disc.struct(), obs, acs).cpu().numpy()                # the same net as a constraint net: 1 - zeta
    assert np.allclose(d, 1.0 - cost, rtol=0, atol=2e-7)


def test_rows_keep_the_small_discriminator_outputs_that_one_minus_cost_loses():
    """an output layer scaled until the sigmoid saturates on both sides: D < 1e-4 and D > 1 - 1e-4 both occur.  Below 1e-4 a float32
    1 - (1 - D) has lost D's low bits (spacing 6e-8 against D's 7e-12), so only a kernel that stores zeta itself matches."""
    from icrl_amd.gail_utils import DiscriminatorCost
    disc = cases.fresh(18, 6, [20], 6, out_scale=60.0)
    rng = np.random.RandomState(0)
    N = 257
    obs = torch.as_tensor(rng.randn(N, 18) * 3.0, device="cuda")
    acs = torch.as_tensor(rng.randn(N, 6).astype(np.float32), device="cuda")
    got, want = _forward(DiscriminatorCost(disc).struct(), obs, acs), cases.disc_reward(disc, obs, acs)
    d = want.cpu().numpy()
    print(f"D: min {d.min():.3e}, max {d.max():.9f}, {np.sum(d < 1e-4)} below 1e-4, {np.sum(d > 1 - 1e-4)} above 1 - 1e-4")
    assert (d < 1e-4).any() and (d > 1 - 1e-4).any() and (d[d < 1e-4] > 0).any()
    assert torch.equal(got, want)
    negated = np.float32(1.0) - _forward(disc.struct(), obs, acs).cpu().numpy()          # what 1 - (1 - D) would store
    assert not np.array_equal(negated, d)


# ---- 2. every launch form against the per-step launches, bit for bit -------------------------------------------------------------------
# (kind, envs, T, rollout_kernel, hidden sizes | None = the fixture of that env / [20], episode_stats) -> what must have launched
_FORMS = [
    ("hc", 7, 33, "auto", None, False, dict(route="persistent", wgs=7)),
    ("hc", 64, 40, "auto", None, False, dict(route="persistent", wgs=64)),                       # <2, 2>
    ("ant", 32, 10, "auto", None, False, dict(route="persistent", wgs=32)),                      # <8, 10>
    ("hc", 128, 20, "auto", None, False, dict(route="wide", wgs=128)),
    ("ant", 128, 10, "auto", None, False, dict(route="wide", wgs=128)),
    ("hc", 20, 33, "multi", None, False, dict(route="multi", envs_per_wg=4, wgs=5)),             # ragged last workgroup
    ("hc", 64, 40, "multi", None, False, dict(route="multi", envs_per_wg=8, wgs=8)),
    ("ant", 116, 10, "multi", None, False, dict(route="multi", envs_per_wg=4, wgs=29)),          # <8, 8>
    ("antbroken", 4096, 3, "multi", None, False, dict(route="multi", envs_per_wg=16, wgs=256)),
    ("point_circle", 12, 20, "auto", None, False, dict(route="multi")),                          # the Point fixture
    ("hc", 16, 12, "wide-policy", None, False, "generic-persistent"),
    ("hc", 8, 8, "auto", [128, 128], False, dict(route="generic-per-step", launches=32)),        # 4 T launches
    ("lgw", 8, 40, "auto", None, False, "persistent"),                                           # one-hot actions
    ("hc", 7, 33, "auto", None, True, dict(route="persistent", wgs=7)),                          # MON
    ("hc", 20, 33, "multi", None, True, dict(route="multi", envs_per_wg=4, wgs=5)),              # MON
]


def _form_id(f):
    return "-".join(str(x) for x in f[:4]) + ("-" + "x".join(map(str, f[4])) if f[4] else "") + ("-mon" if f[5] else "")


def _assert_identical(a_p, e_p, a_s, e_s, it):
    for k in BUF_KEYS:
        got, ref = getattr(a_p.rollout_buffer, k).cpu().numpy(), getattr(a_s.rollout_buffer, k).cpu().numpy()
        assert np.array_equal(got, ref), (it, k, np.abs(got - ref).max())
    for name in ("obs_rms", "ret_rms", "cost_rms"):
        rp, rs = getattr(e_p, name), getattr(e_s, name)
        assert np.array_equal(np.asarray(rp.mean), np.asarray(rs.mean)) and np.array_equal(np.asarray(rp.var), np.asarray(rs.var)), name
        assert rp.count == rs.count, name
    assert torch.equal(e_p.ret, e_s.ret) and torch.equal(e_p.cost_ret, e_s.cost_ret)
    assert torch.equal(a_p._last_obs, a_s._last_obs) and torch.equal(a_p._ag["last_dones"], a_s._ag["last_dones"])
    assert torch.equal(e_p.unwrapped.s, e_s.unwrapped.s) and torch.equal(e_p.unwrapped.t_ep, e_s.unwrapped.t_ep)
    for k in ("raw_rew", "raw_cost", "dones", "last_v_r", "last_v_c", "act_clipped"):
        assert torch.equal(a_p._ag[k], a_s._ag[k]), k


@pytest.mark.parametrize("kind,N,T,kernel,hidden,mon,route", [pytest.param(*f, id=_form_id(f)) for f in _FORMS])
def test_launch_forms_equal_per_step_launches(kind, N, T, kernel, hidden, mon, route):
    from icrl_amd import _lib
    akw = dict(_WIDE_POLICY) if kernel == "wide-policy" else {}
    if mon:
        akw["episode_stats"] = True
    norm = dict(norm_obs=False, norm_reward=False) if kind == "lgw" else {}
    (a_p, e_p), (a_s, e_s) = cases.pair(N, T, 13, kind, hidden, agent_kwargs=akw, **norm)
    assert a_p._fused_chain() is not None and a_p._fused_rollout_ok("cost", T, a_p.rollout_buffer)
    a_s.rollout_kernel = "steps"
    if kernel != "wide-policy":
        a_p.rollout_kernel = kernel
    limit = e_p.unwrapped.max_steps
    noise = cases.noise(kind, 2, T, N)
    a_p._setup_learn(2 * N * T); a_s._setup_learn(2 * N * T)
    for env in (e_p, e_s):
        env.unwrapped.t_ep.fill_(limit - T // 2)           # every env crosses its time limit inside the first rollout
    generic = kernel == "wide-policy" or hidden == [128, 128]
    for it in range(2):
        a_p.collect_rollouts(e_p, None, a_p.rollout_buffer, T, "cost", noise=noise[it])
        got = routes.check_rollout(route, _form_id((kind, N, T, kernel, hidden, mon)))
        assert got["pick"] & _lib.PICK_DISC and not got["pick"] & routes.PICK_ANALYTIC
        assert bool(got["pick"] & routes.PICK_MON) == (mon and got["route"] not in ("per-step", "generic-per-step"))
        a_s.collect_rollouts(e_s, None, a_s.rollout_buffer, T, "cost", noise=noise[it])
        got = routes.check_rollout(dict(route="generic-per-step", launches=4 * T) if generic else dict(route="per-step", launches=2 * T), "steps")
        assert got["pick"] & _lib.PICK_DISC
        a_p.check_rollout_status()
        _assert_identical(a_p, e_p, a_s, e_s, it)
        assert a_p.rollout_buffer.dones.sum().item() >= (N if it == 0 and kind != "lgw" else 0)
        d = a_p.rollout_buffer.orig_costs
        assert 0.0 <= d.min().item() and d.max().item() <= 1.0 and d.std().item() > 0


# ---- 3. the per-step cost is D on the step's own state -----------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["hc", "ant", "point_circle"])
def test_per_step_cost_is_disc_reward_on_the_steps_state(kind):
    N = 8
    (agent, env), _ = cases.pair(N, 1, 5, kind)
    agent.rollout_kernel = "steps"
    agent._setup_learn(4 * N)
    disc = env.venv.cost_function.disc
    for it in range(3):          # (from the second step on the state is no longer the reset state)
        s_before = env.unwrapped.s.clone()
        agent.collect_rollouts(env, None, agent.rollout_buffer, 1, "cost", noise=cases.noise(kind, 1, 1, N, seed=it)[0])
        got = routes.check_rollout(dict(route="per-step", launches=2), kind)
        assert got["pick"] & 32
        want = cases.disc_reward(disc, s_before, agent._ag["act_clipped"].reshape(N, -1).contiguous())
        assert torch.equal(agent._ag["raw_cost"], want), (it, (agent._ag["raw_cost"] - want).abs().max().item())
        assert torch.equal(agent.rollout_buffer.orig_costs.reshape(-1), want)


# ---- 4. the fused launch against the parent's path: the per-step loop over the same object -----------------------------------------------
def test_fused_rollout_equals_the_stepped_loop_under_the_switch(monkeypatch):
    from icrl_amd import _lib
    from icrl_amd.ppo_lag import PPOLagrangian
    N, T = 8, 64
    (a_f, e_f), (a_s, e_s) = cases.pair(N, T, 11, "hc")
    noise = cases.noise("hc", 2, T, N, seed=3)
    a_f._setup_learn(2 * N * T); a_s._setup_learn(2 * N * T)
    calls = []
    inner = PPOLagrangian._collect_rollouts_stepped

    def counted(self, *a, **k):
        calls.append(self)
        return inner(self, *a, **k)
    monkeypatch.setattr(PPOLagrangian, "_collect_rollouts_stepped", counted)
    for it in range(2):
        a_f.collect_rollouts(e_f, None, a_f.rollout_buffer, T, "cost", noise=noise[it])
        got = routes.check_rollout(dict(route="persistent", wgs=N, launches=1), "fused")
        assert got["pick"] & _lib.PICK_DISC and len(calls) == it
        monkeypatch.setenv("ICRL_DISC_COST_STEPPED", "1")
        assert a_s._fused_chain() is None and not a_s._fused_rollout_ok("cost", T, a_s.rollout_buffer)
        # (a call refused before any launch clears the thread's record: what the stepped loop leaves is then its own — nothing)
        assert _lib.lib().icrl_rollout_collect_batch(0, None, None, None, 0.99, 0.95, 0.99, 0.95, 1, None, 0, None) == 1
        _lib.lib().icrl_clear_error()
        a_s.collect_rollouts(e_s, None, a_s.rollout_buffer, T, "cost", noise=noise[it])
        routes.check_rollout(dict(route="none", launches=0), "the stepped loop calls no rollout entry point")
        assert len(calls) == it + 1 and calls[-1] is a_s
        monkeypatch.setenv("ICRL_DISC_COST_STEPPED", "0")
        assert a_s._fused_chain() is not None
        for k in ("observations", "actions", "rewards", "dones"):      # the policy never reads a cost inside a rollout
            got, ref = getattr(a_s.rollout_buffer, k), getattr(a_f.rollout_buffer, k)
            print(f"[stepped vs fused] rollout {it} {k}: max |diff| {(got - ref).abs().max().item():.3e}")
            assert torch.equal(got, ref), (it, k)
        for k in BUF_KEYS:
            got, ref = getattr(a_s.rollout_buffer, k).cpu().numpy(), getattr(a_f.rollout_buffer, k).cpu().numpy()
            assert np.allclose(got, ref, rtol=2e-5, atol=2e-6), (it, k, np.abs(got - ref).max())
    assert a_s.num_timesteps == a_f.num_timesteps == 2 * N * T


# ---- 5. host envs --------------------------------------------------------------------------------------------------------------------------
def test_host_env_rollout_with_the_descriptor(monkeypatch):
    from icrl_amd import envs
    from icrl_amd.gail_utils import DiscriminatorCost
    from icrl_amd.ppo_lag import PPOLagrangian
    from icrl_amd.vec_env import DummyVecEnv, VecCostWrapper, VecNormalizeWithCost
    N, T, seed = 8, 16, 5
    pairs = []
    for _ in range(2):
        env = VecNormalizeWithCost(VecCostWrapper(DummyVecEnv([envs.spec("HostHCWithPos-v0")] * N)))
        env.set_cost_function(DiscriminatorCost(cases.fresh(18, 6, [20], 3)))
        pairs.append((PPOLagrangian("TwoCriticsMlpPolicy", env, n_steps=T, seed=seed), env))
    (a_h, e_h), (a_s, e_s) = pairs
    a_s.policy.load_state_dict(a_h.policy.state_dict())
    e_s.venv.cost_function.disc.load_state_dict(e_h.venv.cost_function.disc.state_dict())
    noise = cases.noise("hc", 2, T, N)
    a_h._setup_learn(2 * N * T); a_s._setup_learn(2 * N * T)
    for env in (e_h, e_s):
        env.unwrapped.env_method("set_t_ep", 1000 - T // 2)      # every env crosses its time limit inside the first rollout
    stepped = []
    inner = PPOLagrangian._collect_rollouts_stepped

    def counted(self, *a, **k):
        stepped.append(self)
        return inner(self, *a, **k)
    monkeypatch.setattr(PPOLagrangian, "_collect_rollouts_stepped", counted)
    for it in range(2):
        assert a_h._host_rollout_ok("cost", T, a_h.rollout_buffer)
        a_h.collect_rollouts(e_h, None, a_h.rollout_buffer, T, "cost", noise=noise[it])
        assert not stepped
        a_s._collect_rollouts_stepped(e_s, None, a_s.rollout_buffer, T, "cost", noise=noise[it])
        # what tests/test_host_rollout_gpu.py asks of a constraint net (test_host_path_equals_stepped_path_and_alternates): identical
        for k in BUF_KEYS:
            got, ref = getattr(a_h.rollout_buffer, k).cpu().numpy(), getattr(a_s.rollout_buffer, k).cpu().numpy()
            print(f"[host vs stepped] rollout {it} {k}: max |diff| {np.abs(got - ref).max():.3e}")
            assert np.array_equal(got, ref), (it, k, np.abs(got - ref).max())
        for name in ("obs_rms", "ret_rms", "cost_rms"):
            rh, rs = getattr(e_h, name), getattr(e_s, name)
            assert np.array_equal(np.asarray(rh.mean), np.asarray(rs.mean)) and np.array_equal(np.asarray(rh.var), np.asarray(rs.var)) and rh.count == rs.count, name
        assert torch.equal(e_h.ret, e_s.ret) and torch.equal(e_h.cost_ret, e_s.cost_ret)
        assert torch.equal(a_h._last_obs, a_s._last_obs) and torch.equal(e_h.unwrapped.s, e_s.unwrapped.s)
        assert a_h.rollout_buffer.dones.sum().item() == (N if it == 0 else a_s.rollout_buffer.dones.sum().item())
        disc = e_h.venv.cost_function.disc
        rb = a_h.rollout_buffer
        want = cases.disc_reward(disc, rb.orig_observations.reshape(T * N, -1).double().contiguous(),
                                 rb.actions.reshape(T * N, -1).clamp(-1.0, 1.0).contiguous()).reshape(T, N)
        assert np.allclose(rb.orig_costs.cpu().numpy(), want.cpu().numpy(), rtol=2e-5, atol=2e-6)      # D, not 1 - D
        stepped.clear()
    monkeypatch.undo()
    e_h.close(); e_s.close()


# ---- 6. cpg --load_gail end to end ----------------------------------------------------------------------------------------------------------
def _cpg_load_gail(path, extra, monkeypatch):
    from icrl_amd import _lib
    from icrl_amd.cpg import build_parser, cpg
    from icrl_amd.ppo_lag import PPOLagrangian
    stepped, picks = [], []
    inner = PPOLagrangian._collect_rollouts_stepped

    def counted(self, *a, **k):
        stepped.append(1)
        return inner(self, *a, **k)
    monkeypatch.setattr(PPOLagrangian, "_collect_rollouts_stepped", counted)
    launch = PPOLagrangian._rollout_launch

    def recorded(self, job):
        launch(self, job)
        picks.append(routes.rollout())
    monkeypatch.setattr(PPOLagrangian, "_rollout_launch", recorded)
    argv = ["cpg", "--load_gail", "--cn_path", path, *extra, "--n_steps", "64", "-t", "2048", "-ne", "2", "-s", "2", "-v", "0"]
    cfg = vars(build_parser().parse_args(argv)); cfg.update(rank=0, world_size=1, save_dir=None)
    model, hist = cpg(types.SimpleNamespace(**cfg), log=None)
    monkeypatch.undo()
    assert not stepped and model.num_timesteps == 2048
    assert all(r["pick"] & _lib.PICK_DISC for r in picks)
    return model, picks


def test_cpg_load_gail_point_runs_in_the_multi_env_kernel(monkeypatch):
    from oracle import gail as o_gail
    model, picks = _cpg_load_gail(cases.POINT_PT, ["-cosd", "0", "1", "-casd", "-1", "-tei", "PointCircle-v0", "-eei", "PointCircleTestBack-v0", "-nt", "16"], monkeypatch)
    assert len(picks) == 2 and all(r["route"] == "multi" and r["launches"] == 1 for r in picks), picks
    rb = model.rollout_buffer
    sd = torch.load(cases.POINT_PT, map_location="cpu", weights_only=False)["network"]
    od = o_gail.make_disc(9, 2, [40, 40], obs_select_dim=[0, 1], acs_select_dim=[-1])
    od.load_state_dict({k: v.numpy() for k, v in sd.items()})
    prev_obs = rb.orig_observations.cpu().numpy().astype(np.float64)
    clipped = np.clip(rb.actions.cpu().numpy(), -0.25, 0.25)
    ref = o_gail.disc_reward(od, prev_obs, clipped, apply_log=False)
    got = rb.orig_costs.cpu().numpy()
    assert got.shape == ref.shape == (64, 16)
    assert np.allclose(got, ref, rtol=2e-5, atol=2e-6), np.abs(got - ref).max()
    assert 0.0 <= got.min() and got.max() <= 1.0 and got.std() > 0


def test_cpg_load_gail_antbroken_runs_in_the_persistent_kernel(monkeypatch):
    from oracle import gail as o_gail
    model, picks = _cpg_load_gail(cases.ANTBROKEN_PT, ["-tei", "AntWallBroken-v0", "-eei", "AntWallBrokenTest-v0", "-nt", "8"], monkeypatch)
    assert len(picks) == 4 and all(r["route"] == "persistent" and r["launches"] == 1 for r in picks), picks
    rb = model.rollout_buffer
    sd = torch.load(cases.ANTBROKEN_PT, map_location="cpu", weights_only=False)["network"]
    od = o_gail.make_disc(113, 8, [40, 40])
    od.load_state_dict({k: v.numpy() for k, v in sd.items()})
    prev_obs = rb.orig_observations.cpu().numpy().astype(np.float64)
    clipped = np.clip(rb.actions.cpu().numpy(), -1.0, 1.0)
    ref = o_gail.disc_reward(od, prev_obs, clipped, apply_log=False)
    got = rb.orig_costs.cpu().numpy()
    assert got.shape == ref.shape == (64, 8)
    assert np.allclose(got, ref, rtol=2e-5, atol=2e-6), np.abs(got - ref).max()
    assert 0.0 <= got.min() and got.max() <= 1.0 and got.std() > 0
