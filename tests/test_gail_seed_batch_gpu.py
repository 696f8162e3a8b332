"""GPU: the batched discriminator step.  icrl_cn_train_minibatch_batch against icrl_cn_train_minibatch run by run, the GAIL rollout-end
kernels (icrl_gail_unnormalize_batch / icrl_gail_relabel_batch) against the torch expressions of the callback they replace and
icrl_disc_reward, whole batched gail runs against the same runs alone, `icrl --seeds`, and the refusals — all bit for bit."""
import os
import types

import numpy as np
import pytest
import torch

from helpers import routes

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
EXPERT = os.path.join(HERE, "golden/expert_hc.npz")

_BUF_KEYS = ("observations", "orig_observations", "new_observations", "new_orig_observations", "actions", "rewards", "costs",
             "orig_costs", "dones", "log_probs", "reward_values", "cost_values", "reward_advantages", "cost_advantages",
             "reward_returns", "cost_returns")


# ---- 1 / 2. icrl_cn_train_minibatch_batch against icrl_cn_train_minibatch ----------------------------------------------------------------
_NN, _NE, _BS, _ITERS = (70, 200, 129), 150, 64, 3
_FORMS = {"gail": dict(train_gail_lambda=True, no_importance_sampling=True),
          "is_episode": dict(per_step_importance_sampling=False),
          "is_step": dict(per_step_importance_sampling=True)}


def _mb_inputs(hidden, in_obs):
    """three runs' rows on `in_obs` observation columns + 6 action columns, shared expert rows, per-run permutations; made once per shape."""
    rng = np.random.RandomState(5)
    exp_obs, exp_acs = rng.randn(_NE, in_obs), rng.uniform(-1, 1, (_NE, 6)).astype(np.float32)
    runs = []
    for r, nn in enumerate(_NN):
        lengths = np.array([nn // 3, nn // 3, nn - 2 * (nn // 3)])
        size = min(nn, _NE)
        runs.append(dict(obs=rng.randn(nn, in_obs) + 0.3 * r, acs=rng.uniform(-1.2, 1.2, (nn, 6)), lengths=lengths,
                         perms=np.stack([rng.permutation(size) for _ in range(_ITERS)]), seed=40 + r))
    return exp_obs, exp_acs, runs


_INPUTS = {}


def _inputs(hidden, in_obs):
    key = (tuple(hidden), in_obs)
    if key not in _INPUTS:
        _INPUTS[key] = _mb_inputs(hidden, in_obs)
    return _INPUTS[key]


def _make_net(hidden, in_obs, exp_obs, exp_acs, seed, form, lr=0.02, **kw):
    from icrl_amd.constraint_net import ConstraintNet
    torch.manual_seed(seed)
    lo = -np.ones(6, np.float32)
    return ConstraintNet(in_obs, 6, list(hidden), _BS, lambda x: lr, exp_obs, exp_acs, False, 0.5, clip_obs=20, action_low=lo, action_high=-lo,
                         **dict(_FORMS[form], **kw))


def _state(cn, job):
    torch.cuda.synchronize()
    return dict(params=cn.params.cpu().numpy().copy(), exp_avg=cn.exp_avg.cpu().numpy().copy(), exp_avg_sq=cn.exp_avg_sq.cpu().numpy().copy(),
                t=int(job["t_dev"].item()), metrics=job["metrics"].cpu().numpy().copy())


def _solo_and_batch(nets_solo, nets_batch, runs, iters):
    from icrl_amd.gail_utils import launch_disc_trains
    solo = []
    for cn, r in zip(nets_solo, runs):
        job = cn._train_begin(iters[len(solo)], r["obs"], r["acs"], r["lengths"], None, None, 1, r["perms"])
        cn._train_launch(job)                                   # icrl_cn_train_minibatch
        solo.append(_state(cn, job))
    jobs = [cn._train_begin(it, r["obs"], r["acs"], r["lengths"], None, None, 1, r["perms"]) for cn, r, it in zip(nets_batch, runs, iters)]
    for cn, j in zip(nets_batch, jobs):
        j["batch_size"] = cn.batch_size
    launch_disc_trains(nets_batch, jobs)                         # ONE icrl_cn_train_minibatch_batch call
    return solo, [_state(cn, j) for cn, j in zip(nets_batch, jobs)]


def _assert_same_states(batch, solo, tag):
    for r, (b, s) in enumerate(zip(batch, solo)):
        for k in ("params", "exp_avg", "exp_avg_sq", "metrics"):
            assert np.array_equal(b[k], s[k], equal_nan=True), (tag, r, k, np.abs(b[k] - s[k]).max())
        assert b["t"] == s["t"], (tag, r)


@pytest.mark.parametrize("form", list(_FORMS))
@pytest.mark.parametrize("hidden,in_obs", [((20,), 18), ((30, 30), 18)], ids=["20", "30x30"])
def test_minibatch_batch_equals_the_single_run_call_run_by_run(hidden, in_obs, form):
    """Nn = 70, 200, 129 against Ne = 150 at batch_size 64, 3 iterations: 2, 3 and 3 minibatches per iteration whose last ones hold 6, 22
    and 1 rows.  Parameters, both Adam moments, adam_step and every metrics row of every run equal the single-run call's."""
    exp_obs, exp_acs, runs = _inputs(hidden, in_obs)
    assert [-(-min(n, _NE) // _BS) for n in _NN] == [2, 3, 3] and [min(n, _NE) % _BS for n in _NN] == [6, 22, 1]
    mk = lambda: [_make_net(hidden, in_obs, exp_obs, exp_acs, r["seed"], form) for r in runs]
    nets_solo, nets_batch = mk(), mk()
    for a, b in zip(nets_solo, nets_batch):
        assert torch.equal(a.params, b.params)
    solo, batch = _solo_and_batch(nets_solo, nets_batch, runs, [_ITERS] * 3)
    _assert_same_states(batch, solo, form)
    for s, n in zip(solo, _NN):
        assert s["t"] == _ITERS * -(-min(n, _NE) // _BS) and np.all(s["metrics"][:, 17] == 1.0)      # every step ran
    assert not np.array_equal(solo[0]["params"], solo[1]["params"])
    # a batch of one is the single-run call
    one_s, one_b = _solo_and_batch(mk()[1:2], mk()[1:2], runs[1:2], [_ITERS])
    _assert_same_states(one_b, one_s, (form, "batch of one"))
    _assert_same_states(one_b, solo[1:2], (form, "batch of one vs the batch of three"))


def test_minibatch_batch_one_run_stops_early_and_the_iteration_counts_differ():
    """per-step importance sampling; run 1 gets a KL threshold its own update crosses after the first iteration (chosen on the CPU oracle:
    half the KL the oracle measures there), the others none, and run 2 asks for 2 iterations only.  Run 1's stop flag fires at iteration 1
    on the oracle and on the GPU, in the batch as alone; the other runs go on."""
    from oracle import cn as o_cn, nets as o_nets
    hidden, in_obs, form = (20,), 18, "is_step"
    exp_obs, exp_acs, runs = _inputs(hidden, in_obs)
    lo = -np.ones(6, np.float32)

    class Replay:
        def __init__(self, perms):
            self.perms, self.i = perms, 0

        def permutation(self, n):
            p = self.perms[self.i]; self.i += 1
            assert len(p) == n
            return p

    def oracle(r, iters, lr=0.02, **tkl):
        torch.manual_seed(r["seed"])
        orc = o_nets.CostNet(in_obs, 6, list(hidden), False, None, None, 20, lo, -lo)
        init = {k: v.clone() for k, v in orc.state_dict().items()}
        opt = torch.optim.Adam(orc.parameters(), lr=lr, eps=1e-5)
        kw = dict(target_kl_old_new=-1, target_kl_new_old=-1)
        kw.update(tkl)
        m = o_cn.cn_train(orc, opt, iters, orc.prepare(r["obs"], r["acs"]), orc.prepare(exp_obs, exp_acs), r["lengths"], reg_coeff=0.5,
                          per_step=True, batch_size=_BS, rng=Replay(r["perms"]), **kw)
        return m, init
    # the two KLs at the start of iteration 1 (two iterations without a threshold: the last importance-weight pass is iteration 1's)
    probe, _ = oracle(runs[1], 2)
    kl_on, kl_no = float(probe["backward/kl_old_new"]), float(probe["backward/kl_new_old"])
    assert np.isfinite(kl_on) and np.isfinite(kl_no) and max(kl_on, kl_no) > 1e-4, (kl_on, kl_no)
    # half of the larger one: crossed at iteration 1 with a factor 2 to spare (fp32 on the GPU vs torch-CPU moves it by ~1e-6 relative)
    tkl = dict(target_kl_new_old=0.5 * kl_no) if kl_no >= kl_on else dict(target_kl_old_new=0.5 * kl_on)
    assert oracle(runs[1], _ITERS, **tkl)[0]["backward/early_stop_itr"] == 1
    none = dict(target_kl_old_new=-1, target_kl_new_old=-1)
    targets, iters = [none, dict(none, **tkl), none], [_ITERS, _ITERS, 2]

    def mk():
        nets = []
        for r, t in zip(runs, targets):
            torch.manual_seed(r["seed"])
            orc = o_nets.CostNet(in_obs, 6, list(hidden), False, None, None, 20, lo, -lo)      # the oracle's initial weights
            cn = _make_net(hidden, in_obs, exp_obs, exp_acs, r["seed"], form, lr=0.02, **t)
            cn.load_state_dict(orc.state_dict())
            nets.append(cn)
        return nets
    solo, batch = _solo_and_batch(mk(), mk(), runs, iters)
    _assert_same_states(batch, solo, "early stop")
    nb = [-(-min(n, _NE) // _BS) for n in _NN]
    assert list(batch[1]["metrics"][:, 0]) == [0.0, 1.0, 0.0] and batch[1]["t"] == nb[1]            # stopped at iteration 1: one iteration of steps
    assert np.all(batch[0]["metrics"][:, 0] == 0) and batch[0]["t"] == _ITERS * nb[0]
    assert np.all(batch[2]["metrics"][:2, 0] == 0) and batch[2]["t"] == 2 * nb[2]


# ---- 3. the rollout-end kernels ----------------------------------------------------------------------------------------------------------
_ROWS = 132


def _true_cost(name):
    from icrl_amd.true_constraint_net import AnalyticCost
    return {"wall": lambda: AnalyticCost.wall_behind(0.1), "both": lambda: AnalyticCost.wall_behind_and_infront(-0.4, 0.6),
            "torque": lambda: AnalyticCost.torque(0.5), "null": AnalyticCost.null, "NULL": lambda: None}[name]()


def _gail_runs(obs_dim, act_dim, discrete, stats, costs, hidden, learn_cost, eps=1e-8, rows=_ROWS):
    """per run: a discriminator, normalised float32 observations [rows, obs], actions, statistics, rewards and the references — the torch
    expressions of the callback (un-normalise, mean cost) and icrl_disc_reward plus a torch add."""
    from icrl_amd import _lib
    from icrl_amd.gail_utils import GailDiscriminator
    from icrl_amd.structs import p
    from icrl_amd.true_constraint_net import mean_cost
    rng = np.random.RandomState(17 + obs_dim)
    runs = []
    for r, cost in enumerate(costs):
        torch.manual_seed(3 + r)
        disc = GailDiscriminator(obs_dim, 2 if discrete else act_dim, list(hidden), None, lambda x: 0.01, None, None, discrete, eps=1e-5)
        obs = torch.as_tensor(rng.randn(rows, obs_dim).astype(np.float32), device="cuda")
        if discrete:
            acs = torch.as_tensor(rng.randint(0, 2, (rows, 1)).astype(np.float32), device="cuda")
        else:
            acs = torch.as_tensor(rng.uniform(-1.2, 1.2, (rows, act_dim)).astype(np.float32), device="cuda")
        mean = torch.as_tensor(rng.randn(obs_dim) * 0.7, device="cuda") if stats else None
        var = torch.as_tensor(rng.uniform(0.2, 3.0, obs_dim), device="cuda") if stats else None
        rewards = torch.as_tensor(rng.randn(rows).astype(np.float32), device="cuda")
        # ---- references
        raw = obs.double()
        if stats:
            raw = raw * torch.sqrt(var + eps) + mean
        tc = _true_cost(cost)
        ref_mean = 0.0 if tc is None else mean_cost(tc, raw, acs)
        logd = torch.empty(rows, device="cuda")
        s = disc.struct()
        _lib.check(_lib.lib().icrl_disc_reward(_lib.byref(s), p(raw.contiguous()), p(acs), rows, p(logd), 1, _lib.current_stream()), "icrl_disc_reward")
        ref_rewards = rewards + logd if learn_cost else logd.clone()
        runs.append(dict(disc=disc, obs=obs, acs=acs, mean=mean, var=var, eps=eps, rewards=rewards.clone(), tc=tc, ref_raw=raw, ref_mean=ref_mean,
                         ref_rewards=ref_rewards, cost=cost))
    return runs


def _run_gail_kernels(runs, learn_cost, obs_dim, act_store, rows=_ROWS):
    from icrl_amd import _lib
    from icrl_amd.structs import GailJobT, addr, p
    S = len(runs)
    keep, jobs = [], []
    for r in runs:
        r["raw"] = torch.full((rows, obs_dim), float("nan"), dtype=torch.float64, device="cuda")
        r["cost_mean"] = torch.full((1,), float("nan"), dtype=torch.float64, device="cuda")
        ds = r["disc"].struct()
        cs = None if r["tc"] is None else r["tc"].struct(obs_dim, act_store)
        keep += [ds, cs]
        jobs.append(GailJobT(addr(ds), addr(cs), p(r["obs"]), p(r["acs"]), p(r["mean"]), p(r["var"]), r["eps"], p(r["raw"]), p(r["rewards"]),
                             p(r["cost_mean"]), rows, int(learn_cost)))
    arr = (GailJobT * S)(*jobs)
    ws = torch.empty(S * _lib.BATCH_ARGS_BYTES, dtype=torch.uint8, device="cuda")
    L = _lib.lib()
    _lib.check(L.icrl_gail_unnormalize_batch(S, arr, p(ws), ws.numel(), _lib.current_stream()), "icrl_gail_unnormalize_batch")
    _lib.check(L.icrl_gail_relabel_batch(S, arr, p(ws), ws.numel(), _lib.current_stream()), "icrl_gail_relabel_batch")
    torch.cuda.synchronize()


_GAIL_SHAPES = [(18, 6, False, True, (30,)), (18, 6, False, False, (30,)), (113, 8, False, True, (64, 64)), (113, 8, False, False, (64, 64)),
                (1, 1, True, True, (16,)), (18, 6, False, True, (128, 100))]


@pytest.mark.parametrize("learn_cost", [0, 1], ids=["replace", "learn_cost"])
@pytest.mark.parametrize("obs_dim,act_dim,discrete,stats,hidden", _GAIL_SHAPES,
                         ids=["hc-stats", "hc-nostats", "ant-stats", "ant-nostats", "discrete", "hc-wide"])
def test_gail_rollout_end_kernels_equal_the_torch_expressions(obs_dim, act_dim, discrete, stats, hidden, learn_cost):
    """132 rows (not a multiple of 64) at n_runs = 3 and 1: raw_obs (float64), the relabelled rewards and cost_mean equal, bit for bit,
    obs.double() * sqrt(var + eps) + mean, rewards (+)= icrl_disc_reward(raw_obs, actions) and mean_cost of the same AnalyticCost.
    hc-wide: a discriminator of the 64-rows-per-workgroup forward (what a solo run with -dl 128 100 takes).
    ant-stats, run 2: the wall fires in 89 rows, a count at which 89 / 132 and torch's device mean, 89 * (1 / 132), differ in the last place."""
    costs = ("null", "NULL", "null") if discrete else (("wall", "both", "torque") if obs_dim == 18 else ("torque", "NULL", "wall"))
    for n_runs in (3, 1):
        runs = _gail_runs(obs_dim, act_dim, discrete, stats, costs[:n_runs], hidden, learn_cost)
        _run_gail_kernels(runs, learn_cost, obs_dim, 1 if discrete else act_dim)
        fired = []
        for i, r in enumerate(runs):
            assert torch.equal(r["raw"], r["ref_raw"]), (n_runs, i, (r["raw"] - r["ref_raw"]).abs().max().item())
            assert torch.equal(r["rewards"], r["ref_rewards"]), (n_runs, i, (r["rewards"] - r["ref_rewards"]).abs().max().item())
            assert float(r["cost_mean"].item()) == r["ref_mean"], (n_runs, i, r["cost"], float(r["cost_mean"].item()), r["ref_mean"])
            fired.append(r["ref_mean"])
        if not discrete and n_runs == 3:
            live = [m for m, c in zip(fired, costs) if c not in ("null", "NULL")]
            assert all(0.0 < m < 2.0 for m in live), fired            # the closed forms fire in some rows and not in others


@pytest.mark.parametrize("learn_cost", [0, 1], ids=["replace", "learn_cost"])
@pytest.mark.parametrize("obs_dim,act_dim,stats,hidden,rows", [(113, 8, True, (64, 64), 4700), (18, 6, True, (30,), 1100)], ids=["ant-stats-4700", "hc-stats-1100"])
def test_gail_rollout_end_kernels_past_one_grid_pass(obs_dim, act_dim, stats, hidden, rows, learn_cost):
    """the same comparison past the first trip of the kernels' walks.  gail_unnormalize_kernel runs min(blocks, 2048) x 256 threads over
    rows x obs_dim: 4700 x 113 = 531 100 elements are more than the 524 288 of one grid pass, so the first 6812 threads take a second element.
    gail_cost_mean_kernel is one block of 1024 threads over the rows: 4700 rows are five trips with a ragged last one, 1100 rows one full trip
    and 76 threads' second.  Everything else (costs, statistics, references, bit equality, n_runs 3 and 1) as in the 132-row test."""
    assert rows > 1024 and (rows * obs_dim > 2048 * 256) == (obs_dim == 113)
    costs = ("wall", "both", "torque") if obs_dim == 18 else ("torque", "NULL", "wall")
    for n_runs in (3, 1):
        runs = _gail_runs(obs_dim, act_dim, False, stats, costs[:n_runs], hidden, learn_cost, rows=rows)
        _run_gail_kernels(runs, learn_cost, obs_dim, act_dim, rows=rows)
        fired = []
        for i, r in enumerate(runs):
            assert r["raw"].shape == (rows, obs_dim) and r["rewards"].shape == (rows,)
            assert torch.equal(r["raw"], r["ref_raw"]), (n_runs, i, (r["raw"] - r["ref_raw"]).abs().max().item())
            assert torch.equal(r["rewards"], r["ref_rewards"]), (n_runs, i, (r["rewards"] - r["ref_rewards"]).abs().max().item())
            assert float(r["cost_mean"].item()) == r["ref_mean"], (n_runs, i, r["cost"], float(r["cost_mean"].item()), r["ref_mean"])
            fired.append(r["ref_mean"])
        if n_runs == 3:
            live = [m for m, c in zip(fired, costs) if c not in ("null", "NULL")]
            assert all(0.0 < m < 2.0 for m in live), fired            # the closed forms fire in some rows and not in others


# ---- 4. whole runs, batch against solo ---------------------------------------------------------------------------------------------------
_HC = ("-tei", "HCWithPos-v0", "-eei", "HCWithPosTest-v0", "-nt", "4", "-ns", "64", "-bs", "64", "-ne", "2", "-dl", "30", "-lc", "-t", "768", "-ee", "256")
_ANT = ("-tei", "AntWall-v0", "-eei", "AntWallTest-v0", "-nt", "4", "-ns", "32", "-bs", "64", "-ne", "2", "-dl", "30", "-lc", "-t", "256", "-ee", "32")
# -ee counts vectorised env steps (callbacks.py): 3 rollouts of 64 steps are 192 calls, so `-ee 256` never fires in these runs; the cases with
# `-ee 64` evaluate after every rollout (5 stochastic episodes of every run in one launch per trigger)
_EVAL = ("-ee", "64")


def _gcfg(seed, shape=_HC, extra=(), save_dir=None, expert=EXPERT):
    from icrl_amd.gail import build_parser
    argv = ["gail", *shape, "-er", "10", "-ep", expert, "-dlr", "0.003", "-s", str(seed), "-v", "0", *extra]
    cfg = vars(build_parser().parse_args(argv))
    cfg.update(rank=0, world_size=1, save_dir=save_dir)
    if save_dir:
        os.makedirs(save_dir, exist_ok=True)
    return types.SimpleNamespace(**cfg)


@pytest.fixture
def dumps(monkeypatch):
    """logger.dump() clears the scalars of the iteration: keep what every dump held (per Logger, i.e. per run)."""
    from icrl_amd import logger
    orig = logger.Logger.dump

    def dump(self, step=0):
        self.__dict__.setdefault("dumped", []).append(dict(self.name_to_value))
        orig(self, step)
    monkeypatch.setattr(logger.Logger, "dump", dump)


def _logged(lg):
    """the discriminator/*, eval/* and train/* scalars of every log line of a run, and what is left after the last one"""
    keep = lambda d: {k: v for k, v in d.items() if k.split("/")[0] in ("discriminator", "eval", "train")}
    return [keep(d) for d in getattr(lg, "dumped", [])] + [keep(lg.name_to_value)]


def _snap(model, disc, history, logged):
    pol, env, rb = model.policy, model.env, model.rollout_buffer
    torch.cuda.synchronize()
    out = dict(params=pol.params.cpu().numpy().copy(), exp_avg=pol.exp_avg.cpu().numpy().copy(), exp_avg_sq=pol.exp_avg_sq.cpu().numpy().copy(),
               pol_t=int(pol.adam_step), d_params=disc.params.cpu().numpy().copy(), d_exp_avg=disc.exp_avg.cpu().numpy().copy(),
               d_exp_avg_sq=disc.exp_avg_sq.cpu().numpy().copy(), d_t=int(disc.adam_step),
               obs_mean=np.asarray(env.obs_rms.mean).copy(), obs_var=np.asarray(env.obs_rms.var).copy(), obs_count=float(env.obs_rms.count),
               ret=(float(env.ret_rms.mean), float(env.ret_rms.var), float(env.ret_rms.count)),
               history=[dict(h) for h in history], logged=list(logged))
    for k in _BUF_KEYS:
        out["buf/" + k] = getattr(rb, k).cpu().numpy().copy()
    return out


def _solo_gail(cfg):
    """the run alone through gail.setup + learn, with the private streams and the two stream opt-ins a batch gives it."""
    from icrl_amd import gail as G
    from icrl_amd.streams import PrivateStreams
    cfg.streams = PrivateStreams(cfg.seed)
    cfg.eval_noise_from_streams = cfg.disc_perms_from_streams = True
    model, cb, disc, gcb = G.setup(cfg, log=None)
    model.learn(total_timesteps=int(cfg.timesteps), callback=cb)
    G.finish(cfg, model, disc)
    from icrl_amd import logger
    return _snap(model, disc, gcb.history, _logged(logger.Logger.CURRENT))


def _assert_same_gail_run(got, want, tag, evals=True):
    for k in want:
        if k in ("history", "logged"):
            continue
        if isinstance(want[k], np.ndarray):
            assert np.array_equal(got[k], want[k], equal_nan=True), (tag, k)
        else:
            assert got[k] == want[k], (tag, k, got[k], want[k])
    assert len(got["history"]) == len(want["history"]) > 0, tag
    for a, b in zip(got["history"], want["history"]):
        assert a.keys() == b.keys() and "eval/mean_cost" in a and "discriminator/disc_loss" in a, (tag, a.keys(), b.keys())
        for k in a:
            assert a[k] == b[k], (tag, k, a[k], b[k])
    assert len(got["logged"]) == len(want["logged"]) == len(want["history"]) + 1, (tag, len(got["logged"]), len(want["logged"]))
    for i, (a, b) in enumerate(zip(got["logged"], want["logged"])):
        assert a.keys() == b.keys(), (tag, i, a.keys() ^ b.keys())
        for k, v in b.items():
            assert a[k] == v or (v != v and a[k] != a[k]), (tag, i, k, a[k], v)
    lines = want["logged"][:-1]
    assert all("discriminator/disc_loss" in d and "eval/mean_cost" in d for d in lines), [sorted(d) for d in lines]
    assert all(any(k.startswith("train/") for k in d) for d in lines[1:]) and any(k.startswith("train/") for k in want["logged"][-1])
    assert all(("eval/mean_reward" in d) == evals for d in lines), [sorted(d) for d in lines]


def _batch_gail(cfgs):
    from icrl_amd.seed_batch import GailSeedBatch
    sb = GailSeedBatch(cfgs)
    out = sb.learn()
    # the batch's last rollout was ONE launch for all runs (S x 4 envs: one workgroup per env, the whole register file; no cost in a GAIL
    # chain), and so was its last update at HalfCheetah widths (up to 16 runs: the kernel a run alone gets); at AntWall widths the updates
    # go run after run through the single-run call (SeedBatch.per_run_wide_updates: four workgroups per network, minibatches of 64 rows)
    S, ant = len(cfgs), "AntWall" in cfgs[0].train_env_id
    routes.check_rollout(dict(route="persistent-batch", n_runs=S, minw=1, launches=1, wgs=4), "gail batch")
    routes.check_update(dict(kind=6, n_runs=1, wgs_per_network=4) if ant else dict(kind=5, n_runs=S, wgs_per_network=4), "gail batch")
    snaps = []
    for st, (model, disc, history) in zip(sb.states, out):
        snaps.append(_snap(model, disc, history, _logged(st["logger"])))
    return snaps


@pytest.mark.parametrize("extra", [(), ("-dbs", "96"), ("--freeze_gail_weights",), _EVAL, ("-dbs", "96") + _EVAL],
                         ids=["one_batch", "dbs96", "frozen", "one_batch-evals", "dbs96-evals"])
def test_batched_gail_equals_solo_gail(extra, dumps):
    """HCWithPos 4 envs x 64 steps x 3 rollouts, seeds 3, 4, 5 alone and in one batch (with -ee 256 as given, and with evaluations after
    every rollout): policy and
    discriminator parameters and Adam state, all 16 buffer arrays after the last rollout, the running moments, the callback's history and
    the logged discriminator/*, eval/* and train/* scalars are equal."""
    seeds = [3, 4, 5]
    solo = [_solo_gail(_gcfg(s, extra=extra)) for s in seeds]
    batch = _batch_gail([_gcfg(s, extra=extra) for s in seeds])
    assert len({s["params"].tobytes() for s in solo}) == len(seeds)
    for sd, got, want in zip(seeds, batch, solo):
        _assert_same_gail_run(got, want, sd, evals="64" in extra)
        assert len(want["history"]) == 3
        if "--freeze_gail_weights" in extra:
            assert want["d_t"] == 3            # evaluated with a zero learning rate: the steps are counted, the weights stay
        else:
            assert want["d_t"] == 3 * (3 if "-dbs" in extra else 1)            # min(256, expert rows) / 96 -> 3 minibatches


def test_batched_gail_equals_solo_gail_at_ant_widths(dumps):
    """AntWall (113 observations: the updates go run after run, SeedBatch.per_run_wide_updates), 4 envs x 32 steps x 2 rollouts, two seeds."""
    expert = os.path.join(HERE, "golden/expert_ant.npz")
    seeds = [3, 4]
    solo = [_solo_gail(_gcfg(s, _ANT, expert=expert)) for s in seeds]
    batch = _batch_gail([_gcfg(s, _ANT, expert=expert) for s in seeds])
    for sd, got, want in zip(seeds, batch, solo):
        _assert_same_gail_run(got, want, sd)
        assert len(want["history"]) == 2


def test_batched_gail_saves_per_run(tmp_path):
    from icrl_amd import utils
    from icrl_amd.gail_utils import GailDiscriminator
    from icrl_amd.seed_batch import run_gail_seed_batch
    base = vars(_gcfg(0, extra=_EVAL, save_dir=str(tmp_path / "batch")))
    base["seeds"] = [3, 4]
    out = run_gail_seed_batch(utils.seed_configs(base))
    for sd, (model, disc, hist) in zip([3, 4], out):
        d = str(tmp_path / "batch" / f"seed_{sd}")
        for name in ("config.json", "best_model.zip", "train_env_stats.pkl", "gail_discriminator.pt"):
            assert os.path.isfile(os.path.join(d, name)), (sd, name)
        assert os.path.isdir(os.path.join(d, "models"))
        again = GailDiscriminator.load(os.path.join(d, "gail_discriminator.pt"))
        for k, v in disc.state_dict().items():
            assert torch.equal(again.state_dict()[k], v), k


# ---- 5. icrl --seeds ---------------------------------------------------------------------------------------------------------------------
def test_icrl_seeds_end_to_end(tmp_path):
    """`icrl --seeds 0 1` with --cn_batch_size 64 (the constraint-net step through icrl_cn_train_minibatch_batch): both seed_<s> directories
    hold what a single run's save_dir holds, and the last iteration's metrics equal run_seed_batch on the same configs."""
    from icrl_amd import icrl as I, utils
    from icrl_amd.seed_batch import run_seed_batch
    expert = os.path.join(HERE, "golden/expert_lgw.npz")
    argv = ["icrl", "-er", "20", "-ep", expert, "-tei", "LGW-v0", "-eei", "CLGW-v0", "-tk", "0.01", "-cl", "20", "-clr", "0.003",
            "-ft", "1000", "-ni", "2", "-bi", "5", "-dno", "-dnr", "-dnc", "-nt", "2", "--n_steps", "250", "-s", "0",
            "--expert_agent_path", expert, "-v", "0", "--cn_batch_size", "64"]
    got = I.main(argv + ["--seeds", "0", "1", "--save_dir", str(tmp_path / "cli")])
    lgw_batch = (dict(route="persistent-batch", n_runs=2, wgs=2, launches=1, minw=1), dict(kind=5, n_runs=2, wgs_per_network=4))      # Discrete, obs 1
    routes.check_rollout(lgw_batch[0], "icrl --seeds"); routes.check_update(lgw_batch[1], "icrl --seeds")
    for sd in (0, 1):
        d = tmp_path / "cli" / f"seed_{sd}"
        for name in ("config.json", "best_nominal_model.zip", "best_nominal_model_policy.pth", "best_cn_model.pt", "train_env_stats.pkl",
                     "models/icrl_0_itrs/nominal_agent.zip", "models/icrl_0_itrs/cn.pt", "models/icrl_0_itrs/0_train_env_stats.pkl"):
            assert os.path.isfile(str(d / name)), (sd, name)
    base = vars(I.build_parser().parse_args(argv))
    base.update(rank=0, world_size=1, seeds=[0, 1])
    _, want, _ = run_seed_batch(utils.seed_configs(base), 2)
    routes.check_rollout(lgw_batch[0], "run_seed_batch"); routes.check_update(lgw_batch[1], "run_seed_batch")
    assert len(got) == len(want) == 2
    for sd in (0, 1):
        a, b = got[sd][-1], want[sd][-1]
        assert a.keys() == b.keys()
        for k in a:
            if k.startswith("time"):            # time(m), time/fps, time/time_elapsed: the wall clock
                continue
            assert a[k] == b[k] or (a[k] != a[k] and b[k] != b[k]), (sd, k, a[k], b[k])
        assert a["iteration"] == 1 and "backward/cn_loss" in a


# ---- 6. the refusals that need the runs set up ---------------------------------------------------------------------------------------------
def test_gail_seed_batch_refuses_generic_shapes_and_mixed_episode_stats():
    from icrl_amd.seed_batch import GailSeedBatch
    with pytest.raises(ValueError, match="generic-shape path"):
        GailSeedBatch([_gcfg(s, extra=("-pl", "128", "128")) for s in (0, 1)])
    with pytest.raises(ValueError, match="generic-shape path"):
        GailSeedBatch([_gcfg(s, _HC[:-7] + ("-dl", "128", "100", "-lc", "-t", "768", "-ee", "256")) for s in (0, 1)])
    with pytest.raises(ValueError, match="episode_stats"):
        GailSeedBatch([_gcfg(0), _gcfg(1, extra=("--episode_stats",))])
