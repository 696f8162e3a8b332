"""Several independent ICRL runs (seeds) sharing ONE GPU — inside the launches.

One run occupies 3 CUs during its PPO-Lagrangian update (the three persistent workgroups of icrl_ppo_lag_train) and one
workgroup per environment during a rollout: 1-25 % of an MI355X.  north_star: "independent seeds ... fan out"; the reference runs
seeds as separate processes (README.md:14-21).  Here S runs of one configuration advance in lock-step from ONE host thread and
every phase of an outer iteration is ONE launch (sequence) whose grid carries all runs, run = blockIdx.y:

    rollouts    icrl_rollout_collect_batch   grid (envs, S) persistent workgroups + the dual GAE of all runs, grid (tiles x C, S)
    update      icrl_ppo_lag_train_batch     grid (3, S): 3 S persistent workgroups, each run a chain of dependent optimiser steps
    sampling    icrl_sample_episodes_batch   grid (episodes, S)
    backward    icrl_cn_train_batch          4 launches per constraint-net iteration, grid.y = S (--cn_batch_size: icrl_cn_train_minibatch_batch,
                                             2 + 4 launches per minibatch)
    evaluation  icrl_sample_episodes_batch, the KL metrics per run (small launches)

The host work between the launches is the per-run bookkeeping of the reference's loop (icrl_amd/icrl.py: the same methods, split
into begin / launch / end) plus ONE device->host copy per phase that brings back every run's scalars.  Each run keeps its own
random streams (icrl_amd/streams.py), logger, env stacks, buffers and networks, so it computes exactly what it computes alone
(tests/test_seed_batch_gpu.py: bit-identical parameters, statistics and metrics).

Co-residency: the persistent kernels wait for the other workgroups of the SAME run only.  Workgroups are dispatched x-fastest, so
the runs of a grid become resident oldest first and a run that does not fit yet starts when earlier ones have finished; the
phases are not mixed (no update workgroup ever competes with rollout workgroups for a CU), which is why no admission control
is needed.  Nothing else may occupy the GPU's CUs for long while a batch runs (include/icrl_hip.h: co-residency precondition).
"""
import os
import ctypes
import time

import numpy as np
import torch

from . import _lib, exploration, logger, utils
from .streams import PrivateStreams
from .structs import CnTrainJobT, CostFnT, MonitorT, PpoTrainJobT, RolloutJobT, SampleJobT, addr, p
from .true_constraint_net import mean_cost
from .vec_env import ENV_IDS, HostVecEnv, sync_envs_normalization


def _refuse_host_envs(*env_ids):
    host = [i for i in env_ids if i not in ENV_IDS]
    if host:
        raise ValueError(f"seed batch: {host} are not device-resident envs (vec_env.ENV_IDS); the batched launches step device envs only — "
                         "run host envs (--env_module) one run at a time")


def setup_runs(configs, on_setup=None):
    """icrl.setup() for every config, one after the other (the constructors seed the process-wide generators); each run gets
    its own PrivateStreams unless the config already carries a `streams` object, and its own scalar log."""
    from . import icrl as I
    states = []
    for cfg in configs:
        _refuse_host_envs(cfg.train_env_id, cfg.eval_env_id)
        if getattr(cfg, "streams", None) is None:
            cfg.streams = PrivateStreams(cfg.seed, discrete=cfg.train_env_id in ("LGW-v0", "CLGW-v0"))
        if getattr(cfg, "warmup_timesteps", None) is not None and not hasattr(cfg.streams, "rollout_noise"):
            raise ValueError("seed batch: every run needs its own random streams")
        logger.configure()
        st = I.setup(cfg)
        st["logger"] = logger.Logger.CURRENT
        if on_setup is not None:
            on_setup(st)
        states.append(st)
    torch.cuda.synchronize()
    return states


class _as_run:
    """per-run context of the shared host thread: the run's scalar log is the current one."""

    def __init__(self, st):
        self.st = st

    def __enter__(self):
        self.prev = logger.Logger.CURRENT
        logger.Logger.CURRENT = self.st["logger"]

    def __exit__(self, *exc):
        logger.Logger.CURRENT = self.prev


def _jobs(cls, rows):
    arr = (cls * len(rows))()
    for i, r in enumerate(rows):
        arr[i] = cls(*r)
    return arr


# The placement calibration of a run's exchange workspace (8 short update launches, PPOLagrangian._tune_sync_placement) pays for a run
# that owns the GPU; in a batch the 3 S update workgroups sit on CUs all over the chip and the timed difference disappears — see the
# measurement next to the switch's use in DESIGN.md section 9.  ICRL_SEED_TUNE=1 restores the per-run calibration.
TUNE_PLACEMENT_IN_BATCH = os.environ.get("ICRL_SEED_TUNE", "0") == "1"


def launch_trains(agents, jobs, args_ws):
    """the updates of several runs (jobs: each agent's PPOLagrangian._train_begin) as ONE icrl_ppo_lag_train_batch launch; every run brings its
    own hyper-parameter block.  args_ws: device bytes, _lib.BATCH_ARGS_BYTES per run."""
    rows = []
    for a, j in zip(agents, jobs):
        ws = a._train_ws
        if not ws["sync_tuned"]:          # first update of the run: where its exchange workspace is fastest (PPOLagrangian._tune_sync_placement)
            if not TUNE_PLACEMENT_IN_BATCH and len(jobs) > 1:
                a.tune_sync_placement = False
            a._tune_sync_placement(j)
        rows.append((addr(j["ps"]), p(a.policy.exp_avg), p(a.policy.exp_avg_sq), p(ws["t"]), addr(j["bs"]), p(j["perms"]), p(ws["nu"]), addr(j["hp"]),
                     p(ws["stats"]), p(ws["sync"])))
    arr = _jobs(PpoTrainJobT, rows)
    _lib.check(_lib.lib().icrl_ppo_lag_train_batch(len(jobs), arr, p(args_ws), args_ws.numel(), _lib.current_stream()), "icrl_ppo_lag_train_batch")


def _eval_callbacks(cb):
    """the EvalCallbacks inside a callback (a CallbackList is walked), in call order."""
    from .callbacks import CallbackList, EvalCallback
    if isinstance(cb, EvalCallback):
        return [cb]
    if isinstance(cb, CallbackList):
        return [e for c in cb.callbacks for e in _eval_callbacks(c)]
    return []


def _gail_callbacks(cb):
    """the GailCallbacks inside a callback (a CallbackList is walked), in call order."""
    from .callbacks import CallbackList
    from .gail_utils import GailCallback
    if isinstance(cb, GailCallback):
        return [cb]
    if isinstance(cb, CallbackList):
        return [g for c in cb.callbacks for g in _gail_callbacks(c)]
    return []


def _refuse_cost_spec(c):
    if getattr(c, "cost_spec", None) is not None:
        raise ValueError("seed batch: --cost_spec (cost_spec) makes the ground-truth cost a RegionCost, and the batched rollout kernels and "
                         "rollout-end launches have no region form (single runs evaluate it inside their fused launches); a batch takes the "
                         "env id's ground-truth cost")


class SeedBatch:
    # observations of 65..128 (AntWall: 113): a run alone updates with FOUR workgroups per network (csrc/ppo_train_quarters*.hip), the
    # batched grid has the row-owning kernel only, whose partial sums associate differently — a batched run would no longer compute
    # what it computes alone.  The drivers that promise exactly that (cpg, gail) set this: the single-run launch of every run, back to
    # back on the stream (no host wait in between).
    per_run_wide_updates = False

    def __init__(self, configs=None, states=None, on_setup=None):
        if states is None:      # refused before anything is set up
            from .icrl import refuse_cn_saliency
            configs = list(configs)
            for c in configs:
                _refuse_cost_spec(c)
                refuse_cn_saliency(c, seed_batch=True)
                exploration.refuse_batched(c, seed_batch=True)
                exploration.refuse_sde(c, seed_batch=True)
        self.states = setup_runs(configs, on_setup) if states is None else states
        if any(isinstance(st["train_env"].unwrapped, HostVecEnv) for st in self.states):
            _refuse_host_envs(*[st["config"].train_env_id for st in self.states])
        c0 = self.states[0]["config"]
        for st in self.states[1:]:
            c = st["config"]
            # everything a batched launch takes from run 0 only: the grids' shapes, and the discounting of the batched GAE
            # (icrl_rollout_collect_batch takes the four gamma / lambda values as scalars)
            same = ("train_env_id", "eval_env_id", "num_threads", "n_steps", "batch_size", "n_epochs", "forward_timesteps", "expert_rollouts",
                    "backward_iters", "cn_batch_size", "cn_layers", "n_iters", "reward_gamma", "reward_gae_lambda", "cost_gamma", "cost_gae_lambda")
            diff = [k for k in same if getattr(c, k) != getattr(c0, k)]
            if diff:
                raise ValueError(f"seed batch: the runs of a batch share every grid; they differ in {diff}")
        if any(st["agent"].policy.wide or int(st["agent"].batch_size) > 256 or getattr(st["constraint_net"], "wide", False) for st in self.states):
            raise ValueError("seed batch: hidden widths above 64 / batch sizes above 256 run on the generic-shape path, which has no batched form")
        if any(st.get("world", 1) > 1 for st in self.states):
            # outer_iteration() below has no per-iteration all-reduce and no rank-0 guard on the saves: a seed batch is a one-rank matter
            raise ValueError("seed batch: the runs of a batch live on ONE rank (launch the batch per GPU; world_size > 1 states would skip the collective)")
        S = len(self.states)
        self.dev = self.states[0]["agent"].device
        self.args_ws = torch.empty(2 * S * _lib.BATCH_ARGS_BYTES, dtype=torch.uint8, device=self.dev)

    # ---- one device->host copy for all runs --------------------------------------------------------------------------------
    @staticmethod
    def _to_host(rows):
        return torch.stack([r.reshape(-1) for r in rows]).cpu().numpy()

    # ---- the batched launches ------------------------------------------------------------------------------------------------
    def _ws(self):
        return p(self.args_ws), self.args_ws.numel()

    def _launch_rollouts(self, agents, jobs):
        a0 = agents[0]
        arr = _jobs(RolloutJobT, [(addr(j["env"]), addr(j["nm"]), addr(j["pol"]), addr(j["cn"]), addr(j["buf"]), addr(j["ag"]), p(j["noise"])) for j in jobs])
        L = _lib.lib()
        ws, nbytes = self._ws()
        mons = [a._mon for a in agents]
        marr = None
        if any(m is not None for m in mons):      # episode statistics: one icrl_monitor_t per run (all runs or none: the kernels are one grid)
            if any(m is None for m in mons):
                raise ValueError("seed batch: episode_stats must be on in every run of a batch or in none")
            marr = (MonitorT * len(mons))(*[m["struct"] for m in mons])
        if any(isinstance(j["cn"], CostFnT) for j in jobs):      # analytic costs (cpg against the ground-truth or the null cost): their entry point
            err = L.icrl_rollout_collect_batch_cost(len(jobs), arr, marr, p(a0._alow), p(a0._ahigh), float(a0.reward_gamma), float(a0.reward_gae_lambda),
                                                    float(a0.cost_gamma), float(a0.cost_gae_lambda), 1, ws, nbytes, _lib.current_stream())
        elif marr is not None:
            err = L.icrl_rollout_collect_batch_mon(len(jobs), arr, marr, p(a0._alow), p(a0._ahigh), float(a0.reward_gamma), float(a0.reward_gae_lambda),
                                                   float(a0.cost_gamma), float(a0.cost_gae_lambda), 1, ws, nbytes, _lib.current_stream())
        else:
            err = L.icrl_rollout_collect_batch(len(jobs), arr, p(a0._alow), p(a0._ahigh), float(a0.reward_gamma), float(a0.reward_gae_lambda),
                                               float(a0.cost_gamma), float(a0.cost_gae_lambda), 1, ws, nbytes, _lib.current_stream())
        if err == 1 and b"batched form" in L.icrl_last_error():       # shapes without a batched persistent kernel: one launch per run
            L.icrl_clear_error()
            for a, j in zip(agents, jobs):
                a._rollout_launch(j)
            return
        _lib.check(err, "icrl_rollout_collect_batch")

    def _launch_trains(self, agents, jobs):
        if self.per_run_wide_updates and agents[0].policy.obs_dim > 64 and len(agents) > 1:
            for a, j in zip(agents, jobs):
                if not a._train_ws["sync_tuned"] and not TUNE_PLACEMENT_IN_BATCH:
                    a.tune_sync_placement = False
                a._train_launch(j)
            return
        launch_trains(agents, jobs, self.args_ws)

    def _launch_episodes(self, runs):
        r0 = runs[0]
        arr = _jobs(SampleJobT, [(addr(r.e), addr(r.nm), addr(r.ps), p(r.noise), p(r.row0), r.rows, 0, p(r.out["orig_obs"]), p(r.out["obs"]),
                                  p(r.out["actions"]), p(r.out["ep_rewards"]), p(r.out["ep_lengths"])) for r in runs])
        ws, nbytes = self._ws()
        _lib.check(_lib.lib().icrl_sample_episodes_batch(len(runs), arr, p(r0.lo), p(r0.hi), r0.eps_per, r0.rows_per, int(r0.deterministic), 1,
                                                         ws, nbytes, _lib.current_stream()), "icrl_sample_episodes_batch")

    def _launch_cn_trains(self, nets, jobs):
        rows = []
        for cn, j in zip(nets, jobs):
            rows.append((addr(j["s"]), p(cn.exp_avg), p(cn.exp_avg_sq), p(j["t_dev"]), p(j["nominal"]), p(j["expert"]), j["nominal"].shape[0],
                         j["expert"].shape[0], p(j["d_off"]), p(j["d_rowep"]), j["n_ep"], 0, addr(j["hp"]), p(j["work"]), p(j["metrics"])))
        arr = _jobs(CnTrainJobT, rows)
        ws, nbytes = self._ws()
        _lib.check(_lib.lib().icrl_cn_train_batch(len(jobs), arr, ws, nbytes, _lib.current_stream()), "icrl_cn_train_batch")

    def _prefetch_permutations(self, agents, after=None):
        """`after`: an event recorded on the main stream BEFORE the update launch — the side stream waits for that point only, so the
        sorts run beside the update kernels (3 S busy CUs) instead of behind them.  (The draws' order is the host's call order: the
        Philox offset of the generator advances on the host.)"""
        if getattr(self, "_side", None) is None:
            self._side = torch.cuda.Stream()
        if after is not None:
            self._side.wait_event(after)
        else:
            self._side.wait_stream(torch.cuda.current_stream())
        for a in agents:
            s_ = a.streams
            if s_ is not None and hasattr(s_, "prefetch_permutations"):
                s_.prefetch_permutations(a.n_epochs, a.rollout_buffer.buffer_size * a.rollout_buffer.n_envs, self._side)

    # ---- phases ----------------------------------------------------------------------------------------------------------------
    def _learn(self, total_timesteps, callbacks=None, prefetch_across_end=None, prefetch=True):
        """PPOLagrangian.learn(total_timesteps, cost_function="cost", callback=callbacks[i]) of every run (ref: on_policy_algorithm.py:430-492),
        rollouts and updates in lock-step.  A run's callback gets the calls learn() makes, in its order: init_callback, on_training_start,
        then per rollout on_rollout_start (before the noise draw), on_steps(n_steps), on_rollout_end (both after the launch, before the log
        line is dumped), and on_training_end.  EvalCallbacks inside it only note their triggers during on_steps; the episodes of all runs
        then go through ONE launch per trigger (_evaluations) and every callback records its own results before on_rollout_end.
        GailCallbacks inside it do their rollout-end work in lock-step as well (_gail_rollout_ends), before the other callbacks' on_rollout_end.
        prefetch=False: no permutations are drawn ahead (a GailCallback draws the discriminator's permutation from the same generator between
        two updates: the draws must keep the order of the run alone)."""
        sts = self.states
        agents = [st["agent"] for st in sts]
        cbs = list(callbacks) if callbacks is not None else [None] * len(sts)
        evals = [_eval_callbacks(cb) for cb in cbs]
        gails = [_gail_callbacks(cb) for cb in cbs]
        if len({len(e) for e in evals}) != 1 or len({len(g) for g in gails}) != 1:
            raise ValueError("seed batch: every run of a batch carries the same callbacks")
        if prefetch_across_end is None:      # ICRL: not when the constraint net draws minibatch permutations from the same generator after learn()
            prefetch_across_end = all("constraint_net" in st and st["constraint_net"].batch_size is None for st in sts)
        totals = []
        for st, a, cb, ev in zip(sts, agents, cbs, evals):
            with _as_run(st):
                totals.append(a._setup_learn(total_timesteps, True))
                if not a._fused_rollout_ok("cost", a.n_steps, a.rollout_buffer):
                    raise ValueError("seed batch: the env chain must be the device-native stack with a ConstraintNet or an AnalyticCost (the fused rollout)")
                for e in ev:
                    e.deferred = []
                if cb is not None:
                    cb.init_callback(a)
                    cb.on_training_start({}, {})
        iteration = 0
        while agents[0].num_timesteps < totals[0]:
            jobs = []
            for st, a, cb in zip(sts, agents, cbs):
                with _as_run(st):
                    jobs.append(a._rollout_begin(cb, a.rollout_buffer, a.n_steps, None, zero_buffer=False))      # (calls on_rollout_start)
            self._launch_rollouts(agents, jobs)
            iteration += 1
            for i, (st, a, j, cb) in enumerate(zip(sts, agents, jobs, cbs)):
                with _as_run(st):
                    a._rollout_end(j, a.env, None, a.rollout_buffer, a.n_steps)
                    if cb is not None and cb.on_steps(a.n_steps) is False:
                        raise ValueError(f"seed batch: a callback of run {i} asked to stop training; the runs of a batch stop together, at total_timesteps")
            self._evaluations(evals)
            self._gail_rollout_ends(gails)
            tjobs = []
            for st, a, j, cb in zip(sts, agents, jobs, cbs):
                with _as_run(st):
                    if cb is not None:
                        cb.on_rollout_end()
                    a._current_progress_remaining = 1.0 - float(a.num_timesteps) / float(totals[0])
                    a._training_infos(iteration)
                    logger.dump(step=a.num_timesteps)
                    tjobs.append(a._train_begin(None))
            before_update = torch.cuda.Event()
            before_update.record()
            self._launch_trains(agents, tjobs)
            # while the updates run (3 S CUs busy, the host idle): the permutations of the NEXT update, on a side stream — their sorts
            # were ~5 ms of device time + ~7 ms of launches per update phase at S = 32, in front of the update launch.  Not across the end
            # of the forward step when the constraint net draws minibatch permutations from the same generator in between.
            more = agents[0].num_timesteps < totals[0]
            if prefetch and (more or prefetch_across_end):
                self._prefetch_permutations(agents, after=before_update)
            host = self._to_host([a.train_readback() for a in agents])          # waits for the update of every run
            for st, a, j, h in zip(sts, agents, tjobs, host):
                with _as_run(st):
                    a._train_end(j, host=h)
        for st, a, cb, ev in zip(sts, agents, cbs, evals):
            with _as_run(st):
                a._training_infos(iteration + 1)
                if cb is not None:
                    cb.on_training_end()
                for e in ev:
                    e.deferred = None
        for gs in gails:
            for g in gs:
                g.batched = False

    def _gail_rollout_ends(self, gails):
        """the rollout ends of the runs' GailCallbacks in lock-step: begin per run (statistics, the permutation draw), the device part of all
        runs through the batched entry points (gail_utils.launch_rollout_ends: un-normalise, discriminator iteration, relabel, dual GAE), ONE
        device->host copy with every run's metrics, mean cost and Adam step, end per run (discriminator/*, eval/mean_cost, history).
        The callbacks' own on_rollout_end is then a no-op (`batched`)."""
        from .gail_utils import launch_rollout_ends
        sts = self.states
        for slot in range(len(gails[0])):
            gs = [g[slot] for g in gails]
            jobs = []
            for st, g in zip(sts, gs):
                with _as_run(st):
                    g.batched = True
                    jobs.append(g._rollout_end_begin())
            if len({j["update"] for j in jobs}) != 1:
                raise ValueError("seed batch: the runs' discriminators update at different rollouts (update_freq differs)")
            launch_rollout_ends(gs, jobs, self.args_ws)
            host = self._to_host([j["readback"] for j in jobs])
            for st, g, j, h in zip(sts, gs, jobs, host):
                with _as_run(st):
                    g._rollout_end_finish(j, h)

    def _evaluations(self, evals):
        """the triggers the runs' EvalCallbacks noted during on_steps: per trigger ONE launch with the evaluation episodes of every run
        (_episodes), then each callback records its rewards and lengths (logs, best model, callback_on_new_best) as of the triggering
        call.  evals[i]: the EvalCallbacks of run i, the same number in every run."""
        sts = self.states
        for slot in range(len(evals[0])):
            es = [ev[slot] for ev in evals]
            if len({(tuple(e.deferred), e.n_eval_episodes, bool(e.deterministic)) for e in es}) != 1:
                raise ValueError("seed batch: the runs' EvalCallbacks trigger at different calls (eval_freq / n_eval_episodes / deterministic differ)")
            for call, ts in list(es[0].deferred):
                noises = []
                for st, e in zip(sts, es):
                    sync_envs_normalization(e.training_env, e.eval_env)
                    noises.append(e.draw_noise())
                runs, rewards = self._episodes([e.eval_env for e in es], es[0].n_eval_episodes, es[0].deterministic, noises, False)
                for st, e, r, rw in zip(sts, es, runs, rewards):
                    with _as_run(st):
                        end = e.n_calls, e.num_timesteps
                        e.n_calls, e.num_timesteps = call, ts
                        e.record(*utils.evaluate_result(r, rw, return_episode_rewards=True))
                        e.n_calls, e.num_timesteps = end
            for e in es:
                e.deferred = []

    def _episodes(self, envs, n_episodes, deterministic, noises, parallel):
        """n_episodes of the 1-env loop of every run (utils.EpisodeRun) in one launch; runs whose speculation failed repeat
        sequentially (one more batched launch for those)."""
        sts = self.states
        runs = [utils.EpisodeRun(st["agent"], env, n_episodes, deterministic, noise, parallel) for st, env, noise in zip(sts, envs, noises)]
        bases = self._to_host([r.senv.step_count[:1].to(torch.int64) for r in runs])[:, 0]
        for r, b in zip(runs, bases):
            r.prepare(base=int(b))
        todo = list(range(len(runs)))
        rewards = [None] * len(runs)
        dbg = os.environ.get("ICRL_SEED_DEBUG")
        while todo:
            if dbg:
                torch.cuda.synchronize(); t_dbg = time.time()
            sub = [runs[i] for i in todo]
            if len({r.n_streams for r in sub}) == 1:
                self._launch_episodes(sub)
            else:
                for r in sub:
                    r.launch()
            host = self._to_host([torch.cat([r.out["ep_lengths"].double(), r.out["ep_rewards"]]) for r in sub])
            again = []
            for i, r, h in zip(todo, sub, host):
                if r.finish(h[:n_episodes]):
                    rewards[i] = h[n_episodes:].copy()
                else:           # an episode ended early: the run repeats with the positions the measured lengths imply
                    r.prepare()
                    again.append(i)
            if dbg:
                torch.cuda.synchronize()
                print(f"[episodes] pass over {len(todo)} run(s), streams {sorted({r.n_streams for r in sub})}: {1e3 * (time.time() - t_dbg):.1f} ms, {len(again)} to repeat", flush=True)
            todo = again
        return runs, rewards

    def outer_iteration(self, itr):
        """icrl.outer_iteration (ref: icrl/icrl.py:199-304) for every run: the same calls in the same order per run, each phase
        issued for all runs at once."""
        import os
        sts = self.states
        cfg0 = sts[0]["config"]
        for st in sts:
            if st["config"].reset_policy and itr != 0:
                with _as_run(st):
                    old_agent = st["agent"]
                    st["agent"] = st["create_nominal_agent"]()
                    if hasattr(old_agent, "_train_ws"):
                        st["agent"]._train_ws = old_agent._train_ws
        agents = [st["agent"] for st in sts]
        progress = 1 - float(itr) / float(cfg0.n_iters)
        # ---- forward step
        self._learn(cfg0.forward_timesteps)
        fwd = []
        for st, a in zip(sts, agents):
            fwd.append(dict(st["logger"].name_to_value))
            st["timesteps"] += a.num_timesteps
        # ---- nominal trajectories
        A = 1 if agents[0].policy.discrete else agents[0].policy.act_dim
        noises = []
        for st in sts:
            sync_envs_normalization(st["train_env"], st["sampling_env"])
            s_ = getattr(st["config"], "streams", None)
            noises.append(None if s_ is None else s_.sample_noise(cfg0.expert_rollouts * st["sampling_env"].unwrapped.max_steps, A))
        runs, rewards = self._episodes([st["sampling_env"] for st in sts], cfg0.expert_rollouts, False, noises, True)
        samples = [utils.sample_result(r, rw) for r, rw in zip(runs, rewards)]
        # ---- backward step
        nets = [st["constraint_net"] for st in sts]
        cjobs = []
        for st, cn, (orig_obs, obs, acts, rews, lengths) in zip(sts, nets, samples):
            mean, var = None, None
            if st["config"].cn_normalize:
                mean, var = st["sampling_env"].obs_rms.mean, st["sampling_env"].obs_rms.var
            perms = None
            s_ = getattr(st["config"], "streams", None)
            if cn.batch_size is not None and s_ is not None and hasattr(s_, "cn_permutations"):
                perms = s_.cn_permutations(cfg0.backward_iters, min(int(orig_obs.shape[0]), int(np.asarray(cn.expert_obs).shape[0])))
            cjobs.append(cn._train_begin(cfg0.backward_iters, orig_obs, acts, lengths, mean, var, progress, perms))
        if nets[0].batch_size is None:
            self._launch_cn_trains(nets, cjobs)
        else:
            from .gail_utils import launch_disc_trains
            for cn, j in zip(nets, cjobs):
                j["batch_size"] = int(cn.batch_size)
            launch_disc_trains(nets, cjobs, self.args_ws)
        host = self._to_host([torch.cat([j["metrics"].reshape(-1).double(), j["t_dev"].double()]) for j in cjobs])
        backward = []
        for st, cn, j, h in zip(sts, nets, cjobs, host):
            backward.append(cn._train_end(j, metrics_host=h[:-1].reshape(j["metrics"].shape), adam_step_host=h[-1]))
            st["train_env"].set_cost_function(cn.cost_function)
        # ---- evaluation
        tail = []
        for st, (orig_obs, obs, acts, rews, lengths) in zip(sts, samples):
            tail.append(torch.stack([(orig_obs[..., 0] < -3).double().mean(), (orig_obs[..., 0] > 3).double().mean()]))
            sync_envs_normalization(st["train_env"], st["eval_env"])
        enoise = []
        for st in sts:
            s_ = getattr(st["config"], "streams", None)
            enoise.append(None if s_ is None else s_.eval_noise(10 * st["eval_env"].unwrapped.max_steps, A))
        eruns, erewards = self._episodes([st["eval_env"] for st in sts], 10, False, enoise, False)
        for i, (st, a) in enumerate(zip(sts, agents)):          # the KL metrics stay on the device until the one copy below
            if st["expert_agent"] is not None:
                orig_obs, obs, acts, rews, lengths = samples[i]
                fkl = utils.compute_kl_device(a, st["d_expert_obs"], st["d_expert_acs"], st["expert_agent"])
                rkl = utils.compute_kl_device(st["expert_agent"], orig_obs, acts, a)
                tail[i] = torch.cat([tail[i], torch.stack([fkl, rkl]).double()])
        tail_h = self._to_host(tail)
        out = []
        for i, (st, a) in enumerate(zip(sts, agents)):
            config = st["config"]
            orig_obs, obs, acts, rews, lengths = samples[i]
            average_true_cost = mean_cost(st["true_cost_function"], orig_obs, acts)
            samples_behind, samples_infront = float(tail_h[i][0]), float(tail_h[i][1])
            average_true_reward, std_true_reward = utils.evaluate_result(eruns[i], erewards[i])
            forward_kl = reverse_kl = float("nan")
            if st["expert_agent"] is not None:
                forward_kl, reverse_kl = float(tail_h[i][2]), float(tail_h[i][3])
            best = st["best"]
            if config.save_dir and itr % config.save_every == 0:
                path = os.path.join(config.save_dir, f"models/icrl_{itr}_itrs")
                os.makedirs(path, exist_ok=True)
                a.save(os.path.join(path, "nominal_agent"))
                torch.save(a.policy.state_dict(), os.path.join(path, "nominal_agent_policy.pth"))
                st["constraint_net"].save(os.path.join(path, "cn.pt"))
                st["train_env"].save(os.path.join(path, f"{itr}_train_env_stats.pkl"))
            if average_true_reward > best["reward"] and config.save_dir:
                a.save(os.path.join(config.save_dir, "best_nominal_model"))
                torch.save(a.policy.state_dict(), os.path.join(config.save_dir, "best_nominal_model_policy.pth"))
                st["constraint_net"].save(os.path.join(config.save_dir, "best_cn_model.pt"))
                st["train_env"].save(os.path.join(config.save_dir, "train_env_stats.pkl"))
            best["reward"] = max(best["reward"], average_true_reward)
            best["cost"] = min(best["cost"], average_true_cost)
            best["fkl"] = min(best["fkl"], forward_kl) if forward_kl == forward_kl else best["fkl"]
            best["rkl"] = min(best["rkl"], reverse_kl) if reverse_kl == reverse_kl else best["rkl"]
            metrics = {"time(m)": (time.time() - st["start_time"]) / 60, "iteration": itr, "timesteps": st["timesteps"],
                       "true/reward": average_true_reward, "true/reward_std": std_true_reward, "true/cost": average_true_cost,
                       "true/samples_infront": samples_infront, "true/samples_behind": samples_behind,
                       "true/forward_kl": forward_kl, "true/reverse_kl": reverse_kl, "best_true/best_reward": best["reward"],
                       "best_true/best_cost": best["cost"], "best_true/best_forward_kl": best["fkl"],
                       "best_true/best_reverse_kl": best["rkl"]}
            metrics.update({k.replace("train/", "forward/"): v for k, v in fwd[i].items()})
            metrics.update(backward[i])
            out.append(metrics)
        return out

    def run(self, first_iteration, n_iters):
        """outer iterations [first_iteration, first_iteration + n_iters) of every run.  Returns (metrics per run, wall seconds)."""
        out = [[] for _ in self.states]
        torch.cuda.synchronize()
        t0 = time.time()
        for it in range(first_iteration, first_iteration + n_iters):
            for i, m in enumerate(self.outer_iteration(it)):
                out[i].append(m)
        torch.cuda.synchronize()
        return out, time.time() - t0


def run_iterations(states, first_iteration, n_iters):
    """outer iterations of every run of `states` (setup_runs), all runs in every launch.  Returns (metrics per run, wall seconds)."""
    return SeedBatch(states=states).run(first_iteration, n_iters)


def run_seed_batch(configs, n_iters, on_setup=None):
    """configs: one icrl config (types.SimpleNamespace, see icrl.build_parser) per run.  Runs `n_iters` outer iterations of
    every run.  Returns (states, metrics per run, wall seconds of the iteration phase)."""
    sb = SeedBatch(configs, on_setup=on_setup)
    out, dt = sb.run(0, n_iters)
    return sb.states, out, dt


# ---- cpg: PPO-Lagrangian against a FIXED cost (the ground-truth cost, the null cost, a frozen constraint net), S seeds in lock-step ----
# everything a batched launch takes from run 0 only (grids, the batched GAE's discounting), plus what decides the sequence of phases
CPG_SAME = ("train_env_id", "eval_env_id", "num_threads", "n_steps", "batch_size", "n_epochs", "reward_gamma", "reward_gae_lambda", "cost_gamma",
            "cost_gae_lambda", "timesteps", "eval_every", "eval_every_rollouts", "use_pid", "use_null_cost")


class CpgSeedBatch(SeedBatch):
    """cpg.setup() per config — each run with its own PrivateStreams, scalar log, env stacks and callbacks — then ONE batched
    learn(timesteps, cost_function="cost"): every rollout (icrl_rollout_collect_batch_cost for analytic costs, icrl_rollout_collect_batch[_mon]
    for constraint nets), update (icrl_ppo_lag_train_batch) and evaluation (icrl_sample_episodes_batch) is one launch sequence for all runs.
    The evaluation noise of a batched run comes from its own streams (config.eval_noise_from_streams, set here); a solo run with that
    attribute and the same PrivateStreams computes the same bits."""

    per_run_wide_updates = True

    def __init__(self, configs, log=None):
        from . import cpg as C
        configs = list(configs)
        if not configs:
            raise ValueError("seed batch: no runs")
        c0 = configs[0]
        for c in configs:
            _refuse_cost_spec(c)
            exploration.refuse_batched(c, seed_batch=True)
            exploration.refuse_sde(c, seed_batch=True)
        if os.environ.get("ICRL_ANALYTIC_COST_STEPPED", "0") not in ("", "0"):
            raise ValueError("seed batch: ICRL_ANALYTIC_COST_STEPPED=1 forces the per-step rollout loop, which has no batched form")
        for c in configs:
            _refuse_host_envs(c.train_env_id, c.eval_env_id)
            if getattr(c, "env_module", None) or getattr(c, "dummy_vec_env", False):
                raise ValueError("seed batch: --env_module / --dummy_vec_env select host envs; the batched launches step device envs only")
            if getattr(c, "world_size", 1) > 1:
                raise ValueError("seed batch: the runs of a batch live on ONE rank (world_size > 1: launch one batch per GPU)")
            if c.load_gail:
                raise ValueError("seed batch: --load_gail (load_gail) reads the loaded net as a discriminator cost, and the batched rollout kernels have no "
                                 "discriminator form yet (single runs make their rollouts in fused launches); a batch takes a constraint net, the "
                                 "ground-truth cost or the null cost")
            if c.cost_info_str is None:
                raise ValueError("seed batch: -cis None hands learn() the cost as a callable (the per-step loop); a batch needs the cost inside the env chain")
            diff = [k for k in CPG_SAME if getattr(c, k) != getattr(c0, k)]
            if (c.cn_path is None) != (c0.cn_path is None):
                diff.append("cn_path is None")
            if diff:
                raise ValueError(f"seed batch: the runs of a batch share every grid and the sequence of phases; they differ in {diff}")
        self.states = []
        for i, cfg in enumerate(configs):
            if getattr(cfg, "streams", None) is None:
                cfg.streams = PrivateStreams(cfg.seed, discrete=cfg.train_env_id in ("LGW-v0", "CLGW-v0"))
            if not hasattr(cfg.streams, "eval_noise"):
                raise ValueError("seed batch: every run needs its own random streams")
            cfg.eval_noise_from_streams = True
            model, cb, learn_cost, hist = C.setup(cfg, log)
            cw = model.env.venv
            cn = cw.constraint_net() if hasattr(cw, "constraint_net") else None
            if model.policy.wide or int(model.batch_size) > 256 or getattr(cn, "wide", False):
                raise ValueError(f"seed batch: run {i}: hidden widths above 64 / batch sizes above 256 run on the generic-shape path, which has no batched form")
            if isinstance(model.env.unwrapped, HostVecEnv) or not isinstance(learn_cost, str):
                raise ValueError(f"seed batch: run {i}: the batched launches step device envs with the cost inside the env chain")
            self.states.append(dict(config=cfg, agent=model, callback=cb, hist=hist, logger=logger.Logger.CURRENT, train_env=model.env))
        torch.cuda.synchronize()
        self.dev = self.states[0]["agent"].device
        self.args_ws = torch.empty(2 * len(self.states) * _lib.BATCH_ARGS_BYTES, dtype=torch.uint8, device=self.dev)

    def learn(self):
        """one batched learn(); returns (model, history) per run like cpg(), final_model_policy.pth saved per run."""
        self._learn(int(self.states[0]["config"].timesteps), callbacks=[st["callback"] for st in self.states], prefetch_across_end=False)
        out = []
        for st in self.states:
            cfg = st["config"]
            if cfg.save_dir:
                torch.save(st["agent"].policy.state_dict(), os.path.join(cfg.save_dir, "final_model_policy.pth"))
            out.append((st["agent"], st["hist"].history))
        return out


def run_cpg_seed_batch(configs, log=None):
    """configs: one cpg config (types.SimpleNamespace, see cpg.build_parser / cpg.seed_configs) per run.  Returns (model, history) per run."""
    return CpgSeedBatch(configs, log).learn()


# ---- gail: plain PPO + the discriminator's rollout-end work (icrl_amd/gail_utils.py: GailCallback), S seeds in lock-step ----
GAIL_SAME = ("train_env_id", "eval_env_id", "num_threads", "n_steps", "batch_size", "n_epochs", "reward_gamma", "reward_gae_lambda", "timesteps",
             "eval_every", "learn_cost", "disc_batch_size", "disc_layers", "policy_layers", "reward_vf_layers", "dont_normalize_obs",
             "disc_obs_select_dim", "disc_acs_select_dim")


class GailSeedBatch(SeedBatch):
    """gail.setup() per config — each run with its own PrivateStreams, scalar log, env stack, discriminator and callbacks — then ONE batched
    learn(): rollouts (icrl_rollout_collect_batch[_mon]), evaluations (icrl_sample_episodes_batch), the GailCallbacks' rollout ends
    (icrl_gail_unnormalize_batch, icrl_cn_train_minibatch_batch, icrl_gail_relabel_batch, icrl_gae_dual_batch) and updates
    (icrl_ppo_lag_train_batch) are one launch sequence for all runs.  Evaluation noise and the discriminator's permutation of a batched run
    come from its own streams (config.eval_noise_from_streams, config.disc_perms_from_streams, set here); a solo run with both and the same
    PrivateStreams computes the same bits."""

    per_run_wide_updates = True

    def __init__(self, configs, log=None):
        from . import gail as G
        configs = list(configs)
        if not configs:
            raise ValueError("seed batch: no runs")
        c0 = configs[0]
        for c in configs:      # ---- refused before anything is set up
            _refuse_cost_spec(c)
            exploration.refuse_sde(c, seed_batch=True)
        for c in configs:
            _refuse_host_envs(c.train_env_id, c.eval_env_id)
            if getattr(c, "env_module", None) or getattr(c, "dummy_vec_env", False):
                raise ValueError("seed batch: --env_module / --dummy_vec_env select host envs; the batched launches step device envs only")
            if getattr(c, "world_size", 1) > 1:
                raise ValueError("seed batch: the runs of a batch live on ONE rank (world_size > 1: launch one batch per GPU)")
            if getattr(c, "use_cost_shaping_callback", False):
                raise NotImplementedError("--use_cost_shaping_callback (a shaping ablation of the reference) is outside the hot path")
            diff = [k for k in GAIL_SAME if getattr(c, k) != getattr(c0, k)]
            if (c.gail_path is None) != (c0.gail_path is None):
                diff.append("gail_path is None")
            if bool(getattr(c, "episode_stats", None)) != bool(getattr(c0, "episode_stats", None)):
                diff.append("episode_stats")
            if diff:
                raise ValueError(f"seed batch: the runs of a batch share every grid and the sequence of phases; they differ in {diff}")
        self.states = []
        for i, cfg in enumerate(configs):
            if getattr(cfg, "streams", None) is None:
                cfg.streams = PrivateStreams(cfg.seed, discrete=cfg.train_env_id in ("LGW-v0", "CLGW-v0"))
            if not hasattr(cfg.streams, "eval_noise") or not hasattr(cfg.streams, "cn_permutations"):
                raise ValueError("seed batch: every run needs its own random streams")
            cfg.eval_noise_from_streams = cfg.disc_perms_from_streams = True
            model, cb, disc, gail_cb = G.setup(cfg, log)
            if model.policy.wide or int(model.batch_size) > 256 or disc.wide:
                raise ValueError(f"seed batch: run {i}: hidden widths above 64 / batch sizes above 256 (policy or discriminator) run on the generic-shape "
                                 "path, which has no batched form")
            if isinstance(model.env.unwrapped, HostVecEnv):
                raise ValueError(f"seed batch: run {i}: the batched launches step device envs")
            self.states.append(dict(config=cfg, agent=model, callback=cb, discriminator=disc, gail=gail_cb, logger=logger.Logger.CURRENT, train_env=model.env))
        if len({st["agent"]._mon is None for st in self.states}) != 1:
            raise ValueError("seed batch: episode_stats must be on in every run of a batch or in none")
        if len({tuple(st["discriminator"].hidden_sizes) + (st["discriminator"].input_dims,) for st in self.states}) != 1:
            raise ValueError("seed batch: the discriminators of a batch share one shape")
        torch.cuda.synchronize()
        self.dev = self.states[0]["agent"].device
        self.args_ws = torch.empty(2 * len(self.states) * _lib.BATCH_ARGS_BYTES, dtype=torch.uint8, device=self.dev)

    def learn(self):
        """one batched learn(); returns (model, discriminator, history) per run like gail(), gail_discriminator.pt / train_env_stats.pkl saved per run."""
        from . import gail as G
        self._learn(int(self.states[0]["config"].timesteps), callbacks=[st["callback"] for st in self.states], prefetch=False)
        out = []
        for st in self.states:
            G.finish(st["config"], st["agent"], st["discriminator"])
            out.append((st["agent"], st["discriminator"], st["gail"].history))
        return out


def run_gail_seed_batch(configs, log=None):
    """configs: one gail config (types.SimpleNamespace, see gail.build_parser / utils.seed_configs) per run.  Returns (model, discriminator,
    history) per run."""
    return GailSeedBatch(configs, log).learn()
