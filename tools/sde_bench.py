"""What gSDE costs on the two paths it runs on, against the diagonal Gaussian head on the SAME two paths:

  rollout   microseconds per env step of PPOLagrangian._collect_rollouts_stepped (HCWithPos, --envs envs): policy forward (icrl_policy_forward_sde |
            icrl_policy_forward), env step, cost, normaliser, buffer row — one launch sequence per step, no host read;
  update    microseconds per optimiser step of the fine-grained loop at (obs 18, act 6, batch 64): icrl_minibatch_gather, the policy forward
            (icrl_policy_sde_fwd_bwd | icrl_policy_fwd_bwd, forward only), icrl_ppo_lag_loss_fwd_bwd, the same entry point with the gradient,
            icrl_clip_adam_step — what PPOLagrangian._train_sde_loop enqueues per minibatch;
  fused     microseconds per optimiser step of ONE persistent launch over the same buffer (2048 rows, batch 64: 32 minibatches per epoch,
            --steps / 32 epochs; the warm-up is a launch of --warmup / 32 epochs): icrl_ppo_lag_train_sde for gSDE (what PPOLagrangian._train_sde
            takes by default), and for the diagonal head icrl_ppo_lag_train with the column-split tiles kernel (hp._pad bit 1) — the kernel the gSDE
            launch is built from, so the difference of the two is the cost of the head.

  rollout_fused   microseconds per env step of PPOLagrangian.collect_rollouts as a launch of the library: the gSDE agent with sde_fused_rollout
            (icrl_rollout_collect_sde, the schedule's draws included) and the diagonal head's fused rollout (icrl_rollout_collect_ex) — the
            difference of the two is the cost of the head and of the schedule; the yardstick is the gSDE loop in the same process and run order.
            Both at --envs envs x --steps steps and (keys ending in _64x2048) at 64 envs x 2048 steps, sde_sample_freq 8.

  --episodes   (a mode of its own; nothing else is timed) microseconds per executed env step of utils.sample_from_agent on HCWithPos-v0 and of
            utils.evaluate_policy(deterministic=False) on HCWithPosTest-v0, 10 episodes of at most 1000 steps each, in three forms: the gSDE per-step
            loop (utils.SteppedEpisodeRun, ICRL_SDE_EPISODES_STEPPED=1: the yardstick), the gSDE launch (icrl_sample_episodes_chain_sde), and the
            diagonal head's launch (icrl_sample_episodes_chain) on an agent of the same shape.  --runs interleaved runs per form in one process, the
            first call of each form outside the timed region; the executed steps are the sum of the returned episode lengths.  With --out the
            new keys (episodes_*) are merged into the file.

The loop figures say nothing about the fused launches the diagonal head normally takes (bench.py measures those).  Per run: --steps steps after
--warmup, one synchronisation at each end, host clock around it; --runs runs per form, interleaved.  Needs the GPU.

    python tools/sde_bench.py [--steps 512 --warmup 64 --runs 3 --envs 4] [--wide] [--out profiles/sde.json]
"""
import argparse
import ctypes
import json
import os
import sys
import time
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from icrl_amd import _lib, spaces, structs as S      # noqa: E402
from icrl_amd.buffers import RolloutBufferWithCost   # noqa: E402
from icrl_amd.policies import ActorTwoCriticsPolicy  # noqa: E402

P = _lib.ptr
OBS, ACT, BATCH = 18, 6, 64


class UpdateLoop:
    def __init__(self, use_sde, seed=0, obs=OBS, act=ACT, batch=BATCH):
        OBS, ACT, BATCH = obs, act, batch      # (the shape of this loop; the module's are the default)
        self.batch = batch
        torch.manual_seed(seed)
        rng = np.random.RandomState(seed)
        self.L, self.use_sde = _lib.lib(), use_sde
        T, n_envs = 64, 32
        self.n_rows = T * n_envs
        o, a = spaces.Box(-np.inf, np.inf, (OBS,), np.float64), spaces.Box(-1, 1, (ACT,), np.float32)
        self.rb = RolloutBufferWithCost(T, o, a, "cuda", n_envs=n_envs)
        for k in ("observations", "actions", "reward_advantages", "cost_advantages", "reward_returns", "cost_returns", "reward_values", "cost_values"):
            t = getattr(self.rb, k)
            t.copy_(torch.as_tensor(rng.randn(*t.shape).astype(np.float32)))
        self.policy = pol = ActorTwoCriticsPolicy(o, a, use_sde=use_sde)
        lp = pol.evaluate_actions(self.rb.observations.reshape(-1, OBS).double(), self.rb.actions.reshape(-1, ACT))[2]      # ratio 1 at the first step
        self.rb.log_probs.copy_(lp.reshape(self.rb.log_probs.shape))
        self.buf = self.rb.struct()
        self.idx = torch.as_tensor(np.stack([rng.permutation(T * n_envs)[:BATCH] for _ in range(64)]).astype(np.int32)).cuda().contiguous()
        self.params0 = pol.params.clone()
        f = lambda *shape: torch.zeros(*shape, device="cuda")
        self.grad, self.step = f(pol.n_params), torch.zeros(1, dtype=torch.int32, device="cuda")
        self.work, self.out2, self.terms, self.nu = f(256), f(2), f(8), torch.full((1,), 0.5, device="cuda")
        self.obs, self.act = f(BATCH, OBS), f(BATCH, ACT)
        self.r = {k: f(BATCH) for k in ("old_lp", "adv_r", "adv_c", "ret_r", "ret_c", "old_vr", "old_vc", "v_r", "v_c", "lp", "ent", "d_lp", "d_vr", "d_vc", "d_ent")}
        self.s = pol.struct(sde=use_sde)
        self.fb = self.L.icrl_policy_sde_fwd_bwd if use_sde else self.L.icrl_policy_fwd_bwd
        need = int((self.L.icrl_policy_sde_fwd_bwd_ws_bytes if use_sde else self.L.icrl_policy_fwd_bwd_ws_bytes)(ctypes.byref(self.s), BATCH))
        self.ws = torch.zeros((need + 7) // 8, dtype=torch.float64, device="cuda")
        hp = S.PpoHyperT(BATCH, 1, 0, 0)
        hp.clip_range, hp.ent_coef, hp.reward_vf_coef, hp.cost_vf_coef, hp.max_grad_norm = 0.2, 0.0, 0.5, 0.5, 0.5
        hp.clip_range_reward_vf = hp.clip_range_cost_vf = -1.0
        hp.lr, hp.adam_beta1, hp.adam_beta2, hp.adam_eps = 3e-5, 0.9, 0.999, 1e-5
        self.hp = hp
        self.perms = torch.as_tensor(np.stack([rng.permutation(T * n_envs) for _ in range(64)]).astype(np.int32)).cuda().contiguous()
        self.stats = f(32 + 64)
        self.sync = None

    def one_step(self, i):
        BATCH = self.batch
        L, r, st, b, pol = self.L, self.r, _lib.current_stream(), ctypes.byref, self.policy
        _lib.check(L.icrl_minibatch_gather(b(self.buf), self.idx[i % 64].data_ptr(), BATCH, P(self.obs), P(self.act), P(r["old_lp"]), P(r["adv_r"]), P(r["adv_c"]),
                                           P(r["ret_r"]), P(r["ret_c"]), P(r["old_vr"]), P(r["old_vc"]), st), "icrl_minibatch_gather")
        _lib.check(self.fb(b(self.s), P(self.obs), P(self.act), BATCH, None, None, None, None, P(r["v_r"]), P(r["v_c"]), P(r["lp"]), P(r["ent"]), None, None, 0, st),
                   "policy forward")
        _lib.check(L.icrl_ppo_lag_loss_fwd_bwd(P(r["lp"]), P(r["old_lp"]), P(r["adv_r"]), P(r["adv_c"]), P(r["v_r"]), P(r["v_c"]), P(r["ret_r"]), P(r["ret_c"]), None,
                                               None, P(r["ent"]), P(self.nu), b(self.hp), BATCH, P(self.terms), P(r["d_lp"]), P(r["d_vr"]), P(r["d_vc"]), P(r["d_ent"]),
                                               st), "icrl_ppo_lag_loss_fwd_bwd")
        _lib.check(self.fb(b(self.s), P(self.obs), P(self.act), BATCH, P(r["d_vr"]), P(r["d_vc"]), P(r["d_lp"]), P(r["d_ent"]), None, None, None, None, P(self.grad),
                           P(self.ws), self.ws.numel() * 8, st), "policy backward")
        _lib.check(L.icrl_clip_adam_step(P(pol.params), P(self.grad), P(pol.exp_avg), P(pol.exp_avg_sq), P(self.step), pol.n_params, b(self.hp), P(self.work),
                                         P(self.out2), st), "icrl_clip_adam_step")

    def run(self, steps, warmup):
        pol = self.policy
        pol.params.copy_(self.params0); pol.exp_avg.zero_(); pol.exp_avg_sq.zero_(); self.step.zero_()
        for i in range(warmup):
            self.one_step(i)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(warmup, warmup + steps):
            self.one_step(i)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(pol.params).all())
        return 1e6 * (time.perf_counter() - t0) / max(steps, 1)


    def fused(self, n_steps):
        """one persistent launch of n_steps optimiser steps (whole epochs of the 2048-row buffer)."""
        b, pol, n_mb = ctypes.byref, self.policy, self.n_rows // self.batch
        E = max(1, min(64, n_steps // n_mb))
        hp = S.PpoHyperT.from_buffer_copy(self.hp)
        hp.n_epochs, hp._pad = E, (0 if self.use_sde else 2)      # diagonal: the column-split tiles kernel, the gSDE launch's parent
        if self.sync is None:
            n_bytes = 768 + 48 * 64 * n_mb + 4 * 64 * self.n_rows + 256 + _lib.PPO_SPLIT_BYTES      # ICRL_PPO_SYNC_BYTES at 64 epochs
            self.sync = torch.zeros((n_bytes + 7) // 8, dtype=torch.int64, device="cuda")
        call = self.L.icrl_ppo_lag_train_sde if self.use_sde else self.L.icrl_ppo_lag_train
        _lib.check(call(b(self.s), P(pol.exp_avg), P(pol.exp_avg_sq), P(self.step), b(self.buf), P(self.perms), P(self.nu), b(hp), P(self.stats), P(self.sync),
                        _lib.current_stream()), "fused update")
        return E * n_mb

    def run_fused(self, steps, warmup):
        pol = self.policy
        pol.params.copy_(self.params0); pol.exp_avg.zero_(); pol.exp_avg_sq.zero_(); self.step.zero_()
        self.fused(warmup)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        done = self.fused(steps)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        assert bool(torch.isfinite(pol.params).all()) and float(self.stats[11]) == 0.0 and int(self.stats[1]) == done
        return 1e6 * dt / done


class RolloutLoop:
    """fused: collect_rollouts as a launch of the library (gSDE: --sde_fused_rollout), else the per-step loop"""

    def __init__(self, use_sde, envs, steps, fused=False):
        from icrl_amd import cpg
        argv = ["cpg", "-tei", "HCWithPos-v0", "-eei", "HCWithPosTest-v0", "-nt", str(envs), "--n_steps", str(steps), "-s", "0", "-v", "0"] + (["-us", "-ssf", "8"] if use_sde else [])
        cfg = vars(cpg.build_parser().parse_args(argv + (["-sfr"] if use_sde and fused else [])))
        cfg.update(rank=0, world_size=1)
        self.model, _cb, self.cost, _hist = cpg.setup(types.SimpleNamespace(**cfg), log=None)
        self.steps, self.fused, self.use_sde = steps, fused, use_sde
        self.model._setup_learn(envs * steps)

    def run(self):
        m = self.model
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if self.fused:
            assert m.collect_rollouts(m.env, None, m.rollout_buffer, self.steps, self.cost) is True
        else:
            assert m._collect_rollouts_stepped(m.env, None, m.rollout_buffer, self.steps, self.cost) is True
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if self.fused:      # one launch, and (gSDE) the launch with the head, not the loop
            route = _lib.last_route(_lib.FAMILY_ROLLOUT)
            assert route[7] == 1 and bool(route[4] & _lib.PICK_SDE) == self.use_sde and (not self.use_sde or m.last_sde_rollout == "fused"), route
            m.check_rollout_status()
        return 1e6 * dt / self.steps

    def schedule_us(self):
        """the up-front draws alone (policy.noise_schedule), per env step: the part of a fused gSDE rollout that is not the launch"""
        m = self.model
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m.policy.noise_schedule(m.n_envs, self.steps, m.sde_sample_freq, m.streams)
        torch.cuda.synchronize()
        return 1e6 * (time.perf_counter() - t0) / self.steps


class EpisodeForms:
    """sample_from_agent / evaluate_policy of a gSDE agent through the loop and through the launch, and of a diagonal agent of the same shape"""
    N_EP = 10

    def __init__(self):
        from icrl_amd import cpg, utils
        self.utils = utils
        self.models = {}
        for k, extra in (("gsde", ["-us"]), ("diagonal", [])):
            argv = ["cpg", "-tei", "HCWithPos-v0", "-eei", "HCWithPosTest-v0", "-nt", "4", "--n_steps", "32", "-s", "0", "-v", "0"] + extra
            cfg = vars(cpg.build_parser().parse_args(argv))
            cfg.update(rank=0, world_size=1)
            self.models[k] = cpg.setup(types.SimpleNamespace(**cfg), log=None)[0]
        self.models["gsde"].policy.reset_noise(1)
        self.envs = dict(sample=utils.make_eval_env("HCWithPos-v0", False, seed=0), eval=utils.make_eval_env("HCWithPosTest-v0", False, seed=0))
        self.forms = dict(gsde_loop=("gsde", "1"), gsde_launch=("gsde", None), diagonal_launch=("diagonal", None))

    def run(self, form, phase):
        """(microseconds per executed env step, executed steps, milliseconds)"""
        which, stepped = self.forms[form]
        model, env, utils = self.models[which], self.envs[phase], self.utils
        old = os.environ.pop("ICRL_SDE_EPISODES_STEPPED", None)
        if stepped is not None:
            os.environ["ICRL_SDE_EPISODES_STEPPED"] = stepped
        try:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if phase == "sample":
                lengths = utils.sample_from_agent(model, env, self.N_EP)[4]
            else:
                lengths = utils.evaluate_policy(model, env, self.N_EP, deterministic=False, return_episode_rewards=True)[1]
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
        finally:
            os.environ.pop("ICRL_SDE_EPISODES_STEPPED", None)
            if old is not None:
                os.environ["ICRL_SDE_EPISODES_STEPPED"] = old
        if which == "gsde":
            assert model.last_sde_episodes == ("loop" if stepped else "fused"), (form, model.last_sde_episodes, model.last_sde_episodes_reason)
        steps = int(np.sum(lengths))
        return 1e6 * dt / steps, steps, 1e3 * dt


def episodes_main(a):
    ep = EpisodeForms()
    out = dict(episodes_protocol="host clock between two synchronisations around one sample_from_agent(HCWithPos-v0, 10 episodes) / one "
                                 "evaluate_policy(HCWithPosTest-v0, 10 episodes, deterministic=False) call; microseconds per executed env step = time "
                                 "/ sum of the returned episode lengths; --runs runs per form, interleaved (loop, gSDE launch, diagonal launch), one "
                                 "untimed call of each form first",
               episodes_runs=a.runs, episodes_device=torch.cuda.get_device_name(0))
    for phase in ("sample", "eval"):
        for form in ep.forms:
            ep.run(form, phase)      # outside the timed region
        us = {form: [] for form in ep.forms}
        ms = {form: [] for form in ep.forms}
        steps = {}
        for _ in range(a.runs):
            for form in ep.forms:
                u, n, m = ep.run(form, phase)
                us[form].append(round(u, 2)); ms[form].append(round(m, 2)); steps[form] = n
        for form in ep.forms:
            out[f"episodes_{phase}_us_per_step_{form}"] = us[form]
            out[f"episodes_{phase}_ms_{form}"] = ms[form]
            out[f"episodes_{phase}_steps_{form}"] = steps[form]
            print(f"episodes {phase} {form}: {us[form]} us per step, {ms[form]} ms, {steps[form]} steps", flush=True)
        out[f"episodes_{phase}_every_launch_run_below_the_loops_fastest"] = bool(max(us["gsde_launch"]) < min(us["gsde_loop"]))
        out[f"episodes_{phase}_gsde_launch_speedup_worst_case"] = round(min(ms["gsde_loop"]) / max(ms["gsde_launch"]), 1)
    out["episodes_not_measured"] = "a whole icrl -us -sfr run at the reference's step counts; other envs and shapes; host envs (not served)"
    print(json.dumps(out))
    if a.out:
        merged = {}
        if os.path.exists(a.out):
            with open(a.out) as f:
                merged = json.load(f)
        merged.update(out)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(merged, f, indent=1)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=512)
    ap.add_argument("--warmup", type=int, default=64)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--envs", type=int, default=4)
    ap.add_argument("--wide", action="store_true", help="also time the update forms at (obs 113, act 8, batch 128): keys ending in _113_8_128")
    ap.add_argument("--episodes", action="store_true", help="time sampling / evaluation episodes alone (loop, gSDE launch, diagonal launch); with --out the keys are merged into the file")
    ap.add_argument("--out", default=None, help="write the result as JSON to this file as well")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sde_bench needs the GPU: a time measured elsewhere says nothing about it")
    if a.episodes:
        return episodes_main(a)
    result = dict(status="measured", device=torch.cuda.get_device_name(0), steps=a.steps, warmup=a.warmup, runs=a.runs, envs=a.envs,
                  protocol="host clock between two synchronisations around --steps steps after --warmup; --runs runs per form, interleaved; "
                           "update: obs 18, act 6, batch 64, fine-grained loop; update_fused: the same buffer and shape, one persistent launch of "
                           "steps / 32 epochs (gsde: icrl_ppo_lag_train_sde; diagonal: icrl_ppo_lag_train, tiles kernel); rollout: HCWithPos, per-step "
                           "loop, sde_sample_freq 8; rollout_fused: the same rollout as one launch of the library (gsde: icrl_rollout_collect_sde with "
                           "the schedule's draws inside the timed region; diagonal: icrl_rollout_collect_ex); keys ending in _64x2048: 64 envs x 2048 "
                           "steps; microseconds per env step = time of the rollout / its steps")
    upd = {k: UpdateLoop(k == "gsde") for k in ("diagonal", "gsde")}
    roll = {k: RolloutLoop(k == "gsde", a.envs, a.steps) for k in ("diagonal", "gsde")}
    # the three rollout forms at both shapes: the gSDE loop (the yardstick), the gSDE launch, the diagonal head's launch
    forms = {"rollout_us_per_step_gsde": (True, False), "rollout_fused_us_per_step_gsde": (True, True), "rollout_fused_us_per_step_diagonal": (False, True)}
    shapes = {"": (a.envs, a.steps), "_64x2048": (64, 2048)}
    fused_roll = {key + tag: (roll["gsde"] if (tag == "" and not fused) else RolloutLoop(sde, envs, steps, fused))
                  for tag, (envs, steps) in shapes.items() for key, (sde, fused) in forms.items()}
    for loop in list(roll.values()) + [l for l in fused_roll.values() if l is not roll["gsde"]]:
        loop.run()      # warm-up rollout
    us = {f"{what}_us_per_step_{k}": [] for what in ("update", "update_fused", "rollout") for k in ("diagonal", "gsde")}
    us.update({k: [] for k in fused_roll})
    for _ in range(a.runs):
        for k in ("diagonal", "gsde"):
            us[f"update_us_per_step_{k}"].append(round(upd[k].run(a.steps, a.warmup), 1))
            us[f"update_fused_us_per_step_{k}"].append(round(upd[k].run_fused(a.steps, a.warmup), 2))
        us["rollout_us_per_step_diagonal"].append(round(roll["diagonal"].run(), 1))
        for k, loop in fused_roll.items():      # interleaved: loop, gSDE launch, diagonal launch, per shape
            us[k].append(round(loop.run(), 2 if "fused" in k else 1))
    if a.wide:
        wide = {k: UpdateLoop(k == "gsde", obs=113, act=8, batch=128) for k in ("diagonal", "gsde")}
        for what in ("update", "update_fused"):
            for k in ("diagonal", "gsde"):
                us[f"{what}_us_per_step_{k}_113_8_128"] = []
        for _ in range(a.runs):
            for k in ("diagonal", "gsde"):
                us[f"update_us_per_step_{k}_113_8_128"].append(round(wide[k].run(a.steps, a.warmup), 1))
                us[f"update_fused_us_per_step_{k}_113_8_128"].append(round(wide[k].run_fused(a.steps, a.warmup), 2))
    result.update(us)
    result["not_measured"] = ("rollout_fused: other shapes and action widths, sde_sample_freq 1, a whole cpg -us -sfr run, the per-step launches' own rate; the head's share inside the kernel is the difference to the diagonal rollout less the schedule's share, not a measurement of its own")
    for tag in shapes:      # the launch against the loop of the same process: slowest launch run over fastest loop run
        lo, fu, di = us["rollout_us_per_step_gsde" + tag], us["rollout_fused_us_per_step_gsde" + tag], us["rollout_fused_us_per_step_diagonal" + tag]
        result["rollout_fused_gsde_speedup_worst_case" + tag] = round(min(lo) / max(fu), 1)
        result["rollout_fused_gsde_minus_diagonal_us" + tag] = round(sorted(fu)[len(fu) // 2] - sorted(di)[len(di) // 2], 2)
        result["rollout_fused_gsde_schedule_us_per_step" + tag] = [round(fused_roll["rollout_fused_us_per_step_gsde" + tag].schedule_us(), 2) for _ in range(a.runs)]
    for k, v in us.items():
        print(f"{k}: {v}", flush=True)
    print(json.dumps(result))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
