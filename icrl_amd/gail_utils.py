"""GAIL-constraint baseline: discriminator and rollout-end callback, device-resident.

ref: icrl/gail_utils.py:18-498 (GailDiscriminator), :500-571 (GailCallback).  The discriminator is the constraint net read the
other way round — the same ReLU MLP + sigmoid, trained with BCE on nominal (label 0) vs expert (label 1) rows — so it runs on
the constraint-net kernels (icrl_cn_prepare, icrl_cn_train_minibatch in its BCE mode, icrl_disc_reward).  Reference behaviour
kept on purpose: nothing is normalised or clipped on the way in (normalize_obs is a no-op and clip_actions is commented out,
gail_utils.py:298-316), both sets are truncated to min(n_nominal, n_expert) rows by the shared permutation of get(), and the
callback un-normalises the buffer's float32 NORMALISED observations with the statistics at the end of the rollout instead of
using the raw observations (gail_utils.py:539-542).
"""
import numpy as np
import torch

from . import _lib, callbacks, logger
from .constraint_net import ConstraintNet
from .structs import COST_DISC, CnTrainMbJobT, CostDiscT, GaeJobT, GailJobT, addr, p
from .true_constraint_net import AnalyticCost, null_cost


class GailDiscriminator(ConstraintNet):
    def __init__(self, obs_dim, acs_dim, hidden_sizes, batch_size, lr_schedule, expert_obs, expert_acs, is_discrete,
                 obs_select_dim=None, acs_select_dim=None, optimizer_class=torch.optim.Adam, optimizer_kwargs=None, clip_obs=10.,
                 initial_obs_mean=None, initial_obs_var=None, action_low=None, action_high=None, num_spurious_features=None,
                 freeze_weights=False, eps=1e-5, device="cuda"):
        if num_spurious_features is not None:
            raise NotImplementedError("num_spurious_features (a diagnostic of the reference's grid-world study) is not built")
        super().__init__(obs_dim, acs_dim, hidden_sizes, batch_size, lr_schedule, expert_obs, expert_acs, is_discrete, 0.0,
                         obs_select_dim, acs_select_dim, optimizer_class, optimizer_kwargs, no_importance_sampling=True,
                         clip_obs=None, action_low=None, action_high=None, train_gail_lambda=True, eps=eps, device=device)
        # stored like the reference stores them; its prepare_*_data never applies them
        self.stored_clip_obs, self.stored_action_low, self.stored_action_high = clip_obs, action_low, action_high
        self.freeze_weights = freeze_weights

    @staticmethod
    def flatten(x):
        x = torch.as_tensor(x) if not torch.is_tensor(x) else x
        if x.dim() > 2:
            d0, d1 = x.shape[:2]
            return x.reshape(d0 * d1, -1), (d0, d1)
        return x, (x.shape[0], 1)

    def train(self, iterations, nominal_obs, nominal_acs, obs_mean=None, obs_var=None, current_progress_remaining=1, perms=None):
        """ref: gail_utils.py:163-208 -> the five discriminator/* metrics of the last minibatch."""
        job = self._disc_train_begin(iterations, nominal_obs, nominal_acs, current_progress_remaining, perms)
        launch_disc_trains([self], [job])
        return self._disc_train_end(job)

    # train() in three pieces, like ConstraintNet._train_*: the launch of one or of several discriminators is launch_disc_trains below
    def _disc_train_begin(self, iterations, nominal_obs, nominal_acs, current_progress_remaining=1, perms=None):
        obs, _ = self.flatten(nominal_obs)
        acs, _ = self.flatten(nominal_acs)
        n_exp = int(np.asarray(self.expert_obs).shape[0])
        size = min(int(obs.shape[0]), n_exp)
        keep_bs, keep_sched = self.batch_size, self.lr_schedule
        self.batch_size = size if keep_bs is None else int(keep_bs)     # batch_size None: ONE batch of `size` permuted rows
        if self.freeze_weights:
            self.lr_schedule = lambda _x: 0.0                            # evaluated, not updated
        try:
            job = self._train_begin(int(iterations), obs, acs, np.array([obs.shape[0]]), None, None, current_progress_remaining, perms)
            job["batch_size"] = int(self.batch_size)
        finally:
            self.batch_size, self.lr_schedule = keep_bs, keep_sched
        return job

    def _disc_train_end(self, job, metrics_host=None, adam_step_host=None):
        m = self._train_end(job, metrics_host=metrics_host, adam_step_host=adam_step_host)
        return {"discriminator/disc_loss": m["backward/cn_loss"], "discriminator/expert_loss": m["backward/expert_loss"],
                "discriminator/nominal_loss": m["backward/nominal_loss"],
                "discriminator/mean_nominal_preds": m["backward/nominal_preds_mean"],
                "discriminator/mean_expert_preds": m["backward/expert_preds_mean"]}

    def reward_function(self, obs, acs, apply_log=True):
        """ref: gail_utils.py:147-157 -> device float32 tensor shaped like the leading axes of `obs`."""
        o, shape = self.flatten(obs)
        a, _ = self.flatten(acs)
        assert o.shape[-1] == self.obs_dim, ""
        dev = self.device
        o = o.to(device=dev, dtype=torch.float64).contiguous()
        a = a.to(device=dev, dtype=torch.float32).reshape(o.shape[0], -1).contiguous()
        out = torch.empty(o.shape[0], device=dev)
        s = self.struct()
        _lib.check(_lib.lib().icrl_disc_reward(_lib.byref(s), p(o), p(a), o.shape[0], p(out), int(bool(apply_log)),
                                               _lib.current_stream()), "icrl_disc_reward")
        return out.reshape(shape).squeeze()

    def save(self, save_path):
        torch.save(dict(network=self.state_dict(), optimizer=dict(exp_avg=self.exp_avg.cpu(), exp_avg_sq=self.exp_avg_sq.cpu(), step=self.adam_step),
                        obs_dim=self.obs_dim, acs_dim=self.acs_dim, is_discrete=self.is_discrete, obs_select_dim=self.obs_select_dim,
                        acs_select_dim=self.acs_select_dim, clip_obs=self.stored_clip_obs, obs_mean=self.current_obs_mean,
                        obs_var=self.current_obs_var, action_low=self.stored_action_low, action_high=self.stored_action_high,
                        device=str(self.device), hidden_sizes=self.hidden_sizes), save_path)

    @classmethod
    def load(cls, load_path, obs_dim=None, acs_dim=None, is_discrete=None, expert_obs=None, expert_acs=None, obs_select_dim=None,
             acs_select_dim=None, clip_obs=None, obs_mean=None, obs_var=None, action_low=None, action_high=None, device="auto"):
        """ref: gail_utils.py:356-402 (reads the reference's gail_discriminator.pt: key `network`)."""
        sd = load_path if isinstance(load_path, dict) else torch.load(load_path, map_location="cpu", weights_only=False)
        g = lambda v, k: sd[k] if v is None else v
        net = cls(g(obs_dim, "obs_dim"), g(acs_dim, "acs_dim"), sd["hidden_sizes"], None, (lambda x: 0.0), expert_obs, expert_acs,
                  g(is_discrete, "is_discrete"), g(obs_select_dim, "obs_select_dim"), g(acs_select_dim, "acs_select_dim"), None, None,
                  g(clip_obs, "clip_obs"), g(obs_mean, "obs_mean"), g(obs_var, "obs_var"), g(action_low, "action_low"),
                  g(action_high, "action_high"))
        net.load_state_dict(sd["network"])
        return net


class DiscriminatorCost:
    """The env cost of `cpg --load_gail` (ref: icrl/cpg.py:54-83): the loaded discriminator's output D(previous raw obs, clipped action),
    reward_function with apply_log=False, as an object the rollout entry points can read (VecCostWrapper.discriminator_cost()).

    numpy in -> the float32 numpy array the reference's closure returns; device tensors in -> the same values as a device tensor
    (icrl_disc_reward on the tensors: no host copies).  `.struct()` is the icrl_cost_disc_t the rollout kernels evaluate in their cost
    wave: the discriminator's own icrl_costnet_t behind the tag, read as zeta."""

    def __init__(self, disc):
        self.disc = disc

    def __repr__(self):
        return f"DiscriminatorCost({list(self.disc.hidden_sizes)}, in={self.disc.input_dims})"

    def __call__(self, obs, acs):
        out = self.disc.reward_function(obs, acs, apply_log=False)
        return out if torch.is_tensor(obs) or torch.is_tensor(acs) else out.cpu().numpy()

    def struct(self):
        inner = self.disc.struct()
        s = CostDiscT(inner.obs_dim, inner.acs_dim, inner.in_dim, COST_DISC, addr(inner))
        s._inner = inner      # (the descriptor points at it: alive as long as the descriptor is)
        return s


def _args_ws(n_runs, device, args_ws=None):
    if args_ws is not None and args_ws.numel() >= n_runs * _lib.BATCH_ARGS_BYTES:
        return args_ws
    return torch.empty(n_runs * _lib.BATCH_ARGS_BYTES, dtype=torch.uint8, device=device)


def launch_disc_trains(nets, jobs, args_ws=None):
    """the optimiser steps of one or of several discriminators (jobs of _disc_train_begin; also ConstraintNet._train_begin jobs in
    minibatch mode, with job["batch_size"]) in ONE launch sequence: icrl_cn_train_minibatch_batch, run = grid.y."""
    rows = []
    for cn, j in zip(nets, jobs):
        rows.append(CnTrainMbJobT(addr(j["s"]), p(cn.exp_avg), p(cn.exp_avg_sq), p(j["t_dev"]), p(j["nominal"]), p(j["expert"]), j["nominal"].shape[0],
                                  j["expert"].shape[0], p(j["d_off"]), p(j["d_rowep"]), j["n_ep"], 0, addr(j["hp"]), p(j["work"]), p(j["metrics"]),
                                  p(j["d_perms"]), int(j["batch_size"]), 0))
    arr = (CnTrainMbJobT * len(rows))(*rows)
    ws = _args_ws(len(rows), nets[0].device, args_ws)
    _lib.check(_lib.lib().icrl_cn_train_minibatch_batch(len(rows), arr, p(ws), ws.numel(), _lib.current_stream()), "icrl_cn_train_minibatch_batch")
    jobs[0]["_args_ws"] = ws      # (alive until the launches have run)


class GailCallback(callbacks.BaseCallback):
    """ref: gail_utils.py:500-571 — at the end of every rollout, before the policy update: one discriminator iteration on the
    rollout, eval/mean_cost on the true cost, the buffer's rewards relabelled with log D, returns and advantages recomputed.

    The work comes in three pieces — _rollout_end_begin (host: statistics, the permutation draw), launch_rollout_ends (device: all of it,
    for one run or for the S runs of a seed batch, through the same entry points) and _rollout_end_finish (host: the log records, from ONE
    device-to-host copy per launch sequence).  `perms`: None (the process-wide numpy generator, as the reference draws) or a callable
    itr -> [1, size] permutation (a run's own streams)."""

    def __init__(self, discriminator, learn_cost, true_cost_function, save_dir=None, plot_disc=False, update_freq=1, verbose=1):
        super().__init__(verbose)
        self.discriminator, self.update_freq, self.learn_cost = discriminator, update_freq, learn_cost
        self.true_cost_function = true_cost_function
        self.disc_itr, self.history, self.perms = 0, [], None
        self.batched = False      # a seed batch sets it: the rollout ends of all runs go in lock-step (seed_batch._gail_rollout_ends)

    def _on_rollout_end(self):
        if self.batched:
            return
        job = self._rollout_end_begin()
        launch_rollout_ends([self], [job])
        self._rollout_end_finish(job, job["readback"].cpu().numpy())

    def _rollout_end_begin(self):
        rb, env, disc = self.model.rollout_buffer, self.training_env, self.discriminator
        dev = rb.device
        rows, obs_dim = rb.buffer_size * rb.n_envs, int(np.prod(rb.obs_shape))
        norm = bool(getattr(env, "norm_obs", False))      # VecNormalize.unnormalize_obs with the CURRENT statistics (vec_normalize.py:125-128)
        tc = self.true_cost_function
        if isinstance(tc, AnalyticCost):
            cost = tc.struct(obs_dim, rb.action_dim)
        else:
            cost = None       # no ground truth (null_cost): 0; any other callable is evaluated on the raw observations in _rollout_end_finish
        raw = torch.empty(rb.buffer_size, rb.n_envs, obs_dim, dtype=torch.float64, device=dev)
        job = dict(raw_obs=raw, cost=cost, cost_mean=torch.zeros(1, dtype=torch.float64, device=dev), rows=rows, train=None, disc_s=None,
                   mean=env.obs_rms.d_mean if norm else None, var=env.obs_rms.d_var if norm else None,
                   epsilon=float(getattr(env, "epsilon", 0.0)), update=self.disc_itr % self.update_freq == 0, perms=None)
        if job["update"]:
            disc.current_obs_mean, disc.current_obs_var = env.obs_rms.mean, env.obs_rms.var
            if self.perms is not None:
                job["perms"] = self.perms(self.disc_itr)
        return job

    def _gail_struct(self, job):
        rb = self.model.rollout_buffer
        job["disc_s"] = self.discriminator.struct()
        return GailJobT(addr(job["disc_s"]), addr(job["cost"]), p(rb.observations), p(rb.actions), p(job["mean"]), p(job["var"]), job["epsilon"],
                        p(job["raw_obs"]), p(rb.rewards), p(job["cost_mean"]), job["rows"], int(bool(self.learn_cost)))

    def _gae_struct(self):
        rb, ag = self.model.rollout_buffer, self.model._ag
        return GaeJobT(p(rb.rewards), p(rb.costs), p(rb.reward_values), p(rb.cost_values), p(rb.dones), p(ag["last_v_r"]), p(ag["last_v_c"]),
                       p(ag["last_dones"]), p(rb.reward_advantages), p(rb.cost_advantages), p(rb.reward_returns), p(rb.cost_returns),
                       p(rb.gae_ws), rb.gae_ws.numel() * 8)

    def _rollout_end_finish(self, job, host):
        """host: this run's row of the one copy — the discriminator's metrics rows, its Adam step, the mean cost."""
        rec = {}
        tj = job["train"]
        if tj is not None:
            n = tj["metrics"].numel()
            rec = self.discriminator._disc_train_end(tj, metrics_host=host[:n].reshape(tj["metrics"].shape), adam_step_host=host[n])
            for k, v in rec.items():
                logger.record(k, v)
        tc = self.true_cost_function
        if isinstance(tc, AnalyticCost) or tc is null_cost:
            rec["eval/mean_cost"] = float(host[-1])
        else:
            rb = self.model.rollout_buffer
            c = tc(job["raw_obs"].reshape(-1, job["raw_obs"].shape[-1]), rb.actions.reshape(-1, rb.actions.shape[-1]))
            rec["eval/mean_cost"] = float(c.double().mean().item()) if torch.is_tensor(c) else float(np.mean(c))
        logger.record("eval/mean_cost", rec["eval/mean_cost"])
        self.history.append(rec)
        self.disc_itr += 1


def launch_rollout_ends(cbs, jobs, args_ws=None):
    """the device part of the rollout end of one or of several GailCallbacks (jobs of _rollout_end_begin), every step ONE launch
    (sequence) with run = grid.y: un-normalise + mean cost (icrl_gail_unnormalize_batch), the discriminator iteration
    (icrl_cn_train_minibatch_batch), the rewards relabelled with log D (icrl_gail_relabel_batch), the dual GAE (icrl_gae_dual_batch).
    Leaves job["readback"] per run: metrics rows, Adam step and mean cost as one float64 row (the caller copies them once)."""
    L, S = _lib.lib(), len(cbs)
    dev = cbs[0].model.rollout_buffer.device
    ws = _args_ws(S, dev, args_ws)
    arr = (GailJobT * S)(*[cb._gail_struct(j) for cb, j in zip(cbs, jobs)])
    _lib.check(L.icrl_gail_unnormalize_batch(S, arr, p(ws), ws.numel(), _lib.current_stream()), "icrl_gail_unnormalize_batch")
    train = [(cb, j) for cb, j in zip(cbs, jobs) if j["update"]]
    for cb, j in train:      # (prepare_data reads the raw observations: after their launch)
        j["train"] = cb.discriminator._disc_train_begin(1, j["raw_obs"], cb.model.rollout_buffer.actions, perms=j["perms"])
    if train:
        launch_disc_trains([cb.discriminator for cb, _ in train], [j["train"] for _, j in train], ws)
        for cb, _ in train:
            cb.discriminator.prepare()      # the transposed copy the row forward reads, of the updated parameters
        arr = (GailJobT * S)(*[cb._gail_struct(j) for cb, j in zip(cbs, jobs)])
    _lib.check(L.icrl_gail_relabel_batch(S, arr, p(ws), ws.numel(), _lib.current_stream()), "icrl_gail_relabel_batch")
    rb0 = cbs[0].model.rollout_buffer
    garr = (GaeJobT * S)(*[cb._gae_struct() for cb in cbs])
    _lib.check(L.icrl_gae_dual_batch(S, garr, rb0.buffer_size, rb0.n_envs, float(rb0.reward_gamma), float(rb0.reward_gae_lambda), float(rb0.cost_gamma),
                                     float(rb0.cost_gae_lambda), p(ws), ws.numel(), _lib.current_stream()), "icrl_gae_dual_batch")
    for j in jobs:
        tj = j["train"]
        parts = [] if tj is None else [tj["metrics"].reshape(-1).double(), tj["t_dev"].double()]
        j["readback"] = torch.cat(parts + [j["cost_mean"]])
        j["_args_ws"] = ws
