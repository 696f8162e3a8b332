"""Curiosity and lambda-shaping callbacks (`cpg -ucde / -uls`, `icrl -ucde`), their networks trained on the device.

ref: icrl/exploration.py:13-67 (ExplorationRewardCallback), :176-317 (LambdaShapingCallback); wired in at icrl/cpg.py:176-184 and
     icrl/icrl.py:180-183, 210.

At every rollout end the reference takes ONE full-batch Adam step of a small MLP (`create_mlp(obs + acs, out, [50, 50])`, ReLU) on all
T x N rows of the buffer and uses the per-row squared prediction error of the PRE-step network as an exploration reward.  Here that step
is one call of icrl_reg_mlp_step (csrc/reg_mlp.hip) on flat device buffers: it reads the buffer's observations / actions planes in place
(time-major rows, no concatenated copy), and `cost_advantages /= 1 + exploration_reward` is icrl_shape_advantages.  Each callback makes
one device-to-host read of its scalar block per rollout end.  The networks are initialised exactly like the reference's: the torch
modules are constructed once on the host, in the reference's order, and their tensors copied — the same draws from the global generator.

The third callback of that file, CostShapingCallback (icrl/exploration.py:73-169, `gail -ucsc [-ucn]`, wired in at icrl/gail.py:128-135), is
here too: its classifier (ClassifierNet: the same MLP with one output and a Sigmoid, BCE loss) is stepped by icrl_cls_mlp_step and read a
second time, on the stepped parameters, by icrl_cost_shaping_apply (csrc/cost_shaping.hip).
"""
import numpy as np
import torch

from . import _lib, callbacks, logger, spaces
from ._lib import ptr as p
from .structs import CostNetT, GailJobT, addr

REFUSE_SEED_BATCH = ("{flag}: the exploration callbacks' networks are per-run and unbatched; a seed batch (--seeds with more than one seed) "
                     "does not take them (run the seeds one at a time)")
REFUSE_RANKS = "{flag}: the exploration callbacks' networks would diverge across ranks (no all-reduce covers them); world_size > 1 is not served"


def refuse_batched(config, seed_batch=False):
    """raise, naming the flag, where the callbacks are not served: seed batches and several ranks.  Called before anything is launched."""
    for attr, flag in (("use_curiosity_driven_exploration", "--use_curiosity_driven_exploration (-ucde)"), ("use_lambda_shaping", "--use_lambda_shaping (-uls)")):
        on = config.get(attr, False) if isinstance(config, dict) else getattr(config, attr, False)
        if not on:
            continue
        if seed_batch:
            raise ValueError(REFUSE_SEED_BATCH.format(flag=flag))
        world = config.get("world_size", 1) if isinstance(config, dict) else getattr(config, "world_size", 1)
        if world > 1:
            raise ValueError(REFUSE_RANKS.format(flag=flag))


REFUSE_SDE_SEED_BATCH = ("--use_sde (-us): a gSDE agent runs the per-step rollout and the fine-grained update, which have no batched form; a seed batch "
                         "(--seeds with more than one seed) does not take it (run the seeds one at a time)")
REFUSE_SDE_CALLBACKS = ("--use_sde (-us) with {flag}: the exploration callbacks are served on the fused rollout's buffers only; a gSDE agent collects "
                        "through the per-step loop (use one of the two)")
REFUSE_SDE_RANKS = "--use_sde (-us): the per-rank exploration matrices and the fine-grained update are not covered by the rank collective; world_size > 1 is not served"


def refuse_sde(config, seed_batch=False):
    """raise, naming the flag, where `--use_sde` is not served: seed batches, the exploration callbacks, several ranks.  Called before
    anything is launched (cpg / icrl / gail setup, the seed-batch constructors)."""
    get = (lambda k, d=None: config.get(k, d)) if isinstance(config, dict) else (lambda k, d=None: getattr(config, k, d))
    if not get("use_sde", False):
        return
    if seed_batch:
        raise ValueError(REFUSE_SDE_SEED_BATCH)
    for attr, flag in (("use_curiosity_driven_exploration", "--use_curiosity_driven_exploration (-ucde)"), ("use_lambda_shaping", "--use_lambda_shaping (-uls)")):
        if get(attr, False):
            raise ValueError(REFUSE_SDE_CALLBACKS.format(flag=flag))
    if (get("world_size", 1) or 1) > 1:
        raise ValueError(REFUSE_SDE_RANKS)


class RegressionNet:
    """MLP(in_dim -> h1 -> ReLU -> h2 -> ReLU -> out_dim) with its Adam state as flat device buffers (torch's state_dict order)."""

    def __init__(self, in_dim, out_dim, hidden_layers=(50, 50), lr=3e-3, device="cuda"):
        hidden_layers = [int(h) for h in hidden_layers]
        self.in_dim, self.out_dim, self.hidden_layers, self.lr = int(in_dim), int(out_dim), hidden_layers, float(lr)
        self.betas, self.eps = (0.9, 0.999), 1e-8
        self.device = torch.device("cuda" if str(device) in ("cpu", "auto", "None") else device)
        if len(hidden_layers) != 2:
            raise NotImplementedError(f"RegressionNet: hidden layers {hidden_layers} are not served (two hidden layers of 1..64 units each)")
        # the reference's create_mlp(in, out, hidden): Linear, ReLU, Linear, ReLU, Linear — constructed in that order, so the global
        # generator gives what it gives the reference
        dims = [self.in_dim] + hidden_layers + [self.out_dim]
        mods = []
        for k in range(3):
            mods.append(torch.nn.Linear(dims[k], dims[k + 1]))
            if k < 2:
                mods.append(torch.nn.ReLU())
        seq = torch.nn.Sequential(*mods)
        self.keys = [k for k in seq.state_dict().keys()]      # 0.weight, 0.bias, 2.weight, 2.bias, 4.weight, 4.bias
        self.shapes = [tuple(v.shape) for v in seq.state_dict().values()]
        self.n_params = int(sum(int(np.prod(s)) for s in self.shapes))
        self.params = torch.zeros(self.n_params, device=self.device)
        self.exp_avg, self.exp_avg_sq = torch.zeros_like(self.params), torch.zeros_like(self.params)
        self.adam_step = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.out4 = torch.zeros(4, device=self.device)
        self._ws = None
        self.load_state_dict(seq.state_dict())

    def load_state_dict(self, sd):
        flat = torch.cat([torch.as_tensor(sd[k]).detach().to(torch.float32).reshape(-1).cpu() for k in self.keys])
        assert flat.numel() == self.n_params, f"state_dict of {flat.numel()} values, the network has {self.n_params}"
        self.params.copy_(flat)

    def state_dict(self):
        out, o, host = {}, 0, self.params.detach().cpu()
        for k, s in zip(self.keys, self.shapes):
            n = int(np.prod(s))
            out[k] = host[o:o + n].reshape(s).clone()
            o += n
        return out

    def step(self, xa, xb, target, row_err=None):
        """one regression step on rows (xa | xb) -> target; returns the device block {loss, mean(row_err), std(row_err), 0} of the pre-step
        predictions.  xa [rows, in_a] (None when in_a == 0), xb [rows, in_b], target [rows, out_dim]; row_err [rows] is written when given."""
        rows = int(target.numel() // self.out_dim)
        in_b = int(xb.numel() // rows)
        in_a = self.in_dim - in_b
        h1, h2 = self.hidden_layers
        L = _lib.lib()
        need = int(L.icrl_reg_mlp_ws_bytes(rows, in_a, in_b, h1, h2, self.out_dim))
        if need == 0:
            reason = L.icrl_last_error().decode()
            L.icrl_clear_error()
            raise NotImplementedError(reason)
        if self._ws is None or self._ws.numel() * 8 < need:
            self._ws = torch.empty((need + 7) // 8, dtype=torch.int64, device=self.device)
        _lib.check(L.icrl_reg_mlp_step(p(self.params), p(self.exp_avg), p(self.exp_avg_sq), p(self.adam_step), p(xa) if in_a > 0 else None, p(xb),
                                       p(target), rows, in_a, in_b, h1, h2, self.out_dim, self.lr, self.betas[0], self.betas[1], self.eps,
                                       p(row_err), p(self.out4), p(self._ws), self._ws.numel() * 8, _lib.current_stream()), "icrl_reg_mlp_step")
        return self.out4


def _check_shapes(who, obs_dim, acs_dim, layer_sets):
    L = _lib.lib()
    for hidden, out in layer_sets:
        hidden = list(hidden)
        if len(hidden) != 2:
            raise NotImplementedError(f"{who}: hidden layers {hidden} are not served (two hidden layers of 1..64 units each)")
        if int(L.icrl_reg_mlp_ws_bytes(1, int(obs_dim), int(acs_dim), int(hidden[0]), int(hidden[1]), int(out))) == 0:
            reason = L.icrl_last_error().decode()
            L.icrl_clear_error()
            raise NotImplementedError(f"{who}: {reason}")


def _require_box(who, model):
    if isinstance(model.env.action_space, spaces.Discrete) or getattr(model.policy, "discrete", False):
        raise ValueError(f"{who}: a Box action space is needed (the buffer stores a discrete action as one index column, which the reference "
                         "reshapes to acs_dim columns: not a meaningful network input)")


class ExplorationRewardCallback(callbacks.BaseCallback):
    """ref: icrl/exploration.py:13-67 — a network predicts the next observation from (observation, action); at rollout end it takes one
    step on the whole buffer, the per-row squared error is ADDED to rollout_buffer.rewards, and exploration/predictor_network_loss =
    mean(row error) (what the reference logs under that name — not the MSE).

    on_rollout_end runs after GAE, in the reference (on_policy_algorithm collect_rollouts) as here: the callback changes the stored rewards
    but NOT the advantages / returns the update consumes, so by default it has no effect on training, exactly like the reference's.
    `recompute_advantages=True` (library-only, no CLI flag) re-runs compute_returns_and_advantage on the changed rewards with the rollout's
    last values and dones, as GailCallback does after relabelling, so the bonus reaches the update."""

    def __init__(self, obs_dim, acs_dim, hidden_layers=[50, 50], device="cpu", verbose=1, recompute_advantages=False):
        super().__init__(verbose)
        self.obs_dim, self.acs_dim, self.hidden_layers, self.device = int(obs_dim), int(acs_dim), list(hidden_layers), device
        self.recompute_advantages = bool(recompute_advantages)
        _check_shapes("ExplorationRewardCallback", obs_dim, acs_dim, [(hidden_layers, obs_dim)])
        self.predictor_network = RegressionNet(self.obs_dim + self.acs_dim, self.obs_dim, self.hidden_layers, lr=3e-3, device=device)
        self.row_err, self.history = None, []

    def _init_callback(self):
        _require_box("ExplorationRewardCallback (--use_curiosity_driven_exploration)", self.model)

    def _on_rollout_end(self):
        rb = self.model.rollout_buffer
        rows = rb.buffer_size * rb.n_envs
        if self.row_err is None or self.row_err.numel() != rows:
            self.row_err = torch.empty(rows, device=rb.device)
        out4 = self.predictor_network.step(rb.observations, rb.actions, rb.new_observations, self.row_err)
        rb.rewards += self.row_err.view(rb.buffer_size, rb.n_envs)
        if self.recompute_advantages:
            ag = self.model._ag
            rb.compute_returns_and_advantage(ag["last_v_r"], ag["last_v_c"], ag["last_dones"])
        host = out4.cpu().numpy()
        rec = {"exploration/predictor_network_loss": float(host[1])}
        for k, v in rec.items():
            logger.record(k, v)
        self.history.append(rec)


class LambdaShapingCallback(callbacks.BaseCallback):
    """ref: icrl/exploration.py:176-317 — at rollout end: one step of a cost network on (observation, action) -> the buffer's costs, one
    step of the next-observation predictor, and cost_advantages /= 1 + per-row prediction error (the cost weighs less where the state is
    novel).  Runs after GAE and before the update, which consumes the shaped plane.  The networks are created in _init_callback, cost
    network first, as in the reference."""

    def __init__(self, obs_dim, acs_dim, cost_net_hidden_layers=[50, 50], predictor_net_hidden_layers=[50, 50], device="cpu", verbose=1):
        super().__init__(verbose)
        self.obs_dim, self.acs_dim, self.device = int(obs_dim), int(acs_dim), device
        self.cost_net_hidden_layers, self.predictor_net_hidden_layers = list(cost_net_hidden_layers), list(predictor_net_hidden_layers)
        _check_shapes("LambdaShapingCallback", obs_dim, acs_dim, [(cost_net_hidden_layers, 1), (predictor_net_hidden_layers, obs_dim)])
        self.cost_net = self.predictor_network = self.row_err = None
        self.history = []

    def _init_callback(self):
        _require_box("LambdaShapingCallback (--use_lambda_shaping)", self.model)
        self.cost_net = RegressionNet(self.obs_dim + self.acs_dim, 1, self.cost_net_hidden_layers, lr=3e-3, device=self.device)
        self.predictor_network = RegressionNet(self.obs_dim + self.acs_dim, self.obs_dim, self.predictor_net_hidden_layers, lr=3e-3, device=self.device)

    def _on_rollout_end(self):
        rb = self.model.rollout_buffer
        rows = rb.buffer_size * rb.n_envs
        if self.row_err is None or self.row_err.numel() != rows:
            self.row_err = torch.empty(rows, device=rb.device)
        c4 = self.cost_net.step(rb.observations, rb.actions, rb.costs)
        p4 = self.predictor_network.step(rb.observations, rb.actions, rb.new_observations, self.row_err)
        _lib.check(_lib.lib().icrl_shape_advantages(p(rb.cost_advantages), p(self.row_err), rows, _lib.current_stream()), "icrl_shape_advantages")
        host = torch.cat([p4, c4]).cpu().numpy()
        rec = {"exploration/mean_exploration_reward": float(host[1]), "exploration/std_exploration_reward": float(host[2]),
               "exploration/predictor_network_loss": float(host[0]), "exploration/cost_network_loss": float(host[4])}
        for k, v in rec.items():
            logger.record(k, v)
        self.history.append(rec)


COST_SHAPING_FLAG = "--use_cost_shaping_callback (-ucsc)"


def refuse_cost_shaping(config):
    """raise, naming the flag, where `gail --use_cost_shaping_callback` is not served: several ranks and a gSDE agent.  Called before
    anything is launched (gail.setup)."""
    get = (lambda k, d=None: config.get(k, d)) if isinstance(config, dict) else (lambda k, d=None: getattr(config, k, d))
    if not get("use_cost_shaping_callback", False):
        return
    if get("use_sde", False):
        raise ValueError(REFUSE_SDE_CALLBACKS.format(flag=COST_SHAPING_FLAG))
    if (get("world_size", 1) or 1) > 1:
        raise ValueError(REFUSE_RANKS.format(flag=COST_SHAPING_FLAG))


class ClassifierNet(RegressionNet):
    """sigmoid(MLP(in_dim -> h1 -> ReLU -> h2 -> ReLU -> 1)) with its Adam state as flat device buffers: RegressionNet's construction (the
    same Linear layers in the same order — the Sigmoid has no parameters — so the global generator gives the reference's initial weights)
    and state_dict, stepped by icrl_cls_mlp_step (BCE loss) and read by icrl_cost_shaping_apply (csrc/cost_shaping.hip).  `out8` (device,
    float64) holds {loss, mean(p), mean(target), 0} of the last step and {mean, min, max of shaped, 0} of the last apply."""

    def __init__(self, in_dim, hidden_layers=(50, 50), lr=3e-3, device="cuda"):
        super().__init__(in_dim, 1, hidden_layers, lr=lr, device=device)
        self.out8 = torch.zeros(8, dtype=torch.float64, device=self.device)

    def _workspace(self, rows, in_a, in_b):
        h1, h2 = self.hidden_layers
        L = _lib.lib()
        need = int(L.icrl_cls_mlp_ws_bytes(rows, in_a, in_b, h1, h2))
        if need == 0:
            reason = L.icrl_last_error().decode()
            L.icrl_clear_error()
            raise NotImplementedError(reason)
        if self._ws is None or self._ws.numel() * 8 < need:
            self._ws = torch.empty((need + 7) // 8, dtype=torch.int64, device=self.device)
        return self._ws

    def step(self, xa, xb, target):
        """one classifier step on rows (float32(xa) | xb) -> target; returns the device block {loss, mean(p), mean(target), 0} (float64) of the
        pre-step predictions.  xa [rows, in_a] float64 (None when in_a == 0), xb [rows, in_b] float32, target [rows] float32."""
        rows = int(target.numel())
        in_b = int(xb.numel() // rows)
        in_a = self.in_dim - in_b
        h1, h2 = self.hidden_layers
        ws = self._workspace(rows, in_a, in_b)
        out4 = self.out8[:4]
        _lib.check(_lib.lib().icrl_cls_mlp_step(p(self.params), p(self.exp_avg), p(self.exp_avg_sq), p(self.adam_step), p(xa) if in_a > 0 else None, p(xb),
                                                p(target), rows, in_a, in_b, h1, h2, self.lr, self.betas[0], self.betas[1], self.eps, p(out4), p(ws),
                                                ws.numel() * 8, _lib.current_stream()), "icrl_cls_mlp_step")
        return out4

    def apply(self, xa, xb, target, rewards, use_nn=True):
        """rewards += log(float32 prediction) of the parameters as they are (use_nn), or += log(1e-3) * target in float64 rounded once;
        returns the device block {mean, min, max of the shaped cost, 0} (float64)."""
        rows = int(rewards.numel())
        in_b = int(xb.numel() // rows)
        in_a = self.in_dim - in_b
        h1, h2 = self.hidden_layers
        ws = self._workspace(rows, in_a, in_b)
        out4 = self.out8[4:]
        _lib.check(_lib.lib().icrl_cost_shaping_apply(p(self.params) if use_nn else None, p(xa) if in_a > 0 else None, p(xb), p(target), rows, in_a, in_b,
                                                      h1, h2, p(rewards), p(out4), p(ws), ws.numel() * 8, _lib.current_stream()),
                   "icrl_cost_shaping_apply")
        return out4


def _check_cls_shapes(who, obs_dim, acs_dim, hidden):
    hidden = list(hidden)
    if len(hidden) != 2:
        raise NotImplementedError(f"{who}: hidden layers {hidden} are not served (two hidden layers of 1..64 units each)")
    L = _lib.lib()
    if int(L.icrl_cls_mlp_ws_bytes(1, int(obs_dim), int(acs_dim), int(hidden[0]), int(hidden[1]))) == 0:
        reason = L.icrl_last_error().decode()
        L.icrl_clear_error()
        raise NotImplementedError(f"{who}: {reason}")


class CostShapingCallback(callbacks.BaseCallback):
    """ref: icrl/exploration.py:73-169 (`gail -ucsc [-ucn]`, installed in the place of GailCallback) — a classifier learns the true cost
    and its log-prediction shapes the rewards.  At every rollout end, in the reference's order:
      1. raw observations: the buffer's plane un-normalised with the env's CURRENT statistics, float64 (icrl_gail_unnormalize_batch as a
         batch of one: float64(obs) * sqrt(var + eps) + mean, product and sum rounded separately; unchanged with norm_obs off);
      2. the STORED actions (not the clipped ones);
      3. true costs of (raw observations, actions): an AnalyticCost / RegionCost through its rows kernel on the device, any other callable
         on host copies.  The analytic torque cost compares the float32 action in the rows kernel where the reference compares its float64
         copy: identical for every threshold of TRUE_COSTS (0.5 is exact in both formats);
      4. ONE Adam step of the cost network on float32(raw observation | action) -> true cost, BCE loss (icrl_cls_mlp_step);
      5. shaped = log(prediction of the STEPPED network) in float32, added to rollout_buffer.rewards (icrl_cost_shaping_apply);
      6. CostShaping/{mean_true_cost, mean_shaped_cost, min_shaped_cost, max_shaped_cost, cost_network_loss (pre-step)}: ONE device-to-host
         copy of the two scalar blocks.

    Like the reference's, the callback runs after GAE: it changes the stored rewards, NOT the advantages / returns the update consumes, so by
    default it has no effect on training.  `recompute_advantages=True` (library-only, no CLI flag) re-runs compute_returns_and_advantage on
    the changed rewards with the rollout's last values and dones.

    use_nn_for_shaping=False is the one place where this build does not reproduce the reference, because the reference has no behaviour to
    reproduce: its `np.log(1e-3) * self.get_true_cost(self, obs, acs)` passes one argument too many and raises TypeError at the first
    rollout end.  Served here is the evident intent: shaped = log(1e-3) * true cost in float64, added to the float32 plane in place (rounded
    once); the network is still stepped and its loss logged."""

    def __init__(self, true_cost_function, obs_dim, acs_dim, use_nn_for_shaping, cost_net_hidden_layers=[50, 50], device="cpu", verbose=1,
                 recompute_advantages=False):
        super().__init__(verbose)
        self.true_cost_function = true_cost_function
        self.obs_dim, self.acs_dim, self.use_nn, self.device = int(obs_dim), int(acs_dim), bool(use_nn_for_shaping), device
        self.cost_net_hidden_layers = list(cost_net_hidden_layers)
        self.recompute_advantages = bool(recompute_advantages)
        _check_cls_shapes(f"CostShapingCallback ({COST_SHAPING_FLAG})", obs_dim, acs_dim, self.cost_net_hidden_layers)
        self.cost_net = self.raw_observations = self.true_costs = self._args_ws = None
        self.history = []

    def _init_callback(self):
        _require_box(f"CostShapingCallback ({COST_SHAPING_FLAG})", self.model)
        self.cost_net = ClassifierNet(self.obs_dim + self.acs_dim, self.cost_net_hidden_layers, lr=3e-3, device=self.device)

    def _unnormalize(self, rb, env):
        """step 1: -> [T, N, obs] float64 on the device."""
        norm = bool(getattr(env, "norm_obs", False))
        rows = rb.buffer_size * rb.n_envs
        raw = torch.empty(rb.buffer_size, rb.n_envs, self.obs_dim, dtype=torch.float64, device=rb.device)
        if self._args_ws is None:
            self._args_ws = torch.empty(_lib.BATCH_ARGS_BYTES, dtype=torch.uint8, device=rb.device)
            self._cost_mean = torch.zeros(1, dtype=torch.float64, device=rb.device)
        shape = CostNetT(obs_dim=self.obs_dim, acs_dim=self.acs_dim, in_dim=self.obs_dim + self.acs_dim, n_hidden=1, h1=1)      # read for its widths only
        job = GailJobT(addr(shape), None, p(rb.observations), p(rb.actions), p(env.obs_rms.d_mean) if norm else None, p(env.obs_rms.d_var) if norm else None,
                       float(getattr(env, "epsilon", 0.0)), p(raw), None, p(self._cost_mean), rows, 0)
        _lib.check(_lib.lib().icrl_gail_unnormalize_batch(1, (GailJobT * 1)(job), p(self._args_ws), self._args_ws.numel(), _lib.current_stream()),
                   "icrl_gail_unnormalize_batch")
        return raw

    def _true_costs(self, raw, actions):
        """step 3: -> [rows] float32 on the device."""
        from .true_constraint_net import AnalyticCost, RegionCost
        tc = self.true_cost_function
        if isinstance(tc, (AnalyticCost, RegionCost)):
            c = tc(raw, actions)
        else:
            c = tc(raw.cpu().numpy(), actions.cpu().numpy().astype(float))
            c = torch.as_tensor(np.asarray(c).astype(np.float32), device=raw.device)
        c = c.to(torch.float32).reshape(-1).contiguous()
        if c.numel() != raw.shape[0] * raw.shape[1]:
            raise ValueError(f"CostShapingCallback: the true cost gave {c.numel()} values for {raw.shape[0] * raw.shape[1]} rows (the reference's "
                             "null cost returns one per time step, and its callback fails at the loss in the same way)")
        return c

    def _on_rollout_end(self):
        rb = self.model.rollout_buffer
        raw = self.raw_observations = self._unnormalize(rb, self.training_env)
        target = self.true_costs = self._true_costs(raw, rb.actions)
        self.cost_net.step(raw, rb.actions, target)
        self.cost_net.apply(raw, rb.actions, target, rb.rewards, use_nn=self.use_nn)
        if self.recompute_advantages:
            ag = self.model._ag
            rb.compute_returns_and_advantage(ag["last_v_r"], ag["last_v_c"], ag["last_dones"])
        host = self.cost_net.out8.cpu().numpy()
        rec = {"CostShaping/mean_true_cost": float(host[2]), "CostShaping/mean_shaped_cost": float(host[4]), "CostShaping/min_shaped_cost": float(host[5]),
               "CostShaping/max_shaped_cost": float(host[6]), "CostShaping/cost_network_loss": float(host[0])}
        for k, v in rec.items():
            logger.record(k, v)
        self.history.append(rec)
