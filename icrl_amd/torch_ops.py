"""The two networks as differentiable torch functions over the library's own flat parameter buffers.

`ActorTwoCriticsPolicy.evaluate_actions` and `ConstraintNet.cost_function` return plain tensors.  The functions here run the same
networks through icrl_policy_fwd_bwd / icrl_cost_mlp_fwd_bwd (csrc/mlp_grad.hip) as `torch.autograd.Function`s, so a loss written in
torch on (v_r, v_c, log_prob, entropy) or on zeta sends its gradient into a flat float32 leaf in the object's device layout:

    v_r, v_c, log_prob, entropy = torch_ops.evaluate_actions(policy, obs, actions)       # [N] each
    loss = my_surrogate(log_prob, ...) + (v_r - returns).pow(2).mean() - 0.01 * entropy.mean()
    loss.backward()
    g = torch_ops.leaf(policy).grad          # [n_params], the layout of policy.params: feed icrl_clip_adam_step, or any torch optimiser

`params` defaults to `leaf(obj)`: a leaf that VIEWS the object's own `params` (same memory; the object's tensor itself stays a plain
tensor, so nothing else in the package changes behaviour).  The backward recomputes the forward from (params, inputs); inputs get no
gradient unless the call says `input_grads=True`: then obs / actions (obs / acs of the constraint net) are differentiable too, through
icrl_policy_fwd_bwd_in / icrl_cost_mlp_fwd_bwd_in + icrl_cn_prepare_bwd — saliency, d cost / d action, adversarial observations:

    obs = obs.requires_grad_(True)
    torch_ops.zeta(constraint_net, obs, acs, input_grads=True).sum().backward()           # obs.grad: float64 [N, obs_dim]

There is no torch fallback: a shape the kernels do not serve raises NotImplementedError with the library's reason.
"""
import numpy as np
import torch

from . import _lib
from .structs import p


def leaf(obj):
    """The autograd leaf over `obj.params` (an ActorTwoCriticsPolicy or a ConstraintNet) that the functions here use by default:
    created on first use, shares the object's memory, collects `.grad` like any leaf."""
    t = getattr(obj, "_torch_ops_leaf", None)
    if t is None or t.data_ptr() != obj.params.data_ptr():
        t = obj.params.detach().requires_grad_(True)
        obj._torch_ops_leaf = t
    return t


def _params(obj, params):
    if params is None:
        return leaf(obj)
    if not (torch.is_tensor(params) and params.is_cuda and params.dtype == torch.float32 and params.is_contiguous() and params.numel() == obj.n_params):
        raise ValueError(f"params: a contiguous float32 CUDA tensor of {obj.n_params} elements in the object's device layout")
    return params


def _workspace(obj, key, n, nbytes_fn, what):
    """device scratch of the backward, cached per (object, N); an unserved shape surfaces here with the library's reason."""
    cache = obj.__dict__.setdefault("_torch_ops_ws", {})
    ws = cache.get((key, n))
    if ws is None:
        L = _lib.lib()
        s = obj.struct()
        nbytes = nbytes_fn(L)(_lib.byref(s), n)
        if nbytes == 0:
            reason = L.icrl_last_error().decode()
            L.icrl_clear_error()
            raise NotImplementedError(f"{what}: {reason}")
        ws = cache[(key, n)] = torch.empty(nbytes // 8, dtype=torch.float64, device=obj.params.device)
    return ws


class _EvaluateActions(torch.autograd.Function):
    @staticmethod
    def _call(policy, params, obs, actions, d, outs, grad, ws):
        s = policy.struct()
        s.params = params.data_ptr()
        _lib.check(_lib.lib().icrl_policy_fwd_bwd(_lib.byref(s), p(obs), p(actions), obs.shape[0], *(p(x) for x in d), *(p(x) for x in outs), p(grad),
                                                  p(ws) if grad is not None else None, 0 if grad is None else ws.numel() * 8, _lib.current_stream()),
                   "icrl_policy_fwd_bwd")

    @staticmethod
    def forward(ctx, params, policy, obs, actions):
        n = obs.shape[0]
        ws = _workspace(policy, "policy", n, lambda L: L.icrl_policy_fwd_bwd_ws_bytes, "torch_ops.evaluate_actions")
        outs = tuple(torch.empty(n, device=obs.device) for _ in range(4))
        _EvaluateActions._call(policy, params, obs, actions, (None,) * 4, outs, None, None)
        ctx.policy, ctx.ws = policy, ws
        ctx.save_for_backward(params, obs, actions)
        return outs

    @staticmethod
    def backward(ctx, g_v_r, g_v_c, g_log_prob, g_entropy):
        params, obs, actions = ctx.saved_tensors
        d = tuple(None if g is None else g.to(torch.float32).contiguous() for g in (g_v_r, g_v_c, g_log_prob, g_entropy))
        grad = torch.empty_like(params)
        _EvaluateActions._call(ctx.policy, params, obs, actions, d, (None,) * 4, grad, ctx.ws)
        return grad, None, None, None


class _Zeta(torch.autograd.Function):
    @staticmethod
    def _call(cn, params, x, d_zeta, zeta, grad, ws):
        s = cn.struct()
        s.params = params.data_ptr()
        _lib.check(_lib.lib().icrl_cost_mlp_fwd_bwd(_lib.byref(s), p(x), x.shape[0], p(d_zeta), p(zeta), p(grad), p(ws) if grad is not None else None,
                                                    0 if grad is None else ws.numel() * 8, _lib.current_stream()), "icrl_cost_mlp_fwd_bwd")

    @staticmethod
    def forward(ctx, params, cn, x):
        n = x.shape[0]
        ws = _workspace(cn, "zeta", n, lambda L: L.icrl_cost_mlp_fwd_bwd_ws_bytes, "torch_ops.zeta")
        out = torch.empty(n, device=x.device)
        _Zeta._call(cn, params, x, None, out, None, None)
        ctx.cn, ctx.ws = cn, ws
        ctx.save_for_backward(params, x)
        return out

    @staticmethod
    def backward(ctx, g):
        params, x = ctx.saved_tensors
        grad = torch.empty_like(params)
        _Zeta._call(ctx.cn, params, x, g.to(torch.float32).contiguous(), None, grad, ctx.ws)
        return grad, None, None


class _EvaluateActionsIn(torch.autograd.Function):
    """input_grads=True: the forward is _EvaluateActions' (the same entry point, the same bits); the backward goes through
    icrl_policy_fwd_bwd_in and hands obs / actions their gradients where they ask for one."""

    @staticmethod
    def forward(ctx, params, policy, obs, actions):
        n = obs.shape[0]
        ws = _workspace(policy, "policy_in", n, lambda L: L.icrl_policy_fwd_bwd_in_ws_bytes, "torch_ops.evaluate_actions")
        outs = tuple(torch.empty(n, device=obs.device) for _ in range(4))
        _EvaluateActions._call(policy, params, obs, actions, (None,) * 4, outs, None, None)
        ctx.policy, ctx.ws = policy, ws
        ctx.save_for_backward(params, obs, actions)
        return outs

    @staticmethod
    def backward(ctx, g_v_r, g_v_c, g_log_prob, g_entropy):
        params, obs, actions = ctx.saved_tensors
        policy = ctx.policy
        d = tuple(None if g is None else g.to(torch.float32).contiguous() for g in (g_v_r, g_v_c, g_log_prob, g_entropy))
        grad = torch.empty_like(params) if ctx.needs_input_grad[0] else None
        d_obs = torch.empty_like(obs) if ctx.needs_input_grad[2] else None
        d_act = torch.empty_like(actions) if ctx.needs_input_grad[3] and not policy.discrete else None
        if grad is None and d_obs is None and d_act is None:
            return None, None, None, None
        s = policy.struct()
        s.params = params.data_ptr()
        _lib.check(_lib.lib().icrl_policy_fwd_bwd_in(_lib.byref(s), p(obs), p(actions), obs.shape[0], *(p(x) for x in d), None, None, None, None, p(grad),
                                                     p(d_obs), p(d_act), p(ctx.ws), ctx.ws.numel() * 8, _lib.current_stream()), "icrl_policy_fwd_bwd_in")
        return grad, None, d_obs, d_act


class _ZetaIn(torch.autograd.Function):
    """input_grads=True: zeta as a function of (params, obs, acs).  The backward runs icrl_cost_mlp_fwd_bwd_in on the prepared rows and
    icrl_cn_prepare_bwd through prepare_data, with the normalisation and clip constants the forward saw."""

    @staticmethod
    def forward(ctx, params, cn, obs, acs):
        n = obs.shape[0]
        ws = _workspace(cn, "zeta_in", n, lambda L: L.icrl_cost_mlp_fwd_bwd_in_ws_bytes, "torch_ops.zeta")
        x = cn.prepare_data(obs, acs)
        out = torch.empty(n, device=x.device)
        _Zeta._call(cn, params, x, None, out, None, None)
        ctx.cn, ctx.ws, ctx.struct = cn, ws, cn.struct()
        ctx.consts = (cn.d_select, cn.d_low, cn.d_high, cn.d_mean, cn.d_var)      # (kept alive: the struct holds their addresses)
        ctx.save_for_backward(params, obs, acs, x)
        return out

    @staticmethod
    def backward(ctx, g):
        params, obs, acs, x = ctx.saved_tensors
        cn, s, L = ctx.cn, ctx.struct, _lib.lib()
        s.params = params.data_ptr()
        want_obs, want_acs = ctx.needs_input_grad[2], ctx.needs_input_grad[3] and not cn.is_discrete
        grad = torch.empty_like(params) if ctx.needs_input_grad[0] else None
        d_x = torch.empty_like(x) if want_obs or want_acs else None
        if grad is None and d_x is None:
            return None, None, None, None
        _lib.check(L.icrl_cost_mlp_fwd_bwd_in(_lib.byref(s), p(x), x.shape[0], p(g.to(torch.float32).contiguous()), None, p(grad), p(d_x), p(ctx.ws),
                                              ctx.ws.numel() * 8, _lib.current_stream()), "icrl_cost_mlp_fwd_bwd_in")
        d_obs = torch.empty_like(obs) if want_obs else None
        d_acs = torch.empty_like(acs) if want_acs else None
        if d_x is not None:
            _lib.check(L.icrl_cn_prepare_bwd(_lib.byref(s), p(obs), p(acs), x.shape[0], p(d_x), p(d_obs), p(d_acs), _lib.current_stream()),
                       "icrl_cn_prepare_bwd")
        return grad, None, d_obs, d_acs


def evaluate_actions(policy, obs, actions, params=None, input_grads=False):
    """ActorTwoCriticsPolicy.evaluate_actions (ref: policies.py:752-767) as an autograd function of `params`:
    -> (v_r, v_c, log_prob, entropy), float32 [N] each.  obs [N, obs_dim] (float32 rows, e.g. icrl_minibatch_gather's), actions
    [N, act_dim] ([N] or [N, 1] class indices when discrete).
    input_grads=True: also a function of `obs` and (Box action spaces) `actions` — the tensors among them that require grad receive
    d loss / d obs resp. d loss / d actions in float32 (icrl_policy_fwd_bwd_in); class indices get none.  The default is the call as it
    always was: inputs are detached and get no gradient."""
    dev = policy.params.device
    a_store = 1 if policy.discrete else policy.act_dim
    obs, actions = torch.as_tensor(obs, device=dev), torch.as_tensor(actions, device=dev)
    if not input_grads:
        obs, actions = obs.detach(), actions.detach()
    obs = obs.to(torch.float32).reshape(-1, policy.obs_dim).contiguous()
    actions = actions.to(torch.float32).reshape(-1, a_store).contiguous()
    if actions.shape[0] != obs.shape[0]:
        raise ValueError(f"{obs.shape[0]} observations, {actions.shape[0]} actions")
    fn = _EvaluateActionsIn if input_grads else _EvaluateActions
    return fn.apply(_params(policy, params), policy, obs, actions)


def zeta(constraint_net, obs, acs, params=None, input_grads=False):
    """zeta_theta(obs, acs) = sigmoid(MLP_relu(prepare_data(obs, acs))) (ref: constraint_net.py:101-130, 258-299) as an autograd function
    of `params` -> float32 [N]; takes what `cost_function` takes (obs float64, acs float32; cost = 1 - zeta).
    input_grads=True: also a function of `obs` (float64) and, for a Box action space, `acs` (float32): the tensors among them that require
    grad receive their gradient through the network (icrl_cost_mlp_fwd_bwd_in) and through prepare_data (icrl_cn_prepare_bwd: selection,
    clips, normalisation).  The default is the call as it always was."""
    if not input_grads:
        x = constraint_net.prepare_data(obs, acs)       # icrl_cn_prepare: normalise, clip, one-hot, select
        return _Zeta.apply(_params(constraint_net, params), constraint_net, x)
    dev = constraint_net.device
    a_w = 1 if constraint_net.is_discrete else constraint_net.acs_dim
    obs = torch.as_tensor(np.asarray(obs) if not torch.is_tensor(obs) else obs, device=dev).to(torch.float64).reshape(-1, constraint_net.obs_dim).contiguous()
    acs = torch.as_tensor(np.asarray(acs) if not torch.is_tensor(acs) else acs, device=dev).to(torch.float32).reshape(-1, a_w).contiguous()
    return _ZetaIn.apply(_params(constraint_net, params), constraint_net, obs, acs)
