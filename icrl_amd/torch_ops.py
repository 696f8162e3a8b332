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
gradient.  There is no torch fallback: a shape the kernels do not serve raises NotImplementedError with the library's reason.
"""
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


def evaluate_actions(policy, obs, actions, params=None):
    """ActorTwoCriticsPolicy.evaluate_actions (ref: policies.py:752-767) as an autograd function of `params`:
    -> (v_r, v_c, log_prob, entropy), float32 [N] each.  obs [N, obs_dim] (float32 rows, e.g. icrl_minibatch_gather's), actions
    [N, act_dim] ([N] or [N, 1] class indices when discrete)."""
    dev = policy.params.device
    a_store = 1 if policy.discrete else policy.act_dim
    obs = torch.as_tensor(obs, device=dev).detach().to(torch.float32).reshape(-1, policy.obs_dim).contiguous()
    actions = torch.as_tensor(actions, device=dev).detach().to(torch.float32).reshape(-1, a_store).contiguous()
    if actions.shape[0] != obs.shape[0]:
        raise ValueError(f"{obs.shape[0]} observations, {actions.shape[0]} actions")
    return _EvaluateActions.apply(_params(policy, params), policy, obs, actions)


def zeta(constraint_net, obs, acs, params=None):
    """zeta_theta(obs, acs) = sigmoid(MLP_relu(prepare_data(obs, acs))) (ref: constraint_net.py:101-130, 258-299) as an autograd function
    of `params` -> float32 [N]; takes what `cost_function` takes (obs float64, acs float32; cost = 1 - zeta)."""
    x = constraint_net.prepare_data(obs, acs)       # icrl_cn_prepare: normalise, clip, one-hot, select
    return _Zeta.apply(_params(constraint_net, params), constraint_net, x)
