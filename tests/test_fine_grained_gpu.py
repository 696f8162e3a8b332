"""GPU: the fine-grained entry points of the update (csrc/fine.hip) driven the way a maintainer of the
reference would bind them — the MLPs and autograd stay in torch (here: the oracle's torch policy on the CPU standing in for
`policy.evaluate_actions`), the library computes the loss terms and d loss / d outputs, then clip_grad_norm_ + Adam on the flat
parameter buffer — against the reference's own numbers (tests/golden/g4: its policy / optimizer objects stepped 3 x on one batch)."""
import ctypes

import numpy as np
import pytest
import torch

from helpers import fine_cases as F      # the banded minibatch, the oracle's row gradients, the is-weights case, the CPU-measured bounds
from oracle import nets as o_nets, ppo as o_ppo

pytestmark = pytest.mark.gpu


def _sub(g, prefix):
    return {k[len(prefix):]: g[k] for k in g.files if k.startswith(prefix)}


def _dev(x, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=dtype).cuda().contiguous()


def test_loss_fwd_bwd_and_clip_adam_reproduce_the_reference_steps(golden):
    """ppo_lag.py:216-288 with the network in torch and everything else in the library: three consecutive optimiser steps."""
    from icrl_amd import _lib, structs as S
    L = _lib.lib()
    g = golden("g4_ppo_minibatch")
    B = int(g["obs"].shape[0])
    pol = o_nets.TwoCriticPolicy(18, 6)
    pol.load_state_dict(_sub(g, "w0/"))
    names = list(pol.params)
    sizes = [int(pol.params[k].numel()) for k in names]
    n = sum(sizes)
    flat = _dev(np.concatenate([pol.params[k].detach().numpy().ravel() for k in names]))
    m, v = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    step = torch.zeros(1, dtype=torch.int32, device="cuda")
    work, out2, terms = torch.zeros(256, device="cuda"), torch.zeros(2, device="cuda"), torch.zeros(8, device="cuda")
    hp = S.PpoHyperT(B, 1, 0, 0)
    hp.clip_range, hp.ent_coef, hp.reward_vf_coef, hp.cost_vf_coef, hp.max_grad_norm = float(g["clip"]), 0.0, 0.5, 0.5, 0.5
    hp.clip_range_reward_vf = hp.clip_range_cost_vf = -1.0
    hp.lr, hp.adam_beta1, hp.adam_beta2, hp.adam_eps = float(g["lr"]), 0.9, 0.999, 1e-5
    nu = _dev(np.float32([float(g["nu"])]))
    dev = {k: _dev(g[k]) for k in ("old_lp", "adv_r", "adv_c", "ret_r", "ret_c")}
    obs, act = torch.as_tensor(g["obs"]), torch.as_tensor(g["act"])
    st = _lib.current_stream()
    for s in range(3):
        # ---- the host's part: forward through ITS networks (torch, autograd on)
        for k in names:
            pol.params[k].grad = None
        v_r, v_c, lp, ent = pol.evaluate_actions(obs, act)
        v_r, v_c = v_r.flatten(), v_c.flatten()
        ent_t = ent if ent is not None and ent.dim() > 0 else None
        # ---- the library's part 1: loss terms + d loss / d outputs
        d_lp, d_vr, d_vc, d_en = (torch.empty(B, device="cuda") for _ in range(4))
        o_lp, o_vr, o_vc = _dev(lp.detach().numpy()), _dev(v_r.detach().numpy()), _dev(v_c.detach().numpy())      # (kept alive across the call)
        o_en = _dev(ent_t.detach().numpy()) if ent_t is not None else None
        args = [_lib.ptr(o_lp), _lib.ptr(dev["old_lp"]), _lib.ptr(dev["adv_r"]), _lib.ptr(dev["adv_c"]),
                _lib.ptr(o_vr), _lib.ptr(o_vc), _lib.ptr(dev["ret_r"]), _lib.ptr(dev["ret_c"]), None, None,
                _lib.ptr(o_en), _lib.ptr(nu), ctypes.byref(hp), B, _lib.ptr(terms),
                _lib.ptr(d_lp), _lib.ptr(d_vr), _lib.ptr(d_vc), _lib.ptr(d_en) if ent_t is not None else None, st]
        _lib.check(L.icrl_ppo_lag_loss_fwd_bwd(*args), "icrl_ppo_lag_loss_fwd_bwd")
        t = terms.cpu().numpy()
        for i, key in enumerate(("loss", "policy_loss", "rvl", "cvl", "entropy_loss", "approx_kl", "clip_fraction")):
            ref = float(g[f"s{s}/{key}"])
            assert abs(t[i] - ref) <= 2e-6 + 2e-5 * abs(ref), (s, key, t[i], ref)
        # ---- the host's part: backward through its networks from the library's output gradients
        outs, grads = [lp, v_r, v_c], [d_lp.cpu(), d_vr.cpu(), d_vc.cpu()]
        if ent_t is not None:
            outs.append(ent_t); grads.append(d_en.cpu())
        torch.autograd.backward(outs, grads)
        for k in names:
            ref = g[f"s{s}/grad/{k}"]
            got = pol.params[k].grad.numpy()
            assert np.allclose(got, ref, rtol=2e-4, atol=2e-7), (s, k, np.abs(got - ref).max())
        # ---- the library's part 2: clip_grad_norm_ + Adam on the flat buffer
        gflat = _dev(np.concatenate([pol.params[k].grad.numpy().ravel() for k in names]))
        _lib.check(L.icrl_clip_adam_step(_lib.ptr(flat), _lib.ptr(gflat), _lib.ptr(m), _lib.ptr(v), _lib.ptr(step), n, ctypes.byref(hp), _lib.ptr(work),
                                         _lib.ptr(out2), st), "icrl_clip_adam_step")
        assert abs(out2[0].item() - float(g[f"s{s}/grad_norm"])) <= 1e-5 * max(1.0, float(g[f"s{s}/grad_norm"]))
        new = flat.cpu().numpy()
        off = 0
        with torch.no_grad():
            for k, sz in zip(names, sizes):
                got = new[off:off + sz].reshape(pol.params[k].shape)
                ref = g[f"s{s}/after/{k}"]
                assert np.allclose(got, ref, rtol=1e-5, atol=3e-7), (s, k, np.abs(got - ref).max())
                pol.params[k].copy_(torch.as_tensor(got))
                off += sz
    assert int(step.item()) == 3


def test_minibatch_gather_and_adv_stats():
    """buffers.py:53-65,594-627: flat env-major indices -> rows of the [T, N] buffer; ppo_lag.py:219-222 statistics."""
    _gather_and_adv_stats(40, 7, 18, 6, 100)


def test_minibatch_gather_and_adv_stats_past_one_trip_of_the_block():
    """1000 rows out of a 40 x 32 buffer at 113 observations: adv_stats_kernel is one block of 256 threads, so every thread sums three rows and
    232 a fourth, in both of its passes (the mean, then the deviations); the gather runs 1000 blocks."""
    _gather_and_adv_stats(40, 32, 113, 8, 1000)


def _gather_and_adv_stats(T, N, od, ad, n):
    from icrl_amd import _lib, spaces
    from icrl_amd.buffers import RolloutBufferWithCost
    L = _lib.lib()
    rb = RolloutBufferWithCost(T, spaces.Box(-np.inf, np.inf, (od,), np.float64), spaces.Box(-1, 1, (ad,), np.float32), "cuda", n_envs=N)
    rng = np.random.RandomState(1)
    ref = {}
    for k in ("observations", "actions", "log_probs", "reward_advantages", "cost_advantages", "reward_returns", "cost_returns", "reward_values", "cost_values"):
        a = rng.randn(*getattr(rb, k).shape).astype(np.float32)
        getattr(rb, k).copy_(torch.as_tensor(a))
        ref[k] = o_ppo.env_major(a.reshape(T, N, -1))
    idx = rng.permutation(T * N)[:n].astype(np.int32)
    outs = dict(obs=torch.empty(n, od, device="cuda"), act=torch.empty(n, ad, device="cuda"))
    for k in ("lp", "ar", "ac", "rr", "rc", "vr", "vc"):
        outs[k] = torch.empty(n, device="cuda")
    assert len(set(idx.tolist())) == n and n > 1
    s = rb.struct()
    d_idx = _dev(idx, torch.int32)
    _lib.check(L.icrl_minibatch_gather(ctypes.byref(s), _lib.ptr(d_idx), n, *[_lib.ptr(outs[k]) for k in ("obs", "act", "lp", "ar", "ac", "rr", "rc", "vr", "vc")],
                                       _lib.current_stream()), "icrl_minibatch_gather")
    pairs = dict(obs="observations", act="actions", lp="log_probs", ar="reward_advantages", ac="cost_advantages", rr="reward_returns", rc="cost_returns",
                 vr="reward_values", vc="cost_values")
    for k, name in pairs.items():
        assert np.array_equal(outs[k].cpu().numpy().reshape(n, -1), ref[name][idx].reshape(n, -1)), k
    out4 = torch.zeros(4, device="cuda")
    _lib.check(L.icrl_adv_stats(_lib.ptr(outs["ar"]), _lib.ptr(outs["ac"]), n, _lib.ptr(out4), _lib.current_stream()), "icrl_adv_stats")
    ar, ac = torch.as_tensor(ref["reward_advantages"][idx].ravel()), torch.as_tensor(ref["cost_advantages"][idx].ravel())
    exp = [ar.mean().item(), 1.0 / (ar.std().item() + 1e-8), ac.mean().item(), ar.std().item()]
    assert np.allclose(out4.cpu().numpy(), exp, rtol=2e-6, atol=1e-7)


@pytest.mark.parametrize("case", "abcd")
def test_dual_step_follows_the_reference_trajectories(golden, case):
    """dual_variable.py:9-57 on the device against the reference's own nu trajectories (tests/golden/g5: 200 costs each, incl. the
    clamp-floor case); float32 arithmetic with libm's expf / log1pf instead of torch's: 2e-6 relative."""
    from icrl_amd import _lib
    from icrl_amd.dual_variable import DualVariable, _inv_softplus_floor
    L = _lib.lib()
    g = _sub(golden("g5_dual"), case + "/")
    nu0, lr, budget = (float(x) for x in g["params"])
    host = DualVariable(budget, lr, nu0, None)
    state = _dev(np.float32([host.log_nu, 0, 0, host.nu().item()]))
    t = torch.zeros(1, dtype=torch.int32, device="cuda")
    loss = torch.zeros(1, device="cuda")
    clamp = float(np.float32(_inv_softplus_floor(host.clamp_at)))
    traj = []
    for c in g["costs"]:
        _lib.check(L.icrl_dual_step(_lib.ptr(state), _lib.ptr(t), None, float(c), budget, lr, clamp, _lib.ptr(loss), _lib.current_stream()), "icrl_dual_step")
        traj.append(torch.cat([state[3:4], loss, state[0:1]]).clone())
    got = torch.stack(traj).cpu().numpy()
    assert int(t.item()) == len(g["costs"])
    assert np.allclose(got[:, 0], g["traj"][:, 0], rtol=2e-6, atol=1e-7), np.abs(got[:, 0] - g["traj"][:, 0]).max()      # nu
    assert np.allclose(got[:, 2], g["traj"][:, 2], rtol=2e-6, atol=2e-7)                                                   # log_nu
    assert np.allclose(got[:, 1], g["traj"][:, 1], rtol=2e-5, atol=1e-7)                                                   # loss = -nu (cost - budget)


_PLANES = dict(obs="observations", orig_obs="orig_observations", new_obs="new_observations", new_orig_obs="new_orig_observations", action="actions",
               reward="rewards", cost="costs", orig_cost="orig_costs", done="dones", reward_value="reward_values", cost_value="cost_values", log_prob="log_probs")


def test_buffer_add_writes_row_t():
    """buffers.py:554-592: one step's arrays -> row t of every plane (float64 observations / rewards stored as float32)."""
    _buffer_add(6, 5, 18, 6, 3)


def test_buffer_add_over_several_blocks_first_and_last_row():
    """64 envs x 113 observations = 7232 threads, 29 blocks of 256 (the existing case is one block of 90): `blockIdx.x * 256 + threadIdx.x`
    against the three extents N x obs (the last block ragged), N x act = 512 (two blocks) and N = 64; row 0, then the last row of the
    buffer (t x N x obs at its largest), each with its own values, the other rows untouched."""
    assert -(-64 * 113 // 256) == 29
    rb = _buffer_add(4, 64, 113, 8, 0)
    _buffer_add(4, 64, 113, 8, 3, rb=rb, written=(0,), seed=5)


def _buffer_add(T, N, od, ad, t, rb=None, written=(), seed=2):
    from icrl_amd import _lib, spaces
    from icrl_amd.buffers import RolloutBufferWithCost
    L = _lib.lib()
    if rb is None:
        rb = RolloutBufferWithCost(T, spaces.Box(-np.inf, np.inf, (od,), np.float64), spaces.Box(-1, 1, (ad,), np.float32), "cuda", n_envs=N)
    before = {name: getattr(rb, name).cpu().numpy().copy() for name in _PLANES.values()}
    rng = np.random.RandomState(seed)
    host = dict(obs=rng.randn(N, od), orig_obs=rng.randn(N, od), new_obs=rng.randn(N, od), new_orig_obs=rng.randn(N, od), action=rng.randn(N, ad).astype(np.float32),
                reward=rng.randn(N), cost=rng.rand(N), orig_cost=rng.rand(N).astype(np.float32), done=(rng.rand(N) < 0.5).astype(np.uint8),
                reward_value=rng.randn(N).astype(np.float32), cost_value=rng.randn(N).astype(np.float32), log_prob=rng.randn(N).astype(np.float32))
    dev = {k: torch.as_tensor(v).cuda().contiguous() for k, v in host.items()}
    s = rb.struct()
    order = ("obs", "orig_obs", "new_obs", "new_orig_obs", "action", "reward", "cost", "orig_cost", "done", "reward_value", "cost_value", "log_prob")
    _lib.check(L.icrl_buffer_add(ctypes.byref(s), t, *[_lib.ptr(dev[k]) for k in order], _lib.current_stream()), "icrl_buffer_add")
    for k, name in _PLANES.items():
        got = getattr(rb, name).cpu().numpy()
        assert np.array_equal(got[t].reshape(N, -1), host[k].astype(np.float32).reshape(N, -1)), k
        for r in range(T):          # only row t was touched: the rows written before keep their values, all others are still zero
            if r != t:
                assert np.array_equal(got[r], before[name][r]) and (r in written or not got[r].any()), (k, r)
    assert L.icrl_buffer_add(ctypes.byref(s), T, *[_lib.ptr(dev[k]) for k in order], _lib.current_stream()) == 1       # refused: t outside the buffer
    L.icrl_clear_error()
    return rb


@pytest.mark.parametrize("per_step", [False, True])
def test_is_weights_vs_oracle(per_step):
    """constraint_net.py:231-256 against the oracle restatement (pinned to the reference by g6): ragged episodes."""
    from icrl_amd import _lib
    from oracle import cn as o_cn
    L = _lib.lib()
    rng = np.random.RandomState(3)
    lengths = [7, 40, 1, 23, 64, 12, 33]
    N = sum(lengths)
    old = torch.as_tensor(rng.uniform(0.2, 0.9, (N, 1)).astype(np.float32))
    new = (old + torch.as_tensor(rng.uniform(-0.02, 0.02, (N, 1)).astype(np.float32))).clamp(0.01, 0.99)
    w_ref, kl_on, kl_no = o_cn.is_weights_and_kls(old.clone(), new.clone(), lengths, 1e-5, per_step)
    offs = torch.as_tensor(np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)).cuda()
    d_old, d_new = old.flatten().cuda().contiguous(), new.flatten().cuda().contiguous()
    w, prod, out4 = torch.zeros(N, device="cuda"), torch.zeros(len(lengths), device="cuda"), torch.zeros(4, device="cuda")
    _lib.check(L.icrl_is_weights(_lib.ptr(d_old), _lib.ptr(d_new), N, _lib.ptr(offs), len(lengths), 1e-5, int(per_step), _lib.ptr(w), _lib.ptr(prod), _lib.ptr(out4),
                                 _lib.current_stream()), "icrl_is_weights")
    assert np.allclose(w.cpu().numpy(), w_ref.numpy().ravel(), rtol=2e-5, atol=1e-7)
    o = out4.cpu().numpy()
    assert abs(o[0] - kl_on.item()) <= 2e-5 * max(1.0, abs(kl_on.item())) and abs(o[1] - kl_no.item()) <= 2e-5 * max(1.0, abs(kl_no.item())) + 1e-6


@pytest.mark.parametrize("per_step", [False, True])
def test_is_weights_past_the_first_trip_of_every_walk_vs_float64_oracle(per_step):
    """20 episodes on the kernel's 16 waves (waves 0..3 take a second episode), episodes of up to 1000 steps on a wave's 64 lanes (65 and 129
    steps: one live lane in the last trip; 64, 128, 640: whole trips), N = 6489 rows on 1024 threads (a ragged seventh trip), in the products,
    the ratio sum and the weight stores.  Reference: oracle.cn.is_weights_and_kls in float64 on the float32 inputs; bound per quantity
    4 x max |oracle32 - oracle64| + 1e-12 (helpers/fine_cases.py; measured there: weights 1.0e-6 of up to 2.2 per episode, 2.3e-7 of up to
    1.1 per step, kl_old_new 4.4e-8, kl_new_old 1.1e-7), printed beside the distance.  A numpy emulation of the kernel's lane-strided float32
    product order lands 1.9e-6 from the float64 weights."""
    from icrl_amd import _lib
    L = _lib.lib()
    lengths = list(F.IS_LENGTHS)
    N, n_ep = sum(lengths), len(lengths)
    assert n_ep == 20 and N == 6489 and max(lengths) == 1000
    old, new = F.is_weights_inputs()
    r64, r32, bounds = F.is_weights_oracles(per_step)
    assert 0.1 < r64["prod"].min() and r64["prod"].max() < 2.0, (r64["prod"].min(), r64["prod"].max())      # nothing overflows or vanishes
    offs = torch.as_tensor(np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)).cuda()
    d_old, d_new = old.flatten().cuda().contiguous(), new.flatten().cuda().contiguous()
    w, prod, out4 = torch.full((N + 64,), 7.0, device="cuda"), torch.full((n_ep + 16,), 7.0, device="cuda"), torch.zeros(4, device="cuda")
    _lib.check(L.icrl_is_weights(_lib.ptr(d_old), _lib.ptr(d_new), N, _lib.ptr(offs), n_ep, F.IS_EPS, int(per_step), _lib.ptr(w), _lib.ptr(prod), _lib.ptr(out4),
                                 _lib.current_stream()), "icrl_is_weights")
    w, prod, o = w.cpu().numpy(), prod.cpu().numpy(), out4.cpu().numpy()
    assert np.all(w[N:] == 7.0) and np.all(prod[n_ep:] == 7.0)      # nothing written past the rows / the episodes
    dist = dict(w=float(np.abs(w[:N].astype(np.float64) - r64["w"]).max()), kl_on=abs(float(o[0]) - r64["kl_on"]), kl_no=abs(float(o[1]) - r64["kl_no"]))
    for k in ("w", "kl_on", "kl_no"):
        print(f"FINE_IS per_step={per_step} {k}: |kernel - float64| = {dist[k]:.3g}, bound {bounds[k]:.3g}, ratio {dist[k] / bounds[k]:.2f}")
    for k in ("w", "kl_on", "kl_no"):
        assert dist[k] <= bounds[k], (k, dist[k], bounds[k])


@pytest.mark.parametrize("mode,weights", [(0, True), (0, False), (2, True), (1, False)])
def test_cn_loss_fwd_bwd_vs_autograd(mode, weights):
    """constraint_net.py:188-202 (and gail_utils.py's BCE) on the network's outputs: loss terms and d loss / d prediction against torch
    autograd of the oracle's expressions.  mode 2: the per-step broadcast quirk (nominal_loss = mean(w) * mean(log zeta))."""
    _cn_loss_fwd_bwd(mode, weights, 300, 170)


@pytest.mark.parametrize("mode,weights", [(0, True), (0, False), (2, True), (1, False)])
def test_cn_loss_fwd_bwd_vs_autograd_past_one_trip_of_the_block(mode, weights):
    """Bn = 1000, Be = 700 on cn_loss_fwd_bwd_kernel's one block of 256 threads: every thread takes three nominal and two expert rows, 232
    a fourth nominal and 188 a third expert one, in the sums and in the gradient stores (at Bn 300 / Be 170 only 44 threads took a second
    nominal row, none a second expert row)."""
    _cn_loss_fwd_bwd(mode, weights, 1000, 700)


def _cn_loss_fwd_bwd(mode, weights, Bn, Be):
    from icrl_amd import _lib
    from oracle import cn as o_cn
    L = _lib.lib()
    rng = np.random.RandomState(4)
    reg, eps = 0.5, 1e-5
    nom = torch.as_tensor(rng.uniform(0.05, 0.95, (Bn, 1)).astype(np.float32)).requires_grad_(True)
    exp = torch.as_tensor(rng.uniform(0.05, 0.95, (Be, 1)).astype(np.float32)).requires_grad_(True)
    w = torch.as_tensor(rng.uniform(0.5, 1.5, Bn).astype(np.float32)) if weights else torch.ones(Bn)

    class _Net:                       # the oracle's cn_loss evaluates net.forward(batch): hand it the leaf predictions
        def forward(self, x):
            return x
    is_batch = w[..., None, None] if mode == 2 else w[..., None]
    loss, e_l, n_l, r_l, _, _ = o_cn.cn_loss(_Net(), nom, exp, is_batch, reg, eps, gail=bool(mode & 1), factored=(mode == 2))
    loss.backward()
    d_nom, d_exp, terms = torch.zeros(Bn, device="cuda"), torch.zeros(Be, device="cuda"), torch.zeros(6, device="cuda")
    assert nom.grad.abs().min() > 0 and exp.grad.abs().min() > 0      # (a row the kernel left at its zero fill would differ from the reference)
    dn, de = nom.detach().flatten().cuda().contiguous(), exp.detach().flatten().cuda().contiguous()
    dw = w.cuda().contiguous() if weights else None
    _lib.check(L.icrl_cn_loss_fwd_bwd(_lib.ptr(dn), _lib.ptr(de), _lib.ptr(dw), Bn, Be, reg, eps, mode, _lib.ptr(terms), _lib.ptr(d_nom), _lib.ptr(d_exp),
                                      _lib.current_stream()), "icrl_cn_loss_fwd_bwd")
    t = terms.cpu().numpy()
    for got, ref in zip(t[:4], (loss.item(), e_l.item(), n_l.item(), float(r_l))):
        assert abs(got - ref) <= 2e-6 + 2e-5 * abs(ref), (t, loss.item(), e_l.item(), n_l.item(), float(r_l))
    assert np.allclose(d_nom.cpu().numpy(), nom.grad.numpy().ravel(), rtol=2e-5, atol=1e-8)
    assert np.allclose(d_exp.cpu().numpy(), exp.grad.numpy().ravel(), rtol=2e-5, atol=1e-8)


@pytest.mark.parametrize("n", [1, 7, 2048 * 64, 2048 * 512 + 3])
def test_explained_variance_vs_the_reference_formula(n):
    """icrl_explained_variance against common/utils.py:43-59 (oracle.loop.explained_variance) in the reference's argument order
    (ppo_lag.py:311-312: y_pred = returns, y_true = values), one and two pairs, and the NaN of a constant y_true."""
    from icrl_amd import _lib
    from oracle.loop import explained_variance
    L = _lib.lib()
    rng = np.random.RandomState(n)
    ret_r, val_r = (3 + 2 * rng.randn(n)).astype(np.float32), (3 + 2 * rng.randn(n)).astype(np.float32)
    val_c = (0.3 * rng.randn(n) + 1).astype(np.float32)
    ret_c = (val_c + 0.1 * rng.randn(n)).astype(np.float32)
    d = [_dev(x) for x in (ret_r, val_r, ret_c, val_c)]
    work, out = torch.zeros(8 * 256, dtype=torch.float64, device="cuda"), torch.full((2,), 7.0, device="cuda")
    _lib.check(L.icrl_explained_variance(_lib.ptr(d[0]), _lib.ptr(d[1]), _lib.ptr(d[2]), _lib.ptr(d[3]), n, _lib.ptr(work), _lib.ptr(out),
                                         _lib.current_stream()), "icrl_explained_variance")
    got = out.cpu().numpy()
    for g_, (yp, yt) in zip(got, ((ret_r, val_r), (ret_c, val_c))):
        want = explained_variance(yp.astype(np.float64), yt.astype(np.float64))
        if n == 1:
            assert np.isnan(g_) and np.isnan(want)
        else:
            assert abs(g_ - want) <= 1e-6 * max(1.0, abs(want)), (g_, want)
            assert abs(g_ - explained_variance(yp, yt)) <= 1e-4 * max(1.0, abs(want))      # numpy's own float32 evaluation
    # one pair: out[1] untouched; a constant y_true: NaN
    out.fill_(7.0)
    const = torch.full((max(n, 2),), 1.5, device="cuda")
    _lib.check(L.icrl_explained_variance(_lib.ptr(d[0]) if n > 1 else _lib.ptr(const), _lib.ptr(const), None, None, max(n, 2) if n == 1 else n,
                                         _lib.ptr(work), _lib.ptr(out), _lib.current_stream()), "icrl_explained_variance") if n <= 7 else None
    if n <= 7:
        got = out.cpu().numpy()
        assert np.isnan(got[0]) and got[1] == 7.0


# ---------------------------------------------------------------------------------------------------------------------
# explained variance where the critic is NEARLY CONSTANT (LapGridWorld, early training): y_true = base + a few float32 ulps.  The reference
# (np.var) subtracts the mean first.  Single-pass float64 sums of y and y^2 (Var = E[y^2] - E[y]^2, the single-pass form this kernel replaced)
# cancel there: emulated in numpy in the kernel's summation order (thread-strided partial sums, a 256-leaf tree per block, a tree over the
# blocks) that form gives -3.28e8 against -2.87e8 at 1000 + {0, 1} ulp x 300, -7.46e13 against -6.99e13 at 1 + {0, 1} ulp x 4096, -6.6e17
# instead of NaN for a constant float32(0.05) x 300, and reaches NaN for a constant 1000 only because its variance comes out at -1.2e-10:
# it fails the cases below.  The reference of these tests is the mean-first float64 evaluation on the float32 inputs cast to float64
# (numpy's own float32 evaluation is itself ill-conditioned here and is not used); the bound is the existing 1e-6 max(1, |want|): the
# output is one float32 (6e-8 relative) and a mean-first float64 evaluation is exact far below that.
# ---------------------------------------------------------------------------------------------------------------------
def _ev_launch(pairs, n):
    """icrl_explained_variance on one or two (y_pred, y_true) pairs of float32 arrays -> out2 on the host (7.0 where not written)."""
    from icrl_amd import _lib
    d = [_dev(x) for pair in pairs for x in pair] + [None, None] * (2 - len(pairs))
    work, out = torch.zeros(8 * 256, dtype=torch.float64, device="cuda"), torch.full((2,), 7.0, device="cuda")
    _lib.check(_lib.lib().icrl_explained_variance(*(_lib.ptr(x) for x in d), n, _lib.ptr(work), _lib.ptr(out), _lib.current_stream()),
               "icrl_explained_variance")
    return out.cpu().numpy()


def _ev_want(y_pred, y_true):
    from oracle.loop import explained_variance
    yt = y_true.astype(np.float64)
    assert np.var(yt) > 0, "the case must have a varying y_true in float64"
    return explained_variance(y_pred.astype(np.float64), yt)


def _near_constant(rng, base, k, n):
    b = np.float32(base)
    return (b + np.spacing(b) * rng.randint(0, k + 1, n).astype(np.float32)).astype(np.float32)


@pytest.mark.parametrize("n", [300, 4096, 2048 * 64])
@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("base", [0.05, 1.0, 100.0, 1000.0])
def test_explained_variance_of_a_nearly_constant_critic(base, k, n):
    """pair a: the denominator's variance is the ill-conditioned one (y_pred = base + 0.5 randn); pair b: the numerator's too
    (y_pred = y_true + 1000 + 0.01 randn: y_true - y_pred is -1000 with a spread of 0.01)."""
    rng = np.random.RandomState(int(base * 100) + 7 * k + n)
    yt_a, yt_b = _near_constant(rng, base, k, n), _near_constant(rng, base, k, n)
    yp_a = (np.float32(base) + 0.5 * rng.randn(n)).astype(np.float32)
    yp_b = (yt_b + 1000 + 0.01 * rng.randn(n)).astype(np.float32)
    want = [_ev_want(yp_a, yt_a), _ev_want(yp_b, yt_b)]
    got = _ev_launch([(yp_a, yt_a), (yp_b, yt_b)], n)
    print(f"explained variance base {base} k {k} n {n}: got {got.tolist()} want {want}")
    for g_, w_ in zip(got, want):
        assert abs(g_ - w_) <= 1e-6 * max(1.0, abs(w_)), (g_, w_)


def test_explained_variance_does_not_lean_on_its_first_element():
    """y_true[0] = 0, the rest 1000 + {0, 1} ulp: a first-element pivot would be no better than no pivot."""
    n = 4096
    rng = np.random.RandomState(11)
    yt_a, yt_b = _near_constant(rng, 1000.0, 1, n), _near_constant(rng, 1000.0, 1, n)
    yt_a[0] = yt_b[0] = 0.0
    yp_a = (np.float32(1000.0) + 0.5 * rng.randn(n)).astype(np.float32)
    yp_b = (yt_b + 1000 + 0.01 * rng.randn(n)).astype(np.float32)
    want = [_ev_want(yp_a, yt_a), _ev_want(yp_b, yt_b)]
    got = _ev_launch([(yp_a, yt_a), (yp_b, yt_b)], n)
    print(f"explained variance, first element 0: got {got.tolist()} want {want}")
    for g_, w_ in zip(got, want):
        assert abs(g_ - w_) <= 1e-6 * max(1.0, abs(w_)), (g_, w_)


@pytest.mark.parametrize("value,n", [(0.05, 300), (0.1, 2048 * 64 + 3), (1000.0, 300)])
def test_explained_variance_of_a_constant_critic_is_nan(value, n):
    """np.var of a constant array is exactly 0 (its mean is the constant), so the reference returns NaN — for every constant, not only those whose
    squares happen to cancel."""
    from oracle.loop import explained_variance
    rng = np.random.RandomState(n)
    yt = np.full(n, value, np.float32)
    yp_a, yp_b = (value + rng.randn(n)).astype(np.float32), yt.copy()
    assert np.isnan(explained_variance(yp_a.astype(np.float64), yt.astype(np.float64)))
    got = _ev_launch([(yp_a, yt), (yp_b, yt)], n)
    print(f"explained variance of constant {value} x {n}: got {got.tolist()}")
    assert np.isnan(got[0]) and np.isnan(got[1]), got
    got = _ev_launch([(yp_a, yt)], n)
    assert np.isnan(got[0]) and got[1] == 7.0, got


_hparam_batch, _loss_and_row_grads = F.hparam_batch, F.loss_and_row_grads
# Per-row output gradients: max |float32 oracle - float64 oracle| per row count n, measured on the CPU (helpers/fine_cases.py holds the table
# and the command that prints it).  n = 64 and 100 share the entry measured over their four cases: d_lp 3.5e-9 (of values up to 0.025), d_vr
# 3.4e-9 (of 0.091), d_vc 5.5e-10 (of 0.0087), d_en 3.5e-12 (of 1.6e-4: float32(ent_coef) / n).  n = 300: d_lp 1.18e-9 (of 0.0069), d_vr 1.15e-9
# (of 0.017), d_vc 2.48e-10 (of 0.0017), d_en 3.71e-13 (of 3.3e-5).  n = 1000: d_lp 4.76e-10 (of 0.0025), d_vr 5.86e-10 (of 0.0069), d_vc 8.02e-11
# (of 5.7e-4), d_en 2.53e-13 (of 1e-5).
# The bound is 3 x that: the kernel's reductions (advantage mean and standard deviation) run in another order than torch's.
ROW_GRAD_F32_DEV = F.ROW_GRAD_F32_DEV


@pytest.mark.parametrize("n", [64, 100, 300, 1000])
@pytest.mark.parametrize("hset", ["A", "B"])
def test_loss_fwd_bwd_with_value_clipping_vs_float64_autograd(hset, n):
    """icrl_ppo_lag_loss_fwd_bwd with both old-value pointers set (value clipping on for both critics), the entropy bonus, separate critic
    weights; then icrl_clip_adam_step in the branch of the norm clip the set takes (A: max_grad_norm 0.3 below the norm, B: 50 above it)
    — against float64 autograd of oracle.ppo.minibatch_loss on the same outputs and the explicit clip / Adam formulas.
    n = 300, 1000: past the first trip of loss_fwd_bwd_kernel's one block of 256 threads (44 threads take a second row; every thread three
    and 232 a fourth), where the seven per-thread sums carry over."""
    from helpers import ppo_hparam_cases as H
    from icrl_amd import _lib, structs as S
    L = _lib.lib()
    hpd, nu_f = H.hparams(hset), 0.731
    b = _hparam_batch(n)
    ref_terms, ref_g, margins, shares = _loss_and_row_grads(b, hpd, nu_f, torch.float64)
    # ---- conditions on the inputs, before the kernel
    assert margins[0] >= H.RATIO_MARGIN and margins[1] >= H.VALUE_MARGIN and margins[2] >= H.VALUE_MARGIN, margins
    assert H.CLIP_FRACTION[0] <= shares[0] <= H.CLIP_FRACTION[1] and all(H.VCLIP_SHARE[0] <= s <= H.VCLIP_SHARE[1] for s in shares[1:]), shares
    hp = S.PpoHyperT(n, 1, 0, 0)
    hp.clip_range, hp.ent_coef, hp.reward_vf_coef, hp.cost_vf_coef, hp.max_grad_norm = 0.2, hpd["ent_coef"], hpd["reward_vf_coef"], hpd["cost_vf_coef"], hpd["max_grad_norm"]
    hp.clip_range_reward_vf, hp.clip_range_cost_vf = hpd["clip_range_reward_vf"], hpd["clip_range_cost_vf"]
    hp.lr, hp.adam_beta1, hp.adam_beta2, hp.adam_eps = 3e-4, 0.9, 0.999, 1e-5
    dev = {k: _dev(v) for k, v in b.items()}
    nu, terms = _dev(np.float32([nu_f])), torch.zeros(8, device="cuda")
    got = {k: torch.full((n,), 7.0, device="cuda") for k in ("d_lp", "d_vr", "d_vc", "d_en")}
    st = _lib.current_stream()
    _lib.check(L.icrl_ppo_lag_loss_fwd_bwd(*[_lib.ptr(dev[k]) for k in ("lp", "old_lp", "adv_r", "adv_c", "v_r", "v_c", "ret_r", "ret_c", "old_v_r", "old_v_c", "ent")],
                                           _lib.ptr(nu), ctypes.byref(hp), n, _lib.ptr(terms), *[_lib.ptr(got[k]) for k in ("d_lp", "d_vr", "d_vc", "d_en")], st),
               "icrl_ppo_lag_loss_fwd_bwd")
    t = terms.cpu().numpy()
    for i, key in enumerate(("loss", "policy_loss", "rvl", "cvl", "entropy_loss", "approx_kl", "clip_fraction")):
        print(f"FINE_HP set {hset} n={n} {key}: {t[i]:.9g} vs {ref_terms[i]:.9g}")
    for k in got:
        print(f"FINE_HP set {hset} n={n} {k}: max |kernel - float64| = {np.abs(got[k].cpu().numpy() - ref_g[k]).max():.3g} (bound {3 * ROW_GRAD_F32_DEV[n][k]:.3g})")
    for i, key in enumerate(("loss", "policy_loss", "rvl", "cvl", "entropy_loss", "approx_kl", "clip_fraction")):
        assert abs(t[i] - ref_terms[i]) <= 2e-6 + 2e-5 * abs(ref_terms[i]), (key, t[i], ref_terms[i])
    for k in got:      # row by row
        assert np.abs(got[k].cpu().numpy() - ref_g[k]).max() <= 3 * ROW_GRAD_F32_DEV[n][k], (k, np.abs(got[k].cpu().numpy() - ref_g[k]).max())
    # ---- clip_grad_norm_ + Adam, two steps on a flat buffer of 20 blocks with a ragged tail
    _clip_adam_steps(hset, hpd, hp, 5001, n)


def _clip_adam_steps(hset, hpd, hp, n_p, seed, preset=False):
    """two icrl_clip_adam_step calls on a flat buffer of n_p parameters against clip_coef_explicit / adam_step_explicit in float64.
    preset: then a third call with the step counter set to 999 and the moments as they stand (non-zero), against the same formulas at t = 1000."""
    from icrl_amd import _lib
    L, st = _lib.lib(), _lib.current_stream()
    rng = np.random.RandomState(seed)
    p0, grads = rng.randn(n_p).astype(np.float32), [(rng.randn(n_p) / np.sqrt(n_p) * s).astype(np.float32) for s in (1.0, 2.5)]      # norms ~ 1 and ~ 2.5
    if preset:
        grads.append((rng.randn(n_p) / np.sqrt(n_p) * 1.7).astype(np.float32))
    flat, m, v = _dev(np.concatenate([p0, np.full(300, 7.0, np.float32)])), torch.zeros(n_p + 300, device="cuda"), torch.zeros(n_p + 300, device="cuda")
    m[n_p:], v[n_p:] = 7.0, 7.0                                                                   # sentinels behind the n_p entries of all three
    step, work, out2 = torch.zeros(1, dtype=torch.int32, device="cuda"), torch.zeros(256, device="cuda"), torch.zeros(2, device="cuda")
    rp, rm, rv, qm, qv = (torch.as_tensor(x, dtype=torch.float64) for x in (p0, np.zeros(n_p), np.zeros(n_p), np.zeros(n_p), np.zeros(n_p)))
    w1 = np.float32(1.0 - float(np.float32(0.9)))
    t = 0
    for s, g in enumerate(grads):
        if s == 2:      # the step counter far from its start: bias corrections 1 - 0.9^1000 = 1 and 1 - 0.999^1000 = 0.632 (at t = 1..3: 0.1 .. 0.27, 0.001 .. 0.003)
            step.fill_(999)
            t = 999
            rm, rv = m[:n_p].cpu().double(), v[:n_p].cpu().double()      # the reference continues from the moments the call reads
            qm, qv = rm.clone(), rv.clone()
            rp = flat[:n_p].cpu().double()
            assert float(rm.abs().max()) > 0 and float(rv.max()) > 0
        t += 1
        total, coef = o_ppo.clip_coef_explicit([torch.as_tensor(g)], hpd["max_grad_norm"])
        assert (coef < 1.0) == (hset == "A") and abs(total - hpd["max_grad_norm"]) > 0.1      # the branch the set is about, away from its kink
        gd = _dev(g)
        _lib.check(L.icrl_clip_adam_step(_lib.ptr(flat), _lib.ptr(gd), _lib.ptr(m), _lib.ptr(v), _lib.ptr(step), n_p, ctypes.byref(hp), _lib.ptr(work),
                                         _lib.ptr(out2), st), "icrl_clip_adam_step")
        o = out2.cpu().numpy()
        assert abs(o[0] - total) <= 1e-5 * max(1.0, total), (o, total)
        assert abs(o[1] - coef) <= 1e-5 * coef and (o[1] == 1.0) == (hset == "B"), (o, coef)
        assert all(bool((x[n_p:] == 7.0).all()) for x in (flat, m, v)), "a store behind the last parameter"
        got_p, got_m, got_v = (x[:n_p].cpu().numpy() for x in (flat, m, v))
        # what enters the moments is g x coef, rounded once.  After the first step exp_avg is (1 - beta1) x that, bit for bit: with the coefficient
        # capped at 1 (set B) the first moment is (1 - beta1) g itself, the gradient's direction and scale untouched
        gi = g * o[1]
        if s == 0:
            assert np.array_equal(got_m, w1 * gi)
            assert np.array_equal(got_m, w1 * g) == (hset == "B")
        gc = torch.as_tensor(g, dtype=torch.float64) * coef
        rp, rm, rv = o_ppo.adam_step_explicit(rp, gc, rm, rv, t, 3e-4, eps=1e-5)
        print(f"FINE_ADAM set {hset} n_p={n_p} t={t}: max |kernel - float64| of the parameters = {np.abs(got_p - rp.numpy()).max():.3g} (atol 3e-7, rtol 1e-5)")
        assert np.allclose(got_p, rp.numpy(), rtol=1e-5, atol=3e-7), np.abs(got_p - rp.numpy()).max()
        # the moments: the explicit formula with the betas as icrl_ppo_hyper_t carries them (float32: 1 - float32(0.999) is smaller than 0.001 by 1.3e-5 of it,
        # which the parameter tolerance above and ADAM_DEV_BOUND absorb)
        b1, b2 = float(np.float32(0.9)), float(np.float32(0.999))
        qm, qv = b1 * qm + (1 - b1) * gc, b2 * qv + (1 - b2) * gc * gc
        assert np.allclose(got_m, qm.numpy(), rtol=1e-5, atol=1e-9) and np.allclose(got_v, qv.numpy(), rtol=1e-5, atol=1e-12)
        assert int(step.item()) == t
    assert int(step.item()) == (1000 if preset else 2)


@pytest.mark.parametrize("hset", ["A", "B"])
def test_clip_adam_step_past_one_grid_pass_and_at_step_1000(hset):
    """70 001 parameters: icrl_clip_adam_step caps its grid at 256 blocks of 256 threads (65 536 per pass), so every thread of sqnorm_partials_kernel
    and clip_adam_kernel takes a second element and 4465 do not (the ragged end), and clip_adam_kernel folds 256 partial sums, one per thread.
    The same two-step check as at 5001 parameters, the gradients scaled to norms ~ 1 and ~ 2.5 (set A: max_grad_norm 0.3 below, B: 50 above),
    then a call with the step counter preset to 999 on the moments of those two steps."""
    from helpers import ppo_hparam_cases as H
    from icrl_amd import structs as S
    hpd = H.hparams(hset)
    hp = S.PpoHyperT(64, 1, 0, 0)
    hp.clip_range, hp.ent_coef, hp.reward_vf_coef, hp.cost_vf_coef, hp.max_grad_norm = 0.2, hpd["ent_coef"], hpd["reward_vf_coef"], hpd["cost_vf_coef"], hpd["max_grad_norm"]
    hp.clip_range_reward_vf, hp.clip_range_cost_vf = hpd["clip_range_reward_vf"], hpd["clip_range_cost_vf"]
    hp.lr, hp.adam_beta1, hp.adam_beta2, hp.adam_eps = 3e-4, 0.9, 0.999, 1e-5
    assert 256 * 256 < 70001 < 2 * 256 * 256
    _clip_adam_steps(hset, hpd, hp, 70001, 70001, preset=True)
