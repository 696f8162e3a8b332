"""CPU: discriminator costs (icrl_cost_disc_t / gail_utils.DiscriminatorCost, the cost of `cpg --load_gail`) — descriptor layout and
tag, the ABI that must not move, and the host-side refusals (argument checks that run before any HIP call: no GPU needed).  What needs
the device — the numpy form of DiscriminatorCost against the oracle included, since a discriminator's parameters live in device
memory from construction — is in tests/test_disc_cost_gpu.py."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = "discriminator cost descriptor (icrl_cost_disc_t"


def _lib():
    from icrl_amd import _lib as L
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return L


def _refused(err, L, text):
    assert err == 1
    msg = L.lib().icrl_last_error().decode()
    assert text in msg, msg
    L.lib().icrl_clear_error()


def _net(S, **kw):
    f = dict(obs_dim=18, acs_dim=6, in_dim=24, n_hidden=1, h1=20, h2=0, h3=0, h4=0, is_discrete=0, n_params=24 * 20 + 20 + 21, clip_obs=-1.0)
    f.update(kw)
    return S.CostNetT(**f)


def _desc(S, inner, **kw):
    f = dict(obs_dim=inner.obs_dim, acs_dim=inner.acs_dim, in_dim=inner.in_dim, n_hidden=S.COST_DISC, net=S.addr(inner))
    f.update(kw)
    return S.CostDiscT(**f)


def _rollout_args(S):
    return S.EnvT(4, 18, 6, 1000, 0, 0, 0, 0), S.NormT(1, 1, 1, 1), S.PolicyT(18, 6, 64, 64, 0, 1, None, None), S.BufferT(8, 4, 18, 6), S.AgentT()


def test_descriptor_layout_tag_and_the_abi_that_stays():
    from icrl_amd import structs as S
    assert ctypes.sizeof(S.CostDiscT) == 4 * 4 + 8 and S.CostDiscT.net.offset == 16
    for name in ("obs_dim", "acs_dim", "in_dim", "n_hidden"):
        assert getattr(S.CostDiscT, name).offset == getattr(S.CostNetT, name).offset == getattr(S.CostFnT, name).offset, name
    assert S.CostDiscT.n_hidden.offset == 12
    assert S.COST_DISC == -2 and S.COST_FN == -1
    assert ctypes.sizeof(S.CostNetT) == 112
    L = _lib()
    assert L.lib().icrl_abi_version() == 107 and L.PICK_DISC == 32
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "icrl_hip.h")).read(), flags=re.S)
    assert re.search(r"#define\s+ICRL_COST_DISC\s+\(-2\)", src) and re.search(r"#define\s+ICRL_PICK_DISC\s+32\b", src)
    assert re.search(r"const\s+icrl_costnet_t\s*\*\s*net\s*;\s*}\s*icrl_cost_disc_t\s*;", src)
    assert "icrl_abi_version(void) { return 107; }" in open(os.path.join(ROOT, "icrl_amd", "csrc", "gae.hip")).read()
    for v in (1, 2, 4, 8, 16):      # the pick bits that existed keep their values
        assert re.search(rf"#define\s+ICRL_PICK_\w+\s+{v}\b", src), v


def test_serving_entry_points_refuse_a_bad_descriptor_with_a_reason():
    """NULL inner net, an inner net that is itself a tagged descriptor, header fields that disagree with the inner net, and an inner net
    outside a constraint net's limits (bad_cn, as for a constraint net handed over directly)."""
    from icrl_amd import structs as S
    L = _lib()
    lib, b = L.lib(), ctypes.byref
    env, nm, pol, buf, ag = _rollout_args(S)
    hs = S.HostStepT(8, 0)
    good = _net(S)
    nested = _desc(S, good)
    cases = [(_desc(S, good, net=None), "with a NULL inner net"),
             (_desc(S, good, net=S.addr(nested)), "inner net is itself a tagged descriptor"),
             (_desc(S, good, in_dim=7), "says obs_dim 18, acs_dim 6, in_dim 7, its inner net 18, 6, 24")]
    for d, text in cases:
        for who, call in (("icrl_rollout_collect", lambda: lib.icrl_rollout_collect_ex(b(env), b(nm), b(pol), b(d), b(buf), b(ag), None, None, None, 0.99, 0.95, 0.99, 0.95, 1, None)),
                          ("icrl_rollout_collect", lambda: lib.icrl_rollout_collect(b(env), b(nm), b(pol), b(d), b(buf), b(ag), None, None, None, 0.99, 0.95, 0.99, 0.95, None)),
                          ("icrl_host_step", lambda: lib.icrl_host_step(b(nm), b(pol), b(d), b(buf), b(ag), b(hs), None, None, None, 0, None)),
                          ("icrl_cost_mlp_forward", lambda: lib.icrl_cost_mlp_forward(b(d), None, None, 4, None, None))):
            err = call()
            assert err == 1
            msg = lib.icrl_last_error().decode()
            assert NAMES in msg and text in msg and msg.startswith(who), msg
            lib.icrl_clear_error()
    # the inner net under a constraint net's own limits: in_dim 0 is no constraint net (cn_ok / bad_cn), behind the descriptor as without it
    bad = _net(S, in_dim=0)
    d = _desc(S, bad)
    for cn in (d, bad):
        _refused(lib.icrl_rollout_collect_ex(b(env), b(nm), b(pol), b(cn), b(buf), b(ag), None, None, None, 0.99, 0.95, 0.99, 0.95, 1, None), L,
                 "icrl_rollout_collect: constraint net in_dim 0")
        _refused(lib.icrl_host_step(b(nm), b(pol), b(cn), b(buf), b(ag), b(hs), None, None, None, 0, None), L, "icrl_host_step: constraint net in_dim 0")
    _refused(lib.icrl_cost_mlp_forward(b(d), None, None, 4, None, None), L, "cost forward: constraint net in_dim 0")
    _refused(lib.icrl_cost_mlp_forward(b(_desc(S, good)), None, None, 0, None, None), L, "N = 0 rows")


def test_entry_points_without_a_discriminator_form_refuse_the_descriptor():
    """seed batches (all three entry points), constraint-net training, the two prepare calls, icrl_disc_reward and the GAIL batch entry
    points: each names the descriptor and says where it is served."""
    from icrl_amd import structs as S
    L = _lib()
    lib, b = L.lib(), ctypes.byref
    text = NAMES + ", n_hidden == ICRL_COST_DISC) is not served here"
    env, nm, pol, buf, ag = _rollout_args(S)
    net = _net(S)
    d = _desc(S, net)
    job = S.RolloutJobT(S.addr(env), S.addr(nm), S.addr(pol), S.addr(d), S.addr(buf), S.addr(ag), None)
    scratch = (ctypes.c_char * 8192)()
    ws = ctypes.addressof(scratch)
    _refused(lib.icrl_rollout_collect_batch(1, b(job), None, None, 0.99, 0.95, 0.99, 0.95, 1, ws, 8192, None), L, text)
    _refused(lib.icrl_rollout_collect_batch_mon(1, b(job), None, None, None, 0.99, 0.95, 0.99, 0.95, 1, ws, 8192, None), L, text)
    _refused(lib.icrl_rollout_collect_batch_cost(1, b(job), None, None, None, 0.99, 0.95, 0.99, 0.95, 1, ws, 8192, None), L, text)
    msg_has = "batched rollout kernels have no discriminator form yet"
    lib.icrl_rollout_collect_batch(1, b(job), None, None, 0.99, 0.95, 0.99, 0.95, 1, ws, 8192, None)
    assert msg_has in lib.icrl_last_error().decode()
    lib.icrl_clear_error()
    hp = S.CnHyperT(2, 1, 0, 0)
    _refused(lib.icrl_cn_train(b(d), None, None, None, None, None, 64, 64, None, None, 2, b(hp), None, None, None), L, text)
    _refused(lib.icrl_cn_train_minibatch(b(d), None, None, None, None, None, 64, 64, None, None, 2, b(hp), None, 16, None, None, None), L, text)
    tj = S.CnTrainJobT(S.addr(d), None, None, None, None, None, 64, 64, None, None, 2, 0, S.addr(hp), None, None)
    _refused(lib.icrl_cn_train_batch(1, b(tj), ws, 8192, None), L, text)
    mj = S.CnTrainMbJobT(S.addr(d), None, None, None, None, None, 64, 64, None, None, 2, 0, S.addr(hp), None, None, None, 16, 0)
    _refused(lib.icrl_cn_train_minibatch_batch(1, b(mj), ws, 8192, None), L, text)
    _refused(lib.icrl_cn_prepare(b(d), None, None, 4, None, None), L, text)
    _refused(lib.icrl_costnet_prepare(b(d), None), L, text)
    _refused(lib.icrl_disc_reward(b(d), None, None, 4, None, 0, None), L, text)
    gj = S.GailJobT(S.addr(d), None, None, None, None, None, 0.0, None, None, None, 32, 0)
    _refused(lib.icrl_gail_unnormalize_batch(1, b(gj), ws, 8192, None), L, text)
    _refused(lib.icrl_gail_relabel_batch(1, b(gj), ws, 8192, None), L, text)


def _cfg(seed, extra=()):
    import types
    from icrl_amd.cpg import build_parser
    argv = ["cpg", "-tei", "HCWithPos-v0", "-eei", "HCWithPosTest-v0", "-nt", "8", "-ns", "64", "-t", "1024", "-ne", "2", "-s", str(seed), "-v", "0", *extra]
    cfg = vars(build_parser().parse_args(argv))
    cfg.update(rank=0, world_size=1, save_dir=None)
    return types.SimpleNamespace(**cfg)


def test_seed_batch_still_refuses_load_gail_and_says_why():
    """(the refusal comes before the batch builds anything on the device)"""
    _lib()
    from icrl_amd.seed_batch import CpgSeedBatch
    extra = ("--load_gail", "-cp", "unused.pt")
    with pytest.raises(ValueError, match="load_gail") as e:
        CpgSeedBatch([_cfg(0, extra), _cfg(1, extra)])
    assert "batched rollout kernels have no discriminator form yet" in str(e.value)


def test_the_switch_for_the_parent_path_is_read_beside_the_analytic_one_and_listed():
    ppo = open(os.path.join(ROOT, "icrl_amd", "ppo_lag.py")).read()
    assert "ICRL_DISC_COST_STEPPED" in ppo and "ICRL_ANALYTIC_COST_STEPPED" in ppo
    assert "ICRL_DISC_COST_STEPPED" in open(os.path.join(ROOT, "README.md")).read()
