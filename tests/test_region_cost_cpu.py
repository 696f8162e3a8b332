"""CPU: region costs (icrl_cost_region_t / true_constraint_net.RegionCost, the cost of `--cost_spec`) — descriptor layout and tag, the ABI
that must not move, every host-side refusal (argument checks that run before any HIP call: the descriptors' device pointers are the
address 1), the spec parser and its errors, the numpy form against the one-row-at-a-time evaluator of tests/helpers/region_cost_cases.py
bit for bit, and the six identities with the analytic kinds.  What needs the device is in tests/test_region_cost_gpu.py."""
import ctypes
import json
import math
import os
import re
import types

import numpy as np
import pytest

from helpers import region_cost_cases as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = "icrl_cost_region_t"


def _lib():
    from icrl_amd import _lib as L
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return L


def _refused(err, L, *texts):
    assert err == 1
    msg = L.lib().icrl_last_error().decode()
    for t in texts:
        assert t in msg, msg
    L.lib().icrl_clear_error()
    return msg


def _table(S, clauses):
    """clauses: [(type, negate, cols, a, b, c)]"""
    tab = (S.RegionClauseT * max(len(clauses), 1))()
    for q, (t, ng, cols, a, b, c) in zip(tab, clauses):
        q.type, q.negate, q.n_terms, q.c = t, ng, len(cols), c
        for k in range(min(len(cols), 8)):
            q.col[k], q.a[k], q.b[k] = cols[k], a[k], b[k]
    return tab


def _desc(S, tab=None, n=None, **kw):
    """a region descriptor whose device table is the address 1: a call that touched it would fault, a refusal comes first"""
    if tab is None:
        tab = _table(S, [(S.REGION_BOX, 0, [0], [-1.0], [1.0], 0.0)])
    f = dict(obs_dim=18, acs_dim=6, in_dim=0, n_hidden=S.COST_REGION, n_clauses=len(tab) if n is None else n, combine=S.REGION_ANY,
             clauses=ctypes.addressof(tab), d_clauses=1)
    f.update(kw)
    d = S.CostRegionT(**f)
    d._keep = tab
    return d


def _rollout_args(S, discrete=0, h1=64):
    return (S.EnvT(4, 18, 6, 1000, 0, 0, 0, 0), S.NormT(1, 1, 1, 1), S.PolicyT(18, 6, h1, 64, discrete, 1, None, None),
            S.BufferT(8, 4, 18, 1 if discrete else 6), S.AgentT())


# ---- 1. layout, tag, ABI --------------------------------------------------------------------------------------------------------------------
def test_descriptor_layout_tag_and_the_abi_that_stays():
    from icrl_amd import structs as S
    q = S.RegionClauseT
    assert ctypes.sizeof(q) == 16 + 32 + 64 + 64 + 8 == 184
    assert (q.type.offset, q.negate.offset, q.n_terms.offset, q.col.offset, q.a.offset, q.b.offset, q.c.offset) == (0, 4, 8, 16, 48, 112, 176)
    d = S.CostRegionT
    assert ctypes.sizeof(d) == 40 == ctypes.sizeof(S.CostFnT)      # (it travels in the analytic descriptor's bytes of the argument blocks)
    assert (d.n_clauses.offset, d.combine.offset, d.clauses.offset, d.d_clauses.offset) == (16, 20, 24, 32)
    for name in ("obs_dim", "acs_dim", "in_dim", "n_hidden"):
        assert getattr(d, name).offset == getattr(S.CostNetT, name).offset == getattr(S.CostFnT, name).offset, name
    assert (S.COST_REGION, S.COST_DISC, S.COST_FN) == (-3, -2, -1)
    assert (S.REGION_BOX, S.REGION_HALFSPACE, S.REGION_BALL, S.REGION_ANY, S.REGION_ALL, S.REGION_SUM) == (0, 1, 2, 0, 1, 2)
    assert S.REGION_MAX_CLAUSES == S.REGION_MAX_TERMS == 8
    assert ctypes.sizeof(S.CostNetT) == 112 and ctypes.sizeof(S.CostDiscT) == 24      # every existing struct keeps its size
    L = _lib()
    lib = L.lib()
    assert lib.icrl_abi_version() == 107 and L.PICK_REGION == 128
    assert hasattr(lib, "icrl_cost_region_rows") and hasattr(lib, "icrl_cost_mlp_forward")
    assert L.SIGNATURES["icrl_cost_region_rows"] == L.SIGNATURES["icrl_cost_fn_rows"]
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "icrl_hip.h")).read(), flags=re.S)
    assert re.search(r"#define\s+ICRL_COST_REGION\s+\(-3\)", src) and re.search(r"#define\s+ICRL_PICK_REGION\s+128\b", src)
    assert re.search(r"#define\s+ICRL_REGION_MAX_CLAUSES\s+8\b", src) and re.search(r"#define\s+ICRL_REGION_MAX_TERMS\s+8\b", src)
    assert re.search(r"#define\s+ICRL_PICK_MINW_SHIFT\s+8\b", src)
    assert re.search(r"int\s+icrl_cost_region_rows\(const\s+icrl_cost_region_t\s*\*", src)
    assert "icrl_abi_version(void) { return 107; }" in open(os.path.join(ROOT, "icrl_amd", "csrc", "gae.hip")).read()
    for v in (1, 2, 4, 8, 16, 32, 64):      # the pick bits that existed keep their values
        assert re.search(rf"#define\s+ICRL_PICK_\w+\s+{v}\b", src), v


# ---- 2. refusals ----------------------------------------------------------------------------------------------------------------------------
def test_entry_points_without_a_region_form_refuse_the_descriptor():
    """every *_batch* rollout, icrl_rollout_collect_sde, constraint-net training, the two prepare calls, icrl_disc_reward, the GAIL batch
    entry points: each names the descriptor, before any device call."""
    from icrl_amd import structs as S
    L = _lib()
    lib, b = L.lib(), ctypes.byref
    text = "a region cost descriptor (icrl_cost_region_t, n_hidden == ICRL_COST_REGION) is not served here"
    env, nm, pol, buf, ag = _rollout_args(S)
    d = _desc(S)
    job = S.RolloutJobT(S.addr(env), S.addr(nm), S.addr(pol), S.addr(d), S.addr(buf), S.addr(ag), None)
    scratch = (ctypes.c_char * 8192)()
    ws = ctypes.addressof(scratch)
    _refused(lib.icrl_rollout_collect_batch(1, b(job), None, None, 0.99, 0.95, 0.99, 0.95, 1, ws, 8192, None), L, text, "icrl_rollout_collect_batch:")
    _refused(lib.icrl_rollout_collect_batch_mon(1, b(job), None, None, None, 0.99, 0.95, 0.99, 0.95, 1, ws, 8192, None), L, text)
    _refused(lib.icrl_rollout_collect_batch_cost(1, b(job), None, None, None, 0.99, 0.95, 0.99, 0.95, 1, ws, 8192, None), L, text, "icrl_rollout_collect_batch_cost:")
    _refused(lib.icrl_rollout_collect_sde(b(env), b(nm), b(pol), b(d), b(buf), b(ag), 1, 1, -1, None, None, 0.99, 0.95, 0.99, 0.95, 1, None), L, text,
             "icrl_rollout_collect_sde:")
    hp = S.CnHyperT(2, 1, 0, 0)
    _refused(lib.icrl_cn_train(b(d), None, None, None, None, None, 64, 64, None, None, 2, b(hp), None, None, None), L, text)
    _refused(lib.icrl_cn_train_minibatch(b(d), None, None, None, None, None, 64, 64, None, None, 2, b(hp), None, 16, None, None, None), L, text)
    tj = S.CnTrainJobT(S.addr(d), None, None, None, None, None, 64, 64, None, None, 2, 0, S.addr(hp), None, None)
    _refused(lib.icrl_cn_train_batch(1, b(tj), ws, 8192, None), L, text)
    mj = S.CnTrainMbJobT(S.addr(d), None, None, None, None, None, 64, 64, None, None, 2, 0, S.addr(hp), None, None, None, 16, 0)
    _refused(lib.icrl_cn_train_minibatch_batch(1, b(mj), ws, 8192, None), L, text)
    _refused(lib.icrl_cn_prepare(b(d), None, None, 4, None, None), L, text, "icrl_cn_prepare:")
    _refused(lib.icrl_costnet_prepare(b(d), None), L, text, "icrl_costnet_prepare:")
    _refused(lib.icrl_disc_reward(b(d), None, None, 4, None, 0, None), L, text, "icrl_disc_reward:")
    gj = S.GailJobT(S.addr(d), None, None, None, None, None, 0.0, None, None, None, 32, 0)
    _refused(lib.icrl_gail_unnormalize_batch(1, b(gj), ws, 8192, None), L, text)
    _refused(lib.icrl_gail_relabel_batch(1, b(gj), ws, 8192, None), L, text)
    _refused(lib.icrl_cost_mlp_fwd_bwd(b(d), None, 4, None, None, None, None, 0, None), L, text)


def test_a_generic_shape_policy_and_a_discriminator_wrapper_refuse_it():
    from icrl_amd import structs as S
    L = _lib()
    lib, b = L.lib(), ctypes.byref
    env, nm, pol, buf, ag = _rollout_args(S, h1=128)      # (a layer above 64 units: the generic-shape path)
    d = _desc(S)
    _refused(lib.icrl_rollout_collect_ex(b(env), b(nm), b(pol), b(d), b(buf), b(ag), None, None, None, 0.99, 0.95, 0.99, 0.95, 1, None), L,
             "icrl_rollout_collect:", NAMES, "generic-shape policy")
    _refused(lib.icrl_rollout_collect(b(env), b(nm), b(pol), b(d), b(buf), b(ag), None, None, None, 0.99, 0.95, 0.99, 0.95, None), L, NAMES, "generic-shape policy")
    hs = S.HostStepT(8, 0)
    assert lib.icrl_host_step(b(nm), b(pol), b(d), b(buf), b(ag), b(hs), None, None, None, 0, None) == 1      # (bad_dims: no generic-shape form there at all)
    lib.icrl_clear_error()
    # a region descriptor as the inner net of an icrl_cost_disc_t
    env, nm, pol, buf, ag = _rollout_args(S)
    wrap = S.CostDiscT(18, 6, 0, S.COST_DISC, S.addr(d))
    for call in (lambda: lib.icrl_rollout_collect_ex(b(env), b(nm), b(pol), b(wrap), b(buf), b(ag), None, None, None, 0.99, 0.95, 0.99, 0.95, 1, None),
                 lambda: lib.icrl_host_step(b(nm), b(pol), b(wrap), b(buf), b(ag), b(hs), None, None, None, 0, None),
                 lambda: lib.icrl_cost_mlp_forward(b(wrap), None, None, 4, None, None)):
        _refused(call(), L, "icrl_cost_disc_t", "inner net is a region cost descriptor (icrl_cost_region_t)")


def test_serving_entry_points_refuse_a_bad_descriptor_with_a_reason():
    """header, clause and term counts, type and combine, columns, action columns the policy's action space does not provide, r2 < 0, NULL
    tables — by icrl_rollout_collect[_ex], icrl_host_step, icrl_cost_mlp_forward and icrl_cost_region_rows alike, before any device call."""
    from icrl_amd import structs as S
    L = _lib()
    lib, b = L.lib(), ctypes.byref
    env, nm, pol, buf, ag = _rollout_args(S)
    hs = S.HostStepT(8, 0)
    box = lambda cols, n=None: (S.REGION_BOX, 0, cols, [-1.0] * 8, [1.0] * 8, 0.0)      # noqa: E731
    nine = _table(S, [box([0])] * 9)
    cases = [(_desc(S, in_dim=3), "in_dim = 3 (must be 0)"),
             (_desc(S, n=0), "with 0 clauses (1..8)"),
             (_desc(S, nine), "with 9 clauses (1..8)"),
             (_desc(S, combine=3), "unknown combine rule 3"),
             (_desc(S, combine=-1), "unknown combine rule -1"),
             (_desc(S, clauses=None), "NULL host clause table"),
             (_desc(S, d_clauses=None), "NULL device clause table"),
             (_desc(S, _table(S, [box([0]), (3, 0, [0], [0.0], [0.0], 0.0)])), "clause 1 of unknown type 3"),
             (_desc(S, _table(S, [(S.REGION_HALFSPACE, 0, [], [], [], 0.0)])), "clause 0 with 0 terms (1..8)"),
             (_desc(S, _table(S, [box(list(range(9)))])), "clause 0 with 9 terms (1..8)"),
             (_desc(S, _table(S, [box([0, 24])])), "clause 0, term 1 reads column 24 outside obs_dim 18 + acs_dim 6"),
             (_desc(S, _table(S, [box([-1])])), "clause 0, term 0 reads column -1 outside"),
             (_desc(S, _table(S, [box([0]), (S.REGION_BALL, 0, [1], [0.0], [0.0], -0.25)])), "clause 1 is a ball with r2 = -0.25"),
             (_desc(S, _table(S, [(S.REGION_BALL, 0, [1], [0.0], [0.0], math.nan)])), "clause 0 is a ball with r2 = nan")]
    for d, text in cases:
        for who, call in (("icrl_rollout_collect", lambda: lib.icrl_rollout_collect_ex(b(env), b(nm), b(pol), b(d), b(buf), b(ag), None, None, None, 0.99, 0.95, 0.99, 0.95, 1, None)),
                          ("icrl_rollout_collect", lambda: lib.icrl_rollout_collect(b(env), b(nm), b(pol), b(d), b(buf), b(ag), None, None, None, 0.99, 0.95, 0.99, 0.95, None)),
                          ("icrl_host_step", lambda: lib.icrl_host_step(b(nm), b(pol), b(d), b(buf), b(ag), b(hs), None, None, None, 0, None)),
                          ("icrl_cost_mlp_forward", lambda: lib.icrl_cost_mlp_forward(b(d), 1, 1, 4, 1, None)),
                          ("icrl_cost_region_rows", lambda: lib.icrl_cost_region_rows(b(d), 1, 1, 4, 1, None))):
            msg = _refused(call(), L, NAMES, text)
            assert msg.startswith("icrl_cost_region_rows" if who == "icrl_cost_mlp_forward" else who), msg
    # beside a policy: the env's obs_dim, and action columns the policy's action space provides
    _refused(lib.icrl_rollout_collect_ex(b(env), b(nm), b(pol), b(_desc(S, obs_dim=17)), b(buf), b(ag), None, None, None, 0.99, 0.95, 0.99, 0.95, 1, None), L,
             NAMES, "built for obs_dim 17, the env has 18")
    _refused(lib.icrl_host_step(b(nm), b(pol), b(_desc(S, obs_dim=17)), b(buf), b(ag), b(hs), None, None, None, 0, None), L, "built for obs_dim 17, the env has 18")
    env_d, nm_d, pol_d, buf_d, ag_d = _rollout_args(S, discrete=1)
    act1 = _desc(S, _table(S, [box([18 + 1])]))      # action column 1: a discrete policy provides column 0 alone
    _refused(lib.icrl_rollout_collect_ex(b(env_d), b(nm_d), b(pol_d), b(act1), b(buf_d), b(ag_d), None, None, None, 0.99, 0.95, 0.99, 0.95, 1, None), L,
             NAMES, "clause 0, term 0 reads action column 1, the policy's action space provides 1")
    _refused(lib.icrl_host_step(b(nm_d), b(pol_d), b(act1), b(buf_d), b(ag_d), b(hs), None, None, None, 0, None), L, "reads action column 1")
    wide_acs = _desc(S, _table(S, [box([18 + 6])]), acs_dim=8)      # action column 6 of a descriptor built for 8: the Box policy has 6
    _refused(lib.icrl_rollout_collect_ex(b(env), b(nm), b(pol), b(wide_acs), b(buf), b(ag), None, None, None, 0.99, 0.95, 0.99, 0.95, 1, None), L,
             "reads action column 6, the policy's action space provides 6")
    # the rows entry points: the tag, N, the output, the arrays the clauses read
    good = _desc(S, _table(S, [box([0, 18 + 2])]))
    _refused(lib.icrl_cost_region_rows(b(S.CostFnT(18, 6, 0, S.COST_FN, 0, 0, 0.0, 0.0)), 1, 1, 4, 1, None), L, "not a region cost descriptor", NAMES)
    _refused(lib.icrl_cost_region_rows(None, 1, 1, 4, 1, None), L, "not a region cost descriptor")
    _refused(lib.icrl_cost_region_rows(b(good), 1, 1, 0, 1, None), L, "N = 0 rows")
    _refused(lib.icrl_cost_region_rows(b(good), 1, 1, 4, None, None), L, "N = 4 rows, cost =")
    _refused(lib.icrl_cost_region_rows(b(good), None, 1, 4, 1, None), L, NAMES, "clause 0, term 0 reads the observations, which is NULL")
    _refused(lib.icrl_cost_mlp_forward(b(good), 1, None, 4, 1, None), L, NAMES, "clause 0, term 1 reads the actions, which is NULL")


# ---- 3. the spec parser ---------------------------------------------------------------------------------------------------------------------
def test_spec_parsing_dict_string_and_path(tmp_path):
    from icrl_amd import structs as S
    from icrl_amd.true_constraint_net import RegionCost
    spec = {"combine": "sum", "clauses": [{"type": "box", "cols": ["obs:0", "act:2"], "lo": [None, -0.5], "hi": [1.5, None]},
                                          {"type": "halfspace", "cols": ["obs:3"], "w": [2.0], "b": -1.0, "negate": True},
                                          {"type": "ball", "cols": ["obs:1", "obs:17"], "center": [0.5, -0.5], "radius": 1.5}]}
    path = tmp_path / "disc.json"
    path.write_text(json.dumps(spec))
    for src in (spec, json.dumps(spec), str(path), path):
        rc = RegionCost.from_spec(src, 18, 6)
        assert rc.combine == S.REGION_SUM and (rc.obs_dim, rc.acs_dim, rc.discrete) == (18, 6, False)
        assert rc.clauses == [(S.REGION_BOX, False, [0, 20], [-math.inf, -0.5], [1.5, math.inf], 0.0),
                              (S.REGION_HALFSPACE, True, [3], [2.0], [0.0], -1.0),
                              (S.REGION_BALL, False, [1, 17], [0.5, -0.5], [0.0, 0.0], 2.25)]
        tab = rc.table()
        assert len(tab) == 3 and (tab[0].type, tab[0].n_terms, tab[0].col[1], tab[0].a[0], tab[0].b[1]) == (0, 2, 20, -math.inf, math.inf)
        assert (tab[1].negate, tab[1].c, tab[2].c, tab[2].a[1]) == (1, -1.0, 2.25, -0.5)
        assert rc.reads_obs and rc.reads_acs
    assert RegionCost.from_spec(str(path), 18, 6).name == "disc.json"
    # defaults: combine any, missing box bounds infinite, scalar bounds broadcast, b = 0
    rc = RegionCost.from_spec({"clauses": [{"type": "box", "cols": ["obs:0", "obs:1"], "hi": 2}, {"type": "halfspace", "cols": ["obs:0"], "w": [1]}]}, 4, 2)
    assert rc.combine == S.REGION_ANY and rc.clauses[0][3:5] == ([-math.inf] * 2, [2.0, 2.0]) and rc.clauses[1][5] == 0.0
    # discrete: one action column, whatever acs_dim says
    rc = RegionCost.from_spec({"clauses": [{"type": "box", "cols": ["act:0"], "lo": [1], "hi": [1]}]}, 2, 3, discrete=True)
    assert rc.acs_dim == 1 and rc.clauses[0][2] == [2] and not rc.reads_obs


@pytest.mark.parametrize("spec,text", [
    ("{not json", "not JSON"),
    ([1, 2], "must be an object"),
    ({"combine": "any", "clauses": [], "extra": 1}, "unknown field(s) ['extra']"),
    ({"combine": "xor", "clauses": [{"type": "box", "cols": ["obs:0"]}]}, "combine: 'xor'"),
    ({"combine": "any"}, "clauses: a list of 1..8"),
    ({"clauses": []}, "clauses: a list of 1..8"),
    ({"clauses": [{"type": "box", "cols": ["obs:0"]}] * 9}, "clauses: a list of 1..8"),
    ({"clauses": ["box"]}, "clause 0: an object is required"),
    ({"clauses": [{"type": "box", "cols": ["obs:0"]}, {"type": "cone", "cols": ["obs:0"]}]}, "clause 1: type: 'cone'"),
    ({"clauses": [{"type": "box", "cols": ["obs:0"], "w": [1]}]}, "clause 0: unknown field(s) ['w'] for a box"),
    ({"clauses": [{"type": "box"}]}, "clause 0: cols: a list of 1..8"),
    ({"clauses": [{"type": "box", "cols": []}]}, "clause 0: cols: a list of 1..8"),
    ({"clauses": [{"type": "box", "cols": ["obs:0"] * 9}]}, "clause 0: cols: a list of 1..8"),
    ({"clauses": [{"type": "box", "cols": ["pos:0"]}]}, "clause 0: cols: 'pos:0' is not"),
    ({"clauses": [{"type": "box", "cols": [3]}]}, "clause 0: cols: 3 is not"),
    ({"clauses": [{"type": "box", "cols": ["obs:18"]}]}, "clause 0: cols: 'obs:18' is outside the 18 observation"),
    ({"clauses": [{"type": "box", "cols": ["act:6"]}]}, "clause 0: cols: 'act:6' is outside the 6 action"),
    ({"clauses": [{"type": "box", "cols": ["obs:0", "obs:1"], "lo": [0.0]}]}, "clause 0: lo: 1 values for 2 cols"),
    ({"clauses": [{"type": "box", "cols": ["obs:0"], "hi": ["x"]}]}, "clause 0: hi: 'x' is not a number"),
    ({"clauses": [{"type": "box", "cols": ["obs:0"], "negate": 1}]}, "clause 0: negate: 1 is not true or false"),
    ({"clauses": [{"type": "halfspace", "cols": ["obs:0"]}]}, "clause 0: w: missing"),
    ({"clauses": [{"type": "halfspace", "cols": ["obs:0"], "w": [None]}]}, "clause 0: w: None is not a number"),
    ({"clauses": [{"type": "ball", "cols": ["obs:0"], "center": [0.0]}]}, "clause 0: radius: missing"),
    ({"clauses": [{"type": "ball", "cols": ["obs:0"], "radius": 1.0}]}, "clause 0: center: missing"),
    ({"clauses": [{"type": "ball", "cols": ["obs:0"], "center": [0.0], "radius": -1.0}]}, "clause 0: radius: -1.0 must be >= 0"),
])
def test_spec_validation_errors_name_the_clause_and_the_field(spec, text):
    from icrl_amd.true_constraint_net import RegionCost
    with pytest.raises(ValueError) as e:
        RegionCost.from_spec(spec, 18, 6)
    assert text in str(e.value) and "RegionCost" in str(e.value), str(e.value)


def test_a_discrete_action_space_has_one_action_column():
    from icrl_amd.true_constraint_net import RegionCost
    with pytest.raises(ValueError, match=r"clause 0: cols: 'act:1' is outside the 1 action column\(s\) of a discrete action space"):
        RegionCost.from_spec({"clauses": [{"type": "box", "cols": ["act:1"]}]}, 2, 3, discrete=True)


# ---- 4. the numpy form against the one-row-at-a-time evaluator, bit for bit -----------------------------------------------------------------
_SHAPES = [(18, 6, False), (113, 8, False), (2, 1, True)]


def _check_numpy(spec, od, ad, disc, seed, n=96, want_edge=True):
    from icrl_amd.true_constraint_net import RegionCost
    rc = RegionCost.from_spec(spec, od, ad, disc)
    obs, acs, n_edge = RC.rows_for(spec, seed, n, od, ad, disc)
    if want_edge:
        assert n_edge >= 1 and all(RC.on_threshold(spec, list(obs[i]), acs[i]) for i in range(n_edge)), "rows exactly on a threshold"
    got, want = rc(obs, acs), RC.evaluate(spec, obs, acs)
    assert isinstance(got, np.ndarray) and got.dtype == np.float32 and got.shape == (n,)
    assert np.array_equal(got, want), (spec, np.flatnonzero(got != want))
    return got


@pytest.mark.parametrize("od,ad,disc", _SHAPES)
def test_numpy_form_equals_the_row_evaluator_for_every_type_negate_and_combine(od, ad, disc):
    seen = set()
    for i, (name, spec) in enumerate(RC.product_specs(od, ad)):
        seen.update(_check_numpy(spec, od, ad, disc, 100 + i).tolist())
    assert seen == {0.0, 1.0, 2.0}      # (sum over two clauses reaches all three values)


@pytest.mark.parametrize("od,ad,disc", _SHAPES)
def test_numpy_form_equals_the_row_evaluator_for_an_8_by_8_spec_and_the_general_specs(od, ad, disc):
    spec = RC.full_spec(od, ad)
    assert len(spec["clauses"]) == 8 and all(len(q["cols"]) == 8 for q in spec["clauses"])
    got = _check_numpy(spec, od, ad, disc, 7, n=128, want_edge=not disc)
    assert len(set(got.tolist())) >= 3, set(got.tolist())
    if not disc:
        for i, (name, gs) in enumerate(RC.general_specs(od, ad)):
            got = _check_numpy(gs, od, ad, disc, 40 + i)
            assert 0.0 < got.mean() < 1.0, name


def test_a_nan_makes_the_unnegated_clause_false_and_leading_dimensions_are_kept():
    from icrl_amd.true_constraint_net import RegionCost
    od, ad = 4, 2
    for kind in ("box", "halfspace", "ball"):
        for negate in (False, True):
            spec = dict(combine="any", clauses=[RC.clause_of(kind, ["obs:3", "obs:0", "act:1"], negate)])
            obs = np.zeros((3, od)); obs[1, 0] = np.nan; obs[2, 3] = np.nan
            acs = np.zeros((3, ad), np.float32)
            got = RegionCost.from_spec(spec, od, ad)(obs, acs)
            assert np.array_equal(got, RC.evaluate(spec, obs, acs)) and got[1] == got[2] == (1.0 if negate else 0.0), (kind, negate)
    spec = RC.general_specs(od, ad)[0][1]
    rng = np.random.RandomState(0)
    obs, acs = rng.randn(5, 3, od), rng.randn(5, 3, ad).astype(np.float32)
    got = RegionCost.from_spec(spec, od, ad)(obs, acs)
    assert got.shape == (5, 3) and np.array_equal(got.reshape(-1), RC.evaluate(spec, obs.reshape(-1, od), acs.reshape(-1, ad)))


# ---- 5. the six identities with the analytic kinds ------------------------------------------------------------------------------------------
def test_every_analytic_kind_is_a_region_cost():
    from helpers.cost_fn_cases import boundary_acs, boundary_obs
    from icrl_amd.true_constraint_net import AnalyticCost, RegionCost
    od, ad, index = 18, 6, 17
    lo, hi, thr = -0.25, 0.75, 0.5
    rng = np.random.RandomState(3)
    obs = rng.randn(200, od) * 0.8
    edge = boundary_obs(lo, hi, index, od)      # the thresholds themselves and nextafter on both sides
    obs[:len(edge)] = edge
    acs = (rng.randn(200, ad) * 0.4).astype(np.float32)
    eacs = boundary_acs(thr, ad)
    acs[:len(eacs)] = eacs
    assert (obs[:, index] == lo).any() and (obs[:, index] == hi).any() and (np.abs(acs) == np.float32(thr)).any()
    disc = rng.randint(0, 3, size=(200, 1)).astype(np.float32)
    pairs = [(RegionCost.null(od, ad), AnalyticCost.null(), acs),
             (RegionCost.wall_behind(lo, index, od, ad), AnalyticCost.wall_behind(lo, index), acs),
             (RegionCost.wall_infront(hi, index, od, ad), AnalyticCost.wall_infront(hi, index), acs),
             (RegionCost.wall_behind_and_infront(lo, hi, index, od, ad), AnalyticCost.wall_behind_and_infront(lo, hi, index), acs),
             (RegionCost.wall_behind_and_infront(hi, lo, index, od, ad), AnalyticCost.wall_behind_and_infront(hi, lo, index), acs),
             (RegionCost.torque(thr, od, ad), AnalyticCost.torque(thr), acs),
             (RegionCost.action_equals(1, od), AnalyticCost.action_equals(1), disc)]
    for rc, ac, a in pairs:
        got, want = rc(obs, a), np.asarray(ac(obs, a), np.float32)
        assert got.dtype == np.float32 and np.array_equal(got, want), (rc, np.flatnonzero(got != want))
    assert set(pairs[4][0](obs, acs).tolist()) == {1.0, 2.0}      # (crossed walls: both hold in between)
    # the same identities written as specs
    specs = [({"clauses": [{"type": "box", "cols": [f"obs:{index}"], "hi": [lo]}]}, pairs[1][1]),
             ({"clauses": [{"type": "box", "cols": [f"obs:{index}"], "lo": [hi]}]}, pairs[2][1]),
             ({"combine": "sum", "clauses": [{"type": "box", "cols": [f"obs:{index}"], "hi": [lo]}, {"type": "box", "cols": [f"obs:{index}"], "lo": [hi]}]}, pairs[3][1]),
             ({"clauses": [{"type": "box", "cols": [f"act:{j}" for j in range(ad)], "lo": -thr, "hi": thr, "negate": True}]}, pairs[5][1]),
             ({"clauses": [{"type": "box", "cols": ["obs:0"], "negate": True}]}, pairs[0][1])]
    for spec, ac in specs:
        assert np.array_equal(RegionCost.from_spec(spec, od, ad)(obs, acs), np.asarray(ac(obs, acs), np.float32)), spec
    spec = {"clauses": [{"type": "box", "cols": ["act:0"], "lo": [1], "hi": [1]}]}
    assert np.array_equal(RegionCost.from_spec(spec, od, 3, discrete=True)(obs, disc), np.asarray(AnalyticCost.action_equals(1)(obs, disc), np.float32))


# ---- 6. wiring that needs no device ---------------------------------------------------------------------------------------------------------
_DISC = json.dumps({"clauses": [{"type": "ball", "cols": ["obs:0", "obs:1"], "center": [0.0, 0.0], "radius": 1.0}]})


def _cfg(seed, extra=(), mod="cpg"):
    import importlib
    m = importlib.import_module(f"icrl_amd.{mod}")
    argv = [mod, "-tei", "HCWithPos-v0", "-eei", "HCWithPosTest-v0", "-nt", "8", "-ns", "64", "-t", "1024", "-ne", "2", "-s", str(seed), "-v", "0", *extra]
    cfg = vars(m.build_parser().parse_args(argv))
    cfg.update(rank=0, world_size=1, save_dir=None)
    return types.SimpleNamespace(**cfg)


def test_the_flag_is_parsed_by_cpg_icrl_and_gail_and_absent_unless_given():
    from icrl_amd import cpg, gail, icrl
    for m in (cpg, icrl, gail):
        p = m.build_parser()
        assert "cost_spec" not in vars(p.parse_args([])), m.__name__
        assert vars(p.parse_args(["--cost_spec", "disc.json"]))["cost_spec"] == "disc.json"
        assert vars(p.parse_args(["-csp", _DISC]))["cost_spec"] == _DISC


def test_the_flag_conflicts_with_a_cost_of_another_origin():
    _lib()
    from icrl_amd import cpg
    from icrl_amd.true_constraint_net import check_cost_spec_flags
    for extra, flag in ((("--cn_path", "unused.pt"), "--cn_path"), (("--use_null_cost",), "--use_null_cost")):
        cfg = _cfg(0, ("--cost_spec", _DISC) + extra)
        with pytest.raises(ValueError, match="--cost_spec together with " + flag):
            check_cost_spec_flags(cfg)
        with pytest.raises(ValueError, match="--cost_spec together with " + flag):      # (before setup builds anything)
            cpg.setup(cfg, log=None)
    check_cost_spec_flags(_cfg(0, ("--cn_path", "unused.pt")))
    check_cost_spec_flags(_cfg(0, ("--cost_spec", _DISC)))


def test_a_seed_batch_refuses_cost_spec_and_names_it():
    """(the refusal comes before the batch builds anything on the device)"""
    _lib()
    from icrl_amd.seed_batch import CpgSeedBatch, GailSeedBatch, SeedBatch
    extra = ("--cost_spec", _DISC)
    for cls in (CpgSeedBatch, GailSeedBatch, SeedBatch):
        with pytest.raises(ValueError, match="--cost_spec") as e:
            cls([_cfg(0, extra), _cfg(1, extra)])
        assert "seed batch" in str(e.value) and "no region form" in str(e.value)


def test_the_wrapper_accessor_the_resolver_and_the_sde_reason():
    _lib()
    from icrl_amd import spaces
    from icrl_amd.ppo_lag import PPOLagrangian
    from icrl_amd.true_constraint_net import AnalyticCost, RegionCost, cost_for
    from icrl_amd.vec_env import VecCostWrapper
    rc = RegionCost.from_spec(_DISC, 18, 6)
    cw = VecCostWrapper.__new__(VecCostWrapper)
    cw.cost_function = rc
    assert cw.region_cost() is rc and cw.analytic_cost() is None and cw.discriminator_cost() is None and cw.constraint_net() is None
    cw.cost_function = AnalyticCost.null()
    assert cw.region_cost() is None
    # _sde_rollout_reason: a RegionCost behind the fused chain
    cw.cost_function = rc
    agent = types.SimpleNamespace(sde_fused_rollout=True, _fused_chain=lambda: (None, cw, None))
    buf = types.SimpleNamespace(buffer_size=8)
    assert PPOLagrangian._sde_rollout_reason(agent, "cost", 8, buf) == "a RegionCost (the gSDE kernels have no region form)"
    # _fused_cost_ok and its switch
    assert PPOLagrangian._fused_cost_ok(cw)
    os.environ["ICRL_REGION_COST_STEPPED"] = "1"
    try:
        assert not PPOLagrangian._fused_cost_ok(cw)
    finally:
        del os.environ["ICRL_REGION_COST_STEPPED"]
    # the resolver: the id's cost without a spec, the spec's over the env's spaces with one
    assert cost_for("HCWithPosTest-v0").name == "wall_behind"
    env = types.SimpleNamespace(observation_space=spaces.Box(-np.inf, np.inf, (18,)), action_space=spaces.Box(-1.0, 1.0, (6,)))
    got = cost_for("HCWithPosTest-v0", _DISC, env)
    assert isinstance(got, RegionCost) and (got.obs_dim, got.acs_dim, got.discrete) == (18, 6, False)
    env = types.SimpleNamespace(observation_space=spaces.Box(-np.inf, np.inf, (2,)), action_space=spaces.Discrete(3))
    got = cost_for("CLGW-v0", {"clauses": [{"type": "box", "cols": ["act:0"], "lo": [1], "hi": [1]}]}, env)
    assert (got.obs_dim, got.acs_dim, got.discrete) == (2, 1, True)


def test_the_switch_and_the_flag_are_documented():
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "--cost_spec" in readme and "ICRL_REGION_COST_STEPPED" in readme
    assert "ICRL_REGION_COST_STEPPED" in open(os.path.join(ROOT, "icrl_amd", "ppo_lag.py")).read()
    assert "icrl_cost_region_t" in open(os.path.join(ROOT, "DESIGN.md")).read()
