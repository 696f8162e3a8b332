"""CPU: the batched discriminator step — icrl_cn_train_minibatch_batch, icrl_gail_unnormalize_batch and icrl_gail_relabel_batch are
declared, exported and bound, and refuse bad arguments on the host before any device call (no GPU needed); --seeds of gail and icrl;
what GailSeedBatch refuses before it sets a run up."""
import ctypes
import json
import os
import re
import types

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("icrl_cn_train_minibatch_batch", "icrl_gail_unnormalize_batch", "icrl_gail_relabel_batch")


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


def test_new_exports_are_declared_exported_and_bound():
    L = _lib()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "icrl_hip.h")).read(), flags=re.S)
    job = {"icrl_cn_train_minibatch_batch": "icrl_cn_train_mb_job_t", "icrl_gail_unnormalize_batch": "icrl_gail_job_t",
           "icrl_gail_relabel_batch": "icrl_gail_job_t"}
    for name in NEW:
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", src)
        assert decl is not None, name
        args = [a.strip() for a in decl.group(1).split(",")]
        assert args == ["int n_runs", f"const {job[name]}* jobs", "void* args_ws", "long long args_ws_bytes", "void* stream"], (name, args)
        assert hasattr(L.lib(), name)
        assert L.SIGNATURES[name] == [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_void_p]
        assert L.SIGNATURES[name] == L.SIGNATURES["icrl_cn_train_batch"]
    assert L.lib().icrl_abi_version() == 107           # exports only


def test_no_struct_changed_and_the_new_jobs_have_the_header_layout():
    from icrl_amd import structs as S
    assert ctypes.sizeof(S.CnTrainJobT) == 6 * 8 + 2 * 4 + 2 * 8 + 2 * 4 + 3 * 8
    assert ctypes.sizeof(S.CostNetT) == 10 * 4 + 8 + 5 * 8 + 8 + 2 * 8
    assert ctypes.sizeof(S.CnHyperT) == 4 * 4 + 8 * 4
    assert ctypes.sizeof(S.GaeJobT) == 13 * 8 + 8
    assert ctypes.sizeof(S.CostFnT) == 6 * 4 + 2 * 8
    # icrl_cn_train_mb_job_t: the fields of icrl_cn_train_job_t, then perms and batch_size (+ pad)
    assert ctypes.sizeof(S.CnTrainMbJobT) == ctypes.sizeof(S.CnTrainJobT) + 8 + 2 * 4
    assert [f[0] for f in S.CnTrainMbJobT._fields_][:len(S.CnTrainJobT._fields_)] == [f[0] for f in S.CnTrainJobT._fields_]
    assert S.CnTrainMbJobT.perms.offset == ctypes.sizeof(S.CnTrainJobT) and S.CnTrainMbJobT.batch_size.offset == ctypes.sizeof(S.CnTrainJobT) + 8
    assert ctypes.sizeof(S.GailJobT) == 6 * 8 + 8 + 3 * 8 + 2 * 4
    assert S.GailJobT.epsilon.offset == 48 and S.GailJobT.rows.offset == 80


# ---- host-side refusals of icrl_cn_train_minibatch_batch ----------------------------------------------------------------------------------
def _net(S, hidden=(20,), in_dim=24):
    h = list(hidden) + [0] * (4 - len(hidden))
    n, last = 0, in_dim
    for w in hidden:
        n += w * last + w
        last = w
    n += last + 1
    return S.CostNetT(18, 6, in_dim, len(hidden), h[0], h[1], h[2], h[3], 0, n)


def _mb_job(S, net, hp, perms, batch_size=64, Nn=70, Ne=150):
    return S.CnTrainMbJobT(S.addr(net), None, None, None, None, None, Nn, Ne, None, None, 1, 0, S.addr(hp), None, None,
                           ctypes.addressof(perms) if perms is not None else None, batch_size, 0)


def test_minibatch_batch_refuses_on_the_host():
    from icrl_amd import structs as S
    L = _lib()
    fn = L.lib().icrl_cn_train_minibatch_batch
    hp = S.CnHyperT(3, 0, 0, 1, 0.0, 1e-5, -1.0, -1.0, 0.01, 0.9, 0.999, 1e-5)
    perms = (ctypes.c_int32 * 512)()
    scratch = (ctypes.c_char * 4096)()
    ws = ctypes.addressof(scratch)
    a, b, deeper, wider_in = _net(S), _net(S), _net(S, (30, 30)), _net(S, (20,), 25)            # (kept alive: the jobs hold their addresses)

    def jobs(*js):
        return (S.CnTrainMbJobT * len(js))(*js)
    good = _mb_job(S, a, hp, perms)
    _refused(fn(0, jobs(good), ws, 4096, None), L, "n_runs = 0")
    _refused(fn(2, jobs(good, _mb_job(S, b, hp, perms)), ws, 2 * L.BATCH_ARGS_BYTES - 1, None), L, "args_ws holds")
    _refused(fn(1, jobs(good), None, 4096, None), L, "args_ws holds")
    _refused(fn(1, jobs(_mb_job(S, a, hp, None)), ws, 4096, None), L, "perms = NULL")
    _refused(fn(2, jobs(good, _mb_job(S, b, hp, None)), ws, 4096, None), L, "run 1 has no permutation table")
    _refused(fn(1, jobs(_mb_job(S, a, hp, perms, batch_size=0)), ws, 4096, None), L, "batch_size = 0")
    _refused(fn(2, jobs(good, _mb_job(S, deeper, hp, perms)), ws, 4096, None), L, "network shape differs from run 0's")
    _refused(fn(2, jobs(good, _mb_job(S, wider_in, hp, perms)), ws, 4096, None), L, "network shape differs from run 0's")
    _refused(fn(2, jobs(good, _mb_job(S, b, hp, perms, batch_size=32)), ws, 4096, None), L, "batch_size 32 differs from run 0's 64")
    cf = S.CostFnT(18, 6, 0, S.COST_FN, S.COST_WALL_BEHIND, 0, -3.0, 0.0)
    analytic = _mb_job(S, a, hp, perms)
    analytic.cn = S.addr(cf)
    _refused(fn(1, jobs(analytic), ws, 4096, None), L, "is not served here")
    _refused(fn(2, jobs(good, analytic), ws, 4096, None), L, "is not served here")
    _refused(fn(1, jobs(_mb_job(S, a, hp, perms, Nn=0)), ws, 4096, None), L, "needs nominal rows (0)")


def test_gail_entry_points_refuse_on_the_host():
    from icrl_amd import structs as S
    L = _lib()
    buf = (ctypes.c_char * 64)()
    ptr = ctypes.addressof(buf)            # (never dereferenced on the host)
    scratch = (ctypes.c_char * 4096)()
    ws = ctypes.addressof(scratch)
    net = _net(S)
    cf = S.CostFnT(18, 6, 0, S.COST_FN, S.COST_WALL_BEHIND, 0, -3.0, 0.0)

    def job(**kw):
        f = dict(disc=S.addr(net), true_cost=None, observations=ptr, actions=ptr, obs_mean=None, obs_var=None, epsilon=1e-8, raw_obs=ptr,
                 rewards=ptr, cost_mean=ptr, rows=132, learn_cost=1)
        f.update(kw)
        return (S.GailJobT * 1)(S.GailJobT(*[f[k] for k, _ in S.GailJobT._fields_]))
    for fn in (L.lib().icrl_gail_unnormalize_batch, L.lib().icrl_gail_relabel_batch):
        _refused(fn(0, job(), ws, 4096, None), L, "n_runs = 0")
        _refused(fn(1, job(), ws, L.BATCH_ARGS_BYTES - 1, None), L, "args_ws holds")
        _refused(fn(1, job(disc=S.addr(cf)), ws, 4096, None), L, "is not served here")
        _refused(fn(1, job(rows=0), ws, 4096, None), L, "rows = 0")
    un = L.lib().icrl_gail_unnormalize_batch
    _refused(un(1, job(obs_mean=ptr), ws, 4096, None), L, "obs_mean and obs_var come together")
    _refused(un(1, job(true_cost=S.addr(net)), ws, 4096, None), L, "not an analytic cost descriptor")
    bad = S.CostFnT(18, 6, 0, S.COST_FN, S.COST_WALL_BEHIND, 18, -3.0, 0.0)
    _refused(un(1, job(true_cost=S.addr(bad)), ws, 4096, None), L, "column 18 outside the observation")
    other = _net(S, (30, 30))            # (kept alive: the job holds its address)
    two = (S.GailJobT * 2)(job()[0], job(disc=S.addr(other))[0])
    _refused(L.lib().icrl_gail_relabel_batch(2, two, ws, 4096, None), L, "discriminator shape differs from run 0's")


# ---- command line ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("driver", ["gail", "icrl"])
def test_parsers_accept_seeds_and_change_nothing_else(driver):
    import importlib
    mod = importlib.import_module(f"icrl_amd.{driver}")
    argv = [driver, "-tei", "HCWithPos-v0", "-eei", "HCWithPosTest-v0", "-nt", "8", "-ns", "64", "-s", "3"]
    base = vars(mod.build_parser().parse_args(argv))
    assert base.pop("seeds") is None
    with_seeds = vars(mod.build_parser().parse_args(argv + ["--seeds", "0", "1", "2", "5"]))
    assert with_seeds.pop("seeds") == [0, 1, 2, 5]
    assert with_seeds == base and base["seed"] == 3


def test_seed_configs_is_shared_and_builds_the_per_seed_directories(tmp_path):
    from icrl_amd import cpg, gail, utils
    assert cpg.seed_configs is utils.seed_configs
    cfg = vars(gail.build_parser().parse_args(["gail", "--seeds", "4", "7", "--save_dir", str(tmp_path / "out")]))
    runs = utils.seed_configs(cfg)
    assert [r.seed for r in runs] == [4, 7]
    for r in runs:
        assert r.save_dir == str(tmp_path / "out" / f"seed_{r.seed}")
        saved = json.load(open(os.path.join(r.save_dir, "config.json")))
        assert saved["seed"] == r.seed and saved["save_dir"] == r.save_dir and saved["disc_layers"] == cfg["disc_layers"]
    assert [r.save_dir for r in utils.seed_configs(dict(cfg, save_dir=None))] == [None, None]
    # one value is the single-run path with that seed; several are a batch; duplicates are refused
    one = dict(cfg, seeds=[9])
    assert utils.batch_seeds(one) is None and one["seed"] == 9
    assert utils.batch_seeds(dict(cfg, seeds=None)) is None
    assert utils.batch_seeds(dict(cfg)) == [4, 7]
    for main in (gail.main, __import__("icrl_amd.icrl", fromlist=["main"]).main, cpg.main):
        with pytest.raises(ValueError, match="every seed is given once"):
            main(["x", "--seeds", "1", "2", "1"])


# ---- GailSeedBatch: refused before any run is set up ---------------------------------------------------------------------------------------
def _cfg(seed, *extra, **over):
    from icrl_amd.gail import build_parser
    argv = ["gail", "-tei", "HCWithPos-v0", "-eei", "HCWithPosTest-v0", "-nt", "4", "-ns", "64", "-bs", "64", "-ne", "2", "-dl", "30", "-lc",
            "-t", "768", "-ee", "256", "-s", str(seed), "-v", "0", *extra]
    cfg = vars(build_parser().parse_args(argv))
    cfg.update(rank=0, world_size=1, save_dir=None)
    cfg.update(over)
    return types.SimpleNamespace(**cfg)


def test_gail_seed_batch_refuses_before_set_up(monkeypatch):
    from icrl_amd import gail as G, seed_batch as SB

    def no_setup(*a, **k):
        raise AssertionError("a refused batch must not set a run up")
    monkeypatch.setattr(G, "setup", no_setup)
    with pytest.raises(ValueError, match="not device-resident envs"):
        SB.GailSeedBatch([_cfg(s, train_env_id="HostHCWithPos-v0", eval_env_id="HostHCWithPosTest-v0") for s in (0, 1)])
    with pytest.raises(ValueError, match="ONE rank"):
        SB.GailSeedBatch([_cfg(0), _cfg(1, world_size=2)])
    for key, value in (("timesteps", 1024), ("eval_every", 128.0), ("learn_cost", False), ("disc_batch_size", 96), ("disc_layers", [20]),
                       ("n_steps", 32), ("num_threads", 8)):
        with pytest.raises(ValueError, match=key):
            SB.GailSeedBatch([_cfg(0), _cfg(1, **{key: value})])
    with pytest.raises(ValueError, match="gail_path is None"):
        SB.GailSeedBatch([_cfg(0), _cfg(1, gail_path="some.pt")])
    with pytest.raises(ValueError, match="episode_stats"):
        SB.GailSeedBatch([_cfg(0), _cfg(1, episode_stats=True)])
    with pytest.raises(NotImplementedError, match="use_cost_shaping_callback"):
        SB.GailSeedBatch([_cfg(0, "--use_cost_shaping_callback"), _cfg(1, "--use_cost_shaping_callback")])
    with pytest.raises(ValueError, match="no runs"):
        SB.GailSeedBatch([])
