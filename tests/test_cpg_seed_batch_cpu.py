"""CPU: the batched rollout entry point for runs against a fixed cost (icrl_rollout_collect_batch_cost) — it is declared, exported and
bound, and its argument checks run on the host before any device call (no GPU needed); cpg's --seeds flag."""
import ctypes
import os
import re

import pytest


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


def _rollout_args(S, discrete=False):
    env = S.EnvT(4, 18, 1 if discrete else 6, 1000, 0, 0, 0, 0)
    nm = S.NormT(1, 1, 1, 1)
    pol = S.PolicyT(18, 2 if discrete else 6, 64, 64, 1 if discrete else 0, 1, None, None)
    buf = S.BufferT(8, 4, 18, 1 if discrete else 6)
    ag = S.AgentT()
    return env, nm, pol, buf, ag


def _call(L, n_runs, jobs, scratch, nbytes):
    return L.lib().icrl_rollout_collect_batch_cost(n_runs, jobs, None, None, None, 0.99, 0.95, 0.99, 0.95, 1,
                                                   ctypes.addressof(scratch) if scratch is not None else None, nbytes, None)


def test_entry_point_is_declared_exported_and_bound_like_its_sibling():
    L = _lib()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "icrl_hip.h")).read(), flags=re.S)
    decl = re.search(r"\bint\s+icrl_rollout_collect_batch_cost\s*\(([^;]*)\)\s*;", src)
    assert decl is not None
    args = [a.strip() for a in decl.group(1).split(",")]
    assert len(args) == 13 and args[0] == "int n_runs" and "icrl_rollout_job_t" in args[1] and "icrl_monitor_t" in args[2]
    assert args[-3:] == ["void* args_ws", "long long args_ws_bytes", "void* stream"]
    assert hasattr(L.lib(), "icrl_rollout_collect_batch_cost")
    assert L.SIGNATURES["icrl_rollout_collect_batch_cost"] == L.SIGNATURES["icrl_rollout_collect_batch_mon"]
    assert L.lib().icrl_abi_version() == 107           # exports only: no struct and no existing signature changed


@pytest.mark.parametrize("fields,discrete,text", [
    (dict(kind=7), False, "unknown kind 7"),
    (dict(kind=-1), False, "unknown kind -1"),
    (dict(kind=1, index=18), False, "column 18 outside the observation (obs_dim 18)"),
    (dict(kind=2, index=-1), False, "column -1 outside the observation"),
    (dict(kind=3, index=200), False, "column 200 outside the observation"),
    (dict(kind=4), True, "torque cost needs a Box action space"),
    (dict(kind=5, index=1), False, "action-equals cost needs a discrete action space"),
    (dict(kind=1, in_dim=3), False, "in_dim = 3 (must be 0)"),
])
@pytest.mark.parametrize("bad_run", [0, 1])
def test_a_bad_descriptor_in_any_run_is_refused(fields, discrete, text, bad_run):
    from icrl_amd import structs as S
    L = _lib()
    env, nm, pol, buf, ag = _rollout_args(S, discrete)
    good = S.CostFnT(18, 2 if discrete else 6, 0, S.COST_FN, S.COST_NULL, 0, 0.0, 0.0)
    bad = S.CostFnT(18, 2 if discrete else 6, fields.get("in_dim", 0), S.COST_FN, fields["kind"], fields.get("index", 0), 0.0, 0.0)
    cfs = [good, good]
    cfs[bad_run] = bad
    jobs = (S.RolloutJobT * 2)(*[S.RolloutJobT(S.addr(env), S.addr(nm), S.addr(pol), S.addr(cf), S.addr(buf), S.addr(ag), None) for cf in cfs])
    scratch = (ctypes.c_char * 8192)()
    _refused(_call(L, 2, jobs, scratch, 8192), L, text)


def test_mixed_batches_zero_runs_and_a_small_workspace_are_refused():
    from icrl_amd import structs as S
    L = _lib()
    env, nm, pol, buf, ag = _rollout_args(S)
    cf = S.CostFnT(18, 6, 0, S.COST_FN, S.COST_WALL_BEHIND, 0, -3.0, 0.0)
    net = S.CostNetT(18, 6, 24, 2, 64, 64)           # a constraint net's header: n_hidden = 2 (never dereferenced: the mix is refused first)
    scratch = (ctypes.c_char * 8192)()

    def jobs_of(*cns):
        return (S.RolloutJobT * len(cns))(*[S.RolloutJobT(S.addr(env), S.addr(nm), S.addr(pol), S.addr(c), S.addr(buf), S.addr(ag), None) for c in cns])
    for mix in ((cf, net), (net, cf), (cf, None), (None, cf, cf)):
        _refused(_call(L, len(mix), jobs_of(*mix), scratch, 8192), L, "every run carries an analytic descriptor, or none does")
    _refused(_call(L, 0, jobs_of(cf), scratch, 8192), L, "n_runs = 0")
    _refused(_call(L, -3, jobs_of(cf), scratch, 8192), L, "n_runs = -3")
    # one argument block of ICRL_BATCH_ARGS_BYTES per run: two runs do not fit 1024 + 1023 bytes, and NULL holds nothing
    _refused(_call(L, 2, jobs_of(cf, cf), scratch, 2 * L.BATCH_ARGS_BYTES - 1), L, "args_ws holds")
    _refused(_call(L, 1, jobs_of(cf), None, 8192), L, "args_ws holds")
    # the siblings still take no analytic descriptor
    _refused(L.lib().icrl_rollout_collect_batch_mon(1, jobs_of(cf), None, None, None, 0.99, 0.95, 0.99, 0.95, 1, ctypes.addressof(scratch), 8192, None),
             L, "is not served here")


def test_parser_accepts_seeds_and_changes_nothing_else():
    from icrl_amd.cpg import build_parser, seed_configs
    argv = ["cpg", "-tei", "HCWithPos-v0", "-eei", "HCWithPosTest-v0", "-nt", "8", "-ns", "64", "-t", "1024", "-s", "3"]
    base = vars(build_parser().parse_args(argv))
    assert base.pop("seeds") is None
    # the namespace of the parser before --seeds existed: every flag of build_parser with its default, spelled out once
    assert set(base) == {
        "file_to_run", "config_file", "project", "name", "group", "message", "device", "verbose", "wandb_sweep", "sync_wandb", "cost_info_str",
        "train_env_id", "eval_env_id", "dont_normalize_obs", "dont_normalize_reward", "dont_normalize_cost", "seed", "policy_name", "shared_layers",
        "policy_layers", "reward_vf_layers", "cost_vf_layers", "cnn_features_dim", "timesteps", "n_steps", "batch_size", "n_epochs", "num_threads",
        "save_every", "eval_every", "plot_every", "reward_gamma", "reward_gae_lambda", "cost_gamma", "cost_gae_lambda", "clip_range",
        "clip_range_reward_vf", "clip_range_cost_vf", "ent_coef", "reward_vf_coef", "cost_vf_coef", "target_kl", "max_grad_norm", "learning_rate",
        "use_pid", "penalty_initial_value", "budget", "update_penalty_after", "proportional_control_coeff", "derivative_control_coeff",
        "integral_control_coeff", "proportional_cost_ema_alpha", "derivative_cost_ema_alpha", "pid_delay", "penalty_learning_rate", "use_sde",
        "use_curiosity_driven_exploration", "use_lambda_shaping", "sde_sample_freq", "use_null_cost", "cn_path", "cn_obs_select_dim",
        "cn_acs_select_dim", "cn_device", "load_gail", "save_dir", "eval_every_rollouts", "action_noise", "permutation", "env_module",
        "dummy_vec_env", "episode_stats"}
    assert (base["seed"], base["num_threads"], base["n_steps"], base["timesteps"], base["save_dir"]) == (3, 8, 64, 1024, None)
    with_seeds = vars(build_parser().parse_args(argv + ["--seeds", "0", "1", "2", "5"]))
    assert with_seeds.pop("seeds") == [0, 1, 2, 5]
    assert with_seeds == base


def test_seed_configs_give_every_run_its_seed_and_directory(tmp_path):
    import json
    from icrl_amd.cpg import build_parser, seed_configs
    cfg = vars(build_parser().parse_args(["cpg", "--seeds", "4", "7", "--save_dir", str(tmp_path / "out")]))
    runs = seed_configs(cfg)
    assert [r.seed for r in runs] == [4, 7]
    for r in runs:
        assert r.save_dir == str(tmp_path / "out" / f"seed_{r.seed}")
        saved = json.load(open(os.path.join(r.save_dir, "config.json")))
        assert saved["seed"] == r.seed and saved["save_dir"] == r.save_dir and saved["train_env_id"] == cfg["train_env_id"]
    assert [r.save_dir for r in seed_configs(dict(cfg, save_dir=None))] == [None, None]
