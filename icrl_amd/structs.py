"""ctypes mirrors of the plain-C descriptors in include/icrl_hip.h (host structs holding device pointers)."""
import ctypes as C

i32, f64, vp = C.c_int32, C.c_double, C.c_void_p


class EnvT(C.Structure):
    _fields_ = [("n_envs", i32), ("obs_dim", i32), ("act_dim", i32), ("max_steps", i32), ("reward_form", i32),
                ("wall_terminate", i32), ("broken", i32), ("_pad", i32),
                ("B", vp), ("s", vp), ("t_ep", vp), ("step_count", vp), ("key", vp)]


class NormT(C.Structure):
    _fields_ = [("training", i32), ("norm_obs", i32), ("norm_reward", i32), ("norm_cost", i32),
                ("clip_obs", f64), ("clip_reward", f64), ("clip_cost", f64), ("reward_gamma", f64), ("cost_gamma", f64),
                ("epsilon", f64),
                ("obs_mean", vp), ("obs_var", vp), ("obs_count", vp), ("ret_stats", vp), ("cost_stats", vp),
                ("ret", vp), ("cost_ret", vp)]


class PolicyT(C.Structure):
    _fields_ = [("obs_dim", i32), ("act_dim", i32), ("h1", i32), ("h2", i32), ("discrete", i32), ("n_params", i32),
                ("params", vp), ("params_t", vp), ("arch", vp)]      # arch: host int32 array or NULL (include/icrl_hip.h)


class CostNetT(C.Structure):
    _fields_ = [("obs_dim", i32), ("acs_dim", i32), ("in_dim", i32), ("n_hidden", i32), ("h1", i32), ("h2", i32), ("h3", i32), ("h4", i32),
                ("is_discrete", i32), ("n_params", i32),
                ("clip_obs", f64), ("select_dim", vp), ("action_low", vp), ("action_high", vp), ("obs_mean", vp),
                ("obs_var", vp), ("eps", f64), ("params", vp), ("params_t", vp)]


COST_FN = -1      # ICRL_COST_FN: the value of n_hidden that marks an analytic cost
COST_NULL, COST_WALL_BEHIND, COST_WALL_INFRONT, COST_WALL_BOTH, COST_TORQUE, COST_ACTION_EQUALS = range(6)


class CostFnT(C.Structure):
    """icrl_cost_fn_t: an analytic cost; its first four fields alias CostNetT's and it travels through the same pointer arguments."""
    _fields_ = [("obs_dim", i32), ("acs_dim", i32), ("in_dim", i32), ("n_hidden", i32), ("kind", i32), ("index", i32),
                ("lo", f64), ("hi", f64)]


COST_DISC = -2    # ICRL_COST_DISC: the value of n_hidden that marks a discriminator cost


class CostDiscT(C.Structure):
    """icrl_cost_disc_t: a constraint net read as D = zeta (cpg --load_gail); its first four fields alias CostNetT's, `net` is the host
    address of the inner CostNetT, which must outlive every call that takes this descriptor."""
    _fields_ = [("obs_dim", i32), ("acs_dim", i32), ("in_dim", i32), ("n_hidden", i32), ("net", vp)]


COST_REGION = -3  # ICRL_COST_REGION: the value of n_hidden that marks a region cost
REGION_MAX_CLAUSES = REGION_MAX_TERMS = 8
REGION_BOX, REGION_HALFSPACE, REGION_BALL = range(3)
REGION_ANY, REGION_ALL, REGION_SUM = range(3)


class RegionClauseT(C.Structure):
    """icrl_region_clause_t: box (a = lo, b = hi), halfspace (a = w, c = offset) or ball (a = centre, c = radius squared)."""
    _fields_ = [("type", i32), ("negate", i32), ("n_terms", i32), ("_pad", i32), ("col", i32 * REGION_MAX_TERMS),
                ("a", f64 * REGION_MAX_TERMS), ("b", f64 * REGION_MAX_TERMS), ("c", f64)]


class CostRegionT(C.Structure):
    """icrl_cost_region_t: a region cost; its first four fields alias CostNetT's.  `clauses` is the host address of the clause table,
    `d_clauses` the device address of the same bytes; both must outlive every call that takes this descriptor."""
    _fields_ = [("obs_dim", i32), ("acs_dim", i32), ("in_dim", i32), ("n_hidden", i32), ("n_clauses", i32), ("combine", i32),
                ("clauses", vp), ("d_clauses", vp)]


class BufferT(C.Structure):
    _fields_ = [("T", i32), ("N", i32), ("obs_dim", i32), ("act_store", i32),
                ("observations", vp), ("new_observations", vp), ("orig_observations", vp), ("new_orig_observations", vp),
                ("actions", vp), ("dones", vp), ("log_probs", vp), ("rewards", vp), ("reward_values", vp), ("costs", vp),
                ("orig_costs", vp), ("cost_values", vp), ("reward_advantages", vp), ("reward_returns", vp),
                ("cost_advantages", vp), ("cost_returns", vp), ("gae_ws", vp), ("gae_ws_bytes", C.c_longlong)]


class AgentT(C.Structure):
    _fields_ = [("last_obs", vp), ("last_dones", vp), ("raw_rew", vp), ("raw_cost", vp), ("dones", vp),
                ("last_v_r", vp), ("last_v_c", vp), ("act_clipped", vp), ("status", vp), ("xch_ws", vp), ("xch_ws_bytes", C.c_longlong)]


class HostStepT(C.Structure):
    """icrl_host_step_t: the transfer buffers of the rollout over host envs (icrl_host_step)."""
    _fields_ = [("T", i32), ("_pad", i32), ("stage", vp), ("s", vp), ("act_host", vp), ("ws", vp), ("ws_bytes", C.c_longlong)]


class MonitorT(C.Structure):
    """icrl_monitor_t: the raw-reward plane of a rollout, the per-env episode carries and the ring of the last 100 finished episodes."""
    _fields_ = [("raw_rewards", vp), ("ep_ret", vp), ("ep_len", vp), ("win_ret", vp), ("win_len", vp), ("win_state", vp), ("ws", vp),
                ("ws_bytes", C.c_longlong)]


class HostEpisodeT(C.Structure):
    """icrl_host_episode_t: the transfer buffers and outputs of the episode loop over one host env (icrl_host_episode_step)."""
    _fields_ = [("num_envs", i32), ("obs_dim", i32), ("rows", i32), ("deterministic", i32), ("stage", vp), ("act_host", vp),
                ("orig_obs", vp), ("obs", vp), ("actions", vp)]


class PpoHyperT(C.Structure):
    _fields_ = [("batch_size", i32), ("n_epochs", i32), ("use_target_kl", i32), ("_pad", i32),
                ("clip_range", C.c_float), ("ent_coef", C.c_float), ("reward_vf_coef", C.c_float), ("cost_vf_coef", C.c_float),
                ("max_grad_norm", C.c_float), ("target_kl", C.c_float), ("clip_range_reward_vf", C.c_float),
                ("clip_range_cost_vf", C.c_float), ("lr", C.c_float), ("adam_beta1", C.c_float), ("adam_beta2", C.c_float),
                ("adam_eps", C.c_float)]


class CnHyperT(C.Structure):
    _fields_ = [("iterations", i32), ("importance_sampling", i32), ("per_step", i32), ("gail", i32),
                ("reg_coeff", C.c_float), ("eps", C.c_float), ("target_kl_old_new", C.c_float), ("target_kl_new_old", C.c_float),
                ("lr", C.c_float), ("adam_beta1", C.c_float), ("adam_beta2", C.c_float), ("adam_eps", C.c_float)]


# ---- job descriptors of the batched entry points: pointers to the per-run descriptors above (host memory) + device pointers
class RolloutJobT(C.Structure):
    _fields_ = [("env", vp), ("nm", vp), ("pol", vp), ("cn", vp), ("buf", vp), ("ag", vp), ("noise", vp)]


class GaeJobT(C.Structure):
    _fields_ = [(k, vp) for k in ("rewards", "costs", "reward_values", "cost_values", "dones", "last_v_r", "last_v_c", "last_dones",
                                  "adv_r", "adv_c", "ret_r", "ret_c", "ws")] + [("ws_bytes", C.c_longlong)]


class SampleJobT(C.Structure):
    _fields_ = ([(k, vp) for k in ("env", "nm", "pol", "noise", "stream_row0")] + [("total_rows", i32), ("_pad", i32)] +
                [(k, vp) for k in ("orig_obs", "obs", "actions", "ep_rewards", "ep_lengths")])


class ChainJobT(C.Structure):
    """icrl_chain_job_t: one sequential episode loop of icrl_sample_episodes_chain."""
    _fields_ = ([(k, vp) for k in ("env", "nm", "pol", "noise", "base_count")] +
                [("episodes_per_stream", i32), ("deterministic", i32), ("fixed_len", i32), ("_pad", i32)] +
                [(k, vp) for k in ("orig_obs", "obs", "actions", "ep_rewards", "ep_lengths", "exec_steps")])


class CnTrainJobT(C.Structure):
    _fields_ = [("cn", vp), ("exp_avg", vp), ("exp_avg_sq", vp), ("adam_step", vp), ("nominal", vp), ("expert", vp), ("Nn", i32), ("Ne", i32),
                ("ep_offsets", vp), ("row_episode", vp), ("n_ep", i32), ("_pad", i32), ("hp", vp), ("work", vp), ("metrics", vp)]


class CnTrainMbJobT(C.Structure):
    """icrl_cn_train_mb_job_t: CnTrainJobT's fields + the permutation table and the batch size (icrl_cn_train_minibatch_batch)."""
    _fields_ = CnTrainJobT._fields_ + [("perms", vp), ("batch_size", i32), ("_pad2", i32)]


class GailJobT(C.Structure):
    """icrl_gail_job_t: one run's rollout-end work of the GAIL callback (icrl_gail_unnormalize_batch / icrl_gail_relabel_batch)."""
    _fields_ = [("disc", vp), ("true_cost", vp), ("observations", vp), ("actions", vp), ("obs_mean", vp), ("obs_var", vp), ("epsilon", f64),
                ("raw_obs", vp), ("rewards", vp), ("cost_mean", vp), ("rows", i32), ("learn_cost", i32)]


class PpoTrainJobT(C.Structure):
    _fields_ = [(k, vp) for k in ("pol", "exp_avg", "exp_avg_sq", "adam_step", "buf", "perms", "nu", "hp", "stats", "sync_ws")]


def addr(struct):
    """host address of a ctypes struct (for the pointer fields of a job descriptor); the struct must outlive the call."""
    return C.addressof(struct) if struct is not None else None


def p(t):
    """device pointer of a contiguous tensor (or None -> NULL)."""
    if t is None:
        return None
    assert t.is_contiguous()
    return t.data_ptr()

GAE_WS_BYTES = 256 * (256 * 8 + 4) + 64       # ICRL_GAE_WS_BYTES
