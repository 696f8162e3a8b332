"""ActorTwoCriticsPolicy with its parameters in ONE flat float32 HBM buffer.

ref: stable_baselines3/common/policies.py:598-779 (ActorTwoCriticsPolicy), common/torch_layers.py:129-254 (MlpExtractor),
     common/distributions.py:114-192,249-298 (DiagGaussian / Categorical), icrl/utils.py:636-655 (get_net_arch).

Scope: the two-critics MLP policy — an optional shared tanh trunk, then three tanh MLPs (pi / vf / cvf) and a DiagGaussian (Box) or
Categorical (Discrete) head.  Three storage kinds, by architecture:
  * "fast": no trunk, two hidden layers per branch, every width <= 64 (every BASELINE config) — the persistent kernels; narrower
    layers are stored zero-padded to 64;
  * "wide": the same shape with a layer of 65..256 units — generic-shape path, stored zero-padded to a common multiple of 64;
  * "arch": anything else MlpExtractor builds (`-sl` trunk of up to 4 layers, branches of 0..4 layers, widths 1..256) — generic-shape
    path, natural unpadded layout, described to the library by an `arch` array (include/icrl_hip.h: icrl_policy_t).
Parameter initialisation runs on the host with torch-CPU exactly like the reference (same construction / orthogonal-init order, so
the same seed gives the same weights); after that the flat buffer lives on the device and only kernels touch it.
"""
import math
from collections import OrderedDict

import numpy as np
import torch

from . import _lib, spaces
from .structs import PolicyT, p

BRANCHES = ("policy_net", "value_net", "cost_value_net")
HW = 64        # width the fast kernels are built for (HD in csrc/ppo_common.h, MAX_H in csrc/common.h)
HW_MAX = 256   # widest layer of the generic-shape path (csrc/generic.hip: GEN_MAX_H)
DEPTH_MAX = 4  # layers of the shared trunk / of one branch on the generic-shape path (csrc/generic.hip: GEN_MAX_DEPTH)


def state_dict_names(discrete, n_hidden=2, n_shared=0):
    """parameter names in the reference's state_dict order; n_hidden: one depth for the three branches or a (pi, vf, cvf) triple.
    (A gSDE policy has the same names: its `log_std` is a matrix [H, A] instead of a vector [A].)"""
    depths = (n_hidden,) * 3 if isinstance(n_hidden, int) else tuple(n_hidden)
    names = [] if discrete else ["log_std"]
    for k in range(n_shared):
        names += [f"mlp_extractor.shared_net.{2 * k}.weight", f"mlp_extractor.shared_net.{2 * k}.bias"]
    for b, d in zip(BRANCHES, depths):
        for k in range(d):
            names += [f"mlp_extractor.{b}.{2 * k}.weight", f"mlp_extractor.{b}.{2 * k}.bias"]
    for h in ("action_net", "value_net", "cost_value_net"):
        names += [f"{h}.weight", f"{h}.bias"]
    return names


class ActorTwoCriticsPolicy:
    def __init__(self, observation_space, action_space, lr_schedule=None, net_arch=None, log_std_init=0.0,
                 ortho_init=True, optimizer_kwargs=None, device="cuda", use_sde=False):
        self.observation_space, self.action_space = observation_space, action_space
        self.device = torch.device(device)
        self.obs_dim = int(observation_space.shape[0])
        self.discrete = isinstance(action_space, spaces.Discrete)
        self.act_dim = int(action_space.n) if self.discrete else int(action_space.shape[0])
        if net_arch is None:
            net_arch = [dict(pi=[64, 64], vf=[64, 64], cvf=[64, 64])]
        # net_arch = [shared widths..., dict(pi=[...], vf=[...], cvf=[...])] (ref: torch_layers.py:129-254, icrl/utils.py:636-655); a list
        # without the dict is a trunk the three heads read directly
        n_sh = next((i for i, x in enumerate(net_arch) if isinstance(x, dict)), len(net_arch))
        arch = net_arch[n_sh] if n_sh < len(net_arch) else {}
        self.shared = tuple(int(w) for w in net_arch[:n_sh])
        self.layers = {b: tuple(int(w) for w in (arch.get(k) or ())) for b, k in zip(BRANCHES, ("pi", "vf", "cvf"))}
        every = list(self.shared) + [w for b in BRANCHES for w in self.layers[b]]
        if len(self.shared) > DEPTH_MAX or any(len(v) > DEPTH_MAX for v in self.layers.values()) or any(w < 1 or w > HW_MAX for w in every):
            raise NotImplementedError(f"icrl_amd serves net_arch = [shared..., dict(pi=[...], vf=[...], cvf=[...])] with up to {DEPTH_MAX} shared layers, up to "
                                      f"{DEPTH_MAX} layers per branch and 1..{HW_MAX} units per layer; got {net_arch}")
        two = not self.shared and all(len(v) == 2 for v in self.layers.values())
        # logical widths per branch (-pl / -rvl / -cvl).  "fast" / "wide": the device buffers are `hw` wide — 64 when every layer fits the
        # fast kernels, else the widest layer rounded up to a multiple of 64 (the generic-shape path, csrc/generic.hip) — and a narrower
        # layer is stored zero-padded.  Padding units have zero weights in and out and a zero bias, so they output tanh(0) = 0 exactly,
        # receive a zero gradient and keep zero Adam moments: every real parameter sees exactly the arithmetic of the unpadded network
        # (only zeros are added to its dot products).  "arch": natural widths, no padding.
        widest = max(every) if every else 0
        self.kind = ("fast" if widest <= HW else "wide") if two else "arch"
        self.widths = {b: self.layers[b] for b in BRANCHES} if two else None
        self.hw = (HW if widest <= HW else -(-widest // 64) * 64) if two else 0
        self.wide = self.kind != "fast"   # the persistent rollout / sampling / update kernels do not serve this policy
        self.h1 = self.h2 = self.hw
        self.arch = None
        if self.kind == "arch":           # the descriptor icrl_policy_t.arch points at (host memory, kept alive here)
            desc = [len(self.shared), *self.shared]
            for b in BRANCHES:
                desc += [len(self.layers[b]), *self.layers[b]]
            self.arch = np.ascontiguousarray(desc, dtype=np.int32)
        # gSDE (ref: distributions.py:408-601, policies.py:434-441, 671-690 with PPOLagrangian's defaults: full_std, exp, no squashing, no
        # sde_net_arch): log_std is a matrix, logical [H, A] over the policy branch's last layer, STORED [64, A] zero-padded and still first in
        # the flat buffer.  A padded latent unit is exactly 0, so its row adds exactly 0 to every variance, receives a zero gradient and keeps
        # zero Adam moments, as the padding above does.  Served by icrl_policy_forward_sde / icrl_policy_sde_fwd_bwd (csrc/sde.hip) alone.
        self.use_sde = bool(use_sde)
        if self.use_sde:
            if self.discrete:
                raise NotImplementedError("use_sde: gSDE needs a Box action space (the reference's StateDependentNoiseDistribution is continuous)")
            if self.kind != "fast":
                raise NotImplementedError(f"use_sde: gSDE is served for net_arch without a shared trunk, two hidden layers per branch and widths <= {HW} "
                                          f"(the limit of csrc/sde.hip); got {net_arch}")
            if self.obs_dim > 128 or self.act_dim > 16:
                raise NotImplementedError(f"use_sde: gSDE is served up to obs_dim 128 and act_dim 16; got ({self.obs_dim}, {self.act_dim})")
        self.sde_latent = self.layers["policy_net"][-1] if self.use_sde else 0
        self.sde_E0 = self.sde_E = None
        self.optimizer_kwargs = dict(eps=1e-5) if optimizer_kwargs is None else dict(optimizer_kwargs)  # ref: policies.py:357-361
        self.lr_schedule = lr_schedule
        sd = self._init_host(log_std_init, ortho_init)
        self.logical_shapes = OrderedDict((k, tuple(v.shape)) for k, v in sd.items())
        self.shapes = OrderedDict((k, self._physical_shape(k, shp)) for k, shp in self.logical_shapes.items())
        flat = torch.cat([self._pad(k, v).reshape(-1) for k, v in sd.items()]).float()
        self.n_params = flat.numel()
        self.params = flat.to(self.device).contiguous()
        self.params_t = torch.empty_like(self.params)
        # Adam state of policy.optimizer (exp_avg, exp_avg_sq, step) — flat, same layout
        self.exp_avg = torch.zeros_like(self.params)
        self.exp_avg_sq = torch.zeros_like(self.params)
        self.adam_step = 0
        self.prepare()

    def _physical_shape(self, name, shp):
        if name == "log_std" and self.use_sde:
            return (HW, shp[1])
        if name == "log_std" or self.kind == "arch":
            return shp
        if name.startswith("mlp_extractor."):
            first = name.split(".")[2] == "0"
            return ((self.hw, self.obs_dim if first else self.hw) if name.endswith("weight") else (self.hw,))
        return (shp[0], self.hw) if name.endswith("weight") else shp          # heads: [outputs, last hidden]

    def _pad(self, name, t):
        """logical tensor -> device layout (zeros beyond the logical widths)."""
        t = torch.as_tensor(np.asarray(t), dtype=torch.float32) if not torch.is_tensor(t) else t.detach().float().cpu()
        assert tuple(t.shape) == self.logical_shapes[name], (name, tuple(t.shape), self.logical_shapes[name])
        if self.shapes[name] == self.logical_shapes[name]:
            return t
        out = torch.zeros(self.shapes[name])
        out[tuple(slice(0, n) for n in t.shape)] = t
        return out

    def _split(self, flat, pad=False):
        """flat device-layout vector -> OrderedDict of logical tensors (the padding is dropped)."""
        out, off = OrderedDict(), 0
        for k, shp in self.shapes.items():
            n = int(np.prod(shp))
            out[k] = flat[off:off + n].reshape(shp)[tuple(slice(0, m) for m in self.logical_shapes[k])].clone()
            off += n
        return out

    def _init_host(self, log_std_init, ortho_init):
        """construction + init order of ActorTwoCriticsPolicy._build (ref: policies.py:648-714, torch_layers.py:208-226)."""
        Lin = torch.nn.Linear
        shared, last_sh = [], self.obs_dim
        for w in self.shared:             # the trunk is built first, then layer k of pi, vf, cvf back to back (zip_longest)
            shared.append(Lin(last_sh, w)); last_sh = w
        lins = {b: [] for b in BRANCHES}
        last = {b: last_sh for b in BRANCHES}
        for k in range(max(len(v) for v in self.layers.values())):
            for b in BRANCHES:
                if k < len(self.layers[b]):
                    lins[b].append(Lin(last[b], self.layers[b][k]))
                    last[b] = self.layers[b][k]
        heads = OrderedDict(action_net=Lin(last["policy_net"], self.act_dim))
        if self.use_sde:                  # proba_distribution_net draws its first exploration matrices here (sample_weights: two rsamples)
            torch.empty(last["policy_net"], self.act_dim).normal_(); torch.empty(1, last["policy_net"], self.act_dim).normal_()
        heads["value_net"], heads["cost_value_net"] = Lin(last["value_net"], 1), Lin(last["cost_value_net"], 1)
        if ortho_init:                    # module.apply order: shared_net, policy_net, value_net, cost_value_net, then the heads
            for lin in shared + [lin for b in BRANCHES for lin in lins[b]]:
                torch.nn.init.orthogonal_(lin.weight, gain=math.sqrt(2)); lin.bias.data.fill_(0.0)
            for lin, g in zip(heads.values(), (0.01, 1.0, 1.0)):
                torch.nn.init.orthogonal_(lin.weight, gain=g); lin.bias.data.fill_(0.0)
        sd = OrderedDict()
        if not self.discrete:
            sd["log_std"] = (torch.ones(last["policy_net"], self.act_dim) if self.use_sde else torch.ones(self.act_dim)) * log_std_init
        for k, lin in enumerate(shared):
            sd[f"mlp_extractor.shared_net.{2 * k}.weight"] = lin.weight.data
            sd[f"mlp_extractor.shared_net.{2 * k}.bias"] = lin.bias.data
        for b in BRANCHES:
            for k, lin in enumerate(lins[b]):
                sd[f"mlp_extractor.{b}.{2 * k}.weight"] = lin.weight.data
                sd[f"mlp_extractor.{b}.{2 * k}.bias"] = lin.bias.data
        for name, lin in heads.items():
            sd[f"{name}.weight"], sd[f"{name}.bias"] = lin.weight.data, lin.bias.data
        return sd

    # ---- C-ABI descriptor -------------------------------------------------------------------------------------
    def struct(self, sde=False):
        """sde: the caller is one of the gSDE entry points' wrappers.  Every other call site builds the descriptor for an entry point that
        reads the diagonal layout: a gSDE policy is refused here, before any device call."""
        if self.use_sde and not sde:
            raise NotImplementedError("use_sde: a gSDE policy (log_std [H, A]) is served by icrl_policy_forward_sde / icrl_policy_sde_fwd_bwd alone — the per-step "
                                      "rollout and the fine-grained update; the fused launches and the other entry points read the diagonal layout")
        return PolicyT(self.obs_dim, self.act_dim, self.h1, self.h2, int(self.discrete), self.n_params, p(self.params), p(self.params_t),
                       None if self.arch is None else self.arch.ctypes.data)

    @property
    def row_floats(self):
        """outputs of every layer of one row: the `row_floats` argument of ICRL_PPO_GENERIC_BYTES (include/icrl_hip.h)."""
        if self.kind == "arch":
            return sum(self.shared) + sum(sum(v) for v in self.layers.values()) + self.act_dim + 2
        return 6 * self.hw + self.act_dim + 2

    def prepare(self):
        """refresh the transposed weight copy the rollout kernels read (call after params change)."""
        if self.device.type == "cpu":      # storage only (state-dict handling on a host without a device): nothing reads a transposed copy there
            return
        if self.use_sde:      # the network alone, as a diagonal-layout descriptor whose log_std slot is the matrix's last row (include/icrl_hip.h)
            skip = (HW - 1) * self.act_dim
            s = PolicyT(self.obs_dim, self.act_dim, self.h1, self.h2, 0, self.n_params - skip, p(self.params[skip:]), p(self.params_t[skip:]), None)
        else:
            s = self.struct()
        _lib.check(_lib.lib().icrl_policy_prepare(_lib.byref(s), _lib.current_stream()), "icrl_policy_prepare")

    # ---- state dict (reference names; ref: expert_data/*/files/best_model.zip:policy.pth) --------------------------
    def state_dict(self):
        return self._split(self.params.detach().cpu())

    def check_state_dict_kind(self, sd, where="state dict"):
        """raise, with both kinds named, when `sd` holds the other action distribution's log_std (a vector [A]: diagonal Gaussian; a matrix [H, A]: gSDE)."""
        ls = sd.get("log_std") if hasattr(sd, "get") else None
        if ls is None or self.discrete:
            return
        theirs = np.ndim(ls) == 2
        if theirs != self.use_sde:
            kind = lambda sde: "a gSDE policy (use_sde=True, log_std [H, A])" if sde else "a diagonal-Gaussian policy (use_sde=False, log_std [A])"
            raise ValueError(f"{where} holds {kind(theirs)} with log_std of shape {tuple(np.shape(ls))}; this agent has {kind(self.use_sde)}. Build or load the "
                             f"agent with use_sde={theirs}.")

    def load_state_dict(self, sd):
        self.check_state_dict_kind(sd)
        flat = torch.cat([self._pad(k, sd[k]).reshape(-1) for k in self.shapes])
        assert flat.numel() == self.n_params
        self.params.copy_(flat.to(self.device))
        self.prepare()

    def optimizer_state_dict(self, lr=None, eps=1e-5):
        """policy.optimizer.state_dict() in torch.optim.Adam's own layout (what SB3 stores as policy.optimizer.pth):
        parameters numbered in state_dict order, per-parameter step / exp_avg / exp_avg_sq."""
        m, v = self._split(self.exp_avg.detach().cpu()), self._split(self.exp_avg_sq.detach().cpu())
        state = {i: dict(step=torch.tensor(float(self.adam_step)), exp_avg=m[k], exp_avg_sq=v[k]) for i, k in enumerate(self.shapes)}
        group = dict(lr=lr, betas=(0.9, 0.999), eps=eps, weight_decay=0, amsgrad=False, params=list(range(len(self.shapes))))
        return dict(state=state if self.adam_step > 0 else {}, param_groups=[group])

    def load_optimizer_state_dict(self, osd):
        state = osd.get("state", {})
        if not state:
            self.exp_avg.zero_(); self.exp_avg_sq.zero_(); self.adam_step = 0
            return
        # parameter order = param_groups[0]["params"]: 0..n-1 in current torch, the parameters' id()s in the torch 1.5 files the
        # reference wrote (expert_data/*/files/best_model.zip); both follow policy.parameters() = state_dict order
        keys = [k for g in osd.get("param_groups", []) for k in g["params"]] or sorted(state)
        assert len(keys) == len(self.shapes), "optimizer state does not match the policy's parameter list"
        m = torch.cat([self._pad(name, state[k]["exp_avg"]).reshape(-1) for name, k in zip(self.shapes, keys)])
        v = torch.cat([self._pad(name, state[k]["exp_avg_sq"]).reshape(-1) for name, k in zip(self.shapes, keys)])
        assert m.numel() == self.exp_avg.numel()
        self.exp_avg.copy_(m.to(self.device)); self.exp_avg_sq.copy_(v.to(self.device))
        self.adam_step = int(float(state[keys[0]]["step"]))

    @property
    def log_std(self):
        if self.use_sde:      # the real [H, A] block (a view)
            return self.params[:HW * self.act_dim].view(HW, self.act_dim)[:self.sde_latent]
        return None if self.discrete else self.params[:self.act_dim]

    # ---- gSDE ---------------------------------------------------------------------------------------------------------
    def _sde_normals(self, streams):
        """shape -> standard normals on the device: `streams.sde_noise(shape)` where the streams object has it, else torch's device generator"""
        dev = self.device
        draw = getattr(streams, "sde_noise", None) if streams is not None else None
        def normals(shape):
            if draw is None:
                return torch.randn(shape, device=dev)
            z = draw(shape)
            z = z if torch.is_tensor(z) else torch.as_tensor(np.asarray(z, np.float32))
            return z.to(device=dev, dtype=torch.float32).reshape(shape)
        return normals

    def reset_noise(self, n_envs=1, streams=None):
        """ref: policies.py:434-441 -> distributions.py:483-496 — draw the exploration matrices E0 [H, A] and E [n_envs, H, A] from
        Normal(0, exp(log_std)); kept on the device in the stored [64, A] shape (zero rows beyond H).  `streams.sde_noise(shape)`, where the
        agent's streams object has it, gives the standard normals (teacher forcing); otherwise torch draws them on the device."""
        assert self.use_sde, "reset_noise: not a gSDE policy"
        H, A = self.sde_latent, self.act_dim
        normals = self._sde_normals(streams)
        std = torch.exp(self.log_std)
        self.set_noise(normals((H, A)) * std, normals((int(n_envs), H, A)) * std)

    def set_noise(self, E0, E):
        """install exploration matrices given in their logical shapes [H, A] and [n, H, A]."""
        H, A, dev = self.sde_latent, self.act_dim, self.device
        E0 = torch.as_tensor(E0, device=dev).float().reshape(H, A)
        E = torch.as_tensor(E, device=dev).float().reshape(-1, H, A)
        self.sde_E0 = torch.zeros(HW, A, device=dev); self.sde_E0[:H] = E0
        self.sde_E = torch.zeros(E.shape[0], HW, A, device=dev); self.sde_E[:, :H] = E

    @staticmethod
    def noise_schedule_draws(T, sample_freq):
        """how many of a rollout's draws get used: one per started block of sample_freq steps, or the one at the rollout's start."""
        T, sf = int(T), int(sample_freq)
        return -(-T // sf) if sf > 0 else 1

    def noise_schedule(self, n_envs, T, sample_freq, streams=None):
        """The exploration matrices of a whole rollout, drawn before its first step (icrl_rollout_collect_sde): exactly the reset_noise calls the
        per-step loop makes, in its order — one at the rollout's start, then one at every t with sample_freq > 0 and t % sample_freq == 0, t = 0
        included — so the generator (or `streams.sde_noise`) ends where the loop leaves it, and sde_E0 / sde_E hold the last draw as they do
        after the loop.  Returns the matrices that get used, [D, n_envs, 64, A] with D = noise_schedule_draws(T, sample_freq): step t reads
        draw t // sample_freq (draw 0 when sample_freq <= 0).  One env: the E0 of each draw, which _forward_sde picks for a single row."""
        assert self.use_sde, "noise_schedule: not a gSDE policy"
        n_envs, T, sf = int(n_envs), int(T), int(sample_freq)
        H, A, dev = self.sde_latent, self.act_dim, self.device
        normals = self._sde_normals(streams)
        D = self.noise_schedule_draws(T, sf)
        # the draws themselves stay one call per tensor, in reset_noise's order (their values depend on it); everything behind them — the
        # scaling by exp(log_std), the padding to 64 rows — is done once for the whole schedule (log_std does not change during a rollout)
        z0 = z = None
        used = []
        for d in range(1 + (D if sf > 0 else 0)):
            z0, z = normals((H, A)), normals((n_envs, H, A))
            if sf <= 0 or d >= 1:      # (with a cadence, the rollout's own draw is replaced at step 0 before any step reads it)
                used.append(z0.unsqueeze(0) if n_envs == 1 else z)
        std = torch.exp(self.log_std)
        sched = torch.zeros(D, n_envs, HW, A, device=dev)
        sched[:, :, :H] = torch.stack(used) * std
        self.set_noise(z0 * std, z * std)
        return sched

    def _forward_sde(self, obs, deterministic, clip):
        """icrl_policy_forward_sde with the matrices get_noise picks (distributions.py:577-587): E0 for one row or when the row count is not
        the number of per-env matrices, else row i's own."""
        dev = self.device
        n = obs.shape[0]
        expl, stride = None, 0
        if not deterministic:
            if self.sde_E is None:
                self.reset_noise(1)
            if n == 1 or n != self.sde_E.shape[0]:
                expl = self.sde_E0
            else:
                expl, stride = self.sde_E, HW * self.act_dim
        actions = torch.empty(n, self.act_dim, device=dev); clipped = torch.empty(n, self.act_dim, device=dev)
        v_r, v_c, lp = (torch.empty(n, device=dev) for _ in range(3))
        lo = hi = None
        if clip:
            lo = torch.as_tensor(self.action_space.low, device=dev).float().contiguous()
            hi = torch.as_tensor(self.action_space.high, device=dev).float().contiguous()
        s = self.struct(sde=True)
        _lib.check(_lib.lib().icrl_policy_forward_sde(_lib.byref(s), p(obs), p(expl), stride, n, int(deterministic), p(lo), p(hi), p(actions), p(clipped),
                                                      p(v_r), p(v_c), p(lp), _lib.current_stream()), "icrl_policy_forward_sde")
        self.last_clipped = clipped
        return actions, v_r.reshape(-1, 1), v_c.reshape(-1, 1), lp

    # ---- inference ------------------------------------------------------------------------------------------------
    def forward(self, obs, deterministic=False, noise=None, clip=True):
        """ref: policies.py:716-731.  obs: [N,obs] (device float64 or anything convertible).  noise: [N,act] standard normals
        ([N] uniforms when discrete); None draws them on the device.  Returns (actions, reward_values, cost_values, log_prob)
        plus ``self.last_clipped`` = actions clipped to the action box."""
        dev = self.device
        obs = torch.as_tensor(obs, device=dev).to(torch.float64).reshape(-1, self.obs_dim).contiguous()
        n = obs.shape[0]
        if self.use_sde:      # (`noise` has no meaning here: the exploration matrices are the policy's state, reset_noise / set_noise)
            return self._forward_sde(obs, deterministic, clip)
        if noise is None and not deterministic:
            noise = torch.rand(n, device=dev) if self.discrete else torch.randn(n, self.act_dim, device=dev)
        if noise is not None:
            noise = torch.as_tensor(noise, device=dev).float().contiguous()
        a_store = 1 if self.discrete else self.act_dim
        actions = torch.empty(n, a_store, device=dev); clipped = torch.empty(n, a_store, device=dev)
        v_r, v_c, lp = (torch.empty(n, device=dev) for _ in range(3))
        lo = hi = None
        if clip and not self.discrete:
            lo = torch.as_tensor(self.action_space.low, device=dev).float().contiguous()
            hi = torch.as_tensor(self.action_space.high, device=dev).float().contiguous()
        s = self.struct()
        _lib.check(_lib.lib().icrl_policy_forward(_lib.byref(s), p(obs), p(noise), n, int(deterministic), p(lo), p(hi),
                                                  p(actions), p(clipped), p(v_r), p(v_c), p(lp), _lib.current_stream()),
                   "icrl_policy_forward")
        self.last_clipped = clipped
        return actions, v_r.reshape(-1, 1), v_c.reshape(-1, 1), lp

    def predict(self, observation, state=None, mask=None, deterministic=False, noise=None):
        """ref: policies.py:215-280 — sampled (or mode) action clipped to the action box; returns (actions, state)."""
        self.forward(observation, deterministic, noise)
        return self.last_clipped, state

    def evaluate_actions(self, obs, actions):
        """ref: policies.py:752-767 -> (reward_values, cost_values, log_prob, entropy); device tensors."""
        dev = self.device
        obs = torch.as_tensor(obs, device=dev).to(torch.float64).reshape(-1, self.obs_dim).contiguous()
        a_store = 1 if self.discrete else self.act_dim
        actions = torch.as_tensor(actions, device=dev).to(torch.float32).reshape(-1, a_store).contiguous()
        n = obs.shape[0]
        v_r, v_c, lp, ent = (torch.empty(n, device=dev) for _ in range(4))
        if self.use_sde:      # the update's own kernel, forward only (float64 rounded once; reads `params`)
            s, obs32 = self.struct(sde=True), obs.float().contiguous()
            _lib.check(_lib.lib().icrl_policy_sde_fwd_bwd(_lib.byref(s), p(obs32), p(actions), n, None, None, None, None, p(v_r), p(v_c), p(lp), p(ent), None,
                                                          None, 0, _lib.current_stream()), "icrl_policy_sde_fwd_bwd")
            return v_r.reshape(-1, 1), v_c.reshape(-1, 1), lp, ent
        s = self.struct()
        _lib.check(_lib.lib().icrl_policy_evaluate(_lib.byref(s), p(obs), p(actions), n, p(v_r), p(v_c), p(lp), p(ent),
                                                   _lib.current_stream()), "icrl_policy_evaluate")
        return v_r.reshape(-1, 1), v_c.reshape(-1, 1), lp, ent
