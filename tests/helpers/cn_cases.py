"""Constraint-net update (csrc/cn_train.hip through ConstraintNet.train / prepare_data / cost_function) at the weight layouts, loss forms
and inputs the README runs use, and the conditions every test asserts FROM THE ORACLE ALONE before it looks at a kernel.

At the settings of tests/test_cn_train_gpu.py (four equal episodes or per-step weights, regularizer 0.5 / 0.6, raw observations,
continuous actions, default select_dim, a constant learning rate, one call) a wrong row -> episode map, a second pass over the episodes
that is never taken, a BCE form that keeps the regulariser, a normalisation without epsilon, a one-hot off by one or an Adam step that
forgets the carried count all pass.  A case here is a keyword set; `run(name)` builds the oracle's CostNet + torch.optim.Adam(eps=1e-5),
runs oracle.cn.cn_train with its trace once (cached, shared by the CPU condition file and the GPU parity file, never modified) and
returns data, initial weights and, per train() call, the metrics, the trace, the weights, both Adam moments and the step count.
`product(res)` builds the product's ConstraintNet from the SAME keywords and initial weights.
"""
from collections import OrderedDict

import numpy as np
import torch

from oracle import cn as o_cn, nets as o_nets

# row layouts of the nominal set (episode lengths).  R22: more than 16 episodes (cn_finalize_body's second pass), lengths of 1, one
# under / at / over a wave, over two and three waves, 1082 rows = 16 x 64 + 58 (ragged last block); with 300 expert rows a ragged 44
R22 = [1, 63, 64, 65, 130, 7, 2, 200, 33, 1, 90, 5, 64, 128, 17, 3, 50, 11, 70, 29, 8, 41]
ONE = [300]                      # a single episode: normed = prod / (prod + eps)
R17 = [1] * 16 + [100]           # the seventeenth episode, the only long one, is the second pass's
LAYOUTS = dict(R22=R22, ONE=ONE, R17=R17)

RTOL, ATOL = 3e-3, 3e-4          # the bound of tests/test_cn_train_gpu.py::test_cn_train_vs_oracle (metrics and weights)
MOMENT_ATOL_SHARE = 0.01         # a moment tensor's atol: at most this share of its largest |reference| entry (and never above ATOL)
COST_RTOL, COST_ATOL = 2e-5, 2e-6
SHARE = (0.05, 0.70)             # share of a clipped plane's entries AT each bound

DEFAULT = dict(obs_dim=18, acs_dim=6, hidden=[20], layout="R22", Ne=300, discrete=False, acs_1d=False, obs_select_dim=None,
               acs_select_dim=None, clip_obs=20.0, bounded=True, eps=1e-5, reg=0.0, nis=False, psis=False, gail=False, tk=(-1, -1),
               batch_size=None, clr=0.003, aclr=None, n_iters=10, iters=5, obs_scale=1.0, obs_shift=0.0, acs_range=1.2, stats=None,
               seed=0, calls=None, stop=None, weights=False, clips=False, builder=None)

NORM = dict(obs_scale=3.0, obs_shift=0.4, stats=(0.3, 2.0), clip_obs=1.5, eps=1e-3, obs_select_dim=[0, 3, 17], acs_select_dim=[18, 20, 23],
            acs_range=1.6, clips=True)
DISCRETE = dict(obs_dim=2, bounded=False, discrete=True)

CASES = OrderedDict()
# (a) weight layouts, full batch, per-episode weights
for _lay in ("R22", "ONE", "R17"):
    for _reg in (0.0, 0.5):
        CASES[f"layout/{_lay}-reg{_reg}"] = dict(layout=_lay, reg=_reg, iters=6, weights=_lay != "ONE", clr=0.01 if _lay == "R17" else 0.003)
for _reg in (0.0, 0.5):
    CASES[f"layout/R22-wide-reg{_reg}"] = dict(layout="R22", reg=_reg, hidden=[128, 128], iters=4, clr=0.001, weights=True)
# (b) loss forms, full batch
CASES["form/nis"] = dict(nis=True, reg=0.5)
CASES["form/gail-nis"] = dict(nis=True, gail=True, reg=0.5)
CASES["form/psis-reg0"] = dict(psis=True, reg=0.0)
# (c) input variants, 3 iterations of train
CASES["input/norm"] = dict(NORM, iters=3, reg=0.5)
CASES["input/noclip"] = dict(clip_obs=None, bounded=False, obs_scale=3.0, acs_range=1.6, iters=3, reg=0.5)
CASES["input/discrete2"] = dict(DISCRETE, acs_dim=2, acs_select_dim=[2, 3], iters=3, weights=True)
CASES["input/discrete5-1d"] = dict(DISCRETE, acs_dim=5, acs_select_dim=[2, 3, 4, 5, 6], acs_1d=True, iters=3, weights=True)
CASES["input/select"] = dict(obs_select_dim=[1, 4, 16], acs_select_dim=[19, 22], iters=3, reg=0.5)
CASES["input/obs-only"] = dict(acs_select_dim=[-1], iters=3, reg=0.5)
CASES["input/acs-only"] = dict(obs_select_dim=[-1], acs_select_dim=[18, 19, 20, 21, 22, 23], iters=3, reg=0.5)
CASES["input/default-quirk"] = dict(iters=3, reg=0.5)       # select_dim = range(18) + range(6): the leading observation columns twice
# (d) state across calls: -aclr 0.9 gives every call another learning rate, -cn other statistics; the second call stops at k > 0
CASES["state/three-calls"] = dict(NORM, clr=0.01, aclr=0.9, n_iters=10, reg=0.5, calls=[
    dict(iters=4, progress=1.0, stats=(0.3, 2.0)),
    dict(iters=5, progress=0.7, stats=(0.1, 3.0), stop=dict(direction="on", target=2)),
    dict(iters=4, progress=0.4, stats=(-0.2, 1.2))])
# (e) early stop (thresholds from the oracle's own KLs: see _stop_thresholds)
# At lr 0.0003 both KLs of R22 grow monotonically (Adam's first steps at larger rates overshoot and come back: the KLs peak at iteration 1),
# so half the KL of iteration 3 is first exceeded at iteration 2.
CASES["stop/old-new"] = dict(clr=0.0003, iters=6, stop=dict(direction="on", target=3))
CASES["stop/new-old"] = dict(clr=0.0003, iters=6, stop=dict(direction="no", target=3))
CASES["stop/never"] = dict(clr=0.03, iters=6, stop=dict(direction="never"))
CASES["stop/last"] = dict(clr=0.0003, iters=5, stop=dict(direction="no", target=4, midpoint=True))
CASES["stop/readme"] = dict(clr=0.01, reg=0.5, iters=6, tk=(10, 2.5), stop=dict(direction="readme", target=2))      # -ctkon 10 -ctkno 2.5
# (f) minibatch mode, recorded permutations.  (Per-episode weights on R22 at lr 0.003 with observations scaled by 3 and hidden [64] x 3
# overflow the episode products by iteration 3: these stay at lr 0.001 and unit scale, and the finiteness condition holds them there.)
CASES["mb/episode-R22"] = dict(batch_size=64, clr=0.001, iters=4, weights=True)                          # Nn 1082 > Ne 300: 4 x 64 + 44
CASES["mb/episode-R17-tail1"] = dict(layout="R17", batch_size=23, clr=0.002, iters=4, weights=True)      # Nn 116 < Ne 300: 5 x 23 + 1
CASES["mb/psis-wide"] = dict(hidden=[128, 128], psis=True, batch_size=64, clr=0.001, iters=3, reg=0.5)
CASES["mb/gail-3layers"] = dict(hidden=[64, 48, 64], nis=True, gail=True, batch_size=64, clr=0.001, iters=3, reg=0.5)
CASES["mb/4layers"] = dict(hidden=[24, 20, 16, 12], psis=True, batch_size=100, clr=0.001, iters=3, reg=0.5)   # 100 divides 300
CASES["mb/one-batch"] = dict(layout="R17", batch_size=512, clr=0.002, iters=4, weights=True)             # batch_size > min(Nn, Ne) = 116
# (g) the three runs of one batched launch: layout/R22-reg0.5, form/nis, form/gail-nis (one shape, three forms)
BATCHED = ("layout/R22-reg0.5", "form/nis", "form/gail-nis")
# (h) saturated predictions: one iteration of each form
CASES["sat/gail"] = dict(builder="sat", nis=True, gail=True, iters=1, clr=0.01, layout=None)
CASES["sat/icrl"] = dict(builder="sat", reg=0.5, iters=1, clr=0.01, layout=None)

INPUT_VARIANTS = [k for k in CASES if k.startswith("input/")]
SAT_HIGH, SAT_LOW, SAT_MID, SAT_ROWS = 30.0, -120.0, 12.0, 10


def spec(name):
    unknown = set(CASES[name]) - set(DEFAULT)
    assert not unknown, unknown
    return {**DEFAULT, **CASES[name], "name": name}


def lr_of(sp, progress):
    """-clr / -aclr: ref icrl.py — lr = aclr ** (n_iters * (1 - progress_remaining)) * clr; a constant without -aclr."""
    return float(sp["clr"]) if sp["aclr"] is None else float(sp["aclr"] ** (sp["n_iters"] * (1.0 - progress)) * sp["clr"])


def calls_of(sp):
    calls = sp["calls"] or [dict(iters=sp["iters"], progress=1.0, stats=sp["stats"], stop=sp["stop"])]
    return [dict(dict(stop=None, tk=tuple(sp["tk"])), **c) for c in calls]


def stats_arrays(sp, stats):
    if stats is None:
        return None, None
    return np.full(sp["obs_dim"], stats[0], np.float64), np.full(sp["obs_dim"], stats[1], np.float64)


def make_data(sp):
    rng = np.random.RandomState(sp["seed"] + 17)
    lengths = np.array(LAYOUTS[sp["layout"]])
    Nn, Ne, od, ad = int(lengths.sum()), sp["Ne"], sp["obs_dim"], sp["acs_dim"]
    exp_obs = rng.randn(Ne, od) * sp["obs_scale"] + sp["obs_shift"]
    nom_obs = rng.randn(Nn, od) * 1.5 * sp["obs_scale"] + sp["obs_shift"]
    if sp["discrete"]:
        shape = (lambda n: (n,)) if sp["acs_1d"] else (lambda n: (n, 1))
        exp_acs = rng.randint(0, ad, Ne).astype(np.float32).reshape(shape(Ne))
        nom_acs = rng.randint(0, ad, Nn).astype(np.float32).reshape(shape(Nn))
    else:
        exp_acs = rng.uniform(-sp["acs_range"], sp["acs_range"], (Ne, ad)).astype(np.float32)
        nom_acs = rng.uniform(-sp["acs_range"], sp["acs_range"], (Nn, ad)).astype(np.float32)
    return dict(nom_obs=nom_obs, nom_acs=nom_acs, exp_obs=exp_obs, exp_acs=exp_acs, lengths=lengths)


def oracle_net(sp, stats=None, seed_shift=1):
    torch.manual_seed(sp["seed"] + seed_shift)
    lo = -np.ones(sp["acs_dim"], np.float32) if sp["bounded"] else None
    net = o_nets.CostNet(sp["obs_dim"], sp["acs_dim"], sp["hidden"], sp["discrete"], sp["obs_select_dim"], sp["acs_select_dim"],
                         sp["clip_obs"], lo, None if lo is None else -lo, sp["eps"])
    net.obs_mean, net.obs_var = stats_arrays(sp, stats)
    return net


def logits(net, x):
    """the pre-sigmoid output of an oracle CostNet (CostNet.forward without its last line)."""
    import torch.nn.functional as F
    with torch.no_grad():
        for i in range(net.n_layers):
            x = F.linear(x, net.params[f"{2 * i}.weight"], net.params[f"{2 * i}.bias"])
            if i < net.n_layers - 1:
                x = torch.relu(x)
    return x.numpy().reshape(-1)


def make_saturated(sp):
    """Rows and an output layer for which, BY THE ORACLE'S LOGITS, each set has >= SAT_ROWS rows at logit >= 30 (zeta exactly 1.0f),
    >= SAT_ROWS at logit <= -120 (zeta exactly 0, in torch and with expf), and no row in (12, 30) or (-120, -12), where expf, denormals
    and the -100 clamp of BCELoss legitimately differ.  Rows are picked from a pool by the initial net's logit z; the output layer
    becomes s * (z - c): the top rows land above 33, the bottom rows below -125, the rest within +-10."""
    rng = np.random.RandomState(sp["seed"] + 29)
    od, ad, pool = sp["obs_dim"], sp["acs_dim"], 6000
    obs, acs = rng.randn(pool, od) * 1.5, rng.uniform(-1.2, 1.2, (pool, ad)).astype(np.float32)
    net = oracle_net(sp)
    z = logits(net, net.prepare(obs, acs))
    order = np.argsort(z)
    n_sat = 2 * (SAT_ROWS + 2)
    low, high = order[:n_sat], order[-n_sat:]
    zb, zt = z[low].max(), z[high].min()
    s = (33.0 + 125.0) / (zt - zb)
    c = zb + 125.0 / s
    mid = np.nonzero(np.abs(z - c) <= 10.0 / s)[0]
    assert len(mid) >= 160, len(mid)
    mid = mid[:220]
    k = 2 * (sp["hidden"] and len(sp["hidden"]))
    sd = net.state_dict()
    sd[f"{k}.bias"] = (sd[f"{k}.bias"] - float(c)) * float(s)
    sd[f"{k}.weight"] = sd[f"{k}.weight"] * float(s)
    nom = np.concatenate([low[0::2], mid[0::2], high[0::2]])
    exp = np.concatenate([high[1::2], mid[1::2], low[1::2]])
    lengths = np.array([len(low[0::2]), 40, len(nom) - len(low[0::2]) - 40])
    return dict(nom_obs=obs[nom], nom_acs=acs[nom], exp_obs=obs[exp], exp_acs=acs[exp], lengths=lengths), sd


class _Recorded:
    """np.random's place in oracle.cn.cn_train: hands out the recorded permutations in order."""
    def __init__(self, perms):
        self.perms, self.k = perms, 0

    def permutation(self, size):
        out = self.perms[self.k]
        assert len(out) == size
        self.k += 1
        return out


def _oracle_calls(sp, data, w0, calls):
    """the oracle over the calls of a case (one net, one optimiser): a list with, per call, metrics `om`, `trace`, `sd`, both moments,
    `step`, `perms`, the prepared rows and `lr`."""
    net = oracle_net(sp)
    net.load_state_dict(w0)
    opt = torch.optim.Adam(net.parameters(), lr=sp["clr"], eps=1e-5)
    out = []
    size = min(len(data["nom_obs"]), len(data["exp_obs"]))
    for ci, c in enumerate(calls):
        lr = lr_of(sp, c["progress"])
        for g in opt.param_groups:
            g["lr"] = lr
        net.obs_mean, net.obs_var = stats_arrays(sp, c["stats"])
        nominal, expert = net.prepare(data["nom_obs"], data["nom_acs"]), net.prepare(data["exp_obs"], data["exp_acs"])
        perms = None
        if sp["batch_size"] is not None:
            prng = np.random.RandomState(sp["seed"] + 100 + ci)
            perms = np.stack([prng.permutation(size) for _ in range(c["iters"])])
        trace = []
        om = o_cn.cn_train(net, opt, c["iters"], nominal, expert, data["lengths"], reg_coeff=sp["reg"], importance_sampling=not sp["nis"],
                           per_step=sp["psis"], target_kl_old_new=c["tk"][0], target_kl_new_old=c["tk"][1], eps=sp["eps"], gail=sp["gail"],
                           batch_size=sp["batch_size"], factored=True, rng=_Recorded(perms), trace=trace)
        state = [opt.state[p] for p in net.parameters()]
        out.append(dict(om=om, trace=trace, sd=net.state_dict(), lr=lr, perms=perms, nominal=nominal, expert=expert, call=c,
                        exp_avg=OrderedDict((k, s["exp_avg"].clone()) for k, s in zip(net.params, state)),
                        exp_avg_sq=OrderedDict((k, s["exp_avg_sq"].clone()) for k, s in zip(net.params, state)),
                        step=int(state[0]["step"])))
    return out


def _stop_thresholds(stop, trace):
    """(target_kl_old_new, target_kl_new_old, stated iteration) of an early-stop case from the KLs of the oracle's run WITHOUT thresholds:
    the stopping direction gets half its KL at the target iteration (midpoint: the mean of the target's and the previous iteration's, for
    a stop at an iteration the half would put earlier); the other direction -1 ("on") or twice its largest |KL| + 1 ("no").  The stated
    iteration is the first whose KL exceeds the threshold, again by the oracle."""
    on = np.array([t["kl_old_new"] for t in trace])
    no = np.array([t["kl_new_old"] for t in trace])
    d = stop["direction"]
    if d == "never":
        return -1, -1, None
    if d == "readme":
        return 10, 2.5, stop["target"]
    kl, k = (on, no)[d == "no"], stop["target"]
    thr = 0.5 * (kl[k] + kl[k - 1]) if stop.get("midpoint") else 0.5 * kl[k]
    assert thr > 0, (d, kl)
    stated = int(np.nonzero(kl > thr)[0][0])
    return (float(thr), -1, stated) if d == "on" else (2.0 * float(np.abs(on).max()) + 1.0, float(thr), stated)


_RUNS = {}


def run(name):
    """the oracle's side of a case, computed once: dict(spec, data, w0, calls=[...], stated=[...])."""
    if name in _RUNS:
        return _RUNS[name]
    sp = spec(name)
    if sp["builder"] == "sat":
        data, w0 = make_saturated(sp)
    else:
        data, w0 = make_data(sp), oracle_net(sp).state_dict()
    calls, stated = calls_of(sp), []
    if any(c["stop"] for c in calls):
        # thresholds of a stopping call come from a run of the same calls in which that call (and every later one) has none
        for ci, c in enumerate(calls):
            if c["stop"] is None:
                stated.append(None)
                continue
            probe = _oracle_calls(sp, data, w0, [dict(x, tk=(-1, -1)) if i >= ci else x for i, x in enumerate(calls)][:ci + 1])
            tk_on, tk_no, st = _stop_thresholds(c["stop"], probe[ci]["trace"])
            calls[ci] = dict(c, tk=(tk_on, tk_no))
            stated.append(st)
    else:
        stated = [None] * len(calls)
    res = dict(spec=sp, data=data, w0=w0, calls=_oracle_calls(sp, data, w0, calls), stated=stated)
    _RUNS[name] = res
    return res


# ---- the conditions, from the oracle alone ------------------------------------------------------------------------------------------
def share_at(x, bound):
    x = np.asarray(x)
    return float(np.mean(x == np.asarray(bound, x.dtype)))


def compared_numbers(call):
    """every number of a call that a parity test compares."""
    out = [float(v) for v in call["om"].values()]
    for t in call["trace"]:
        out += [t[k] for k in ("kl_old_new", "kl_new_old", "is_min", "is_max", "is_mean") if t[k] is not None]
        out += [] if t["prod"] is None else list(t["prod"])
        for s in t["steps"]:
            out += list(s.values())
    for d in (call["sd"], call["exp_avg"], call["exp_avg_sq"]):
        for v in d.values():
            out += list(v.numpy().reshape(-1))
    return np.asarray(out, np.float64)


def check_conditions(res):
    """asserts the input conditions of a case on res = run(name); nothing here comes from the code under test."""
    sp, n_cond = res["spec"], 0
    for ci, call in enumerate(res["calls"]):
        c, trace = call["call"], call["trace"]
        assert np.isfinite(compared_numbers(call)).all(), (sp["name"], ci)
        expected_steps = 1 if sp["batch_size"] is None else -(-min(len(call["nominal"]), len(call["expert"])) // sp["batch_size"])
        assert all(len(t["steps"]) == (0 if t["stopped"] else expected_steps) for t in trace)
        assert call["step"] == sum(len(t["steps"]) for t in trace) + (res["calls"][ci - 1]["step"] if ci else 0)
        if sp["weights"]:
            # per-episode weights are meant to matter: from iteration 1 on (at iteration 0 every ratio is 1) they spread by >= 2x, >= 3 distinct
            assert not sp["psis"] and not sp["nis"] and len(trace) >= 3
            for t in trace[1:]:
                assert t["is_max"] >= 2.0 * max(t["is_min"], 0.0) and t["is_max"] > 0, (sp["name"], t["itr"], t["is_min"], t["is_max"])
                assert len(np.unique(t["prod"])) >= 3
            n_cond += 1
        if sp["clips"]:
            x = call["nominal"].numpy()
            n_obs = len(sp["obs_select_dim"])
            for side in (1.0, -1.0):
                s_obs, s_acs = share_at(x[:, :n_obs], side * sp["clip_obs"]), share_at(x[:, n_obs:], side)
                assert SHARE[0] <= s_obs <= SHARE[1] and SHARE[0] <= s_acs <= SHARE[1], (sp["name"], side, s_obs, s_acs)
            assert np.abs(x[:, :n_obs]).max() <= np.float32(sp["clip_obs"]) and np.abs(x[:, n_obs:]).max() <= 1.0
            n_cond += 1
        if c["stop"] is not None:
            d, stated = c["stop"]["direction"], res["stated"][ci]
            stops = [t["itr"] for t in trace if t["stopped"]]
            if d == "never":
                assert stops == [] and len(trace) == c["iters"] and c["tk"] == (-1, -1)
                assert max(t["kl_old_new"] for t in trace) > 5.0 and max(t["kl_new_old"] for t in trace) > 2.5      # the README thresholds would stop
            else:
                assert stops == [stated] and stated > 0 and call["om"]["backward/early_stop_itr"] == stated, (sp["name"], stops, stated)
                if "target" in c["stop"] and (c["stop"].get("midpoint") or d == "readme"):
                    assert stated == c["stop"]["target"], (sp["name"], stated)
                t = trace[-1]
                on_over = c["tk"][0] != -1 and t["kl_old_new"] > c["tk"][0]
                no_over = c["tk"][1] != -1 and t["kl_new_old"] > c["tk"][1]
                assert (on_over, no_over) == ((True, False) if d == "on" else (False, True)), (sp["name"], t["kl_old_new"], t["kl_new_old"], c["tk"])
                # each KL compared with the OTHER direction's threshold would stop at another iteration, or not at all
                swapped = [x["itr"] for x in trace if (c["tk"][0] != -1 and x["kl_new_old"] > c["tk"][0]) or
                           (c["tk"][1] != -1 and x["kl_old_new"] > c["tk"][1])]
                assert swapped[:1] != [stated], (sp["name"], swapped, stated)
            n_cond += 1
        if sp["gail"]:
            assert all(s["reg"] == 0 for t in trace for s in t["steps"]) and sp["reg"] in (0.0, 0.5)
        if sp["builder"] == "sat":
            net = oracle_net(sp)
            net.load_state_dict(res["w0"])
            for rows in (call["nominal"], call["expert"]):
                z = logits(net, rows)
                assert (z >= SAT_HIGH).sum() >= SAT_ROWS and (z <= SAT_LOW).sum() >= SAT_ROWS, (sp["name"], z.min(), z.max())
                assert not (((z > SAT_MID) & (z < SAT_HIGH)) | ((z < -SAT_MID) & (z > SAT_LOW))).any()
                zeta = net.forward(rows).detach().numpy().reshape(-1)
                assert (zeta[z >= SAT_HIGH] == 1.0).all() and (zeta[z <= SAT_LOW] == 0.0).all()
                assert (np.abs(z) <= SAT_MID).sum() >= 64
            n_cond += 1
    return n_cond


# ---- comparisons --------------------------------------------------------------------------------------------------------------------
ROW = dict(stopped=0, kl_old_new=1, kl_new_old=2, is_mean=3, is_max=4, is_min=5, loss=6, expert_loss=7, unweighted_nominal_loss=8,
           nominal_loss=9, reg=10, nominal_preds_max=11, nominal_preds_min=12, nominal_preds_mean=13, expert_preds_max=14,
           expert_preds_min=15, expert_preds_mean=16, executed=17)      # a row of the metrics table (include/icrl_hip.h: ICRL_CN_METRICS)


def close(got, ref, rtol=RTOL, atol=ATOL):
    return abs(float(got) - float(ref)) <= atol + rtol * abs(float(ref))


def moment_atol(ref):
    return min(ATOL, MOMENT_ATOL_SHARE * float(np.abs(np.asarray(ref)).max()))


def split_flat(cn, flat):
    out, off = OrderedDict(), 0
    flat = flat.detach().cpu().numpy()
    for k, shp in cn.shapes.items():
        n = int(np.prod(shp))
        out[k] = flat[off:off + n].reshape(shp)
        off += n
    return out


def product_of(sp, data, w0, stats=None, tk=(-1, -1)):
    """the product's ConstraintNet under a case's keywords with the given initial weights (needs the GPU)."""
    from icrl_amd.constraint_net import ConstraintNet
    lo = -np.ones(sp["acs_dim"], np.float32) if sp["bounded"] else None
    mean, var = stats_arrays(sp, stats)
    cn = ConstraintNet(sp["obs_dim"], sp["acs_dim"], list(sp["hidden"]), sp["batch_size"], lambda x: lr_of(sp, x), data["exp_obs"], data["exp_acs"],
                       sp["discrete"], sp["reg"], obs_select_dim=sp["obs_select_dim"], acs_select_dim=sp["acs_select_dim"],
                       no_importance_sampling=sp["nis"], per_step_importance_sampling=sp["psis"], clip_obs=sp["clip_obs"],
                       initial_obs_mean=mean, initial_obs_var=var, action_low=lo, action_high=None if lo is None else -lo,
                       target_kl_old_new=tk[0], target_kl_new_old=tk[1], train_gail_lambda=sp["gail"], eps=sp["eps"])
    cn.load_state_dict(w0)
    return cn


def product(res):
    """the product's ConstraintNet of a case: the oracle's keywords and initial weights."""
    c = res["calls"][0]["call"]
    return product_of(res["spec"], res["data"], res["w0"], c["stats"], c["tk"])


def begin_call(cn, res, ci):
    """ConstraintNet._train_begin of call ci of a case (thresholds, statistics, progress and permutations of that call)."""
    call, d = res["calls"][ci], res["data"]
    c = call["call"]
    cn.target_kl_old_new, cn.target_kl_new_old = c["tk"]
    mean, var = stats_arrays(res["spec"], c["stats"])
    return cn._train_begin(c["iters"], d["nom_obs"], d["nom_acs"], d["lengths"], mean, var, c["progress"], call["perms"])
