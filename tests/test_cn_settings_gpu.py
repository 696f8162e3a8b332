"""GPU parity of the constraint-net update (csrc/cn_train.hip through ConstraintNet.train / prepare_data / cost_function) with the oracle at
the weight layouts, loss forms and inputs of tests/helpers/cn_cases.py.  Every test first asserts its case's input conditions from the
oracle (tests/test_cn_cases_cpu.py keeps them verified without a GPU), then compares EVERY metrics row the oracle's trace has, the final
weights, both Adam moments and the step count, at the bound of test_cn_train_vs_oracle (rtol 3e-3 / atol 3e-4; a moment tensor's atol is
at most 1 % of its largest reference entry)."""
import numpy as np
import pytest
import torch

from helpers import cn_cases as C

pytestmark = pytest.mark.gpu

STEP_KEYS = ("loss", "expert_loss", "unweighted_nominal_loss", "nominal_loss", "reg", "nominal_preds_max", "nominal_preds_min",
             "nominal_preds_mean", "expert_preds_max", "expert_preds_min", "expert_preds_mean")


def _units(got, ref, rtol, atol):
    """largest |got - ref| in units of the bound atol + rtol |ref| (<= 1: np.allclose holds)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.max(np.abs(got - ref) / (atol + rtol * np.abs(ref))))


def _launch(cn, res, ci):
    job = C.begin_call(cn, res, ci)
    cn._train_launch(job)
    return job, cn._train_end(job)


def _compare_call(cn, job, bw, call, what):
    """one train() call against the oracle's: every traced metrics row, the returned dict, weights, moments, step count."""
    worst, bad = [0.0, None], []

    def chk(name, got, ref, atol=C.ATOL):
        u = _units(got, ref, C.RTOL, atol)
        if u > worst[0]:
            worst[:] = [u, name]
        if not u <= 1.0:
            bad.append((name, np.asarray(got).reshape(-1)[:4], np.asarray(ref).reshape(-1)[:4], round(u, 2)))

    m, trace, om = job["metrics"].cpu().numpy(), call["trace"], call["om"]
    for t in trace:
        row = m[t["itr"]]
        assert row[C.ROW["stopped"]] == float(t["stopped"]), (what, t["itr"], "stopped")
        assert row[C.ROW["executed"]] == float(len(t["steps"]) > 0), (what, t["itr"], "executed")
        for k in ("kl_old_new", "kl_new_old", "is_mean", "is_max", "is_min"):
            if t[k] is not None:
                chk(f"row {t['itr']} {k}", row[C.ROW[k]], t[k])
        if t["steps"]:      # (minibatch mode: the row holds the iteration's LAST optimiser step, as the reference's metrics do)
            for k in STEP_KEYS:
                chk(f"row {t['itr']} {k}", row[C.ROW[k]], t["steps"][-1][k])
    assert not m[len(trace):].any(), (what, "rows after the last iteration entered")
    assert set(bw) == set(om), (what, set(bw) ^ set(om))
    if "backward/early_stop_itr" in om:
        assert bw["backward/early_stop_itr"] == om["backward/early_stop_itr"], (what, bw["backward/early_stop_itr"], om["backward/early_stop_itr"])
    for k in om:       # which row each reported number comes from: losses / predictions of the last executed, KLs / is_* of the last entered
        chk(k, bw[k], om[k])
    for k, v in cn.state_dict().items():
        chk("weights " + k, v.numpy(), call["sd"][k].numpy())
    for name, flat, ref in (("exp_avg", cn.exp_avg, call["exp_avg"]), ("exp_avg_sq", cn.exp_avg_sq, call["exp_avg_sq"])):
        for k, v in C.split_flat(cn, flat).items():
            chk(f"{name} {k}", v, ref[k].numpy(), atol=C.moment_atol(ref[k].numpy()))
    assert cn.adam_step == call["step"], (what, cn.adam_step, call["step"])
    print(f"[cn parity] {what}: worst {worst[0]:.3f} of the bound at {worst[1]}")
    assert not bad, (what, bad)


def _parity(name):
    res = C.run(name)
    C.check_conditions(res)
    cn = C.product(res)
    for ci, call in enumerate(res["calls"]):
        job, bw = _launch(cn, res, ci)
        _compare_call(cn, job, bw, call, f"{name} call {ci}")
    return res, cn, bw


@pytest.mark.parametrize("name", [n for n in C.CASES if n.startswith("layout/")])
def test_per_episode_weight_layouts(name):
    """per-episode weights over 22 unequal episodes (two passes of cn_finalize_body, the row -> episode map), one episode, and sixteen
    one-row episodes before a long one; regulariser off (LapGrid-ICRL) and on; weights in LDS and ([128, 128]) in device memory."""
    res, cn, _ = _parity(name)
    assert cn.wide == (res["spec"]["hidden"] != [20])


@pytest.mark.parametrize("name", [n for n in C.CASES if n.startswith("form/")])
def test_full_batch_loss_forms(name):
    """-nis alone, --train_gail_lambda -nis (the BCE form through the full-batch kernels: no regulariser although -crc 0.5 is given), and
    the per-step form without a regulariser."""
    res, cn, bw = _parity(name)
    if res["spec"]["gail"]:
        assert res["spec"]["reg"] == 0.5 and bw["backward/regularizer_loss"] == 0.0


@pytest.mark.parametrize("name", C.INPUT_VARIANTS)
def test_input_variants(name):
    """normalisation + clip_obs + eps, no clips at all, one-hot discrete actions ([N, 1] and [N]), select_dim subsets, observations only,
    actions only and the default re-selection of the leading observation columns, at three levels: prepare_data bit for bit, cost_function
    on a narrow and a wide net (cn_cost_rows_body's own copy of the arithmetic) at 1 / 64 / 65 / 257 rows, and 3 iterations of train."""
    res = C.run(name)
    C.check_conditions(res)
    sp, d, call = res["spec"], res["data"], res["calls"][0]
    cn = C.product(res)
    for obs, acs, ref in ((d["nom_obs"], d["nom_acs"], call["nominal"]), (d["exp_obs"], d["exp_acs"], call["expert"])):
        got = cn.prepare_data(obs, acs).cpu().numpy()
        assert got.shape == tuple(ref.shape) and np.array_equal(got, ref.numpy()), (name, "prepare_data", np.abs(got - ref.numpy()).max())
    for hidden in ([20], [128, 128]):
        spw = dict(sp, hidden=hidden)
        orc = C.oracle_net(spw, call["call"]["stats"], seed_shift=3)
        net = C.product_of(spw, d, orc.state_dict(), call["call"]["stats"])
        assert net.wide == (hidden != [20])
        for n in (1, 64, 65, 257):
            got = net.cost_function(d["nom_obs"][:n], d["nom_acs"][:n])
            ref = orc.cost_function(d["nom_obs"][:n], d["nom_acs"][:n])
            assert got.shape == ref.shape == (n,)
            assert np.allclose(got, ref, rtol=C.COST_RTOL, atol=C.COST_ATOL), (name, hidden, n, np.abs(got - ref).max())
    job, bw = _launch(cn, res, 0)
    _compare_call(cn, job, bw, call, name)


def test_state_across_calls():
    """three train() calls on one net: another learning rate (-aclr 0.9) and other normalisation statistics (-cn: the expert rows are
    prepared again) per call, on a continued Adam state; the second call early-stops at k > 0 and advances the step count by k."""
    res, cn, _ = _parity("state/three-calls")
    k = res["stated"][1]
    assert 0 < k < res["calls"][1]["call"]["iters"] and cn.adam_step == 4 + k + 4


@pytest.mark.parametrize("name", [n for n in C.CASES if n.startswith("stop/")])
def test_early_stop(name):
    """each KL direction alone, -1 meaning never, a stop at the last iteration, the README thresholds: the stopping iteration, and which
    row each reported number comes from (_train_end: last_exec / last_is)."""
    res, cn, bw = _parity(name)
    stated = res["stated"][0]
    assert bw["backward/early_stop_itr"] == (res["calls"][0]["call"]["iters"] if stated is None else stated)


@pytest.mark.parametrize("name", [n for n in C.CASES if n.startswith("mb/")])
def test_minibatch_mode(name):
    """--cn_batch_size with recorded permutations: per-episode weights gathered through the permutation on unequal episodes, weights in
    device memory, 3 and 4 layers, the BCE form, Nn < Ne and Nn > Ne, a tail batch of one row, one batch, an exact divisor."""
    _parity(name)


@pytest.mark.parametrize("name", [n for n in C.CASES if n.startswith("sat/")])
def test_saturated_predictions(name):
    """zeta exactly 1.0f and exactly 0 in both sets (the -100 clamp of BCELoss, log(0 + eps), zero sigmoid gradients): losses, gradients
    (through the moments of one step) and updated weights, BCE form and ICRL form."""
    _parity(name)


def test_batched_launch_equals_single_runs():
    """icrl_cn_train_batch over three runs of one shape and three forms (per-episode on R22, -nis, BCE), the job table built as
    seed_batch._launch_cn_trains builds it: metrics, weights, moments and step counts equal the single-run calls bit for bit."""
    from icrl_amd import _lib
    from icrl_amd.seed_batch import _jobs
    from icrl_amd.structs import CnTrainJobT, addr, p
    runs = [C.run(n) for n in C.BATCHED]
    solo = []
    for res in runs:
        cn = C.product(res)
        job, _ = _launch(cn, res, 0)
        solo.append((job["metrics"].cpu().numpy(), cn.params.cpu().numpy(), cn.exp_avg.cpu().numpy(), cn.exp_avg_sq.cpu().numpy(), cn.adam_step))
    nets = [C.product(res) for res in runs]
    jobs = [C.begin_call(cn, res, 0) for cn, res in zip(nets, runs)]
    rows = [(addr(j["s"]), p(cn.exp_avg), p(cn.exp_avg_sq), p(j["t_dev"]), p(j["nominal"]), p(j["expert"]), j["nominal"].shape[0],
             j["expert"].shape[0], p(j["d_off"]), p(j["d_rowep"]), j["n_ep"], 0, addr(j["hp"]), p(j["work"]), p(j["metrics"])) for cn, j in zip(nets, jobs)]
    ws = torch.empty(2 * len(jobs) * _lib.BATCH_ARGS_BYTES, dtype=torch.uint8, device="cuda")
    _lib.check(_lib.lib().icrl_cn_train_batch(len(jobs), _jobs(CnTrainJobT, rows), p(ws), ws.numel(), _lib.current_stream()), "icrl_cn_train_batch")
    for name, cn, j, ref, res in zip(C.BATCHED, nets, jobs, solo, runs):
        bw = cn._train_end(j)
        got = (j["metrics"].cpu().numpy(), cn.params.cpu().numpy(), cn.exp_avg.cpu().numpy(), cn.exp_avg_sq.cpu().numpy(), cn.adam_step)
        for what, g, r in zip(("metrics", "weights", "exp_avg", "exp_avg_sq", "adam_step"), got, ref):
            assert np.array_equal(g, r), (name, what)
        _compare_call(cn, j, bw, res["calls"][0], name + " (batched)")
