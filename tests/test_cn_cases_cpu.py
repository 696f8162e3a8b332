"""The input conditions of tests/helpers/cn_cases.py, asserted from the oracle alone (no GPU): every case of the constraint-net parity file
(tests/test_cn_settings_gpu.py) is finite, its per-episode weights spread, its clips are reached, its stop happens at the stated iteration
in the stated direction, its saturated rows sit in the stated logit bands.  Also the oracle's trace, and the refusal of optimiser
settings the kernels do not implement."""
import numpy as np
import pytest
import torch

from helpers import cn_cases as C
from oracle import cn as o_cn


@pytest.mark.parametrize("name", list(C.CASES))
def test_case_conditions(name):
    res = C.run(name)
    n = C.check_conditions(res)
    sp = res["spec"]
    assert n >= int(sp["weights"]) + int(sp["clips"]) + int(sp["builder"] == "sat") + sum(c["call"]["stop"] is not None for c in res["calls"])


def test_layouts():
    assert len(C.R22) == 22 and sum(C.R22) == 1082 and sum(C.R22) % 64 == 58 and C.DEFAULT["Ne"] % 64 == 44
    assert {1, 63, 64, 65}.issubset(C.R22) and max(C.R22) > 192 and any(128 < n <= 192 for n in C.R22)
    assert C.ONE == [300] and C.R17 == [1] * 16 + [100]
    assert len({C.spec(n)["hidden"][0] for n in C.BATCHED}) == 1 and len({C.spec(n)["layout"] for n in C.BATCHED}) == 1


def test_case_table_covers_the_settings():
    sp = {n: C.spec(n) for n in C.CASES}
    assert any(s["gail"] and s["nis"] and s["batch_size"] is None and s["reg"] == 0.5 for s in sp.values())      # the *-Glag runs
    assert any(s["discrete"] and s["reg"] == 0 and not s["psis"] and len(C.LAYOUTS[s["layout"]]) > 16 for s in sp.values())      # LapGrid
    assert any(s["batch_size"] and len(s["hidden"]) == 3 for s in sp.values()) and any(s["batch_size"] and len(s["hidden"]) == 4 for s in sp.values())
    r = C.run("mb/episode-R17-tail1")
    assert min(len(r["calls"][0]["nominal"]), len(r["calls"][0]["expert"])) % r["spec"]["batch_size"] == 1
    r = C.run("mb/4layers")
    assert min(len(r["calls"][0]["nominal"]), len(r["calls"][0]["expert"])) % r["spec"]["batch_size"] == 0
    r = C.run("state/three-calls")
    assert len({c["lr"] for c in r["calls"]}) == 3 and 0 < r["stated"][1] < r["calls"][1]["call"]["iters"]
    assert [c["step"] for c in r["calls"]] == [4, 4 + r["stated"][1], 8 + r["stated"][1]]
    on, no = C.run("stop/old-new"), C.run("stop/new-old")
    assert on["calls"][0]["call"]["tk"][1] == -1 and no["calls"][0]["call"]["tk"][0] > 0
    last = C.run("stop/last")
    assert last["stated"][0] == last["calls"][0]["call"]["iters"] - 1
    assert C.run("stop/readme")["calls"][0]["call"]["tk"] == (10, 2.5)


def test_trace_leaves_the_oracle_unchanged():
    """cn_train with and without a trace list returns the same metrics and leaves the same weights; the trace's last rows are the metrics."""
    res = C.run("layout/R17-reg0.5")
    sp, call = res["spec"], res["calls"][0]
    net = C.oracle_net(sp)
    net.load_state_dict(res["w0"])
    opt = torch.optim.Adam(net.parameters(), lr=call["lr"], eps=1e-5)
    om = o_cn.cn_train(net, opt, call["call"]["iters"], call["nominal"], call["expert"], res["data"]["lengths"], reg_coeff=sp["reg"], factored=True)
    assert om == call["om"]
    assert all(torch.equal(v, call["sd"][k]) for k, v in net.state_dict().items())
    t = call["trace"]
    assert [x["itr"] for x in t] == list(range(call["call"]["iters"])) and not any(x["stopped"] for x in t)
    assert t[-1]["steps"][-1]["loss"] == om["backward/cn_loss"] and t[-1]["kl_new_old"] == om["backward/kl_new_old"]
    assert t[-1]["is_max"] == om["backward/is_max"] and t[-1]["prod"].shape == (17,) and t[0]["kl_old_new"] == pytest.approx(0, abs=1e-4)


@pytest.mark.parametrize("kw,word", [(dict(optimizer_kwargs=dict(eps=1e-5, betas=(0.5, 0.9))), "betas"),
                                     (dict(optimizer_kwargs=dict(weight_decay=0.1)), "weight_decay"),
                                     (dict(optimizer_class=torch.optim.SGD), "SGD")])
def test_unsupported_optimizer_settings_are_refused(kw, word, monkeypatch):
    """the kernels hard-code Adam with betas (0.9, 0.999) and read optimizer_kwargs['eps'] only: anything else is refused by name, before
    the library or the device is touched."""
    from icrl_amd import _lib
    from icrl_amd.constraint_net import ConstraintNet

    def never(*a, **k):
        raise AssertionError("the refusal must come before the library is loaded")
    monkeypatch.setattr(_lib, "lib", never)
    with pytest.raises(NotImplementedError, match=word):
        ConstraintNet(18, 6, [20], None, lambda x: 0.01, None, None, False, **kw)
