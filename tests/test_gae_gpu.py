"""GPU parity: icrl_gae_dual (HIP, through the C ABI) vs the oracle and vs the reference's golden vectors."""
import numpy as np
import pytest
import torch

from helpers import gae_cases as G, routes
from oracle import gae as o_gae

pytestmark = pytest.mark.gpu


def _run(arrs, params, W=0):
    from icrl_amd import _lib
    L = _lib.lib()
    dev = torch.device("cuda:0")
    f = lambda k: torch.as_tensor(np.ascontiguousarray(arrs[k], dtype=np.float32), device=dev)
    r, c, vr, vc, d = f("rewards"), f("costs"), f("reward_values"), f("cost_values"), f("dones")
    lvr, lvc = f("last_v_r"), f("last_v_c")
    ld = torch.as_tensor(np.asarray(arrs["last_dones"]).astype(np.uint8), device=dev)
    T, N = r.shape
    outs = [torch.full((T, N), float("nan"), device=dev) for _ in range(4)]
    err = L.icrl_gae_dual_ex(*(_lib.ptr(x) for x in (r, c, vr, vc, d, lvr, lvc, ld, *outs)), T, N,
                             *[float(p) for p in params], W, _lib.current_stream())
    _lib.check(err, "icrl_gae_dual_ex")
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in outs]


def _ulp_diff(a, b):
    ai, bi = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    return np.abs(ai - bi).max()


_G1_CASES = {"t8n3": 3, "t2000n1": 1, "t256n16": 16, "t1n4": 4, "t64n5": 5}          # case -> N
# launch shapes: library heuristic, 1 / 4 / 16 waves per tile, streaming one column per lane (106), four columns per lane (108, 111: N % 4 == 0)
_G1_PARAMS = [(c, W) for c in _G1_CASES for W in (0, 1, 4, 16, 106, 108, 111) if W <= 106 or _G1_CASES[c] % 4 == 0]


@pytest.mark.parametrize("case,W", _G1_PARAMS)
def test_gae_golden(golden, case, W):
    g = golden("g1_gae")
    arrs = {k.split("/")[1]: g[k] for k in g.files if k.startswith(case + "/")}
    adv_r, adv_c, ret_r, ret_c = _run(arrs, arrs["params"], W)
    for got, key in ((adv_r, "reward_advantages"), (adv_c, "cost_advantages"), (ret_r, "reward_returns"), (ret_c, "cost_returns")):
        if W == 1 or W > 100:
            assert np.array_equal(got, arrs[key]), key          # sequential scan: bit-exact with the reference
        else:
            # time-chunked scan re-associates float64 products: <= 1 ulp of float32 (rtol 1.2e-7), in practice exact
            assert np.allclose(got, arrs[key], rtol=2e-7, atol=1e-7), key


@pytest.mark.parametrize("T,N", [(2048, 64), (2048, 256), (500, 1000), (37, 4097), (2048, 4096), (33, 65536), (9, 131076), (5, 131074), (256, 131072)])
def test_gae_vs_oracle_random(T, N):
    """(256, 131 072): the launch shape bench.py's roofline is quoted on (gae_dual_x4_kernel<4,1>, 512 one-wave workgroups, 64 batches of
    the double-buffered 4-row loop per column).  incl. the streaming shapes the heuristic picks: one column per lane from 65 536 envs on, four columns per lane from 131 072
    on when N % 4 == 0 (131 076: a ragged last wave; 131 074: falls back to one column per lane); all bit-exact."""
    rng = np.random.RandomState(T + N)
    arrs = dict(rewards=rng.randn(T, N), costs=rng.rand(T, N), reward_values=rng.randn(T, N), cost_values=rng.randn(T, N),
                dones=(rng.rand(T, N) < 0.002), last_v_r=rng.randn(N), last_v_c=rng.randn(N), last_dones=rng.rand(N) < 0.2)
    arrs = {k: (v.astype(np.float32) if v.dtype != bool else v) for k, v in arrs.items()}
    params = (0.99, 0.95, 0.99, 0.9)
    o = o_gae.dual_gae(arrs["rewards"], arrs["costs"], arrs["reward_values"], arrs["cost_values"],
                       arrs["dones"].astype(np.float32), arrs["last_v_r"], arrs["last_v_c"], arrs["last_dones"], *params)
    for W in (0, 1):
        adv_r, adv_c, ret_r, ret_c = _run(arrs, params, W)
        for got, key in ((adv_r, "reward_advantages"), (adv_c, "cost_advantages"), (ret_r, "reward_returns"), (ret_c, "cost_returns")):
            if W == 1 or N >= 65536:
                assert np.array_equal(got, o[key]), (key, W)
            else:
                assert np.allclose(got, o[key], rtol=2e-7, atol=1e-7), (key, W)
                assert (got != o[key]).mean() < 1e-5


def test_gae_linearity_full_size():
    """Size-independent property at BASELINE scale (N = 65536, T = 2048 would be 4.8 GB of inputs; use 16384 x 2048):
    with dones = 0, GAE is linear in (rewards, values): gae(x + y) == gae(x) + gae(y) to float32 rounding."""
    T, N = 2048, 16384
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    from icrl_amd import _lib
    L = _lib.lib()

    def run(r, v):
        z = torch.zeros(T, N, device=dev)
        outs = [torch.empty(T, N, device=dev) for _ in range(4)]
        ld = torch.zeros(N, dtype=torch.uint8, device=dev)
        _lib.check(L.icrl_gae_dual(*(_lib.ptr(x) for x in (r, r, v, v, z, v[-1].contiguous(), v[-1].contiguous(), ld, *outs)),
                                   T, N, 0.99, 0.95, 0.99, 0.95, _lib.current_stream()), "gae")
        return outs[0], outs[1]
    r1, v1 = torch.randn(T, N, device=dev, generator=g), torch.randn(T, N, device=dev, generator=g)
    r2, v2 = torch.randn(T, N, device=dev, generator=g), torch.randn(T, N, device=dev, generator=g)
    a1, c1 = run(r1, v1)
    a2, _ = run(r2, v2)
    a12, _ = run(r1 + r2, v1 + v2)
    assert torch.equal(a1, c1)                         # reward and cost chains fed the same data agree bit-for-bit
    assert torch.allclose(a12, a1 + a2, rtol=1e-4, atol=1e-4)


def _run_ws(arrs, params, shape, ws):
    from icrl_amd import _lib
    L = _lib.lib()
    dev = torch.device("cuda:0")
    f = lambda k: torch.as_tensor(np.ascontiguousarray(arrs[k], dtype=np.float32), device=dev)
    r, c, vr, vc, d = f("rewards"), f("costs"), f("reward_values"), f("cost_values"), f("dones")
    lvr, lvc = f("last_v_r"), f("last_v_c")
    ld = torch.as_tensor(np.asarray(arrs["last_dones"]).astype(np.uint8), device=dev)
    T, N = r.shape
    outs = [torch.full((T, N), float("nan"), device=dev) for _ in range(4)]
    _lib.check(L.icrl_gae_dual_ws(*(_lib.ptr(x) for x in (r, c, vr, vc, d, lvr, lvc, ld, *outs)), T, N, *[float(p) for p in params],
                                  shape, _lib.ptr(ws), ws.numel() * 8, _lib.current_stream()), "icrl_gae_dual_ws")
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in outs]


def _ws(T=2048, N=1024):
    """a zeroed workspace of the size the library asks for at this shape (never below ICRL_GAE_WS_BYTES)."""
    from icrl_amd import _lib
    from icrl_amd.structs import GAE_WS_BYTES
    return torch.zeros(max(int(_lib.lib().icrl_gae_dual_ws_bytes(T, N)), GAE_WS_BYTES) // 8, dtype=torch.int64, device="cuda:0")


@pytest.mark.parametrize("case", ["t8n3", "t2000n1", "t256n16", "t1n4", "t64n5"])
@pytest.mark.parametrize("C", [2, 3, 16])
def test_gae_split_over_workgroups_golden(golden, case, C):
    """two-level scan (time axis split over C workgroups x 8 waves): the reference's golden vectors, incl. chunks that are empty
    (T = 1, T = 8 with 16 x 8 waves) and ragged; one workspace reused by every launch."""
    g = golden("g1_gae")
    arrs = {k.split("/")[1]: g[k] for k in g.files if k.startswith(case + "/")}
    ws = _ws()
    for _ in range(2):
        outs = _run_ws(arrs, arrs["params"], 200 + C, ws)
        for got, key in zip(outs, ("reward_advantages", "cost_advantages", "reward_returns", "cost_returns")):
            assert np.allclose(got, arrs[key], rtol=2e-7, atol=1e-7), key


@pytest.mark.parametrize("T,N", [(2048, 64), (2048, 256), (512, 256), (256, 512), (2048, 4096), (1000, 130), (100, 64)])
def test_gae_split_vs_oracle_random(T, N):
    """the shapes the loop launches (64 envs x 2048, the shard shapes of configs[2..4]) through the default heuristic with a
    workspace: <= 1 ulp of float32 from the sequential scan, and almost everywhere equal."""
    rng = np.random.RandomState(T + N)
    arrs = dict(rewards=rng.randn(T, N), costs=rng.rand(T, N), reward_values=rng.randn(T, N), cost_values=rng.randn(T, N),
                dones=(rng.rand(T, N) < 0.002), last_v_r=rng.randn(N), last_v_c=rng.randn(N), last_dones=rng.rand(N) < 0.2)
    arrs = {k: (v.astype(np.float32) if v.dtype != bool else v) for k, v in arrs.items()}
    params = (0.99, 0.95, 0.99, 0.9)
    o = o_gae.dual_gae(arrs["rewards"], arrs["costs"], arrs["reward_values"], arrs["cost_values"],
                       arrs["dones"].astype(np.float32), arrs["last_v_r"], arrs["last_v_c"], arrs["last_dones"], *params)
    ws = _ws(T, N)
    for rep in range(3):
        outs = _run_ws(arrs, params, 0, ws)
        # (a workspace of icrl_gae_dual_ws_bytes at T <= 2048 and fewer than 1024 tiles: the register-resident split, 128 rows per workgroup)
        routes.check_gae(dict(route="regsplit", code=-(-T // 128), tiles=-(-N // 64), n_runs=1), f"{T}x{N}")
        for got, key in zip(outs, ("reward_advantages", "cost_advantages", "reward_returns", "cost_returns")):
            assert np.allclose(got, o[key], rtol=2e-7, atol=1e-7), (key, rep)
            assert (got != o[key]).mean() < 1e-5


def _random_arrs(T, N, seed=None, done_rate=0.002):
    return G.random_arrs(T, N, seed, done_rate)


@pytest.mark.parametrize("case", ["t8n3", "t2000n1", "t256n16", "t1n4", "t64n5"])
def test_gae_register_resident_split_golden(golden, case):
    """the register-resident split scan (round 6; shape code 500) on the reference's golden vectors: T = 1 (head row only), T = 8 (one wave),
    T = 2000 (16 chunks, the last ragged), one workspace reused by consecutive launches."""
    g = golden("g1_gae")
    arrs = {k.split("/")[1]: g[k] for k in g.files if k.startswith(case + "/")}
    T, N = arrs["rewards"].shape
    ws = _ws(T, N)
    for _ in range(2):
        outs = _run_ws(arrs, arrs["params"], 500, ws)
        for got, key in zip(outs, ("reward_advantages", "cost_advantages", "reward_returns", "cost_returns")):
            assert np.allclose(got, arrs[key], rtol=2e-7, atol=1e-7), key
    assert int(ws.view(torch.int32)[-1].item()) == 0


@pytest.mark.parametrize("T,N", [(2048, 8192), (1024, 32768), (1000, 16390), (129, 9000), (256, 65472)])
def test_gae_mid_range_vs_oracle(T, N):
    """8 192 .. 65 472 envs (between the cache-resident and the streaming regime) through the DEFAULT heuristic with the
    workspace the library asks for: 2 048 .. 16 368 workgroups of the register-resident split scan, non-temporal accesses; ragged tiles and
    ragged chunks; <= 1 ulp of float32 from the sequential scan and almost everywhere equal (ref: buffers.py:493-552).  That the automatic
    call took the register-resident split is asserted from the library's record of it (128 rows per workgroup; the automatic choice takes
    that form below 1024 column tiles, and 65 472 envs are 1023)."""
    arrs = _random_arrs(T, N)
    params = (0.99, 0.95, 0.99, 0.9)
    o = o_gae.dual_gae(arrs["rewards"], arrs["costs"], arrs["reward_values"], arrs["cost_values"],
                       arrs["dones"].astype(np.float32), arrs["last_v_r"], arrs["last_v_c"], arrs["last_dones"], *params)
    ws = _ws(T, N)
    assert -(-N // 64) < 1024
    for rep in range(2):
        outs = _run_ws(arrs, params, 0, ws)
        routes.check_gae(dict(route="regsplit", code=-(-T // 128), tiles=-(-N // 64), n_runs=1), f"{T}x{N}")
        for got, key in zip(outs, ("reward_advantages", "cost_advantages", "reward_returns", "cost_returns")):
            assert np.allclose(got, o[key], rtol=2e-7, atol=1e-7), (key, rep)
            assert (got != o[key]).mean() < 1e-5
    assert int(ws.view(torch.int32)[-1].item()) == 0
    # the sequential shape forced on the same inputs is bit-exact against the oracle (the split scan above is not required to be)
    seq = _run_ws(arrs, params, 1, ws)
    routes.check_gae(dict(route="sequential", code=101, n_runs=1), "forced")
    assert np.array_equal(seq[0], o["reward_advantages"])


@pytest.mark.parametrize("shape", [501, 304])
def test_gae_split_wait_is_bounded_and_reported(shape):
    """every wait of the split scans ends.  Shape codes 501 (register-resident) / 300 + C (two-pass) withhold the map of the
    workgroup holding the LATEST rows and shorten the poll limit: the launch must end, the workspace's status word must be 1, and
    RolloutBufferWithCost.check_gae_status must raise and clear it; the next healthy launch on the same workspace is correct again."""
    T, N = 1024, 192
    arrs = _random_arrs(T, N, 7)
    params = (0.99, 0.95, 0.99, 0.95)
    ws = _ws(T, N)
    _run_ws(arrs, params, shape, ws)                      # returns (synchronised) instead of hanging
    status = ws.view(torch.int32)[-1:]
    assert int(status.item()) == 1
    from icrl_amd.buffers import RolloutBufferWithCost
    rb = RolloutBufferWithCost.__new__(RolloutBufferWithCost)
    rb.gae_status = status
    with pytest.raises(RuntimeError, match="affine map"):
        rb.check_gae_status()
    assert int(status.item()) == 0
    o = o_gae.dual_gae(arrs["rewards"], arrs["costs"], arrs["reward_values"], arrs["cost_values"],
                       arrs["dones"].astype(np.float32), arrs["last_v_r"], arrs["last_v_c"], arrs["last_dones"], *params)
    outs = _run_ws(arrs, params, 500 if shape == 501 else 204, ws)
    assert np.allclose(outs[0], o["reward_advantages"], rtol=2e-7, atol=1e-7) and int(status.item()) == 0


# ---------------------------------------------------------------------------------------------------------------------
# The rollout-end launches at the parameters, done patterns and shapes the tests above do not reach.  Every output plane is
# allocated [T + 1, N] and starts as NaN; its first T rows are passed.  Afterwards all T x N entries must be finite and the extra row
# still NaN: a store from a dead lane of a ragged tile, or past the last row, shows.
# ---------------------------------------------------------------------------------------------------------------------
def _upload(arrs):
    dev = torch.device("cuda:0")
    ins = [torch.as_tensor(np.array(arrs[k], dtype=np.float32), device=dev)
           for k in ("rewards", "costs", "reward_values", "cost_values", "dones", "last_v_r", "last_v_c")]
    return ins + [torch.as_tensor(np.array(arrs["last_dones"]).astype(np.uint8), device=dev)]


def _guarded(T, N):
    return [torch.full((T + 1, N), float("nan"), device="cuda:0") for _ in range(4)]


def _check_guard(outs, T):
    for o, key in zip(outs, G.OUT_KEYS):
        assert bool(torch.isfinite(o[:T]).all()), f"{key}: an element was not written (or is not finite)"
        assert bool(torch.isnan(o[T]).all()), f"{key}: a store past row T - 1"


def _launch(ins, outs, T, N, params, shape, ws):
    from icrl_amd import _lib
    _lib.check(_lib.lib().icrl_gae_dual_ws(*(_lib.ptr(x) for x in (*ins, *outs)), T, N, *[float(p) for p in params], shape, _lib.ptr(ws),
                                           ws.numel() * 8 if ws is not None else 0, _lib.current_stream()), "icrl_gae_dual_ws")
    torch.cuda.synchronize()


def _status(ws):
    return int(ws.view(torch.int32)[-1].item())


def _run_guarded(arrs, params, shape, ws=None, launches=1):
    """`launches` consecutive launches (on the same workspace), each into fresh guarded planes; the host copies of every launch."""
    T, N = arrs["rewards"].shape
    ins, res = _upload(arrs), []
    for _ in range(launches):
        outs = _guarded(T, N)
        _launch(ins, outs, T, N, params, shape, ws)
        _check_guard(outs, T)
        res.append([o[:T].cpu().numpy() for o in outs])
    return res


# scan form -> N: 1 / 4 / 16 waves per tile, streaming one column per lane (106), four per lane (108, 111: N % 4 == 0), the two-pass split
# over 3 workgroups (203), the register-resident split (500) and the heuristic with a workspace (0: the register-resident split here)
_FORMS = [(1, 70), (4, 70), (16, 70), (106, 70), (108, 72), (111, 72), (203, 70), (500, 70), (0, 70)]


@pytest.mark.parametrize("p,pattern", G.CASES)
@pytest.mark.parametrize("shape,N", _FORMS)
def test_gae_every_form_at_every_parameter_set_and_done_pattern(shape, N, p, pattern):
    """T = 300 (= 2 x 128 + 44: ragged chunks, ragged and empty waves), N = 70 (two tiles, six live lanes in the second) / 72.  Four different
    gammas / lambdas (a reward / cost swap in the step loop shows), lambda = 1 (the buffer's default), gamma = lambda = 1, lambda = 0
    (every affine map has P = 0); dones none / all / at 0.3 / on the seams of every chunking / last_dones all and none.  Sequential forms:
    bit-equal to the oracle.  Chunked forms: the project's bound for the re-associated float64 fold, and at most 1e-3 of an array's elements
    unequal — tests/test_gae_fold_cpu.py shows the reference arithmetic alone stays inside that on these inputs."""
    arrs, params, o = G.form_case(N, p, pattern)
    ws = _ws(G.T_FORMS, N) if shape in (203, 500, 0) else None
    (outs,) = _run_guarded(arrs, params, shape, ws)
    routes.check_gae({1: dict(route="sequential", code=101), 4: dict(route="sequential", code=4), 16: dict(route="sequential", code=16),
                      106: dict(route="sequential", code=106), 108: dict(route="sequential", code=108), 111: dict(route="sequential", code=111),
                      203: dict(route="split", code=3), 500: dict(route="regsplit", code=3), 0: dict(route="regsplit", code=3)}[shape], f"form {shape}")
    for got, key in zip(outs, G.OUT_KEYS):
        if shape in (1, 106, 108, 111):
            assert np.array_equal(got, o[key]), key
        else:
            assert np.allclose(got, o[key], rtol=2e-7, atol=1e-7), key
            assert (got != o[key]).mean() <= 1e-3, (key, int((got != o[key]).sum()))
    if ws is not None:
        assert _status(ws) == 0


_SWAP_PARAMS = G.PARAM_SETS[0]


def _swap_case(T, N, seed=None):
    """random inputs with dones at 0.02 and the oracle at four different gammas / lambdas, read-only."""
    arrs = _random_arrs(T, N, seed, 0.02)
    o = G.oracle(arrs, _SWAP_PARAMS)
    for v in (*arrs.values(), *o.values()):
        v.setflags(write=False)
    return arrs, o


def _assert_split_bounds(got, want, key):
    assert np.allclose(got, want, rtol=2e-7, atol=1e-7), key
    if got.size >= 1e6:
        assert (got != want).mean() < 1e-5, (key, int((got != want).sum()))


_TWO_PASS_C = {(2049, 70): 16, (2304, 130): 10, (4096, 64): 16, (2304, 1100): 14, (512, 200): 4, (1000, 130): 16}      # workgroups per tile (the docstring's)


@pytest.mark.parametrize("T,N,shape", [(2049, 70, 0), (2304, 130, 0), (4096, 64, 0), (2304, 1100, 0), (512, 200, 204), (1000, 130, 216)])
def test_gae_two_pass_split_where_it_is_the_default_and_over_several_tiles(T, N, shape):
    """gae_dual_split_kernel: the default for every T > 2048 with a workspace (shape 0: 16 / 10 / 16 workgroups per tile; 18 tiles under the
    256-workgroup cap: 14 ragged chunks of 165 rows) and forced over 4 tiles x 4 and 3 tiles x 16 workgroups.  Two launches on one workspace."""
    arrs, o = _swap_case(T, N)
    ws = _ws(T, N)
    for outs in _run_guarded(arrs, _SWAP_PARAMS, shape, ws, launches=2):
        for got, key in zip(outs, G.OUT_KEYS):
            _assert_split_bounds(got, o[key], key)
    routes.check_gae(dict(route="split", code=_TWO_PASS_C[T, N], tiles=-(-N // 64), n_runs=1), f"{T}x{N} shape {shape}")
    assert _status(ws) == 0


@pytest.mark.parametrize("params", [G.PARAM_SETS[0], G.PARAM_SETS[2]])
@pytest.mark.parametrize("T", [256, 1024, 2048])
def test_gae_register_resident_scan_equals_the_two_pass_scan_bit_for_bit(T, params):
    """ADVICE.md (round 6), first item.  The register-resident scan exchanges its maps with relaxed atomics only, the two-pass scan with
    release / acquire.  At T = 128 C both use 128-row chunks and 16 rows per wave, compose the wave maps and the chunk maps in the same order
    and apply the same per-row arithmetic on replay (the two-pass body walks its rows again through walk_chunk, the register-resident body
    through rs_head_apply + run_batch on the rows it kept in registers): the same float64 operations in the same order, so all four outputs
    agree bit for bit."""
    N = 130
    arrs = _random_arrs(T, N, None, 0.02)
    ws = _ws(T, N)
    (reg,) = _run_guarded(arrs, params, 500, ws)
    (two,) = _run_guarded(arrs, params, 200 + T // 128, ws)
    for a, b, key in zip(reg, two, G.OUT_KEYS):
        ne = np.argwhere(a != b)
        assert ne.size == 0, (key, len(ne), ne[:4].tolist())
    assert _status(ws) == 0


class _BatchRun:
    """one run of a batch: its own data (own seed, own last values), guarded outputs, its own zeroed workspace of icrl_gae_dual_ws_bytes."""

    def __init__(self, T, N, seed, with_ws=True):
        from icrl_amd import _lib
        arrs, self.o = _swap_case(T, N, seed)
        self.ins = _upload(arrs)
        self.outs = _guarded(T, N)
        nbytes = int(_lib.lib().icrl_gae_dual_ws_bytes(T, N))
        self.ws = torch.zeros(nbytes // 8, dtype=torch.int64, device="cuda:0") if with_ws else None

    def job(self):
        from icrl_amd import _lib, structs as S
        return S.GaeJobT(*(_lib.ptr(x) for x in (*self.ins, *self.outs)), _lib.ptr(self.ws), self.ws.numel() * 8 if self.ws is not None else 0)


def _dev_bounds(got, want, key):
    """_assert_split_bounds on the device (the large case would spend seconds in numpy)."""
    w = torch.as_tensor(np.array(want), device=got.device)
    assert bool(torch.isclose(got, w, rtol=2e-7, atol=1e-7).all()), key
    if w.numel() >= 1e6:
        assert float((got != w).float().mean()) < 1e-5, key


# (T, N, n_runs, variant)
_BATCH_CASES = [(300, 130, 3, ""),              # register-resident batch kernel, three chunks, ragged
                (2048, 64, 8, ""),              # the shape the seed-batch throughput is quoted on: 16 chunks, grid.y = 8
                (2304, 70, 3, ""), (2304, 1100, 2, ""),      # T > 2048: gae_dual_split_batch_kernel, 16 chunks / 18 tiles x 14 ragged chunks
                (1025, 16400, 2, ""),           # 257 tiles x 1025 rows > 128 x 2048: the non-temporal kernel, 9 chunks, the last of one row
                (300, 130, 3, "job1_no_ws"),    # one job without workspace: n_runs single launches
                (300, 130, 3, "no_args_ws")]    # no argument scratch: n_runs single launches


_BATCH_ROUTES = {(300, 130, ""): "batch-regsplit", (2048, 64, ""): "batch-regsplit", (2304, 70, ""): "batch-split", (2304, 1100, ""): "batch-split",
                 (1025, 16400, ""): "batch-regsplit", (300, 130, "job1_no_ws"): "batch-singles", (300, 130, "no_args_ws"): "batch-singles"}


@pytest.mark.parametrize("T,N,n_runs,variant", _BATCH_CASES)
def test_gae_dual_batch_vs_oracle_and_vs_the_single_launch(T, N, n_runs, variant):
    """icrl_gae_dual_batch on its own: every branch (register-resident, non-temporal register-resident, two-pass, the fallback to single
    launches), every run against the ORACLE and bit-equal to icrl_gae_dual_ws(shape 0) on the same inputs with a workspace of the same
    size (include/icrl_hip.h: "computes for each run exactly what the single-run call computes"); status words, guard rows, two launches
    on the same workspaces (the fold order is fixed, so the second launch must repeat the first bit for bit)."""
    from icrl_amd import _lib, structs as S
    L = _lib.lib()
    runs = [_BatchRun(T, N, 1000 + 17 * r + T + N, with_ws=not (variant == "job1_no_ws" and r == 1)) for r in range(n_runs)]
    garr = (S.GaeJobT * n_runs)(*[r.job() for r in runs])
    args_ws = None if variant == "no_args_ws" else torch.zeros(n_runs * _lib.BATCH_ARGS_BYTES, dtype=torch.uint8, device="cuda:0")
    first = None
    for launch in range(2):
        _lib.check(L.icrl_gae_dual_batch(n_runs, garr, T, N, *[float(p) for p in _SWAP_PARAMS], _lib.ptr(args_ws),
                                         args_ws.numel() if args_ws is not None else 0, _lib.current_stream()), "icrl_gae_dual_batch")
        routes.check_gae(dict(route=_BATCH_ROUTES[T, N, variant], tiles=-(-N // 64), n_runs=n_runs), f"batch {T}x{N} {variant}")
        torch.cuda.synchronize()
        for r in runs:
            _check_guard(r.outs, T)
            assert r.ws is None or _status(r.ws) == 0
        if launch == 0:
            for r in runs:
                for got, key in zip(r.outs, G.OUT_KEYS):
                    _dev_bounds(got[:T], r.o[key], key)
            first = [[o.clone() for o in r.outs] for r in runs]
            for r in runs:
                for o in r.outs:
                    o.fill_(float("nan"))
        else:
            for r, f in zip(runs, first):
                for got, was, key in zip(r.outs, f, G.OUT_KEYS):
                    assert torch.equal(got[:T], was[:T]), ("second launch", key)
    # the single launch on the same inputs: a workspace of the same size (or none where the job had none)
    for r, f in zip(runs, first):
        ws = torch.zeros_like(r.ws) if r.ws is not None else None
        single = _guarded(T, N)
        _launch(r.ins, single, T, N, _SWAP_PARAMS, 0, ws)
        _check_guard(single, T)
        for got, want, key in zip(f, single, G.OUT_KEYS):
            assert torch.equal(got[:T], want[:T]), ("batch != single launch", key)
        assert ws is None or _status(ws) == 0


def test_gae_dual_batch_refuses_no_runs_and_no_rows():
    from icrl_amd import _lib, structs as S
    L = _lib.lib()
    run = _BatchRun(8, 4, 5)
    garr = (S.GaeJobT * 1)(run.job())
    args_ws = torch.zeros(_lib.BATCH_ARGS_BYTES, dtype=torch.uint8, device="cuda:0")
    call = lambda n_runs, T: L.icrl_gae_dual_batch(n_runs, garr, T, 4, 0.99, 0.95, 0.99, 0.95, _lib.ptr(args_ws), args_ws.numel(), _lib.current_stream())
    try:
        assert call(0, 8) != 0 and "n_runs" in L.icrl_last_error().decode()
        L.icrl_clear_error()
        assert call(1, 0) != 0 and "T = 0" in L.icrl_last_error().decode()
    finally:
        L.icrl_clear_error()
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(o).all()) for o in run.outs)          # a refused call launches nothing
