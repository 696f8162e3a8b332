"""What a fused call launched (icrl_debug_last_route), for the tests that compare one launch form with another: a case that names a
kernel family states the route it expects as data beside its parameters and reads the record immediately after the call under test —
before the comparison run's call overwrites it.  A ladder that falls through to the per-step launches then fails the case instead
of comparing per-step launches with per-step launches."""
from icrl_amd import _lib

ROLLOUT_WORDS = ("route", "ws", "wgs", "envs_per_wg", "pick", "packed", "n_runs", "launches")
UPDATE_WORDS = ("kind", "wgs_per_network", "n_runs", "packed")
GAE_WORDS = ("route", "code", "tiles", "n_runs")
PICK_SMALL, PICK_ANALYTIC, PICK_MON, PICK_GRAN, PICK_CN128 = _lib.PICK_SMALL, _lib.PICK_ANALYTIC, _lib.PICK_MON, _lib.PICK_GRAN, _lib.PICK_CN128
_ROUTE_NAME = {v: k for k, v in _lib.ROUTE.items()}
_GAE_NAME = {v: k for k, v in _lib.GAE_ROUTE.items()}


def rollout():
    """the calling thread's last rollout call: its words by name, `route` as its name (_lib.ROUTE), `minw` split off `pick`."""
    w = dict(zip(ROLLOUT_WORDS, _lib.last_route(_lib.FAMILY_ROLLOUT)))
    w["route"] = _ROUTE_NAME[w["route"]]
    w["minw"] = w["pick"] >> _lib.PICK_MINW_SHIFT
    w["pick"] &= (1 << _lib.PICK_MINW_SHIFT) - 1
    return w


def update():
    return dict(zip(UPDATE_WORDS, _lib.last_route(_lib.FAMILY_UPDATE)))


def gae():
    w = dict(zip(GAE_WORDS, _lib.last_route(_lib.FAMILY_GAE)))
    w["route"] = _GAE_NAME[w["route"]]
    return w


def _check(got, expect, what):
    print(f"[route] {what}: {got}")
    for k, v in expect.items():
        assert got[k] == v, f"{what}: {k} = {got[k]!r}, expected {v!r} (the call launched {got})"
    return got


def check_rollout(expect, what=""):
    """expect: a route name, or a dict of words (route by name).  Prints the record, then asserts; returns it."""
    return _check(rollout(), dict(route=expect) if isinstance(expect, str) else dict(expect), what or "rollout")


def check_update(expect, what=""):
    """expect: a kind, or a dict of words."""
    return _check(update(), dict(kind=expect) if isinstance(expect, int) else dict(expect), what or "update")


def check_gae(expect, what=""):
    return _check(gae(), dict(route=expect) if isinstance(expect, str) else dict(expect), what or "gae")
