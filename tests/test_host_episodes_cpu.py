"""CPU: the ABI of the episode loop over host envs (icrl_host_episode_step / icrl_host_episode_t) and its switch in the README."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, "include", "icrl_hip.h")).read()


def test_host_episode_struct_matches_the_header():
    from icrl_amd import structs as S
    body = re.search(r"typedef struct icrl_host_episode_t \{(.*?)\} icrl_host_episode_t;", _header(), re.S).group(1)
    fields = re.findall(r"^\s*(?:const\s+)?(?:long\s+)?(\w+)\s*\*?\s*(\w+);", body, re.M)
    assert [f for _, f in fields] == [f for f, _ in S.HostEpisodeT._fields_]
    ctype = {"int": ctypes.c_int32, "void": ctypes.c_void_p, "float": ctypes.c_void_p, "double": ctypes.c_void_p}
    assert [ctype[t] for t, _ in fields] == [t for _, t in S.HostEpisodeT._fields_]      # (every non-int member is a pointer)
    assert ctypes.sizeof(S.HostEpisodeT) == 4 * 4 + 5 * 8


def test_host_episode_step_is_declared_and_listed():
    from icrl_amd import _lib
    decl = re.search(r"int icrl_host_episode_step\((.*?)\);", _header(), re.S)
    assert decl is not None
    params = [a.strip() for a in decl.group(1).split(",")]
    sig = _lib.SIGNATURES["icrl_host_episode_step"]
    assert len(sig) == len(params) == 9
    for a, t in zip(params, sig):
        assert t is (ctypes.c_void_p if "*" in a else ctypes.c_int), a
    assert "icrl_host_episode_step" not in _lib.RESTYPES         # returns int (hipError_t), like its neighbours
    # an additive change: the ABI version stays where icrl_host_step left it
    assert "icrl_abi_version(void) { return 107; }" in open(os.path.join(ROOT, "icrl_amd", "csrc", "gae.hip")).read()


def test_readme_documents_the_switch():
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "ICRL_HOST_EPISODES_STEPPED" in readme
    assert "Sampling and evaluation run the reference's per-step episode loop" not in readme


def test_dispatch_predicate_needs_no_gpu():
    """host_episodes_ok only looks at the chain and the policy's shape; the switch turns it off."""
    from icrl_amd import utils
    src = open(os.path.join(ROOT, "icrl_amd", "utils.py")).read()
    assert "ICRL_HOST_EPISODES_STEPPED" in src and hasattr(utils, "HostEpisodeRun") and hasattr(utils, "host_episodes_ok")
    assert utils.host_episodes_ok(None, object()) is False        # not a VecNormalize chain: no attribute of the agent is read
