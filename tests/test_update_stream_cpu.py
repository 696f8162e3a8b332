"""CPU: the size of the pre-gathered minibatch stream of the update (icrl_ppo_stream_ws_bytes: host arithmetic, no launch) and what it
refuses, each with a reason."""
import ctypes

import pytest

from helpers.update_stream import SHAPES, stream_bytes


def _ask(O, A, AS, T, N, B, E, discrete=0, h=64, arch=None, pad=0):
    from icrl_amd import _lib, structs as S
    L = _lib.lib()
    pol = S.PolicyT(O, A, h, h, discrete, 1, None, None, arch)
    buf = S.BufferT(T, N, O, AS)
    hp = S.PpoHyperT(B, E, 0, pad)
    return L, int(L.icrl_ppo_stream_ws_bytes(ctypes.byref(pol), ctypes.byref(buf), ctypes.byref(hp)))


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_stream_bytes_of_the_test_shapes(name):
    O, A, AS, disc, T, N, B, E = SHAPES[name]
    L, got = _ask(O, A, AS, T, N, B, E, disc)
    assert got == stream_bytes(O, AS, T * N, B, E) and got % 16 == 0
    assert L.icrl_last_error() == b""
    # the two-part form of the kernel (hp._pad & 32) and the phase timers (& 1) read the same stream
    assert _ask(O, A, AS, T, N, B, E, disc, pad=32 | 1)[1] == got


def test_flagship_size():
    """HCWithPos, 64 envs x 2048 steps, batch 64, 10 epochs: 20 480 chunks (+1) x 4 records x 1 984 B, 20 482 table entries."""
    _, got = _ask(18, 6, 6, 2048, 64, 64, 10)
    assert got == 4 * 20481 * 1984 + 16 * 20482 == stream_bytes(18, 6, 2048 * 64, 64, 10)


def test_what_the_stream_does_not_serve_says_why():
    import numpy as np
    L, got = _ask(113, 8, 8, 16, 8, 64, 2)
    assert got == 0 and b"obs_dim 113" in L.icrl_last_error() and b"obs_dim 1..32" in L.icrl_last_error()
    L.icrl_clear_error()
    arch = np.ascontiguousarray([1, 48, 1, 64, 1, 40, 0], dtype=np.int32)
    L, got = _ask(18, 6, 6, 16, 8, 64, 2, h=0, arch=arch.ctypes.data)
    assert got == 0 and b"`arch` descriptor" in L.icrl_last_error()
    L.icrl_clear_error()
    L, got = _ask(18, 6, 6, 16, 8, 257, 2)
    assert got == 0 and b"batch_size 257 (2..256)" in L.icrl_last_error()
    L.icrl_clear_error()
    L, got = _ask(18, 6, 6, 16, 8, 64, 2, pad=16)       # the wave-pair kernel was asked for
    assert got == 0 and b"another update kernel" in L.icrl_last_error()
    L.icrl_clear_error()
    L, got = _ask(18, 6, 6, 4096, 1024, 64, 10)         # 4 M rows x 10 epochs x 124 B: beyond 32-bit byte offsets
    assert got == 0 and b"32-bit byte offsets" in L.icrl_last_error()
    L.icrl_clear_error()
