"""The streaming stage of the search without a GPU: where GulpSearch.feed cuts a piece (search.gulp_cuts, plain
arithmetic), and the entry points' answer to a missing handle."""
import ctypes as C
import importlib

import pytest

from helpers import libpb

search = importlib.import_module("vlite-fast_amd.search")
cuts = search.gulp_cuts


def test_cuts_by_hand():
    N = 512
    # smaller than the gulp: one part, no fire; then the part that completes the gulp fires
    assert cuts(0, 100, N) == [(0, 100, False)]
    assert cuts(100, 411, N) == [(0, 411, False)]
    assert cuts(100, 412, N) == [(0, 412, True)]                 # a cut exactly at the gulp's end: no empty part after it
    assert cuts(100, 413, N) == [(0, 412, True), (412, 1, False)]
    # equal to the gulp
    assert cuts(0, N, N) == [(0, N, True)]
    assert cuts(1, N, N) == [(0, N - 1, True), (N - 1, 1, False)]
    # several times the gulp
    assert cuts(0, 3 * N, N) == [(0, N, True), (N, N, True), (2 * N, N, True)]
    assert cuts(500, 2 * N + 20, N) == [(0, 12, True), (12, N, True), (12 + N, N, True), (12 + 2 * N, 8, False)]
    assert cuts(500, 2 * N + 12, N) == [(0, 12, True), (12, N, True), (12 + N, N, True)]
    assert cuts(500, N + 11, N) == [(0, 12, True), (12, N - 1, False)]
    # an empty piece
    assert cuts(0, 0, N) == [] and cuts(511, 0, N) == []
    # a gulp of one sample fires after every sample
    assert cuts(0, 3, 1) == [(0, 1, True), (1, 1, True), (2, 1, True)]


def test_cuts_tile_the_piece_and_fire_every_gulp():
    import random
    rnd = random.Random(7)
    for _ in range(300):
        N = rnd.randint(1, 40)
        since, fired, total = 0, 0, 0
        for _ in range(rnd.randint(1, 12)):
            n = rnd.choice([0, 1, N - 1, N, N + 1, 3 * N, rnd.randint(0, 100)])
            parts = cuts(since, n, N)
            assert [p[0] for p in parts] == [sum(q[1] for q in parts[:i]) for i in range(len(parts))]
            assert sum(p[1] for p in parts) == n and all(p[1] > 0 for p in parts)
            for _, k, fire in parts:
                since += k
                assert since <= N and fire == (since == N)
                if fire:
                    since, fired = 0, fired + 1
            total += n
        assert fired == total // N and since == total % N


def test_cuts_refuse_nonsense():
    for bad in ((0, 1, 0), (5, 1, 5), (-1, 1, 5), (0, -1, 5)):
        with pytest.raises(ValueError):
            cuts(*bad)


def test_no_handle_is_refused_with_a_message():
    L = libpb().load()
    n, t, fill = C.c_int(), C.c_int(), C.c_int()
    buf = (C.c_int32 * 4)()
    byte = (C.c_uint8 * 8)()
    calls = [lambda: L.pb_search_push(None, byte, 0, 1, 8, C.byref(fill)),
             lambda: L.pb_search_gulp_peaks(None, C.c_float(6.0), buf, 1, C.byref(n), C.byref(t)),
             lambda: L.pb_search_gulp_advance(None, 0),
             lambda: L.pb_search_set_gulp(None, 16),
             lambda: L.pb_search_gulp_run(None, None, None, None, None, C.byref(t)),
             lambda: L.pb_search_gulp_fetch(None, byte, 8, C.byref(fill))]
    for call in calls:
        assert call() == -22                                        # PB_EINVAL
        assert b"no search handle" in L.pb_search_last_error(None)
    assert L.pb_search_gulp_timers(None, (C.c_float * 3)()) == -22
