"""CPU (-m "not gpu"): the piece arithmetic of zjni_compress_pieces_batch_device (zstd-jni_amd/csrc/zj_frames.h), built lane-serial from tests/emu_pieces/emu_pieces.cpp,
against a plain-Python restatement of the rules of include/zjni_amd.h.

A cut list is legal when d_cut_off ascends at the buffer, the cuts ascend strictly, every cut lies in (0, size) and no piece exceeds the chunk size; the pieces are the gaps.
A buffer with an illegal list answers 42 and owns no entry of the caller's index; inside the call it is walked on the fixed grid (its frames go nowhere), because an
entry ends where the next one begins and its bytes lie between its neighbours'.  Checked: the count kernel's verdict and both entry counts, the emit kernel's source
offsets and scratch destinations whole and in slices, where every walked entry lies in the caller's index, and zjni_compressBound_pieces against the summed
zjni_compressBound.  The -m gpu twin is tests/test_gpu_pieces.py."""
import ctypes as C
import os
import random

import numpy as np
import pytest

from pieces_cases import bound, illegal, lay_out, legal
from util import emu_so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAXU = (1 << 64) - 1
ERR42 = (1 << 64) - 42
CHUNK = 1000


def _load(name, sub):
    return C.CDLL(emu_so(sub, name))


@pytest.fixture(scope="module")
def emu():
    L = _load("libzjni_emu_pieces.so", "emu_pieces")
    vp, ull = C.c_void_p, C.c_ulonglong
    L.emu_pieces_count.restype = ull
    L.emu_pieces_count.argtypes = [vp, C.c_uint, ull, vp, vp, vp, vp, vp]
    L.emu_pieces_emit.restype = None
    L.emu_pieces_emit.argtypes = [vp, vp, vp, C.c_uint, ull, vp, vp, ull, C.c_uint, ull, vp, vp]
    L.emu_pieces_index.restype = None
    L.emu_pieces_index.argtypes = [vp, vp, C.c_uint, ull, C.c_uint, vp]
    L.emu_entry_owner.restype = ull
    L.emu_entry_owner.argtypes = [vp, ull, ull]
    L.emu_pieces_bound.restype = ull
    L.emu_pieces_bound.argtypes = [ull, ull]
    L.emu_compress_bound.restype = ull
    L.emu_compress_bound.argtypes = [ull]
    return L


@pytest.fixture(scope="module")
def emu_frames():
    L = _load("libzjni_emu_frames.so", "emu_frames")
    L.emu_chunks_count.restype = C.c_ulonglong
    L.emu_chunks_count.argtypes = [C.c_void_p, C.c_uint, C.c_ulonglong, C.c_void_p, C.c_void_p]
    L.emu_chunks_emit.restype = None
    L.emu_chunks_emit.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint, C.c_ulonglong, C.c_ulonglong, C.c_uint, C.c_ulonglong, C.c_void_p, C.c_void_p]
    return L


def u64(values):
    return np.array(list(values), dtype=np.uint64)


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


# ------------------------------------------------------------------------------------------------ what the kernels must say
def grid(size, chunk):
    return list(range(chunk, size, chunk))


def expect(buffers, chunk, lead=7):
    """buffers: (size, cuts or None for the fixed grid, d_cut_off ascends) -> what the kernels must say"""
    first, ifirst, ferr, src = [0], [0], [], []
    lo = lead
    for size, cuts, asc in buffers:
        ok = cuts is None or legal(size, cuts, chunk, asc)
        starts = [0] + (grid(size, chunk) if (cuts is None or not ok) else list(cuts))
        src += [lo + s for s in starts]
        first.append(first[-1] + len(starts))
        ifirst.append(ifirst[-1] + (len(starts) if ok else 0))
        ferr.append(0 if ok else ERR42)
        lo += size
    return first, ifirst, ferr, src + [lo]


def arrays(buffers, lead=7, null=False):
    off = u64(np.cumsum([lead] + [b[0] for b in buffers]))
    if null:
        return off, None, None
    flat, cut_off = lay_out([(b[1], b[2]) for b in buffers])
    return off, u64(flat), u64(cut_off)


def run_count(emu, buffers, chunk, null=False):
    n = len(buffers)
    off, cut, cut_off = arrays(buffers, null=null)
    first, ifirst, ferr = np.zeros(n + 1, np.uint64), np.zeros(n + 1, np.uint64), np.zeros(n, np.uint64)
    E = emu.emu_pieces_count(ptr(off), n, chunk, ptr(cut) if cut is not None else None, ptr(cut_off) if cut is not None else None, ptr(first), ptr(ifirst), ptr(ferr))
    return off, cut, cut_off, first, ifirst, ferr, E


def run_emit(emu, off, cut, cut_off, first, ifirst, n, chunk, a, m, E):
    s, d = np.full(m + 1, MAXU, np.uint64), np.full(m + 1, MAXU, np.uint64)
    emu.emu_pieces_emit(ptr(off), ptr(first), ptr(ifirst), n, chunk, ptr(cut) if cut is not None else None, ptr(cut_off) if cut is not None else None, a, m, E, ptr(s), ptr(d))
    return s.tolist(), d.tolist()


def check(emu, buffers, chunk, slices=()):
    n = len(buffers)
    off, cut, cut_off, first, ifirst, ferr, E = run_count(emu, buffers, chunk)
    wf, wi, we, wsrc = expect(buffers, chunk)
    assert first.tolist() == wf and ifirst.tolist() == wi and ferr.tolist() == we and E == wf[-1]
    s, d = run_emit(emu, off, cut, cut_off, first, ifirst, n, chunk, 0, E, E)
    assert s == wsrc and d == [j * bound(chunk) for j in range(E + 1)]
    for a, m in slices:
        s, d = run_emit(emu, off, cut, cut_off, first, ifirst, n, chunk, a, m, E)
        assert s == [wsrc[min(a + j, E)] for j in range(m + 1)], (a, m)
        assert d == [j * bound(chunk) for j in range(m + 1)], (a, m)
    # the caller's index: entries of legal buffers in order without gaps, entries of illegal ones nowhere
    at = np.zeros(max(E, 1), np.uint64)
    emu.emu_pieces_index(ptr(first), ptr(ifirst), n, 0, E, ptr(at))
    want = []
    for i in range(n):
        k = wf[i + 1] - wf[i]
        want += [wi[i] + j for j in range(k)] if wi[i + 1] > wi[i] else [MAXU] * k
    assert at.tolist()[:E] == want
    assert [x for x in want if x != MAXU] == list(range(wi[-1]))
    return wf, wi


def cuts_of(sizes):
    return list(np.cumsum(sizes)[:-1]), int(sum(sizes))


# ------------------------------------------------------------------------------------------------ tests
def test_legal_lists(emu):
    c = CHUNK
    lists = [[1], [1, 1, 1], [255], [255, 1, 255], [c], [c, c], [c - 1], [c - 1, c, 1], [1, 255, c, c - 1, 7], [c] * 70, [1] * 130, [3, c] * 40]
    buffers = []
    for sizes in lists:
        cuts, size = cuts_of(sizes)
        buffers.append((size, cuts, True))
    wf, wi = check(emu, buffers, c)
    assert wf == wi and [wf[i + 1] - wf[i] for i in range(len(lists))] == [len(x) for x in lists]


ILLEGAL = illegal(CHUNK)


@pytest.mark.parametrize("kind", sorted(ILLEGAL))
def test_illegal_list_alone_and_between_neighbours(emu, kind):
    bad = ILLEGAL[kind]
    assert not legal(bad[0], bad[1], CHUNK, bad[2])
    good_a = (sum([1, 255, 7]), cuts_of([1, 255, 7])[0], True)
    good_b = (CHUNK, [], True)
    wf, wi = check(emu, [bad], CHUNK)
    assert wi == [0, 0] and wf[1] == max(1, -(-bad[0] // CHUNK))
    wf, wi = check(emu, [good_a, bad, good_b, bad, bad, good_a], CHUNK, slices=[(0, 2), (2, 3), (3, wf[1]), (1, 5)])
    assert wi == [0, 3, 3, 4, 4, 4, 7]


def test_empty_buffers(emu):
    wf, wi = check(emu, [(0, [], True), (5, [2], True), (0, [], True), (0, [], True)], CHUNK)
    assert wf == wi == [0, 1, 3, 4, 5]


def test_owner_search_over_repeated_values(emu):
    """the caller's index has buffers without entries: the owner of entry e is still the last i with ifirst[i] <= e, the buffer that holds it"""
    ifirst = u64([0, 3, 3, 3, 4, 4, 9, 9])
    for e, owner in ((0, 0), (2, 0), (3, 3), (4, 5), (8, 5)):
        assert emu.emu_entry_owner(ptr(ifirst), 7, e) == owner


def test_null_list_is_the_fixed_grid(emu, emu_frames):
    for chunk in (256, 1000, 131072):
        sizes = [0, 1, chunk - 1, chunk, chunk + 1, 3 * chunk + 5, 0, 7 * chunk]
        buffers = [(s, None, True) for s in sizes]
        n = len(sizes)
        off, cut, cut_off, first, ifirst, ferr, E = run_count(emu, buffers, chunk, null=True)
        f2, bbase = np.zeros(n + 1, np.uint64), np.zeros(n + 1, np.uint64)
        assert emu_frames.emu_chunks_count(ptr(off), n, chunk, ptr(f2), ptr(bbase)) == E
        assert first.tolist() == ifirst.tolist() == f2.tolist() and not ferr.any()
        for a, m in ((0, E), (0, 3), (3, 4), (E - 2, 2), (5, E - 5)):
            s, d = run_emit(emu, off, None, None, first, ifirst, n, chunk, a, m, E)
            s2, d2 = np.zeros(m + 1, np.uint64), np.zeros(m + 1, np.uint64)
            emu_frames.emu_chunks_emit(ptr(off), ptr(f2), ptr(bbase), n, chunk, a, m, E, ptr(s2), ptr(d2))
            assert s == s2.tolist(), (chunk, a, m)                       # the same pieces of the source
            assert d == [j * bound(chunk) for j in range(m + 1)]          # each in a scratch destination of the full bound: never less than emu_chunks_emit's
            assert all(x >= y for x, y in zip(d, d2.tolist()))


def test_slices(emu):
    rnd = random.Random(5)
    buffers = []
    for i in range(40):
        sizes = [rnd.choice((1, 7, 255, CHUNK, CHUNK - 1, rnd.randrange(1, CHUNK + 1))) for _ in range(rnd.randrange(1, 90))]
        cuts, size = cuts_of(sizes)
        buffers.append((size, cuts, True))
        if i % 7 == 3:
            buffers.append(ILLEGAL[sorted(ILLEGAL)[i % len(ILLEGAL)]])
    wf, wi, _, _ = expect(buffers, CHUNK)
    E = wf[-1]
    S = 97
    slices = [(a, min(S, E - a)) for a in range(0, E, S)]                # a and m wherever they fall, the last slice with the sentinel
    slices += [(wf[3], wf[5] - wf[3]), (wf[3] + 1, 2), (wf[10], E - wf[10]), (E - 1, 1)]      # at buffer boundaries, inside a buffer, the end
    check(emu, buffers, CHUNK, slices=slices)


def test_bound_covers_the_pieces(emu):
    rnd = random.Random(14)
    for s in (0, 1, 255, 256, 131071, 131072, 131073, 1 << 20):
        assert emu.emu_compress_bound(s) == bound(s)
    assert emu.emu_pieces_bound(0, 0) == 64 and emu.emu_pieces_bound(1000, 1) == 1000 + 3 + 64
    for _ in range(1000):
        chunk = rnd.choice((256, 1000, 4096, 65536, 131072))
        pieces = [rnd.choice((1, 7, 255, chunk, chunk - 1, rnd.randrange(1, chunk + 1))) for _ in range(rnd.randrange(1, 200))]
        size = sum(pieces)
        assert emu.emu_pieces_bound(size, len(pieces)) >= sum(bound(p) for p in pieces), (chunk, len(pieces))
    assert emu.emu_pieces_bound(0, 1) >= bound(0)
