"""CPU (-m "not gpu"): the arithmetic of indexed range reads (zstd-jni_amd/csrc/zj_index.h), built lane-serial from tests/emu_index/emu_index.cpp.

BUILDERS: the scan and the legality rules against a model in plain Python, from-pieces against from-sizes on the cut lists of tests/pieces_cases.py.  PLAN CHECK:
for every buffer of tests/inspect_cases.py and tests/test_emu_frames.py that the walked entry indexes, the true index from the reference's
ZSTD_findFrameCompressedSize / ZSTD_getFrameContentSize, and every range whose ends come from {0, every entry boundary - 1 / + 0 / + 1, T, T + 1, 2^64 - 1}: with one
request per buffer the record, the entry arrays and the copy runs must equal those of the walked entry's emulation (tests/emu_frames_range, imported, the oracle
here).  PLAN EXECUTION: the reference decodes every planned entry into simulated slots and scratch; result and every byte, the 0xCD fill included, must be "the
reference decodes the buffer, sliced".  REQUESTS: many per buffer, overlapping, out of buffer order, b >= n, a coarse index, entries of no content.  FALSE INDEXES:
the codes the header names, and for indexes of random words every offset the plan produces inside the buffer's extent and the request's slot.
The -m gpu twin is tests/test_gpu_index.py."""
import ctypes as C
import itertools
import os
import random

import numpy as np
import pytest

import pieces_cases as pc
from util import emu_so
import test_emu_frames_range as fr
from test_emu_frames_range import Rec, arr, ptr, MAXU, ERROR, FILL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZE_MAX = (1 << 32) - 1
world = fr.world


class Req(C.Structure):
    """ZIReq (zj_index.h)"""
    _fields_ = [(f, C.c_uint64) for f in ("e0", "cBase", "uBase", "srcLo")]


def _load(directory, name):
    return C.CDLL(emu_so(directory, name))


@pytest.fixture(scope="module")
def range_emu():
    L = _load("emu_frames_range", "libzjni_emu_frames_range.so")
    vp = C.c_void_p
    L.emu_range_count.restype = None
    L.emu_range_count.argtypes = [vp, vp, vp, vp, C.c_uint, vp, vp, vp]
    L.emu_range_emit.restype = None
    L.emu_range_emit.argtypes = [vp, vp, vp, vp, vp, C.c_uint, vp, vp, vp, vp, vp, vp]
    return L


@pytest.fixture(scope="module")
def emu():
    L = _load("emu_index", "libzjni_emu_index.so")
    vp, ull = C.c_void_p, C.c_ulonglong
    L.emu_index_bytes.restype = ull
    L.emu_index_bytes.argtypes = [ull, ull]
    L.emu_index_from_sizes.restype = None
    L.emu_index_from_sizes.argtypes = [ull, vp, vp, vp, vp, ull, vp]
    L.emu_index_from_pieces.restype = None
    L.emu_index_from_pieces.argtypes = [vp, ull, ull, vp, vp, vp, vp, vp, ull, vp]
    L.emu_index_request.restype = None
    L.emu_index_request.argtypes = [vp, ull, ull, vp, vp, vp, C.c_uint, vp, vp, vp, vp, vp]
    L.emu_index_emit.restype = None
    L.emu_index_emit.argtypes = [vp, ull, ull, vp, vp, vp, vp, vp, C.c_uint, vp, vp, vp, vp, vp, vp]
    L.emu_index_finish.restype = None
    L.emu_index_finish.argtypes = [vp, ull, ull, vp, vp, vp, vp, vp, vp, vp, C.c_uint, vp, vp]
    assert L.emu_index_rec_bytes() == C.sizeof(Rec) and L.emu_index_req_bytes() == C.sizeof(Req)
    return L


# ------------------------------------------------------------------------------------------------ the index, in plain Python
def model_index(first, sizes, contents, results=None):
    """zjni_index_from_sizes_device's rules: the words of the index"""
    n, E = len(first) - 1, len(sizes)
    valid = []
    for i in range(n):
        ok = first[i] <= first[i + 1] <= E
        ok = ok and all(sizes[e] <= SIZE_MAX and contents[e] <= SIZE_MAX for e in range(first[i], first[i + 1]))
        code = 0 if ok else 42
        if results is not None and results[i] > 1 << 40:
            code = (1 << 64) - results[i]
        valid.append(code)
    c, u = [0], [0]
    for s, t in zip(sizes, contents):
        c.append(c[-1] + (s if s <= SIZE_MAX else 0))
        u.append(u[-1] + (t if t <= SIZE_MAX else 0))
    return list(first) + valid + c + u


def true_index(cases):
    """the index of a batch of indexable buffers, an entry a frame, written by hand (a caller may): no limit on an entry's content"""
    first, sizes, contents = [0], [], []
    for c in cases:
        sizes += [f[1] for f in c.frames]
        contents += [f[2] for f in c.frames]
        first.append(len(sizes))
    cs, us = list(itertools.accumulate([0] + sizes)), list(itertools.accumulate([0] + contents))
    return first + [0] * len(cases) + cs + us, len(sizes)


def run_index(emu, words, n, E, src_off, requests, dst_off):
    """the request kernel, the scans and the emit kernels: what fr.run_emu returns for the walked entry, plus what the finish kernel needs"""
    R = len(requests)
    idx = arr([w & MAXU for w in words] + [0xDEAD] * 4)
    rec, ireq, bad = (Rec * max(R, 1))(), (Req * max(R, 1))(), np.zeros(max(R, 1), dtype=np.uint32)
    scan, total = np.zeros(5 * (R + 1), dtype=np.uint64), np.zeros(max(R, 1), dtype=np.uint64)
    off, doff, req = arr(src_off), arr(dst_off), arr([v for r in requests for v in r] + [0])
    emu.emu_index_request(ptr(idx), n, E, ptr(off), ptr(req), ptr(doff), R, C.byref(rec), C.byref(ireq), ptr(bad), ptr(scan), ptr(total))
    tot = [int(scan[k * (R + 1) + R]) for k in range(5)]
    ea, eb = tot[0], tot[1]
    a_s, a_d = np.full(ea + 1, 0xDEAD, dtype=np.uint64), np.full(ea + 1, 0xDEAD, dtype=np.uint64)
    b_s, b_d = np.full(eb + 1, 0xDEAD, dtype=np.uint64), np.full(eb + 1, 0xDEAD, dtype=np.uint64)
    cin, cout = np.full(9 * R + 3, 0xDEAD, dtype=np.uint64), np.full(6 * R + 3, 0xDEAD, dtype=np.uint64)
    if R:
        emu.emu_index_emit(ptr(idx), n, E, C.byref(rec), C.byref(ireq), ptr(bad), ptr(scan), ptr(doff), R, ptr(a_s), ptr(a_d), ptr(b_s), ptr(b_d), ptr(cin), ptr(cout))
    triples = lambda a, k: [tuple(int(x) for x in a[3 * j:3 * j + 3]) for j in range(k)]      # noqa: E731
    lst = lambda a: [int(x) for x in a]      # noqa: E731
    state = dict(idx=idx, rec=rec, ireq=ireq, bad=bad, scan=scan, cout=cout, n=n, E=E, R=R)
    return rec, lst(total)[:R], tot, lst(a_s), lst(a_d), lst(b_s), lst(b_d), triples(cin, 3 * R), triples(cout, 2 * R), state


def finish(emu, state, res_a, res_b):
    R = state["R"]
    result, stat = np.zeros(max(R, 1), dtype=np.uint64), np.zeros(4, dtype=np.uint32)
    ra, rb = arr(list(res_a) + [0]), arr(list(res_b) + [0])
    emu.emu_index_finish(ptr(state["idx"]), state["n"], state["E"], C.byref(state["rec"]), C.byref(state["ireq"]), ptr(state["bad"]), ptr(state["scan"]), ptr(ra), ptr(rb),
                         ptr(result), R, ptr(state["cout"]), ptr(stat))
    cout = [tuple(int(x) for x in state["cout"][3 * j:3 * j + 3]) for j in range(2 * R)]
    signed = [int(x) - (1 << 64) if int(x) > 1 << 63 else int(x) for x in result[:R]]
    return signed, cout, [int(x) for x in stat]


def same_plan(mine, theirs, what):
    rec, total, tot, a_s, a_d, b_s, b_d, cin, cout = mine[:9]
    rec2, total2, tot2, a_s2, a_d2, b_s2, b_d2, cin2, cout2 = theirs
    assert total == total2 and tot == tot2, what
    for i in range(len(total)):
        for f in fr.REC_FIELDS + ("status", "frames", "edges"):
            if rec2[i].status != 0 and f not in ("status", "total", "lo", "hi"):
                continue                                    # (nothing selected: the walked record keeps what its walk passed)
            assert getattr(rec[i], f) == getattr(rec2[i], f), (what, i, f)
    assert (a_s, a_d, b_s, b_d) == (a_s2, a_d2, b_s2, b_d2), what
    assert cin == cin2 and cout == cout2, what


def decode(w, z, cap, use_dict):
    if not z:
        return -72
    key = (z, cap, use_dict)
    if key not in w.entry_cache:
        try:
            w.entry_cache[key] = w.ref.decompress_using_dict(z, w.dictionary, cap) if use_dict else w.ref.decompress(z, cap)
        except w.ref.ZstdRefError as e:
            w.entry_cache[key] = -e.code
    return w.entry_cache[key]


def execute(emu, w, cases, blob, plan, requests, dst_off):
    """the gathers in Python, every entry by the reference, the finish rule by the emulation: (results, the destination with 64 bytes beyond its end)"""
    rec, total, tot, a_s, a_d, b_s, b_d, cin, cout, state = plan
    R = len(requests)
    scan = [int(x) for x in state["scan"]]
    f_a, f_b = scan[:R + 1], scan[R + 1:2 * (R + 1)]
    compact, scratch = bytearray(b"\xEE" * b_s[-1]), bytearray(b"\xEE" * b_d[-1])
    dst = bytearray(bytes([FILL]) * (dst_off[-1] + 64))
    for key, other, length in cin:
        compact[key:key + length] = blob[other:other + length]
    res = {}
    for tag, s_off, d_off, base, firsts in (("A", a_s, a_d, dst, f_a), ("B", b_s, b_d, scratch, f_b)):
        res[tag] = []
        for e in range(len(s_off) - 1):
            owner = max(r for r in range(R) if firsts[r] <= e)
            closing = tag == "A" and e == f_a[owner + 1] - 1
            z, cap = bytes(compact[s_off[e]:s_off[e + 1]]), max(d_off[e + 1] - d_off[e], 0)
            if closing:
                assert z == b""
                res[tag].append(0)
                continue
            b = requests[owner][0]
            got = decode(w, z, cap, cases[b].dict)
            res[tag].append(len(got) if not isinstance(got, int) else (1 << 64) + got)
            if not isinstance(got, int):
                assert len(got) <= cap
                base[d_off[e]:d_off[e] + len(got)] = got
    results, cout2, stat = finish(emu, state, res["A"], res["B"])
    for key, other, length in cout2:
        dst[other:other + length] = scratch[key:key + length]
    return results, dst, stat


def whole_of(w, c):
    """the reference's decode of every frame of the buffer, joined: bytes, with '?' where a frame answers an error; and the frames' answers"""
    parts = [w.frame(c, k) for k in range(len(c.frames))]
    return b"".join(p if not isinstance(p, int) else b"?" * c.frames[k][2] for k, p in enumerate(parts)), parts


def check_execution(w, cases, requests, dst_off, results, dst, ends=True):
    for r, (b, lo, length) in enumerate(requests):
        c = cases[b]
        lo2, hi2 = min(lo, c.T), min(lo + length, MAXU, c.T)
        slot = bytes(dst[dst_off[r]:dst_off[r + 1]])
        whole, parts = whole_of(w, c)
        pre, sel = 0, []
        for k, f in enumerate(c.frames):
            if f[2] and pre < hi2 and pre + f[2] > lo2:
                sel.append(k)
            pre += f[2]
        codes = [parts[k] for k in range(sel[0], sel[-1] + 1) if isinstance(parts[k], int)] if sel else []
        if lo2 == hi2:
            assert results[r] == 0 and slot == bytes([FILL]) * len(slot), (c.name, requests[r])
        elif len(slot) < hi2 - lo2:
            assert results[r] == -70 and slot == bytes([FILL]) * len(slot), (c.name, requests[r])
        elif codes:
            assert results[r] == codes[0], (c.name, requests[r])
            assert slot[hi2 - lo2:] == bytes([FILL]) * (len(slot) - (hi2 - lo2))
        else:
            assert results[r] == hi2 - lo2 and slot[:hi2 - lo2] == whole[lo2:hi2], (c.name, requests[r])
            assert slot[hi2 - lo2:] == bytes([FILL]) * (len(slot) - (hi2 - lo2)), (c.name, requests[r])
    assert not ends or (bytes(dst[:dst_off[0]]) == bytes([FILL]) * dst_off[0] and bytes(dst[dst_off[-1]:]) == bytes([FILL]) * 64)


@pytest.fixture(scope="module")
def good(world):
    """the buffers the walked entry indexes"""
    world.entry_cache = {}
    cases = [c for c in world.cases if c.code == 0]
    assert len(cases) > 20 and any(len(c.frames) == 40 for c in cases) and any(any(f[2] == 0 for f in c.frames) for c in cases)
    return cases


def lay(cases, lead=3):
    blob = b"\xAA" * lead + b"".join(c.data for c in cases)
    return blob, np.cumsum([lead] + [len(c.data) for c in cases]).tolist()


# ------------------------------------------------------------------------------------------------ builders
def test_index_bytes_and_layout(emu):
    for n, E in ((0, 0), (1, 0), (1, 1), (5, 1023), (3, 100000)):
        b = emu.emu_index_bytes(n, E)
        assert b % 256 == 0 and 0 <= b - 8 * (2 * n + 1 + 2 * (E + 1)) < 256


def test_from_sizes_scan_and_legality(emu):
    rnd = random.Random(7)
    wg = emu.emu_index_scan_wg()
    assert wg == 1024
    for E in (0, 1, 2, wg - 1, wg, wg + 1, 2 * wg - 1, 2 * wg, 2 * wg + 1, 3 * wg + 7, 5000):
        for n in (0, 1, 3, 7):
            sizes = [rnd.choice((0, 1, 9, 300, 70000, SIZE_MAX)) for _ in range(E)]
            contents = [rnd.choice((0, 0, 1, 256, 4096, 131072, SIZE_MAX)) for _ in range(E)]
            first = sorted(rnd.randint(0, E) for _ in range(n + 1))
            if n:
                first[0], first[n] = 0, E
            else:
                first = [E]
            words = np.full(emu.emu_index_bytes(n, E) // 8, 0xDEAD, dtype=np.uint64)
            emu.emu_index_from_sizes(n, ptr(arr(first)), ptr(arr(sizes + [0])), ptr(arr(contents + [0])), None, E, ptr(words))
            want = model_index(first, sizes, contents)
            assert [int(x) for x in words[:len(want)]] == want, (n, E)
            assert all(v == 0 for v in want[n + 1:2 * n + 1])


def test_from_sizes_illegal_buffers_leave_the_others_alone(emu):
    E = 30
    sizes, contents = [20 + e for e in range(E)], [100 * e for e in range(E)]
    first = [0, 5, 4, 12, 40, 25, 30]                       # buffer 1 descends; buffer 3 ends beyond E; buffer 4 descends from it
    sizes[27], contents[13] = SIZE_MAX + 1, 1 << 40        # buffer 5 and buffer 3 hold an oversized entry
    contents[2] = SIZE_MAX                                 # the maximum itself is legal
    words = np.zeros(emu.emu_index_bytes(6, E) // 8, dtype=np.uint64)
    emu.emu_index_from_sizes(6, ptr(arr(first)), ptr(arr(sizes)), ptr(arr(contents)), None, E, ptr(words))
    want = model_index(first, sizes, contents)
    assert [int(x) for x in words[:len(want)]] == want
    assert want[7:13] == [0, 42, 0, 42, 42, 42]
    # a buffer's own error answers before the legality of its entries
    results = [10, MAXU + 1 - 70, 10, 10, MAXU + 1 - 64, 10]
    emu.emu_index_from_sizes(6, ptr(arr(first)), ptr(arr(sizes)), ptr(arr(contents)), ptr(arr(results)), E, ptr(words))
    assert [int(x) for x in words[7:13]] == [0, 70, 0, 42, 64, 42]


def test_from_pieces_against_from_sizes(emu):
    """the cut lists of tests/pieces_cases.py, legal and illegal, and the fixed grid: the content sizes are the gaps between the cuts"""
    chunk = 1024
    rnd = random.Random(3)
    lists = [(900, [300, 600], True), (0, [], True), (chunk, [], True), (3000, [1000, 1024, 2048], True), (1, [], True), (2500, [1, 2, 1026, 2050], True)]
    bad = sorted(pc.illegal(chunk).items())
    for with_bad in (False, True):
        bufs = list(lists)
        if with_bad:
            for k, (_, spec) in enumerate(bad):
                bufs.insert(1 + 2 * k % len(bufs), spec)
        sizes_src = [b[0] for b in bufs]
        src_off = np.cumsum([11] + sizes_src).tolist()
        legal = [pc.legal(s, cuts, chunk, asc) and (bool(cuts) or s <= chunk) for s, cuts, asc in bufs]
        cut, cut_off = pc.lay_out([(cuts, asc) for _, cuts, asc in bufs])
        first, contents, results = [0], [], []
        for (s, cuts, _), ok in zip(bufs, legal):
            if ok:
                edges = [0] + list(cuts) + [s]
                contents += [b - a for a, b in zip(edges[:-1], edges[1:])]
            results.append(123 if ok else MAXU + 1 - 42)
            first.append(len(contents))
        E = len(contents)
        psize = [rnd.randint(9, 2000) for _ in range(E)]
        n = len(bufs)
        got = np.zeros(emu.emu_index_bytes(n, E) // 8, dtype=np.uint64)
        emu.emu_index_from_pieces(ptr(arr(src_off)), n, chunk, ptr(arr(cut)), ptr(arr(cut_off)), ptr(arr(results)), ptr(arr(first)), ptr(arr(psize)), E, ptr(got))
        want = np.zeros_like(got)
        emu.emu_index_from_sizes(n, ptr(arr(first)), ptr(arr(psize)), ptr(arr(contents + [0])), ptr(arr(results)), E, ptr(want))
        assert (got == want).all() and [int(x) for x in got[n + 1:2 * n + 1]] == [0 if ok else 42 for ok in legal]
        assert with_bad == (42 in [int(x) for x in got[n + 1:2 * n + 1]])
    # the fixed grid
    src = [0, 1, chunk - 1, chunk, chunk + 1, 5 * chunk, 5 * chunk + 7]
    src_off = np.cumsum([0] + src).tolist()
    contents, first = [], [0]
    for s in src:
        contents += [min(chunk, s - a) for a in range(0, max(s, 1), chunk)]
        first.append(len(contents))
    E, n = len(contents), len(src)
    psize = [rnd.randint(9, 2000) for _ in range(E)]
    got, want = np.zeros(emu.emu_index_bytes(n, E) // 8, dtype=np.uint64), np.zeros(emu.emu_index_bytes(n, E) // 8, dtype=np.uint64)
    emu.emu_index_from_pieces(ptr(arr(src_off)), n, chunk, None, None, None, ptr(arr(first)), ptr(arr(psize)), E, ptr(got))
    emu.emu_index_from_sizes(n, ptr(arr(first)), ptr(arr(psize)), ptr(arr(contents)), None, E, ptr(want))
    assert (got == want).all() and int(got[2 * n + 1 + 2 * E + 1]) == sum(src)


# ------------------------------------------------------------------------------------------------ plan check and plan execution
def test_one_request_per_buffer_equals_the_walked_entry(emu, range_emu, world, good):
    """every buffer, every range: records, entry arrays and copy runs of the walked entry's emulation; the plan executed for the buffers that are not huge"""
    w = world
    selected = executed = 0
    for c in good:
        words, E = true_index([c])
        small = c.T <= 1 << 22
        for j, (lo, length) in enumerate(fr.ranges_of(c)):
            want = min(lo + length, c.T) - min(lo, c.T)
            slot = (want + (j % 3) * 5 if j % 7 else max(want - 1, 0)) if small else want
            lead = j % 16
            blob, src_off = lay([c], lead)
            dst_off = [7, 7 + slot] if small else [0, slot]
            src = np.frombuffer(blob, dtype=np.uint8)
            mine = run_index(emu, words, 1, E, src_off, [(0, lo, length)], dst_off)
            theirs = fr.run_emu(range_emu, src, src_off, dst_off, [(lo, length)])
            same_plan(mine, theirs, (c.name, lo, length, slot))
            selected += mine[0][0].status == 0
            if small and (j % 3 == 0 or len(c.frames) < 8):
                results, dst, _ = execute(emu, w, [c], blob, mine, [(0, lo, length)], dst_off)
                check_execution(w, [c], [(0, lo, length)], dst_off, results, dst)
                executed += 1
    assert selected > 5000 and executed > 2000


def test_batches_equal_the_walked_entry(emu, range_emu, world, good):
    """many buffers in one call, a request each: bases in C and U that are not 0, the scans, the closing entries between the requests"""
    w = world
    pool = [c for c in good if c.T <= 1 << 22 and not c.name.startswith("random")]
    assert len(pool) > 30
    words, E = true_index(pool)
    blob, src_off = lay(pool, 5)
    src = np.frombuffer(blob, dtype=np.uint8)
    for rnd in range(10):
        ranges, slots = [], []
        for i, c in enumerate(pool):
            rs = fr.ranges_of(c)
            lo, length = rs[(rnd * 131 + i * 17) % len(rs)]
            want = min(lo + length, c.T) - min(lo, c.T)
            ranges.append((lo, length))
            slots.append(max(want - 1, 0) if (i + rnd) % 11 == 0 else want + (i % 4) * 3)
        dst_off = np.cumsum([9] + slots).tolist()
        requests = [(i, lo, length) for i, (lo, length) in enumerate(ranges)]
        mine = run_index(emu, words, len(pool), E, src_off, requests, dst_off)
        same_plan(mine, fr.run_emu(range_emu, src, src_off, dst_off, ranges), rnd)
        results, dst, stat = execute(emu, w, pool, blob, mine, requests, dst_off)
        check_execution(w, pool, requests, dst_off, results, dst)
        assert sum(r > 0 for r in results) >= 5 and stat[0] + stat[3] == len(pool)


# ------------------------------------------------------------------------------------------------ request handling
def coarse_index(cases, group):
    """an index whose entries are `group` frames each (the last of a buffer: what is left)"""
    first, sizes, contents = [0], [], []
    for c in cases:
        for k in range(0, len(c.frames), group):
            sizes.append(sum(f[1] for f in c.frames[k:k + group]))
            contents.append(sum(f[2] for f in c.frames[k:k + group]))
        first.append(len(sizes))
    return model_index(first, sizes, contents), len(sizes)


def test_many_requests_per_buffer_any_order_and_coarse_indexes(emu, world, good):
    w = world
    rnd = random.Random(11)
    pool = [c for c in good if 3 <= len(c.frames) <= 60 and 0 < c.T <= 1 << 20 and all(not isinstance(w.frame(c, k), int) for k in range(len(c.frames)))][:14]
    assert len(pool) >= 8 and any(c.frames[0][2] == 0 for c in good) and any(c.frames[-1][2] == 0 for c in good)
    zero = [c for c in good if c.T and c.T <= 1 << 20 and (c.frames[0][2] == 0 or c.frames[-1][2] == 0 or any(f[2] == 0 for f in c.frames[1:-1]))][:8]
    pool += [c for c in zero if c not in pool and all(not isinstance(w.frame(c, k), int) for k in range(len(c.frames)))]
    blob, src_off = lay(pool, 2)
    n = len(pool)
    for group in (1, 2, 3):
        words, E = (true_index(pool) if group == 1 else coarse_index(pool, group))
        requests = []
        for _ in range(120):
            b = rnd.randrange(n + 1)                        # (b == n: no such buffer)
            T = pool[b].T if b < n else 1000
            ends = fr.ranges_of(pool[b]) if b < n else [(0, 5)]
            lo, length = rnd.choice(ends) if rnd.random() < 0.5 else (rnd.randrange(T + 1), rnd.randrange(T + 2))
            requests.append((b, lo, length))
        slots = []
        for k, (b, lo, length) in enumerate(requests):
            want = 0 if b >= n else min(lo + length, pool[b].T) - min(lo, pool[b].T)
            slots.append(want + k % 3)
        dst_off = np.cumsum([4] + slots).tolist()
        plan = run_index(emu, words, n, E, src_off, requests, dst_off)
        results, dst, stat = execute(emu, w, pool, blob, plan, requests, dst_off)
        inside = [(r, q) for r, q in enumerate(requests) if q[0] < n]
        for r, q in enumerate(requests):
            if q[0] >= n:
                assert results[r] == -42 and plan[1][r] == ERROR and bytes(dst[dst_off[r]:dst_off[r + 1]]) == bytes([FILL]) * slots[r]
        check_requests = [q if q[0] < n else None for q in requests]
        for r, q in inside:
            check_execution(w, pool, [q], [dst_off[r], dst_off[r + 1]], [results[r]], dst, ends=False)
            assert plan[1][r] == pool[q[0]].T
        assert bytes(dst[:dst_off[0]]) == bytes([FILL]) * dst_off[0] and bytes(dst[dst_off[-1]:]) == bytes([FILL]) * 64
        assert check_requests.count(None) > 0 and stat[0] + stat[3] == len(requests) and stat[3] == check_requests.count(None)


# ------------------------------------------------------------------------------------------------ false indexes
def test_false_indexes_answer_their_codes(emu, world, good):
    w = world
    c = next(c for c in good if c.name == "forty")
    d = next(c for c in good if c.name == "one")
    pool = [d, c, d]
    blob, src_off = lay(pool, 1)
    words, E = true_index(pool)
    n = 3
    first, valid, cs, us = words[:n + 1], words[n + 1:2 * n + 1], words[2 * n + 1:2 * n + 2 + E], words[2 * n + 2 + E:]
    requests = [(0, 0, MAXU), (1, 0, MAXU), (2, 0, MAXU), (1, 3, c.T - 5)]
    slots = [d.T, c.T + 1, d.T, c.T]
    dst_off = np.cumsum([0] + slots).tolist()

    def run(words2, E2=E):
        plan = run_index(emu, words2, n, E2, src_off, requests, dst_off)
        results, dst, _ = execute(emu, w, pool, blob, plan, requests, dst_off)
        return results, plan[1], dst
    results, totals, dst = run(words)
    assert results == [d.T, c.T, d.T, c.T - 5]
    # sizes that do not sum to the source extent: 72 for that buffer, its neighbours answer as before
    sizes = [f[1] for f in d.frames] + [f[1] for f in c.frames] + [f[1] for f in d.frames]
    contents = [f[2] for f in d.frames] + [f[2] for f in c.frames] + [f[2] for f in d.frames]
    s2 = list(sizes); s2[len(d.frames) + 7] += 1
    res2, tot2, dst2 = run(model_index(first, s2, contents))
    assert res2 == [d.T, -72, d.T, -72] and tot2 == [d.T, ERROR, d.T, ERROR]
    assert bytes(dst2[dst_off[1]:dst_off[2]]) == bytes([FILL]) * (c.T + 1) and bytes(dst2[:dst_off[1]]) == bytes(dst[:dst_off[1]])
    # a first that does not ascend: 42 for that buffer only (the builder marks it; the read refuses it again by itself)
    f2 = [0, len(d.frames) + 3, len(d.frames), E]           # buffer 1 descends
    marked = model_index(f2, sizes, contents)
    assert marked[n + 1:2 * n + 1] == [0, 42, 0]
    res3, tot3, _ = run(marked)
    assert res3[1] == res3[3] == -42 and tot3[1] == ERROR
    unmarked = list(marked); unmarked[n + 2] = 0
    assert run(unmarked)[0][1] == -42
    # a content size one above the truth: the entry decodes without error to another size, 20; one below: it does not fit its slot, the decoder's 70
    k = len(d.frames) + 7
    for delta, code in ((1, -20), (-1, -70)):
        c2 = list(contents); c2[k] += delta
        res4, tot4, _ = run(model_index(first, sizes, c2))
        assert res4[0] == d.T and res4[2] == d.T and res4[1] == code and tot4[1] == c.T + delta, (delta, res4)
    # a size above 2^32 - 1: 42, from the builder
    s3 = list(sizes); s3[k] = SIZE_MAX + 1
    res5, _, _ = run(model_index(first, s3, contents))
    assert res5 == [d.T, -42, d.T, -42]
    # a code in valid answers itself
    coded = list(words); coded[n + 1] = 64
    assert run(coded)[0][0] == -64
    # an interior entry whose sums descend (C[k] raised above C[k + 1]): 20, none of its entries has a slot, and the requests around it — one with slack behind
    # its range, one of an empty range — keep every byte of theirs: the marked request's gathered run lies in its own entries, not in a neighbour's closing entry
    twisted = list(words); twisted[2 * n + 1 + k] = twisted[2 * n + 2 + k] + 5
    requests = [(0, 0, MAXU), (0, d.T, 5), (1, 0, MAXU), (2, 0, MAXU), (1, 0, MAXU)]
    slots = [d.T + 7, 9, c.T, d.T + 3, c.T]
    dst_off = np.cumsum([5] + slots).tolist()
    plan = run_index(emu, twisted, n, E, src_off, requests, dst_off)
    assert list(plan[9]["bad"][:5]) == [0, 0, 1, 0, 1] and plan[2][2] > 0
    scan = [int(x) for x in plan[9]["scan"]]
    for r in range(5):
        assert plan[3][scan[r + 1] - 1] == plan[3][scan[r + 1]]             # every closing entry without a source byte
    results, dst, stat = execute(emu, w, pool, blob, plan, requests, dst_off)
    assert results == [d.T, 0, -20, d.T, -20] and stat == [3, 2 * len(d.frames) + 2 * len(c.frames), 0, 2]
    want = bytearray(bytes([FILL]) * len(dst))
    want[dst_off[0]:dst_off[0] + d.T] = whole_of(w, d)[0]
    want[dst_off[3]:dst_off[3] + d.T] = whole_of(w, d)[0]
    assert bytes(dst) == bytes(want)


def test_indexes_of_random_words_keep_every_offset_inside(emu, world, good):
    """whatever the index holds: sources inside the buffer's extent, destinations inside the request's slot, the entry arrays ascending (the decoders take sizes
    as differences of neighbours), compact bytes and scratch inside what the scans counted"""
    rnd = random.Random(5)
    pool = [c for c in good if 2 <= len(c.frames) <= 60 and 0 < c.T <= 1 << 20][:6]
    blob, src_off = lay(pool, 3)
    n = len(pool)
    true_words, E = true_index(pool)
    reached = marked = 0
    for trial in range(1500):
        words = list(true_words)
        kind = trial % 5
        if kind == 0:
            words = [rnd.getrandbits(64) for _ in words]
        elif kind == 1:
            words = [rnd.getrandbits(rnd.choice((4, 12, 20, 33, 64))) for _ in words]
            words[0] = 0
        else:
            for _ in range(rnd.randint(1, 6)):
                at = rnd.randrange(2 * n + 1 if kind == 2 else 0, len(words)) if kind != 4 else rnd.randrange(2 * n + 2 + E, len(words))
                words[at] = rnd.choice((0, 1, words[at] + rnd.randint(-300, 300), words[rnd.randrange(len(words))], rnd.getrandbits(64), rnd.getrandbits(20))) & MAXU
        requests = []
        for _ in range(6):
            b = rnd.randrange(n)
            requests.append((b, rnd.randrange(pool[b].T + 2), rnd.choice((1, 100, pool[b].T, MAXU))))
        slots = [rnd.choice((0, 50, pool[b].T, pool[b].T + 9)) for b, _, _ in requests]
        dst_off = np.cumsum([13] + slots).tolist()
        rec, total, tot, a_s, a_d, b_s, b_d, cin, cout, state = run_index(emu, words, n, E, src_off, requests, dst_off)
        R = len(requests)
        scan = [int(x) for x in state["scan"]]
        f_a, f_b = scan[:R + 1], scan[R + 1:2 * (R + 1)]
        comp_end, edge_end = tot[2] + tot[3], tot[4]
        assert a_s == sorted(a_s) and b_s == sorted(b_s) and b_d == sorted(b_d) and a_s[-1] == tot[2] and b_s[0] >= tot[2] and b_s[-1] == comp_end and b_d[-1] == edge_end
        for r, (b, lo, length) in enumerate(requests):
            dlo, dhi, ext_lo, ext_hi = dst_off[r], dst_off[r + 1], src_off[b], src_off[b + 1]
            assert a_s[f_a[r + 1] - 1] == a_s[f_a[r + 1]], (trial, r)                  # the closing entry holds no source byte: what a request gathers lies in its own entries
            marked += int(state["bad"][r])
            ent = a_d[f_a[r]:f_a[r + 1]]
            assert ent == sorted(ent) and all(dlo <= x <= dhi for x in ent), (trial, r)
            for key, other, ln in (cin[r], cin[R + 2 * r], cin[R + 2 * r + 1]):
                assert key + ln <= comp_end and (ln == 0 or (ext_lo <= other and other + ln <= ext_hi)), (trial, r)
            for key, other, ln in (cout[2 * r], cout[2 * r + 1]):
                assert key + ln <= edge_end and (ln == 0 or (dlo <= other and other + ln <= dhi)), (trial, r)
            for e in range(f_b[r], f_b[r + 1]):
                assert b_d[e + 1] - b_d[e] <= 128 << 20
            reached += rec[r].status == 0
        results, _, _ = finish(emu, state, [5] * tot[0], [5] * tot[1])
        assert len(results) == R
    assert reached > 300 and marked > 20


def test_entries_fail_loudly_without_gpu(zj):
    import torch
    L = zj.lib()
    assert L.zjni_index_bytes(0, 0) == 256 and L.zjni_index_bytes(3, 1000) == (8 * (7 + 2002) + 255) // 256 * 256
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    out4 = (C.c_uint * 4)()
    buf, dst = C.create_string_buffer(b"x" * 64, 64), C.create_string_buffer(64)
    one = (C.c_uint64 * 1)(64)
    for r in (L.zjni_index_from_sizes_device(0, None, None, None, 0, None, None), L.zjni_index_from_pieces_device(None, 0, 4096, None, None, None, None, None, 0, None, None),
              L.zjni_decompress_index_range_batch_device(None, None, 0, None, 0, None, None, None, None, None, 0, None, None),
              L.zjni_decompress_index_range(dst, 64, buf, 64, 0, 10, one, one, 1, None, None)):
        assert L.zjni_isError(r) and L.zjni_getErrorCode(r) == 200
    assert L.zjni_last_index_range(out4) == -200
