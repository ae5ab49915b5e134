"""CPU (-m "not gpu"): the index of buffers of concatenated frames from their bytes alone (zstd-jni_amd/csrc/zj_index.h: zj_index_walk, zj_index_frames_emit),
built lane-serial from tests/emu_index_walk/emu_index_walk.cpp as zjni_index_count_frames_device and zjni_index_from_frames_device run it.

TRUE INDEX: every buffer of tests/inspect_cases.py and tests/test_emu_frames.py; where the walked entry's emulation (tests/emu_frames_range) finds the buffer indexable
the walk-built index is test_emu_index.true_index (the reference's ZSTD_findFrameCompressedSize / ZSTD_getFrameContentSize), elsewhere valid[i] is that emulation's
status and the buffer owns no entry.  The one documented addition: a buffer the walked entry indexes but with a frame that records more than 2^32 - 1 bytes of
content answers 14 (the index's entry format).  WALKED AGAINST INDEXED: over test_emu_index's boundary ranges the plan from the walk-built index (record, entry
arrays, copy runs) is the walked entry's.  PINNED CASES.  DISTRUST OF THE FIRST PASS: a false first[] or bytes changed between the passes give that buffer 42, no
write outside its extent (guard words around every array), the neighbours exact.  HOST FORM: the arrays of the device emulation, the 70 protocol, the library's own
entry (pure host code), and a stand-alone program under the host sanitizers.  The -m gpu twin is tests/test_gpu_index_walk.py."""
import ctypes as C
import itertools
import os
import struct
import subprocess

import numpy as np
import pytest

from util import emu_so
import test_emu_frames_range as fr
import test_emu_index as ti
from test_emu_index import emu as index_emu, range_emu, true_index      # noqa: F401  (the two fixtures by their names)
from test_emu_frames_range import arr, ptr, MAXU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZE_MAX = (1 << 32) - 1
GUARD = 0xFEEDFACECAFEBEEF
PAD = 4
world = fr.world
HERE = os.path.join(ROOT, "tests", "emu_index_walk")


@pytest.fixture(scope="module")
def walk():
    L = C.CDLL(emu_so("emu_index_walk", "libzjni_emu_index_walk.so"))
    vp, ull = C.c_void_p, C.c_ulonglong
    L.emu_walk_count.restype = None
    L.emu_walk_count.argtypes = [vp, vp, ull, vp]
    L.emu_walk_emit.restype = None
    L.emu_walk_emit.argtypes = [vp, vp, ull, vp, ull, vp, vp, vp]
    L.emu_walk_host.restype = ull
    L.emu_walk_host.argtypes = [vp, ull, vp, vp, ull, vp]
    return L


class Stand:
    """what true_index reads of a case"""

    def __init__(self, frames):
        self.frames = frames


def lay(datas, lead=3):
    blob = b"\xAA" * lead + b"".join(datas) + b"\xAA" * 8
    return np.frombuffer(blob, dtype=np.uint8), np.cumsum([lead] + [len(d) for d in datas]).tolist()


def count(L, src, off):
    n = len(off) - 1
    first = np.full(n + 1 + 2 * PAD, GUARD, dtype=np.uint64)
    inner = first[PAD:PAD + n + 1]
    L.emu_walk_count(ptr(src), ptr(arr(off)), n, ptr(inner))
    assert all(int(x) == GUARD for x in first[:PAD]) and all(int(x) == GUARD for x in first[PAD + n + 1:])
    return [int(x) for x in inner]


def emit(L, src, off, first, E, sizes=True):
    """the second pass with guard words around the index and both arrays: (index words, size[E], content[E])"""
    n = len(off) - 1
    words = 2 * n + 1 + 2 * (E + 1)
    idx = np.full(words + 2 * PAD, GUARD, dtype=np.uint64)
    size, content = np.full(E + 2 * PAD, GUARD, dtype=np.uint64), np.full(E + 2 * PAD, GUARD, dtype=np.uint64)
    i_in, s_in, c_in = idx[PAD:PAD + words], size[PAD:PAD + E + 1], content[PAD:PAD + E + 1]
    L.emu_walk_emit(ptr(src), ptr(arr(off)), n, ptr(arr(first)), E, ptr(i_in), ptr(s_in) if sizes else None, ptr(c_in) if sizes else None)
    for a, used in ((idx, words), (size, E if sizes else 0), (content, E if sizes else 0)):
        assert all(int(x) == GUARD for x in a[:PAD]) and all(int(x) == GUARD for x in a[PAD + used:]), "a write outside the array"
    return [int(x) for x in i_in], [int(x) for x in size[PAD:PAD + E]], [int(x) for x in content[PAD:PAD + E]]


def build(L, datas, lead=3, sizes=True):
    src, off = lay(datas, lead)
    first = count(L, src, off)
    words, size, content = emit(L, src, off, first, first[-1], sizes)
    return words, first[-1], size, content, src, off


def walked_status(range_emu, data):
    """rule 1 of the walked entry's emulation for one buffer: 1 (an empty range of an indexable buffer), or the code that answers for it"""
    src, off = lay([data], 1)
    rec = fr.run_emu(range_emu, src, off, [0, 0], [(0, 0)])[0]
    return int(rec[0].status)


def expectation(range_emu, c):
    """(valid, frames) of a case: the reference's frames where the walked emulation indexes the buffer, else its status and no entry"""
    status = walked_status(range_emu, c.data)
    if status != 1:
        assert c.code == status, c.name
        return status, []
    assert c.code == 0, c.name
    if any(f[2] > SIZE_MAX for f in c.frames):
        return 14, []                                       # the addition the entry format forces
    return 0, c.frames


def expected_words(exp):
    words, E = true_index([Stand(frames) for _, frames in exp])
    n = len(exp)
    for i, (valid, _) in enumerate(exp):
        words[n + 1 + i] = valid
    return words, E


# ------------------------------------------------------------------------------------------------ 1. the true index
def test_walk_builds_the_true_index(walk, range_emu, world):
    cases = world.cases
    exp = [expectation(range_emu, c) for c in cases]
    assert sum(v == 0 and len(f) >= 2 for v, f in exp) > 10 and {10, 14, 72} <= {v for v, _ in exp}
    assert any(v == 14 and c.code == 0 for (v, _), c in zip(exp, cases)), "no buffer takes the addition"
    for order in (list(range(len(cases))), list(reversed(range(len(cases))))):
        want, E = expected_words([exp[i] for i in order])
        words, E2, size, content, _, _ = build(walk, [cases[i].data for i in order])
        assert E2 == E and words == want
        frames = [f for i in order for f in exp[i][1]]
        assert size == [f[1] for f in frames] and content == [f[2] for f in frames]
        again = build(walk, [cases[i].data for i in order], sizes=False)      # the arrays in library scratch: the same index
        assert again[0] == want
    for c, e in list(zip(cases, exp))[:60]:                 # and alone, n == 1
        want, E = expected_words([e])
        assert build(walk, [c.data], lead=0)[:2] == (want, E), c.name


# ------------------------------------------------------------------------------------------------ 2. walked against indexed
def test_plans_from_the_walk_built_index_equal_the_walked_entry(walk, index_emu, range_emu, world):
    selected = 0
    good = [c for c in world.cases if c.code == 0 and all(f[2] <= SIZE_MAX for f in c.frames)]
    assert len(good) > 20 and any(len(c.frames) == 40 for c in good)
    for c in good:
        small = c.T <= 1 << 22
        for lead in (0, 5):
            words, E, _, _, src, src_off = build(walk, [c.data], lead)
            for j, (lo, length) in enumerate(fr.ranges_of(c)):
                if j % 2 != (lead != 0):
                    continue                                # (each range once, half of them at either lead)
                want = min(lo + length, c.T) - min(lo, c.T)
                slot = (want + (j % 3) * 5 if j % 7 else max(want - 1, 0)) if small else want
                dst_off = [7, 7 + slot]
                mine = ti.run_index(index_emu, words, 1, E, src_off, [(0, lo, length)], dst_off)
                theirs = fr.run_emu(range_emu, src, src_off, dst_off, [(lo, length)])
                ti.same_plan(mine, theirs, (c.name, lo, length, slot))
                selected += mine[0][0].status == 0
    assert selected > 5000


# ------------------------------------------------------------------------------------------------ 3. pinned cases
def header_only(content):
    """a frame of a header and an empty last block that claims `content` bytes"""
    return struct.pack("<IBQ", 0xFD2FB528, 0xE0, content) + b"\x01\x00\x00"


def one_buffer(walk, data):
    words, E, size, content, _, _ = build(walk, [data], lead=2)
    assert words[0] == 0 and words[1] == E
    return words[2], E, size, content


def test_pinned_content_size_at_the_entry_limit(walk, range_emu):
    big, edge = header_only(1 << 32), header_only(SIZE_MAX)
    assert walked_status(range_emu, big) == 1 and walked_status(range_emu, edge) == 1       # the walked entry indexes both
    assert one_buffer(walk, big) == (14, 0, [], [])
    assert one_buffer(walk, edge) == (0, 1, [len(edge)], [SIZE_MAX])
    assert one_buffer(walk, edge + big) == (14, 0, [], [])                                  # at that frame, wherever it stands
    assert one_buffer(walk, edge + edge) == (0, 2, [len(edge)] * 2, [SIZE_MAX] * 2)


def test_pinned_empty_buffer(walk):
    assert one_buffer(walk, b"") == (0, 0, [], [])
    words, E, _, _, _, _ = build(walk, [b"", b"", b""])
    assert E == 0 and words == [0, 0, 0, 0, 0, 0, 0, 0, 0]


def test_pinned_one_frame(walk, oracle_ref):
    text = b"one frame is an index of one entry. " * 9
    z = oracle_ref.compress(text, 3)
    assert one_buffer(walk, z) == (0, 1, [len(z)], [len(text)])


def test_pinned_skippable_frames_first_last_and_alone(walk, oracle_ref):
    import inspect_cases as ic
    text = b"a skippable frame is an entry of no content. " * 7
    z, s, t = oracle_ref.compress(text, 1), ic.skippable(b"seek table?", 1), ic.skippable(b"", 15)
    assert one_buffer(walk, s + z) == (0, 2, [len(s), len(z)], [0, len(text)])
    assert one_buffer(walk, z + z + t) == (0, 3, [len(z), len(z), 8], [len(text), len(text), 0])
    assert one_buffer(walk, s) == (0, 1, [len(s)], [0])
    assert one_buffer(walk, s + t + s) == (0, 3, [len(s), 8, len(s)], [0, 0, 0])


def test_pinned_trailing_garbage_shorter_than_a_header(walk, range_emu, oracle_ref):
    z = oracle_ref.compress(b"then something that is no frame. " * 5, 3)
    for tail, code in ((b"\x00", 10), (b"\x28\xB5", 72), (b"\x28\xB5\x2F\xFD", 72), (b"\x50\x2A\x4D", 72), (b"\x28\xB5\x2F\xFE", 10), (b"\xFF\xFF\xFF\xFF", 10)):
        assert walked_status(range_emu, z + tail) == code, tail
        assert one_buffer(walk, z + tail) == (code, 0, [], []), tail


# ------------------------------------------------------------------------------------------------ 4. distrust of the first pass
def model_emit(true_frames, first, E):
    """what the second pass leaves for buffers whose extents do not overlap: (valid[n], size[E], content[E])"""
    size, content, valid = [0] * E, [0] * E, []
    for i, frames in enumerate(true_frames):
        if not first[i] <= first[i + 1] <= E:
            valid.append(42)
        elif first[i + 1] - first[i] != len(frames):
            valid.append(42)
        else:
            valid.append(0)
            for k, f in enumerate(frames):
                size[first[i] + k], content[first[i] + k] = f[1], f[2]
    return valid, size, content


def test_the_second_pass_trusts_nothing_of_the_first(walk, world):
    by = {c.name: c for c in world.cases}
    trio = [by["forty"], by["two"], by["skip_first"]]
    datas = [c.data for c in trio]
    frames = [c.frames for c in trio]
    src, off = lay(datas)
    honest = count(walk, src, off)
    assert honest == [0, 40, 42, 45]
    false_firsts = {"honest": (honest, 45, [0, 0, 0]),
                    "too small": ([0, 40, 41, 44], 44, [0, 42, 0]),
                    "too large": ([0, 40, 45, 48], 48, [0, 42, 0]),
                    "too large, room behind": ([0, 40, 50, 53], 60, [0, 42, 0]),
                    "descending": ([50, 90, 0, 3], 90, [0, 42, 0]),
                    "past E": ([0, 40, 42, 45], 44, [0, 0, 42]),
                    "first of all too small": ([0, 39, 41, 44], 44, [42, 0, 0]),
                    "a count of none": ([0, 40, 40, 43], 43, [0, 42, 0])}
    for name, (first, E, verdicts) in false_firsts.items():
        words, size, content = emit(walk, src, off, first, E)
        valid, want_size, want_content = model_emit(frames, first, E)
        assert valid == verdicts, name
        n = 3
        assert words[:n + 1] == first and words[n + 1:2 * n + 1] == valid, name
        assert size == want_size and content == want_content, name
        assert words[2 * n + 1:2 * n + 2 + E] == list(itertools.accumulate([0] + want_size)), name
        assert words[2 * n + 2 + E:] == list(itertools.accumulate([0] + want_content)), name
    # bytes changed between the passes: the magic of frame 20 of the first buffer, a frame cut off the second, a frame more in the third
    for which, change in ((0, "magic"), (1, "shorter"), (2, "longer"), (1, "empty")):
        datas2 = list(datas)
        if change == "magic":
            at = trio[0].frames[20][0]
            datas2[0] = datas[0][:at] + b"\x00" + datas[0][at + 1:]
        elif change == "shorter":
            datas2[1] = datas[1][:trio[1].frames[1][0]]
        elif change == "longer":
            datas2[2] = datas[2] + by["one"].data
        else:
            datas2[1] = b""
        src2, off2 = lay(datas2)
        words, size, content = emit(walk, src2, off2, honest, 45)
        valid, want_size, want_content = model_emit([f if i != which else [] for i, f in enumerate(frames)], [0, 40, 42, 45], 45)
        valid[which] = 42
        assert words[4:7] == valid and size == want_size and content == want_content, change
        assert words[7:7 + 46] == list(itertools.accumulate([0] + want_size)), change


# ------------------------------------------------------------------------------------------------ 5. the host form
def host_walk(fn, data, capacity):
    buf = (C.c_ubyte * max(len(data), 1)).from_buffer_copy(data or b"\0")
    size, content = np.full(capacity + 2, GUARD, dtype=np.uint64), np.full(capacity + 2, GUARD, dtype=np.uint64)
    n = C.c_size_t(77)
    r = fn(buf, len(data), ptr(size) if capacity else None, ptr(content) if capacity else None, capacity, C.byref(n))
    assert int(size[capacity]) == GUARD and int(content[capacity]) == GUARD
    code = (1 << 64) - r if r > MAXU - 120 else 0
    return code, n.value, [int(x) for x in size[:capacity]], [int(x) for x in content[:capacity]]


def test_host_form_gives_the_device_emulations_arrays(walk, zj, world):
    L = zj.lib()
    for fn in (walk.emu_walk_host, L.zjni_index_from_frames):
        for c in world.cases[:400]:
            valid, E, size, content = one_buffer(walk, c.data)
            code, n, _, _ = host_walk(fn, c.data, 0)                    # the counting call
            if valid:
                assert (code, n) == (valid, 0), c.name
                continue
            assert (code, n) == (70 if E else 0, E), c.name
            assert host_walk(fn, c.data, E) == (0, E, size, content), c.name
            assert host_walk(fn, c.data, E + 3)[:2] == (0, E), c.name
            if E:
                code, n, s1, c1 = host_walk(fn, c.data, E - 1)          # one too few: 70, the count needed, nothing beyond the capacity
                assert (code, n, s1, c1) == (70, E, size[:E - 1], content[:E - 1]), c.name


def test_host_form_under_the_host_sanitizers(walk, world, tmp_path):
    """tests/emu_index_walk/walk_main.cpp, built with -fsanitize=address,undefined -fno-sanitize-recover=all: every buffer on an exact-size malloc copy"""
    cases = world.cases
    path = tmp_path / "buffers.bin"
    with open(path, "wb") as f:
        for c in cases:
            f.write(struct.pack("<Q", len(c.data)) + c.data)
    out = subprocess.run([os.path.join(HERE, "walk_main"), str(path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    lines = out.stdout.decode().splitlines()
    assert len(lines) == len(cases)
    for c, line in zip(cases, lines):
        valid, E, size, content = one_buffer(walk, c.data)
        head, s, t = line.split("|")
        code, n, short = (int(x) for x in head.split())
        assert (code, n) == (valid, E), c.name
        assert [int(x) for x in s.split()] == size and [int(x) for x in t.split()] == content, c.name
        assert short == (E if E else 0), c.name


def test_device_entries_fail_loudly_without_gpu(zj):
    import torch
    L = zj.lib()
    n = C.c_size_t(0)
    assert L.zjni_index_from_frames(None, 0, None, None, 0, C.byref(n)) == 0 and n.value == 0      # the host form needs no device
    if not torch.cuda.is_available():
        first = (C.c_uint64 * 2)()
        for r in (L.zjni_index_count_frames_device(None, None, 0, first, None), L.zjni_index_from_frames_device(None, None, 0, first, 0, first, None, None, None)):
            assert L.zjni_isError(r) and L.zjni_getErrorCode(r) == 200
