"""CPU (-m "not gpu"): a compress stream continued from its state (zj_encode.h ze_compress_stream_resume), built lane-serial from tests/emu_cstream/emu_cstream.cpp
over a state in host memory.  A stream is cut into calls by a script of (bytes written, flush | end); every call compresses only the bytes behind the last
flush and returns only the frame's new bytes.  The calls' outputs, concatenated, are ZSTD_compressStream2's frame (oracle/ref.py compress_stream) where that
helper can express the script (a flush with every k-th write of one size), and the one-call ze_compress_stream's frame on the whole stream where it cannot;
the state's counters show that no byte was parsed twice.  The -m gpu twin is tests/test_gpu_cstream.py."""
import ctypes as C
import os
import random

import pytest

from util import emu_so

from conftest import golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEVELS = [3, 2, 1, -1, -7]
FLUSH, END, WRITE = "flush", "end", "write"          # WRITE: bytes are buffered and a call is made that flushes nothing


def window(level):
    return 1 << (18 + max(level, 1))                  # the unknown-size rows: 512 KiB / 1 MiB / 2 MiB at levels 1 / 2 / 3, level 1's at negative levels


@pytest.fixture(scope="module")
def emu():
    L = C.CDLL(emu_so("emu_cstream", "libzjni_emu_cstream.so"))
    L.emu_cs_state_bytes.restype = C.c_uint
    L.emu_cs_state_bytes.argtypes = [C.c_int]
    sig = [C.c_char_p, C.c_uint, C.c_char_p, C.c_uint, C.c_int, C.c_int, C.POINTER(C.c_uint), C.c_uint, C.c_int, C.c_int]
    L.emu_cs_continue.restype = C.c_ulonglong
    L.emu_cs_continue.argtypes = [C.c_void_p] + sig
    L.emu_cs_compress_stream.restype = C.c_ulonglong
    L.emu_cs_compress_stream.argtypes = sig
    L.emu_cs_info.argtypes = [C.c_void_p, C.POINTER(C.c_uint)]
    return L


@pytest.fixture(scope="module")
def xml(oracle_ref):
    return oracle_ref.decompress(golden("xml-1.zst"), 6_000_000)


def _res(r, dst):
    return -((1 << 64) - r) if r >= (1 << 63) else dst.raw[:r]


def bound(new, new_flushes):
    """what include/zjni_amd.h documents as always enough for one call"""
    return new + (new >> 8) + 4096 + 64 * (new_flushes + 4)


class CStream:
    """one stream: its state (zeroed = nothing done yet), everything written so far, where it was flushed"""

    def __init__(self, L, level, ck=False, all_flushes=True):
        self.L, self.level, self.ck, self.all_flushes = L, level, ck, all_flushes
        self.state = C.create_string_buffer(L.emu_cs_state_bytes(level))
        self.buf = bytearray()
        self.flushes = []
        self.passed = 0                                # flush positions handed over so far (all_flushes = False: only new ones are passed)
        self.touched = False

    def info(self):
        out = (C.c_uint * 8)()
        self.L.emu_cs_info(self.state, out)
        return dict(zip(("consumed", "produced", "parsed", "blocks", "closed", "error", "notFirst", "lastFlag"), out[:]))

    def call(self, data, what, cap=None, level=None, ck=None, src=None):
        known_empty = what == END and not self.touched and not data and not self.buf
        self.touched = True
        before = self.info()["consumed"]
        self.buf += data
        if what == FLUSH:
            self.flushes.append(len(self.buf))
        fl = self.flushes if self.all_flushes else self.flushes[self.passed:]
        self.passed = len(self.flushes)
        src = bytes(self.buf) if src is None else src
        if cap is None:
            cap = bound(len(src) - before, len([f for f in fl if f > before]))
        dst = C.create_string_buffer(cap + 8)
        r = self.L.emu_cs_continue(self.state, src, len(src), dst, cap, self.level if level is None else level, int(self.ck if ck is None else ck),
                                   (C.c_uint * max(len(fl), 1))(*fl), len(fl), int(what == END), int(known_empty))
        return _res(r, dst)


def one_call(L, d, level, ck, flushes, final=True, known_empty=None):
    """the route that was there before: ze_compress_stream on the whole stream"""
    if known_empty is None:
        known_empty = final and not d and not flushes
    cap = len(d) + (len(d) >> 8) + 4096 + 64 * (len(flushes) + 2)
    dst = C.create_string_buffer(cap)
    r = L.emu_cs_compress_stream(d, len(d), dst, cap, level, int(ck), (C.c_uint * max(len(flushes), 1))(*flushes), len(flushes), int(final), int(known_empty))
    return _res(r, dst)


def walk(frame, ck):
    """the frame's blocks as (type, size, last); the frame must end behind its last block (and checksum)"""
    assert frame[:4] == b"\x28\xb5\x2f\xfd"
    desc = frame[4]
    assert (desc >> 2) & 1 == int(ck) and desc >> 6 == 0
    at = 6                                             # window byte, or the one-byte content size of a single-segment frame
    blocks = []
    while True:
        h = frame[at] | frame[at + 1] << 8 | frame[at + 2] << 16
        last, typ, size = h & 1, (h >> 1) & 3, h >> 3
        body = 1 if typ == 1 else size
        blocks.append((typ, size, last, frame[at + 3:at + 3 + body]))
        at += 3 + body
        if last:
            break
    assert at + (4 if ck else 0) == len(frame)
    return blocks


def run_script(L, d, level, ck, script, all_flushes=True):
    """-> (concatenated outputs, flush positions, the stream).  Checks the counters after every call."""
    s = CStream(L, level, ck, all_flushes)
    out, at, parsed = b"", 0, 0
    for n, what in script:
        before = s.info()
        got = s.call(d[at:at + n], what)
        at += n
        assert isinstance(got, bytes), (level, ck, script, got)
        out += got
        i = s.info()
        if what == END:
            assert i["closed"] == 1 and i["consumed"] == at
        else:
            newest = max([f for f in s.flushes] + [0])
            assert i["consumed"] == newest and i["closed"] == 0
            # no rework: the counters grow by exactly the bytes between the previous and the newest flush
            assert i["parsed"] - before["parsed"] == newest - before["consumed"], (level, script)
            if newest == before["consumed"]:
                assert got == b"" and i == before, "nothing flushed since the last call: no bytes, nothing moves"
        assert i["produced"] == len(out) and i["error"] == 0
    assert at == len(d)
    i = s.info()
    blocks = walk(out, ck)
    real = [b for b in blocks if not (b[0] == 0 and b[1] == 0)]           # (the 3-byte epilogue block is none of them)
    assert i["parsed"] == len(d) and i["blocks"] == len(real), (level, script, i, len(blocks))
    assert i["lastFlag"] == (1 if real and real[-1][2] else 0)
    return out, list(s.flushes), s


def writes(total, w, k):
    """`w` bytes per write, a flush with every k-th, then the close: what oracle/ref.py compress_stream(chunk=w, flush_every=k) does"""
    script, at, j = [], 0, 0
    while at < total:
        n = min(w, total - at); j += 1
        script.append((n, FLUSH if j % k == 0 else WRITE))
        at += n
    return script + [(0, END)]


def synth_mixed(zj, size):
    """the benchmark's buffers, a new class every 64 KiB"""
    return b"".join(zj.synth_host(65536, i, 1) for i in range(size // 65536 + 1))[:size]


def text(rnd, n):
    words = [b"alpha", b"beta", b"gamma", b"delta", b"epsilon", b"zeta", b"\"id\":", b"\"name\":", b"compress", b"level", b"\n", b"{", b"}"]
    out = bytearray()
    while len(out) < n:
        out += rnd.choice(words) + b" "
    return bytes(out[:n])


def skewed(rnd, n):
    """letters drawn with fixed, uneven odds: nothing to match, literals that one Huffman table serves block after block"""
    return bytes(rnd.choices(b"etaoinshrdlu ,.\n", weights=[12, 9, 8, 8, 7, 7, 6, 6, 6, 4, 4, 3, 14, 2, 2, 2], k=n))


def test_state_sizes(emu):
    """header + the unknown-size row's tables (N/compress/clevels.h:26-30): level 1 2^14 entries, level 2 2^16, level 3 2^17 + 2^16, negative levels 2^13"""
    for level, entries in ((1, 1 << 14), (2, 1 << 16), (3, (1 << 17) + (1 << 16)), (0, (1 << 17) + (1 << 16)), (-1, 1 << 13), (-7, 1 << 13), (-200000, 1 << 13)):
        n = emu.emu_cs_state_bytes(level)
        assert n == 1280 + 4 * entries and n % 256 == 0, (level, n)
    for level in (4, 5, 19):
        assert emu.emu_cs_state_bytes(level) == 0


@pytest.mark.parametrize("level", LEVELS)
def test_flush_with_every_kth_write(emu, oracle_ref, zj, xml, level):
    """the scripts the reference helper expresses: against ZSTD_compressStream2, and the one-call route beside it (which must give what it gave before)"""
    rnd = random.Random(100 + level)
    n = 0
    for w, k, total in ((1000, 1, 20500), (10000, 1, 95000), (50000, 1, 230000), (65536, 1, 300000), (131072, 1, 400000), (200000, 1, 500000),
                        (10000, 2, 95000), (50000, 2, 230000), (1000, 7, 20500), (10000, 7, 200000), (65536, 2, 524288)):
        total = min(total, window(level))
        o = rnd.randrange(0, len(xml) - total - 1)
        for d in (xml[o:o + total], synth_mixed(zj, total)):
            ck = bool(n & 1); n += 1
            got, flushes, _ = run_script(emu, d, level, ck, writes(total, w, k), all_flushes=bool(n & 2))
            want = oracle_ref.compress_stream(d, level, ck, chunk=w, flush_every=k)
            assert got == want, (level, ck, w, k, total)
            assert one_call(emu, d, level, ck, flushes) == want, ("the one-call route", level, ck, w, k, total)


@pytest.mark.parametrize("level", LEVELS)
def test_script_classes(emu, oracle_ref, xml, level):
    rnd = random.Random(200 + level)
    for ck in (False, True):
        o = rnd.randrange(0, len(xml) - 400000)
        d = xml[o:o + 150000]
        # a flush with nothing written since the last one, two flushes at one position, close right after a flush: the 3-byte empty last block
        script = [(30000, FLUSH), (0, FLUSH), (0, FLUSH), (50000, WRITE), (0, FLUSH), (0, FLUSH), (70000, FLUSH), (0, END)]
        got, flushes, s = run_script(emu, d, level, ck, script)
        assert flushes == [30000, 30000, 30000, 80000, 80000, 150000]
        assert got == one_call(emu, d, level, ck, flushes)
        assert oracle_ref.decompress(got, len(d)) == d
        assert s.info()["lastFlag"] == 0 and got[len(got) - 3 - (4 if ck else 0):len(got) - (4 if ck else 0)] == b"\x01\x00\x00"
        # close with bytes buffered: the buffered rest is the last piece, its last block the frame's last
        script = [(1000, FLUSH), (40000, WRITE), (60000, WRITE), (0, FLUSH), (49000, WRITE), (0, END)]
        got, flushes, s = run_script(emu, d, level, ck, script, all_flushes=False)
        assert got == one_call(emu, d, level, ck, flushes) and s.info()["lastFlag"] == 1
        assert oracle_ref.decompress(got, len(d)) == d
        # ... and data arriving with the close itself
        got, flushes, _ = run_script(emu, d, level, ck, [(100000, FLUSH), (50000, END)])
        assert got == one_call(emu, d, level, ck, flushes)
        # a first call that flushes nothing (and a second one), then the stream as usual
        s = CStream(emu, level, ck)
        assert s.call(d[:5000], WRITE) == b"" and s.call(b"", WRITE) == b""
        i = s.info()
        assert (i["consumed"], i["produced"], i["parsed"], i["blocks"]) == (0, 0, 0, 0)
        got = s.call(d[5000:9000], FLUSH) + s.call(d[9000:], END)
        assert got == one_call(emu, d, level, ck, [9000])
        assert oracle_ref.decompress(got, len(d)) == d
        # closed before anything else was called on it: the size (0) is known
        s = CStream(emu, level, ck)
        got = s.call(b"", END)
        assert got == oracle_ref.compress_stream(b"", level, ck) and got[4] & 0x20
        assert (s.info()["parsed"], s.info()["blocks"], s.info()["closed"]) == (0, 0, 1)
        # flushed empty first: the size is not known any more
        s = CStream(emu, level, ck)
        assert s.call(b"", FLUSH) == b""
        got = s.call(b"", END)
        assert got == one_call(emu, b"", level, ck, [0], known_empty=False) and not got[4] & 0x20
        assert oracle_ref.decompress(got, 0) == b""
        # one write, one close: the plain stream
        for size in (1, 70000, 131072, 200000):
            got, _, _ = run_script(emu, xml[o:o + size], level, ck, [(size, END)])
            assert got == oracle_ref.compress_stream(xml[o:o + size], level, ck, chunk=131072)


@pytest.mark.parametrize("level", LEVELS)
def test_inputs_that_make_each_carried_field_matter(emu, oracle_ref, zj, level):
    rnd = random.Random(300 + level)
    noise = bytes(rnd.getrandbits(8) for _ in range(40000))
    for ck in (False, True):
        # text (words, and letters that only Huffman codes shorten) flushed every 1 000 - 4 000 bytes: the next block repeats the previous Huffman table (a treeless literals section) and uses the repcodes
        d = b"".join(text(rnd, 300) + skewed(rnd, 700) for _ in range(60))
        script, at = [], 0
        while at < len(d):
            n = min(rnd.randrange(1000, 4001), len(d) - at)
            script.append((n, FLUSH)); at += n
        got, flushes, _ = run_script(emu, d, level, ck, script + [(0, END)], all_flushes=ck)
        assert got == one_call(emu, d, level, ck, flushes)
        assert oracle_ref.decompress(got, len(d)) == d
        if level > 0:                                 # (negative levels store literals raw)
            assert any(t == 2 and body[0] & 3 == 3 for t, _, _, body in walk(got, ck)[1:]), "no block repeated the previous block's Huffman table"
        # noise between two text spans, each flushed: the raw block confirms neither the repcodes nor the table
        d = text(rnd, 30000) + noise + text(rnd, 30000)
        got, flushes, _ = run_script(emu, d, level, ck, [(15000, FLUSH), (15000, FLUSH), (40000, FLUSH), (3000, FLUSH), (27000, END)])
        assert got == one_call(emu, d, level, ck, flushes)
        assert [t for t, _, _, _ in walk(got, ck)][2] == 0
        assert oracle_ref.decompress(got, len(d)) == d
        # a long run of one byte across two flushes: RLE blocks are never the frame's first, so isFirst has to survive a call
        d = b"a" * 13000
        got, flushes, _ = run_script(emu, d, level, ck, [(5000, FLUSH), (5000, FLUSH), (3000, FLUSH), (0, END)])
        assert got == one_call(emu, d, level, ck, flushes) == oracle_ref.compress_stream(d, level, ck, chunk=5000, flush_every=1)
        assert [t for t, _, _, _ in walk(got, ck)] == [2, 1, 1, 0]
        # a new class every 64 KiB, a flush at 1 000 and 300 000 more bytes before the close: a full 128 KiB piece with the pre-split behind a resume,
        # `savings` from the cumulative count
        d = synth_mixed(zj, 301000)
        got, flushes, _ = run_script(emu, d, level, ck, [(1000, FLUSH), (300000, END)])
        assert got == one_call(emu, d, level, ck, flushes)
        got2, flushes, _ = run_script(emu, d, level, ck, [(1000, FLUSH), (200000, WRITE), (100000, FLUSH), (0, END)])
        assert got2 == one_call(emu, d, level, ck, flushes)
        assert oracle_ref.decompress(got, len(d)) == d
    # up to the window
    d = synth_mixed(zj, window(level)) if level != 3 else synth_mixed(zj, 600000)
    if level == 2:
        d = d[:600000]
    got, flushes, _ = run_script(emu, d, level, False, writes(len(d), 150000, 1))
    assert got == oracle_ref.compress_stream(d, level, False, chunk=150000, flush_every=1)


def test_refusals_and_dead_states(emu, xml):
    d = xml[:120000]
    for level in (1, 3, -3):
        def started():
            s = CStream(emu, level, False)
            assert isinstance(s.call(d[:50000], FLUSH), bytes)
            return s

        def dead(s, code):
            assert s.info()["error"] == code
            assert s.call(b"", FLUSH) == -code and s.call(d[:10], END) == -code     # the same code from then on

        # beyond the window
        s = CStream(emu, level, False)
        assert s.call(bytes(window(level) + 1), FLUSH) == -201
        dead(s, 201)
        s = started()
        assert s.call(b"", FLUSH, src=bytes(window(level) + 1)) == -201
        dead(s, 201)
        # closed
        s = started()
        assert isinstance(s.call(d[50000:], END), bytes)
        assert s.call(b"x", FLUSH) == -60
        dead(s, 60)
        # begun with another level word, another checksum flag
        s = started()
        assert s.call(d[50000:60000], FLUSH, level=2 if level != 2 else 1) == -60
        dead(s, 60)
        if level < 0:
            s = started()
            assert s.call(d[50000:60000], FLUSH, level=level - 1) == -60
            dead(s, 60)
        s = started()
        assert s.call(d[50000:60000], FLUSH, ck=True) == -60
        dead(s, 60)
        # less than what was consumed already
        s = started()
        assert s.call(b"", FLUSH, src=d[:49999]) == -60
        dead(s, 60)
        # a slot one byte short
        probe = started()
        need = len(probe.call(d[50000:], FLUSH))
        s = started()
        assert s.call(d[50000:], FLUSH, cap=need - 1) == -70
        dead(s, 70)
        probe = started()
        need = len(probe.call(b"", END))
        assert need == 3
        s = started()
        assert s.call(b"", END, cap=2) == -70
        dead(s, 70)
        s = CStream(emu, level, True)
        assert s.call(d[:100], FLUSH, cap=17) == -70                       # the header wants ZSTD_FRAMEHEADERSIZE_MAX of room, as in the one-call route
        dead(s, 70)
    assert CStream(emu, 1).call(b"abc", END, level=4) == -42
