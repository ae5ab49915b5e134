"""CPU (-m "not gpu"): the "continue" mode of a compress stream continued from its state (zj_encode.h ze_compress_stream_resume, mode bit 4 of the device form),
built lane-serial from tests/emu_cstream_pieces/emu_cstream_pieces.cpp over a state in host memory.  With the bit a call that neither flushes nor closes compresses
every full 128 KiB piece behind the newest flush, as ZSTD_compressStream2(ZSTD_e_continue) does the moment its input buffer is full (ZSTD_compressStream_generic,
zcss_load).  The reference is driven call by call through oracle.ref.lib(): one ZSTD_compressStream2 per write, into a destination of ZSTD_compressBound(total) + 64
bytes, so that it hands every piece out in the call that fills it; its cumulative output.pos after every call is what the stream here must have produced by then,
byte for byte.  The -m gpu twin is tests/test_gpu_cstream_pieces.py."""
import ctypes as C
import os
import random

import pytest

from util import emu_so

from conftest import golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEVELS = [1, 2, 3, -1, -7]
CONT, FLUSH, END = 0, 1, 2                              # ZSTD_e_continue / ZSTD_e_flush / ZSTD_e_end
PIECE = 131072
M_END, M_EMPTY, M_CONT = 1, 2, 4                        # the device form's mode word


def window(level):
    return 1 << (18 + max(level, 1))                  # the unknown-size rows: 512 KiB / 1 MiB / 2 MiB at levels 1 / 2 / 3, level 1's at negative levels


@pytest.fixture(scope="module")
def emu():
    L = C.CDLL(emu_so("emu_cstream_pieces", "libzjni_emu_cstream_pieces.so"))
    L.emu_csp_state_bytes.restype = C.c_uint
    L.emu_csp_state_bytes.argtypes = [C.c_int]
    L.emu_csp_continue.restype = C.c_ulonglong
    L.emu_csp_continue.argtypes = [C.c_void_p, C.c_char_p, C.c_ulonglong, C.c_char_p, C.c_uint, C.c_int, C.c_int, C.POINTER(C.c_uint), C.c_uint, C.c_uint]
    L.emu_csp_compress_stream.restype = C.c_ulonglong
    L.emu_csp_compress_stream.argtypes = [C.c_char_p, C.c_uint, C.c_char_p, C.c_uint, C.c_int, C.c_int, C.POINTER(C.c_uint), C.c_uint, C.c_int, C.c_int]
    L.emu_csp_info.argtypes = [C.c_void_p, C.POINTER(C.c_uint)]
    return L


@pytest.fixture(scope="module")
def inputs(oracle_ref):
    """2 MiB each: text-like, incompressible (raw blocks), all-zero (RLE blocks: they confirm neither the repcodes nor a Huffman table)"""
    xml = oracle_ref.decompress(golden("xml-1.zst"), 6_000_000)
    return {"text": xml[300000:300000 + (2 << 20)], "noise": random.Random(11).randbytes(2 << 20), "zero": bytes(2 << 20)}


def _res(r, dst):
    return -((1 << 64) - r) if r >= (1 << 63) else dst.raw[:r]


def bound(new, new_flushes):
    """what include/zjni_amd.h documents as always enough for one call"""
    return new + (new >> 8) + 4096 + 64 * (new_flushes + 4)


class _Buf(C.Structure):
    _fields_ = [("ptr", C.c_void_p), ("size", C.c_size_t), ("pos", C.c_size_t)]


def ref_calls(ref, d, level, ck, script):
    """ZSTD_compressStream2 once per (bytes, directive) of the script -> (the frame, output.pos after every call)"""
    L = ref.lib()
    L.ZSTD_compressStream2.restype = C.c_size_t
    L.ZSTD_compressStream2.argtypes = [C.c_void_p, C.POINTER(_Buf), C.POINTER(_Buf), C.c_int]
    cctx = L.ZSTD_createCCtx()
    try:
        ref._check(L.ZSTD_CCtx_setParameter(cctx, ref.ZSTD_c_compressionLevel, level))
        ref._check(L.ZSTD_CCtx_setParameter(cctx, ref.ZSTD_c_checksumFlag, int(ck)))
        cap = L.ZSTD_compressBound(len(d)) + 64
        dst = C.create_string_buffer(cap)
        src = C.create_string_buffer(d, max(len(d), 1))
        ob = _Buf(C.addressof(dst), cap, 0)
        at, pos = 0, []
        for n, what in script:
            ib = _Buf(C.addressof(src) + at, n, 0)
            r = ref._check(L.ZSTD_compressStream2(cctx, C.byref(ob), C.byref(ib), what))
            assert ib.pos == n and (what == CONT or r == 0), "the reference wanted a second call: the destination is too small for the test's premise"
            at += n
            pos.append(ob.pos)
        assert at == len(d)
        return dst.raw[:ob.pos], pos
    finally:
        L.ZSTD_freeCCtx(cctx)


class CStream:
    """one stream: its state (zeroed = nothing done yet), everything written so far, where it was flushed"""

    def __init__(self, L, level, ck=False, pieces=True, bit_everywhere=False):
        self.L, self.level, self.ck, self.pieces, self.bit_everywhere = L, level, ck, pieces, bit_everywhere
        self.state = C.create_string_buffer(L.emu_csp_state_bytes(level))
        self.buf = bytearray()
        self.flushes = []
        self.touched = False

    def info(self):
        out = (C.c_uint * 8)()
        self.L.emu_csp_info(self.state, out)
        return dict(zip(("consumed", "produced", "parsed", "blocks", "closed", "error", "notFirst", "lastFlag"), out[:]))

    def call(self, data, what, cap=None, level=None, ck=None, src=None, src_size=None):
        known_empty = what == END and not self.touched and not data and not self.buf
        self.touched = True
        before = self.info()["consumed"]
        self.buf += data
        if what == FLUSH:
            self.flushes.append(len(self.buf))
        mode = (M_END if what == END else 0) | (M_EMPTY if known_empty else 0)
        if self.pieces and (what == CONT or self.bit_everywhere):
            mode |= M_CONT
        src = bytes(self.buf) if src is None else src
        fl = self.flushes
        if cap is None:
            cap = bound(max(len(src) - before, 0), len([f for f in fl if f > before]))
        dst = C.create_string_buffer(cap + 8)
        r = self.L.emu_csp_continue(self.state, src, len(src) if src_size is None else src_size, dst, cap, self.level if level is None else level,
                                    int(self.ck if ck is None else ck), (C.c_uint * max(len(fl), 1))(*fl), len(fl), mode)
        return _res(r, dst)


def one_call(L, d, level, ck, flushes):
    """ze_compress_stream on the whole stream"""
    cap = len(d) + (len(d) >> 8) + 4096 + 64 * (len(flushes) + 2)
    dst = C.create_string_buffer(cap)
    r = L.emu_csp_compress_stream(d, len(d), dst, cap, level, int(ck), (C.c_uint * max(len(flushes), 1))(*flushes), len(flushes), 1, int(not d and not flushes))
    return _res(r, dst)


def writes(total, w, tail=((0, END),)):
    """`w` bytes per ZSTD_e_continue write, then the close"""
    return [(min(w, total - a), CONT) for a in range(0, total, w)] + list(tail)


def scripts_for(level):
    """(name, script): the totals 131072, 131073, 262144, 3 x 131072 + 777 in writes of 50 000, 131072 and 1 bytes, the flush positions and the closes.
    A close brings no bytes that complete a piece: the stream routes' rule, in every mode, is that a full piece is never the last block (ZstdOutputStream
    writes with ZSTD_e_continue and closes without bytes), where the reference, handed the piece's last byte WITH ZSTD_e_end, marks that piece as last."""
    P = PIECE
    out = []
    for total in (P, P + 1, 2 * P, 3 * P + 777):
        out.append(("%d by 50000" % total, writes(total, 50000)))
        out.append(("%d by 131072" % total, writes(total, P)))
    out += [
        ("one write of 131073, then the close", [(P + 1, CONT), (0, END)]),
        ("one write of 3 pieces + 777", [(3 * P + 777, CONT), (0, END)]),
        ("1-byte writes around the piece's end", [(P - 2, CONT), (1, CONT), (1, CONT), (1, CONT), (P - 2, CONT), (1, CONT), (1, CONT), (0, END)]),
        ("bytes arriving with the close", [(P, CONT), (P - 2, CONT), (1, END)]),
        ("a flush in the middle of a piece", [(50000, CONT), (50000, FLUSH), (50000, CONT), (P, CONT), (P, CONT), (777, CONT), (0, END)]),
        ("a flush exactly on a piece boundary", [(P, CONT), (0, FLUSH), (50000, CONT), (P, FLUSH), (0, FLUSH), (P, CONT), (0, END)]),
        ("a flush that completes the piece", [(50000, CONT), (P - 50000, FLUSH), (P, CONT), (1, CONT), (0, END)]),
        ("a flush, then 128 KiB more", [(1000, FLUSH), (P, CONT), (0, END)]),
        ("a flush, then 128 KiB more in two writes and a tail", [(70000, FLUSH), (P - 1, CONT), (1, CONT), (P + 5, CONT), (0, FLUSH), (0, END)]),
        ("calls without bytes", [(0, CONT), (P, CONT), (0, CONT), (0, FLUSH), (0, CONT), (0, END)]),
    ]
    return out


def run_script(L, ref, d, level, ck, script, bit_everywhere=False):
    """every call's output against the reference's; -> (the frame, the flush positions)"""
    assert sum(n for n, _ in script) == len(d)
    want, pos = ref_calls(ref, d, level, ck, script)
    s = CStream(L, level, ck, bit_everywhere=bit_everywhere)
    out, at = b"", 0
    for k, (n, what) in enumerate(script):
        before = s.info()
        got = s.call(d[at:at + n], what)
        at += n
        assert isinstance(got, bytes), (level, ck, k, got)
        out += got
        # the content and the call in which it appears
        assert len(out) == pos[k], (level, ck, k, (n, what), len(out), pos[k])
        assert out == want[:pos[k]], (level, ck, k)
        i = s.info()
        assert i["produced"] == len(out) and i["error"] == 0
        last_flush = max(s.flushes + [0])
        if what == END:
            assert i["closed"] == 1 and i["consumed"] == at
        else:
            edge = at if what == FLUSH else last_flush + (at - last_flush) // PIECE * PIECE
            assert i["consumed"] == edge and i["closed"] == 0 and (edge - last_flush) % PIECE == 0
            assert i["parsed"] - before["parsed"] == edge - before["consumed"]                # nothing is parsed twice
            if edge == before["consumed"]:
                assert got == b"" and i == before, "no piece was completed: no bytes, nothing moves"
    assert out == want
    assert s.info()["parsed"] == len(d)
    return out, list(s.flushes)


@pytest.mark.parametrize("level", LEVELS)
def test_pieces_appear_in_the_call_that_fills_them(emu, oracle_ref, inputs, level):
    rnd = random.Random(400 + level)
    n = 0
    for kind, data in inputs.items():
        for name, script in scripts_for(level):
            total = sum(c for c, _ in script)
            o = rnd.randrange(0, len(data) - total)
            d = data[o:o + total]
            for ck in (False, True):
                n += 1
                got, flushes = run_script(emu, oracle_ref, d, level, ck, script, bit_everywhere=bool(n & 2))
                chunked = [(c, w) for c, w in script if c]
                if all(w == CONT for _, w in script[:-1]) and len({c for c, _ in chunked[:-1]}) <= 1 and chunked and chunked[0][0] >= chunked[-1][0] and script[-1] == (0, END):
                    assert got == oracle_ref.compress_stream(d, level, ck, chunk=chunked[0][0]), (kind, name)          # the reference helper's frame, where it expresses the script
                assert got == one_call(emu, d, level, ck, flushes), (kind, name, level, ck)
            if kind != "text":
                assert (got[6] >> 1) & 3 == (0 if kind == "noise" else 2), (kind, name)          # noise: raw blocks; zeros: RLE blocks behind a compressed first one


@pytest.mark.parametrize("level", LEVELS)
def test_a_full_window_written_in_pieces(emu, oracle_ref, inputs, level):
    """the level's whole window without a flush: every write of 128 KiB hands one piece out, the close the 3-byte last block (and the checksum)"""
    total = window(level)
    ck = level in (2, -1)
    d = inputs["text"][:total]
    got, _ = run_script(emu, oracle_ref, d, level, ck, writes(total, PIECE))
    assert got == oracle_ref.compress_stream(d, level, ck, chunk=PIECE) == one_call(emu, d, level, ck, [])
    assert got[len(got) - 3 - (4 if ck else 0):len(got) - (4 if ck else 0)] == b"\x01\x00\x00"
    if level in (1, -7):                                # ... and in writes of 50 000 with a flush on the way, on the noise and on the zeros
        for kind in ("noise", "zero"):
            d = inputs[kind][:total]
            script = writes(total // 2, 50000, tail=[(0, FLUSH)]) + writes(total - total // 2, 50000)
            run_script(emu, oracle_ref, d, level, not ck, script)


@pytest.mark.parametrize("level", [1, 3, -7])
def test_without_the_bit_a_write_only_buffers(emu, oracle_ref, inputs, level):
    """mode bit 4 clear: what there was before — a call that neither flushes nor closes returns nothing and moves nothing, a flush or a close returns everything
    written since the last flush, which is what the reference has produced by then"""
    d = inputs["text"][5000:5000 + 3 * PIECE + 777]
    script = [(50000, CONT), (PIECE, CONT), (50000, FLUSH), (PIECE, CONT), (2 * PIECE + 777 - 100000 - PIECE, CONT), (0, END)]
    for ck in (False, True):
        want, pos = ref_calls(oracle_ref, d, level, ck, script)
        s = CStream(emu, level, ck, pieces=False)
        out, at = b"", 0
        for k, (n, what) in enumerate(script):
            before = s.info()
            got = s.call(d[at:at + n], what)
            at += n
            if what == CONT:
                assert got == b"" and s.info() == before
            else:
                out += got
                assert out == want[:pos[k]]
        assert out == want == one_call(emu, d, level, ck, s.flushes) and s.info()["parsed"] == len(d)


@pytest.mark.parametrize("level", LEVELS)
def test_a_flush_inside_a_continue_call_is_two_reference_calls_in_one(emu, oracle_ref, inputs, level):
    """the device form takes, in one call that does not close, a new flush position below the source's size with full pieces behind it: the reference's flush
    call and its continue call merged — the piece counts from the flush, and the call returns what the reference has produced after both"""
    P = PIECE
    for kind, ck, cuts in (("text", False, (1000, P, 5)), ("noise", True, (50000, 2 * P, 777)), ("zero", False, (P, P, 1)), ("text", True, (P + 7, 2 * P, 0))):
        first, more, tail = cuts
        d = inputs[kind][4321:4321 + first + more + tail]
        want, pos = ref_calls(oracle_ref, d, level, ck, [(first, FLUSH), (more, CONT), (tail, CONT), (0, END)])
        s = CStream(emu, level, ck)
        s.buf += d[:first]; s.flushes.append(first)               # the flush position arrives together with the bytes behind it
        got = s.call(d[first:first + more], CONT)
        assert got == want[:pos[1]], (level, kind, len(got), pos[1])
        i = s.info()
        assert i["consumed"] == first + more and i["parsed"] == first + more and i["error"] == 0
        assert s.call(d[first + more:], CONT) == b""
        got += s.call(b"", END)
        assert got == want == one_call(emu, d, level, ck, [first]) and s.info()["parsed"] == len(d)


def test_refusals_hold_in_continue_mode(emu, inputs):
    d = inputs["text"][:3 * PIECE]
    for level in (1, 3, -3):
        def started():
            s = CStream(emu, level, False)
            got = s.call(d[:PIECE + 5], CONT)
            assert isinstance(got, bytes) and got and s.info()["consumed"] == PIECE
            return s

        def dead(s, code):
            assert s.info()["error"] == code
            assert s.call(b"", CONT) == -code and s.call(d[:10], FLUSH) == -code and s.call(b"", END) == -code     # the same code from then on

        # beyond the window, fresh and begun; beyond every window (the kernel's clamp)
        s = CStream(emu, level, False)
        assert s.call(bytes(window(level) + 1), CONT) == -201
        dead(s, 201)
        s = started()
        assert s.call(b"", CONT, src=bytes(window(level) + 1)) == -201
        dead(s, 201)
        s = started()
        assert s.call(b"", CONT, src=b"", src_size=1 << 33) == -201
        dead(s, 201)
        # closed
        s = started()
        assert isinstance(s.call(b"", END), bytes)
        assert s.call(d[:PIECE], CONT) == -60
        dead(s, 60)
        # begun with another level word, another checksum flag
        s = started()
        assert s.call(d[PIECE + 5:2 * PIECE + 5], CONT, level=2 if level != 2 else 1) == -60
        dead(s, 60)
        s = started()
        assert s.call(d[PIECE + 5:2 * PIECE + 5], CONT, ck=True) == -60
        dead(s, 60)
        # less than what was consumed already
        s = started()
        assert s.call(b"", CONT, src=d[:PIECE - 1]) == -60
        dead(s, 60)
        # a slot one byte short of what the piece takes; the header alone wants 18 bytes of room
        probe = started()
        need = len(probe.call(d[PIECE + 5:2 * PIECE + 5], CONT))
        assert need > 3
        s = started()
        assert s.call(d[PIECE + 5:2 * PIECE + 5], CONT, cap=need - 1) == -70
        dead(s, 70)
        s = CStream(emu, level, True)
        assert s.call(d[:PIECE], CONT, cap=17) == -70
        dead(s, 70)
        # no piece is full: nothing is checked against the slot, nothing moves
        s = started()
        before = s.info()
        assert s.call(d[PIECE + 5:PIECE + 100], CONT, cap=0) == b"" and s.info() == before
    assert CStream(emu, 1).call(bytes(PIECE), CONT, level=4) == -42
