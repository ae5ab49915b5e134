"""GPU (-m gpu): full 128 KiB pieces of a compress stream compressed as they are written — mode bit 4 of zjni_compress_stream_continue_batch_device
(ze_compress_stream_resume's `pieces` on zj_encode_stream_continue_kernel) and the eager host form (zjni_createCStream2 with ZJNI_CSTREAM_EAGER,
zjni_cstream_pending, zstd_jni_amd.ZstdCompressStream(eager=True)).  The reference is ZSTD_compressStream2 driven call by call (ref_calls of
tests/test_emu_cstream_pieces.py, the CPU twin): what a stream has produced after a call is what the reference has produced after the same call."""
import ctypes as C
import itertools
import random

import pytest

from conftest import golden
from test_emu_cstream_pieces import CONT, END, FLUSH, PIECE, ref_calls, window

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu(zj):
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    zj.batch.init(0)
    return zj


@pytest.fixture(scope="module")
def xml(oracle_ref):
    return oracle_ref.decompress(golden("xml-1.zst"), 6_000_000)


def to_dev(b):
    import torch
    return torch.frombuffer(bytearray(b) or bytearray(1), dtype=torch.uint8).to("cuda")


def offsets(sizes):
    import torch
    return torch.tensor([0] + list(itertools.accumulate(sizes)), dtype=torch.int64, device="cuda")


def script_for(k, total):
    """one stream's calls: the classes of tests/test_emu_cstream_pieces.py"""
    P = PIECE
    fam = k % 6
    if fam == 0:
        s = [(min(50000, total - a), CONT) for a in range(0, total, 50000)] + [(0, END)]
    elif fam == 1:
        s = [(min(P, total - a), CONT) for a in range(0, total, P)] + [(0, END)]
    elif fam == 2:
        s = [(total, CONT), (0, END)]                                                       # every full piece in one call
    elif fam == 3:
        s = [(50000, CONT), (50000, FLUSH)] + [(min(P, total - 7 - a), CONT) for a in range(100000, total - 7, P)]   # a flush in the middle of a piece
        s += [(7, END)]                                                                                           # bytes arriving with the close
    elif fam == 4:
        s = [(P, CONT), (0, FLUSH), (total - P - 5, CONT), (5, END)]                        # a flush exactly on a piece boundary
    else:
        s = [(1000, FLUSH), (P, CONT), (total - P - 1000, CONT), (0, FLUSH), (0, END)]     # a flush, then 128 KiB more
    assert sum(n for n, _ in s) == total
    return s


@pytest.mark.parametrize("level", [1, 3, -1])
def test_gpu_pieces_batch_in_lock_step(gpu, oracle_ref, xml, level):
    """one launch per round over 70 streams: streams that start rounds later than others (fresh states beside begun ones), bit 4 beside flushes and closes,
    closed streams (60 from then on) and one stream beyond the window (201 from then on)"""
    import torch
    rnd = random.Random(900 + level)
    n, ck = 70, level == 3
    noise = rnd.randbytes(4 * PIECE)
    datas, scripts, start = [], [], []
    for k in range(n - 1):
        total = PIECE + 1 if k == 0 else rnd.randrange(PIECE + 1, 3 * PIECE + 5000)
        total = max(total, PIECE + 1000) if k % 6 >= 4 else total                           # (room for those scripts' fixed parts)
        last_flush = {3: 100000, 4: PIECE, 5: total}[k % 6] if k % 6 >= 3 else 0
        if k % 6 in (3, 4) and (total - last_flush) % PIECE == 0:
            total += 1                                                                      # (a close never brings the bytes that complete a piece: the streams' rule)
        o = rnd.randrange(0, len(xml) - total - 1)
        datas.append(noise[:total] if k % 11 == 7 else bytes(total) if k % 11 == 9 else xml[o:o + total])
        scripts.append(script_for(k, total))
        start.append(k % 3)
    datas.append(bytes(window(level) + 1)); scripts.append([(PIECE, CONT), (window(level) + 1 - PIECE, CONT), (0, END)]); start.append(1)      # beyond the window in its second call
    refs = [ref_calls(oracle_ref, d, level, ck, s) for d, s in zip(datas[:-1], scripts[:-1])]

    size = gpu.lib().zjni_cstream_state_bytes(level)
    states = gpu.batch.stream_states(n, level)
    states.fill_(0x5A)                                                                      # a state is fresh when it is zeroed, which happens in the round a stream starts
    buf, flushes, outs, at, done, touched = [bytearray() for _ in range(n)], [[] for _ in range(n)], [b""] * n, [0] * n, [False] * n, [False] * n
    rounds = max(st + len(s) for st, s in zip(start, scripts)) + 1
    for j in range(rounds):
        live = [i for i in range(n) if j >= start[i]]
        for i in live:
            if j == start[i]:
                states[i * size:(i + 1) * size].zero_()
        steps, mode = {}, []
        for i in live:
            step = j - start[i]
            cnt, what = scripts[i][step] if step < len(scripts[i]) else (0, CONT)
            data = datas[i][at[i]:at[i] + cnt]; at[i] += cnt
            known_empty = what == END and not touched[i] and not data
            touched[i] = True
            buf[i] += data
            if what == FLUSH:
                flushes[i].append(len(buf[i]))
            mode.append((1 if what == END else 0) | (2 if known_empty else 0) | (4 if what == CONT or i % 2 else 0))
            steps[i] = (step, what)
        info = {k: v.cpu().tolist() for k, v in gpu.batch.stream_state_info(states, level).items()}
        new = [max(len(buf[i]) - (info["consumed"][i] if j > start[i] else 0), 0) for i in live]
        caps = [m + (m >> 8) + 4096 + 64 * (len(flushes[i]) + 4) for m, i in zip(new, live)]
        # the streams of this round are a slice of the state tensor: they are ordered by their start round, so gather them
        sub = torch.cat([states[i * size:(i + 1) * size] for i in live])
        blob, off = to_dev(b"".join(bytes(buf[i]) for i in live)), offsets([len(buf[i]) for i in live])
        dst, doff = torch.zeros(sum(caps) + 8, dtype=torch.uint8, device="cuda"), offsets(caps)
        fa = torch.tensor(list(itertools.chain(*[flushes[i] for i in live])) or [0], dtype=torch.int64, device="cuda").to(torch.int32)
        fo = offsets([len(flushes[i]) for i in live])
        md = torch.tensor(mode, dtype=torch.int32, device="cuda")
        res = gpu.batch.compress_stream_continue(blob, off, dst, doff, sub, level, ck, fa, fo, md)
        torch.cuda.synchronize()
        for q, i in enumerate(live):
            states[i * size:(i + 1) * size] = sub[q * size:(q + 1) * size]
        out, rs, dl = dst.cpu().numpy().tobytes(), res.cpu().tolist(), doff.cpu().tolist()
        for q, i in enumerate(live):
            step, what = steps[i]
            if i == n - 1:
                assert rs[q] == (-201 if step >= 1 else rs[q]) and (step >= 1 or rs[q] > 0), (level, j, rs[q])
                continue
            if done[i]:
                assert rs[q] == -60, (level, i, j, rs[q])                                   # closed: stage_wrong, and from then on
                continue
            assert rs[q] >= 0, (level, i, j, rs[q])
            outs[i] += out[dl[q]:dl[q] + rs[q]]
            want, pos = refs[i]
            assert len(outs[i]) == pos[step], (level, i, j, scripts[i][step], len(outs[i]), pos[step])      # the call in which the bytes appear
            assert outs[i] == want[:pos[step]], (level, i, j)
            done[i] = what == END
    assert all(done[:-1])
    info = {k: v.cpu().tolist() for k, v in gpu.batch.stream_state_info(states, level).items()}
    assert info["error"][n - 1] == 201
    for i in range(n - 1):
        assert outs[i] == refs[i][0]
        assert outs[i] == gpu.compress_stream(datas[i], level, ck, flush_at=flushes[i]), (level, i)
        assert info["parsed"][i] == len(datas[i]) and info["error"][i] == 60 and info["closed"][i] == 1, (level, i)      # (60: every stream was called once more after its close)


def test_gpu_flush_inside_a_continue_call(gpu, oracle_ref, xml):
    """one call that does not close, with a new flush position below the source's size and full pieces behind it (the reference's flush call and its continue
    call in one): four streams of one launch, then their closes"""
    import torch
    P, level, ck = PIECE, 3, True
    cuts = [(1000, P, 5), (50000, 2 * P, 777), (P, P, 1), (P + 7, 2 * P, 0)]
    datas = [xml[9000 * k:9000 * k + sum(c)] for k, c in enumerate(cuts)]
    refs = [ref_calls(oracle_ref, d, level, ck, [(c[0], FLUSH), (c[1], CONT), (c[2], CONT), (0, END)]) for d, c in zip(datas, cuts)]
    n = len(cuts)
    states = gpu.batch.stream_states(n, level)
    fa = torch.tensor([c[0] for c in cuts], dtype=torch.int32, device="cuda")
    fo = offsets([1] * n)

    def call(srcs, mode):
        caps = [len(s) + (len(s) >> 8) + 4096 + 64 * 5 for s in srcs]
        blob, off = to_dev(b"".join(srcs)), offsets([len(s) for s in srcs])
        dst, doff = torch.zeros(sum(caps) + 8, dtype=torch.uint8, device="cuda"), offsets(caps)
        res = gpu.batch.compress_stream_continue(blob, off, dst, doff, states, level, ck, fa, fo, torch.tensor([mode] * n, dtype=torch.int32, device="cuda"))
        torch.cuda.synchronize()
        out, rs, dl = dst.cpu().numpy().tobytes(), res.cpu().tolist(), doff.cpu().tolist()
        assert all(r >= 0 for r in rs), rs
        return [out[dl[i]:dl[i] + rs[i]] for i in range(n)]

    first = call([d[:c[0] + c[1]] for d, c in zip(datas, cuts)], 4)
    last = call(datas, 1)
    info = {k: v.cpu().tolist() for k, v in gpu.batch.stream_state_info(states, level).items()}
    for i in range(n):
        want, pos = refs[i]
        assert first[i] == want[:pos[1]], (i, len(first[i]), pos[1])
        assert first[i] + last[i] == want and info["parsed"][i] == len(datas[i]), i


def _cs(gpu):
    L = gpu.lib()

    def call(h, data, directive, cap):
        dst = C.create_string_buffer(max(cap, 1))
        r = L.zjni_cstream_compress(h, dst, cap, data, len(data), directive)
        return -((1 << 64) - r) if L.zjni_isError(r) else dst.raw[:r]
    return L, call


def bound(new):
    return new + (new >> 8) + 4096 + 64 * 5


@pytest.mark.parametrize("level,ck", [(3, True), (1, False), (-1, False)])
def test_gpu_eager_handle(gpu, oracle_ref, xml, level, ck):
    """32 KiB writes to two pieces and a tail on an eager handle: a piece's bytes come out of a later call than the one that fills it, never later than the
    next flush or the close; a plain handle beside it returns everything with the close"""
    L, call = _cs(gpu)
    W, total = 32768, 2 * PIECE + 40000
    d = xml[777:777 + total]
    script = [(min(W, total - a), CONT) for a in range(0, total, W)] + [(0, END)]
    want, pos = ref_calls(oracle_ref, d, level, ck, script)
    h = L.zjni_createCStream2(level, int(ck), 1)
    plain = L.zjni_createCStream2(level, int(ck), 0)
    assert h and plain
    try:
        for frame in range(2):
            out, at, late = b"", 0, 0
            for k, (n, what) in enumerate(script):
                cap = L.zjni_cstream_pending(h) + (bound(total) if what == END else 0)
                got = call(h, d[at:at + n], what, cap)
                assert isinstance(got, bytes), (level, k, got)
                out += got
                at += n
                assert (pos[k - 1] if k else 0) <= len(out) <= pos[k], (level, k, len(out), pos[k])
                assert out == want[:len(out)]
                late += len(out) < pos[k]
                if what == CONT:
                    assert call(plain, d[at - n:at], what, 0) == b""
            assert out == want and L.zjni_cstream_pending(h) == 0
            assert late == 2, "each of the two pieces is launched by the call that fills it and handed out by a later one"
            assert call(plain, b"", END, bound(total)) == want and L.zjni_cstream_pending(plain) == 0          # the plain handle: as before, everything at the close
            assert call(h, b"x", CONT, 0) == -60
            assert L.zjni_cstream_reset(h) == 0 and L.zjni_cstream_reset(plain) == 0                          # the next frame on the same handles
        # a flush in the middle: what is held comes first; a destination too small for held + bound changes nothing
        out = call(h, d[:PIECE + 5000], CONT, 0)
        assert out == b""
        held = L.zjni_cstream_pending(h)
        ref_flush, fpos = ref_calls(oracle_ref, d[:PIECE + 5000 + 3], level, ck, [(PIECE + 5000, CONT), (0, FLUSH), (3, END)])
        assert held == fpos[0] > 0
        assert call(h, b"", FLUSH, held + bound(5000) - 1) == -70
        assert L.zjni_cstream_pending(h) == held
        assert call(h, b"", CONT, 10) == ref_flush[:10]                                                     # ... handed out as far as the destination allows
        assert L.zjni_cstream_pending(h) == held - 10
        assert call(h, b"", FLUSH, held - 10 + bound(5000) - 1) == -70
        got = call(h, b"", FLUSH, held - 10 + bound(5000))
        assert ref_flush[:10] + got == ref_flush[:fpos[1]] and L.zjni_cstream_pending(h) == 0
        assert ref_flush[:fpos[1]] + call(h, d[PIECE + 5000:PIECE + 5003], END, bound(3)) == ref_flush
        # reset with a piece in flight, then a second frame
        assert L.zjni_cstream_reset(h) == 0
        assert call(h, d[:PIECE], CONT, 0) == b""
        assert L.zjni_cstream_reset(h) == 0
        assert L.zjni_cstream_pending(h) == 0
        e = d[50000:50000 + PIECE + 9]
        got = call(h, e, CONT, 0)
        got += call(h, b"", END, L.zjni_cstream_pending(h) + bound(9))
        assert got == ref_calls(oracle_ref, e, level, ck, [(len(e), CONT), (0, END)])[0]
        # beyond the window: 201, what is held is dropped, the handle is dead until it is reset
        assert L.zjni_cstream_reset(h) == 0
        assert call(h, d[:PIECE], CONT, 0) == b""
        assert call(h, bytes(window(level)), CONT, 0) == -201
        assert L.zjni_cstream_pending(h) == 0 and call(h, b"", END, bound(0)) == -201
    finally:
        L.zjni_freeCStream(h)
        L.zjni_freeCStream(plain)
    assert not L.zjni_createCStream2(level, int(ck), 2)                                                       # an unknown flag


def test_gpu_eager_python_class(gpu, oracle_ref, xml):
    d = xml[123456:123456 + 3 * PIECE + 777]
    for level, ck in ((3, False), (2, True)):
        want = oracle_ref.compress_stream(d, level, ck, chunk=50000)
        s, p = gpu.ZstdCompressStream(level, ck, eager=True), gpu.ZstdCompressStream(level, ck)
        out = b""
        for a in range(0, len(d), 50000):
            got = s.write(d[a:a + 50000])
            assert isinstance(got, bytes)
            out += got
            assert p.write(d[a:a + 50000]) is None and p.pending() == 0
        assert 0 < len(out) < len(want) and s.pending() > 0                                 # the third piece was launched by the last write that filled it
        out += s.close()
        assert out == want == p.close() and s.pending() == 0
        s.reset()
        assert s.write(d[:PIECE]) == b""
        assert s.flush() + s.close() == oracle_ref.compress_stream(d[:PIECE], level, ck, chunk=PIECE)
        s.free(); p.free()
