"""GPU (-m gpu): compress streams continued from device state — zjni_compress_stream_continue_batch_device (ze_compress_stream_resume on
zj_encode_stream_continue_kernel), the host form zjni_cstream_* and zstd_jni_amd.ZstdCompressStream.  The calls' outputs, concatenated, are the frame the existing
route (zjni_compress_stream) writes for the whole stream and ZSTD_compressStream2's (oracle/ref.py compress_stream); the states' counters show that no byte was
parsed twice.  The cases of tests/test_emu_cstream.py on the device, a batch of streams driven in lock-step."""
import itertools
import random

import pytest

from conftest import golden

pytestmark = pytest.mark.gpu
FLUSH, END, WRITE = "flush", "end", "write"


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


def offsets(sizes, dtype=None):
    import torch
    return torch.tensor([0] + list(itertools.accumulate(sizes)), dtype=dtype or torch.int64, device="cuda")


def blocks_of(frame, ck):
    """(type, size, last) of the frame's blocks"""
    at, out = 6, []
    while True:
        h = frame[at] | frame[at + 1] << 8 | frame[at + 2] << 16
        out.append(((h >> 1) & 3, h >> 3, h & 1))
        at += 3 + (1 if (h >> 1) & 3 == 1 else h >> 3)
        if h & 1:
            break
    assert at + (4 if ck else 0) == len(frame)
    return out


class Batch:
    """n streams of one level behind one state tensor; call() is one zjni_compress_stream_continue_batch_device over all of them"""

    def __init__(self, gpu, n, level, ck, states=None):
        self.gpu, self.n, self.level, self.ck = gpu, n, level, ck
        self.states = gpu.batch.stream_states(n, level) if states is None else states
        self.buf = [bytearray() for _ in range(n)]
        self.flushes = [[] for _ in range(n)]
        self.touched = [False] * n

    def info(self):
        return {k: v.cpu().tolist() for k, v in self.gpu.batch.stream_state_info(self.states, self.level).items()}

    def call(self, steps, caps=None, level=None, ck=None, src=None):
        """steps[i] = (new bytes, FLUSH | END | WRITE) -> per stream the new frame bytes, or the negative code"""
        import torch
        consumed = self.info()["consumed"]
        mode, new_fl = [], []
        for i, (data, what) in enumerate(steps):
            known_empty = what == END and not self.touched[i] and not data
            self.touched[i] = True
            self.buf[i] += data
            if what == FLUSH:
                self.flushes[i].append(len(self.buf[i]))
            mode.append((1 if what == END else 0) | (2 if known_empty else 0))
            new_fl.append(self.flushes[i] if i % 2 else [f for f in self.flushes[i] if f > consumed[i]])       # all of them, or only the new ones
        srcs = [bytes(b) for b in self.buf] if src is None else src
        if caps is None:
            caps = [len(s) - min(c, len(s)) + ((len(s) - min(c, len(s))) >> 8) + 4096 + 64 * (len([f for f in fl if f > c]) + 4) for s, c, fl in zip(srcs, consumed, new_fl)]
        blob, off = to_dev(b"".join(srcs)), offsets([len(s) for s in srcs])
        dst, doff = torch.zeros(sum(caps) + 8, dtype=torch.uint8, device="cuda"), offsets(caps)
        fa = torch.tensor(list(itertools.chain(*new_fl)) or [0], dtype=torch.int64, device="cuda").to(torch.int32)
        fo = offsets([len(f) for f in new_fl])
        md = torch.tensor(mode, dtype=torch.int32, device="cuda")
        res = self.gpu.batch.compress_stream_continue(blob, off, dst, doff, self.states, self.level if level is None else level, self.ck if ck is None else ck, fa, fo, md)
        torch.cuda.synchronize()
        out, rs, dl = dst.cpu().numpy().tobytes(), res.cpu().tolist(), doff.cpu().tolist()
        return [out[dl[i]:dl[i] + r] if r >= 0 else r for i, r in enumerate(rs)]


def scripts_for(size, k):
    """the script classes of tests/test_emu_cstream.py, one per stream"""
    w = max(size // 3, 1)
    return [
        [(size, END)],                                                                                # one write, closed (size 0: the size is known)
        [(min(w, size - a), FLUSH) for a in range(0, size, w)] + [(0, END)],                          # a flush after every write, close right after a flush
        [(min(1000, size), FLUSH), (0, FLUSH), (0, FLUSH), (size - min(1000, size), WRITE), (0, END)],   # flushes with nothing new, close with bytes buffered
        [(0, WRITE), (size // 2, WRITE), (size - size // 2, FLUSH), (0, FLUSH), (0, END)],            # first calls that flush nothing, two flushes at one position
        [(min(1000, size), FLUSH), (size - min(1000, size), END)],                                    # a full piece behind a resume, data arriving with the close
    ][k % 5]


@pytest.mark.parametrize("level", [1, 2, 3, -3])
def test_gpu_cstream_batch_in_lock_step(gpu, oracle_ref, xml, level):
    """call j carries every stream's j-th directive: fresh streams, mid-stream ones, closing ones and ones with nothing new share a launch; a stream that
    was closed in an earlier call answers 60 in every later one"""
    rnd = random.Random(50 + level)
    ck = level in (2, -3)
    sizes = [0, 1, 70000, 131072, 200000, 300000, 524288, 70000, 200000, 131072]
    datas, scripts = [], []
    for k, size in enumerate(sizes):
        o = rnd.randrange(0, len(xml) - size - 1)
        datas.append(xml[o:o + size] if k % 2 else b"".join(gpu.synth_host(65536, 7 * k + i, 1) for i in range(size // 65536 + 1))[:size])
        scripts.append(scripts_for(size, k + (level & 3)))
    n = len(sizes)
    b = Batch(gpu, n, level, ck)
    outs, at, done = [b""] * n, [0] * n, [False] * n
    for j in range(max(len(s) for s in scripts)):
        before = b.info()
        steps = []
        for i in range(n):
            cnt, what = scripts[i][j] if j < len(scripts[i]) else (0, WRITE)
            steps.append((datas[i][at[i]:at[i] + cnt], what)); at[i] += cnt
        got = b.call(steps)
        after = b.info()
        for i in range(n):
            if done[i]:
                assert got[i] == -60 and after["error"][i] == 60, (level, i, j)                      # closed: stage_wrong, and from then on
                continue
            assert isinstance(got[i], bytes), (level, i, j, got[i])
            outs[i] += got[i]
            newest = max(b.flushes[i] + [0])
            if steps[i][1] == END:
                done[i] = True
                assert after["closed"][i] == 1 and after["consumed"][i] == len(datas[i])
            else:
                assert after["consumed"][i] == newest
                assert after["parsed"][i] - before["parsed"][i] == newest - before["consumed"][i], (level, i, j)       # no rework
                if newest == before["consumed"][i]:
                    assert got[i] == b"" and after["blocks"][i] == before["blocks"][i]
            assert after["produced"][i] == len(outs[i])
    assert all(done)
    final = b.info()
    for i in range(n):
        assert outs[i] == gpu.compress_stream(datas[i], level, ck, flush_at=b.flushes[i], known_empty=(sizes[i] == 0 and len(scripts[i]) == 1)), (level, i, sizes[i])
        if len(scripts[i]) == 1:
            assert outs[i] == oracle_ref.compress_stream(datas[i], level, ck, chunk=131072), (level, i)
        elif all(w == FLUSH for _, w in scripts[i][:-1]) and scripts[i][-1] == (0, END) and sizes[i] >= 3:
            assert outs[i] == oracle_ref.compress_stream(datas[i], level, ck, chunk=max(sizes[i] // 3, 1), flush_every=1), (level, i)
        assert oracle_ref.decompress(outs[i], max(sizes[i], 1)) == datas[i]
        real = [x for x in blocks_of(outs[i], ck) if not (x[0] == 0 and x[1] == 0)]
        assert final["parsed"][i] == sizes[i] and final["blocks"][i] == len(real), (level, i)


def test_gpu_cstream_refusals(gpu, xml):
    d = xml[1000:121000]
    level = 1
    b = Batch(gpu, 5, level, False)
    got = b.call([(bytes((1 << 19) + 1), FLUSH)] + [(d[:50000], FLUSH)] * 4)
    assert got[0] == -201 and all(isinstance(g, bytes) and g for g in got[1:])
    probe = Batch(gpu, 1, level, False)
    probe.call([(d[:50000], FLUSH)])
    need = len(probe.call([(d[50000:], FLUSH)])[0])                                          # what stream 4's next call writes
    assert need > 18
    # stream 1 is closed here and called again below; 3: less than what was consumed; 4: a slot one byte short
    got = b.call([(b"", FLUSH), (d[50000:], END), (d[50000:], FLUSH), (b"", FLUSH), (d[50000:], FLUSH)],
                 caps=[4096, 80000, 80000, 4096, need - 1], src=[b"", d, d, d[:49999], d])
    assert got[0] == -201 and isinstance(got[1], bytes) and isinstance(got[2], bytes) and got[3] == -60 and got[4] == -70
    got = b.call([(b"", FLUSH), (b"x", FLUSH), (b"", FLUSH), (b"", FLUSH), (b"", FLUSH)])
    assert got[0] == -201 and got[1] == -60 and got[2] == b"" and got[3] == -60 and got[4] == -70
    assert b.call([(b"", END)] * 5) [0:2] == [-201, -60]
    assert b.info()["error"] == [201, 60, 0, 60, 70] and b.info()["closed"][2] == 1
    # begun with another level word / another checksum flag (one stream in a tensor of four level-1 states: room for a level-2 state, whose stride the wrong call takes)
    for kw in ({"level": 2}, {"level": -1}, {"ck": True}):
        s = Batch(gpu, 1, level, False, states=gpu.batch.stream_states(4, level))
        assert isinstance(s.call([(d[:50000], FLUSH)])[0], bytes)
        assert s.call([(d[50000:60000], FLUSH)], **kw) == [-60]
        assert s.call([(b"", FLUSH)]) == [-60] and s.info()["error"][0] == 60
    assert gpu.lib().zjni_cstream_state_bytes(4) == 0
    with pytest.raises(gpu.ZstdException) as e:
        gpu.batch.stream_states(1, 5)
    assert e.value.getErrorCode() == 42


def test_gpu_cstream_host_form_and_python_class(gpu, oracle_ref, xml):
    rnd = random.Random(77)
    for level, ck, w, total in ((3, False, 16384, 300000), (1, True, 50000, 524288), (-5, False, 10000, 95000), (2, True, 131072, 400000), (3, True, 1000, 20500)):
        o = rnd.randrange(0, len(xml) - total - 1)
        d = xml[o:o + total]
        s = gpu.ZstdCompressStream(level, ck)
        for frame in range(2):                                                 # reset(): the next frame on the same handle
            out = b""
            for a in range(0, total, w):
                s.write(d[a:a + w // 2]); s.write(d[a + w // 2:a + w])
                out += s.flush()
            assert s.flush() == b""
            out += s.close()
            assert out == oracle_ref.compress_stream(d, level, ck, chunk=w, flush_every=1), (level, ck, w, frame)
            assert out == gpu.compress_stream(d, level, ck, flush_at=[min(a + w, total) for a in range(0, total, w)])
            with pytest.raises(gpu.ZstdException) as e:
                s.write(b"x")
            assert e.value.getErrorCode() == 60                                # closed: stage_wrong until reset()
            s.reset()
            d = d[::-1] if frame == 0 else d
        s.free()
    # closed before anything else: the size (0) is known; flushed empty first: it is not
    s = gpu.ZstdCompressStream(3, True)
    assert s.close() == oracle_ref.compress_stream(b"", 3, True)
    s.reset()
    assert s.flush() == b""
    assert s.close() == gpu.compress_stream(b"", 3, True, flush_at=[0], known_empty=False)
    # a destination below the bound: dstSize_tooSmall, and the stream goes on as if the call had not been made
    s.reset()
    d = xml[5000:105000]
    s.write(d[:40000])
    bound = 40000 + (40000 >> 8) + 4096 + 64 * 5
    with pytest.raises(gpu.ZstdException) as e:
        s.flush(capacity=bound - 1)
    assert e.value.getErrorCode() == 70
    out = s.flush(capacity=bound)
    s.write(d[40000:])
    with pytest.raises(gpu.ZstdException) as e:
        s.close(capacity=100)
    assert e.value.getErrorCode() == 70
    out += s.close()
    assert oracle_ref.decompress(out, len(d)) == d
    assert out == gpu.compress_stream(d, 3, True, flush_at=[40000])
    s.free()
    # beyond the window: 201, the handle is dead until it is reset
    s = gpu.ZstdCompressStream(1, False)
    s.write(bytes(300000))
    assert s.flush()
    with pytest.raises(gpu.ZstdException) as e:
        s.write(bytes(300000))
    assert e.value.getErrorCode() == 201
    for call in (s.flush, s.close, lambda: s.write(b"a")):
        with pytest.raises(gpu.ZstdException) as e:
            call()
        assert e.value.getErrorCode() == 201
    s.reset()
    s.write(b"abc")
    assert s.close() == oracle_ref.compress_stream(b"abc", 1, False)
    with pytest.raises(gpu.ZstdException):
        gpu.ZstdCompressStream(4)


def test_gpu_cstream_ordered_with_other_batch_calls(gpu, oracle_ref, xml):
    """a continuation call and a plain compress batch of multi-block frames on two torch streams, back to back: both take the device's scratch slots, so the
    second has to wait for the first (BatchOrder) — both results are right"""
    import torch
    n, size = 24, 200000
    datas = [xml[i * 150000:i * 150000 + size] for i in range(n)]
    b = Batch(gpu, n, 3, False)
    first = b.call([(d[:100000], FLUSH) for d in datas])
    blob, off = to_dev(b"".join(datas)), offsets([size] * n)
    caps = [size + 4096] * n
    dst1, dst2, doff = torch.zeros(sum(caps), dtype=torch.uint8, device="cuda"), torch.zeros(sum(caps), dtype=torch.uint8, device="cuda"), offsets(caps)
    md = torch.ones(n, dtype=torch.int32, device="cuda")
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s1):
        r1 = gpu.batch.compress_stream_continue(blob, off, dst1, doff, b.states, 3, False, None, None, md)
    with torch.cuda.stream(s2):
        r2 = gpu.batch.compress(blob, off, dst2, doff, 3)
    torch.cuda.synchronize()
    o1, o2, r1, r2, dl = dst1.cpu().numpy().tobytes(), dst2.cpu().numpy().tobytes(), r1.cpu().tolist(), r2.cpu().tolist(), doff.cpu().tolist()
    for i, d in enumerate(datas):
        assert r1[i] > 0 and r2[i] > 0
        assert first[i] + o1[dl[i]:dl[i] + r1[i]] == gpu.compress_stream(d, 3, False, flush_at=[100000]), i
        assert o2[dl[i]:dl[i] + r2[i]] == oracle_ref.compress(d, 3), i
