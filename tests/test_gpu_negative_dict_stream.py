"""GPU (-m gpu): negative compression levels (zstd's --fast=N) with compression dictionaries and in compress streams, through the C-ABI, the Python
classes and the JNI library.  A CDict of level -N (zjni_createCDict: row 0 parameters, targetLength = N) makes frames byte-identical to the reference's
ZSTD_createCDict(dict, -N) + ZSTD_CCtx_refCDict + ZSTD_compress2: attach mode on zj_enc_match_dict_kernel_neg, copy mode on
zj_encode_cdict_copy_kernel_neg, 40 / 201 where levels 1-3 give them.  Streams at -N (zjni_compress_stream, zjni_compress_stream_batch_device) make
what ZSTD_compressStream2 writes without a pledged size.  The CPU twin of the kernel bodies is tests/test_emu_negative_dict_stream.py."""
import ctypes as C
import itertools
import os
import random
import subprocess

import pytest

from conftest import golden
from util import json_records

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ZJNI_FRAME_CHECKSUM, ZJNI_FRAME_NO_DICTID = 1, 4


@pytest.fixture(scope="module")
def gpu(zj):
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    zj.batch.init(0)
    return zj


@pytest.fixture(scope="module")
def corpus(oracle_ref):
    recs = json_records(30000, seed=3)
    samples = [b",".join(recs[i * 13:i * 13 + 200])[:4096] for i in range(1500)]
    return recs, oracle_ref.train_dict(samples, 112640), oracle_ref.train_dict(samples, 16384)


def batch_flags(gpu, srcs, cd, flags):
    """zjni_compress_batch_usingCDict with a frame-flag word (checksum / no dictID)"""
    L = gpu.lib()
    n = len(srcs)
    keep = [C.create_string_buffer(bytes(s), max(len(s), 1)) for s in srcs]
    caps = [gpu.Zstd.compressBound(len(s)) for s in srcs]
    outs = [C.create_string_buffer(max(c, 1)) for c in caps]
    res = (C.c_size_t * n)()
    r = L.zjni_compress_batch_usingCDict((C.c_void_p * n)(*[C.addressof(k) for k in keep]), (C.c_size_t * n)(*[len(s) for s in srcs]),
                                         (C.c_void_p * n)(*[C.addressof(o) for o in outs]), (C.c_size_t * n)(*caps), res, n, cd._ptr, flags)
    assert r == 0
    return [(-L.zjni_getErrorCode(res[i]) if L.zjni_isError(res[i]) else outs[i].raw[:res[i]]) for i in range(n)]


def mixed(recs, rnd, n):
    """records in the attach range, sources in copy mode, and the two refusals: 201 above one block, 40 at 128 KiB where the dictionary is small"""
    out = []
    for i in range(n):
        k = rnd.randrange(0, len(recs) - 3000)
        size = rnd.choice([0, 1, 7, 100, 1000, 4096, 4096, 4096, 8192, rnd.randrange(0, 8193), 8193, 20000, rnd.randrange(8193, 131072), 131072, 131073])
        out.append(b",".join(recs[k:k + 3000])[:size] if size <= 131072 else bytes(size))
    return out


@pytest.mark.parametrize("level", [-1, -3, -7, -131072, -200000])
def test_cdict_small_batches(gpu, oracle_ref, corpus, level):
    recs, d110, d16 = corpus
    rnd = random.Random(700 - level)
    for d in (d110, d16):
        ref = oracle_ref.CDict(d, level)
        small = d is d16                                     # content < 128 KiB / 6: a 128 KiB source re-derives the parameters (40); the 110 KiB one keeps them
        with gpu.ZstdDictCompress(d, level) as cd, gpu.ZstdDictDecompress(d) as dd:
            assert cd.level() == level and cd.getDictID() == oracle_ref.dict_id(d)
            for n, flags in ((1, 0), (40, ZJNI_FRAME_CHECKSUM), (300, ZJNI_FRAME_NO_DICTID), (300, ZJNI_FRAME_CHECKSUM | ZJNI_FRAME_NO_DICTID)):
                srcs = mixed(recs, rnd, n)
                frames = batch_flags(gpu, srcs, cd, flags)
                for k, (x, z) in enumerate(zip(srcs, frames)):
                    if len(x) > 131072:
                        assert z == -201, (k, z)
                    elif len(x) == 131072 and small:
                        assert z == -40, (k, z)
                    else:
                        assert z == ref.compress(x, bool(flags & 1), not flags & 4), (level, len(d), n, k, len(x))
                good = [(x, z) for x, z in zip(srcs, frames) if isinstance(z, bytes)]
                outs = gpu.decompress_batch([z for _, z in good], [len(x) for x, _ in good], dd)
                assert all(o == x for (x, _), o in zip(good, outs))


def test_cdict_large_batch(gpu, oracle_ref, corpus):
    """8 192 frames of BASELINE config 4's shape (4 KiB records, 110 KiB dictionary), refusal slots and copy-mode sources mixed in"""
    recs, d110, _ = corpus
    rnd = random.Random(5)
    srcs = []
    for i in range(8192):
        k = rnd.randrange(0, len(recs) - 3000)
        size = 4096 if i % 17 else rnd.choice([0, 33, 8193, 50000, 131073])
        srcs.append(b",".join(recs[k:k + 3000])[:size] if size <= 131072 else bytes(size))
    for level in (-1, -5):
        ref = oracle_ref.CDict(d110, level)
        with gpu.ZstdDictCompress(d110, level) as cd, gpu.ZstdDictDecompress(d110) as dd:
            frames = gpu.compress_batch(srcs, checksum=True, dictionary=cd)
            for k, (x, z) in enumerate(zip(srcs, frames)):
                if len(x) > 131072:
                    assert isinstance(z, gpu.ZstdException) and z.getErrorCode() == 201
                else:
                    assert z == ref.compress(x, checksum=True), (level, k, len(x))
            good = [(x, z) for x, z in zip(srcs, frames) if isinstance(z, bytes)]
            outs = gpu.decompress_batch([z for _, z in good], [len(x) for x, _ in good], dd)
            assert all(o == x for (x, _), o in zip(good, outs))


def test_cdict_refusals_and_python_classes(gpu, oracle_ref, corpus):
    recs, d110, d16 = corpus
    with pytest.raises(gpu.ZstdException):
        gpu.ZstdDictCompress(b"abcdefg", -1)                 # under 8 bytes: no CDict
    x = b",".join(recs[10:60])[:3000]
    with gpu.ZstdDictCompress(d16, -4) as cd:
        assert gpu.Zstd.compress(x, cd) == oracle_ref.CDict(d16, -4).compress(x)
        with gpu.ZstdCompressCtx() as ctx:
            ctx.loadDict(cd)
            assert ctx.compress(x) == oracle_ref.CDict(d16, -4).compress(x)
    with gpu.ZstdCompressCtx() as ctx:                       # setLevel(-N).loadDict(byte[]): the local CDict at -N
        ctx.setLevel(-6).loadDict(d16)
        assert ctx.compress(x) == oracle_ref.CDict(d16, -6).compress(x)
    big = b",".join(recs[:3000])[:131072]
    with gpu.ZstdDictCompress(b",".join(recs[:30])[:2000], -2) as cd:
        f = gpu.compress_batch([big, x], dictionary=cd)
        assert isinstance(f[0], gpu.ZstdException) and f[0].getErrorCode() == 40     # 128 KiB and >= 6 x the dictionary: the reference re-derives the parameters


def stream_inputs(gpu, oracle_ref, size, rnd):
    xml = oracle_ref.decompress(golden("xml-1.zst"), 6_000_000)
    o = rnd.randrange(0, len(xml) - size - 1)
    return [xml[o:o + size], b"".join(gpu.synth_host(65536, i, 1) for i in range(size // 65536 + 1))[:size]]


def test_stream_single_entry(gpu, oracle_ref):
    rnd = random.Random(13)
    n = 0
    for size in (0, 1, 100, 131071, 131072, 131073, 262144, 262145, 393216, 524287, 524288):
        for d in stream_inputs(gpu, oracle_ref, size, rnd):
            for level in (-1, -3, -7, -131072, -200000):
                ck = bool(n & 1); n += 1
                got = gpu.compress_stream(d, level, ck)
                assert got == oracle_ref.compress_stream(d, level, ck), (size, level, ck)
                assert oracle_ref.decompress(got, max(size, 1)) == d
    for level in (-1, -9):
        with pytest.raises(gpu.ZstdException) as e:
            gpu.compress_stream(bytes(524289), level)
        assert e.value.getErrorCode() == 201
        assert gpu.compress_stream(b"", level, False, final=False, known_empty=False) == b""
    for size in (50000, 300000, 524288):                     # flushes, and the frame's beginning when flushed but not closed
        for d in stream_inputs(gpu, oracle_ref, size, rnd):
            for chunk, k in ((50000, 1), (10000, 3), (131072, 1)):
                calls = (size + chunk - 1) // chunk
                flushes = [min(j * chunk, size) for j in range(1, calls + 1) if j % k == 0]
                full = gpu.compress_stream(d, -2, True, flush_at=flushes)
                assert full == oracle_ref.compress_stream(d, -2, True, chunk=chunk, flush_every=k), (size, chunk, k)
                if flushes and flushes[-1] < size:
                    part = gpu.compress_stream(d[:flushes[-1]], -2, True, flush_at=flushes, final=False)
                    assert part and full.startswith(part), (size, chunk, k)


def test_stream_batch_on_the_device(gpu, oracle_ref):
    import torch
    rnd = random.Random(19)
    sizes = [rnd.choice([0, 5000, 70000, 131072, 140000, 300000, 524288, 524289]) for _ in range(32)]
    datas = [gpu.synth_host(65536, 80 + i, 9)[:s] if s <= 589824 else bytes(s) for i, s in enumerate(sizes)]
    dev = "cuda"
    blob = torch.frombuffer(bytearray(b"".join(datas) or b"\0"), dtype=torch.uint8).to(dev)
    off = torch.tensor([0] + list(itertools.accumulate(sizes)), dtype=torch.int64, device=dev)
    caps = [s + (s >> 8) + 4096 for s in sizes]
    doff = torch.tensor([0] + list(itertools.accumulate(caps)), dtype=torch.int64, device=dev)
    dst = torch.zeros(sum(caps), dtype=torch.uint8, device=dev)
    res = torch.zeros(len(sizes), dtype=torch.int64, device=dev)
    mode = torch.tensor([1 | (2 if s == 0 else 0) for s in sizes], dtype=torch.int32, device=dev)
    L = gpu.lib()
    for level in (-1, -4):
        r = L.zjni_compress_stream_batch_device(blob.data_ptr(), off.data_ptr(), dst.data_ptr(), doff.data_ptr(), res.data_ptr(), len(sizes), level, 1, None, None,
                                                mode.data_ptr(), torch.cuda.current_stream().cuda_stream)
        assert r == 0
        torch.cuda.synchronize()
        out = dst.cpu().numpy().tobytes(); rs = [v & ((1 << 64) - 1) for v in res.cpu().tolist()]; dl = doff.cpu().tolist()
        for i, d in enumerate(datas):
            if len(d) > 524288:
                assert L.zjni_isError(rs[i]) and L.zjni_getErrorCode(rs[i]) == 201
                continue
            assert not L.zjni_isError(rs[i]), (i, sizes[i])
            assert out[dl[i]:dl[i] + rs[i]] == oracle_ref.compress_stream(d, level, True), (level, i, sizes[i])


def test_jni_dictionary_and_stream_natives_on_the_gpu():
    shim = os.path.join(ROOT, "zstd-jni_amd", "lib", "libzstd-jni-amd.so")
    refjni = os.path.join(ROOT, "oracle", "_ref", "libzstd-jni-ref.so")
    assert os.path.exists(shim) and os.path.exists(refjni), "prebuilt JNI shim / reference JNI library missing"
    exe = os.path.join(ROOT, "tests", "jni", "_build", "negative_dict_stream")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["gcc", "-O1", "-g", "-std=c99", "-Wall", "-I" + os.path.join(ROOT, "zstd-jni_amd", "jni", "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "jni", "negative_dict_stream.c"), "-ldl"])
    env = dict(os.environ, ZSTD_JNI_CPU_LIB=refjni, ZSTD_JNI_GPU_PER_BUFFER="1")
    out = subprocess.run([exe, refjni, shim], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "NEGATIVE-DICT-STREAM OK" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
