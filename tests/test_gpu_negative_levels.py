"""GPU (-m gpu): negative compression levels (zstd's --fast=N) through the C-ABI, the Python classes and the JNI library.  Every frame is
byte-identical to the reference's ZSTD_compress2 at that level (row 0 parameters, stepSize = -L + 1, raw literals; levels below -131072
clamped).  Small batches take the fused kernel, batches from 4 096 frames the lane-per-frame matcher (zj_enc_match_kernel_neg /
zj_enc_match_wide_kernel_neg, ZJNI_ROUTE_LANE), frames above 128 KiB the multi-block kernel (zj_encode_multi_kernel_neg).  The CPU twin of
the kernel bodies is tests/test_emu_negative_levels.py."""
import ctypes as C
import os
import random
import subprocess
import threading

import pytest

from conftest import golden

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ZJNI_ROUTE_FUSED, ZJNI_ROUTE_LANE = 1, 3


@pytest.fixture(scope="module")
def gpu(zj):
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    zj.batch.init(0)
    return zj


def text(rnd, n):
    words = [b"alpha", b"beta", b"gamma", b"delta", b"epsilon", b"zeta", b"eta", b"theta", b"compress", b"level", b"\n"]
    out = bytearray()
    while len(out) < n:
        out += rnd.choice(words) + b" "
    return bytes(out[:n])


def small_set(gpu):
    rnd = random.Random(4)
    t = text(rnd, 600000)
    out = [b"", b"x", b"\x07" * 70000, (b"0123456789abcdefghij" * 7000)[:131072], bytes(rnd.getrandbits(8) for _ in range(40000)),
           t[:131072], t[:300000], t[:524288], golden("xmlsmall")[:20000]]
    out += [gpu.synth_host(n, n, 1) for n in (16384, 16385, 65536, 65537, 131072, 200000)]
    out += [gpu.synth_host(rnd.randrange(1, 70000), rnd.randrange(100000), 1) for _ in range(25)]
    return out


@pytest.mark.parametrize("level", [-1, -3, -7, -100, -131072, -200000])
def test_small_batch_byte_identical(gpu, oracle_ref, level):
    datas = small_set(gpu)
    for ck in (False, True):
        outs = gpu.compress_batch(datas, level, checksum=ck)
        for d, z in zip(datas, outs):
            assert not isinstance(z, Exception), (len(d), level, z)
            assert z == oracle_ref.compress(d, level, ck), (len(d), level, ck)
    assert gpu.lib().zjni_last_route() == ZJNI_ROUTE_FUSED


def test_beyond_the_window_and_explicit_table_sizes_are_refused(gpu):
    L = gpu.lib()
    big = gpu.synth_host(524289, 1, 1)
    outs = gpu.compress_batch([big, b"abc" * 100], -1)
    assert isinstance(outs[0], Exception) and isinstance(outs[1], bytes)
    dst = C.create_string_buffer(1 << 20)
    assert L.zjni_getErrorCode(L.zjni_compress(dst, 1 << 20, big, len(big), -3)) == 201
    sp = (C.c_void_p * 1)(C.cast(C.c_char_p(b"abcdefgh" * 100), C.c_void_p)); ss = (C.c_size_t * 1)(800)
    dp = (C.c_void_p * 1)(C.cast(dst, C.c_void_p)); dc = (C.c_size_t * 1)(1 << 20); res = (C.c_size_t * 1)()
    assert L.zjni_getErrorCode(L.zjni_compress_batch_advanced(sp, ss, dp, dc, res, 1, -2, 0, 14, 0)) == 40


@pytest.fixture(scope="module")
def large_set(gpu):
    rnd = random.Random(12)
    sizes = [rnd.choice([700, 4096, 9000, 16384, 30000, 65536]) if i % 64 else 100000 for i in range(8192)]
    return sizes, [gpu.synth_host(s, 7 * i + 3, 1) for i, s in enumerate(sizes)]


@pytest.mark.parametrize("level", [-1, -3, -7])
def test_large_batch_takes_the_lane_route(gpu, oracle_ref, large_set, level):
    """8 192 frames: the data-parallel lane-per-frame matcher; list A (<= 64 KiB) and list B (larger frames) both used"""
    sizes, datas = large_set
    outs = gpu.compress_batch(datas, level)
    L = gpu.lib()
    assert L.zjni_last_route() == ZJNI_ROUTE_LANE
    lists = (C.c_uint * 3)()
    assert L.zjni_last_lists(lists) == 0 and lists[0] > 0 and lists[1] >= 128, list(lists)
    bad = [i for i, (d, z) in enumerate(zip(datas, outs)) if z != oracle_ref.compress(d, level)]
    assert not bad, (len(bad), bad[:5])
    back = gpu.decompress_batch(outs[:512], sizes[:512])
    assert back == datas[:512]


def test_device_entry_and_round_trip(gpu, oracle_ref):
    import torch
    n, size = 64, 16384
    raw = gpu.synth_host(size, 11, n)
    bufs = [raw[i * size:(i + 1) * size] for i in range(n)]
    src = torch.frombuffer(bytearray(raw), dtype=torch.uint8).cuda()
    off = torch.arange(0, (n + 1) * size, size, dtype=torch.int64).cuda()
    cap = gpu.Zstd.compressBound(size)
    dst = torch.zeros(n * cap, dtype=torch.uint8).cuda()
    doff = torch.arange(0, (n + 1) * cap, cap, dtype=torch.int64).cuda()
    res = gpu.batch.compress(src, off, dst, doff, level=-4, checksum=True)
    torch.cuda.synchronize()
    res = res.cpu().tolist(); host = dst.cpu().numpy().tobytes()
    frames = [host[i * cap:i * cap + res[i]] for i in range(n)]
    for b, z in zip(bufs, frames):
        assert z == oracle_ref.compress(b, -4, True)
    assert gpu.decompress_batch(frames, [size] * n) == bufs


def test_blocking_entries_begin_finish_and_multi(gpu, oracle_ref):
    L = gpu.lib()
    rnd = random.Random(2)
    datas = [gpu.synth_host(rnd.randrange(1, 200000), i, 1) for i in range(40)]
    n = len(datas)
    caps = [gpu.Zstd.compressBound(len(d)) for d in datas]
    srcb = [C.create_string_buffer(d, len(d)) for d in datas]
    dsts = [C.create_string_buffer(c) for c in caps]
    sp = (C.c_void_p * n)(*[C.cast(b, C.c_void_p) for b in srcb]); ss = (C.c_size_t * n)(*[len(d) for d in datas])
    dp = (C.c_void_p * n)(*[C.cast(b, C.c_void_p) for b in dsts]); dc = (C.c_size_t * n)(*caps)

    def check(level, ck):
        for i, d in enumerate(datas):
            assert dsts[i].raw[:res[i]] == oracle_ref.compress(d, level, ck), (i, level)
    res = (C.c_size_t * n)()
    assert L.zjni_compress_batch(sp, ss, dp, dc, res, n, -2) == 0; check(-2, False)
    assert L.zjni_compress_batch2(sp, ss, dp, dc, res, n, -5, 1) == 0; check(-5, True)
    assert L.zjni_compress_batch_advanced(sp, ss, dp, dc, res, n, -9, 0, 0, 0) == 0; check(-9, False)
    job = L.zjni_compress_batch_begin(sp, ss, dp, dc, res, n, -6, 0)
    assert job and L.zjni_batch_finish(job) == 0; check(-6, False)
    dv = (C.c_int * 1)(0)
    for mode in (0, 1):
        assert L.zjni_compress_batch_multi(sp, ss, dp, dc, res, n, -3, 0, dv, 1, mode) == 0; check(-3, False)
    for level in (-1, -8):
        r = L.zjni_compress(dsts[0], caps[0], srcb[0], len(datas[0]), level)
        assert dsts[0].raw[:r] == oracle_ref.compress(datas[0], level)
        r = L.zjni_compress2(dsts[1], caps[1], srcb[1], len(datas[1]), level, 1)
        assert dsts[1].raw[:r] == oracle_ref.compress(datas[1], level, True)


def test_aggregator(gpu, oracle_ref):
    L = gpu.lib()
    agg = L.zjni_createAggregator(0, 256, 20000)
    assert agg
    bufs = {(t, j): gpu.synth_host([700, 4096, 20000, 65536][(t + j) % 4], 31 * t + j, 1) for t in range(16) for j in range(4)}
    out, errs = {}, []

    def worker(t):
        try:
            for j in range(4):
                d = bufs[t, j]; level = [-1, -2, 1, -1][j]; ck = t % 2
                cap = gpu.Zstd.compressBound(len(d)); dst = C.create_string_buffer(cap)
                r = L.zjni_aggregator_compress(agg, dst, cap, d, len(d), level, ck)
                assert not L.zjni_isError(r), L.zjni_getErrorCode(r)
                back = C.create_string_buffer(len(d))
                assert L.zjni_aggregator_decompress(agg, back, len(d), dst.raw[:r], r) == len(d) and back.raw == d
                out[t, j] = (level, ck, dst.raw[:r])
        except Exception as ex:                             # noqa: BLE001
            errs.append(repr(ex))
    th = [threading.Thread(target=worker, args=(t,)) for t in range(16)]
    for x in th: x.start()
    for x in th: x.join()
    assert not errs, errs[:3]
    for (t, j), (level, ck, z) in out.items():
        assert z == oracle_ref.compress(bufs[t, j], level, bool(ck)), (t, j, level)
    L.zjni_freeAggregator(agg)


def test_python_classes(gpu, oracle_ref):
    d = golden("xmlsmall")
    assert gpu.Zstd.compress(d, -5) == oracle_ref.compress(d, -5)
    with gpu.ZstdCompressCtx() as ctx:
        ctx.setLevel(-5)
        assert ctx.compress(d) == oracle_ref.compress(d, -5)
        ctx.setLevel(-1).setChecksum(True)
        assert ctx.compress(d) == oracle_ref.compress(d, -1, True)
    assert gpu.Zstd.decompress(gpu.Zstd.compress(d, -30), len(d)) == d


def test_jni_compress_natives_on_the_gpu():
    shim = os.path.join(ROOT, "zstd-jni_amd", "lib", "libzstd-jni-amd.so")
    refjni = os.path.join(ROOT, "oracle", "_ref", "libzstd-jni-ref.so")
    assert os.path.exists(shim) and os.path.exists(refjni), "prebuilt JNI shim / reference JNI library missing"
    exe = os.path.join(ROOT, "tests", "jni", "_build", "negative_levels")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["gcc", "-O1", "-g", "-std=c99", "-Wall", "-I" + os.path.join(ROOT, "zstd-jni_amd", "jni", "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "jni", "negative_levels.c"), "-ldl"])
    env = dict(os.environ, ZSTD_JNI_CPU_LIB=refjni, ZSTD_JNI_GPU_PER_BUFFER="1")
    out = subprocess.run([exe, refjni, shim], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "NEGATIVE-LEVELS OK" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
