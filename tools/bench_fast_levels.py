"""Compress-call rate at zstd's fast levels, torch-free (the C-ABI and the HIP runtime through ctypes, as tools/prof_driver.py):
one JSON line per level, all in one process on one device.  For each level: the synthetic set (zj_synth.h) of N buffers of SIZE bytes
on the device, zjni_compress_batch_device2 timed with HIP events (warmup calls first, best and mean of the timed ones), the whole batch's
frames packed on the device and compared byte for byte with the reference's frames of the same buffers, and the reference's rate on
16 host threads (oracle.port.cpu_baseline2: reused contexts, barrier start, best pass).

--dict: BASELINE config 4's shape instead — the JSON-like records of bench.py's dictionary mode (class 1 of the generator: buffers 4 i + 1; 2^20 x 4 KiB
unless --n / --size say otherwise) and its 110 KiB dictionary trained the same way from 10 000 records; each level gets its own ZstdDictCompress
(zjni_createCDict) and zjni_compress_batch_device_usingCDict is timed; the reference's frames and rate are ZSTD_createCDict at that level +
ZSTD_CCtx_refCDict + ZSTD_compress2 on the same threads.

usage: python tools/bench_fast_levels.py [--dict] [--n 65536] [--size 65536] [--levels 1,-1,-3,-7] [--steps 5] [--warmup 2] [--threads 16]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry          # noqa: E402
from oracle import port                  # noqa: E402

GIB = float(1 << 30)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dict", action="store_true", help="config 4: 4 KiB JSON-like records against a shared 110 KiB trained dictionary")
    ap.add_argument("--n", type=int, default=None, help="buffers (default 65536; 1048576 with --dict)")
    ap.add_argument("--size", type=int, default=None, help="bytes per buffer (default 65536; 4096 with --dict)")
    ap.add_argument("--levels", default="1,-1,-3,-7")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--cpu-seconds", type=float, default=1.0)
    ap.add_argument("--no-reference", action="store_true", help="GPU timing only (no identity check, no CPU leg): for runs under a profiler")
    a = ap.parse_args()
    zj = entry.load_package()
    L = zj.lib()
    hip = C.CDLL("libamdhip64.so")
    vp = C.c_void_p

    def chk(r):
        assert r == 0, r

    def dmalloc(nb):
        p = vp(); chk(hip.hipMalloc(C.byref(p), C.c_size_t(nb))); return p

    def upload(arr):
        p = dmalloc(arr.nbytes); chk(hip.hipMemcpy(p, arr.ctypes.data_as(vp), C.c_size_t(arr.nbytes), 1)); return p

    n = a.n if a.n else (1 << 20 if a.dict else 65536)
    size = a.size if a.size else (4096 if a.dict else 65536)
    assert L.zjni_init(0) == 0
    bound = int(L.zjni_compressBound(size))
    src = dmalloc(n * size); comp = dmalloc(n * bound); packed = dmalloc(n * bound)
    soff = upload(np.arange(n + 1, dtype=np.uint64) * size); coff = upload(np.arange(n + 1, dtype=np.uint64) * bound)
    csz = dmalloc(n * 8); poff = dmalloc((n + 1) * 8)
    dict_bytes = None
    if a.dict:
        # bench.py's dictionary mode: the generator's class-1 buffers (indices 4 i + 1) and a 110 KiB dictionary trained from 10 000 of them
        from oracle import ref
        big = dmalloc(4 * n * size)
        chk(L.zjni_synth_fill_device(big, size, 0, 4 * n, None))
        hip.hipMemcpy2D.argtypes = [vp, C.c_size_t, vp, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int]
        chk(hip.hipMemcpy2D(src, size, vp(big.value + size), 4 * size, size, n, 3))
        chk(hip.hipDeviceSynchronize()); chk(hip.hipFree(big))
        train = zj.synth_host(size, (1 << 24), 40000)
        dict_bytes = ref.train_dict([train[i * size:(i + 1) * size] for i in range(1, 40000, 4)], 112640)
    else:
        chk(L.zjni_synth_fill_device(src, size, 0, n, None))
    chk(hip.hipDeviceSynchronize())
    host = None
    if not a.no_reference:
        host = np.empty(n * size, dtype=np.uint8)
        chk(hip.hipMemcpy(host.ctypes.data_as(vp), src, C.c_size_t(host.nbytes), 2))
    ev = [vp(), vp()]
    for x in ev: chk(hip.hipEventCreate(C.byref(x)))
    L.zjni_build_stamp.restype = C.c_char_p
    stamp = L.zjni_build_stamp().decode()
    for level in [int(x) for x in a.levels.split(",")]:
        times = []
        cd = L.zjni_createCDict(dict_bytes, len(dict_bytes), level) if dict_bytes else None
        assert cd or not dict_bytes, level
        for it in range(a.warmup + a.steps):
            chk(hip.hipEventRecord(ev[0], None))
            if cd:
                chk(L.zjni_compress_batch_device_usingCDict(src, soff, comp, coff, csz, n, cd, 0, None))
            else:
                chk(L.zjni_compress_batch_device2(src, soff, comp, coff, csz, n, level, 0, None))
            chk(hip.hipEventRecord(ev[1], None)); chk(hip.hipDeviceSynchronize())
            ms = C.c_float(); chk(hip.hipEventElapsedTime(C.byref(ms), ev[0], ev[1]))
            if it >= a.warmup: times.append(ms.value)
        route = int(L.zjni_last_route())
        h_csz = np.zeros(n, dtype=np.uint64)
        chk(hip.hipMemcpy(h_csz.ctypes.data_as(vp), csz, C.c_size_t(n * 8), 2))
        ok_sizes = bool((h_csz < np.uint64(1 << 63)).all())
        identical = None
        ref = None if a.no_reference else port.cpu_baseline2(host, size, n, level, a.threads, a.cpu_seconds, dictionary=dict_bytes, keep_frames=True)
        if cd:
            L.zjni_freeCDict(cd)
        if ok_sizes and ref is not None:
            h_poff = np.zeros(n + 1, dtype=np.uint64); h_poff[1:] = np.cumsum(h_csz)
            chk(hip.hipMemcpy(poff, h_poff.ctypes.data_as(vp), C.c_size_t((n + 1) * 8), 1))
            chk(L.zjni_pack_batch_device(comp, coff, csz, packed, poff, n, None)); chk(hip.hipDeviceSynchronize())
            total = int(h_poff[-1])
            mine = np.empty(total, dtype=np.uint8)
            chk(hip.hipMemcpy(mine.ctypes.data_as(vp), packed, C.c_size_t(total), 2))
            identical = ref["frames"] is not None and bool(np.array_equal(ref["sizes"], h_csz)) and bool(np.array_equal(ref["frames"], mine))
        best, mean = min(times), sum(times) / len(times)
        gib = n * size / GIB
        print(json.dumps({"tool": "bench_fast_levels", "level": level, "n": n, "size": size, "build_stamp": stamp, "route": route,
                          "dictionary": None if not dict_bytes else {"bytes": len(dict_bytes), "kind": "bench.py config 4: trained from 10 000 class-1 records"},
                          "compress_ms_best": round(best, 3), "compress_ms_mean": round(mean, 3), "steps": a.steps, "warmup": a.warmup,
                          "compress_GiBps": round(gib / (best / 1e3), 2), "compress_GiBps_mean": round(gib / (mean / 1e3), 2),
                          "compressed_bytes": int(h_csz.sum()) if ok_sizes else None, "ratio": round(n * size / max(1, int(h_csz.sum())), 4) if ok_sizes else None,
                          "all_frames_byte_identical_to_reference": identical,
                          "reference_cpu": None if ref is None else {"threads": a.threads, "compress_GiBps": round(gib / ref["compress_s"], 2), "compressed_bytes": ref["compressed_bytes"],
                                            "passes": ref["passes"][0], "kind": "oracle.port.cpu_baseline2, best pass"}}), flush=True)
    for p in (src, comp, packed, soff, coff, csz, poff):
        hip.hipFree(p)


if __name__ == "__main__":
    main()
