#!/usr/bin/env python3
"""The range-read index built from the frames alone (zjni_index_count_frames_device + zjni_index_from_frames_device), measured on the two stores of
tools/bench_index_range.py, leg by leg in one process.

  a  `--buffers` x `--buffer-bytes` of the benchmark's mixed-entropy data at chunk 64 KiB.  B: both passes of the build together, the read of E between them
     included.  W0: zjni_decompress_frames_range_batch_device with an empty range at the end of every buffer — the ranged entry's counting walk, its scans, its
     one wait and an emit and finish with nothing selected — the walk the build does twice.  Then the reads of bench_index_range's leg a, one request per
     buffer: W (the walked entry), X (the index zjni_index_from_pieces_device built) and F (the same call over the walk-built index), alternating.
  b  the record store: config 4's 4 KiB JSON-like records and trained dictionary, 64 buffers cut at the records.  B and W0 as above; 1 % of the records at random
     as requests of one indexed call over the pieces-built index (X) and the walk-built one (F), back to back, in either order in turn.

The walk-built index is compared with the pieces-built one word for word before anything is timed.  A warm-up of each leg, then the legs alternating; every call
between two device events and a synchronise.  Every decoded byte is compared with the source in the run.  No torch: HBM through the HIP runtime.

usage: bench_index_walk.py [--legs a,b] [--buffers 64] [--buffer-bytes 67108864] [--range-bytes 1048576] [--records 1048576] [--steps 12] [--read-steps 4]
                           [--warmup 2] [--out file.json]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

SIZE = 4096


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="a,b")
    ap.add_argument("--buffers", type=int, default=64)
    ap.add_argument("--buffer-bytes", type=int, default=64 << 20)
    ap.add_argument("--chunk", type=int, default=65536)
    ap.add_argument("--range-bytes", type=int, default=1 << 20)
    ap.add_argument("--records", type=int, default=1 << 20)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--read-steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out")
    a = ap.parse_args()
    zj = entry.load_package()
    L = zj.lib()
    hip = C.CDLL("libamdhip64.so")
    vp = C.c_void_p

    def chk(r):
        assert r == 0, r

    def dmalloc(nbytes):
        p = vp()
        chk(hip.hipMalloc(C.byref(p), C.c_size_t(max(nbytes, 8))))
        return p

    def upload(arr):
        arr = np.ascontiguousarray(arr)
        p = dmalloc(arr.nbytes)
        chk(hip.hipMemcpy(p, arr.ctypes.data_as(vp), C.c_size_t(arr.nbytes), 1))
        return p

    def download(p, nbytes, dtype=np.uint8, at=0):
        out = np.empty(nbytes // np.dtype(dtype).itemsize, dtype=dtype)
        chk(hip.hipMemcpy(out.ctypes.data_as(vp), vp(p.value + at), C.c_size_t(nbytes), 2))
        return out

    assert L.zjni_init(0) == 0, "needs a GPU"
    ev = [vp(), vp()]
    for e in ev:
        chk(hip.hipEventCreate(C.byref(e)))

    def timed(call):
        chk(hip.hipEventRecord(ev[0], None))
        call()
        chk(hip.hipEventRecord(ev[1], None))
        chk(hip.hipDeviceSynchronize())
        ms = C.c_float()
        chk(hip.hipEventElapsedTime(C.byref(ms), ev[0], ev[1]))
        return ms.value

    def stats(ts):
        q = statistics.quantiles(ts, n=4) if len(ts) >= 2 else [ts[0]] * 3
        return {"median_ms": round(statistics.median(ts), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3), "iqr_ms": round(q[2] - q[0], 3), "calls": len(ts)}

    def emit(line):
        line["build_stamp"] = zj.build_stamp()
        print(json.dumps(line), flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(json.dumps(line) + "\n")

    def walk_builder(packed, poff, n, E, first_w, index_w):
        """both passes and the eight bytes between them, as a caller runs them"""
        e_host = np.zeros(1, dtype=np.uint64)

        def build():
            chk(L.zjni_index_count_frames_device(packed, poff, n, first_w, None))
            chk(hip.hipMemcpy(e_host.ctypes.data_as(vp), vp(first_w.value + n * 8), C.c_size_t(8), 2))
            assert int(e_host[0]) == E, (int(e_host[0]), E)
            chk(L.zjni_index_from_frames_device(packed, poff, n, first_w, E, index_w, None, None, None))
        return build

    stats4 = (C.c_uint * 4)()
    legs = a.legs.split(",")
    piece = 256 << 20

    # ------------------------------------------------------------------------------------------------ a
    if "a" in legs:
        n, size, chunk, part = a.buffers, a.buffer_bytes, a.chunk, a.range_bytes
        assert size % chunk == 0 and part + chunk < size // 2
        per = size // chunk
        E, total = n * per, n * size
        slot = L.zjni_compressBound_pieces(size, per)
        src, comp, packed = dmalloc(total), dmalloc(n * slot), dmalloc(n * slot)
        back, back_p = dmalloc(total), dmalloc(n * part)
        soff, coff, poff = upload(np.arange(n + 1, dtype=np.uint64) * size), upload(np.arange(n + 1, dtype=np.uint64) * slot), dmalloc((n + 1) * 8)
        part_off, zero_off = upload(np.arange(n + 1, dtype=np.uint64) * part), upload(np.zeros(n + 1, dtype=np.uint64))
        res_c, res_r, tot_r, first, psize = dmalloc(n * 8), dmalloc(n * 8), dmalloc(n * 8), dmalloc((n + 1) * 8), dmalloc(E * 8)
        words = L.zjni_index_bytes(n, E)
        index, index_w, first_w = dmalloc(words), dmalloc(words), dmalloc((n + 1) * 8)
        chk(L.zjni_synth_fill_device(src, chunk, 0, E, None))
        chk(L.zjni_compress_pieces_batch_device(src, soff, comp, coff, res_c, n, 3, 0, chunk, None, None, None, first, psize, E, None))
        chk(L.zjni_pack_batch_device2(comp, coff, res_c, packed, poff, n, None))
        chk(L.zjni_index_from_pieces_device(soff, n, chunk, None, None, res_c, first, psize, E, index, None))
        chk(hip.hipDeviceSynchronize())
        h_poff = download(poff, (n + 1) * 8, np.uint64)
        build = walk_builder(packed, poff, n, E, first_w, index_w)
        build()
        chk(hip.hipDeviceSynchronize())
        used = (2 * n + 1 + 2 * (E + 1)) * 8
        assert (download(index_w, used, np.uint64) == download(index, used, np.uint64)).all(), "the walk-built index differs from the pieces-built one"

        mid = size // 2 + chunk // 3
        shapes = {"middle": (mid, part), "tail": (size - part, part), "whole": (0, size)}
        ranges = {k: upload(np.array([lo, ln] * n, dtype=np.uint64)) for k, (lo, ln) in shapes.items()}
        reqs = {k: upload(np.array([[i, lo, ln] for i in range(n)], dtype=np.uint64)) for k, (lo, ln) in shapes.items()}
        empty = upload(np.array([size, 0] * n, dtype=np.uint64))

        def walked_empty():
            chk(L.zjni_decompress_frames_range_batch_device(packed, poff, back_p, zero_off, empty, res_r, tot_r, n, None, None))

        def walked(name):
            whole = name == "whole"
            return lambda: chk(L.zjni_decompress_frames_range_batch_device(packed, poff, back if whole else back_p, soff if whole else part_off, ranges[name], res_r, tot_r, n, None, None))

        def indexed(name, idx):
            whole = name == "whole"
            return lambda: chk(L.zjni_decompress_index_range_batch_device(packed, poff, n, idx, E, reqs[name], back if whole else back_p, soff if whole else part_off,
                                                                          res_r, tot_r, n, None, None))

        def verify(name, last):
            lo, ln = shapes[name]
            assert (download(res_r, n * 8, np.uint64) == ln).all() and (download(tot_r, n * 8, np.uint64) == size).all(), name
            chk(last(stats4))
            if name == "whole":
                for at in range(0, total, piece):
                    m = min(piece, total - at)
                    assert (download(back, m, at=at) == download(src, m, at=at)).all(), "decoded bytes (%s) differ at %d" % (name, at)
                chk(hip.hipMemset(back, 0, C.c_size_t(total)))
            else:
                got = download(back_p, n * part)
                for i in range(n):
                    assert (got[i * part:(i + 1) * part] == download(src, part, at=i * size + lo)).all(), "decoded bytes (%s) differ in buffer %d" % (name, i)
                chk(hip.hipMemset(back_p, 0, C.c_size_t(n * part)))
            return {"served": stats4[0], "entries": stats4[1], "edges": stats4[2], "errors": stats4[3]}

        for _ in range(a.warmup):
            timed(build)
            timed(walked_empty)
            for name in shapes:
                timed(walked(name))
                timed(indexed(name, index))
                timed(indexed(name, index_w))
        tb, t0 = [], []
        tw, tx, tf, seen = {k: [] for k in shapes}, {k: [] for k in shapes}, {k: [] for k in shapes}, {}
        for k in range(a.steps):
            tb.append(timed(build))
            t0.append(timed(walked_empty))
            for name in shapes:
                last = k == a.steps - 1
                tw[name].append(timed(walked(name)))
                if last:
                    seen["W_" + name] = verify(name, L.zjni_last_frames_range)
                tx[name].append(timed(indexed(name, index)))
                if last:
                    seen["X_" + name] = verify(name, L.zjni_last_index_range)
                tf[name].append(timed(indexed(name, index_w)))
                if last:
                    seen["F_" + name] = verify(name, L.zjni_last_index_range)
        b, w0 = stats(tb), stats(t0)
        line = {"leg": "a", "buffers": n, "buffer_bytes": size, "chunk": chunk, "entries": E, "range_bytes": part, "frames_bytes": int(h_poff[-1]),
                "index_bytes": words, "B_walk_build_both_passes": b, "W0_walked_entry_empty_range": w0, "B_over_W0": round(b["median_ms"] / w0["median_ms"], 2),
                "walk_built_index_equals_pieces_built": True}
        for name in shapes:
            w, x, f = stats(tw[name]), stats(tx[name]), stats(tf[name])
            line["W_" + name], line["X_" + name], line["F_" + name] = w, x, f
            line["F_over_X_" + name] = round(f["median_ms"] / x["median_ms"], 3)
        saved = line["W_middle"]["median_ms"] - line["F_middle"]["median_ms"]
        line["small_reads_until_the_build_is_paid"] = round(b["median_ms"] / saved, 2) if saved > 0 else None
        line["diagnostics"] = seen
        line["outputs_compared"] = "results, totals and all decoded bytes of every leg against the source (the destination zeroed between the legs)"
        emit(line)
        for p in (src, comp, packed, back, back_p, index, index_w):
            chk(hip.hipFree(p))

    # ------------------------------------------------------------------------------------------------ b
    if "b" in legs:
        from oracle import ref
        n, E = a.buffers, a.records
        assert E % n == 0
        per = E // n
        size, total = per * SIZE, E * SIZE
        src, soff_e = dmalloc(total), upload(np.arange(E + 1, dtype=np.uint64) * SIZE)
        part = min(E, 1 << 18)
        big, pick_sizes = dmalloc(4 * part * SIZE), upload(np.full(part, SIZE, dtype=np.uint64))
        for at in range(0, E, part):                                  # config 4's data: class 1 of the generator (every fourth buffer), as tools/bench_pieces.py lays it out
            m = min(part, E - at)
            chk(L.zjni_synth_fill_device(big, SIZE, 4 * at, 4 * m, None))
            pick = upload((np.arange(m + 1, dtype=np.uint64) * 4 + 1) * SIZE)
            chk(L.zjni_pack_batch_device(big, pick, pick_sizes, src, vp(soff_e.value + at * 8), m, None))
            chk(hip.hipDeviceSynchronize())
            chk(hip.hipFree(pick))
        chk(hip.hipFree(big))
        train = zj.synth_host(SIZE, 1 << 24, 40000)
        dic = ref.train_dict([train[i * SIZE:(i + 1) * SIZE] for i in range(1, 40000, 4)], 112640)
        dd, cd = L.zjni_createDDict(dic, len(dic)), L.zjni_createCDict(dic, len(dic), 3)
        assert dd and cd
        slot = L.zjni_compressBound_pieces(size, per)
        soff, coff = upload(np.arange(n + 1, dtype=np.uint64) * size), upload(np.arange(n + 1, dtype=np.uint64) * slot)
        cut = upload(np.tile(np.arange(1, per, dtype=np.uint64) * SIZE, n))
        cut_off = upload(np.arange(n + 1, dtype=np.uint64) * (per - 1))
        comp, packed = dmalloc(n * slot), dmalloc(n * slot)
        res, poff, first, psize = dmalloc(n * 8), dmalloc((n + 1) * 8), dmalloc((n + 1) * 8), dmalloc(E * 8)
        words = L.zjni_index_bytes(n, E)
        index, index_w, first_w = dmalloc(words), dmalloc(words), dmalloc((n + 1) * 8)
        chk(L.zjni_compress_pieces_batch_device(src, soff, comp, coff, res, n, 0, 0, SIZE, cut, cut_off, cd, first, psize, E, None))
        chk(L.zjni_pack_batch_device2(comp, coff, res, packed, poff, n, None))
        chk(hip.hipFree(comp))
        chk(L.zjni_index_from_pieces_device(soff, n, SIZE, cut, cut_off, res, first, psize, E, index, None))
        build = walk_builder(packed, poff, n, E, first_w, index_w)
        build()
        chk(hip.hipDeviceSynchronize())
        used = (2 * n + 1 + 2 * (E + 1)) * 8
        assert (download(index_w, used, np.uint64) == download(index, used, np.uint64)).all(), "the walk-built index differs from the pieces-built one"
        sizes = download(psize, E * 8, np.uint64)
        rng = np.random.default_rng(103)
        chosen = np.sort(rng.choice(E, size=max(E // 100, 1), replace=False))
        R = len(chosen)
        owner, within = chosen // per, chosen % per
        out_x, out_off, res_x = dmalloc(R * SIZE), upload(np.arange(R + 1, dtype=np.uint64) * SIZE), dmalloc(R * 8)
        req = upload(np.stack([owner, within * SIZE, np.full(R, SIZE)], axis=1).astype(np.uint64))
        empty, zero_off, res_r = upload(np.array([size, 0] * n, dtype=np.uint64)), upload(np.zeros(n + 1, dtype=np.uint64)), dmalloc(n * 8)

        def walked_empty():
            chk(L.zjni_decompress_frames_range_batch_device(packed, poff, out_x, zero_off, empty, res_r, None, n, dd, None))

        def call(idx):
            return lambda: chk(L.zjni_decompress_index_range_batch_device(packed, poff, n, idx, E, req, out_x, out_off, res_x, None, R, dd, None))

        def verify():
            assert (download(res_x, R * 8, np.uint64) == SIZE).all()
            chk(L.zjni_last_index_range(stats4))
            got = download(out_x, R * SIZE)
            for j, e in enumerate(chosen):
                assert (got[j * SIZE:(j + 1) * SIZE] == download(src, SIZE, at=int(e) * SIZE)).all(), "record %d differs" % e
            chk(hip.hipMemset(out_x, 0, C.c_size_t(R * SIZE)))
            return {"served": stats4[0], "entries": stats4[1], "edges": stats4[2], "errors": stats4[3]}

        timed(build); timed(walked_empty); timed(call(index)); timed(call(index_w))
        tb, t0, tx, tf = [], [], [], []
        for k in range(a.read_steps):                                 # X and F back to back, in either order in turn; nothing but the calls between them
            tb.append(timed(build))
            t0.append(timed(walked_empty))
            for idx in ((index, index_w) if k % 2 == 0 else (index_w, index)):
                (tx if idx is index else tf).append(timed(call(idx)))
        timed(call(index))
        seen_x = verify()
        timed(call(index_w))
        seen_f = verify()
        assert (download(res_r, n * 8, np.uint64) == 0).all()
        b, w0, x, f = stats(tb), stats(t0), stats(tx), stats(tf)
        emit({"leg": "b", "buffers": n, "records": E, "record_bytes": SIZE, "level": 3, "frames_bytes": int(sizes.sum()), "records_read": R, "index_bytes": words,
              "B_walk_build_both_passes": b, "W0_walked_entry_empty_range": w0, "B_over_W0": round(b["median_ms"] / w0["median_ms"], 2),
              "walk_built_index_equals_pieces_built": True, "X_one_indexed_call": x, "F_one_indexed_call_walk_built_index": f, "F_over_X": round(f["median_ms"] / x["median_ms"], 3),
              "last_index_range_X": seen_x, "last_index_range_F": seen_f, "outputs_compared": "every record read by X and F with the source"})


if __name__ == "__main__":
    main()
