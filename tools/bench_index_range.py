#!/usr/bin/env python3
"""Range reads by a caller-held index, measured beside what they replace, leg by leg in one process.

  a  tools/bench_range.py's shape: `--buffers` x `--buffer-bytes` of the benchmark's mixed-entropy data at chunk 64 KiB.  One request per buffer — `--range-bytes`
     from the middle, the last `--range-bytes`, the whole — through zjni_decompress_index_range_batch_device (X) beside zjni_decompress_frames_range_batch_device
     (W, the walked entry), and the index build (zjni_index_from_pieces_device) on its own.
  b  tools/bench_pieces.py's record store: config 4's 4 KiB JSON-like records and trained dictionary, 64 buffers cut at the records.  1 % of the records at random
     as requests of ONE indexed call (X) beside leg I (zjni_pack_batch_device + zjni_decompress_batch_device_usingDDict by the caller's own offsets) and leg R (the
     walked entry, one range per buffer and call); and as many ranges that straddle two records, which neither I nor one ranged call serves.
  c  the host form on one buffer of leg a: zjni_decompress_index_range beside zjni_decompress_frames_range (wall clock: both block), with the bytes each sends over
     the link.

A warm-up of each leg, then the legs alternating; device legs between two device events and a synchronise (the entries' host wait is inside the window).  Every
decoded byte is compared with the source in the run.  No torch: HBM through the HIP runtime, so the same command runs under `rocprofv3 --kernel-trace --stats`.

usage: bench_index_range.py [--legs a,b,c] [--buffers 64] [--buffer-bytes 67108864] [--range-bytes 1048576] [--records 1048576] [--steps 12] [--read-steps 3]
                            [--warmup 2] [--out file.json]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

SIZE = 4096


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="a,b,c")
    ap.add_argument("--buffers", type=int, default=64)
    ap.add_argument("--buffer-bytes", type=int, default=64 << 20)
    ap.add_argument("--chunk", type=int, default=65536)
    ap.add_argument("--range-bytes", type=int, default=1 << 20)
    ap.add_argument("--records", type=int, default=1 << 20)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--read-steps", type=int, default=3)
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

    stats4 = (C.c_uint * 4)()
    legs = a.legs.split(",")
    piece = 256 << 20

    # ------------------------------------------------------------------------------------------------ a (and c on one of its buffers)
    if "a" in legs or "c" in legs:
        n, size, chunk, part = a.buffers, a.buffer_bytes, a.chunk, a.range_bytes
        assert size % chunk == 0 and part + chunk < size // 2
        per = size // chunk
        E, total = n * per, n * size
        slot = L.zjni_compressBound_pieces(size, per)
        src, comp, packed = dmalloc(total), dmalloc(n * slot), dmalloc(n * slot)
        back, back_p = dmalloc(total), dmalloc(n * part)
        soff, coff, poff = upload(np.arange(n + 1, dtype=np.uint64) * size), upload(np.arange(n + 1, dtype=np.uint64) * slot), dmalloc((n + 1) * 8)
        part_off = upload(np.arange(n + 1, dtype=np.uint64) * part)
        res_c, res_r, tot_r, first, psize = dmalloc(n * 8), dmalloc(n * 8), dmalloc(n * 8), dmalloc((n + 1) * 8), dmalloc(E * 8)
        index = dmalloc(L.zjni_index_bytes(n, E))
        chk(L.zjni_synth_fill_device(src, chunk, 0, E, None))
        chk(L.zjni_compress_pieces_batch_device(src, soff, comp, coff, res_c, n, 3, 0, chunk, None, None, None, first, psize, E, None))
        chk(L.zjni_pack_batch_device2(comp, coff, res_c, packed, poff, n, None))
        chk(hip.hipDeviceSynchronize())
        h_poff, h_psize = download(poff, (n + 1) * 8, np.uint64), download(psize, E * 8, np.uint64)
        assert (download(first, (n + 1) * 8, np.uint64) == np.arange(n + 1, dtype=np.uint64) * per).all() and (h_psize < (1 << 32)).all()

        def build():
            chk(L.zjni_index_from_pieces_device(soff, n, chunk, None, None, res_c, first, psize, E, index, None))

        mid = size // 2 + chunk // 3
        shapes = {"middle": (mid, part), "tail": (size - part, part), "whole": (0, size)}
        ranges = {k: upload(np.array([lo, ln] * n, dtype=np.uint64)) for k, (lo, ln) in shapes.items()}
        reqs = {k: upload(np.array([[i, lo, ln] for i in range(n)], dtype=np.uint64)) for k, (lo, ln) in shapes.items()}

        def walked(name):
            whole = name == "whole"
            return lambda: chk(L.zjni_decompress_frames_range_batch_device(packed, poff, back if whole else back_p, soff if whole else part_off, ranges[name], res_r, tot_r, n, None, None))

        def indexed(name):
            whole = name == "whole"
            return lambda: chk(L.zjni_decompress_index_range_batch_device(packed, poff, n, index, E, reqs[name], back if whole else back_p, soff if whole else part_off,
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

    if "a" in legs:
        build()
        for _ in range(a.warmup):
            timed(build)
            for name in shapes:
                timed(walked(name))
                timed(indexed(name))
        tb, tw, tx, seen = [], {k: [] for k in shapes}, {k: [] for k in shapes}, {}
        for k in range(a.steps):
            tb.append(timed(build))
            for name in shapes:
                tw[name].append(timed(walked(name)))
                if k == a.steps - 1:
                    seen["W_" + name] = verify(name, L.zjni_last_frames_range)
                tx[name].append(timed(indexed(name)))
                if k == a.steps - 1:
                    seen["X_" + name] = verify(name, L.zjni_last_index_range)
        line = {"leg": "a", "buffers": n, "buffer_bytes": size, "chunk": chunk, "entries": E, "range_bytes": part, "frames_bytes": int(h_poff[-1]),
                "index_bytes": L.zjni_index_bytes(n, E), "index_build": stats(tb)}
        for name in shapes:
            w, x = stats(tw[name]), stats(tx[name])
            line["W_" + name], line["X_" + name] = w, x
            line["X_minus_W_ms_" + name] = round(x["median_ms"] - w["median_ms"], 3)
            line["X_not_slower_than_W_beyond_W_spread_" + name] = bool(x["median_ms"] <= w["median_ms"] + (w["max_ms"] - w["min_ms"]))
        line["diagnostics"] = seen
        line["outputs_compared"] = "results, totals and all decoded bytes of every leg against the source (the destination zeroed between the legs)"
        emit(line)

    # ------------------------------------------------------------------------------------------------ c
    if "c" in legs:
        comp_size = int(h_poff[1] - h_poff[0])
        data = download(packed, comp_size).tobytes()
        sizes = (C.c_uint64 * per)(*[int(x) for x in h_psize[:per]])
        contents = (C.c_uint64 * per)(*([chunk] * per))
        want_src = download(src, size)
        C_sum = np.concatenate([[0], np.cumsum(h_psize[:per])])
        line = {"leg": "c", "buffer_bytes": size, "frames_bytes": comp_size, "entries": per}
        for name, (lo, ln) in shapes.items():
            dst_w, dst_x = C.create_string_buffer(ln), C.create_string_buffer(ln)
            tot = C.c_ulonglong(0)
            tw, tx = [], []
            for k in range(a.read_steps + 1):
                t0 = time.perf_counter()
                r = L.zjni_decompress_frames_range(dst_w, ln, data, comp_size, lo, ln, C.byref(tot))
                t1 = time.perf_counter()
                assert r == ln and tot.value == size
                r = L.zjni_decompress_index_range(dst_x, ln, data, comp_size, lo, ln, sizes, contents, per, C.byref(tot), None)
                t2 = time.perf_counter()
                assert r == ln and tot.value == size
                if k:
                    tw.append((t1 - t0) * 1e3)
                    tx.append((t2 - t1) * 1e3)
            assert dst_w.raw == want_src[lo:lo + ln].tobytes() == dst_x.raw, name
            e_first, e_last = lo // chunk, (lo + ln - 1) // chunk
            sent = int(C_sum[e_last + 1] - C_sum[e_first])
            line[name] = {"W_host_walked": stats(tw), "X_host_indexed": stats(tx), "W_source_bytes_uploaded": comp_size, "X_source_bytes_uploaded": sent,
                          "X_index_bytes_uploaded": L.zjni_index_bytes(1, e_last - e_first + 1), "entries_selected": e_last - e_first + 1}
        line["uploaded_bytes_are"] = "the selected entries' sizes summed from the index, as the entry stages them; not a counter"
        line["outputs_compared"] = "both forms' bytes with the source"
        emit(line)

    # ------------------------------------------------------------------------------------------------ b
    if "b" in legs:
        from oracle import ref
        for p in ("src", "comp", "packed", "back", "back_p"):
            if p in locals():
                chk(hip.hipFree(locals()[p]))
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
        index = dmalloc(L.zjni_index_bytes(n, E))
        chk(L.zjni_compress_pieces_batch_device(src, soff, comp, coff, res, n, 0, 0, SIZE, cut, cut_off, cd, first, psize, E, None))
        chk(L.zjni_pack_batch_device2(comp, coff, res, packed, poff, n, None))
        chk(hip.hipFree(comp))

        def build():
            chk(L.zjni_index_from_pieces_device(soff, n, SIZE, cut, cut_off, res, first, psize, E, index, None))

        build()
        chk(hip.hipDeviceSynchronize())
        sizes = download(psize, E * 8, np.uint64)
        rng = np.random.default_rng(103)
        chosen = np.sort(rng.choice(E, size=max(E // 100, 1), replace=False))
        R = len(chosen)
        owner, within = chosen // per, chosen % per
        starts = np.concatenate([[0], np.cumsum(sizes)])[:-1].astype(np.uint64)
        sel_src_off, sel_sizes = upload(np.concatenate([starts[chosen], [0]]).astype(np.uint64)), upload(sizes[chosen])
        sel_off = upload(np.concatenate([[0], np.cumsum(sizes[chosen])]).astype(np.uint64))
        sel, out_i, out_off, res_i = dmalloc(int(sizes[chosen].sum())), dmalloc(R * SIZE), upload(np.arange(R + 1, dtype=np.uint64) * SIZE), dmalloc(R * 8)
        out_x, res_x = dmalloc(R * SIZE), dmalloc(R * 8)
        req = upload(np.stack([owner, within * SIZE, np.full(R, SIZE)], axis=1).astype(np.uint64))
        # ranges of one record's length that begin in the middle of a record: two records each, both edges
        strad = np.minimum(within, per - 2)
        req_s = upload(np.stack([owner, strad * SIZE + SIZE // 2, np.full(R, SIZE)], axis=1).astype(np.uint64))

        def call_i():
            chk(L.zjni_pack_batch_device(packed, sel_src_off, sel_sizes, sel, sel_off, R, None))
            chk(L.zjni_decompress_batch_device_usingDDict(sel, sel_off, out_i, out_off, res_i, R, dd, None))

        def call_x(which=req):
            return lambda: chk(L.zjni_decompress_index_range_batch_device(packed, poff, n, index, E, which, out_x, out_off, res_x, None, R, dd, None))

        rounds = int(np.bincount(owner, minlength=n).max())
        mine_of = [np.nonzero(owner == i)[0] for i in range(n)]
        range_sets = []
        for k in range(rounds):
            rg = np.zeros((n, 2), dtype=np.uint64)
            for i in range(n):
                if k < len(mine_of[i]):
                    rg[i] = (int(within[mine_of[i][k]]) * SIZE, SIZE)
            range_sets.append(upload(rg))
        out_r, out_r_off, res_r = dmalloc(rounds * n * SIZE), upload(np.arange(rounds * n + 1, dtype=np.uint64) * SIZE), dmalloc(rounds * n * 8)

        def call_r():
            for k in range(rounds):
                chk(L.zjni_decompress_frames_range_batch_device(packed, poff, out_r, vp(out_r_off.value + k * n * 8), range_sets[k], vp(res_r.value + k * n * 8), None, n, dd, None))

        timed(call_i)
        timed(call_x())
        timed(call_x(req_s))
        timed(build)
        ti, tx, ts, tb = [], [], [], []
        for _ in range(a.read_steps):
            ti.append(timed(call_i))
            tx.append(timed(call_x()))
            tb.append(timed(build))
        assert (download(res_i, R * 8, np.uint64) == SIZE).all() and (download(res_x, R * 8, np.uint64) == SIZE).all()
        chk(L.zjni_last_index_range(stats4))
        seen_x = {"served": stats4[0], "entries": stats4[1], "edges": stats4[2], "errors": stats4[3]}
        got_i, got_x = download(out_i, R * SIZE), download(out_x, R * SIZE)
        for j, e in enumerate(chosen):
            want = download(src, SIZE, at=int(e) * SIZE)
            assert (got_i[j * SIZE:(j + 1) * SIZE] == want).all() and (got_x[j * SIZE:(j + 1) * SIZE] == want).all(), "record %d differs" % e
        for _ in range(a.read_steps):
            ts.append(timed(call_x(req_s)))
        assert (download(res_x, R * 8, np.uint64) == SIZE).all()
        chk(L.zjni_last_index_range(stats4))
        seen_s = {"served": stats4[0], "entries": stats4[1], "edges": stats4[2], "errors": stats4[3]}
        got_s = download(out_x, R * SIZE)
        for j in range(R):
            at = (int(owner[j]) * per + int(strad[j])) * SIZE + SIZE // 2
            assert (got_s[j * SIZE:(j + 1) * SIZE] == download(src, SIZE, at=at)).all(), "straddling range %d differs" % j
        tr = [timed(call_r)]
        rr, got_r = download(res_r, rounds * n * 8, np.uint64), download(out_r, rounds * n * SIZE)
        for k in range(rounds):
            for i in range(n):
                hit = k < len(mine_of[i])
                assert int(rr[k * n + i]) == (SIZE if hit else 0)
                if hit:
                    j, at = mine_of[i][k], (k * n + i) * SIZE
                    assert (got_r[at:at + SIZE] == got_i[j * SIZE:(j + 1) * SIZE]).all(), "record %d differs (range)" % chosen[j]
        emit({"leg": "b", "buffers": n, "records": E, "record_bytes": SIZE, "level": 3, "frames_bytes": int(sizes.sum()), "records_read": R,
              "index_bytes": L.zjni_index_bytes(n, E), "index_build": stats(tb),
              "X_one_indexed_call": stats(tx), "X_calls": 1, "I_pack_and_plain_decompress": stats(ti), "R_walked_one_range_per_buffer": stats(tr), "R_calls": rounds,
              "X_straddling_two_records_one_call": stats(ts), "last_index_range_X": seen_x, "last_index_range_straddling": seen_s,
              "outputs_compared": "every record read by X, I and R, and every straddling range, with the source"})


if __name__ == "__main__":
    main()
