#!/usr/bin/env python3
"""A record store measured: BASELINE config 4's data (4 KiB JSON-like records, its trained 110 KiB dictionary) held as a few large buffers, cut at the records.

  P   zjni_compress_pieces_batch_device            n buffers, cuts at the record boundaries, the dictionary, the frame sizes out
  c0  zjni_compress_batch_device_usingCDict        the same records as E separate buffers                          (the ceiling of P: the layer's own cost is P - c0)
  I   zjni_pack_batch_device + zjni_decompress_batch_device_usingDDict
                                                   1 % of the records, chosen at random, found by P's index alone: gathered, then decoded as a plain batch
  R   zjni_decompress_frames_range_batch_device    the same records, one range per buffer and call: as many calls as the fullest buffer has chosen records

All in one process, after a warm-up of each, every leg between two device events and a synchronise (the host waits of P and R are inside the window); P and c0
alternate, I and R alternate.  The outputs are compared: P's packed frames with c0's byte for byte and P's index with c0's sizes; every record I and R decode with
the source.  No torch: HBM through the HIP runtime, so the same command runs under `rocprofv3 --kernel-trace --stats`.  The scratch of P is
zjni_compressBound(chunk) per piece and a call is cut into slices of at most 65 536 pieces: the line reports the slice count beside the number.

usage: bench_pieces.py [--buffers 64] [--records 1048576] [--levels 1,3] [--steps 8] [--read-steps 3] [--warmup 2] [--out file.json]"""
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
    ap.add_argument("--buffers", type=int, default=64)
    ap.add_argument("--records", type=int, default=1 << 20)
    ap.add_argument("--levels", default="1,3")
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--read-steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out")
    a = ap.parse_args()
    zj = entry.load_package()
    L = zj.lib()
    from oracle import ref
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
    n, E = a.buffers, a.records
    assert E % n == 0
    per = E // n
    size = per * SIZE
    total = E * SIZE
    # config 4's data: class 1 of the generator (every fourth buffer), and its dictionary
    src, soff_e = dmalloc(total), upload(np.arange(E + 1, dtype=np.uint64) * SIZE)
    part = min(E, 1 << 18)
    big, pick_sizes = dmalloc(4 * part * SIZE), upload(np.full(part, SIZE, dtype=np.uint64))
    for at in range(0, E, part):
        m = min(part, E - at)
        chk(L.zjni_synth_fill_device(big, SIZE, 4 * at, 4 * m, None))
        pick = upload((np.arange(m + 1, dtype=np.uint64) * 4 + 1) * SIZE)
        chk(L.zjni_pack_batch_device(big, pick, pick_sizes, src, vp(soff_e.value + at * 8), m, None))
        chk(hip.hipDeviceSynchronize())
        chk(hip.hipFree(pick))
    chk(hip.hipFree(big))
    train = zj.synth_host(SIZE, 1 << 24, 40000)
    dic = ref.train_dict([train[i * SIZE:(i + 1) * SIZE] for i in range(1, 40000, 4)], 112640)
    dd = L.zjni_createDDict(dic, len(dic))
    assert dd

    slot, bound = L.zjni_compressBound_pieces(size, per), L.zjni_compressBound(SIZE)
    soff, coff = upload(np.arange(n + 1, dtype=np.uint64) * size), upload(np.arange(n + 1, dtype=np.uint64) * slot)
    coff_e = upload(np.arange(E + 1, dtype=np.uint64) * bound)
    cut = upload(np.tile(np.arange(1, per, dtype=np.uint64) * SIZE, n))
    cut_off = upload(np.arange(n + 1, dtype=np.uint64) * (per - 1))
    comp, comp0, packed, packed0 = dmalloc(n * slot), dmalloc(E * bound), dmalloc(n * slot), dmalloc(E * bound)
    res, res0, poff, poff_e = dmalloc(n * 8), dmalloc(E * 8), dmalloc((n + 1) * 8), dmalloc((E + 1) * 8)
    first, psize = dmalloc((n + 1) * 8), dmalloc(E * 8)
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

    gib = total / (1 << 30)

    def stats(ts, of_gib=None):
        q = statistics.quantiles(ts, n=4) if len(ts) >= 2 else [ts[0]] * 3
        med = statistics.median(ts)
        out = {"median_ms": round(med, 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3), "iqr_ms": round(q[2] - q[0], 3), "calls": len(ts)}
        if of_gib:
            out["GiBps_of_source_at_median"] = round(of_gib / (med / 1e3), 2)
        return out

    for level in [int(x) for x in a.levels.split(",")]:
        cd = L.zjni_createCDict(dic, len(dic), level)
        assert cd

        def call_p():
            chk(L.zjni_compress_pieces_batch_device(src, soff, comp, coff, res, n, 0, 0, SIZE, cut, cut_off, cd, first, psize, E, None))

        def call_c0():
            chk(L.zjni_compress_batch_device_usingCDict(src, soff_e, comp0, coff_e, res0, E, cd, 0, None))

        for _ in range(a.warmup):
            timed(call_c0)
            timed(call_p)
        tp, tc0 = [], []
        for _ in range(a.steps):
            tc0.append(timed(call_c0))
            tp.append(timed(call_p))
        chk(L.zjni_pack_batch_device2(comp0, coff_e, res0, packed0, poff_e, E, None))
        chk(L.zjni_pack_batch_device2(comp, coff, res, packed, poff, n, None))
        chk(hip.hipDeviceSynchronize())
        sizes0, sizes = download(res0, E * 8, np.uint64), download(psize, E * 8, np.uint64)
        h_first, h_poff = download(first, (n + 1) * 8, np.uint64), download(poff, (n + 1) * 8, np.uint64)
        frames_bytes = int(sizes0.sum())
        assert (sizes0 < (1 << 40)).all() and (sizes == sizes0).all(), "the index differs from the separate frames' sizes"
        assert (h_first == np.arange(n + 1, dtype=np.uint64) * per).all() and int(h_poff[-1]) == frames_bytes
        piece = 256 << 20
        for at in range(0, frames_bytes, piece):
            m = min(piece, frames_bytes - at)
            assert (download(packed, m, at=at) == download(packed0, m, at=at)).all(), "the frames differ from the separate frames at %d" % at

        # ---- record reads: 1 % of the records, by the index (I) and by ranges (R)
        rng = np.random.default_rng(level + 100)
        chosen = np.sort(rng.choice(E, size=max(E // 100, 1), replace=False))
        R = len(chosen)
        starts = np.concatenate([[0], np.cumsum(sizes)])[:-1].astype(np.uint64)          # (packed: frame e begins where the frames before it end)
        sel_src_off, sel_sizes = upload(np.concatenate([starts[chosen], [0]]).astype(np.uint64)), upload(sizes[chosen])
        sel_off = upload(np.concatenate([[0], np.cumsum(sizes[chosen])]).astype(np.uint64))
        sel, out_i, out_off, res_i = dmalloc(int(sizes[chosen].sum())), dmalloc(R * SIZE), upload(np.arange(R + 1, dtype=np.uint64) * SIZE), dmalloc(R * 8)

        def call_i():
            chk(L.zjni_pack_batch_device(packed, sel_src_off, sel_sizes, sel, sel_off, R, None))
            chk(L.zjni_decompress_batch_device_usingDDict(sel, sel_off, out_i, out_off, res_i, R, dd, None))

        owner, within = chosen // per, chosen % per
        rounds = int(np.bincount(owner, minlength=n).max())
        range_sets, slots = [], []
        mine_of = [np.nonzero(owner == i)[0] for i in range(n)]
        for k in range(rounds):                                                             # round k: the k-th chosen record of every buffer that has one (others: an empty range)
            rg = np.zeros((n, 2), dtype=np.uint64)
            where = np.full(n, -1, dtype=np.int64)
            for i in range(n):
                mine = mine_of[i]
                if k < len(mine):
                    rg[i] = (int(within[mine[k]]) * SIZE, SIZE)
                    where[i] = mine[k]
            range_sets.append(upload(rg))
            slots.append(where)
        out_r, out_r_off, res_r = dmalloc(rounds * n * SIZE), upload(np.arange(rounds * n + 1, dtype=np.uint64) * SIZE), dmalloc(rounds * n * 8)
        edges = (C.c_uint * 4)()

        def call_r():
            for k in range(rounds):
                chk(L.zjni_decompress_frames_range_batch_device(packed, poff, out_r, vp(out_r_off.value + k * n * 8), range_sets[k], vp(res_r.value + k * n * 8), None, n, dd, None))

        for _ in range(min(a.warmup, 1)):
            timed(call_i)
            timed(call_r)
        chk(L.zjni_last_frames_range(edges))
        ti, tr = [], []
        for _ in range(a.read_steps):
            ti.append(timed(call_i))
            tr.append(timed(call_r))
        assert (download(res_i, R * 8, np.uint64) == SIZE).all(), "a record did not decode by the index"
        got_i, got_r, rr = download(out_i, R * SIZE), download(out_r, rounds * n * SIZE), download(res_r, rounds * n * 8, np.uint64)
        for j, e in enumerate(chosen):
            assert (got_i[j * SIZE:(j + 1) * SIZE] == download(src, SIZE, at=int(e) * SIZE)).all(), "record %d differs (index)" % e
        for k in range(rounds):
            for i in range(n):
                j = slots[k][i]
                at = (k * n + i) * SIZE
                assert int(rr[k * n + i]) == (SIZE if j >= 0 else 0)
                assert j < 0 or (got_r[at:at + SIZE] == got_i[j * SIZE:(j + 1) * SIZE]).all(), "record %d differs (range)" % chosen[j]
        si, sr = stats(ti), stats(tr)
        sp, sc0 = stats(tp, gib), stats(tc0, gib)
        line = {"buffers": n, "records": E, "record_bytes": SIZE, "level": level, "source_GiB": round(gib, 3), "frames_bytes": frames_bytes, "ratio": round(total / frames_bytes, 3),
                "P_compress_pieces": sp, "c0_compress_usingCDict_separate_buffers": sc0, "P_over_c0": round(sp["median_ms"] / sc0["median_ms"], 3),
                "slices_of_P": -(-E // 65536), "scratch_per_piece": bound,
                "records_read": R, "I_index_gather_and_plain_decompress": si, "R_ranged_one_range_per_buffer": sr, "R_calls": rounds, "R_over_I": round(sr["median_ms"] / si["median_ms"], 1),
                "last_frames_range_of_one_R_call": {"served": edges[0], "frames": edges[1], "edges": edges[2], "errors": edges[3]},
                "outputs_compared": "P's packed frames with c0's byte for byte, P's index with c0's sizes; every record read by I and by R with the source",
                "build_stamp": zj.build_stamp()}
        print(json.dumps(line), flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(json.dumps(line) + "\n")
        for p in (sel_src_off, sel_sizes, sel_off, sel, out_i, out_off, res_i, out_r, out_r_off, res_r, *range_sets):
            chk(hip.hipFree(p))
        L.zjni_freeCDict(cd)


if __name__ == "__main__":
    main()
