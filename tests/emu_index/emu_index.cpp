// tests/emu_index/emu_index.cpp — lane-serial build of zj_index.h as the kernels of zjni_index_from_*_device and zjni_decompress_index_range_batch_device call it:
// every lane, wave or workgroup in turn over a batch in host memory, the scans between the kernels done here.  For tests/test_emu_index.py.
// TEST INFRASTRUCTURE ONLY: never linked into libzjni_amd.so.
#include "../../zstd-jni_amd/csrc/zj_index.h"
#include <stdlib.h>
#include <string.h>
#include <vector>

typedef unsigned long long ull;
extern "C" unsigned emu_index_rec_bytes(void) { return (unsigned)sizeof(ZRRec); }
extern "C" unsigned emu_index_req_bytes(void) { return (unsigned)sizeof(ZIReq); }
extern "C" unsigned emu_index_scan_wg(void) { return ZJ_INDEX_SCAN_WG; }
extern "C" unsigned emu_index_emit_wg(void) { return ZJ_INDEX_EMIT_WG; }
extern "C" ull emu_index_bytes(ull n, ull E) { return zj_index_bytes(n, E); }

// zj_index_scan_kernel, one workgroup: lane t sums its share, the shares are scanned, lane t writes its share's prefixes
static void scan_wg(const u64* in, u64 E, u64* out) {
    std::vector<u64> part(ZJ_INDEX_SCAN_WG);
    u64 const per = (E + ZJ_INDEX_SCAN_WG - 1u) / ZJ_INDEX_SCAN_WG;
    for (u32 t = 0; t < ZJ_INDEX_SCAN_WG; t++) {
        u64 const lo0 = (u64)t * per, lo = lo0 < E ? lo0 : E, hi = lo + per < E ? lo + per : E;
        u64 sum = 0;
        for (u64 i = lo; i < hi; i++) sum += zj_index_term(in[i]);
        part[t] = sum;
    }
    for (u32 t = 1; t < ZJ_INDEX_SCAN_WG; t++) part[t] += part[t - 1];
    for (u32 t = 0; t < ZJ_INDEX_SCAN_WG; t++) {
        u64 const lo0 = (u64)t * per, lo = lo0 < E ? lo0 : E, hi = lo + per < E ? lo + per : E;
        u64 run = t ? part[t - 1] : 0;
        for (u64 i = lo; i < hi; i++) { out[i] = run; run += zj_index_term(in[i]); }
    }
    out[E] = part[ZJ_INDEX_SCAN_WG - 1u];
}
// zj_index_buffers_kernel (a wave per buffer, lanes striding its entries) + zj_index_scan_kernel; result: NULL or the compress call's answers
extern "C" void emu_index_from_sizes(ull n, const ull* first, const ull* size, const ull* content, const ull* result, ull E, ull* idx) {
    u64* const valid = (u64*)idx + n + 1; u64* const C = (u64*)idx + 2 * n + 1; u64* const U = C + E + 1;
    for (u64 i = 0; i <= n; i++) idx[i] = first[i];
    for (u64 i = 0; i < n; i++) {
        bool all = true;
        for (u32 lane = 0; lane < 64; lane++) {
            bool ok = zj_index_first_ok((const u64*)first, i, E);
            for (u64 e = first[i] + lane; ok && e < first[i + 1]; e += 64) ok = size[e] <= ZJ_INDEX_SIZE_MAX && content[e] <= ZJ_INDEX_SIZE_MAX;
            all = all && ok;
        }
        valid[i] = zj_index_valid(all, (const u64*)result, i);
    }
    scan_wg((const u64*)size, E, C);
    scan_wg((const u64*)content, E, U);
}
// zj_index_content_kernel (a lane per entry), then the kernels above
extern "C" void emu_index_from_pieces(const ull* off, ull n, ull chunk, const ull* cut, const ull* cutOff, const ull* result, const ull* first, const ull* size, ull E, ull* idx) {
    std::vector<u64> content(E + 1);
    for (u64 e = 0; e < E; e++) {
        content[e] = 0;
        if (!n) continue;
        u64 const i = zj_entry_owner((const u64*)first, n, e), f0 = first[i];
        if (e < f0 || e >= first[i + 1]) continue;
        u64 const lo = off[i], hi = off[i + 1], sz = hi > lo ? hi - lo : 0;
        const u64* list = nullptr; u64 c = 0;
        if (cut) { u64 const c0 = cutOff[i], c1 = cutOff[i + 1]; c = c1 > c0 ? c1 - c0 : 0; list = (const u64*)cut + c0; }
        content[e] = zj_index_piece_content(sz, chunk, list, c, e - f0);
    }
    emu_index_from_sizes(n, first, size, (const ull*)content.data(), result, E, idx);
}
// zj_index_request_kernel + zj_range_scan_kernel with n := R: rec[R], ireq[R], bad[R], scan[5][R + 1], total[R]
extern "C" void emu_index_request(const ull* idx, ull n, ull E, const ull* off, const ull* req, const ull* dstOff, unsigned R, void* rec, void* ireq, unsigned* bad, ull* scan, ull* total) {
    u64 run[5] = {0, 0, 0, 0, 0};
    for (u32 i = 0; i < R; i++) {
        u64 const dlo = dstOff[i], dhi = dstOff[i + 1];
        u64 q[5];
        zj_index_request((const u64*)idx, n, E, (const u64*)off, req[3 * i], req[3 * i + 1], req[3 * i + 2], dhi > dlo ? dhi - dlo : 0, ((ZRRec*)rec)[i], ((ZIReq*)ireq)[i], q);
        bad[i] = 0;
        for (u32 k = 0; k < 5; k++) { scan[(u64)k * (R + 1) + i] = run[k]; run[k] += q[k]; }
        if (total) total[i] = ((ZRRec*)rec)[i].total;
    }
    for (u32 k = 0; k < 5; k++) scan[(u64)k * (R + 1) + R] = run[k];
}
// zj_index_check_kernel, zj_index_emit_kernel (a lane per entry of set A each), zj_index_edges_kernel (a lane per request)
extern "C" void emu_index_emit(const ull* idx, ull n, ull E, const void* recv, const void* ireqv, unsigned* bad, const ull* scan, const ull* dstOff, unsigned R,
                               ull* srcA, ull* dstA, ull* srcB, ull* dstB, ull* in3, ull* out3) {
    const ZRRec* const rec = (const ZRRec*)recv; const ZIReq* const ireq = (const ZIReq*)ireqv;
    u64 const n1 = (u64)R + 1u;
    const u64* const fA = (const u64*)scan; const u64* const fB = fA + n1; const u64* const cA = fA + 2 * n1; const u64* const cB = fA + 3 * n1; const u64* const eB = fA + 4 * n1;
    ZIView const v = zj_index_view((const u64*)idx, n, E);
    u64 const EA = fA[R];
    for (u64 g = 0; g < EA; g++) {
        u64 const r = zj_entry_owner(fA, R, g), j = g - fA[r], m = fA[r + 1] - fA[r] - 1u;
        if (j >= m || rec[r].status != ZJ_RANGE_SELECTED) continue;
        if (!zj_index_entry_ok(v.C, v.U, rec[r], ireq[r], j)) bad[r] = 1u;
    }
    for (u64 g = 0; g < EA; g++) {
        u64 const r = zj_entry_owner(fA, R, g);
        u64 s, d;
        zj_index_entry(v.C, v.U, rec[r], ireq[r], bad[r] != 0u, g - fA[r], cA[r], dstOff[r], &s, &d);
        srcA[g] = s; dstA[g] = d;
    }
    ZRCopy* const in = (ZRCopy*)in3; ZRCopy* const out = (ZRCopy*)out3;
    for (u32 i = 0; i < R; i++) {
        u64 const a1 = fA[i + 1], b0 = fB[i];
        ZRCopy cin[3], cout[2];
        u64 closeSrc, closeDst;
        zj_range_emit(nullptr, 0, rec[i], ireq[i].srcLo, dstOff[i], 0u, cA[i], cA[R] + cB[i], eB[i], &closeSrc, &closeDst, (u64*)srcB + b0, (u64*)dstB + b0, cin, cout);
        in[i] = cin[0]; in[(u64)R + 2 * i] = cin[1]; in[(u64)R + 2 * i + 1] = cin[2];
        out[2 * i] = cout[0]; out[2 * i + 1] = cout[1];
        if (i + 1 == R) { srcA[a1] = cA[R]; dstA[a1] = dstA[a1 - 1]; srcB[fB[R]] = cA[R] + cB[R]; dstB[fB[R]] = eB[R]; }
    }
}
// zj_index_finish_kernel, a wave per request done by one lane: result[R], the copy runs of a request with an error emptied, stat[4]
extern "C" void emu_index_finish(const ull* idx, ull n, ull E, const void* recv, const void* ireqv, const unsigned* bad, const ull* scan, const ull* resA, const ull* resB,
                                 ull* result, unsigned R, ull* out3, unsigned* stat) {
    const ZRRec* const rec = (const ZRRec*)recv; const ZIReq* const ireq = (const ZIReq*)ireqv;
    const u64* const U = zj_index_view((const u64*)idx, n, E).U;
    ZRCopy* const out = (ZRCopy*)out3;
    for (u32 i = 0; i < R; i++) {
        u32 const status = rec[i].status, e = rec[i].edges;
        if (status != ZJ_RANGE_SELECTED) { result[i] = status == ZJ_RANGE_NOTHING ? 0 : ZJ_ERR64(status); stat[status == ZJ_RANGE_NOTHING ? 0 : 3]++; continue; }
        u64 const a0 = scan[i], m = scan[i + 1] - a0 - 1u, b0 = scan[(u64)R + 1u + i], e0 = ireq[i].e0;
        u64 err = bad[i] ? ZJ_ERR64(ZJ_E_CORRUPTION) : 0;
        if (!err && (e & 1u)) err = zj_index_verdict(resB[b0], rec[i].fcsF);
        for (u64 k = 0; k < m && !err; k++) err = zj_index_verdict(resA[a0 + k], U[e0 + k + 1] - U[e0 + k]);
        if (!err && (e & 2u)) err = zj_index_verdict(resB[b0 + (e & 1u)], rec[i].fcsL);
        result[i] = err ? err : rec[i].hi - rec[i].lo;
        if (err) { out[2 * (u64)i].len = 0; out[2 * (u64)i + 1].len = 0; }
        stat[err ? 3 : 0]++; stat[1] += rec[i].frames; stat[2] += zj_range_edge_count(e);
    }
}
