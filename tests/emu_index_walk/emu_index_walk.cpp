// tests/emu_index_walk/emu_index_walk.cpp — lane-serial build of the index walk (zj_index.h: zj_index_walk, zj_index_frames_emit) as the kernels of
// zjni_index_count_frames_device and zjni_index_from_frames_device call it: every lane in turn over a batch in host memory, the scans between the kernels done
// here; and the host form as zjni_index_from_frames runs it.  For tests/test_emu_index_walk.py.
// TEST INFRASTRUCTURE ONLY: never linked into libzjni_amd.so.
#include "../../zstd-jni_amd/csrc/zj_index.h"
#include <stdlib.h>
#include <string.h>
#include <vector>

typedef unsigned long long ull;

// zj_index_walk_count_kernel (a lane per buffer) + zj_pack_offsets_kernel: first[n + 1]
extern "C" void emu_walk_count(const unsigned char* src, const ull* off, ull n, ull* first) {
    u64 run = 0;
    for (u64 i = 0; i < n; i++) {
        u64 const lo = off[i], hi = off[i + 1];
        u64 entries, wrote;
        (void)zj_index_walk(src + lo, hi > lo ? hi - lo : 0, 0, nullptr, nullptr, &entries, &wrote);
        first[i] = run; run += entries;
    }
    first[n] = run;
}
// zjni_index_from_frames_device: first copied, the two arrays zeroed, zj_index_walk_emit_kernel (a lane per buffer), zj_index_scan_kernel (lane t sums its share).
// size / content: the caller's [E], or NULL (library scratch)
extern "C" void emu_walk_emit(const unsigned char* src, const ull* off, ull n, const ull* first, ull E, ull* idx, ull* size, ull* content) {
    std::vector<u64> scratchS(E + 1), scratchC(E + 1);
    u64* const sz = size ? (u64*)size : scratchS.data();
    u64* const ct = content ? (u64*)content : scratchC.data();
    u64* const valid = (u64*)idx + n + 1; u64* const C = (u64*)idx + 2 * n + 1; u64* const U = C + E + 1;
    for (u64 i = 0; i <= n; i++) idx[i] = first[i];
    for (u64 e = 0; e < E; e++) sz[e] = ct[e] = 0;
    for (u64 i = 0; i < n; i++) {
        u64 const lo = off[i], hi = off[i + 1];
        valid[i] = zj_index_frames_emit(src + lo, hi > lo ? hi - lo : 0, (const u64*)first, i, E, sz, ct);
    }
    for (u32 w = 0; w < 2; w++) {
        const u64* const in = w ? ct : sz; u64* const out = w ? U : C;
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
}
// zjni_index_from_frames, statement for statement (the library's own is checked against this one where the library is loaded)
extern "C" ull emu_walk_host(const unsigned char* src, ull srcSize, ull* pieceSize, ull* pieceContent, ull capacity, ull* nPieces) {
    *nPieces = 0;
    u64 entries = 0, wrote = 0;
    u32 const verdict = zj_index_walk(src, srcSize, capacity, (u64*)pieceSize, (u64*)pieceContent, &entries, &wrote);
    if (verdict) return ZJ_ERR64(verdict);
    *nPieces = entries;
    return entries > capacity ? ZJ_ERR64(ZJ_E_DSTSIZE_TOO_SMALL) : 0;
}
