// tests/emu_pieces/emu_pieces.cpp — lane-serial build of zj_frames.h's piece arithmetic as the kernels of zjni_compress_pieces_batch_device call it: every wave's lanes
// in turn (the wave-wide AND of the count kernel becomes an AND over 64 lane results), every entry's lane in turn, the prefix sums between them done here.
// For tests/test_emu_pieces.py.  TEST INFRASTRUCTURE ONLY: never linked into libzjni_amd.so.
#include "../../zstd-jni_amd/csrc/zj_frames.h"
#include <stdlib.h>

typedef unsigned long long ull;

// zj_pieces_count_kernel + its two scans: first[0 .. n] over the entries walked, ifirst[0 .. n] over the entries of the caller's index, ferr[0 .. n); returns E (= first[n])
extern "C" ull emu_pieces_count(const ull* off, unsigned n, ull chunk, const ull* cut, const ull* cutOff, ull* first, ull* ifirst, ull* ferr) {
    u64 e = 0, x = 0;
    for (u32 i = 0; i < n; i++) {
        u64 const lo = off[i], hi = off[i + 1], size = hi > lo ? hi - lo : 0;
        bool all = true; u64 pieces = zj_chunk_count(size, chunk);
        if (cut) {
            u64 const c0 = cutOff[i], c1 = cutOff[i + 1], c = c1 > c0 ? c1 - c0 : 0;
            bool const head = c1 >= c0 && (c || zj_cut_none_ok(size, chunk));
            for (u32 lane = 0; lane < 64; lane++) {
                bool ok = head;
                for (u64 k = lane; ok && k < c; k += 64) ok = zj_cut_ok((const u64*)cut + c0, c, k, size, chunk);
                all = all && ok;
            }
            pieces = c + 1;
        }
        first[i] = e; ifirst[i] = x;
        e += zj_pieces_walked(all, pieces, size, chunk); x += all ? pieces : 0; ferr[i] = all ? 0 : (u64)0 - 42;
    }
    first[n] = e; ifirst[n] = x;
    return e;
}
// zj_pieces_emit_kernel for the slice [a, a + m], its end included: srcOffS[0 .. m], dstOffS[0 .. m]
extern "C" void emu_pieces_emit(const ull* off, const ull* first, const ull* ifirst, unsigned n, ull chunk, const ull* cut, const ull* cutOff,
                                ull a, unsigned m, ull E, ull* srcOffS, ull* dstOffS) {
    u64 const bound = zj_compress_bound(chunk);
    for (u64 j = 0; j <= m; j++) {
        dstOffS[j] = j * bound;
        u64 const e = a + j;
        if (e >= E) { srcOffS[j] = off[n]; continue; }
        u64 const i = zj_entry_owner((const u64*)first, n, e);
        bool const legal = ifirst[i + 1] > ifirst[i];
        srcOffS[j] = zj_piece_src(off[i], chunk, (cut && legal) ? (const u64*)cut + cutOff[i] : nullptr, e - first[i]);
    }
}
// zj_pieces_sizes_kernel for the slice [a, a + m): where entry a + j lies in the caller's index, ~0 for an entry of a buffer with an illegal list
extern "C" void emu_pieces_index(const ull* first, const ull* ifirst, unsigned n, ull a, unsigned m, ull* at) {
    for (u64 j = 0; j < m; j++) {
        u64 const e = a + j, i = zj_entry_owner((const u64*)first, n, e);
        at[j] = ifirst[i + 1] > ifirst[i] ? ifirst[i] + (e - first[i]) : ~(u64)0;
    }
}
// zj_entry_owner over any ascending array (the caller's index has buffers without entries: repeated values)
extern "C" ull emu_entry_owner(const ull* first, ull n, ull e) { return zj_entry_owner((const u64*)first, n, e); }
extern "C" ull emu_pieces_bound(ull size, ull pieces) { return zj_pieces_bound(size, pieces); }
extern "C" ull emu_compress_bound(ull size) { return zj_compress_bound(size); }
