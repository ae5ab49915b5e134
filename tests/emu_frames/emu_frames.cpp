// tests/emu_frames/emu_frames.cpp — lane-serial build of zj_frames.h as the kernels of zjni_decompress_frames_batch_device and zjni_compress_chunked_batch_device
// call it: every "lane" (buffer, or entry) in turn over a batch in host memory, with the prefix sums between the two walks done here.  For tests/test_emu_frames.py.
// TEST INFRASTRUCTURE ONLY: never linked into libzjni_amd.so.
#include "../../zstd-jni_amd/csrc/zj_frames.h"
#include <stdlib.h>

// zj_frames_count_kernel + the scan: first[0 .. n] = exclusive prefix sums of the buffers' entry counts; returns E
extern "C" unsigned long long emu_frames_count(const unsigned char* src, const unsigned long long* off, unsigned n, unsigned long long* first) {
    u64 run = 0;
    for (u32 i = 0; i < n; i++) {
        u64 const lo = off[i], hi = off[i + 1];
        first[i] = run;
        run += zj_frames_count(src + lo, hi > lo ? hi - lo : 0);
    }
    first[n] = run;
    return run;
}
// zj_frames_emit_kernel: srcOffE[0 .. E], dstOffE[0 .. E]
extern "C" void emu_frames_emit(const unsigned char* src, const unsigned long long* off, const unsigned long long* dstOff, const unsigned long long* first, unsigned n,
                                unsigned long long* srcOffE, unsigned long long* dstOffE) {
    for (u32 i = 0; i < n; i++) {
        u64 const lo = off[i], hi = off[i + 1], dlo = dstOff[i], dhi = dstOff[i + 1], e0 = first[i], e1 = first[i + 1];
        zj_frames_emit(src + lo, hi > lo ? hi - lo : 0, lo, dlo, dhi > dlo ? dhi - dlo : 0, (u32)(e1 - e0), (u64*)srcOffE + e0, (u64*)dstOffE + e0);
        if (i + 1 == n) { srcOffE[e1] = hi; dstOffE[e1] = dhi; }
    }
}
// zj_chunks_count_kernel + its two scans: first[0 .. n] (entries), bbase[0 .. n] (scratch destinations); returns E
extern "C" unsigned long long emu_chunks_count(const unsigned long long* off, unsigned n, unsigned long long chunk, unsigned long long* first, unsigned long long* bbase) {
    u64 e = 0, b = 0;
    for (u32 i = 0; i < n; i++) {
        u64 const lo = off[i], hi = off[i + 1], size = hi > lo ? hi - lo : 0;
        first[i] = e; bbase[i] = b;
        e += zj_chunk_count(size, chunk); b += zj_chunk_bound_total(size, chunk);
    }
    first[n] = e; bbase[n] = b;
    return e;
}
// zj_chunks_emit_kernel for the slice [a, a + m], its end included: srcOffS[0 .. m], dstOffS[0 .. m]
extern "C" void emu_chunks_emit(const unsigned long long* off, const unsigned long long* first, const unsigned long long* bbase, unsigned n, unsigned long long chunk,
                                unsigned long long a, unsigned m, unsigned long long E, unsigned long long* srcOffS, unsigned long long* dstOffS) {
    for (u64 j = 0; j <= m; j++) {
        u64 const ia = zj_entry_owner((const u64*)first, n, a), dstA = zj_chunk_dst(bbase[ia], chunk, a - first[ia]);
        u64 const e = a + j;
        if (e >= E) { srcOffS[j] = off[n]; dstOffS[j] = bbase[n] - dstA; continue; }
        u64 const i = zj_entry_owner((const u64*)first, n, e), k = e - first[i];
        srcOffS[j] = zj_chunk_src(off[i], chunk, k);
        dstOffS[j] = zj_chunk_dst(bbase[i], chunk, k) - dstA;
    }
}
extern "C" unsigned long long emu_chunk_bound_total(unsigned long long size, unsigned long long chunk) { return zj_chunk_bound_total(size, chunk); }
