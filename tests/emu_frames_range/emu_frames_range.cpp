// tests/emu_frames_range/emu_frames_range.cpp — lane-serial build of zj_frames_range.h as the kernels of zjni_decompress_frames_range_batch_device call it: every
// "lane" (buffer) or workgroup (tile) in turn over a batch in host memory, with the five prefix sums between the two walks done here.  For
// tests/test_emu_frames_range.py.  TEST INFRASTRUCTURE ONLY: never linked into libzjni_amd.so.
#include "../../zstd-jni_amd/csrc/zj_frames_range.h"
#include <stdlib.h>
#include <string.h>

typedef unsigned long long ull;
extern "C" unsigned emu_range_rec_bytes(void) { return (unsigned)sizeof(ZRRec); }
extern "C" unsigned emu_range_tile(void) { return ZJ_RANGE_TILE; }

// zj_range_count_kernel + zj_range_scan_kernel: rec[n], scan[5][n + 1] (scan[k][n] = the totals the host reads), total[n]
extern "C" void emu_range_count(const unsigned char* src, const ull* off, const ull* dstOff, const ull* range, unsigned n, void* rec, ull* scan, ull* total) {
    u64 run[5] = {0, 0, 0, 0, 0};
    for (u32 i = 0; i < n; i++) {
        u64 const lo = off[i], hi = off[i + 1], dlo = dstOff[i], dhi = dstOff[i + 1];
        u64 q[5];
        zj_range_count(src + lo, hi > lo ? hi - lo : 0, range[2 * i], range[2 * i + 1], dhi > dlo ? dhi - dlo : 0, ((ZRRec*)rec)[i], q);
        for (u32 k = 0; k < 5; k++) { scan[(u64)k * (n + 1) + i] = run[k]; run[k] += q[k]; }
        if (total) total[i] = ((ZRRec*)rec)[i].total;
    }
    for (u32 k = 0; k < 5; k++) scan[(u64)k * (n + 1) + n] = run[k];
}
// zj_range_emit_kernel: srcA / dstA [EA + 1], srcB / dstB [EB + 1], in [3n] (key, other, len), out [2n]
extern "C" void emu_range_emit(const unsigned char* src, const ull* off, const ull* dstOff, const void* rec, const ull* scan, unsigned n,
                               ull* srcA, ull* dstA, ull* srcB, ull* dstB, ull* in3, ull* out3) {
    u64 const n1 = (u64)n + 1u;
    const ull* const fA = scan; const ull* const fB = scan + n1; const ull* const cA = scan + 2 * n1; const ull* const cB = scan + 3 * n1; const ull* const eB = scan + 4 * n1;
    ZRCopy* const in = (ZRCopy*)in3; ZRCopy* const out = (ZRCopy*)out3;
    for (u32 i = 0; i < n; i++) {
        u64 const lo = off[i], hi = off[i + 1], a0 = fA[i], a1 = fA[i + 1], b0 = fB[i];
        ZRCopy cin[3], cout[2];
        zj_range_emit(src + lo, hi > lo ? hi - lo : 0, ((const ZRRec*)rec)[i], lo, dstOff[i], (u32)(a1 - a0 - 1u), cA[i], cA[n] + cB[i], eB[i],
                      (u64*)srcA + a0, (u64*)dstA + a0, (u64*)srcB + b0, (u64*)dstB + b0, cin, cout);
        in[i] = cin[0]; in[(u64)n + 2 * i] = cin[1]; in[(u64)n + 2 * i + 1] = cin[2];
        out[2 * i] = cout[0]; out[2 * i + 1] = cout[1];
        if (i + 1 == n) { srcA[a1] = cA[n]; dstA[a1] = dstA[a1 - 1]; srcB[fB[n]] = cA[n] + cB[n]; dstB[fB[n]] = eB[n]; }
    }
}
// one copy as a workgroup of zj_range_gather_kernel makes it: the plan's head, body and tail, piece by piece; returns head | tail << 8 | wide << 16, *body = the pieces
static u32 copy_planned(const u8* s, u8* d, u64 len, u64* body) {
    ZRPlan const pl = zj_range_copy_plan((u64)(uintptr_t)s, (u64)(uintptr_t)d, len);
    for (u32 t = 0; t < pl.head; t++) d[t] = s[t];
    const u8* const sb = s + pl.head; u8* const db = d + pl.head;
    for (u64 k = 0; k < pl.body; k++) {
        if (pl.wide) { if (((uintptr_t)(sb + 16 * k) | (uintptr_t)(db + 16 * k)) & 15u) abort(); memcpy(db + 16 * k, sb + 16 * k, 16); }
        else { u64 const a = ld64(sb + 16 * k), b = ld64(sb + 16 * k + 8); st64(db + 16 * k, a); st64(db + 16 * k + 8, b); }
    }
    for (u32 t = 0; t < pl.tail; t++) db[(pl.body << 4) + t] = sb[(pl.body << 4) + t];
    if (pl.head > 15u || pl.tail > 15u || pl.head + (pl.body << 4) + pl.tail != len) abort();
    if (body) *body = pl.body;
    return pl.head | (pl.tail << 8) | (pl.wide << 16);
}
extern "C" unsigned emu_range_copy(const unsigned char* s, unsigned char* d, ull len, ull* body) { return copy_planned(s, d, len, (u64*)body); }
// zj_range_gather_kernel, every tile in turn; returns the tiles that moved at least one byte
extern "C" ull emu_range_gather(const ull* runs3, ull D, const unsigned char* srcBase, unsigned char* dstBase, unsigned keyIsDst, ull keyEnd) {
    const ZRCopy* const runs = (const ZRCopy*)runs3;
    u64 busy = 0;
    for (u64 tLo = 0; tLo < keyEnd; tLo += ZJ_RANGE_TILE) {
        u64 const tHi = tLo + ZJ_RANGE_TILE < keyEnd ? tLo + ZJ_RANGE_TILE : keyEnd;
        bool moved = false;
        for (u64 d = zj_range_tile_first(runs, D, tLo); d < D; d++) {
            ZRCopy const c = runs[d];
            if (c.key >= tHi) break;
            u64 at = 0;
            u64 const len = zj_range_tile_part(c, tLo, tHi, &at);
            if (!len) continue;
            copy_planned(srcBase + (keyIsDst ? c.other : c.key) + at, dstBase + (keyIsDst ? c.key : c.other) + at, len, nullptr);
            moved = true;
        }
        busy += moved;
    }
    return busy;
}
