// zj_frames_range.h — ranged decompress of a buffer of many frames: which frames a range of decoded bytes touches, where they decode to, and what is
// copied where.  Arithmetic only, host and device (zjni_decompress_frames_range_batch_device; the kernels are in zj_kernels.hip beside the frames layer).
//
// A buffer is INDEXABLE when a walk with zj_frame_step from byte 0 until no byte is left meets no error, every zstd frame records a content size, the source
// is at most 2^32 - 1 bytes and the content sizes sum below 2^64; whatever fails first in walk order answers for the buffer.  T = that sum.  The range
// [lo, lo + len) is clamped to [lo', hi') within [0, T].  `first` is the frame holding decoded byte lo', `last` the one holding hi' - 1 (a frame of no content
// holds no byte); every frame from first to last is SELECTED and nothing else is looked at by a decoder.  first is an EDGE when it begins before lo', last when it
// ends after hi'; one frame that is both counts once.  The other selected frames are INTERIOR.
//
// Interior frame k decodes straight into the caller's slot at dlo + (P_k - lo') (P_k: content before it) with a slot of exactly its content size.  An edge frame
// decodes into scratch, a slot of exactly its content size again, and its part of the range is copied out afterwards.  The decode pipelines want contiguous
// uint64[E + 1] offsets on one base, and selections of different buffers are not neighbours in the source, so the selected source bytes are copied first:
//   set A (base: the caller's destination)  the interior frames of every buffer, then one CLOSING entry per buffer: no source byte, a slot up to the next
//                                           buffer's first interior; it writes nothing and its answer is not read
//   set B (base: scratch)                   the edge frames, at most two per buffer
// Copies are runs {key, other, len}: `key` is the offset on the scratch side, which ascends from run to run, `other` the offset on the caller's side.  The
// gather cuts the KEY space into tiles of ZJ_RANGE_TILE bytes, so a long run spreads over the device and a tile finds its runs by bisection.
#pragma once
#include "zj_frames.h"

#define ZJ_RANGE_SELECTED 0u      // ZRRec.status: frames are decoded; 1: the clamped range is empty, the answer is 0; anything else: that error code
#define ZJ_RANGE_NOTHING 1u
#define ZJ_RANGE_TILE 65536u

// what the counting walk keeps of a buffer
struct ZRRec {
    u64 total, lo, hi;            // T (ZJ_FI_ERROR: not indexable), lo', hi'
    u64 posF, endF, posL, endL;   // the source extents of first and last inside the buffer
    u64 preF, preL;               // content before first / before last
    u64 fcsF, fcsL;               // their content sizes
    u32 status, frames;           // frames: first .. last
    u32 edges, pad;               // bit 0: first is an entry of set B; bit 1: last is one too, and another frame than first
};
struct ZRCopy { u64 key, other, len; };

ZJ_HD u32 zj_range_edge_count(u32 edges) { return (edges & 1u) + (edges >> 1); }

// The counting walk of buffer [p, p + n) for the range [lo, lo + len) and a destination slot of `slot` bytes.  q[0 .. 5): entries of set A, entries of set B,
// source bytes of set A, source bytes of set B, scratch bytes of the edge frames — what the scans add up.
ZJ_HD void zj_range_count(const u8* p, u64 n, u64 lo, u64 len, u64 slot, ZRRec& r, u64* q) {
    r.total = ZJ_FI_ERROR; r.lo = r.hi = 0; r.posF = r.endF = r.posL = r.endL = 0; r.preF = r.preL = r.fcsF = r.fcsL = 0;
    r.status = ZJ_E_FRAMEPARAM_UNSUPPORTED; r.frames = 0; r.edges = 0; r.pad = 0;
    q[0] = 1; q[1] = q[2] = q[3] = q[4] = 0;
    if (n > ZJ_FRAMES_SRC_MAX) return;
    u64 const hi = zj_sat_add(lo, len);
    ZFStep s;
    u64 pos = 0, P = 0;
    u32 idx = 0, idxF = 0, idxL = 0;
    bool found = false;
    ZJ_NO_UNROLL
    while (pos < n) {
        zj_frame_step(p + pos, n - pos, s);
        if (zj_fi_is_err(s.csize)) { r.status = (u32)((u64)0 - s.csize); return; }
        if (!s.skippable && s.fcs == ZJ_FI_UNKNOWN) return;
        u64 const fcs = s.skippable ? 0 : s.fcs;
        if (P + fcs < P) return;
        if (fcs) {
            if (!found && P + fcs > lo) { found = true; r.posF = pos; r.endF = pos + s.csize; r.preF = P; r.fcsF = fcs; idxF = idx; }
            if (P < hi) { r.posL = pos; r.endL = pos + s.csize; r.preL = P; r.fcsL = fcs; idxL = idx; }
        }
        P += fcs; pos += s.csize; idx++;
    }
    r.total = P; r.lo = lo < P ? lo : P; r.hi = hi < P ? hi : P;
    if (r.lo == r.hi) { r.status = ZJ_RANGE_NOTHING; return; }
    if (slot < r.hi - r.lo) { r.status = ZJ_E_DSTSIZE_TOO_SMALL; return; }
    u32 const frames = idxL - idxF + 1u;
    bool const eF = r.preF < r.lo, eL = r.preL + r.fcsL > r.hi;
    u32 const edges = frames == 1u ? (u32)(eF || eL) : ((u32)eF | ((u32)eL << 1));
    if (((edges & 1u) && r.fcsF > ZJNI_RANGE_EDGE_MAX) || ((edges & 2u) && r.fcsL > ZJNI_RANGE_EDGE_MAX)) { r.status = 64u; return; }
    r.status = ZJ_RANGE_SELECTED; r.frames = frames; r.edges = edges;
    u64 const runLo = (edges & 1u) ? r.endF : r.posF, runHi = (edges & 2u) ? r.posL : r.endL;
    q[0] = (u64)(frames - zj_range_edge_count(edges)) + 1u;
    q[1] = zj_range_edge_count(edges);
    q[2] = runHi - runLo;
    q[3] = ((edges & 1u) ? r.endF - r.posF : 0) + ((edges & 2u) ? r.endL - r.posL : 0);
    q[4] = ((edges & 1u) ? r.fcsF : 0) + ((edges & 2u) ? r.fcsL : 0);
}

// The second walk of buffer [p, p + n), which lies at srcLo in the batch's source and has its slot at dlo: from `first`, over the `interior` frames counted.
//   srcA, dstA   the buffer's interior + 1 entries of set A (the last is the closing entry); sources begin at a0 in the compact bytes
//   srcB, dstB   its entries of set B; sources begin at b0 in the compact bytes, scratch slots at e0
//   in[3]        source -> compact bytes (key: compact): the interior run, edge first, edge last
//   out[2]       edge scratch (key) -> the caller's slot: the part of each edge frame inside the range
// The walk is bounded by the counts and every offset by the extents the first walk recorded, whatever the bytes say now.
ZJ_HD void zj_range_emit(const u8* p, u64 n, const ZRRec& r, u64 srcLo, u64 dlo, u32 interior, u64 a0, u64 b0, u64 e0,
                         u64* srcA, u64* dstA, u64* srcB, u64* dstB, ZRCopy* in, ZRCopy* out) {
    in[0].key = a0; in[0].other = 0; in[0].len = 0;
    in[1].key = in[2].key = b0; in[1].other = in[2].other = 0; in[1].len = in[2].len = 0;
    out[0].key = out[1].key = e0; out[0].other = out[1].other = 0; out[0].len = out[1].len = 0;
    if (r.status != ZJ_RANGE_SELECTED) { srcA[0] = a0; dstA[0] = dlo; return; }
    u32 const e = r.edges;
    u64 const runLo = (e & 1u) ? r.endF : r.posF, runHi = (e & 2u) ? r.posL : r.endL, bytesA = runHi - runLo, want = r.hi - r.lo;
    in[0].other = srcLo + runLo; in[0].len = bytesA;
    u64 at = b0, atE = e0;
    u32 k = 0;
    if (e & 1u) {
        u64 const sLo = r.lo - r.preF, sHi = (r.hi < r.preF + r.fcsF ? r.hi : r.preF + r.fcsF) - r.preF;
        srcB[k] = at; dstB[k] = atE; k++;
        in[1].other = srcLo + r.posF; in[1].len = r.endF - r.posF;
        out[0].key = atE + sLo; out[0].other = dlo; out[0].len = sHi - sLo;
        at += r.endF - r.posF; atE += r.fcsF;
    }
    in[2].key = at; out[1].key = atE;
    if (e & 2u) {
        srcB[k] = at; dstB[k] = atE;
        in[2].other = srcLo + r.posL; in[2].len = r.endL - r.posL;
        out[1].other = dlo + (r.preL - r.lo); out[1].len = r.hi - r.preL;
    }
    ZFStep s;
    u64 pos = runLo, done = ((e & 1u) ? r.preF + r.fcsF : r.preF) - r.lo;
    ZJ_NO_UNROLL
    for (u32 j = 0; j < interior; j++) {
        srcA[j] = a0 + (pos - runLo);
        dstA[j] = dlo + (done < want ? done : want);
        if (pos >= runHi) continue;                         // (only when the bytes changed between the walks: empty entries, inside the buffer's extents)
        zj_frame_step(p + pos, n - pos, s);
        if (zj_fi_is_err(s.csize) || s.csize > runHi - pos) { pos = runHi; continue; }
        if (!s.skippable && s.fcs != ZJ_FI_UNKNOWN) done = zj_sat_add(done, s.fcs);
        pos += s.csize;
    }
    srcA[interior] = a0 + bytesA;
    dstA[interior] = dlo + (done < want ? done : want);
}

// ---- the gather ----
// the first run a tile that begins at key tLo can touch: the last d with c[d].key <= tLo (keys ascend; runs of no byte share a key with the run behind them)
ZJ_HD u64 zj_range_tile_first(const ZRCopy* c, u64 D, u64 tLo) {
    u64 lo = 0, hi = D;
    while (hi - lo > 1) { u64 const mid = lo + (hi - lo) / 2; if (c[mid].key <= tLo) lo = mid; else hi = mid; }
    return lo;
}
// what of run c lies in the tile [tLo, tHi) of the key space: its bytes (0: none) and where in the run they begin
ZJ_HD u64 zj_range_tile_part(const ZRCopy& c, u64 tLo, u64 tHi, u64* at) {
    u64 const lo = c.key > tLo ? c.key : tLo, end = c.key + c.len, hi = end < tHi ? end : tHi;
    if (hi <= lo) return 0;
    *at = lo - c.key;
    return hi - lo;
}
// len bytes from address src to address dst: `head` single bytes, `body` pieces of 16, `tail` single bytes.  wide: source and destination share their
// residue mod 16, the head reaches the boundary and the pieces are aligned on both sides; otherwise the pieces are two unaligned 8-byte words from byte 0.
struct ZRPlan { u64 body; u32 head, tail, wide; };
ZJ_HD ZRPlan zj_range_copy_plan(u64 src, u64 dst, u64 len) {
    ZRPlan pl;
    pl.wide = ((src ^ dst) & 15u) == 0;
    u64 const toBoundary = (16u - (dst & 15u)) & 15u;
    pl.head = pl.wide ? (u32)(toBoundary < len ? toBoundary : len) : 0u;
    pl.body = (len - pl.head) >> 4;
    pl.tail = (u32)(len - pl.head - (pl.body << 4));
    return pl;
}
