// zj_frames.h — large buffers as many frames: the arithmetic that turns "n large buffers" into "E small entries", host and device.
//
// Decompress (zjni_decompress_frames_batch_device): a buffer of concatenated frames is SPLIT into one entry per frame when
//   (a) it holds at most 2^32 - 1 bytes,
//   (b) a walk with zj_frame_step from byte 0 until no byte is left meets no error,
//   (c) every zstd frame on the way records a content size, and
//   (d) there are at least two zstd frames;
// otherwise it is one entry, the whole buffer.  A skippable frame of a split buffer is an entry that decodes to 0 bytes.  Entry sources are the frames'
// extents; entry destinations start at the buffer's slot plus the content sizes before them, clamped to the slot's end (zjni_decompress_offsets_device's
// trick: what does not fit gets a short slot and the decoder answers dstSize_tooSmall by itself).  Both are contiguous, so one uint64[E + 1] array each.
// zj_frames_count is the first walk (one lane per buffer), zj_frames_emit the second, behind a prefix sum of the counts.
//
// Compress (zjni_compress_chunked_batch_device): buffer i is cut into max(1, ceil(size / chunk)) pieces, each its own frame; zj_chunk_* say how many,
// where piece k begins and where its zjni_compressBound-sized scratch destination lies.
#pragma once
#include "zj_frameinfo.h"

#define ZJ_FRAMES_SRC_MAX 0xFFFFFFFFull

// entries of the buffer [p, p + n): 1 = not split, otherwise the number of its frames (zstd and skippable; at least 2)
ZJ_HD u32 zj_frames_count(const u8* p, u64 n) {
    if (n > ZJ_FRAMES_SRC_MAX) return 1u;
    ZFStep s;
    u64 pos = 0;
    u32 frames = 0, entries = 0;
    ZJ_NO_UNROLL
    while (pos < n) {
        zj_frame_step(p + pos, n - pos, s);
        if (zj_fi_is_err(s.csize)) return 1u;
        if (!s.skippable) {
            if (s.fcs == ZJ_FI_UNKNOWN) return 1u;
            frames++;
        }
        entries++;
        pos += s.csize;
    }
    return frames >= 2u ? entries : 1u;
}

// The entries of buffer [p, p + n) = source bytes [srcLo, srcLo + n) with the destination slot [dstLo, dstLo + dstCap): srcOff[0 .. entries) and
// dstOff[0 .. entries) (the caller passes the arrays at the buffer's first entry; the end of an entry is the beginning of the next one, the last entry's
// the next buffer's).  `entries` is zj_frames_count's answer: the walk is bounded by it, so it writes exactly that many whatever the bytes say now.
ZJ_HD void zj_frames_emit(const u8* p, u64 n, u64 srcLo, u64 dstLo, u64 dstCap, u32 entries, u64* srcOff, u64* dstOff) {
    srcOff[0] = srcLo; dstOff[0] = dstLo;
    if (entries < 2u) return;
    ZFStep s;
    u64 pos = 0, out = 0;
    ZJ_NO_UNROLL
    for (u32 k = 0; k < entries; k++) {
        srcOff[k] = srcLo + pos;
        dstOff[k] = dstLo + (out < dstCap ? out : dstCap);
        if (pos >= n) continue;                             // (only when the bytes changed between the walks: empty entries, inside the buffer)
        zj_frame_step(p + pos, n - pos, s);
        if (zj_fi_is_err(s.csize)) { pos = n; continue; }
        if (!s.skippable && s.fcs != ZJ_FI_UNKNOWN) out = zj_sat_add(out, s.fcs);
        pos += s.csize;
    }
}

// ---- chunked compress ----
ZJ_HD u64 zj_compress_bound(u64 s) { return s + (s >> 8) + (s < (128u << 10) ? (((128u << 10) - s) >> 11) : 0); }      // ZSTD_COMPRESSBOUND (zjni_compressBound)
// pieces of a buffer of `size` bytes: an empty buffer is the one frame of an empty input
ZJ_HD u64 zj_chunk_count(u64 size, u64 chunk) { return size ? (size - 1) / chunk + 1 : 1; }
// bytes of piece k
ZJ_HD u64 zj_chunk_size(u64 size, u64 chunk, u64 k) { u64 const at = k * chunk; return size - at < chunk ? size - at : chunk; }
// zjni_compressBound_chunked: the sum of zjni_compressBound over the pieces = what the pieces' scratch destinations take
ZJ_HD u64 zj_chunk_bound_total(u64 size, u64 chunk) {
    u64 const c = zj_chunk_count(size, chunk);
    return (c - 1) * zj_compress_bound(chunk) + zj_compress_bound(size - (c - 1) * chunk);
}
// where piece k of a buffer starts: in the source (the buffer begins at srcLo) and among the scratch destinations (the buffer's first begins at dstBase)
ZJ_HD u64 zj_chunk_src(u64 srcLo, u64 chunk, u64 k) { return srcLo + k * chunk; }
ZJ_HD u64 zj_chunk_dst(u64 dstBase, u64 chunk, u64 k) { return dstBase + k * zj_compress_bound(chunk); }
// the buffer that owns entry e: the last i with first[i] <= e (first[0 .. n] ascending, first[0] = 0, every buffer owns at least one entry, e < first[n])
ZJ_HD u64 zj_entry_owner(const u64* first, u64 n, u64 e) {
    u64 lo = 0, hi = n;
    while (hi - lo > 1) { u64 const mid = lo + (hi - lo) / 2; if (first[mid] <= e) lo = mid; else hi = mid; }
    return lo;
}

// ---- pieces: the caller's cuts (zjni_compress_pieces_batch_device) ----
// A buffer of `size` bytes with the cuts cut[0 .. c): its pieces are the gaps [0, cut[0]), [cut[0], cut[1]), ..., [cut[c - 1], size).
// zjni_compressBound_pieces: ZSTD_COMPRESSBOUND's small-input margin is at most (128 KiB >> 11) = 64 a piece, and the pieces' >> 8 terms sum to at most the whole's
ZJ_HD u64 zj_pieces_bound(u64 size, u64 pieces) { return size + (size >> 8) + 64 * (pieces ? pieces : 1); }
// a list without cuts: one piece, legal when it is not above `chunk` (an empty buffer is the one frame of an empty input)
ZJ_HD bool zj_cut_none_ok(u64 size, u64 chunk) { return size <= chunk; }
// cut k of c, one lane's share of the legality check: strictly above its left neighbour (0 for the first: no cut of 0), below `size`, the piece it closes not above
// `chunk`; the last cut answers for the piece behind it as well
ZJ_HD bool zj_cut_ok(const u64* cut, u64 c, u64 k, u64 size, u64 chunk) {
    u64 const v = cut[k], left = k ? cut[k - 1] : 0;
    if (v <= left || v >= size || v - left > chunk) return false;
    return k + 1 < c || size - v <= chunk;
}
// where piece k begins in the source (the buffer begins at srcLo): behind cut k - 1, or on the fixed grid when the buffer has no list (cut == nullptr)
ZJ_HD u64 zj_piece_src(u64 srcLo, u64 chunk, const u64* cut, u64 k) { return cut ? srcLo + (k ? cut[k - 1] : 0) : zj_chunk_src(srcLo, chunk, k); }
// A buffer with an illegal list owns no entry of the caller's index, but its bytes lie between its neighbours' and an entry ends where the next one begins: inside
// the call it is walked on the fixed grid (zj_chunk_count entries whose frames go nowhere), so that every entry of a legal buffer keeps its own extent.
ZJ_HD u64 zj_pieces_walked(bool legal, u64 pieces, u64 size, u64 chunk) { return legal ? pieces : zj_chunk_count(size, chunk); }
