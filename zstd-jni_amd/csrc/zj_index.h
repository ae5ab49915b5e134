// zj_index.h — range reads by a caller-held index instead of a walk over the frame headers: the prepared index, the request that finds its entries by bisection,
// and the entries of set A one lane each.  Arithmetic only, host and device (zjni_index_from_*_device, zjni_decompress_index_range_batch_device; the kernels are in
// zj_kernels.hip beside the range layer).  The index is built from the sizes the compress call returned, or from the frames alone by a walk over their headers
// (zj_index_walk: zjni_index_count_frames_device, zjni_index_from_frames_device, zjni_index_from_frames).
//
// THE INDEX of n buffers and E entries is (2n + 1) + 2(E + 1) words of 64 bits in the caller's device memory:
//   first[n + 1]   entries before each buffer           valid[n]   0, or the error code that answers for the buffer (2 .. 2^32 - 1)
//   C[E + 1]       exclusive running sums of the entries' compressed sizes over the whole batch          U[E + 1]   the same of their content sizes
// An entry is a whole number of frames.  Everything a request needs of buffer b is a difference against C[first[b]] / U[first[b]].
//
// A REQUEST (b, lo, len) is decided by zj_index_request as zj_range_count decides a buffer, with bisection over U where that one walks: it fills the same ZRRec and
// the same five quantities, so the scans, set B, the copy runs, the gather and the decode launches behind it are the range layer's own (zj_frames_range.h).
//
// The index is caller memory and may hold anything.  Rule 1 keeps every read of it inside its E + 1 sums; every extent the record keeps is clamped into the
// buffer (0 <= posF <= endF <= posL <= endL <= the source extent); a selection the sums contradict (the entry found does not hold the byte, an edge that is no
// edge) answers 20; and an interior entry whose own two sums do not ascend inside the run marks its request (zj_index_entry_ok), whose entries then all get a
// slot of no byte (the run's gathered bytes lie in its own last interior entry) and whose answer is 20 — the decoders take sizes as differences of neighbours,
// so the arrays they are handed ascend whatever the sums say, and every closing entry stays without a source byte.
#pragma once
#include "zj_frames_range.h"

#define ZJ_INDEX_SIZE_MAX 0xFFFFFFFFull       // an entry's compressed size and content size
#define ZJ_INDEX_SCAN_WG 1024u                // lanes of the scan workgroup: lane t sums ceil(E / 1024) neighbours
#define ZJ_INDEX_EMIT_WG 256u                 // lanes of a workgroup of the kernels that take one entry of set A per lane

ZJ_HD u64 zj_index_words(u64 n, u64 E) { return 2 * n + 1 + 2 * (E + 1); }
ZJ_HD u64 zj_index_bytes(u64 n, u64 E) { return (zj_index_words(n, E) * 8 + 255) & ~(u64)255; }
struct ZIView { const u64* first; const u64* valid; const u64* C; const u64* U; };
ZJ_HD ZIView zj_index_view(const u64* idx, u64 n, u64 E) { ZIView v; v.first = idx; v.valid = idx + n + 1; v.C = idx + 2 * n + 1; v.U = v.C + E + 1; return v; }

// ---- the builders ----
// what an entry's size counts in the sums: a size above the maximum makes its buffer illegal and counts 0, so the other buffers' differences stay exact
ZJ_HD u64 zj_index_term(u64 size) { return size > ZJ_INDEX_SIZE_MAX ? 0 : size; }
// buffer i of the caller's first[n + 1]: does it ascend at i and end inside the E entries (its sizes are looked at only then)
ZJ_HD bool zj_index_first_ok(const u64* first, u64 i, u64 E) { return first[i] <= first[i + 1] && first[i + 1] <= E; }
// valid[i]: the buffer's own error first (result: NULL, or what the compress call answered), then the legality of its entries
ZJ_HD u64 zj_index_valid(bool legal, const u64* result, u64 i) {
    if (result && result[i] > ((u64)1 << 40)) { u64 const c = (u64)0 - result[i]; return c >= 2 && c <= 0xFFFFFFFFull ? c : 42u; }
    return legal ? 0 : 42u;
}
// the content size of entry k of a buffer of `size` bytes cut as zjni_compress_pieces_batch_device cuts it: by its c cuts, or on the fixed grid (cut == nullptr)
ZJ_HD u64 zj_index_piece_content(u64 size, u64 chunk, const u64* cut, u64 c, u64 k) {
    if (!cut) return k < zj_chunk_count(size, chunk) ? zj_chunk_size(size, chunk, k) : 0;
    if (k > c) return 0;
    u64 const lo = k ? cut[k - 1] : 0, hi = k < c ? cut[k] : size;
    return hi > lo ? hi - lo : 0;
}

// ---- the index from the frames alone (zjni_index_count_frames_device, zjni_index_from_frames_device, zjni_index_from_frames) ----
// The walk of buffer [p, p + n): its verdict (0: indexable, else the code that answers for it) and, in *entries, its entry count — one entry a frame, a
// skippable frame an entry of content 0; a buffer that is not indexable has 0 entries, as has an empty one.  The first min(frames passed, cap) frames'
// compressed sizes and content sizes go to size[] and content[] (cap == 0: nothing is written, the counting call), and *wrote says how many did.
// The verdict is rule 1 of the ranged entry (zj_range_count) in walk order, first failure first: a source above ZJ_FRAMES_SRC_MAX 14, a step's error that
// step's code, a zstd frame without a content size 14, content sizes summing past 64 bits 14.  ONE ADDITION, which the index's entry format forces
// (ZJ_INDEX_SIZE_MAX): a frame that records a content size above 2^32 - 1 answers 14 at that frame.  It is the only place where the walked ranged entry and
// a read by the walk-built index may answer differently for the same bytes.  (A frame's compressed size cannot exceed the maximum: the source does not.)
ZJ_HD u32 zj_index_walk(const u8* p, u64 n, u64 cap, u64* size, u64* content, u64* entries, u64* wrote) {
    *entries = 0; *wrote = 0;
    if (n > ZJ_FRAMES_SRC_MAX) return ZJ_E_FRAMEPARAM_UNSUPPORTED;
    ZFStep s;
    u64 pos = 0, P = 0, k = 0;
    ZJ_NO_UNROLL
    while (pos < n) {
        zj_frame_step(p + pos, n - pos, s);
        if (zj_fi_is_err(s.csize)) return (u32)((u64)0 - s.csize);
        if (!s.skippable && s.fcs == ZJ_FI_UNKNOWN) return ZJ_E_FRAMEPARAM_UNSUPPORTED;
        u64 const fcs = s.skippable ? 0 : s.fcs;
        if (fcs > ZJ_INDEX_SIZE_MAX || P + fcs < P) return ZJ_E_FRAMEPARAM_UNSUPPORTED;
        if (k < cap) { size[k] = s.csize; content[k] = fcs; *wrote = k + 1; }
        P += fcs; pos += s.csize; k++;
    }
    *entries = k;
    return 0;
}
// The second walk of buffer i = [p, p + n), whose entries lie at first[i] .. first[i + 1] of size[E] and content[E]: valid[i].  It trusts nothing of the first
// walk, whatever the bytes say now: a first[] that does not ascend at i or ends beyond E answers 42 and writes nothing (zj_index_first_ok); the walk writes
// inside the buffer's own extent only; one that does not end at the buffer's end with exactly first[i + 1] - first[i] entries answers 42, and what it wrote is
// written again as 0.  (A buffer that is not indexable owns no entry and keeps its verdict.)
ZJ_HD u64 zj_index_frames_emit(const u8* p, u64 n, const u64* first, u64 i, u64 E, u64* size, u64* content) {
    if (!zj_index_first_ok(first, i, E)) return 42u;
    u64 const f0 = first[i], cap = first[i + 1] - f0;
    u64 entries, wrote;
    u32 const verdict = zj_index_walk(p, n, cap, size + f0, content + f0, &entries, &wrote);
    if (verdict ? cap == 0 : entries == cap) return verdict;
    for (u64 k = 0; k < wrote; k++) { size[f0 + k] = 0; content[f0 + k] = 0; }
    return 42u;
}

// ---- the request ----
struct ZIReq { u64 e0, cBase, uBase, srcLo; };      // first entry of the request's set A in the index; C and U at the buffer's first entry; the buffer in the source
// the last j in [f0, f1) with U[j] - base <= x (f0 < f1; U[f0] - base = 0 <= x)
ZJ_HD u64 zj_index_bisect(const u64* U, u64 f0, u64 f1, u64 base, u64 x) {
    u64 lo = f0, hi = f1;
    while (hi - lo > 1) { u64 const mid = lo + (hi - lo) / 2; if (U[mid] >= base && U[mid] - base <= x) lo = mid; else hi = mid; }
    return lo;
}
ZJ_HD u64 zj_index_rel(u64 v, u64 base, u64 lo, u64 hi) { u64 const r = v >= base ? v - base : 0; return r < lo ? lo : (r > hi ? hi : r); }
// Rules 1-4 for request (b, lo, len) with a slot of `slot` bytes: the record, ir, and q[0 .. 5) as zj_range_count gives them.  off[n + 1]: the buffers in the source.
ZJ_HD void zj_index_request(const u64* idx, u64 n, u64 E, const u64* off, u64 b, u64 lo, u64 len, u64 slot, ZRRec& r, ZIReq& ir, u64* q) {
    r.total = ZJ_FI_ERROR; r.lo = r.hi = 0; r.posF = r.endF = r.posL = r.endL = 0; r.preF = r.preL = r.fcsF = r.fcsL = 0;
    r.status = 42u; r.frames = 0; r.edges = 0; r.pad = 0;
    ir.e0 = ir.cBase = ir.uBase = ir.srcLo = 0;
    q[0] = 1; q[1] = q[2] = q[3] = q[4] = 0;
    if (b >= n) return;
    ZIView const v = zj_index_view(idx, n, E);
    u64 const f0 = v.first[b], f1 = v.first[b + 1], bad = v.valid[b];
    if (bad) { r.status = bad >= 2 && bad <= 0xFFFFFFFFull ? (u32)bad : 42u; return; }
    if (f0 > f1 || f1 > E) return;
    u64 const sLo = off[b], sHi = off[b + 1], ext = sHi > sLo ? sHi - sLo : 0, c0 = v.C[f0], u0 = v.U[f0];
    if (v.C[f1] < c0 || v.C[f1] - c0 != ext) { r.status = ZJ_E_SRCSIZE_WRONG; return; }
    u64 const T = v.U[f1] >= u0 ? v.U[f1] - u0 : 0, hi = zj_sat_add(lo, len);
    r.total = T; r.lo = lo < T ? lo : T; r.hi = hi < T ? hi : T;
    if (r.lo == r.hi) { r.status = ZJ_RANGE_NOTHING; return; }
    if (slot < r.hi - r.lo) { r.status = ZJ_E_DSTSIZE_TOO_SMALL; return; }
    u64 const eF = zj_index_bisect(v.U, f0, f1, u0, r.lo), eL = zj_index_bisect(v.U, f0, f1, u0, r.hi - 1);
    r.status = ZJ_E_CORRUPTION;
    if (eL < eF || eL - eF >= 0xFFFFFFFFull) return;
    u64 const uF0 = v.U[eF], uF1 = v.U[eF + 1], uL0 = v.U[eL], uL1 = v.U[eL + 1];
    if (uF0 < u0 || uF1 < uF0 || uL0 < uF0 || uL1 < uL0 || (eL != eF && uL0 < uF1)) return;
    r.preF = uF0 - u0; r.fcsF = uF1 - uF0; r.preL = uL0 - u0; r.fcsL = uL1 - uL0;
    if (r.preF > r.lo || r.preF + r.fcsF <= r.lo || r.preL >= r.hi || r.preL + r.fcsL < r.hi) return;      // (the entries found do not hold the two bytes)
    r.posF = zj_index_rel(v.C[eF], c0, 0, ext); r.endF = zj_index_rel(v.C[eF + 1], c0, r.posF, ext);
    if (eL == eF) { r.posL = r.posF; r.endL = r.endF; }
    else { r.posL = zj_index_rel(v.C[eL], c0, r.endF, ext); r.endL = zj_index_rel(v.C[eL + 1], c0, r.posL, ext); }
    u32 const frames = (u32)(eL - eF) + 1u;
    bool const edgeF = r.preF < r.lo, edgeL = r.preL + r.fcsL > r.hi;
    u32 const edges = frames == 1u ? (u32)(edgeF || edgeL) : ((u32)edgeF | ((u32)edgeL << 1));
    if (((edges & 1u) && r.fcsF > ZJNI_RANGE_EDGE_MAX) || ((edges & 2u) && r.fcsL > ZJNI_RANGE_EDGE_MAX)) { r.status = 64u; return; }
    r.status = ZJ_RANGE_SELECTED; r.frames = frames; r.edges = edges;
    u64 const runLo = (edges & 1u) ? r.endF : r.posF, runHi = (edges & 2u) ? r.posL : r.endL;
    ir.e0 = eF + (edges & 1u); ir.cBase = c0; ir.uBase = u0; ir.srcLo = sLo;
    q[0] = (u64)(frames - zj_range_edge_count(edges)) + 1u;
    q[1] = zj_range_edge_count(edges);
    q[2] = runHi - runLo;
    q[3] = ((edges & 1u) ? r.endF - r.posF : 0) + ((edges & 2u) ? r.endL - r.posL : 0);
    q[4] = ((edges & 1u) ? r.fcsF : 0) + ((edges & 2u) ? r.fcsL : 0);
}

// ---- set A, one lane per entry ----
ZJ_HD u64 zj_index_run_lo(const ZRRec& r) { return (r.edges & 1u) ? r.endF : r.posF; }
ZJ_HD u64 zj_index_run_hi(const ZRRec& r) { return (r.edges & 2u) ? r.posL : r.endL; }
// interior entry j of a selected request (index entry ir.e0 + j): its two sums of each kind ascend and lie inside the request's interior run and clamped range
ZJ_HD bool zj_index_entry_ok(const u64* C, const u64* U, const ZRRec& r, const ZIReq& ir, u64 j) {
    u64 const e = ir.e0 + j, c0 = C[e], c1 = C[e + 1], u0 = U[e], u1 = U[e + 1];
    if (c0 < ir.cBase || c1 < c0 || u0 < ir.uBase || u1 < u0) return false;
    return c0 - ir.cBase >= zj_index_run_lo(r) && c1 - ir.cBase <= zj_index_run_hi(r) && u0 - ir.uBase >= r.lo && u1 - ir.uBase <= r.hi;
}
// entry j of the request's m + 1 entries of set A (j == m: the closing entry): its source in the compact bytes, which begin at a0 for the request, and its
// destination in the slot at dlo.  A request that is not selected has its one entry empty at the slot's first byte; one that an entry marked (bad) has every slot empty there.
ZJ_HD void zj_index_entry(const u64* C, const u64* U, const ZRRec& r, const ZIReq& ir, bool bad, u64 j, u64 a0, u64 dlo, u64* src, u64* dst) {
    *src = a0; *dst = dlo;
    if (r.status != ZJ_RANGE_SELECTED) return;
    u64 const runLo = zj_index_run_lo(r), runHi = zj_index_run_hi(r), want = r.hi - r.lo;
    // (the run's bytes are gathered all the same and the next request's begin behind them: the request's own last interior entry holds them, with a slot of no byte;
    //  its closing entry and the one of the request before it stay without a source byte)
    if (bad) { if (j >= r.frames - zj_range_edge_count(r.edges)) *src = a0 + (runHi - runLo); return; }
    u64 const e = ir.e0 + j;
    u64 const at = zj_index_rel(C[e], ir.cBase, runLo, runHi), done = zj_index_rel(U[e], ir.uBase, r.lo, r.hi) - r.lo;
    *src = a0 + (at - runLo);
    *dst = dlo + (done < want ? done : want);
}
// what a selected entry's decode answers for the request: its error, 20 when it decoded to another size than the index says, else 0
ZJ_HD u64 zj_index_verdict(u64 res, u64 content) { return res > ((u64)1 << 40) ? res : (res != content ? ZJ_ERR64(ZJ_E_CORRUPTION) : 0); }
