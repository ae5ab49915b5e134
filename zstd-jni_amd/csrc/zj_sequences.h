// zj_sequences.h — frames from sequences the CALLER found: ZSTD_compressSequences with explicit block delimiters
// (N/compress/zstd_compress.c:6599-6731 validation and transfer, :6895-7061 block loop, :7063-7110 frame), for batches.
//
// Two steps, a kernel each (zj_kernels.hip):
//   zs_convert         one wave per frame walks the frame's ZSTD_Sequence[] in tiles of a wave: a prefix sum of litLength + matchLength
//                      places every sequence in the source, a ballot finds the delimiters, lanes validate and write the ZESeq records
//                      and literal offsets the entropy stage reads (ZEPre), and every delimiter's lane writes its block's entry.
//   zs_compress_frame  a workgroup per frame runs the reference's block loop over the block entries: ze_compress_t(pre, ba) per
//                      block with the previous compressed block's Huffman table as repeat candidate, raw / RLE / compressed headers,
//                      the frame header in front and the checksum behind.
//
// Slot layout.  Frame i with sequences [q0, q1) of the call owns slots [q0 + i, q1 + i + 1) of two parallel arrays, `rec` (ZESeq, 16
// bytes) and `lit` (u32): slot 0 of the frame is a header slot, sequence r sits in slot r + 1.  A match's slot holds its record
// {litLength, matchLength, offBase, literal start in the block} and its literal offset in the block — without code bytes: the entropy
// stage's gather fills them in, as it does for the match finders' records.  A DELIMITER's slot (and the header slot) holds the entry
// of the block that STARTS behind it: rec = {nbSeq, litSize, lastLL, start in the source} (the first three are ZEPre::meta),
// lit = block size | ZS_BAD | ZS_SOFT.  So a block's records are contiguous behind its entry, and the next entry is nbSeq + 1 slots on.
// 20 bytes of scratch per sequence, 4 per frame (the number of delimiters).
//
// Offsets are never dereferenced: the entropy stage reads literals only.  That is what makes the reference's own leniency safe to
// restate — it accepts an offset that reaches up to matchLength bytes in front of the source (the bound is the position BEHIND the
// sequence, :6683-6684) and writes a frame no decoder accepts; so does this.  Nothing here reads outside [seqs, seqs + nSeqs) or the
// source whatever the array holds: every length is checked against its block before a literal is touched.
//
// Served: levels whose (level, srcSize) row ze_params_of has, sources to ZE_MULTI_MAX that fit the row's window (201 otherwise).
// Strategies from lazy upward (the rows of level 5 to 16 KiB and of levels 6-8) choose the sequence tables' modes by estimated cost with the previous
// block's tables as a candidate (zstd_compress_sequences.c:196-222), which the entropy stage does not carry: their frames are served
// while the first block is the last one, a second block answers 201.
//
// ---- ZSTD_sf_noBlockDelimiters (ZJNI_SEQ_NO_DELIMITERS) ----
// The array has no delimiters and the library cuts the blocks: ZSTD_transferSequences_noDelim (:6744-6868) under determine_blockSize
// (:6918-6927) and the block loop (:6969-7057).  zs_convert_nodelim is that rule for one frame, a wave:
//   prefix   tiles of a wave give every sequence its end in the uncut stream, P[i] (4 bytes a sequence of scratch).  A length counts as at most
//            ZS_ND_LEN_CAP and positions saturate at ZS_POS_CAP, both beyond any served source, so every P below a block edge is exact.  The pass stops
//            with the tile that reaches the end of the source: sequences behind it are never read (nor does the reference read them).
//   cut      the one serial chain, a step a BLOCK.  A block aims at T = min(128 KiB, remaining) and lastBlock = (T == remaining) is taken before
//            the transfer may shorten it (:6972-6975).  With the block starting `sp` bytes into sequence idx at source position `at`, the edge is
//            E = at + T and J the first sequence with P[J] >= E (bisection).  P[J] == E: J ends the block.  No J: the sequences ran out, the rest are
//            last literals (:6775).  Else the edge lies in J: in its literals (:6826-6829) the block ends at E; in its match (:6799-6825) the match is
//            split if matchLength > T and the first half >= cParams.minMatch (the row's own, not the validator's 3 / 4), the edge moving back if the
//            second half would be under minMatch — otherwise the block is shortened to end in front of the match.
//   emit     lanes over the block's sequences write records, literal offsets and the block entry in the slot layout above; the first sequence is
//            trimmed by `sp`, a split last one stored as its first half (the second opens the next block with litLength 0).  Every lane validates
//            its STORED sequence with the position behind it (:6837-6844).  Records leave with the raw offBase and ZS_SOFT: repcodes are always
//            searched in this mode (:6762-6763, :6831-6835), so the frame loop runs zs_resolve_block whatever the flag word says.  offset == 0 is
//            no delimiter here but offBase 3, as in the reference, which accepts it and writes an undecodable frame.
// Three corners of the reference, restated or fenced:
//   * a last block under 7 bytes that the transfer shortened is written raw WITH the last-block bit and the loop goes on (:6989-6998 `continue`s
//     past :7047): the frame holds blocks behind its "last" one.  So does this.
//   * a block that starts AT a match with fewer than minMatch bytes of source left consumes nothing (bytesAdjustment == blockSize): the reference
//     writes empty raw blocks until the destination is full and answers dstSize_tooSmall.  ZS_STUCK: the frame loop answers that at once.
//   * litLength + matchLength beyond 32 bits, and a block that starts INSIDE a match with fewer than minMatch bytes left (iend < istart), are
//     undefined in the reference; a frame that reaches either answers 107.
// Blocks per frame.  A block without the last-block bit is full (T bytes, or T less an adjustment under minMatch <= 7) or was shortened because a
// match M straddles its edge E.  The block behind a shortened one starts at M, and M's first half there is its whole target >= minMatch, so that
// block is not shortened at M: it holds all of M (and ends behind E) or is full.  Two consecutive blocks without the bit therefore cover more
// than 128 KiB - 7 bytes: at most 2 * (srcSize / 131066) + 1 of them, which is <= (srcSize >> 16) + 2 up to ZE_MULTI_MAX.  Blocks WITH the bit
// behind the first such (the first corner) are each under 7 bytes and followed by a split, a stuck or an undefined block: a handful.
// zs_nd_max_blocks = (srcSize >> 16) + 8; a block brings one entry slot and at most one record more than the array has (the second half of a
// split), so frame i owns cnt + 2 * zs_nd_max_blocks slots from zs_nd_slot_base.  Every slot index is checked against that slice regardless, and
// a frame that would leave it answers 107.
#pragma once
#include "zj_encode.h"

struct ZSSeq { u32 offset, litLength, matchLength, rep; };           // == ZSTD_Sequence == zjni_sequence
#define ZS_FLAG_REPCODES 8u        /* ZSTD_c_searchForExternalRepcodes = ZSTD_ps_enable (ZJNI_SEQ_REPCODES) */
#define ZS_E_SEQUENCES 107u        /* ZSTD_error_externalSequences_invalid */
#define ZS_BAD 0x80000000u         /* block entry: a sequence of the block, its delimiter or its size is invalid whatever the repcode history */
#define ZS_SOFT 0x40000000u        /* block entry / record.pos: the raw offset is beyond the bound — invalid unless the repcode walk turns it into a repcode */
#define ZS_LEN_CAP (1u << 18)      /* a length above a block's size is counted as this much: the block is invalid either way */
#define ZS_POS_CAP (1u << 30)      /* running positions saturate here, far beyond any served source */
#define ZS_NO_FRAME 0xFFFFFFFFu    /* per-frame delimiter count: the frame's slice of the sequence array is not one */
#define ZS_FLAG_NODELIM 16u        /* ZSTD_c_blockDelimiters = ZSTD_sf_noBlockDelimiters (ZJNI_SEQ_NO_DELIMITERS) */
#define ZS_LAST 0x10000000u        /* no-delimiter block entry: lastBlock of :6975, taken before the transfer shortened the block */
#define ZS_STUCK 0x20000000u       /* no-delimiter block entry: the transfer consumed nothing and never will (header) */
#define ZS_ND_LEN_CAP (1u << 24)   /* no-delimiter prefix: a sequence counts as at most this much, eight times ZE_MULTI_MAX; a tile's sum stays below 2^31 */

// the group of the sequence entries: ze_compress_t's own instantiation, with ZSTD_compressSequences' RLE rule (ZEExtSeq)
template <int W_> struct GrpSeq : Grp<W_> {};
template <int W_> struct ZEExtSeq<GrpSeq<W_> > { static constexpr bool v = true; };

ZJ_HD u64 zs_sequence_bound(u64 srcSize) { return srcSize / 3u + 1u + srcSize / 1024u + 1u; }      // ZSTD_sequenceBound (:3514-3518)

// the level word of a caller's level (zj_encode.h: ZE_LW_NEG carries a negative level's acceleration, clamped as ZSTD_minCLevel() clamps it); 0 means 3
ZJ_HD u32 zs_level_word(int level) { return level == 0 ? 3u : (level < 0 ? ZE_LW_NEGATIVE((u32)(level < -131072 ? 131072 : -level)) : (u32)level); }
// what the conversion needs of the row: the match-length floor (:6614) and ZSTD_maxNbSeq (:1697) of the block size ZSTD_resetCCtx_internal
// derives from the pledged size, min(128 KiB, window, max(1, srcSize))
ZJ_HD u32 zs_ml_min(const ZEParams& p) { return p.minMatch == 3u ? 3u : 4u; }
ZJ_HD u32 zs_max_nbseq(const ZEParams& p, u32 srcSize) {
    u64 w = (u64)1 << p.windowLog; if (w > srcSize) w = srcSize; if (w < 1u) w = 1u; if (w > ZE_BLOCK_MAX) w = ZE_BLOCK_MAX;
    return (u32)w / (p.minMatch == 3u ? 3u : 4u);
}

// inclusive scan over the wave, in registers; lane k's value in lane j (k differs per lane)
template <class G>
ZJ_DEV u32 zs_scan_incl(const G& g, u32 v) {
#if ZJ_ON_GPU
    u32 const l = g.lane();
#pragma unroll
    for (int d = 1; d < G::W; d <<= 1) { u32 const t = __shfl_up(v, d, G::W); if ((int)l >= d) v += t; }
#else
    (void)g;
#endif
    return v;
}
template <class G>
ZJ_DEV u32 zs_shfl(const G& g, u32 v, u32 k) {
#if ZJ_ON_GPU
    (void)g; return (u32)__shfl((int)v, (int)k, G::W);
#else
    (void)g; (void)k; return v;
#endif
}
ZJ_HD u64 zs_bits_to(u32 j) { return j >= 63u ? ~(u64)0 : (((u64)2 << j) - 1u); }                  // bits 0..j

// One frame's ZSTD_Sequence[cnt] -> records, literal offsets and block entries in the frame's slots (rec / lit point at its header
// slot).  mlMin: 3 when the row's minMatch is 3, else 4 (:6614); maxNbSeq: ZSTD_maxNbSeq of the frame's block size (:1697, :6690).
// Without `repcodes` nothing is serial but the carry between tiles: offBase = offset + 3 (:6674).  With it the records still leave
// here with the raw offBase — which repcode an offset is depends on the history, and the history on which earlier blocks the entropy
// stage emitted compressed (:7031-7037) — and the frame loop's walk finishes them (zs_resolve_block); an offset beyond its bound is
// then only marked (ZS_SOFT), since a repcode passes the check (:6615) whatever the raw offset was.
template <class G>
ZJ_DEV void zs_convert(const G& g, const ZSSeq* in, u32 cnt, u32 srcSize, u32 mlMin, u32 maxNbSeq, bool repcodes, ZESeq* rec, u32* lit, u32* nBlocksOut) {
    u32 pos = 0, litPos = 0;                     // source bytes / literals the sequences before this tile cover
    u32 bStart = 0, bLit = 0, bFirst = 0;        // the open block: where it starts in the source and in the literals, its first sequence
    bool bBad = false, bSoft = false;
    u32 nBlocks = 0;
    for (u32 t = 0; t < cnt; t += (u32)G::W) {
        u32 const j = g.lane(), idx = t + j;
        bool const in_ = idx < cnt;
        u32 off = 1, ll = 0, ml = 0;
        if (in_) { ZSSeq const s = in[idx]; off = s.offset; ll = s.litLength; ml = s.matchLength; }
        bool const big = ll > ZE_BLOCK_MAX || ml > ZE_BLOCK_MAX;
        u32 const len = big ? ZS_LEN_CAP : ll + ml, llc = zj_min(ll, ZS_LEN_CAP);
        u32 const eIn = zs_scan_incl(g, len), lIn = zs_scan_incl(g, llc);
        u32 const e = pos + eIn, L = litPos + lIn;                   // position / literal count BEHIND this sequence (posInSrc of :6683)
        bool const delim = in_ && off == 0;                          // :6904 — with a match length it is a format error (:6907), below
        u64 const dmask = grp_ballot(g, delim);
        u64 const below = j ? (dmask & zs_bits_to(j - 1u)) : 0;
        bool const fresh = below != 0;                               // this sequence's block starts inside the tile, behind lane p
        u32 const p = fresh ? 63u - (u32)__builtin_clzll(below) : 0u;
        u32 const eP = zs_shfl(g, e, p), lP = zs_shfl(g, L, p);
        u32 const bs = fresh ? eP : bStart, bl = fresh ? lP : bLit, bf = fresh ? t + p + 1u : bFirst;
        u32 const offBase = off + 3u;                                // OFFSET_TO_OFFBASE in 32 bits, as the reference computes it
        bool const offFail = in_ && !delim && (u64)offBase > (u64)e + 3u;          // :6615, the bound being posInSrc: the source fits its window, no dictionary
        bool const hard = in_ && (big || (delim ? ml != 0 : (ml < mlMin || offBase == 0u)) || (offFail && !repcodes));   // :6617, :6907
        bool const soft = offFail && repcodes;
        u64 const hmask = grp_ballot(g, hard), smask = grp_ballot(g, soft);
        if (in_ && !delim) {
            ZESeq r; r.ll = ll; r.ml = ml; r.off = offBase; r.pos = ((e - len - bs) & 0x3FFFFFFFu) | (soft ? ZS_SOFT : 0u);
            rec[idx + 1u] = r; lit[idx + 1u] = (L - llc) - bl;
        }
        if (delim) {                                                 // the entry of the block this delimiter closes, into the slot in front of its records
            u64 const range = zs_bits_to(j) & ~(fresh ? zs_bits_to(p) : 0);
            bool bad = (hmask & range) != 0 || (!fresh && bBad);
            bool const sft = (smask & range) != 0 || (!fresh && bSoft);
            u32 const size = e - bs, nb = idx - bf;
            if (size > ZE_BLOCK_MAX || e > srcSize || nb > maxNbSeq) bad = true;     // :6931, :6933, :6690
            ZESeq r; r.ll = nb; r.ml = L - bl; r.off = ll; r.pos = bs;
            rec[bf] = r; lit[bf] = zj_min(size, 0x0FFFFFFFu) | (bad ? ZS_BAD : 0u) | (sft ? ZS_SOFT : 0u);
        }
        // the carry: everything below is wave-uniform
        u32 const last = (u32)G::W - 1u;
        u32 const total = ZJ_UNI(zs_shfl(g, eIn, last)), totalL = ZJ_UNI(zs_shfl(g, lIn, last));
        if (dmask) {
            u32 const q = 63u - (u32)__builtin_clzll(dmask);
            bStart = ZJ_UNI(zs_shfl(g, e, q)); bLit = ZJ_UNI(zs_shfl(g, L, q)); bFirst = t + q + 1u;
            u64 const above = ~zs_bits_to(q);
            bBad = (hmask & above) != 0; bSoft = (smask & above) != 0;
            nBlocks += (u32)__builtin_popcountll(dmask);
        } else { bBad = bBad || hmask != 0; bSoft = bSoft || smask != 0; }
        pos = zj_min(pos + total, ZS_POS_CAP); litPos = zj_min(litPos + totalL, ZS_POS_CAP);
        bStart = zj_min(bStart, pos); bLit = zj_min(bLit, litPos);
    }
    GRP_SERIAL(g) { *nBlocksOut = nBlocks; }
}

// ---- no block delimiters (header) ----
ZJ_HD u32 zs_nd_max_blocks(u32 srcSize) { return (srcSize >> 16) + 8u; }
// frame i's first slot: its sequences' offset plus what the frames in front of it may add.  (s1 >> 16) - (s0 >> 16) >= (s1 - s0) >> 16, so
// consecutive slices do not overlap while the offsets ascend.
ZJ_HD u64 zs_nd_slot_base(u64 q0, u64 s0, u64 i) { return q0 + 2u * (s0 >> 16) + 16u * i; }
ZJ_HD u64 zs_nd_slots(u64 totalSeqs, u64 totalSrc, u64 n) { return totalSeqs + 2u * (totalSrc >> 16) + 16u * n; }

// One frame's ZSTD_Sequence[cnt] without delimiters -> records, literal offsets and block entries in the frame's `slots` slots.  minMatch: the row's
// cParams.minMatch (the split rule); mlMin, maxNbSeq as zs_convert.  pfx: cnt words of scratch.  *nBlocksOut: the entries written, or ZS_NO_FRAME
// when the frame left its budget of blocks or slots (107).
template <class G>
ZJ_DEV void zs_convert_nodelim(const G& g, const ZSSeq* in, u32 cnt, u32 srcSize, u32 mlMin, u32 minMatch, u32 maxNbSeq, u32* pfx, ZESeq* rec, u32* lit, u32 slots, u32* nBlocksOut) {
    u32 const lane = g.lane(), lastLane = (u32)G::W - 1u;
    // prefix: P[i], the end of sequence i in the uncut stream
    u32 lim = 0, wrapAt = 0xFFFFFFFFu;               // sequences placed; the first one whose lengths do not fit 32 bits
    {   u32 pos = 0;
        for (u32 t = 0; t < cnt && pos < srcSize; t += (u32)G::W) {
            u32 const idx = t + lane;
            bool const in_ = idx < cnt;
            u32 ll = 0, ml = 0;
            if (in_) { ZSSeq const s = in[idx]; ll = s.litLength; ml = s.matchLength; }
            u64 const sum = (u64)ll + ml;
            u32 const len = sum > ZS_ND_LEN_CAP ? ZS_ND_LEN_CAP : (u32)sum;
            u32 const eIn = zs_scan_incl(g, len);
            if (in_) pfx[idx] = zj_min(pos + eIn, ZS_POS_CAP);
            u64 const wmask = grp_ballot(g, in_ && sum > 0xFFFFFFFFull);
            if (wmask && wrapAt == 0xFFFFFFFFu) wrapAt = t + (u32)__builtin_ctzll(wmask);
            pos = zj_min(pos + ZJ_UNI(zs_shfl(g, eIn, lastLane)), ZS_POS_CAP);
            lim = zj_min(t + (u32)G::W, cnt);
        }
    }
    zj_mem_order();
    g.sync();
    // cut and emit, a block a step; everything but the record lanes is wave-uniform
    u32 const maxBlocks = zs_nd_max_blocks(srcSize);
    u32 idx = 0, sp = 0, at = 0, slot = 0, nBlocks = 0;
    while (at < srcSize) {
        if (nBlocks == maxBlocks) { nBlocks = ZS_NO_FRAME; break; }
        u32 const remaining = srcSize - at, T = zj_min((u32)ZE_BLOCK_MAX, remaining), E = at + T;
        u32 const lastBit = T == remaining ? 1u : 0u;
        u32 lo = idx, hi = lim;                      // J: the first sequence from idx on that ends at or behind the edge, lim if none does
        while (lo < hi) { u32 const mid = lo + ((hi - lo) >> 1); if (ZJ_UNI(pfx[mid]) >= E) hi = mid; else lo = mid + 1u; }
        u32 const J = lo;
        u32 endRec = lim, nextIdx = lim, nextSp = sp, size = T, splitLl = 0, splitMl = 0;
        bool split = false, bad = false, stuck = false;
        if (J < lim) {
            if (ZJ_UNI(pfx[J]) == E) { endRec = J + 1u; nextIdx = J + 1u; nextSp = 0; }      // :6783-6793, and endPosInSequence == 0 ends the loop (:6775)
            else {
                u32 const sll = ZJ_UNI(in[J].litLength), sml = ZJ_UNI(in[J].matchLength);
                u32 const A = J ? ZJ_UNI(pfx[J - 1u]) : 0u;                              // < E: exact
                u32 const spJ = J == idx ? sp : 0u;
                u32 endRel = E - A;                                                      // endPosInSequence
                endRec = J; nextIdx = J;
                if (endRel > sll) {                                                      // :6799
                    u32 const llT = spJ >= sll ? 0u : sll - spJ;
                    u32 firstHalf = endRel - spJ - llT;
                    if (sml > T && firstHalf >= minMatch) {                              // :6803
                        u32 const second = sml + sll - endRel;
                        if (second < minMatch) { u32 const adj = minMatch - second; endRel -= adj; firstHalf -= adj; size = T - adj; }
                        split = true; splitLl = llT; splitMl = firstHalf; endRec = J + 1u; nextSp = endRel;
                    } else if (spJ > sll) bad = true;                                    // iend < istart in the reference: undefined there (header)
                    else { size = A + sll - at; nextSp = sll; stuck = size == 0u; }     // :6822-6824
                } else nextSp = endRel;                                                  // :6826-6829
            }
        }
        u32 const nb = endRec - idx;
        if ((J < lim ? J : lim - 1u) >= wrapAt && lim) bad = true;                        // a sequence the reference's 32-bit arithmetic cannot hold was reached
        if ((u64)slot + 1u + nb > slots) { nBlocks = ZS_NO_FRAME; break; }
        u32 litCarry = 0; bool soft = false;
        for (u32 t = 0; t < nb; t += (u32)G::W) {
            u32 const k = t + lane, j = idx + k;
            bool const in_ = k < nb;
            u32 off = 1, ll = 0, ml = 0, start = at;
            if (in_) {
                ZSSeq const s = in[j]; off = s.offset; ll = s.litLength; ml = s.matchLength;
                if (j == idx) { if (sp >= ll) { ml -= sp - ll; ll = 0; } else ll -= sp; }            // :6784-6790
                else start = pfx[j - 1u];
                if (split && j == J) { ll = splitLl; ml = splitMl; }                                 // :6801, :6812
            }
            u32 const llc = zj_min(ll, ZS_ND_LEN_CAP);
            u32 const lIn = zs_scan_incl(g, llc);
            u32 const e = start + ll + ml;                                                           // posInSrc behind the stored sequence (:6838)
            u32 const offBase = off + 3u;
            bool const sft = in_ && (u64)offBase > (u64)e + 3u;                                      // :6615 — unless the walk makes it a repcode
            bool const hard = in_ && (ml < mlMin || offBase == 0u || k >= maxNbSeq);                 // :6617, :6844
            if (grp_ballot(g, hard)) bad = true;
            if (grp_ballot(g, sft)) soft = true;
            if (in_) {
                ZESeq r; r.ll = ll; r.ml = ml; r.off = offBase; r.pos = ((start - at) & 0x3FFFFFFFu) | (sft ? ZS_SOFT : 0u);
                rec[slot + 1u + k] = r; lit[slot + 1u + k] = litCarry + lIn - llc;
            }
            litCarry = zj_min(litCarry + ZJ_UNI(zs_shfl(g, lIn, lastLane)), ZS_POS_CAP);
        }
        // last literals: from the end of the last stored sequence to the block's end (:6857-6865)
        u32 const seqEnd = nb == 0u ? at : (split ? at + size : ZJ_UNI(pfx[endRec - 1u]));
        u32 const lastLL = at + size - seqEnd;
        GRP_SERIAL(g) {
            ZESeq r; r.ll = nb; r.ml = litCarry + lastLL; r.off = lastLL; r.pos = at;
            rec[slot] = r; lit[slot] = size | (lastBit ? ZS_LAST : 0u) | (stuck ? ZS_STUCK : 0u) | (bad ? ZS_BAD : 0u) | (soft ? ZS_SOFT : 0u);
        }
        nBlocks++; slot += nb + 1u; at += size; idx = nextIdx; sp = nextSp;
        if (bad || stuck || (lastBit && (size >= 7u || at == srcSize))) break;             // :7047 — a last block under 7 bytes does not end the loop (:6998)
    }
    GRP_SERIAL(g) { *nBlocksOut = nBlocks; }
}

// what the frame loop carries besides ZEncShared
struct ZSState { u32 rep[3], nextRep[3], fail; };

// ZSTD_c_searchForExternalRepcodes = enable: ZSTD_finalizeOffBase + ZSTD_updateRep per sequence (:6622-6636, :6676-6678,
// zstd_compress_internal.h:818-835), one lane as the reference's loop; the history starts from the last block that was emitted compressed.
ZJ_DEV void zs_resolve_block(ZSState& st, ZESeq* seqs, u32 nb) {
    u32 r0 = st.rep[0], r1 = st.rep[1], r2 = st.rep[2]; u32 fail = 0;
    for (u32 i = 0; i < nb; i++) {
        ZESeq s = seqs[i];
        u32 const raw = s.off - 3u, ll0 = s.ll == 0u ? 1u : 0u;
        u32 offBase = s.off;
        if (!ll0 && raw == r0) offBase = 1u;
        else if (raw == r1) offBase = 2u - ll0;
        else if (raw == r2) offBase = 3u - ll0;
        else if (ll0 && raw == r0 - 1u) offBase = 3u;
        if (offBase > 3u) { r2 = r1; r1 = r0; r0 = offBase - 3u; }
        else {
            u32 const repCode = offBase - 1u + ll0;
            if (repCode > 0u) { u32 const cur = repCode == 3u ? r0 - 1u : (repCode == 1u ? r1 : r2); if (repCode >= 2u) r2 = r1; r1 = r0; r0 = cur; }
        }
        if ((s.pos & ZS_SOFT) && offBase > 3u) { fail = 1; break; }                // "Offset too large!" (:6615): only a repcode is within every bound
        if (offBase == 0u) { fail = 1; break; }
        s.off = offBase; s.pos &= 0x3FFFFFFFu; seqs[i] = s;
    }
    st.nextRep[0] = r0; st.nextRep[1] = r1; st.nextRep[2] = r2; st.fail = fail;
}

// The frame: ZSTD_compressSequences (:7063-7110) around ZSTD_compressSequences_internal (:6944-7061).
// rec / lit: the frame's slots as zs_convert left them, nBlocks its delimiters.  Returns the frame's size or ZJ_ERR64(code).
// ND: the slots are zs_convert_nodelim's — the entry carries lastBlock, the frame ends on that bit even when bytes are left, and the repcode
// walk always runs.  A compile-time property: the explicit instantiation is the code it was.
template <class G, bool ND = false>
ZJ_DEV u64 zs_compress_frame(const G& g, ZEncShared& sh, ZSState& st, u8* lds, const u8* src, u32 srcSize, u8* dst, u32 dstCap, u32 level, u32 flags,
                             ZESeq* rec, const u32* lit, u32 nBlocks, u8* ws, ZjProf& pf, u32 ldsBytes) {
    ZEParams const p = ze_params_of(level, srcSize);                 // the level's row for the pledged size (ZSTD_CCtx_init_compressStream2 with ZSTD_e_end, :7074)
    if (p.strategy == 0u || srcSize > ZE_MULTI_MAX || (u64)srcSize > ((u64)1 << p.windowLog)) return ZJ_ERR64(201);
    if (nBlocks == ZS_NO_FRAME) return ZJ_ERR64(ZS_E_SEQUENCES);
    u32 const tail = (flags & ZE_FLAG_CHECKSUM) ? 4u : 0u;
    // ZSTD_writeFrameHeader (:4695-4745): content size, single segment (the source fits the window), no dictionary; ZSTD_FRAMEHEADERSIZE_MAX of room (:4711-4712)
    if (dstCap < 18u) return ZJ_ERR64(ZJ_E_DSTSIZE_TOO_SMALL);
    u32 const fcsCode = (srcSize >= 256u) + (srcSize >= 65536u + 256u);
    u32 const hdr = 5u + (fcsCode == 0u ? 1u : (fcsCode == 1u ? 2u : 4u));
    GRP_SERIAL(g) {
        st32(dst, 0xFD2FB528u); dst[4] = (u8)((1u << 5) + (fcsCode << 6) + (tail ? 4u : 0u));
        if (fcsCode == 0u) dst[5] = (u8)srcSize; else if (fcsCode == 1u) st16(dst + 5, srcSize - 256u); else st32(dst + 5, srcSize);
        // a fresh CCtx: no table to repeat, the repcodes of ZSTD_reset_compressedBlockState; `sh` outlives the frame, so all of it is set here
        sh.dictHufRep = ZC_REPEAT_NONE; sh.dictHufMaxSV = 0; sh.blkRep[0] = 1; sh.blkRep[1] = 4; sh.blkNextRep[0] = 1; sh.blkNextRep[1] = 4;
        st.rep[0] = 1; st.rep[1] = 4; st.rep[2] = 8; st.fail = 0;
    }
    zj_mem_order();
    g.sync();
    u32 pos = hdr;
    if (srcSize == 0u) {                                             // :6960-6967: the empty raw last block, written as four bytes
        if (dstCap - pos < 4u) return ZJ_ERR64(ZJ_E_DSTSIZE_TOO_SMALL);
        GRP_SERIAL(g) { dst[pos] = 1; dst[pos + 1] = 0; dst[pos + 2] = 0; }
        pos += 3u;
    }
    u32 at = 0, isFirst = 1, slot = 0; bool closed = srcSize == 0u;
    for (u32 k = 0; k < nBlocks && !closed; k++) {
        ZESeq const en = rec[slot];
        u32 const nb = ZJ_UNI(en.ll), word = ZJ_UNI(lit[slot]), size = word & 0x0FFFFFFFu;
        // determine_blockSize and the transfer's checks (:6929-6935, :6684-6695, :6728); a block in front of a bad one has been written by
        // now and could have run out of room first — the order the reference meets its errors in
        if (word & ZS_BAD) return ZJ_ERR64(ZS_E_SEQUENCES);
        if (ND && (word & ZS_STUCK)) return ZJ_ERR64(ZJ_E_DSTSIZE_TOO_SMALL);          // empty raw blocks until the destination is full (header)
        ZESeq* const seqs = rec + slot + 1u;
        if (ND || (flags & ZS_FLAG_REPCODES)) {
            GRP_SERIAL(g) { zs_resolve_block(st, seqs, nb); }
            zj_mem_order();
            g.sync();
            if (ZJ_UNI(st.fail)) return ZJ_ERR64(ZS_E_SEQUENCES);
        }
        u32 const lastBlock = ND ? ((word & ZS_LAST) ? 1u : 0u) : ((at + size == srcSize) ? 1u : 0u);      // :6975; sequences behind such a block are never looked at (:7047)
        u32 const room = dstCap - pos;
        if (size < 7u) {                                             // :6989: MIN_CBLOCK_SIZE + ZSTD_blockHeaderSize + 1 + 1 — raw, and the frame's "first block" stays open (the `continue` skips :7054)
            if (size + 3u > room) return ZJ_ERR64(ZJ_E_DSTSIZE_TOO_SMALL);           // ZSTD_noCompressBlock
            GRP_SERIAL(g) { u32 const bh = lastBlock + (size << 3); dst[pos] = (u8)bh; dst[pos + 1] = (u8)(bh >> 8); dst[pos + 2] = (u8)(bh >> 16); for (u32 q = 0; q < size; q++) dst[pos + 3u + q] = src[at + q]; }
            pos += 3u + size;
        } else {
            if (p.strategy >= 4u && !(isFirst && lastBlock)) return ZJ_ERR64(201);   // mode choice by cost against the previous block's tables: not carried (header)
            if (room < 3u) return ZJ_ERR64(ZJ_E_DSTSIZE_TOO_SMALL);                  // :7001
            ZEPre pre; pre.seqs = seqs; pre.litOff = lit + slot + 1u; pre.meta = &rec[slot].ll;
            ZEBlockArgs ba; ba.frameBase = src; ba.frameSize = srcSize; ba.paramSize = 0; ba.start = at; ba.isFirst = isFirst; ba.lastBlock = lastBlock; ba.tables = nullptr; ba.serialParse = 0;
            u64 const r = ze_compress_t<G, u32>(g, sh, lds, src + at, size, dst + pos, room, level, ws, pf, &pre, flags & ZE_FLAG_CHECKSUM, nullptr, ldsBytes, &ba);
            if (r > ZJ_ERR64(256)) return r;
            zj_mem_order();
            g.sync();
            // :7031-7037: only a block emitted compressed confirms its repcodes (and, inside ze_compress_t, its Huffman table).  The
            // offcode table's valid -> check step of :7035 needs a dictionary's table to be valid in the first place: there is none here.
            if ((ND || (flags & ZS_FLAG_REPCODES)) && ((ZJ_UNI((u32)dst[pos]) >> 1) & 3u) == 2u) {
                GRP_SERIAL(g) { st.rep[0] = st.nextRep[0]; st.rep[1] = st.nextRep[1]; st.rep[2] = st.nextRep[2]; }
                g.sync();
            }
            pos += (u32)r;
            if (!lastBlock) isFirst = 0;                             // :7054
        }
        at += size; slot += nb + 1u;
        if (ND ? (lastBlock && (size >= 7u || at == srcSize)) : lastBlock != 0u) closed = true;      // (ND: the raw path `continue`s past :7047)
    }
    if (!closed) return ZJ_ERR64(ZS_E_SEQUENCES);                    // :6913 / :6695: the source goes on and no delimiter is left
    if (tail) {
        if (dstCap - pos < 4u) return ZJ_ERR64(ZJ_E_DSTSIZE_TOO_SMALL);              // :7102
        u64 const h = zj_xxh64(g, src, srcSize);
        GRP_SERIAL(g) { st32(dst + pos, (u32)h); }
        pos += 4u;
    }
    zj_mem_order();
    g.sync();
    return pos;
}
