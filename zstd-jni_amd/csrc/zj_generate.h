// zj_generate.h — the matchers' parse OUT: ZSTD_generateSequences (N/compress/zstd_compress.c:3520-3553, ZSTD_copyBlockSequences :3429-3512)
// for batches.  The other half of the seam zj_sequences.h opened: there the caller's ZSTD_Sequence[] goes into the entropy stage, here
// the match finders' records come out as ZSTD_Sequence[] with explicit block delimiters.
//
// Two pieces, one kernel (zj_generate_kernel in zj_kernels.hip):
//   zg_export_block    one wave turns a block's ZESeq records {litLength, matchLength, offBase, literal start} into
//                      {raw offset, litLength, matchLength, rep} in tiles of a wave — 16 bytes in, 16 bytes out per lane — and writes the
//                      delimiter {0, lastLiterals, 0, 0} behind them.  What is serial is the repcode history (:3469-3492): a tile without a
//                      repcode (a ballot says so) takes its new history from its last three offsets; a tile with one is walked in scalar
//                      registers, every lane keeping the answer of its own step.
//   zg_generate_frame  one wave parses a frame block by block with the parse functions the compress entries run (the wave matcher and the
//                      one-lane parses over tables in HBM, ze_block_lazy for the chain and row finders) and exports every block from the
//                      workgroup's own record area.
//
// The reference's rules (collecting mode).  A block is min(128 KiB, what is left): ZSTD_compressBlock_internal returns 0 while collecting, every
// block is stored raw, `savings` never reaches 3 and ZSTD_optimalBlockSize never pre-splits (:4560-4569, :4651-4653).  EVERY block confirms its
// repcodes (:4408-4411) — in a compressed frame only a block emitted compressed does.  The history a block's walk starts from is the
// compressor's prevCBlock->rep: {rep0, rep1} as the match finder left them and a third entry that ZSTD_buildSeqStore copies from block to block
// unchanged, 8 since the frame's start.  A block under 7 bytes is "no compress" in ZSTD_buildSeqStore, which collecting turns into
// sequenceProducer_failed (106, :4402): sources of k x 128 KiB + 1 .. 6 bytes answer that, an empty source answers 0 sequences.  Capacity is
// checked per block, sequences plus delimiter, before anything of the block is written (:3445-3448): dstSize_tooSmall (70).
#pragma once
#include "zj_sequences.h"

#define ZG_E_PRODUCER 106u         /* ZSTD_error_sequenceProducer_failed */
#define ZG_MIN_BLOCK 7u            /* MIN_CBLOCK_SIZE + ZSTD_blockHeaderSize + 1 + 1 (ZSTD_buildSeqStore) */

// a caller's level as the kernels take it: zs_level_word, and at level 3 the reference's own table sizes (hashLog 16 / chainLog 15 before the
// adjustment to the size) — what zj_level3_word gives a compress call that set nothing
ZJ_HD u32 zg_level_word(int level) {
    u32 const w = zs_level_word(level);
    return (w == 3u) ? (ZE_LW(3u, 16u, 15u) | ZE_LW_IMPLICIT) : w;
}

// the (level word, size) pairs the entries serve — those of the compress entries without a dictionary — and the refusal of a last block under 7 bytes
ZJ_HD u32 zg_refusal(u32 levelWord, u64 srcSize) {
    if (srcSize == 0u) return 0u;
    if (srcSize > ZE_MULTI_MAX) return 201u;
    ZEParams const p = ze_params_of(levelWord, (u32)srcSize);
    if (p.strategy == 0u || srcSize > ((u64)1 << p.windowLog)) return 201u;
    u32 const last = (u32)srcSize - (((u32)srcSize - 1u) / ZE_BLOCK_MAX) * ZE_BLOCK_MAX;
    return last < ZG_MIN_BLOCK ? ZG_E_PRODUCER : 0u;
}

// One block's records -> out[0 .. nbSeq], the delimiter included.  r0..r2: the history at the block's start.  The caller has checked the capacity.
template <class G>
ZJ_DEV void zg_export_block(const G& g, const ZESeq* rec, u32 nbSeq, u32 lastLL, u32 r0, u32 r1, u32 r2, ZSSeq* out) {
    for (u32 t = 0; t < nbSeq; t += (u32)G::W) {
        u32 const j = g.lane(), idx = t + j;
        bool const in_ = idx < nbSeq;
        u32 const cnt = zj_min((u32)G::W, nbSeq - t);
        u32 ll = 1, ml = 0, ob = 4;
        if (in_) { ZESeq const s = rec[idx]; ll = ZE_LOW24(s.ll); ml = ZE_LOW24(s.ml); ob = ZE_LOW24(s.off); }
        u32 off = ob - 3u, rep = 0;
        u64 const repMask = grp_ballot(g, in_ && ob <= 3u);
        if (repMask == 0 && cnt >= 3u) {                              // no repcode in the tile: the history is its last three offsets
            r2 = grp_bcast(g, ob, cnt - 3u) - 3u; r1 = grp_bcast(g, ob, cnt - 2u) - 3u; r0 = grp_bcast(g, ob, cnt - 1u) - 3u;
        } else {
            for (u32 k = 0; k < cnt; k++) {                           // :3469-3492 and ZSTD_updateRep, wave-uniform
                u32 const obk = ZJ_UNI(grp_bcast(g, ob, k)), ll0 = ZJ_UNI(grp_bcast(g, ll, k)) == 0u ? 1u : 0u;
                u32 raw, code = 0;
                if (obk > 3u) { raw = obk - 3u; r2 = r1; r1 = r0; r0 = raw; }
                else {
                    code = obk;
                    u32 const rc = obk - 1u + ll0;                    // 0: rep[0] again; 3: rep[0] - 1
                    raw = rc == 0u ? r0 : (rc == 1u ? r1 : (rc == 2u ? r2 : r0 - 1u));
                    if (rc > 0u) { if (rc >= 2u) r2 = r1; r1 = r0; r0 = raw; }
                }
                if (j == k) { off = raw; rep = code; }
            }
        }
        if (in_) { ZSSeq q; q.offset = off; q.litLength = ll; q.matchLength = ml; q.rep = rep; out[idx] = q; }
    }
    GRP_SERIAL(g) { ZSSeq q; q.offset = 0; q.litLength = lastLL; q.matchLength = 0; q.rep = 0; out[nbSeq] = q; }
}

// One frame, parse and export (zj_generate_kernel).  `tables`: the workgroup's frame-wide tables in HBM (ZE_MULTI_TABLE_BYTES), `lds`: a ZXLds for
// the wave matcher, `ws`: the workgroup's scratch slot — records at ZE_WS_SEQ, literal offsets (which nothing here reads) at ZE_WS_BODY.
// Which function parses is what the compress entries choose for the (level word, size): double-fast on the whole wave (zx_block_dfast_wave;
// under 64 bytes of a single block the one-lane loop, as ze_compress_t), fast on one lane, greedy / lazy / lazy2 in ze_block_lazy.  A frame's
// blocks all take the same one: the wave matcher's table entries carry tags the one-lane loops do not.
// Returns the entries written or ZJ_ERR64(code).
template <class G>
ZJ_DEV u64 zg_generate_frame(const G& g, ZEncShared& sh, u8* lds, const u8* src, u32 srcSize, ZSSeq* out, u64 cap, u32 level, u8* ws, u32* tables) {
    {   u32 const e = zg_refusal(level, srcSize); if (e) return ZJ_ERR64(e); }
    if (srcSize == 0u) return 0;
    ZEParams const p = ze_params_of(level, srcSize);
    bool const rows = ze_params_uses_rows(p);
    u32 const entries = p.strategy >= 3u ? (rows ? (1u << p.hashLog) + (1u << p.hashLog) / 4u : (1u << p.hashLog) + (1u << p.chainLog))
                                         : (1u << p.hashLog) + (p.strategy == 2u ? (1u << p.chainLog) : 0u);
    GRP_FOR(g, i, entries) tables[i] = 0;
    GRP_SERIAL(g) { sh.blkRep[0] = 1; sh.blkRep[1] = 4; sh.blkNextRep[0] = 1; sh.blkNextRep[1] = 4; }
    zj_mem_order();
    g.sync();
    ZESeq* const seqs = (ZESeq*)(ws + ZE_WS_SEQ);
    bool const multi = srcSize > ZE_BLOCK_MAX;
    u64 written = 0;
    for (u32 at = 0; at < srcSize; at += ZE_BLOCK_MAX) {
        u32 const end = zj_min(srcSize, at + ZE_BLOCK_MAX);
        if (p.strategy == 2u && (multi || srcSize >= 64u)) {
            ZEOut o; o.seqs = seqs; o.litOff = (u32*)(ws + ZE_WS_BODY); o.n = 0; o.lit = 0;
            u32 const lastLL = zx_block_dfast_wave(lds, o, src, srcSize, at, end, p.hashLog, p.chainLog, p.minMatch, tables, tables + (1u << p.hashLog), sh.blkRep, sh.blkNextRep, true);
            GRP_SERIAL(g) { sh.nbSeq = o.n; sh.lastLL = lastLL; }
        } else GRP_SERIAL(g) {
            ZEOut o; o.seqs = seqs; o.litOff = (u32*)(ws + ZE_WS_BODY); o.n = 0; o.lit = 0;
            u32 lastLL;
            if (p.strategy >= 3u) lastLL = ze_block_lazy(o, src, srcSize, p, tables, tables + (1u << p.hashLog));       // (single block: zg_refusal)
            else if (p.strategy == 1u) lastLL = ze_block_fast_x<ZEEnt32>(o, src, at, end, p.hashLog, p.minMatch, tables, sh.blkRep, sh.blkNextRep, ze_fast_step(level));
            else lastLL = ze_block_dfast_x<ZEEnt32>(o, src, at, end, p.hashLog, p.chainLog, p.minMatch, tables, tables + (1u << p.hashLog), sh.blkRep, sh.blkNextRep);
            sh.nbSeq = o.n; sh.lastLL = lastLL;
        }
        zj_mem_order();
        g.sync();
        u32 const nbSeq = ZJ_UNI(sh.nbSeq), lastLL = ZJ_UNI(sh.lastLL);
        if ((u64)nbSeq + 1u > cap - written) return ZJ_ERR64(ZJ_E_DSTSIZE_TOO_SMALL);          // :3445-3448, per block
        zg_export_block(g, seqs, nbSeq, lastLL, ZJ_UNI(sh.blkRep[0]), ZJ_UNI(sh.blkRep[1]), 8u, out + written);
        written += (u64)nbSeq + 1u;
        g.sync();
        GRP_SERIAL(g) { sh.blkRep[0] = sh.blkNextRep[0]; sh.blkRep[1] = sh.blkNextRep[1]; }      // :4408-4411: every block confirms
        zj_mem_order();
        g.sync();
    }
    return written;
}

// ZSTD_mergeBlockDelimiters (:3555-3569): every delimiter's literals go to the next sequence, the delimiters go; host code
static inline size_t zg_merge_block_delimiters(ZSSeq* s, size_t n) {
    size_t in = 0, out = 0;
    for (; in < n; ++in) {
        if (s[in].offset == 0 && s[in].matchLength == 0) { if (in != n - 1) s[in + 1].litLength += s[in].litLength; }
        else { s[out] = s[in]; ++out; }
    }
    return out;
}
