// tests/emu_sequences_nodelim/emu_sequences_nodelim.cpp — lane-serial (W = 1) build of the no-delimiter half of zstd-jni_amd/csrc/zj_sequences.h: the prefix, cut and
// emit passes (zs_convert_nodelim) and the frame loop's no-delimiter instantiation (zs_compress_frame<G, true>, which runs the entropy stage of zj_encode.h), as
// zj_seq_cut_kernel and zj_encode_sequences_nodelim_kernel call them.  TEST INFRASTRUCTURE ONLY: never linked into libzjni_amd.so.
#include "../../zstd-jni_amd/csrc/zj_sequences.h"
#include <stdlib.h>
#include <string.h>

// A workgroup's uniforms, LDS and scratch outlive a frame and nothing clears them: one poisoned set per process, so that a frame
// which relies on what the previous one left fails here.
struct EmuSeqWg { ZEncShared* sh; ZSState* st; u8* lds; u8* ws; };
static EmuSeqWg& emu_seq_wg() {
    static EmuSeqWg wg = { nullptr, nullptr, nullptr, nullptr };
    if (!wg.sh) {
        wg.sh = (ZEncShared*)malloc(sizeof(ZEncShared)); memset(wg.sh, 0xA5, sizeof(ZEncShared));
        wg.sh->dictLoaded = 0; wg.sh->ctDict[0] = 0; wg.sh->ctDict[1] = 0; wg.sh->ctDict[2] = 0;      // the kernel's prologue
        wg.st = (ZSState*)malloc(sizeof(ZSState)); memset(wg.st, 0xA5, sizeof(ZSState));
        wg.lds = (u8*)malloc(160 * 1024); memset(wg.lds, 0x5A, 160 * 1024);
        wg.ws = (u8*)malloc(ZE_SCRATCH_BYTES); memset(wg.ws, 0xC3, ZE_SCRATCH_BYTES);
    }
    return wg;
}

extern "C" unsigned emu_nodelim_max_blocks(unsigned srcSize) { return zs_nd_max_blocks(srcSize); }

// One frame.  Source, sequence array, prefix words and destination are exact-size heap copies, the slots exactly the frame's slice (nSeqs + 2 * zs_nd_max_blocks):
// a read or write outside any of them is one outside a heap block.  Returns the frame's size or 2^64 - code; blocksOut (may be null): the entries the cut wrote.
extern "C" unsigned long long emu_compress_sequences_nodelim(const unsigned char* src, unsigned srcSize, const unsigned* seqs, unsigned nSeqs,
                                                             unsigned char* dst, unsigned dstCap, int level, unsigned flags, unsigned* blocksOut) {
    GrpSeq<1> g;
    EmuSeqWg& wg = emu_seq_wg();
    u32 const lw = zs_level_word(level);
    ZEParams const p = ze_params_of(lw, srcSize);
    u8* const s = (u8*)malloc(srcSize ? srcSize : 1); if (srcSize) memcpy(s, src, srcSize);
    ZSSeq* const q = (ZSSeq*)malloc(nSeqs ? (size_t)nSeqs * 16 : 1); if (nSeqs) memcpy(q, seqs, (size_t)nSeqs * 16);
    u8* const d = (u8*)malloc(dstCap ? dstCap : 1); if (dstCap) memcpy(d, dst, dstCap);
    size_t const slots = (size_t)nSeqs + 2u * zs_nd_max_blocks(srcSize);
    ZESeq* const rec = (ZESeq*)malloc(slots * 16); memset(rec, 0xC3, slots * 16);
    u32* const lit = (u32*)malloc(slots * 4); memset(lit, 0xC3, slots * 4);
    u32* const pfx = (u32*)malloc(nSeqs ? (size_t)nSeqs * 4 : 1); memset(pfx, 0xC3, nSeqs ? (size_t)nSeqs * 4 : 1);
    u32 nBlocks = 0;                                 // (the kernel writes 0 for a row it does not serve and skips the conversion)
    if (p.strategy != 0u && srcSize <= ZE_MULTI_MAX)
        zs_convert_nodelim(g, q, nSeqs, srcSize, zs_ml_min(p), p.minMatch, zs_max_nbseq(p, srcSize), pfx, rec, lit, (u32)slots, &nBlocks);
    if (blocksOut) *blocksOut = nBlocks;
    ZjProf pf; pf.start(nullptr);
    u64 const r = srcSize > ZE_MULTI_MAX ? ZJ_ERR64(201)
                : zs_compress_frame<GrpSeq<1>, true>(g, *wg.sh, *wg.st, wg.lds, s, srcSize, d, dstCap, lw, flags & (ZE_FLAG_CHECKSUM | ZS_FLAG_REPCODES), rec, lit, nBlocks, wg.ws, pf, 160u * 1024u);
    if (dstCap) memcpy(dst, d, dstCap);
    free(s); free(q); free(d); free(rec); free(lit); free(pfx);
    return r;
}
