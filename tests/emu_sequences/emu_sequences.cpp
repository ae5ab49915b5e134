// tests/emu_sequences/emu_sequences.cpp — lane-serial (W = 1) build of zstd-jni_amd/csrc/zj_sequences.h: the conversion of a caller's
// ZSTD_Sequence[] (zs_convert) and the frame loop over its blocks (zs_compress_frame, which runs the entropy stage of zj_encode.h), as
// zj_seq_convert_kernel and zj_encode_sequences_kernel call them.  TEST INFRASTRUCTURE ONLY: never linked into libzjni_amd.so.
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

extern "C" unsigned long long emu_sequence_bound(unsigned long long srcSize) { return zs_sequence_bound(srcSize); }

// One frame.  Source, sequence array and destination are exact-size heap copies, the slots exactly nSeqs + 1: a read or write outside
// any of them is one outside a heap block.  Returns the frame's size or 2^64 - code.
extern "C" unsigned long long emu_compress_sequences(const unsigned char* src, unsigned srcSize, const unsigned* seqs, unsigned nSeqs,
                                                     unsigned char* dst, unsigned dstCap, int level, unsigned flags) {
    GrpSeq<1> g;
    EmuSeqWg& wg = emu_seq_wg();
    u8* const s = (u8*)malloc(srcSize ? srcSize : 1); if (srcSize) memcpy(s, src, srcSize);
    ZSSeq* const q = (ZSSeq*)malloc(nSeqs ? (size_t)nSeqs * 16 : 1); if (nSeqs) memcpy(q, seqs, (size_t)nSeqs * 16);
    u8* const d = (u8*)malloc(dstCap ? dstCap : 1); if (dstCap) memcpy(d, dst, dstCap);
    ZESeq* const rec = (ZESeq*)malloc(((size_t)nSeqs + 1) * 16); memset(rec, 0xC3, ((size_t)nSeqs + 1) * 16);
    u32* const lit = (u32*)malloc(((size_t)nSeqs + 1) * 4); memset(lit, 0xC3, ((size_t)nSeqs + 1) * 4);
    u32 const lw = zs_level_word(level);
    ZEParams const p = ze_params_of(lw, srcSize);
    u32 nBlocks = 0xC3C3C3C3u;
    zs_convert(g, q, nSeqs, srcSize, zs_ml_min(p), zs_max_nbseq(p, srcSize), (flags & ZS_FLAG_REPCODES) != 0, rec, lit, &nBlocks);
    ZjProf pf; pf.start(nullptr);
    u64 const r = zs_compress_frame(g, *wg.sh, *wg.st, wg.lds, s, srcSize, d, dstCap, lw, flags & (ZE_FLAG_CHECKSUM | ZS_FLAG_REPCODES), rec, lit, nBlocks, wg.ws, pf, 160u * 1024u);
    if (dstCap) memcpy(dst, d, dstCap);
    free(s); free(q); free(d); free(rec); free(lit);
    return r;
}

// The frame loop's answer for a slot the conversion kernel marked ZS_NO_FRAME (the frame's pair of sequence offsets descends): no slot is read.
extern "C" unsigned long long emu_compress_no_frame(const unsigned char* src, unsigned srcSize, unsigned char* dst, unsigned dstCap, int level, unsigned flags) {
    GrpSeq<1> g;
    EmuSeqWg& wg = emu_seq_wg();
    u8* const s = (u8*)malloc(srcSize ? srcSize : 1); if (srcSize) memcpy(s, src, srcSize);
    u8* const d = (u8*)malloc(dstCap ? dstCap : 1);
    ZjProf pf; pf.start(nullptr);
    u64 const r = zs_compress_frame(g, *wg.sh, *wg.st, wg.lds, s, srcSize, d, dstCap, zs_level_word(level), flags & (ZE_FLAG_CHECKSUM | ZS_FLAG_REPCODES), (ZESeq*)nullptr, (const u32*)nullptr, ZS_NO_FRAME, wg.ws, pf, 160u * 1024u);
    free(s); free(d);
    return r;
}
