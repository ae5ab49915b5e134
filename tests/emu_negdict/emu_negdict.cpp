// tests/emu_negdict/emu_negdict.cpp — lane-serial (W = 1) build of the dictionary and stream bodies at negative levels (zstd's --fast=N), for the CPU-side
// parity tests (tests/test_emu_negative_dict_stream.py).  The entries take the PUBLIC level, as the C-ABI does, and turn it into the level word the way
// zjni_createCDict / zjni_compress_stream_batch_device (zj_kernels.hip) do, so the clamp and the CDict's word are under test too.  Each entry runs what
// the GPU route runs: the digest of zj_cdict_digest_kernel_neg; the classification of zjni_compress_batch_device_usingCDict (one block at most), then the
// attach-mode search of zj_enc_match_dict_kernel_neg or the copy-mode body of zj_encode_cdict_copy_kernel_neg, then the entropy stage with the CDict's
// word; and zj_encode_stream_kernel's body with the stream's word.
// TEST INFRASTRUCTURE ONLY: never linked into libzjni_amd.so.
#include "../../zstd-jni_amd/csrc/zj_cdict.h"
#include <stdlib.h>
#include <string.h>

static u32 emu_nd_word(int level) {
    if (level == 0) level = 3;
    if (level > 0) return (u32)level;
    return ZE_LW_NEGATIVE((u32)(level < -131072 ? 131072 : -level));
}
// persistent, poisoned workgroup state (as tests/emu/emu.cpp keeps it): state leaking from one frame into the next shows up
struct EmuNdWg { ZEncShared* sh; u8* lds; u8* ws; };
static EmuNdWg& emu_nd_wg() {
    static EmuNdWg w = { nullptr, nullptr, nullptr };
    if (!w.sh) {
        w.sh = (ZEncShared*)malloc(sizeof(ZEncShared)); memset(w.sh, 0xA5, sizeof(ZEncShared));
        w.lds = (u8*)malloc(160 * 1024); memset(w.lds, 0x5A, 160 * 1024);
        w.ws = (u8*)malloc(ZE_SCRATCH_BYTES); memset(w.ws, 0xC3, ZE_SCRATCH_BYTES);
    }
    return w;
}
extern "C" unsigned emu_nd_level_word(int level) { return emu_nd_word(level); }

// ZSTD_createCDict at any level <= 3: NULL where zjni_createCDict answers NULL
extern "C" void* emu_nd_cdict_create(const unsigned char* dict, unsigned dictSize, int level) {
    if (dictSize < 8 || level > 3) return nullptr;
    u32 const lw = emu_nd_word(level);
    ZEParams const cp = ze_cdict_params_of(lw, dictSize);
    size_t const tablesBytes = (size_t)ze_cdict_table_entries(cp) * 4u;
    size_t const head = (sizeof(ZECDictDev) + 15) & ~(size_t)15;
    u8* buf = (u8*)calloc(1, head + tablesBytes + dictSize + 16);
    ZECDictDev* cd = (ZECDictDev*)buf;
    cd->tablesOff = (u32)head; cd->rawOff = (u32)(head + tablesBytes);
    memcpy(buf + cd->rawOff, dict, dictSize);
    Grp<1> g;
    ZDecShared* sh = (ZDecShared*)calloc(1, sizeof(ZDecShared));
    ZEEntropy* e = (ZEEntropy*)calloc(1, sizeof(ZEEntropy));
    ze_cdict_digest(g, *sh, *e, dictSize, lw, cd, cp);
    free(e); free(sh);
    if (cd->status) { free(buf); return nullptr; }
    return buf;
}
extern "C" void emu_nd_cdict_free(void* cd) { free(cd); }
// {dictID, contentSize, windowLog, chainLog, hashLog, minMatch, strategy, level word, attach step, copy step}
extern "C" void emu_nd_cdict_info(const void* p, unsigned* out) {
    const ZECDictDev* cd = (const ZECDictDev*)p;
    out[0] = cd->dictID; out[1] = cd->contentSize; out[2] = cd->windowLog; out[3] = cd->chainLog; out[4] = cd->hashLog; out[5] = cd->minMatch; out[6] = cd->strategy;
    out[7] = cd->level; out[8] = ze_dms_step(cd->level); out[9] = ze_fast_step(cd->level);
}
// One frame against the CDict, flags = ZE_FLAG_* (checksum, no dictID).  *route: 1 attach mode, 2 copy mode, 0 neither (refused).
// Returns the frame size or ZJ_ERR64(code).
extern "C" unsigned long long emu_nd_compress_cdict(const void* p, const unsigned char* src, unsigned srcSize, unsigned char* dst, unsigned dstCap, unsigned flags, int* route) {
    const ZECDictDev* cd = (const ZECDictDev*)p;
    bool const neg = (cd->level & ZE_LW_NEG) != 0u;
    *route = 0;
    if (srcSize > ZE_BLOCK_MAX) return ZJ_ERR64(201);                  // zj_enc_classify_kernel: more than one block
    Grp<1> g;
    EmuNdWg& wg = emu_nd_wg();
    u8* table = (u8*)calloc(1, ZC_TABLE_STRIDE);
    u8* fs = (u8*)malloc(ZE_FRAME_STRIDE(ZC_MAX_SRC));
    u32 meta[3] = {0, srcSize, srcSize};
    ZEPre pre; pre.seqs = (ZESeq*)fs; pre.litOff = (const u32*)(fs + (size_t)ZE_FRAME_MAXSEQ(ZC_MAX_SRC) * 16u); pre.meta = meta;
    u32* big = nullptr;
    if (srcSize <= ze_attach_cutoff(cd->strategy)) {
        ze_match_lane_dict(src, srcSize, cd, table, fs, ZC_MAX_SRC, meta, neg ? ze_dms_step(cd->level) : 1u);
        *route = 1;
    } else if (ze_cdict_copy_mode(cd->strategy, srcSize, cd->contentSize)) {
        big = (u32*)malloc(ZE_MULTI_TABLE_BYTES); memset(big, 0xA5, ZE_MULTI_TABLE_BYTES);
        ze_cdict_copy_tables(g, cd, big);
        ze_cdict_copy_parse(cd, src, srcSize, big, wg.ws, meta, neg ? ze_fast_step(cd->level) : 2u);
        pre.seqs = (ZESeq*)(wg.ws + ZE_WS_SEQ); pre.litOff = (const u32*)(wg.ws + ZE_WS_BODY); pre.copyMode = 1u;
        *route = 2;
    }
    // (the workgroup's dictionary uniforms are loaded once per kernel: a fresh kernel per frame here)
    wg.sh->dictLoaded = 0; wg.sh->ctDict[0] = 0; wg.sh->ctDict[1] = 0; wg.sh->ctDict[2] = 0;
    ZjProf pf; pf.start(nullptr);
    u64 const r = ze_compress(g, *wg.sh, wg.lds, src, srcSize, dst, dstCap, cd->level, wg.ws, pf, &pre, flags & ZE_FLAG_MASK, cd, 160u * 1024u);
    free(big); free(fs); free(table);
    return r;
}

// zjni_compress_stream's frame: level checked and turned into its word as the entry does, then zj_encode_stream_kernel's body with the entry's default
// flags (the one-lane block parses).  Returns the frame's bytes so far or ZJ_ERR64(code).
extern "C" unsigned long long emu_nd_compress_stream(const unsigned char* src, unsigned srcSize, unsigned char* dst, unsigned dstCap, int level, int checksum,
                                                    const unsigned* flushAt, unsigned nFlush, int final_, int knownEmpty) {
    if (level == 0) level = 3;
    if (level > 3) return ZJ_ERR64(42);
    if (srcSize > (1u << ze_stream_window_log(level < 0 ? 1u : (u32)level)) || srcSize > ZE_MULTI_MAX) return ZJ_ERR64(201);
    u32 const lw = emu_nd_word(level);
    Grp<1> g;
    EmuNdWg& wg = emu_nd_wg();
    wg.sh->dictLoaded = 0;
    u32* tables = (u32*)malloc(ZE_MULTI_TABLE_BYTES); memset(tables, 0xA5, ZE_MULTI_TABLE_BYTES);
    ZjProf pf; pf.start(nullptr);
    u32 const flags = (checksum ? ZE_FLAG_CHECKSUM : 0u) | ZE_FLAG_MULTI_FAST_SERIAL;
    u64 const r = ze_compress_stream(g, *wg.sh, wg.lds, src, srcSize, dst, dstCap, lw, wg.ws, pf, flags, tables, 160u * 1024u, flushAt, nFlush, final_ ? 1u : 0u, knownEmpty ? 1u : 0u);
    free(tables);
    return r;
}
