// tests/emu_fast/emu_fast.cpp — lane-serial (W = 1) build of the encoder bodies at negative levels (zstd's --fast=N), for the CPU-side
// parity tests (tests/test_emu_negative_levels.py).  The entry takes the PUBLIC level, as the C-ABI does, and turns it into the level
// word the way compress_chunked (zj_kernels.hip) does, so the clamp and the word's layout (zj_encode.h: ZE_LW_NEG) are under test too.
// TEST INFRASTRUCTURE ONLY: never linked into libzjni_amd.so.
#include "../../zstd-jni_amd/csrc/zj_encode.h"
#include <stdlib.h>
#include <string.h>

static u32 emu_fast_word(int level) {
    if (level >= 0) return (u32)level;
    return ZE_LW_NEGATIVE((u32)(level < -131072 ? 131072 : -level));
}
// persistent, poisoned workgroup state (as tests/emu/emu.cpp keeps it): state leaking from one frame into the next shows up
struct EmuFastWg { ZEncShared* sh; u8* lds; u8* ws; };
static EmuFastWg& emu_fast_wg() {
    static EmuFastWg w = { nullptr, nullptr, nullptr };
    if (!w.sh) {
        w.sh = (ZEncShared*)malloc(sizeof(ZEncShared)); memset(w.sh, 0xA5, sizeof(ZEncShared));
        w.sh->dictLoaded = 0; w.sh->ctDict[0] = 0; w.sh->ctDict[1] = 0; w.sh->ctDict[2] = 0;
        w.lds = (u8*)malloc(160 * 1024); memset(w.lds, 0x5A, 160 * 1024);
        w.ws = (u8*)malloc(ZE_SCRATCH_BYTES); memset(w.ws, 0xC3, ZE_SCRATCH_BYTES);
    }
    return w;
}
extern "C" unsigned emu_fast_level_word(int level) { return emu_fast_word(level); }
extern "C" void emu_fast_params(int level, unsigned srcSize, unsigned* out) {
    ZEParams const p = ze_params_of(emu_fast_word(level), srcSize);
    out[0] = p.windowLog; out[1] = p.chainLog; out[2] = p.hashLog; out[3] = p.minMatch; out[4] = p.strategy; out[5] = p.targetLength; out[6] = ze_fast_step(emu_fast_word(level));
}
// route 0: the fused kernel's body (tables in LDS, one-lane parse); 1: lane-per-frame match finding (ZLaneF, records in scratch) then the
// entropy stage; frames above 128 KiB: the multi-block frame loop (zj_encode_multi_kernel's body, one-lane parse of each block).
// flags: ZE_FLAG_* frame flags (checksum, no content size).  Returns the frame size or ZJ_ERR64(code).
extern "C" unsigned long long emu_fast_compress(const unsigned char* src, unsigned srcSize, unsigned char* dst, unsigned dstCap, int level, unsigned flags, int route) {
    Grp<1> g;
    u32 const lw = emu_fast_word(level);
    EmuFastWg& wg = emu_fast_wg();
    ZjProf pf; pf.start(nullptr);
    flags &= ZE_FLAG_MASK;
    if (srcSize > ZE_BLOCK_MAX) {
        u32* tables = (u32*)malloc(ZE_MULTI_TABLE_BYTES); memset(tables, 0xA5, ZE_MULTI_TABLE_BYTES);
        u64 const r = ze_compress_multi(g, *wg.sh, wg.lds, src, srcSize, dst, dstCap, lw, wg.ws, pf, flags | ZE_FLAG_MULTI_FAST_SERIAL, tables, 160u * 1024u);
        free(tables);
        return r;
    }
    if (route == 0) return ze_compress(g, *wg.sh, wg.lds, src, srcSize, dst, dstCap, lw, wg.ws, pf, nullptr, flags);
    // the classification kernel's split: list B (4-byte positions, 2^15-entry tables) when level 1's tables would not fit the LDS of list A
    u32 const ldsA = 8192u * 2u;
    bool const wide = ze_lds_need(ZE_LW_LEVEL(lw), srcSize) > (ldsA > (u32)sizeof(ZEEntropy) ? ldsA : (u32)sizeof(ZEEntropy));
    u32 const maxSrc = wide ? ZE_WIDE_MAX_SRC : 65536u;
    u8* table = (u8*)calloc(1, ze_lane_table_stride(lw, wide));
    u8* fs = (u8*)malloc(ZE_FRAME_STRIDE(maxSrc));
    u32 meta[3];
    ze_match_lane(src, srcSize, lw, table, fs, maxSrc, meta, wide);
    ZEPre pre; pre.seqs = (ZESeq*)fs; pre.litOff = (const u32*)(fs + (size_t)ZE_FRAME_MAXSEQ(maxSrc) * 16u); pre.meta = meta;
    u64 const r = ze_compress(g, *wg.sh, wg.lds, src, srcSize, dst, dstCap, lw, wg.ws, pf, &pre, flags, nullptr, 160u * 1024u);
    free(fs); free(table);
    return r;
}
