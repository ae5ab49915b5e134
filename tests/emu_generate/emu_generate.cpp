// tests/emu_generate/emu_generate.cpp — lane-serial (W = 1) build of zstd-jni_amd/csrc/zj_generate.h: the export of the match finders' records
// as ZSTD_Sequence[] (zg_export_block) and the parse-then-export frame loop (zg_generate_frame), as zj_generate_kernel
// calls them.  TEST INFRASTRUCTURE ONLY: never
// linked into libzjni_amd.so.
#include "../../zstd-jni_amd/csrc/zj_generate.h"
#include <stdlib.h>
#include <string.h>

// A workgroup's uniforms, LDS, scratch and tables outlive a frame and nothing clears them: one poisoned set per process, so that a frame
// which relies on what the previous one left fails here.
struct EmuGenWg { ZEncShared* sh; u8* lds; u8* ws; u32* tables; };
static EmuGenWg& emu_gen_wg() {
    static EmuGenWg wg = { nullptr, nullptr, nullptr, nullptr };
    if (!wg.sh) {
        wg.sh = (ZEncShared*)malloc(sizeof(ZEncShared)); memset(wg.sh, 0xA5, sizeof(ZEncShared));
        wg.lds = (u8*)malloc(160 * 1024); memset(wg.lds, 0x5A, 160 * 1024);
        wg.ws = (u8*)malloc(ZE_SCRATCH_BYTES); memset(wg.ws, 0xC3, ZE_SCRATCH_BYTES);
        wg.tables = (u32*)malloc(ZE_MULTI_TABLE_BYTES); memset(wg.tables, 0x3C, ZE_MULTI_TABLE_BYTES);
    }
    return wg;
}

#define EMU_GUARD 4u               /* slots of canary in front of and behind the caller's */
#define EMU_TOUCHED 0xFFFFFFFFFFFF0001ull
struct EmuSlots {
    ZSSeq* block; u64 cap;
    explicit EmuSlots(u64 c) : cap(c) { block = (ZSSeq*)malloc((size_t)(cap + 2u * EMU_GUARD) * 16); memset(block, 0xEE, (size_t)(cap + 2u * EMU_GUARD) * 16); }
    ZSSeq* slots() { return block + EMU_GUARD; }
    bool intact() const {
        const u8* const b = (const u8*)block;
        for (size_t i = 0; i < EMU_GUARD * 16; i++) if (b[i] != 0xEE || b[(size_t)(cap + EMU_GUARD) * 16 + i] != 0xEE) return false;
        return true;
    }
    ~EmuSlots() { free(block); }
};

extern "C" unsigned emu_generate_level_word(int level) { return zg_level_word(level); }
extern "C" unsigned emu_generate_refusal(int level, unsigned long long srcSize) { return zg_refusal(zg_level_word(level), srcSize); }

// One frame.  route 0: the wave route (zg_generate_frame), the only one.  The source is an exact-size heap copy, the slots exactly `cap` between canaries.  Returns the entries written, 2^64 - code,
// or EMU_TOUCHED when something outside the slots was written.
extern "C" unsigned long long emu_generate(const unsigned char* src, unsigned srcSize, int level, unsigned* out, unsigned long long cap, int route) {
    Grp<1> g;
    EmuGenWg& wg = emu_gen_wg();
    u32 const lw = zg_level_word(level);
    u8* const s = (u8*)malloc(srcSize ? srcSize : 1); if (srcSize) memcpy(s, src, srcSize);
    EmuSlots q(cap);
    u64 r;
    if (route == 0) r = zg_generate_frame(g, *wg.sh, wg.lds, s, srcSize, q.slots(), cap, lw, wg.ws, wg.tables);
    else r = ZJ_ERR64(ZJ_E_GENERIC);
    if (!q.intact()) r = EMU_TOUCHED;
    else if (r <= cap && r) memcpy(out, q.slots(), (size_t)r * 16);
    free(s);
    return r;
}

// The export alone on records the caller wrote: rec = {ll, ml, offBase, pos} x n, a block-start history, `cap` slots.
extern "C" unsigned long long emu_export_records(const unsigned* rec, unsigned n, unsigned lastLL, unsigned r0, unsigned r1, unsigned r2, unsigned* out, unsigned long long cap) {
    Grp<1> g;
    ZESeq* const rc = (ZESeq*)malloc(n ? (size_t)n * 16 : 1); if (n) memcpy(rc, rec, (size_t)n * 16);
    EmuSlots q(cap);
    u64 r = (u64)n + 1u;
    if (r > cap) r = ZJ_ERR64(ZJ_E_DSTSIZE_TOO_SMALL);
    else zg_export_block(g, rc, n, lastLL, r0, r1, r2, q.slots());
    if (!q.intact()) r = EMU_TOUCHED;
    else if (r <= cap) memcpy(out, q.slots(), (size_t)r * 16);
    free(rc);
    return r;
}

extern "C" unsigned long long emu_merge_block_delimiters(unsigned* seqs, unsigned long long n) { return zg_merge_block_delimiters((ZSSeq*)seqs, (size_t)n); }
