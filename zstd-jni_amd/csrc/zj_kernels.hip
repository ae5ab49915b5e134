// zj_kernels.hip — gfx950 kernels + the C-ABI of include/zjni_amd.h (libzjni_amd.so).
//
// Launch shape: persistent workgroups of ONE wavefront (64 lanes); each pulls frame indices from a
// device-scope atomic counter (frames differ 4x in cost), so the grid is
// (#CUs x resident workgroups/CU), not the batch size.  Block b lands on XCD b % 8; frames are
// independent, so no cross-XCD traffic exists and the per-XCD L2s only see their own frames.
#include <hip/hip_runtime.h>
#include <mutex>
#include <algorithm>
#include <thread>
#include <sched.h>
#include <atomic>
#include <condition_variable>
#include <chrono>
#include <map>
#include <string>
#include <system_error>
#include <memory>
#include <vector>
#include <initializer_list>
#include <string.h>
#include <stdio.h>
#include <stdlib.h>
#include "../../include/zjni_amd.h"
#include "zj_decode.h"
#include "zj_decode_split.h"
#include "zj_encode.h"
#include "zj_cdict.h"
#ifndef ZW_FRAME_IN_LDS
#define ZW_FRAME_IN_LDS 0
#endif
#include "zj_match_wave.h"
#include "zj_synth.h"
#include "zj_frameinfo.h"
#include "zj_frames.h"
#include "zj_frames_range.h"
#include "zj_index.h"
#include "zj_sequences.h"
#include "zj_generate.h"

#define ZJNI_ERR(code) ((size_t)0 - (size_t)(code))

// A/B and debug switches (ZJNI_*): read from the environment ONCE per process and kept — getenv() races with setenv() from other JVM threads, and the
// per-buffer natives would otherwise pay ~30 lookups per call.  ZJNI_DEBUG_LIVE_SWITCHES=1 (set before the library loads; tests/conftest.py does) keeps
// them live so a test can flip a switch between two calls.
static const char* zj_env(const char* name) {
    static bool const live = []() { const char* v = getenv("ZJNI_DEBUG_LIVE_SWITCHES"); return v && atoi(v) == 1; }();
    if (live) return getenv(name);
    static std::mutex m; static std::map<std::string, std::pair<bool, std::string> > cache;     // (map nodes never move: the returned pointers stay valid)
    std::lock_guard<std::mutex> g(m);
    auto it = cache.find(name);
    if (it == cache.end()) { const char* v = getenv(name); it = cache.emplace(name, std::make_pair(v != nullptr, std::string(v ? v : ""))).first; }
    return it->second.first ? it->second.second.c_str() : nullptr;
}

// Experiment knobs (grid sizes, losing routes kept for A/B runs, measurement hooks) exist in a TUNING build only — tools/build_variant.sh <name> -DZJ_TUNING_KERNELS,
// its stamp ends in "+tuning" — and read as unset in the product, which keeps ten documented switches: ZJNI_SPLIT_MIN, ZJNI_DSPLIT_MIN,
// ZJNI_L3_WAVE_MAX, ZJNI_NEED, ZJNI_DEC_LIT, ZJNI_DEC_MB, ZJNI_WIDE_SLICE, ZJNI_HOST_THREADS, ZJNI_HOST_TRACE, ZJNI_DEBUG_SYNC (+ ZJNI_DEBUG_LIVE_SWITCHES above).
#ifdef ZJ_TUNING_KERNELS
static const char* zj_tune(const char* name) { return zj_env(name); }
#else
static constexpr const char* zj_tune(const char*) { return nullptr; }
#endif

// ============================================================================ kernels ==========
// Next work item of a persistent workgroup: one device-scope atomic by lane 0, broadcast through
// v_readfirstlane so the index (and everything derived from it) is wave-uniform.
__device__ __forceinline__ u32 zj_next_index(u32* counter) {
    u32 v = 0;
    if (threadIdx.x == 0) v = atomicAdd(counter, 1u);
    return (u32)__builtin_amdgcn_readfirstlane((int)v);
}

// Fused wave-per-frame decoder: frame i of the batch, or (list != nullptr) the frames a list names.
// DICT = true is the ZSTD_decompress_usingDDict variant (a second kernel, so that the common one keeps its registers).
template <bool DICT>
__global__ __launch_bounds__(64, 4) void zj_decode_kernel_t(const u8* __restrict__ src, const u64* __restrict__ srcOff,
                                                        u8* __restrict__ dst, const u64* __restrict__ dstOff,
                                                        u64* __restrict__ result, u32 n, u32* counter, u8* scratch, unsigned long long* prof,
                                                        const u32* __restrict__ list, const u32* listCount,
                                                        const ZDDictDev* dd, const u8* dictRaw) {
    __shared__ ZDecShared sh;
    ZjProf pf; pf.start(prof);
    Grp<64> g;
    u8* const lit = scratch + (size_t)blockIdx.x * ZD_LIT_SCRATCH;
    u32 const count = list ? ZJ_UNI(*listCount) : n;
    for (;;) {
        u32 const k = zj_next_index(counter);      // wave-uniform (SGPR)
        if (k >= count) break;
        u32 const i = list ? ZJ_UNI(list[k]) : k;
        u64 const s0 = srcOff[i], s1 = srcOff[i + 1], d0 = dstOff[i], d1 = dstOff[i + 1];
        u64 const cap = d1 - d0, len = s1 - s0;
        u64 const r = len > 0xFFFFFFFFull ? ZJ_ERR64(ZJ_E_SRCSIZE_WRONG)      // sizes are 32-bit inside the decoder: no silent truncation
                    : zd_decompress<DICT>(g, sh, src + s0, (u32)len, dst + d0, (u32)(cap > 0xFFFFFFFFull ? 0xFFFFFFFFull : cap), lit, pf, dd, dictRaw);
        pf.mark(8);
        if (threadIdx.x == 0) result[i] = r;
        __syncthreads();
    }
}

extern __shared__ __attribute__((aligned(16))) u8 zj_dyn_lds[];

#define zj_decode_kernel zj_decode_kernel_t<false>
#define zj_dec_prep_kernel zj_dec_prep_kernel_t<false>
#define zj_dec_exec_kernel zj_dec_exec_kernel_t<false>
#define zj_decode_dict_kernel zj_decode_kernel_t<true>

// ZSTD_createDDict on the device: one workgroup digests the raw dictionary at dictRaw into *out
__global__ __launch_bounds__(64) void zj_ddict_digest_kernel(const u8* dictRaw, u32 dictSize, ZDDictDev* out) {
    __shared__ ZDecShared sh;
    Grp<64> g;
    zd_ddict_digest(g, sh, dictRaw, dictSize, out);
}

// ---- split decode pipeline (zj_decode_split.h): prep -> lane-per-frame sequence decode -> execute ----
// append k to a completion queue (the producer's records are visible before the entry): match kernel -> entropy kernel, sequence decode -> execution
__device__ __forceinline__ void zj_publish_done(u32* doneList, u32* doneCount, u32 k) {
    if (!doneList) return;
    zj_release();                                          // records + meta visible before the queue entry
    u32 const slot = atomicAdd(doneCount, 1u);
    __hip_atomic_store(&doneList[slot], k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// the queue entry alone, behind a release fence the caller has made for several lanes at once (zj_match_run)
__device__ __forceinline__ void zj_queue_done(u32* doneList, u32* doneCount, u32 k) {
    u32 const slot = atomicAdd(doneCount, 1u);
    __hip_atomic_store(&doneList[slot], k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
#ifndef ZJ_HAND_ROUNDS
#define ZJ_HAND_ROUNDS 256u      /* rounds between a match wave's hand-overs to the entropy kernel (a power of two; 32: -5 %, 256: -7 %, 2048: -2 % of the level-3 match kernel against a fence per frame, profiles/r05/f_) */
#endif
// Multi-block frames (zj_decode_split.h, "multi-block frames"): what stage 1 claims from — mb.ctr[0] blocks, [1] entries of seqList, [2] entries of listM, [4..5] records of the pool (64 bit)
struct ZDMbArgs { ZDFrameMB* frames; ZDBlk* blks; u16* tabs; u32* ctr; u32 blkCap; u32 minBlocks; unsigned long long seqCap; u32* seqList; u32* listM; unsigned long long litCap; u32* litList; };      // ctr: ... [8] lit list, [10..11] literal pool bytes (64 bit), [12] work of the literal pass
template <bool DICT>
__global__ __launch_bounds__(64, 4) void zj_dec_prep_kernel_t(const u8* __restrict__ src, const u64* __restrict__ srcOff, const u64* __restrict__ dstOff,
                                                          u32 n, u32* counter, u16* tabs, ZDMeta* metas, u32* listA, u32* listB, u32* listCounts,
                                                          const ZDDictDev* dd, u32* doneList, u32* procFlag, ZDMbArgs mb, u32 mbOnly, u8* __restrict__ dst, u64* __restrict__ result) {
    __shared__ ZDecShared sh;
    Grp<64> g;
    for (;;) {
        u32 const i = zj_next_index(counter);
        if (i >= n) break;
        u64 const s0 = srcOff[i], s1 = srcOff[i + 1], d0 = dstOff[i], d1 = dstOff[i + 1];
        u64 const cap = d1 - d0;
        bool const simple = !mbOnly && zd_prep_frame<DICT>(g, sh, src + s0, (u32)(s1 - s0), (u32)(cap > 0xFFFFFFFFull ? 0xFFFFFFFFull : cap),
                                                           tabs + (size_t)i * ZD_SPLIT_CELLS, metas + i, dd);
        bool multi = false, stored = false;
        if (!DICT && !simple && dst && s1 - s0 <= 0xFFFFFFFFull) stored = zd_prep_frame_stored(g, sh, src + s0, (u32)(s1 - s0), dst + d0, cap, result + i);      // one raw / RLE block: copied here ([11] counts them)
        if (!DICT && !simple && !stored && mb.frames && s1 - s0 <= 0xFFFFFFFFull) {
            // (minBlocks: a small batch keeps its single-block frames on the fused kernel — one launch instead of three)
            multi = zd_prep_frame_multi(g, sh, src + s0, (u32)(s1 - s0), cap, i, mb.frames + i, mb.blks, mb.tabs, mb.ctr, mb.blkCap, (unsigned long long*)(mb.ctr + 4), mb.seqCap, mb.seqList, mb.ctr + 1, mb.minBlocks,
                                        (unsigned long long*)(mb.ctr + 10), mb.litCap, mb.litList, mb.ctr + 8);
        }
        if (threadIdx.x == 0) {
            if (doneList) { doneList[i] = 0xFFFFFFFFu; procFlag[i] = 0; }       // slot i of the completion queue / frame i's "executed by the side pass" flag
            // |A| and the batch's sequence total share one 64-bit counter ([8] = |A|, [9] = sequences, see zj_dec_heavy): one same-address atomic per frame
            if (simple) listA[(u32)atomicAdd((unsigned long long*)&listCounts[8], 1ull | ((unsigned long long)sh.nbSeq << 32))] = i;
            else if (stored) atomicAdd(&listCounts[11], 1u);
            else if (multi) mb.listM[atomicAdd(mb.ctr + 2, 1u)] = i;
            else listB[atomicAdd(&listCounts[1], 1u)] = i;
        }
        __syncthreads();
    }
}
// Multi-block frames, stage 2b: a WAVE per block regenerates its Huffman-coded literals into the block's slot of the literal pool (zd_lit_block)
__global__ __launch_bounds__(64) void zj_dec_lit_mb_kernel(const u8* __restrict__ src, const u64* __restrict__ srcOff, const u32* __restrict__ litList, const u32* countPtr, u32* workCounter,
                                                            ZDBlk* blks, u8* litPool) {
    ZDecShared& sh = *(ZDecShared*)zj_dyn_lds;          // allocated without the tANS tables, the windows of zd_huf_streams_wave behind it (ZD_EXEC_LDS)
    ZjProf pf; pf.start(nullptr);
    Grp<64> g;
    u32 const count = ZJ_UNI(*countPtr);
    for (;;) {
        u32 const k = zj_next_index(workCounter);
        if (k >= count) break;
        u32 const b = ZJ_UNI(litList[k]);
        bool const ok = zd_lit_block(g, sh, src + zj_uni64(srcOff[ZJ_UNI(blks[b].frame)]), blks, b, litPool, pf, (u8*)zj_dyn_lds + ZD_HP_LDS_OFF);
        if (threadIdx.x == 0 && ok) blks[b].litReady = 1u;
        __syncthreads();
    }
}
// Multi-block frames, stage 2: a LANE per block (ZDSeqLaneT<true>: repcode history carried symbolically), records into the pool
__global__ __launch_bounds__(64) void zj_dec_seq_mb_kernel(const u8* __restrict__ src, const u64* __restrict__ srcOff, const u32* __restrict__ seqList, const u32* countPtr, u32* workCounter,
                                                            const u16* tabs, u64* pool, ZDBlk* blks, u32 beside) {
    __shared__ u32 llBase[36], mlBase[53];
    zd_seq_symtabs(llBase, mlBase, threadIdx.x, 64u);
    __syncthreads();
    if (beside) __builtin_amdgcn_s_setprio(3);              // the chain of rounds is the critical path; stage 3's waves beside it (waiting for blocks, executing them) fill the gaps
    u32 const count = *countPtr;
    ZDSeqLaneT<true> m; m.st = 2; m.llBase = llBase; m.mlBase = mlBase;
    for (;;) {
        if (m.st == 2) {
            u32 const k = atomicAdd(workCounter, 1u);
            if (k >= count) break;
            u32 const b = seqList[k];
            ZDBlk* const bk = blks + b;
            m.init_block(src + srcOff[bk->frame], tabs + (size_t)b * ZD_SPLIT_CELLS, pool + (((u64)bk->seqHi << 32) | bk->seqLo), bk);
            continue;
        }
        m.round();
    }
}
// Multi-block frames, stage 3: a wave per frame walks its blocks in order (zd_exec_frame_multi); what it hands over goes to list B (the fused kernel)
__global__ __launch_bounds__(64) void zj_dec_exec_mb_kernel(const u8* __restrict__ src, const u64* __restrict__ srcOff, u8* __restrict__ dst, const u64* __restrict__ dstOff, u64* __restrict__ result,
                                                             const u32* __restrict__ listM, const u32* countPtr, u32* workCounter, const ZDFrameMB* frames, const ZDBlk* blks, const u64* pool,
                                                             u8* scratch, u32* listB, u32* listBCount, const u8* litPool, u32 mode, u32* procFlag) {
    // mode 0: list entry k.  mode 1: the same BESIDE stage 2 — a frame's blocks are executed in order, each as soon as stage 2 has set its seqReady (bounded wait; a
    // frame given up on is left to the mode-2 pass).  mode 2: the list entries mode 1 did not finish.
    __shared__ ZDecShared sh;
    ZjProf pf; pf.start(nullptr);
    Grp<64> g;
    u8* const lit = scratch + (size_t)blockIdx.x * ZD_LIT_SCRATCH;
    u32 const count = ZJ_UNI(*countPtr);
    for (;;) {
        u32 const k = zj_next_index(workCounter);
        if (k >= count) break;
        u32 const i = ZJ_UNI(listM[k]);
        if (mode == 2u && ZJ_UNI(procFlag[i])) continue;
        u64 const s0 = zj_uni64(srcOff[i]), d0 = zj_uni64(dstOff[i]), d1 = zj_uni64(dstOff[i + 1]);
        u64 const r = zd_exec_frame_multi(g, sh, src + s0, dst + d0, d1 - d0, frames + i, blks, pool, lit, (u8*)sh.ll, pf, litPool, mode == 1u);      // (sh.ll .. sh.ml: 4 KiB of LDS this kernel has no tANS tables in)
        if (threadIdx.x == 0 && r != ~(u64)0 - 1u) { if (r == ~(u64)0) listB[atomicAdd(listBCount, 1u)] = i; else result[i] = r; if (mode == 1u) procFlag[i] = 1u; }
        __syncthreads();
    }
}
// The sequence decode and the execution kernel run BESIDE each other when the frames carry enough sequences for the chain of
// decode rounds to dominate (>= 512 per frame on average: 64 KiB buffers have ~2 500, 4 KiB records ~100); for light frames the
// per-frame start-up dominates, every wave slot goes to the sequence decode and the execution kernel follows it.
__device__ __forceinline__ bool zj_dec_heavy(const u32* countA) { return countA[1] >= 512u * countA[0]; }      // countA = &listCounts[8]


__global__ __launch_bounds__(64) void zj_dec_seq_kernel(const u8* __restrict__ src, const u64* __restrict__ srcOff, const u32* __restrict__ list,
                                                         const u32* countPtr, u32* workCounter, const u16* tabs, u64* seqs, ZDMeta* metas,
                                                         const ZDDictDev* dd, u32* doneList, u32* doneCount, u32 heavyWaves) {
    if (doneList && !zj_dec_heavy(countPtr)) doneList = nullptr;
    if (doneList && blockIdx.x >= heavyWaves) return;        // fewer resident waves = fewer decode cells alive at a time (2.5 KiB per lane); a lane takes more frames instead
    __shared__ u32 llBase[36], mlBase[53];
    zd_seq_symtabs(llBase, mlBase, threadIdx.x, 64u);
    __syncthreads();
#ifndef ZD_SEQ_PRIO
#define ZD_SEQ_PRIO 3
#endif
    if (doneList) __builtin_amdgcn_s_setprio(ZD_SEQ_PRIO);   // the chain of rounds is the critical path; the execution kernel's waves beside it fill the gaps
    u32 const count = *countPtr;
    ZDSeqLane m; m.st = 2; m.llBase = llBase; m.mlBase = mlBase;
    u32 cur = 0xFFFFFFFFu;                                   // the frame this lane is decoding
    for (;;) {
        if (m.st == 2) {
            if (cur != 0xFFFFFFFFu) { zj_publish_done(doneList, doneCount, cur); cur = 0xFFFFFFFFu; }   // the execution kernel runs beside this one and takes frames as they finish
            u32 const k = atomicAdd(workCounter, 1u);
            if (k >= count) break;
            u32 const i = list[k];
            m.init(src + srcOff[i], tabs + (size_t)i * ZD_SPLIT_CELLS, seqs + (size_t)i * ZD_SPLIT_MAXSEQ, metas + i, dd);
            cur = i;
            continue;
        }
        m.round();
    }
}

// Stage 2b: the Huffman-coded literals of list A's frames into their slots (zd_lit_frame), beside the sequence decode and ahead of the execution pass on the same side
// stream.  A kernel of its own since round 6 (it was the execution kernel's mode 3): the four streams are decoded by the whole wave (zd_huf_streams_wave), whose
// windows take ZD_HP_LDS bytes of LDS behind the workgroup state — the execution kernel keeps its registers and its workgroups per CU.
__global__ __launch_bounds__(64) void zj_dec_lit_kernel(const u8* __restrict__ src, const u64* __restrict__ srcOff, const u32* __restrict__ list, const u32* countPtr,
                                                         u32* workCounter, ZDMeta* metas, u8* litSlots, u32 litSlot, unsigned long long* prof) {
    ZDecShared& sh = *(ZDecShared*)zj_dyn_lds;          // allocated without the tANS tables, the windows behind it (ZD_EXEC_LDS)
    ZjProf pf; pf.start(prof);
    Grp<64> g;
    u32 const count = ZJ_UNI(*countPtr);
    for (;;) {
        u32 const k = zj_next_index(workCounter);
        if (k >= count) break;
        u32 const i = ZJ_UNI(list[k]);
        bool const ok = zd_lit_frame(g, sh, src + srcOff[i], metas + i, litSlots + (size_t)i * litSlot, litSlot, pf, (u8*)zj_dyn_lds + ZD_HP_LDS_OFF);
        if (threadIdx.x == 0 && ok) metas[i].pad = 1u;      // the frame record says where the execution stage finds the literals
        __syncthreads();
    }
}

template <bool DICT>
__global__ __launch_bounds__(64) void zj_dec_exec_kernel_t(const u8* __restrict__ src, const u64* __restrict__ srcOff, u8* __restrict__ dst,
                                                          const u64* __restrict__ dstOff, u64* __restrict__ result, const u32* __restrict__ list,
                                                          const u32* countPtr, u32* workCounter, ZDMeta* metas, const u64* seqs, u8* scratch,
                                                          u32* listB, u32* listBCount, unsigned long long* prof, const ZDDictDev* dd, const u8* dictRaw,
                                                          u32 mode, const u32* doneList, u32* procFlag, u8* litSlots, u32 litSlot, u32* processed) {      // (metas: written by mode 3 only — the literal pass marks the frames it served; processed: frames mode 1 executed)
    // mode 0: list entry k.  mode 1: the k-th frame the sequence-decode kernel finishes while this kernel runs beside it (bounded
    // wait; a workgroup that gives up leaves the rest to the mode-2 pass).  mode 2: list entries mode 1 did not get to.
    // litSlots: slot i holds frame i's literals when its record says so (zj_dec_lit_kernel, beside the sequence decode).
    ZDecShared& sh = *(ZDecShared*)zj_dyn_lds;          // allocated without the tANS tables (ZD_SHARED_NO_FSE)
    ZjProf pf; pf.start(prof);
    Grp<64> g;
    u8* const lit = scratch + (size_t)blockIdx.x * ZD_LIT_SCRATCH;
    u32 const count = ZJ_UNI(*countPtr);
    if (mode == 1 && !zj_dec_heavy(countPtr)) return;        // light frames: everything is the mode-2 pass's
    if (mode == 2 && processed && ZJ_UNI(*processed) == count) return;      // the pass beside the sequence decode took every frame (round 6: walking the list to find that out was 0.7 ms)
    for (;;) {
        u32 const k = zj_next_index(workCounter);
        if (k >= count) break;
        u32 i;
        if (mode == 1) {
            u32 v = 0xFFFFFFFFu;
            if (threadIdx.x == 0) {
                u64 const t0 = wall_clock64();            // 100 MHz
                for (;;) {
                    v = __hip_atomic_load(&doneList[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // relaxed poll, fence below (see zj_encode_kernel)
                    if (v != 0xFFFFFFFFu || wall_clock64() - t0 > 200000000ull) break;     // 2 s
                    __builtin_amdgcn_s_sleep(127); __builtin_amdgcn_s_sleep(127);
                }
            }
            v = (u32)__builtin_amdgcn_readfirstlane((int)v);
            if (v == 0xFFFFFFFFu) break;
            zj_acquire();
            i = v;
        } else {
            i = ZJ_UNI(list[k]);
            if (mode == 2 && ZJ_UNI(procFlag[i])) continue;
        }
        u64 const r = zd_exec_frame<DICT>(g, sh, src + srcOff[i], dst + dstOff[i], metas + i, seqs + (size_t)i * ZD_SPLIT_MAXSEQ, lit, pf, dd, dictRaw,
                                          litSlots ? litSlots + (size_t)i * litSlot : (const u8*)nullptr, litSlot);
        pf.mark(8);
        if (threadIdx.x == 0) { if (r == ~(u64)0) listB[atomicAdd(listBCount, 1u)] = i; else result[i] = r; if (mode == 1) { procFlag[i] = 1u; if (processed) atomicAdd(processed, 1u); } }
        __syncthreads();
    }
}

// Encoder: dynamic LDS = the match-finder tables of the launch's (level, size class); the entropy stage
// overlays them.  A classification kernel splits the batch into two index lists: frames whose tables
// fit the LDS of the common case (list A) and the few that need more (list B; e.g. level-1 inputs of
// 8-16 KiB use hashLog 15, inputs > 64 KiB use 4-byte positions).  The same persistent kernel then runs
// once per list — with 128 KiB of LDS for list B, exiting at once when that list is empty.

__global__ __launch_bounds__(256) void zj_enc_classify_kernel(const u64* __restrict__ srcOff, u64* __restrict__ result, u32 n, u32 level,
                                                               u32 ldsA, u32* counters, u32* listA, u32* listB, u32* listC) {
    u32 const i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    u64 const size = srcOff[i + 1] - srcOff[i];
    if (ZE_LW_LEVEL(level) >= 4u) {                   // levels 4-8: frames <= 16 KiB -> list A here = the lane-per-frame chain parsers (zj_enc_match_chain_kernel);
        if (size <= (16u << 10)) listA[atomicAdd(&counters[0], 1u)] = i;                      // up to 128 KiB -> list C (level 4: double-fast, levels 5-8: the row-based finder;
        else if (listC && size <= ZE_BLOCK_MAX) listC[atomicAdd(&counters[4], 1u)] = i;       //   tables in HBM, one lane parses);
        else result[i] = ZJ_ERR64(201);                                                        // larger inputs: multi-block frames of these strategies are not served
        return;
    }
    if (size > ZE_BLOCK_MAX) {                        // multi-block frames (list C, zj_encode_multi_kernel) up to ZE_MULTI_MAX, without explicit table sizes
        if (listC && size <= ZE_MULTI_MAX && (!(ZE_LW_HL(level) | ZE_LW_CL(level)) || (level & ZE_LW_IMPLICIT))) { listC[atomicAdd(&counters[4], 1u)] = i; atomicAdd(&counters[6], 1u); }      // ([6]: the multi-block frames among list C — zj_pipe_route)
        else result[i] = ZJ_ERR64(201);
        return;
    }
    if (listC && (level & ZE_LW_WAVE_ROUTE)) { listC[atomicAdd(&counters[4], 1u)] = i; return; }      // a small level-3 batch: every frame its own wave (zj_match_wavex.h)
    bool const a = ZE_LW_TUNED(level) ? (size <= 65536u)                            // table sizes beyond the LDS: lane pipeline only, split by record width
                                                         : (ze_lds_need(ZE_LW_LEVEL(level), (u32)size) <= ldsA);
    if (a) listA[atomicAdd(&counters[0], 1u)] = i;
    else listB[atomicAdd(&counters[1], 1u)] = i;
}

// Lane-per-frame match finding (large batches): every lane owns one frame and runs the reference's
// sequential parse as a round-synchronous state machine (zj_match_lane.h); a lane whose frame is finished
// pulls the next list entry from a device counter inside the same loop, so the 64 lanes of a wave keep
// sharing memory round trips although frames differ 30x in cost.  Tables and sequence records of list
// entry k live at tables + k*tableStride and fscratch + k*ZE_FRAME_STRIDE(maxSrc) in HBM.
// Completion queue between the match kernel and the entropy kernel running beside it: a lane that has
// finished frame k (records and meta written) appends k; entropy workgroups consume the queue in order, so
// the cheap frames are entropy-coded while the expensive ones are still being parsed.
// Work queue over a list sorted by search density (zj_enc_score_kernel), cut at `split` (the first entry whose score reaches
// the threshold).  Entries [split, count) are the wave-per-frame kernel's alone (a lane would sit on such a frame for ~70 000
// rounds); it takes them from the back with its own counter.  Entries [0, split) are a two-ended queue: the lane-per-frame
// kernel claims from the front, the wave kernel — once its own part is done — from the back, and they meet wherever their
// speeds put them.  One 64-bit counter holds both cursors of that part (front low, back high), so every claim sees a
// consistent pair and exactly `split` claims succeed; a failed claim means the part is exhausted for good.
// Layout at work2: [0] u64 cursor pair, [2] u32 split, [3] u32 cursor of the wave kernel's own part.
__device__ __forceinline__ bool zj_claim_front(unsigned long long* work2, u32& k) {
    u32 const split = ((const u32*)work2)[2];
    unsigned long long const old = atomicAdd(work2, 1ull);
    u32 const head = (u32)old, tail = (u32)(old >> 32);
    k = head;
    return (u64)head + tail < split;
}
__device__ __forceinline__ bool zj_claim_back(unsigned long long* work2, u32 count, u32& k) {
    u32 const split = ((const u32*)work2)[2];
    u32 const t = atomicAdd(&((u32*)work2)[3], 1u);
    if (t < count - split) { k = count - 1u - t; return true; }
    unsigned long long const old = atomicAdd(work2, 1ull << 32);
    u32 const head = (u32)old, tail = (u32)(old >> 32);
    k = split - 1u - tail;
    return (u64)head + tail < split;
}

#ifdef ZL_PROFILE
__device__ unsigned long long zlWaveProf[4 * 2048];      // per workgroup of the last large match launch: cycles in the round loop, XCC_ID << 32 | HW_ID, rounds of lane 0, wall clock (100 MHz) at its start
extern "C" int zjni_debug_wave_profile(unsigned long long* out) { return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(zlWaveProf), sizeof(zlWaveProf)); }
__device__ u32 zlFrameRounds[131072];                    // per frame of the last large match launch: the round in which its lane finished it (the launch's active lanes over time, profiles/r05/)
extern "C" int zjni_debug_frame_rounds(unsigned* out) { return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(zlFrameRounds), sizeof(zlFrameRounds)); }
#endif
template <class M>
__device__ __forceinline__ void zj_match_run(const u8* __restrict__ src, const u64* __restrict__ srcOff, u32 level,
                                             const u32* __restrict__ list, u32 count, u32* workCounter,
                                             u8* tables, u32 tableStride, u8* fscratch, u32 maxSrc, u32* meta, u32* doneList, u32* doneCount,
                                             unsigned long long* work2 = nullptr, const u8* flagsBase = nullptr, const u8* gate = nullptr,
                                             const u32* ready = nullptr, u32 flagStride = ZN_FLAG_STRIDE) {      // ready[k] != 0: the flags of list entry k are written (gate[k] says whether any will come); flagStride: flag bytes per list entry
    M m; m.st = ZL_DONE; m.lastLL = 0; m.o.n = 0; m.o.lit = 0;
#ifdef ZL_PROFILE
    u64 const zlWaveT0 = __builtin_readcyclecounter(); u64 zlRounds = 0; u64 const zlWall0 = wall_clock64();
#endif
    u32 have = 0, pend = 0, late = 0; u32 k = 0; u64 tPend = 0;          // (per-lane flags as 0 / 1 in vector registers: a loop-carried bool is a lane mask and every divergent assignment three scalar instructions)
    // Finished frames go to the entropy kernel's queue at the WAVE's hand-overs, every ZJ_HAND_ROUNDS rounds, behind ONE release fence for all lanes that finished since
    // (round 5).  On this part an agent-scope release writes the XCD's L2 back; a fence per finished frame — 65 536 per launch — was 8 % of the level-3 match kernel
    // (137.5 -> 126.0 ms with the fences taken out for a timing run, profiles/r05/f_).  A lane without a frame left stays (idle) until the whole wave is.
    u32 pubK = 0xFFFFFFFFu, idle = 0;
    u32 const period = ZE_LW_PERIOD(level) ? ZE_LW_PERIOD(level) : M::default_period(); u32 ph = 0;   // double-fast machines: rounds per rotation of the non-search states
    for (u32 r = 0;; r++) {
        if (pend) {                                       // (machines that cannot take their flags late) a frame that will get flags: start it when they are there — or without them when the wait runs out (50 ms)
            bool const rdy = __hip_atomic_load(&ready[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u;
            if (rdy || wall_clock64() - tPend > 5000000ull) {
                if (rdy) zj_acquire();
                u32 const i = list[k];
                u64 const s0 = srcOff[i]; u32 const size = (u32)(srcOff[i + 1] - s0);
                m.init(src + s0, size, ze_params_of(level, size), tables + (size_t)k * tableStride, fscratch + (size_t)k * ZE_FRAME_STRIDE(maxSrc), maxSrc,
                       rdy ? flagsBase + (size_t)k * flagStride : nullptr);
                pend = 0u; have = 1u;
            }
        } else if (m.st == ZL_DONE && !idle) {
            if (have) {
                u32* const mt = meta + 3 * (size_t)k; mt[0] = m.o.n; mt[1] = m.o.lit + m.lastLL; mt[2] = m.lastLL; have = 0u;
#ifdef ZL_PROFILE
                if (count > 4096u && list[k] < 131072u) zlFrameRounds[list[k]] = r;          // (by frame index: the synthetic set's class is index & 3)
#endif
                if (doneList) {
                    if (pubK != 0xFFFFFFFFu) zj_publish_done(doneList, doneCount, pubK);      // (a second frame finished before the hand-over: with a fence of its own)
                    pubK = k;
                }
            }
            late = 0u;
            bool more;
            if (work2) more = zj_claim_front(work2, k);
            else { k = atomicAdd(workCounter, 1u); more = k < count; }
            if (!more) { if (!doneList) break; idle = 1u; }
            else {
            u32 const i = list[k];
            u64 const s0 = srcOff[i]; u32 const size = (u32)(srcOff[i + 1] - s0);
            u8* const tb = tables + (size_t)k * tableStride; u8* const fs = fscratch + (size_t)k * ZE_FRAME_STRIDE(maxSrc);
            if (size < ZL_MIN_FRAME) { ze_match_lane_serial(src + s0, size, level, tb, fs, maxSrc, meta + 3 * (size_t)k); zj_publish_done(doneList, doneCount, k); continue; }
            bool const flagged = flagsBase && gate[k];
            if (flagged && !M::takes_flags_late()) { pend = 1u; tPend = wall_clock64(); }
            else { m.init(src + s0, size, ze_params_of(level, size), tb, fs, maxSrc, nullptr); have = 1u; late = flagged ? 1u : 0u; }
            }
        }
        // A frame whose flags are still being computed starts WITHOUT them and takes them over when they arrive (flags only ever remove work, and what
        // they say about a position does not depend on when it is asked): once per rotation the lane asks; the request travels with the round's own loads.
        u32 rdyNow = 0;
        if (M::takes_flags_late() && late && ph == 0u) rdyNow = __hip_atomic_load(&ready[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#ifdef ZL_PROFILE
        zlRounds++;
#endif
        if (m.st != ZL_DONE) m.round(ZE_LW_LEVEL(level) == 3 ? ZJ_UNI(ph) : ZJ_UNI(r));
        if (M::takes_flags_late() && rdyNow != 0u) { zj_acquire(); m.take_flags(flagsBase + (size_t)k * flagStride); late = 0u; }
        ph = ph + 1u >= period ? 0u : ph + 1u;
        if (doneList) {                                   // the wave's hand-over (wave-uniform test)
            bool const allIdle = __ballot(!idle) == 0;
            if ((r & (ZJ_HAND_ROUNDS - 1u)) == ZJ_HAND_ROUNDS - 1u || allIdle) {
                if (__ballot(pubK != 0xFFFFFFFFu) != 0) {
                    zj_release();                         // records + meta of every frame the wave finished since the last one, before their queue entries
                    if (pubK != 0xFFFFFFFFu) { zj_queue_done(doneList, doneCount, pubK); pubK = 0xFFFFFFFFu; }
                }
                if (allIdle) break;
            }
        }
    }
#ifdef ZL_PROFILE
    if (threadIdx.x == 0 && blockIdx.x < 2048u && count > 4096u) { zlWaveProf[4 * blockIdx.x] = __builtin_readcyclecounter() - zlWaveT0; zlWaveProf[4 * blockIdx.x + 1] = ((u64)(u32)__builtin_amdgcn_s_getreg(63508) << 32) | (u32)__builtin_amdgcn_s_getreg(63492); zlWaveProf[4 * blockIdx.x + 2] = zlRounds; zlWaveProf[4 * blockIdx.x + 3] = zlWall0; }
    if (ZL_PROFILE > 1 && blockIdx.x == 0 && threadIdx.x < 4) printf("match lane profile: lane %u (frame class %u) done after %llu rounds, %llu Mcycles; cycles/round: phase1 %llu, loads %llu, phase3 %llu\n", threadIdx.x, threadIdx.x & 3, (unsigned long long)m.pR, (unsigned long long)((m.pA + m.pB + m.pC) / 1000000ull), (unsigned long long)(m.pA / m.pR), (unsigned long long)(m.pB / m.pR), (unsigned long long)(m.pC / m.pR));
#endif
}
// entries [listBase, listBase + sliceLen) of a list whose length sits in device memory (a slice past its end is empty)
__device__ __forceinline__ u32 zj_slice_count(const u32* countPtr, u32 listBase, u32 sliceLen) {
    u32 const count = *countPtr;
    return count > listBase ? zj_min(count - listBase, sliceLen) : 0u;
}
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 2))) void zj_enc_match_kernel(const u8* __restrict__ src, const u64* __restrict__ srcOff, u32 level,
                                                           const u32* __restrict__ list, const u32* countPtr, u32* workCounter,
                                                           u8* tables, u32 tableStride, u8* fscratch, u32 maxSrc, u32* meta, u32* doneList, u32* doneCount,
                                                           u32 listBase, u32 sliceLen, unsigned long long* work2) {
    level &= ~ZE_LW_NEG;                                  // negative levels run zj_enc_match_kernel_neg: here the step is 2 at compile time
    u32 const count = zj_slice_count(countPtr, listBase, sliceLen);
    list += listBase;
    if (ZE_LW_LEVEL(level) == 3) zj_match_run<ZLaneD<ZEEntTag> >(src, srcOff, level, list, count, workCounter, tables, tableStride, fscratch, maxSrc, meta, doneList, doneCount, work2);
    else zj_match_run<ZLaneF<ZEEnt16> >(src, srcOff, level, list, count, workCounter, tables, tableStride, fscratch, maxSrc, meta, doneList, doneCount, work2);
}
// Negative levels (zstd's --fast=N; level word with ZE_LW_NEG): the same lane-per-frame fast machine (ZLaneF) with the level's step N + 1 carried in
// the word.  A kernel of its own so that the level 1-2 kernel above keeps its constant step and its registers (ZJNI_ROUTE_LANE reports both).
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 2))) void zj_enc_match_kernel_neg(const u8* __restrict__ src, const u64* __restrict__ srcOff, u32 level,
                                                           const u32* __restrict__ list, const u32* countPtr, u32* workCounter,
                                                           u8* tables, u32 tableStride, u8* fscratch, u32 maxSrc, u32* meta, u32* doneList, u32* doneCount,
                                                           u32 listBase, u32 sliceLen, unsigned long long* work2) {
    u32 const count = zj_slice_count(countPtr, listBase, sliceLen);
    list += listBase;
    zj_match_run<ZLaneF<ZEEnt16> >(src, srcOff, level, list, count, workCounter, tables, tableStride, fscratch, maxSrc, meta, doneList, doneCount, work2);
}

// ---- need-gated level 3 (zj_need.h; ZJNI_NEED = 2 by default: flags for the frames zn_worth() picks) ----
// zj_enc_worth_kernel decides per frame whether it gets flags (gate[k]); zj_enc_need_kernel — one workgroup of 1 024 lanes per picked frame, Bloom
// filters in LDS — computes the flag bytes (which probes can match, which writes can be read) BESIDE the match kernel.  Every frame starts at once;
// a lane with a picked frame asks for ready[k] once per rotation and takes the flags over mid-frame when they are there (the run machine: what a flag
// says about a position does not depend on when it is asked, and until then every flag counts as set).  Nothing ever waits for the flag kernel: if it
// is late, or never scheduled beside the match kernel, frames simply run longer without flags (148 against 152 ms with the bounded wait this replaced,
// profiles/r03/l_late_flags_ab.txt).  The older gated machine (ZJNI_LANE_MACHINE=0) still waits, bounded by 50 ms, and then runs unflagged.
static u32 zj_need_threads() {        // lanes per frame of the flag kernel (one workgroup per CU: its filters take 108 KiB of LDS): ZJNI_NEED_THREADS, 64 .. 1 024
    u32 t = 1024; if (const char* ov = zj_tune("ZJNI_NEED_THREADS")) { int const v = atoi(ov); if (v >= 64 && v <= 1024) t = (u32)v & ~63u; }
    return t;
}
struct ZNThreads {
    __device__ __forceinline__ u32 id() const { return threadIdx.x; }
    __device__ __forceinline__ u32 count() const { return blockDim.x; }
    __device__ __forceinline__ void sync() const { __syncthreads(); }
};
// gate[k] = 1: list entry k will get flags (its slot number goes to pickList); selective = 0: every frame the lane machine takes
__global__ __launch_bounds__(256) void zj_enc_worth_kernel(const u8* __restrict__ src, const u64* __restrict__ srcOff, const u32* __restrict__ list, const u32* countPtr,
                                                           u8* gate, u32* ready, u32 selective, u32* pickList, u32* pickCount) {
    __shared__ u32 bm[136];
    ZNThreads t;
    u32 const count = *countPtr;
    for (u32 k = blockIdx.x; k < count; k += gridDim.x) {
        u32 const i = list[k];
        u64 const s0 = srcOff[i]; u32 const size = (u32)(srcOff[i + 1] - s0);
        bool take = size >= ZL_MIN_FRAME;                 // (the plain loops take smaller frames, zj_match_run)
        if (take && selective) take = zn_worth(t, bm, src + s0, size);
        if (threadIdx.x == 0) { gate[k] = take ? 1 : 0; ready[k] = 0; if (take) pickList[atomicAdd(pickCount, 1u)] = k; }
    }
}
__global__ __launch_bounds__(1024) void zj_enc_need_kernel(const u8* __restrict__ src, const u64* __restrict__ srcOff, u32 level,
                                                          const u32* __restrict__ list, const u32* __restrict__ pickList, const u32* pickCount,
                                                          u8* flagsBase, u32* ready, u32* work, u32 flagStride) {
    ZNLds& L = *(ZNLds*)zj_dyn_lds;
    __shared__ u32 next;
    ZNThreads t;
    u32 const count = *pickCount;
    u32 prev = 0xFFFFFFFFu;                               // the slot whose flags this workgroup finished last: published by lane 0 in the SAME divergent region that claims
    for (;;) {                                            // the next one (a separate `if (lane 0)` at the loop's end makes the compiler route lane 0 around the barriers)
        if (threadIdx.x == 0) {                           // a work queue: workgroups differ in speed, and the match kernel's lanes are waiting
            if (prev != 0xFFFFFFFFu) { zj_release(); __hip_atomic_store(&ready[prev], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
            next = atomicAdd(work, 1u);
        }
        __syncthreads();
        u32 const q = next;
        __syncthreads();
        if (q >= count) break;
        u32 const k = pickList[q], i = list[k];
        u64 const s0 = srcOff[i]; u32 const size = (u32)(srcOff[i + 1] - s0);
        ZEParams const p = ze_params_of(level, size);
        if (size > 65536u) zn_flags_frame_wide(t, L, src + s0, size, p.hashLog, p.chainLog, p.minMatch, flagsBase + (size_t)k * flagStride);      // (the wide launch's frames: a table at a time)
        else zn_flags_frame(t, L, src + s0, size, p.hashLog, p.chainLog, p.minMatch, flagsBase + (size_t)k * flagStride);      // (ends with a barrier: every lane's flag bytes are written)
        prev = k;
    }
}
// The level-3 match kernel of large batches: the run machine (zj_match_run.h) for every frame of the launch — register windows for the sequential
// streams, and for the frames with flags a run of quiet positions per round; frames without flags run it with every flag set.  Mixed waves on
// purpose: a wave of search-dense frames alone issues four times the requests per round (measured with a role split: 201 ms against 168).
template <u32 JMAX>
__device__ __forceinline__ void zj_enc_match_run_body(const u8* __restrict__ src, const u64* __restrict__ srcOff, u32 level,
                                                       const u32* __restrict__ list, const u32* countPtr, u32* workCounter,
                                                       u8* tables, u32 tableStride, u8* fscratch, u32 maxSrc, u32* meta, u32* doneList, u32* doneCount,
                                                       u32 listBase, u32 sliceLen, const u8* flagsBase, const u8* gate, const u32* ready) {
    u32 const count = zj_slice_count(countPtr, listBase, sliceLen);
    zj_match_run<ZLaneR<ZEEntTag, JMAX> >(src, srcOff, level, list + listBase, count, workCounter, tables, tableStride, fscratch, maxSrc, meta, doneList, doneCount, nullptr, flagsBase, gate, ready);
}
#define ZJ_RUN_KERNEL(NAME, JMAX) \
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 2))) void NAME(const u8* __restrict__ src, const u64* __restrict__ srcOff, u32 level, \
                                                           const u32* __restrict__ list, const u32* countPtr, u32* workCounter, \
                                                           u8* tables, u32 tableStride, u8* fscratch, u32 maxSrc, u32* meta, u32* doneList, u32* doneCount, \
                                                           u32 listBase, u32 sliceLen, const u8* flagsBase, const u8* gate, const u32* ready) { \
    zj_enc_match_run_body<JMAX>(src, srcOff, level, list, countPtr, workCounter, tables, tableStride, fscratch, maxSrc, meta, doneList, doneCount, listBase, sliceLen, flagsBase, gate, ready); }
ZJ_RUN_KERNEL(zj_enc_match_run_kernel, ZR_JMAX_DEFAULT)
#ifdef ZJ_TUNING_KERNELS                                      /* run-length sweep for A/B runs (tools/ab.sh, ZJNI_RUN_JMAX) */
ZJ_RUN_KERNEL(zj_enc_match_run3_kernel, 3u)
ZJ_RUN_KERNEL(zj_enc_match_run4_kernel, 4u)
ZJ_RUN_KERNEL(zj_enc_match_run6_kernel, 6u)
ZJ_RUN_KERNEL(zj_enc_match_run7_kernel, 7u)
#endif
#ifdef ZJ_TUNING_KERNELS
// ZJNI_LANE_MACHINE=0: the previous machine (ZLaneD with its table accesses predicated on the flags), kept selectable for A/B runs
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 2))) void zj_enc_match_gated_kernel(const u8* __restrict__ src, const u64* __restrict__ srcOff, u32 level,
                                                           const u32* __restrict__ list, const u32* countPtr, u32* workCounter,
                                                           u8* tables, u32 tableStride, u8* fscratch, u32 maxSrc, u32* meta, u32* doneList, u32* doneCount,
                                                           u32 listBase, u32 sliceLen, const u8* flagsBase, const u8* gate, const u32* ready) {
    u32 const count = zj_slice_count(countPtr, listBase, sliceLen);
    list += listBase;
    zj_match_run<ZLaneD<ZEEntTag, true> >(src, srcOff, level, list, count, workCounter, tables, tableStride, fscratch, maxSrc, meta, doneList, doneCount, nullptr, flagsBase, gate, ready);
}
#endif

// Levels 4-8, frames <= 16 KiB: the hash-chain parsers (ze_block_lazy: greedy / lazy / lazy2), one LANE per frame as plain loops —
// 64 frames per wave instead of one lane of 64 busy; the chain walk (up to 2^searchLog dependent candidate fetches per position)
// keeps the lanes apart, so the wave runs the union of their paths, but every memory round trip still serves up to 64 frames.
// Tables: hash then chain, u32, cleared by the host before the launch; records and meta where the entropy kernel expects them.
#define ZE_CHAIN_MAX_SRC (16u << 10)
#define ZE_CHAIN_TABLE_BYTES (((1u << 14) + (1u << 14)) * 4u)
__global__ __launch_bounds__(64) void zj_enc_match_chain_kernel(const u8* __restrict__ src, const u64* __restrict__ srcOff, u32 level,
                                                                 const u32* __restrict__ list, const u32* countPtr, u32* workCounter,
                                                                 u8* tables, u8* fscratch, u32* meta) {
    u32 const count = *countPtr;
    for (;;) {
        u32 const k = atomicAdd(workCounter, 1u);
        if (k >= count) break;
        u32 const i = list[k];
        u64 const s0 = srcOff[i]; u32 const size = (u32)(srcOff[i + 1] - s0);
        u8* const fs = fscratch + (size_t)k * ZE_FRAME_STRIDE(ZE_CHAIN_MAX_SRC); u32* const mt = meta + 3 * (size_t)k;
        ZEOut o; o.seqs = (ZESeq*)fs; o.litOff = (u32*)(fs + (size_t)ZE_FRAME_MAXSEQ(ZE_CHAIN_MAX_SRC) * 16u); o.n = 0; o.lit = 0;
        u32 lastLL = size;
        if (size >= 7u) {
            ZEParams const p = ze_params_of(level, size);
            u32* const t = (u32*)(tables + (size_t)k * ZE_CHAIN_TABLE_BYTES);
            lastLL = ze_block_lazy(o, src + s0, size, p, t, t + (1u << p.hashLog));
        }
        mt[0] = o.n; mt[1] = o.lit + lastLL; mt[2] = lastLL;
    }
}

// Levels 4-8, 16 KiB < frame <= 128 KiB, large batches: the same plain-loop parsers one lane per frame — level 4's double-fast with
// 2^17-entry tables, levels 5-8 on the row-based finder — with a table set (ZE_MULTI_TABLE_BYTES) per LANE SLOT of the launch instead
// of per frame: a wave's lanes each claim a frame, the wave clears the claimed slots' tables together (coalesced), every lane parses
// its frame, repeat.  Records and meta go to slice-relative slots; the entropy kernel follows on the same slice.
__global__ __launch_bounds__(64) void zj_enc_match_big_kernel(const u8* __restrict__ src, const u64* __restrict__ srcOff, u32 level,
                                                               const u32* __restrict__ list, const u32* countPtr, u32* workCounter,
                                                               u32* tables, u8* fscratch, u32* meta, u32 listBase, u32 sliceLen) {
    u32 const count = zj_slice_count(countPtr, listBase, sliceLen);
    list += listBase;
    u32* const t = tables + ((size_t)blockIdx.x * 64u + threadIdx.x) * (ZE_MULTI_TABLE_BYTES / 4u);
    for (;;) {
        u32 const k = atomicAdd(workCounter, 1u);
        bool const have = k < count;
        if (!__ballot(have)) break;
        u32 size = 0, entries = 0; u64 s0 = 0; ZEParams p; p.windowLog = p.chainLog = p.hashLog = p.minMatch = p.strategy = p.searchLog = 0;
        if (have) {
            u32 const i = list[k];
            s0 = srcOff[i]; size = (u32)(srcOff[i + 1] - s0);
            p = ze_params_of(level, size);
            entries = ze_params_uses_rows(p) ? (1u << p.hashLog) + (1u << p.hashLog) / 4u : (1u << p.hashLog) + (1u << p.chainLog);
        }
        for (u64 m = __ballot(have && size >= 7u); m; m &= m - 1) {          // clear the claimed slots' tables, one slot at a time, all lanes
            u32 const j = (u32)__builtin_ctzll(m);
            u32* const tj = tables + ((size_t)blockIdx.x * 64u + j) * (ZE_MULTI_TABLE_BYTES / 4u);
            u32 const ej = (u32)__shfl((int)entries, (int)j, 64);
            for (u32 x = threadIdx.x; x < ej; x += 64u) tj[x] = 0;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup"); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        if (have) {
            u8* const fs = fscratch + (size_t)k * ZE_FRAME_STRIDE(ZE_BLOCK_MAX); u32* const mt = meta + 3 * (size_t)k;
            ZEOut o; o.seqs = (ZESeq*)fs; o.litOff = (u32*)(fs + (size_t)ZE_FRAME_MAXSEQ(ZE_BLOCK_MAX) * 16u); o.n = 0; o.lit = 0;
            u32 lastLL = size;
            if (size >= 7u) lastLL = p.strategy >= 3u ? ze_block_lazy(o, src + s0, size, p, t, t + (1u << p.hashLog))
                                                      : ze_block_dfast<ZEEnt32>(o, src + s0, size, p.hashLog, p.chainLog, p.minMatch, t, t + (1u << p.hashLog));
            mt[0] = o.n; mt[1] = o.lit + lastLL; mt[2] = lastLL;
        }
    }
}

// Wave-per-frame match finding (zj_match_wave.h): level-3 frames <= 64 KiB with the tables in LDS, claimed from the back of the
// sorted list.  Records and meta of list entry k go where the lane kernel would put them, completion goes to the same queue.
__global__ __launch_bounds__(64) void zj_enc_match_wave_kernel(const u8* __restrict__ src, const u64* __restrict__ srcOff, u32 level,
                                                                const u32* __restrict__ list, const u32* countPtr, unsigned long long* work2,
                                                                u8* fscratch, u32 maxSrc, u32* meta, u32* doneList, u32* doneCount) {
    ZWLds& lds = *(ZWLds*)zj_dyn_lds;
    u32 const count = ZJ_UNI(*countPtr);
    for (;;) {
        u32 k = 0, ok = 0;
        if (threadIdx.x == 0) ok = zj_claim_back(work2, count, k) ? 1u : 0u;
        ok = ZJ_UNI(ok); k = ZJ_UNI(k);
        if (!ok) break;
        u32 const i = ZJ_UNI(list[k]);
        u64 const s0 = zj_uni64(srcOff[i]); u32 const size = (u32)(zj_uni64(srcOff[i + 1]) - s0);
        u8* const fs = fscratch + (size_t)k * ZE_FRAME_STRIDE(maxSrc); u32* const mt = meta + 3 * (size_t)k;
        if (size >= 64u) zw_match_frame(lds, src + s0, size, level, fs, maxSrc, mt);
        else {                                           // tiny frame: the plain loop on lane 0, tables in LDS
            ZEParams const p = ze_params_of(level, size);
            for (u32 j = threadIdx.x; j < (1u << p.hashLog); j += 64u) lds.HL[j] = 0;
            for (u32 j = threadIdx.x; j < (1u << p.chainLog); j += 64u) lds.HS[j] = 0;
            __syncthreads();
            if (threadIdx.x == 0) {
                ZEOut o; o.seqs = (ZESeq*)fs; o.litOff = (u32*)(fs + (size_t)ZE_FRAME_MAXSEQ(maxSrc) * 16u); o.n = 0; o.lit = 0;
                u32 lastLL = size;
                if (size >= 7u) lastLL = ze_block_dfast<ZEEnt16>(o, src + s0, size, p.hashLog, p.chainLog, p.minMatch, lds.HL, lds.HS);
                mt[0] = o.n; mt[1] = o.lit + lastLL; mt[2] = lastLL;
            }
        }
        if (threadIdx.x == 0) zj_publish_done(doneList, doneCount, k);
        __syncthreads();
    }
}

#ifdef ZJ_TUNING_KERNELS      /* the ZJNI_HYBRID experiment (DESIGN history, round 2): it stayed off and lives in tuning builds only */
// Search-density score of each listed frame: distinct 4-byte values among 1 024 consecutive positions from the middle of the
// frame (hashed into a 4 096-bit set), 0..63.  Text-like frames (few distinct values: almost every position starts a match)
// score low, frames that are searched position by position score high.
__global__ __launch_bounds__(64) void zj_enc_score_kernel(const u8* __restrict__ src, const u64* __restrict__ srcOff, const u32* __restrict__ list,
                                                           const u32* countPtr, u8* score) {
    __shared__ u32 bm[128];
    u32 const count = ZJ_UNI(*countPtr);
    for (u32 k = blockIdx.x; k < count; k += gridDim.x) {
        u32 const i = ZJ_UNI(list[k]);
        u64 const s0 = zj_uni64(srcOff[i]); u32 const size = (u32)(zj_uni64(srcOff[i + 1]) - s0);
        u32 sc = 0;
        if (size >= 64u) {
            u32 const avail = size - 4u, S = avail < 1024u ? avail : 1024u, off = (avail - S) >> 1;
            bm[threadIdx.x] = 0; bm[threadIdx.x + 64u] = 0;
            __syncthreads();
            for (u32 p = threadIdx.x; p < S; p += 64u) {
                u32 const h = (ld32(src + s0 + off + p) * 2654435761u) >> 20;
                atomicOr(&bm[h >> 5], 1u << (h & 31u));
            }
            __syncthreads();
            u32 c = (u32)__popc(bm[threadIdx.x]) + (u32)__popc(bm[threadIdx.x + 64u]);
            for (int d = 32; d >= 1; d >>= 1) c += __shfl_xor(c, d, 64);
            sc = (c * 64u) / S; if (sc > 63u) sc = 63u;
            __syncthreads();
        }
        if (threadIdx.x == 0) score[k] = (u8)sc;
    }
}
// Partition of the list for the two match kernels: frames scoring at least `threshold` go to the back (the wave kernel's own
// part, counted from the end) — at most `cap` of them, the wave kernel is the slower of the two per frame and what it takes
// off the lane kernel is HBM requests — everything else to the front IN LIST ORDER (as far as the atomics keep it): a lane
// wave should hold a mix of cheap and expensive frames, 64 expensive ones in one wave leave it running alone at the end.
// work2: [0] u64 cursor pair, [2] split, [3] cursor of the wave kernel's part, [4] search-dense frames seen, [5] front fill.
__global__ __launch_bounds__(256) void zj_enc_partition_kernel(const u32* __restrict__ list, const u32* countPtr, const u8* __restrict__ score, u32 threshold,
                                                               u32 sharePermille, unsigned long long* work2, u32* sorted) {
    u32 const k = blockIdx.x * blockDim.x + threadIdx.x, count = *countPtr;
    if (k >= count) return;
    u32* const w = (u32*)work2;
    u32 const cap = (u32)(((u64)count * sharePermille) / 1000u);
    if (score[k] >= threshold) {
        u32 const r = atomicAdd(&w[4], 1u);
        if (r < cap) { sorted[count - 1u - r] = list[k]; return; }
    }
    sorted[atomicAdd(&w[5], 1u)] = list[k];
}
__global__ void zj_enc_partition_done_kernel(const u32* countPtr, u32 sharePermille, unsigned long long* work2) {
    u32* const w = (u32*)work2;
    u32 const count = *countPtr, cap = (u32)(((u64)count * sharePermille) / 1000u);
    w[2] = count - (w[4] < cap ? w[4] : cap);
}
#endif

// The wide launch: frames > 64 KiB and the fast-strategy frames whose tables exceed the common size; 4-byte positions.
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 2))) void zj_enc_match_wide_kernel(const u8* __restrict__ src, const u64* __restrict__ srcOff, u32 level,
                                                           const u32* __restrict__ list, const u32* countPtr, u32* workCounter,
                                                           u8* tables, u32 tableStride, u8* fscratch, u32 maxSrc, u32* meta, u32 listBase, u32 sliceLen, u32* doneList, u32* doneCount,
                                                           const u8* flagsBase, const u8* gate, const u32* ready) {
    level &= ~ZE_LW_NEG;                                  // negative levels: zj_enc_match_wide_kernel_neg
    u32 const count = zj_slice_count(countPtr, listBase, sliceLen);
    list += listBase;
    // With need flags (level 3, flagsBase != nullptr): the run machine for every frame of the slice, flags of ZN_FLAG_STRIDE_WIDE bytes per entry for the frames
    // zj_enc_worth_kernel picked, taken over when zj_enc_need_kernel has written them (zn_flags_frame_wide) — what zj_enc_match_run_kernel does on the common path.
    if (flagsBase) { zj_match_run<ZLaneR<ZEEntTag> >(src, srcOff, level, list, count, workCounter, tables, tableStride, fscratch, maxSrc, meta, doneList, doneCount, nullptr, flagsBase, gate, ready, ZN_FLAG_STRIDE_WIDE); return; }
    // without flags, level 3: ZLaneD.  The run machine WITHOUT flags was measured here in round 4 and is not faster on 128 KiB frames:
    // 65 536 x 128 KiB 382-441 ms with ZLaneD, 445-492 ms with ZLaneR (profiles/r04/d_, e_); tests/test_emu_encode.py keeps the machine exact at these sizes.
    if (ZE_LW_LEVEL(level) == 3) zj_match_run<ZLaneD<ZEEntTag> >(src, srcOff, level, list, count, workCounter, tables, tableStride, fscratch, maxSrc, meta, doneList, doneCount);
    else zj_match_run<ZLaneF<ZEEnt32> >(src, srcOff, level, list, count, workCounter, tables, tableStride, fscratch, maxSrc, meta, doneList, doneCount);
}
// negative levels, frames of list B (4-byte positions): ZLaneF with the level's step, as zj_enc_match_kernel_neg (no need flags: those are level 3's)
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 2))) void zj_enc_match_wide_kernel_neg(const u8* __restrict__ src, const u64* __restrict__ srcOff, u32 level,
                                                           const u32* __restrict__ list, const u32* countPtr, u32* workCounter,
                                                           u8* tables, u32 tableStride, u8* fscratch, u32 maxSrc, u32* meta, u32 listBase, u32 sliceLen, u32* doneList, u32* doneCount,
                                                           const u8* flagsBase, const u8* gate, const u32* ready) {
    u32 const count = zj_slice_count(countPtr, listBase, sliceLen);
    list += listBase;
    zj_match_run<ZLaneF<ZEEnt32> >(src, srcOff, level, list, count, workCounter, tables, tableStride, fscratch, maxSrc, meta, doneList, doneCount);
}
// zero the first `count` slots of `stride` bytes (the table slots of a slice; nothing to do for an empty slice)
__global__ __launch_bounds__(256) void zj_zero_slots_kernel(u8* base, u32 stride, const u32* countPtr, u32 listBase, u32 sliceLen) {
    u32 const count = zj_slice_count(countPtr, listBase, sliceLen);
    size_t const total16 = (size_t)count * (stride / 16u);
    uint4* const w = (uint4*)base;
    for (size_t j = (size_t)blockIdx.x * 256 + threadIdx.x; j < total16; j += (size_t)gridDim.x * 256) w[j] = make_uint4(0, 0, 0, 0);
}

// At most 168 VGPRs (three waves a SIMD): this kernel runs BESIDE the match kernels, and what it takes of the register file they
// cannot have — at 223 VGPRs the dictionary match kernel ran 16.5 -> 20.8 ms a slice (profiles/r03/i_entropy_vgpr_ab.txt).
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(3, 8))) void zj_encode_kernel(const u8* __restrict__ src, const u64* __restrict__ srcOff,
                                                        u8* __restrict__ dst, const u64* __restrict__ dstOff,
                                                        u64* __restrict__ result, u32 level, const u32* __restrict__ list,
                                                        const u32* countPtr, u32* workCounter, u8* scratch, unsigned long long* prof,
                                                        u8* fscratch, u32 maxSrc, const u32* meta,
                                                        u32 mode, const u32* doneList, u32* procFlag, u32 flags, const ZECDictDev* cd, u32 ldsBytes, u32 listBase, u32 sliceLen) {
    // mode 0: list entry k.  mode 1: k-th entry of the completion queue the match kernel fills while this kernel
    // runs (bounded wait; a workgroup that gives up leaves its frame to the mode-2 pass).  mode 2: list entries
    // mode 1 did not finish.
    __shared__ ZEncShared sh;
    ZjProf pf; pf.start(prof);
    Grp<64> g;
    if (threadIdx.x == 0) { sh.dictLoaded = 0; sh.ctDict[0] = 0; sh.ctDict[1] = 0; sh.ctDict[2] = 0; }
    __syncthreads();
    u8* const ws = scratch + (size_t)blockIdx.x * ZE_SCRATCH_BYTES;
    u32 const count = ZJ_UNI(zj_slice_count(countPtr, listBase, sliceLen));
    list += listBase;
    for (;;) {
        u32 k = zj_next_index(workCounter);           // wave-uniform (SGPR)
        if (k >= count) break;
        if (mode == 1) {
            u32 v = 0xFFFFFFFFu;
            if (threadIdx.x == 0) {
                u64 const t0 = wall_clock64();            // 100 MHz
                for (;;) {
                    // relaxed poll: an acquire here would invalidate this CU's L1 every few microseconds, under the
                    // match waves that share it; the fence after the loop orders the reads of the frame's records
                    v = __hip_atomic_load(&doneList[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (v != 0xFFFFFFFFu || wall_clock64() - t0 > 200000000ull) break;     // 2 s
                    __builtin_amdgcn_s_sleep(127); __builtin_amdgcn_s_sleep(127);
                }
            }
            v = (u32)__builtin_amdgcn_readfirstlane((int)v);
            if (v == 0xFFFFFFFFu) break;
            zj_acquire();
            k = v;
        } else if (mode == 2) {
            if (ZJ_UNI(procFlag[k])) continue;
        }
        u32 const i = ZJ_UNI(list[k]);
        u64 const s0 = zj_uni64(srcOff[i]), s1 = zj_uni64(srcOff[i + 1]), d0 = zj_uni64(dstOff[i]), d1 = zj_uni64(dstOff[i + 1]);
        u64 const cap = d1 - d0;
        ZEPre pre; const ZEPre* prePtr = nullptr;
        if (fscratch) {                                   // sequences were found by zj_enc_match_kernel
            u8* const fs = fscratch + (size_t)k * ZE_FRAME_STRIDE(maxSrc);
            pre.seqs = (ZESeq*)fs; pre.litOff = (const u32*)(fs + (size_t)ZE_FRAME_MAXSEQ(maxSrc) * 16u); pre.meta = meta + 3 * (size_t)k;
            prePtr = &pre;
        }
        u64 const r = ze_compress(g, sh, zj_dyn_lds, src + s0, (u32)(s1 - s0), dst + d0, (u32)(cap > 0xFFFFFFFFull ? 0xFFFFFFFFull : cap), level, ws, pf, prePtr, flags, cd, ldsBytes);
        pf.mark(7);
        if (threadIdx.x == 0) { result[i] = r; if (mode == 1) procFlag[k] = 1u; }
        __syncthreads();
    }
}

// Which of the two kernels serves list C is decided on the device, by both, from the classify kernel's counters (countPtr = &counters[4]: |C|, work, multi-block frames):
// the pipelined one when every frame is resident at once (|C| <= pipeMax workgroups) and at least half of them are multi-block frames; the other one returns at once.
__device__ __forceinline__ bool zj_pipe_route(const u32* countPtr, u32 pipeMax) { u32 const c = countPtr[0]; return pipeMax != 0u && c <= pipeMax && 2u * countPtr[2] >= c && c != 0u; }
// Multi-block frames (128 KiB < input <= ZE_MULTI_MAX): one wavefront walks a frame block by block (ze_compress_multi); its
// frame-wide hash tables sit in HBM, one set per resident workgroup.
#ifndef ZJ_MULTI_WAVES
#define ZJ_MULTI_WAVES 2       /* resident waves per SIMD the register allocation aims at (the wave matcher's windows want ~220 VGPRs) */
#endif
__global__ __launch_bounds__(64, ZJ_MULTI_WAVES) void zj_encode_multi_kernel(const u8* __restrict__ src, const u64* __restrict__ srcOff, u8* __restrict__ dst, const u64* __restrict__ dstOff,
                                                              u64* __restrict__ result, u32 level, const u32* __restrict__ list, const u32* countPtr, u32* workCounter,
                                                              u8* scratch, u32* tables, u32 flags, u32 ldsBytes, u32 pipeMax) {
    if (zj_pipe_route(countPtr, pipeMax)) return;          // zj_encode_pipe_kernel's batch (queued ahead of this launch)
    level &= ~ZE_LW_NEG;                                   // negative levels: zj_encode_multi_kernel_neg
    __shared__ ZEncShared sh;
#ifdef ZX_PROFILE          /* analysis build: the entropy stage's phase marks of workgroup 0, printed when it is done (tools/ab_call*.sh) */
    __shared__ unsigned long long zxPhase[16];
    if (threadIdx.x < 16) zxPhase[threadIdx.x] = 0;
    __syncthreads();
    ZjProf pf; pf.start(blockIdx.x == 0 ? zxPhase : nullptr);
#else
    ZjProf pf; pf.start(nullptr);
#endif
    Grp<64> g;
    if (threadIdx.x == 0) { sh.dictLoaded = 0; sh.ctDict[0] = 0; sh.ctDict[1] = 0; sh.ctDict[2] = 0; }
    __syncthreads();
    u8* const ws = scratch + (size_t)blockIdx.x * ZE_SCRATCH_BYTES;
    u32* const tb = tables + (size_t)blockIdx.x * (ZE_MULTI_TABLE_BYTES / 4u);
    u32 const count = ZJ_UNI(*countPtr);
    for (;;) {
        u32 const k = zj_next_index(workCounter);
        if (k >= count) break;
        u32 const i = ZJ_UNI(list[k]);
        u64 const s0 = zj_uni64(srcOff[i]), s1 = zj_uni64(srcOff[i + 1]), d0 = zj_uni64(dstOff[i]), d1 = zj_uni64(dstOff[i + 1]);
        u64 const cap = d1 - d0;
        u32 const size = (u32)(s1 - s0), capU = (u32)(cap > 0xFFFFFFFFull ? 0xFFFFFFFFull : cap);
        // level 4 (one block, tables too large for LDS) or a multi-block frame of levels 1-3
        u64 const r = size <= ZE_BLOCK_MAX ? ze_compress_t<Grp<64>, u32>(g, sh, zj_dyn_lds, src + s0, size, dst + d0, capU, level, ws, pf, nullptr, flags, nullptr, ldsBytes, nullptr, tb)
                                           : ze_compress_multi(g, sh, zj_dyn_lds, src + s0, size, dst + d0, capU, level, ws, pf, flags, tb, ldsBytes);
        if (threadIdx.x == 0) result[i] = r;
        __syncthreads();
    }
#ifdef ZX_PROFILE
    if (blockIdx.x == 0 && threadIdx.x == 0)
        printf("zx phases wg 0 (kcycles): zero+params %llu  match %llu  literals gather+codes %llu  hist+huffman table %llu  huffman encode %llu  sequence tables %llu  sequence encode %llu  block place %llu\n",
               zxPhase[0] / 1000ull, zxPhase[1] / 1000ull, zxPhase[2] / 1000ull, zxPhase[3] / 1000ull, zxPhase[4] / 1000ull, zxPhase[5] / 1000ull, zxPhase[6] / 1000ull, zxPhase[7] / 1000ull);
#endif
}

// Negative levels, list C (their multi-block frames only: single-block frames of these levels are lists A / B): the frame loop above with the
// level's step in the one-lane parse of every block (the wave matcher ZWaveF walks step 2 only) and raw literals.  A kernel of its own so that
// the one above keeps its registers; the pipelined kernel below does not take these levels.
__global__ __launch_bounds__(64, ZJ_MULTI_WAVES) void zj_encode_multi_kernel_neg(const u8* __restrict__ src, const u64* __restrict__ srcOff, u8* __restrict__ dst, const u64* __restrict__ dstOff,
                                                              u64* __restrict__ result, u32 level, const u32* __restrict__ list, const u32* countPtr, u32* workCounter,
                                                              u8* scratch, u32* tables, u32 flags, u32 ldsBytes, u32 pipeMax) {
    __shared__ ZEncShared sh;
    ZjProf pf; pf.start(nullptr);
    Grp<64> g;
    if (threadIdx.x == 0) { sh.dictLoaded = 0; sh.ctDict[0] = 0; sh.ctDict[1] = 0; sh.ctDict[2] = 0; }
    __syncthreads();
    u8* const ws = scratch + (size_t)blockIdx.x * ZE_SCRATCH_BYTES;
    u32* const tb = tables + (size_t)blockIdx.x * (ZE_MULTI_TABLE_BYTES / 4u);
    u32 const count = ZJ_UNI(*countPtr);
    for (;;) {
        u32 const k = zj_next_index(workCounter);
        if (k >= count) break;
        u32 const i = ZJ_UNI(list[k]);
        u64 const s0 = zj_uni64(srcOff[i]), s1 = zj_uni64(srcOff[i + 1]), d0 = zj_uni64(dstOff[i]), d1 = zj_uni64(dstOff[i + 1]);
        u64 const cap = d1 - d0;
        u32 const size = (u32)(s1 - s0), capU = (u32)(cap > 0xFFFFFFFFull ? 0xFFFFFFFFull : cap);
        u64 const r = ze_compress_multi(g, sh, zj_dyn_lds, src + s0, size, dst + d0, capU, level, ws, pf, flags | ZE_FLAG_MULTI_FAST_SERIAL, tb, ldsBytes);
        if (threadIdx.x == 0) result[i] = r;
        __syncthreads();
    }
}

// Multi-block frames, PIPELINED (round 6; zj_encode.h "multi-block frames, PIPELINED"): a workgroup of TWO waves per frame — wave 1 parses block b + 1 while wave 0
// entropy-codes block b.  For batches that cannot fill the device with one-wave chains (a thousand 1 MiB frames: BASELINE config 1); with every wave slot taken the
// one-wave kernel above does the same work in fewer wave-milliseconds, so large batches stay there (compress_batch_device_impl).  Scratch: two slots of encScratch
// per workgroup (block b in slot b & 1), one table set; dynamic LDS: [ZEEntropy of the entropy wave][ZJ_PIPE_LDS_P bytes of the parse wave].
#define ZJ_PIPE_LDS_P 10240u
static_assert(sizeof(ZXLds) <= ZJ_PIPE_LDS_P && 2064u <= ZJ_PIPE_LDS_P, "the parse wave's LDS holds the wave matcher's scoreboards, or the pre-splitter's histograms");
__global__ __launch_bounds__(128, 2) void zj_encode_pipe_kernel(const u8* __restrict__ src, const u64* __restrict__ srcOff, u8* __restrict__ dst, const u64* __restrict__ dstOff,
                                                             u64* __restrict__ result, u32 level, const u32* __restrict__ list, const u32* countPtr, u32* workCounter,
                                                             u8* scratch, u32* tables, u32 flags, u32 ldsBytesE, u32 pipeMax) {
    if (!zj_pipe_route(countPtr, pipeMax)) return;
    level &= ~ZE_LW_NEG;                                   // (never launched for negative levels)
    // (ONE LDS object: declared as separate variables the two waves' uniforms came out OVERLAID — group_segment_fixed_size 1 440 instead of 2 700: each is used by one
    //  role's code only, and the LDS lowering does not know that the roles run at the same time on different waves)
    struct PipeShared { ZEncShared e, p; ZEPipe pipe; u32 nextK; };
    __shared__ PipeShared S;
    ZEncShared& shE = S.e; ZEncShared& shP = S.p; ZEPipe& pipe = S.pipe; u32& nextK = S.nextK;
    u32 const role = threadIdx.x >> 6;                     // 0: the entropy wave (and single-block frames of the list), 1: the parse wave
    GrpWave g;
    ZjProf pf; pf.start(nullptr);
    if (threadIdx.x == 0) { shE.dictLoaded = 0; shE.ctDict[0] = 0; shE.ctDict[1] = 0; shE.ctDict[2] = 0; shP.dictLoaded = 0; shP.ctDict[0] = 0; shP.ctDict[1] = 0; shP.ctDict[2] = 0; }
    __syncthreads();
    u8* const ws0 = scratch + (size_t)(2u * blockIdx.x) * ZE_SCRATCH_BYTES; u8* const ws1 = ws0 + ZE_SCRATCH_BYTES;
    u32* const tb = tables + (size_t)blockIdx.x * (ZE_MULTI_TABLE_BYTES / 4u);
    u8* const ldsE = zj_dyn_lds; u8* const ldsP = zj_dyn_lds + ((ldsBytesE + 15u) & ~15u);      // (sizeof(ZEEntropy) is 4 mod 8 and the wave matcher's scoreboards are 64-bit LDS atomics)
    u32 const count = ZJ_UNI(*countPtr);
    for (;;) {
        if (threadIdx.x == 0) nextK = atomicAdd(workCounter, 1u);
        __syncthreads();
        u32 const k = ZJ_UNI(nextK);
        __syncthreads();                                    // (both waves have it before the next round writes it)
        if (k >= count) break;
        u32 const i = ZJ_UNI(list[k]);
        u64 const s0 = zj_uni64(srcOff[i]), s1 = zj_uni64(srcOff[i + 1]), d0 = zj_uni64(dstOff[i]), d1 = zj_uni64(dstOff[i + 1]);
        u64 const cap = d1 - d0;
        u32 const size = (u32)(s1 - s0), capU = (u32)(cap > 0xFFFFFFFFull ? 0xFFFFFFFFull : cap);
        ZEParams const p = ze_params_of(ZE_LW_LEVEL(level), size);
        if (size <= ZE_BLOCK_MAX) {                         // level 4 (one block, tables too large for LDS): the entropy wave alone, as zj_encode_multi_kernel does it
            if (role == 0) { u64 const r = ze_compress_t<GrpWave, u32>(g, shE, ldsE, src + s0, size, dst + d0, capU, level, ws0, pf, nullptr, flags, nullptr, ldsBytesE, nullptr, tb); if ((threadIdx.x & 63u) == 0) result[i] = r; }
        } else if (size > ZE_MULTI_MAX || size > (1u << p.windowLog)) { if (threadIdx.x == 0) result[i] = ZJ_ERR64(201); }
        else {
            if (threadIdx.x == 0) { pipe.ready = 0; pipe.done = 0; pipe.err = 0; }
            __syncthreads();
            if (role == 1) {
                ze_pipe_parse_role(g, shP, ldsP, pipe, src + s0, size, capU, level, flags, tb, ws0, ws1, [&](u32 want) {
                    for (;;) {
                        if (ZJ_UNI(ze_pipe_load(&pipe.done)) >= want || ZJ_UNI(ze_pipe_load(&pipe.err))) break;
                        __builtin_amdgcn_s_sleep(32);
                    }
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
                });
            } else {
                ZEPipeE st;
                ze_pipe_entropy_init(g, shE, st, dst + d0, capU, size, level, flags);
                if (st.finished) { if ((threadIdx.x & 63u) == 0) pipe.err = 1; }
#ifdef ZE_PIPE_DEBUG
                u64 dbgWaitE = 0, dbgWorkE = 0;
#endif
                while (!st.finished) {
#ifdef ZE_PIPE_DEBUG
                    u64 const t0 = wall_clock64();
#endif
                    while (ZJ_UNI(ze_pipe_load(&pipe.ready)) <= st.b) __builtin_amdgcn_s_sleep(32);
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
#ifdef ZE_PIPE_DEBUG
                    u64 const t1 = wall_clock64(); dbgWaitE += t1 - t0;
#endif
                    ze_pipe_entropy_step(g, shE, ldsE, pipe, st, src + s0, size, dst + d0, capU, level, flags, ws0, ws1, pf, ldsBytesE);
#ifdef ZE_PIPE_DEBUG
                    dbgWorkE += wall_clock64() - t1;
#endif
                }
#ifdef ZE_PIPE_DEBUG
                if (blockIdx.x < 4u && (threadIdx.x & 63u) == 0) printf("pipe E wg %u: %u blocks, waiting %llu us, working %llu us\n", blockIdx.x, st.b, (unsigned long long)(dbgWaitE / 100ull), (unsigned long long)(dbgWorkE / 100ull));
#endif
                if ((threadIdx.x & 63u) == 0) result[i] = st.result;
            }
        }
        __syncthreads();
    }
}

// Stream frames (ze_compress_stream, zj_encode.h): what the reference's stream classes produce without a pledged size, one wavefront per stream over the
// multi-block kernel's table slots.  mode[i]: bit 0 final (close()), bit 1 the stream was closed before anything else was called on it; flushAt / flushOff:
// the flush positions of stream i = flushAt[flushOff[i] .. flushOff[i + 1]) (flushOff == nullptr: none).
__global__ __launch_bounds__(64, ZJ_MULTI_WAVES) void zj_encode_stream_kernel(const u8* __restrict__ src, const u64* __restrict__ srcOff, u8* __restrict__ dst, const u64* __restrict__ dstOff,
                                                               u64* __restrict__ result, u32 level, u32 count, u32* workCounter, u8* scratch, u32* tables, u32 flags, u32 ldsBytes,
                                                               const u32* __restrict__ flushAt, const u64* __restrict__ flushOff, const u32* __restrict__ mode) {
    __shared__ ZEncShared sh;
    ZjProf pf; pf.start(nullptr);
    Grp<64> g;
    if (threadIdx.x == 0) { sh.dictLoaded = 0; sh.ctDict[0] = 0; sh.ctDict[1] = 0; sh.ctDict[2] = 0; }
    __syncthreads();
    u8* const ws = scratch + (size_t)blockIdx.x * ZE_SCRATCH_BYTES;
    u32* const tb = tables + (size_t)blockIdx.x * (ZE_MULTI_TABLE_BYTES / 4u);
    for (;;) {
        u32 const i = zj_next_index(workCounter);
        if (i >= count) break;
        u64 const s0 = zj_uni64(srcOff[i]), s1 = zj_uni64(srcOff[i + 1]), d0 = zj_uni64(dstOff[i]), d1 = zj_uni64(dstOff[i + 1]);
        u64 const cap = d1 - d0, size64 = s1 - s0;
        u32 const capU = (u32)(cap > 0xFFFFFFFFull ? 0xFFFFFFFFull : cap);
        u64 const f0 = flushOff ? zj_uni64(flushOff[i]) : 0, f1 = flushOff ? zj_uni64(flushOff[i + 1]) : 0;
        u32 const md = mode ? ZJ_UNI(mode[i]) : 1u;
        u64 const r = size64 > ZE_MULTI_MAX ? ZJ_ERR64(201)
                                            : ze_compress_stream(g, sh, zj_dyn_lds, src + s0, (u32)size64, dst + d0, capU, level, ws, pf, flags, tb, ldsBytes, flushAt + f0, (u32)(f1 - f0), md & 1u, (md >> 1) & 1u);
        if (threadIdx.x == 0) result[i] = r;
        __syncthreads();
    }
}

// Stream frames continued from their state (ze_compress_stream_resume, zj_encode.h): the loop above with stream i's ZEStreamState at state + i * stateStride — its
// tables are parsed in place, so the launch takes no table slots, only the scratch slots.  A kernel of its own so that the one above keeps its registers.
__global__ __launch_bounds__(64, ZJ_MULTI_WAVES) void zj_encode_stream_continue_kernel(const u8* __restrict__ src, const u64* __restrict__ srcOff, u8* __restrict__ dst, const u64* __restrict__ dstOff,
                                                               u64* __restrict__ result, u32 level, u32 count, u32* workCounter, u8* scratch, u8* state, u64 stateStride, u32 flags, u32 ldsBytes,
                                                               const u32* __restrict__ flushAt, const u64* __restrict__ flushOff, const u32* __restrict__ mode) {
    __shared__ ZEncShared sh;
    ZjProf pf; pf.start(nullptr);
    Grp<64> g;
    if (threadIdx.x == 0) { sh.dictLoaded = 0; sh.ctDict[0] = 0; sh.ctDict[1] = 0; sh.ctDict[2] = 0; }
    __syncthreads();
    u8* const ws = scratch + (size_t)blockIdx.x * ZE_SCRATCH_BYTES;
    for (;;) {
        u32 const i = zj_next_index(workCounter);
        if (i >= count) break;
        u64 const s0 = zj_uni64(srcOff[i]), s1 = zj_uni64(srcOff[i + 1]), d0 = zj_uni64(dstOff[i]), d1 = zj_uni64(dstOff[i + 1]);
        u64 const cap = d1 - d0, size64 = s1 - s0;
        u32 const capU = (u32)(cap > 0xFFFFFFFFull ? 0xFFFFFFFFull : cap);
        u32 const size = size64 > ZE_MULTI_MAX ? ZE_MULTI_MAX + 1u : (u32)size64;              // (beyond every window: 201, and the state is dead)
        u64 const f0 = flushOff ? zj_uni64(flushOff[i]) : 0, f1 = flushOff ? zj_uni64(flushOff[i + 1]) : 0;
        u32 const md = mode ? ZJ_UNI(mode[i]) : 1u;
        u64 const r = ze_compress_stream_resume(g, sh, zj_dyn_lds, src + s0, size, dst + d0, capU, level, ws, pf, flags, (ZEStreamState*)(state + (size_t)i * stateStride), ldsBytes,
                                                flushAt + f0, (u32)(f1 - f0), md & 1u, (md >> 1) & 1u, (md >> 2) & 1u);
        if (threadIdx.x == 0) result[i] = r;
        __syncthreads();
    }
}

// ZSTD_createCDict on the device: one workgroup digests the dictionary held in `out` (header, zeroed tables, raw bytes)
__global__ __launch_bounds__(64) void zj_cdict_digest_kernel(u32 dictSize, u32 level, ZECDictDev* out) {
    __shared__ ZDecShared sh;
    __shared__ ZEEntropy e;
    Grp<64> g;
    ze_cdict_digest(g, sh, e, dictSize, level, out);
}
// the same at a negative level (`level`: its word, zj_encode.h ZE_LW_NEG): row 0's parameters (zj_cdict.h ze_cdict_params_neg).  A kernel of its own so that
// the one above keeps its registers.
__global__ __launch_bounds__(64) void zj_cdict_digest_kernel_neg(u32 dictSize, u32 level, ZECDictDev* out) {
    __shared__ ZDecShared sh;
    __shared__ ZEEntropy e;
    Grp<64> g;
    ze_cdict_digest(g, sh, e, dictSize, level, out, ze_cdict_params_neg(level, dictSize));
}

// Attach-mode match finding against a dictionary, lane per frame (zj_cdict.h): the dictionary's tables and content
// are shared by every lane (L2-resident), each frame's own tables sit in its HBM slot.  Frames outside the attach
// range are left to the entropy kernel, which reports them.
__global__ __launch_bounds__(64) void zj_enc_match_dict_kernel(const u8* __restrict__ src, const u64* __restrict__ srcOff, const ZECDictDev* __restrict__ cd,
                                                                const u32* __restrict__ list, const u32* countPtr, u32* workCounter,
                                                                u8* tables, u8* fscratch, u32* meta) {
    u32 const count = *countPtr;
    u32 const cutoff = ze_attach_cutoff(cd->strategy);
    for (;;) {
        u32 const k = atomicAdd(workCounter, 1u);
        if (k >= count) break;
        u32 const i = list[k];
        u64 const s0 = srcOff[i]; u64 const size = srcOff[i + 1] - s0;
        if (size > cutoff) continue;
        ze_match_lane_dict(src + s0, (u32)size, cd, tables + (size_t)k * ZC_TABLE_STRIDE, fscratch + (size_t)k * ZE_FRAME_STRIDE(ZC_MAX_SRC), ZC_MAX_SRC, meta + 3 * (size_t)k);
    }
}
// a CDict of a negative level: the same search stepping the acceleration N (ze_dms_step; step 1 at compile time above, whose registers stay as they were)
__global__ __launch_bounds__(64) void zj_enc_match_dict_kernel_neg(const u8* __restrict__ src, const u64* __restrict__ srcOff, const ZECDictDev* __restrict__ cd,
                                                                    const u32* __restrict__ list, const u32* countPtr, u32* workCounter,
                                                                    u8* tables, u8* fscratch, u32* meta) {
    u32 const count = *countPtr;
    u32 const cutoff = ze_attach_cutoff(cd->strategy);
    u32 const step = ze_dms_step(cd->level);
    for (;;) {
        u32 const k = atomicAdd(workCounter, 1u);
        if (k >= count) break;
        u32 const i = list[k];
        u64 const s0 = srcOff[i]; u64 const size = srcOff[i + 1] - s0;
        if (size > cutoff) continue;
        ze_match_lane_dict(src + s0, (u32)size, cd, tables + (size_t)k * ZC_TABLE_STRIDE, fscratch + (size_t)k * ZE_FRAME_STRIDE(ZC_MAX_SRC), ZC_MAX_SRC, meta + 3 * (size_t)k, step);
    }
}

// Dictionary compression beyond the attach range (copy mode, zj_cdict.h): counted per call, then one wave per frame — the dictionary's
// tables copied (tags stripped) into the workgroup's HBM slot, the external-segment parse on lane 0 into the workgroup's record
// scratch, the entropy stage with the dictionary's tables as "previous block".  Such sources are rare next to the 4-16 KiB records
// dictionaries are made for; the kernel returns at once when the call has none.
__global__ __launch_bounds__(256) void zj_cdict_count_copy_kernel(const u64* __restrict__ srcOff, u32 n, const ZECDictDev* __restrict__ cd, u32* counter) {
    u32 const i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    u64 const size = srcOff[i + 1] - srcOff[i];
    if (size <= ZE_BLOCK_MAX && ze_cdict_copy_mode(cd->strategy, (u32)size, cd->contentSize)) atomicAdd(counter, 1u);
}
__global__ __launch_bounds__(64) void zj_encode_cdict_copy_kernel(const u8* __restrict__ src, const u64* __restrict__ srcOff, u8* __restrict__ dst, const u64* __restrict__ dstOff,
                                                                   u64* __restrict__ result, u32 n, const ZECDictDev* __restrict__ cd, const u32* copyCount, u32* workCounter,
                                                                   u8* scratch, u32* tables, u32 flags, u32 ldsBytes) {
    if (*copyCount == 0) return;
    __shared__ ZEncShared sh;
    __shared__ u32 metaL[4];
    ZjProf pf; pf.start(nullptr);
    Grp<64> g;
    if (threadIdx.x == 0) { sh.dictLoaded = 0; sh.ctDict[0] = 0; sh.ctDict[1] = 0; sh.ctDict[2] = 0; }
    __syncthreads();
    u8* const ws = scratch + (size_t)blockIdx.x * ZE_SCRATCH_BYTES;
    u32* const tb = tables + (size_t)blockIdx.x * (ZE_MULTI_TABLE_BYTES / 4u);
    u32 const strategy = ZJ_UNI(cd->strategy), content = ZJ_UNI(cd->contentSize);
    for (;;) {
        u32 const i = zj_next_index(workCounter);
        if (i >= n) break;
        u64 const s0 = zj_uni64(srcOff[i]), s1 = zj_uni64(srcOff[i + 1]), d0 = zj_uni64(dstOff[i]), d1 = zj_uni64(dstOff[i + 1]);
        if (s1 - s0 > ZE_BLOCK_MAX || !ze_cdict_copy_mode(strategy, (u32)(s1 - s0), content)) continue;
        u32 const size = (u32)(s1 - s0); u64 const cap = d1 - d0;
        ze_cdict_copy_tables(g, cd, tb);
        zj_mem_order();
        __syncthreads();
        if (threadIdx.x == 0) ze_cdict_copy_parse(cd, src + s0, size, tb, ws, metaL);
        zj_mem_order();
        __syncthreads();
        ZEPre pre; pre.seqs = (ZESeq*)(ws + ZE_WS_SEQ); pre.litOff = (const u32*)(ws + ZE_WS_BODY); pre.meta = metaL; pre.copyMode = 1u;
        u64 const r = ze_compress(g, sh, zj_dyn_lds, src + s0, size, dst + d0, (u32)(cap > 0xFFFFFFFFull ? 0xFFFFFFFFull : cap), ZJ_UNI(cd->level), ws, pf, &pre, flags, cd, ldsBytes);
        if (threadIdx.x == 0) result[i] = r;
        __syncthreads();
    }
}
// a CDict of a negative level: the extDict parse steps N + 1 (ze_fast_step of the CDict's word); the entropy stage takes the word too (raw literals).
// A kernel of its own so that the one above keeps its constant step and its registers.
__global__ __launch_bounds__(64) void zj_encode_cdict_copy_kernel_neg(const u8* __restrict__ src, const u64* __restrict__ srcOff, u8* __restrict__ dst, const u64* __restrict__ dstOff,
                                                                       u64* __restrict__ result, u32 n, const ZECDictDev* __restrict__ cd, const u32* copyCount, u32* workCounter,
                                                                       u8* scratch, u32* tables, u32 flags, u32 ldsBytes) {
    if (*copyCount == 0) return;
    __shared__ ZEncShared sh;
    __shared__ u32 metaL[4];
    ZjProf pf; pf.start(nullptr);
    Grp<64> g;
    if (threadIdx.x == 0) { sh.dictLoaded = 0; sh.ctDict[0] = 0; sh.ctDict[1] = 0; sh.ctDict[2] = 0; }
    __syncthreads();
    u8* const ws = scratch + (size_t)blockIdx.x * ZE_SCRATCH_BYTES;
    u32* const tb = tables + (size_t)blockIdx.x * (ZE_MULTI_TABLE_BYTES / 4u);
    u32 const strategy = ZJ_UNI(cd->strategy), content = ZJ_UNI(cd->contentSize), lw = ZJ_UNI(cd->level);
    for (;;) {
        u32 const i = zj_next_index(workCounter);
        if (i >= n) break;
        u64 const s0 = zj_uni64(srcOff[i]), s1 = zj_uni64(srcOff[i + 1]), d0 = zj_uni64(dstOff[i]), d1 = zj_uni64(dstOff[i + 1]);
        if (s1 - s0 > ZE_BLOCK_MAX || !ze_cdict_copy_mode(strategy, (u32)(s1 - s0), content)) continue;
        u32 const size = (u32)(s1 - s0); u64 const cap = d1 - d0;
        ze_cdict_copy_tables(g, cd, tb);
        zj_mem_order();
        __syncthreads();
        if (threadIdx.x == 0) ze_cdict_copy_parse(cd, src + s0, size, tb, ws, metaL, ze_fast_step(lw));
        zj_mem_order();
        __syncthreads();
        ZEPre pre; pre.seqs = (ZESeq*)(ws + ZE_WS_SEQ); pre.litOff = (const u32*)(ws + ZE_WS_BODY); pre.meta = metaL; pre.copyMode = 1u;
        u64 const r = ze_compress(g, sh, zj_dyn_lds, src + s0, size, dst + d0, (u32)(cap > 0xFFFFFFFFull ? 0xFFFFFFFFull : cap), lw, ws, pf, &pre, flags, cd, ldsBytes);
        if (threadIdx.x == 0) result[i] = r;
        __syncthreads();
    }
}

// Clears exactly the part of each frame's table slot its attach-mode parameters use (24 KiB for a 4 KiB record, not the
// 96 KiB slot): one workgroup per list entry, 16 bytes per lane per step.
__global__ __launch_bounds__(256) void zj_cdict_zero_tables_kernel(const u64* __restrict__ srcOff, const ZECDictDev* __restrict__ cd,
                                                                   const u32* __restrict__ list, const u32* countPtr, u8* tables) {
    u32 const count = *countPtr;
    ZEParams cdp; cdp.windowLog = cd->windowLog; cdp.chainLog = cd->chainLog; cdp.hashLog = cd->hashLog; cdp.minMatch = cd->minMatch; cdp.strategy = cd->strategy;
    u32 const cutoff = ze_attach_cutoff(cdp.strategy);
    for (u32 k = blockIdx.x; k < count; k += gridDim.x) {
        u32 const i = list[k];
        u64 const size = srcOff[i + 1] - srcOff[i];
        if (size < 7 || size > cutoff) continue;
        ZEParams const p = ze_attach_params(cdp, (u32)size);
        u32 const bytes = ((1u << p.hashLog) + (p.strategy == 2 ? (1u << p.chainLog) : 0u)) * 2u;
        uint4* const w = (uint4*)(tables + (size_t)k * ZC_TABLE_STRIDE);
        for (u32 j = threadIdx.x; j < bytes / 16u; j += 256) w[j] = make_uint4(0, 0, 0, 0);
    }
}

__global__ void zj_synth_kernel(u8* dst, u32 bufSize, u64 firstIndex, u32 n) {
    u32 const i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) zs_fill(dst + (size_t)i * bufSize, bufSize, firstIndex + i);
}

// Tight packing of a batch's variable-size outputs (for the multi-GPU gather): frame i moves from
// src[srcOff[i] .. +size[i]) to dst[dstOff[i] ..).  One workgroup per frame, 16 B per lane.
__global__ __launch_bounds__(256) void zj_pack_kernel(const u8* __restrict__ src, const u64* __restrict__ srcOff, const u64* __restrict__ sizes,
                                                       u8* __restrict__ dst, const u64* __restrict__ dstOff, u32 n) {
    for (u32 i = blockIdx.x; i < n; i += gridDim.x) {
        u64 const sz = sizes[i];
        if (sz > ((u64)1 << 40)) continue;              // error result: nothing to move
        const u8* s = src + srcOff[i]; u8* d = dst + dstOff[i];
        u32 const n16 = (u32)(sz >> 4);                  // (round 6 tried 16 aligned bytes per store behind a byte-wise head: 4.7 ms against 3.6 for the metric batch's 2 GB — not kept)
        for (u32 k = threadIdx.x; k < n16; k += 256) { u64 a = ld64(s + 16 * k), b = ld64(s + 16 * k + 8); st64(d + 16 * k, a); st64(d + 16 * k + 8, b); }
        for (u32 k = (n16 << 4) + threadIdx.x; k < (u32)sz; k += 256) d[k] = s[k];
    }
}

// ============================================================================ host state =======
namespace {
#define ZJ_ENC_LDS_BIG 131072u
// pass-0 LDS per level: the tables of > 16 KiB inputs up to 64 KiB (u16 positions)
#define ZJ_BIG_SLICE ((size_t)16384)    /* frames of 16-128 KiB at levels 4-8 per pass of the lane-per-frame route (655 KiB of records each) */
#define ZJ_LEVEL_MAX 8                 /* levels 1-3 on every path; level 4 (inputs <= 128 KiB) and levels 5-8 (<= 16 KiB), no dictionary, no explicit table sizes, on the HBM-table kernel */
#define ZJ_LEVEL_MIN (-131072)         /* ZSTD_minCLevel() = -ZSTD_TARGETLENGTH_MAX: lower levels are clamped to it, as the reference clamps them */
// the levels the batch entries serve: 1..ZJ_LEVEL_MAX, and every negative level (zstd's --fast=N: the fast strategy with step N + 1 and raw literals,
// on the paths of level 1 — no explicit table sizes; CDicts and streams at these levels: zjni_createCDict, zjni_compress_stream*).  0 means 3 and is mapped by the caller.
static inline bool zj_level_served(int level) { return level < 0 || (level >= 1 && level <= ZJ_LEVEL_MAX); }
// a negative level's word (zj_encode.h: ZE_LW_NEG, the acceleration clamped as ZSTD_minCLevel() clamps it); other levels stay as they are
static inline int zj_negative_word(int level) { return level < 0 ? (int)ZE_LW_NEGATIVE((u32)(level < ZJ_LEVEL_MIN ? -ZJ_LEVEL_MIN : -level)) : level; }
size_t enc_lds_pass0(int level) {
    size_t const need = level == 1 ? (8192u * 2u) : (level == 2 ? (32768u * 2u) : (((1u << ZE_L3_HASHLOG) + (1u << ZE_L3_CHAINLOG)) * 2u));
    return need > sizeof(ZEEntropy) ? need : sizeof(ZEEntropy);
}
enum { ZJ_ROUTE_WAVE_HBM = ZJNI_ROUTE_WAVE_HBM, ZJ_ROUTE_FUSED = ZJNI_ROUTE_FUSED, ZJ_ROUTE_WAVE = ZJNI_ROUTE_WAVE, ZJ_ROUTE_LANE = ZJNI_ROUTE_LANE, ZJ_ROUTE_LANE_GATED = ZJNI_ROUTE_LANE_GATED,
       ZJ_ROUTE_RUN = ZJNI_ROUTE_RUN, ZJ_ROUTE_RUN_FLAGS = ZJNI_ROUTE_RUN_FLAGS, ZJ_ROUTE_HYBRID = ZJNI_ROUTE_HYBRID, ZJ_ROUTE_OTHER = ZJNI_ROUTE_OTHER };
// HIP maps a process's streams onto GPU_MAX_HW_QUEUES hardware queues per device (4 by default), and a hardware queue runs its packets in order: a stream that shares
// one with the stream of a 130 ms persistent kernel (the entropy kernel beside the match kernel, the match kernel itself) does not move until that kernel has left —
// measured with two host batches in flight: the second batch's pack kernel and D2H copies waited 130 ms behind the first's entropy kernel (profiles/r05/e_).  This
// library keeps up to ten streams busy at once (a caller's, three of its own per device, three per staging slot): a deployment that keeps two host batches in flight
// sets GPU_MAX_HW_QUEUES=16 in the environment the process is STARTED with.  The library itself never touches the environment: it is
// dlopen()ed into a running JVM, where setenv() races with every other thread's getenv() (rounds 4-5 called setenv from a static initialiser here).
// The host-pointer entries stage a batch through pinned host memory and a device area of the same layout.  Round 5: TWO such slots per device, each with its own
// streams and events, so that two host-pointer calls (two JVM threads in compressBatch0, or zjni_*_batch_begin twice) are in flight at once: while one call's kernels run,
// the other's sources cross the link one way and a third's frames the other — the lane pipeline wants a whole batch resident, so the overlap a single compress call cannot
// have (H2D 75 + kernels 143 + D2H 35 ms in sequence on the metric batch) comes from the next call.  The kernels of the two calls still follow each other (BatchOrder: they
// share the per-device scratch).  A third concurrent call waits for a slot.
#define ZJ_STAGE_SLOTS 2
struct StageSlot {
    std::mutex mu;
    u8* hPinned = nullptr; size_t hPinnedCap = 0;
    u8* dStage = nullptr; size_t dStageCap = 0;
    hipStream_t hostIn = nullptr, hostK = nullptr, hostOut = nullptr;       // H2D / kernels / D2H (the decompress entry runs slices of one call on all three at once: PCIe is full duplex)
    std::vector<hipEvent_t> stageEv;                  // one event per returned slice (compress)
    std::vector<hipEvent_t> pipeEv;                   // three events per slice: source landed, decoded, returned (decompress)
};
struct DevState {
    bool needLdsSet = false;                      // zj_enc_need_kernel's LDS attribute has been set on this device
    int lastRoute = 0;                            // ZJNI_ROUTE_* of the last large compress call (zjni_last_route)
    int ordinal = -1;
    int numCU = 0;
    int decGrid = 0, decDictGrid = 0, encGrid = 0;          // encGrid = largest encoder grid (level-1 LDS)
    int encGridLvl[4] = {0, 0, 0, 0};     // resident workgroups per level for pass 0
    int encGridBig = 0;                    // pass 1 (128 KiB LDS)
    int encGridSmall = 0;                  // entropy stage with small frames staged in LDS (ZE_SMALL_LDS_BYTES)
    // dictionary compress: slice s's entropy kernel (side stream) runs beside slice s+1's match kernel; two sets of records / lists / counters
    u8* wideBuf = nullptr; size_t wideBufCap = 0;     // lane-per-frame path of list B: [tables][frame scratch][meta] for one slice
    StageSlot* slot[ZJ_STAGE_SLOTS] = {};             // host-pointer entries: their staging areas, streams and events (below)
    std::atomic<unsigned>* slotTicket = nullptr;
    std::mutex* hostDecompMu = nullptr;
    u32* multiTables = nullptr; int multiGrid = 0;    // multi-block frames: frame-wide hash tables, one set per resident workgroup
    int seqGrid = 0;                                  // resident workgroups of zj_encode_sequences_kernel (0: not asked yet)
    const u8* genCounters = nullptr; u32 genFrames = 0;     // the last generate call: where its counters are (framesBuf as it was then) and its frames (zjni_last_generate)
    int contGrid = 0;                                 // resident workgroups of zj_encode_stream_continue_kernel (0: not asked yet)
    u32 lastPipeMax = 0;                              // what the last compress call passed to zj_pipe_route (diagnostics: zjni_last_lists)
    int pipeGrid = 0;                                 // ... and the resident workgroups of the pipelined kernel (two waves, two scratch slots each); 0: not available
    u8* cdBuf = nullptr; size_t cdBufCap = 0; size_t cdSliceCap = 0;
    u32* cdList = nullptr; size_t cdListCap = 0;
    hipEvent_t cdMatchDone[2] = {}, cdEncDone[2] = {};
    u32* counters = nullptr;       // [0] decode, [16] encode (separate cache lines)
    u8* decScratch = nullptr; int dseqHeavy = 0;
    volatile u32* encStat = nullptr; hipEvent_t evLists = nullptr;      // pinned: the classify kernel's list counts of the running compress call ([0] |A|, [1] |B|, [4] |C|), valid behind evLists — asked for only while the wide slice does not exist
    volatile u32* decStat = nullptr;                  // pinned: [0] |A|, [1] sequences of the last split-decode slice that ran (copied back asynchronously, read without waiting)
    u8* encScratch = nullptr;
    // staging for the host-pointer entries
    unsigned long long* prof = nullptr;    // 32 phase counters (16 decode + 16 encode) when ZJNI_PROFILE is set
    u32* encList = nullptr; size_t encListCap = 0;   // two index lists of encListCap entries each
    u8* splitBuf = nullptr; size_t splitBufCap = 0;    // lane-per-frame path: [tables][frame scratch][meta]
    int matchGrid = 0;
    int dseqGrid = 0, dexecGrid = 0, dlitGrid = 0;                  // split decode pipeline
    hipEvent_t tev[12] = {};                          // stage boundaries of the last batch calls (zjni_last_timing): [0,1] match, [2..6] decode stages, [8,9] wide match (last slice)
    bool tevWide = false;
    bool tevCompress = false, tevDecompress = false;
    hipStream_t sideStream = nullptr; hipEvent_t evFork = nullptr, evJoin = nullptr;
    hipStream_t waveStream = nullptr; hipEvent_t evJoinWave = nullptr; int waveGrid = 0;   // wave-per-frame matcher beside the lane-per-frame one
    // Level-3 tables of the lane pipeline (n x 384 KiB: 24 GiB for 65 536 frames) have to be zero when a call's match kernel starts.  Clearing them is
    // 5-6 ms of pure HBM writes in front of a kernel that waits on latency; so a call clears them for the NEXT one as soon as its own match
    // kernel is done, on a stream of its own (beside its entropy tail and whatever the host does next), and the next call over the same range
    // only waits for that.  clearedValid: the range [clearedPtr, + clearedBytes) is zero, or will be when evCleared fires.
    hipStream_t clearStream = nullptr; hipEvent_t evMatchDone = nullptr, evCleared = nullptr; u8* clearedPtr = nullptr; size_t clearedBytes = 0; bool clearedValid = false;
    // batch calls share the per-device scratch: they are enqueued under `enqueueMu`, and each call's kernels wait (on the
    // GPU) for the previous call's last kernel, whatever streams the callers use — many host threads may call at once
    std::mutex* enqueueMu = nullptr; hipEvent_t lastDone = nullptr; bool lastValid = false;
    u8* dsplitBuf = nullptr; size_t dsplitBufCap = 0;  // [tables][sequences][frame records][list A][list B]
    u8* dlitBuf = nullptr; size_t dlitBufCap = 0;      // literal slots of the split decode pipeline (stage 2b), one per frame of a slice
    u8* dmbBuf = nullptr; size_t dmbBufCap = 0;        // multi-block frames on the split pipeline: [block tables][blocks][frames][seq list][list M][record pool]
    u64* slotPart = nullptr; size_t slotPartCap = 0;   // zjni_decompress_offsets_device: one partial sum per 1 024 buffers (8 B each; not counted as pipeline scratch)
    // large buffers as many frames (zj_frames.h): the per-buffer and per-entry arrays of zjni_decompress_frames_batch_device / zjni_compress_chunked_batch_device and the
    // chunked compress's scratch destinations; counts as scratch, but is not evicted by scratch_free_all (the pipelines run inside these calls, which hold it)
    u8* framesBuf = nullptr; size_t framesBufCap = 0;
    u32* framesStat = nullptr;                         // device: [0] buffers split, [1] not split, [2] buffers on the redo list, [3] work counter of the redo launch
    volatile u64* framesE = nullptr; hipEvent_t evFramesE = nullptr;      // pinned: the entry count of the running call, valid behind evFramesE
    u64 lastFramesE = 0;                               // entries the last zjni_decompress_frames_batch_device decoded (zjni_last_frames)
};
std::mutex g_mu;        // guards g_dev
std::vector<DevState> g_dev;
thread_local int t_dev = -1;

int dev_count() {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

DevState* get_state(int ordinal) {
    std::lock_guard<std::mutex> lk(g_mu);
    int const n = dev_count();
    if (n <= 0 || ordinal < 0 || ordinal >= n) return nullptr;
    if ((int)g_dev.size() < n) g_dev.resize(n);
    DevState& d = g_dev[ordinal];
    if (hipSetDevice(ordinal) != hipSuccess) return nullptr;
    if (d.ordinal < 0) {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, ordinal) != hipSuccess) return nullptr;
        d.numCU = prop.multiProcessorCount;
        int perCU = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&perCU, zj_decode_kernel, 64, 0) != hipSuccess || perCU < 1) perCU = 8;
        d.decGrid = d.numCU * perCU;
        {   int p2 = 0; if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&p2, zj_decode_dict_kernel, 64, 0) != hipSuccess || p2 < 1) p2 = 4;
            d.decDictGrid = d.numCU * (p2 < perCU ? p2 : perCU); }
        if (const char* ov = zj_tune("ZJNI_DEBUG_WG_PER_CU")) { int const v = atoi(ov); if (v >= 1 && v < perCU) d.decGrid = d.numCU * v; }   // occupancy experiments
        if (hipFuncSetAttribute((const void*)zj_encode_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ZJ_ENC_LDS_BIG) != hipSuccess) return nullptr;
        for (int lvl = 1; lvl <= 3; lvl++) {
            if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&perCU, zj_encode_kernel, 64, enc_lds_pass0(lvl)) != hipSuccess || perCU < 1) perCU = 1;
            d.encGridLvl[lvl] = d.numCU * perCU;
            if (const char* ov = zj_tune("ZJNI_DEBUG_WG_PER_CU")) { int const v = atoi(ov); if (v >= 1 && v < perCU) d.encGridLvl[lvl] = d.numCU * v; }
            if (d.encGridLvl[lvl] > d.encGrid) d.encGrid = d.encGridLvl[lvl];
        }
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&perCU, zj_encode_kernel, 64, ZJ_ENC_LDS_BIG) != hipSuccess || perCU < 1) perCU = 1;
        d.encGridBig = d.numCU * perCU;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&perCU, zj_encode_kernel, 64, ZE_SMALL_LDS_BYTES) != hipSuccess || perCU < 1) perCU = 1;
        d.encGridSmall = d.numCU * perCU;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&perCU, zj_enc_match_kernel, 64, 0) != hipSuccess || perCU < 1) perCU = 4;
        d.matchGrid = d.numCU * perCU;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&perCU, zj_dec_seq_kernel, 64, 0) != hipSuccess || perCU < 1) perCU = 4;
        d.dseqGrid = d.numCU * perCU;
        // Resident waves of the sequence decode when the execution kernel runs beside it (zj_dec_heavy).  A lane takes its next frame from
        // a counter, so fewer waves than frames / 64 only means more frames per lane; the pipeline's time is flat from 1 to 2 waves per CU
        // (24.7-25.3 ms per 65 536 x 64 KiB) and the decode cells alive at a time shrink with the wave count: 1.5 waves per CU.
        d.dseqHeavy = d.numCU * 3 / 2;
        if (const char* ov = zj_tune("ZJNI_DSEQ_WAVES")) { int const v = atoi(ov); if (v >= 1) d.dseqHeavy = v; }
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&perCU, zj_dec_exec_kernel, 64, ZD_SHARED_NO_FSE) != hipSuccess || perCU < 1) perCU = 8;
        d.dexecGrid = d.numCU * perCU;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&perCU, zj_dec_lit_kernel, 64, ZD_EXEC_LDS) != hipSuccess || perCU < 1) perCU = 8;
        d.dlitGrid = d.numCU * perCU;
        for (auto& e : d.tev) { if (hipEventCreate(&e) != hipSuccess) return nullptr; }
        d.enqueueMu = new std::mutex(); d.slotTicket = new std::atomic<unsigned>(0); d.hostDecompMu = new std::mutex();
        for (int k = 0; k < ZJ_STAGE_SLOTS; k++) d.slot[k] = new StageSlot();
        if (hipEventCreateWithFlags(&d.lastDone, hipEventDisableTiming) != hipSuccess) return nullptr;
        if (hipStreamCreateWithFlags(&d.sideStream, hipStreamNonBlocking) != hipSuccess) return nullptr;
        if (hipEventCreateWithFlags(&d.evFork, hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&d.evJoin, hipEventDisableTiming) != hipSuccess) return nullptr;
        if (hipMalloc(&d.counters, 1024) != hipSuccess) return nullptr;
        if (hipStreamCreateWithFlags(&d.waveStream, hipStreamNonBlocking) != hipSuccess || hipEventCreateWithFlags(&d.evJoinWave, hipEventDisableTiming) != hipSuccess) return nullptr;
        if (hipStreamCreateWithFlags(&d.clearStream, hipStreamNonBlocking) != hipSuccess || hipEventCreateWithFlags(&d.evMatchDone, hipEventDisableTiming) != hipSuccess
            || hipEventCreateWithFlags(&d.evCleared, hipEventDisableTiming) != hipSuccess) return nullptr;
        if (hipFuncSetAttribute((const void*)zj_enc_match_wave_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(ZWLds)) != hipSuccess) return nullptr;
        {   int w = 3; if (const char* ov = zj_tune("ZJNI_WAVE_PER_CU")) { int const v = atoi(ov); if (v >= 1 && v <= 3) w = v; }
            d.waveGrid = d.numCU * w; }
        for (int p = 0; p < 2; p++) if (hipEventCreateWithFlags(&d.cdMatchDone[p], hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&d.cdEncDone[p], hipEventDisableTiming) != hipSuccess) return nullptr;
        {   void* hp = nullptr; if (hipHostMalloc(&hp, 64, hipHostMallocDefault) == hipSuccess) { memset(hp, 0, 64); d.decStat = (volatile u32*)hp; } }
        {   void* hp = nullptr; if (hipHostMalloc(&hp, 64, hipHostMallocDefault) == hipSuccess && hipEventCreateWithFlags(&d.evLists, hipEventDisableTiming) == hipSuccess) { memset(hp, 0, 64); d.encStat = (volatile u32*)hp; } }
        if (hipMalloc(&d.decScratch, (size_t)(d.decGrid > d.dexecGrid ? d.decGrid : d.dexecGrid) * ZD_LIT_SCRATCH) != hipSuccess) return nullptr;
        if (hipMalloc(&d.encScratch, (size_t)d.encGrid * ZE_SCRATCH_BYTES) != hipSuccess) return nullptr;
        if (zj_tune("ZJNI_PROFILE")) { if (hipMalloc(&d.prof, 32 * 8) != hipSuccess || hipMemset(d.prof, 0, 32 * 8) != hipSuccess) return nullptr; }
        d.ordinal = ordinal;
    }
    return &d;
}

DevState* cur_state() {
    if (t_dev < 0) {
        int cur = 0;
        if (dev_count() <= 0) return nullptr;
        if (hipGetDevice(&cur) != hipSuccess) return nullptr;
        t_dev = cur;
    }
    return get_state(t_dev);
}

// ---- scratch budget (zjni_set_scratch_limit) ----
// The pipelines keep per-frame scratch in HBM (hash tables, sequence records, decode cells): four buffers per device, one per
// pipeline, allocated on first use and kept.  With a limit set, a batch is cut into slices whose scratch fits and a buffer that
// has to grow first evicts the other pipelines' buffers (after the device has drained).  0 = no limit (sized for 288 GB).
size_t g_scratch_limit = 0;
#define ZJ_SCRATCH_LIMIT_MIN ((size_t)4 << 30)
size_t scratch_total(const DevState* d) { return d->splitBufCap + d->wideBufCap + d->cdBufCap + d->dsplitBufCap + d->dlitBufCap + d->dmbBufCap + d->framesBufCap; }
void scratch_free_all(DevState* d) {
    d->clearedValid = false;                                    // (hipFree drains the device, the clear stream included)
    if (d->splitBuf) (void)hipFree(d->splitBuf); d->splitBuf = nullptr; d->splitBufCap = 0;
    if (d->wideBuf) (void)hipFree(d->wideBuf); d->wideBuf = nullptr; d->wideBufCap = 0;
    if (d->cdBuf) (void)hipFree(d->cdBuf); d->cdBuf = nullptr; d->cdBufCap = 0; d->cdSliceCap = 0;
    if (d->dsplitBuf) (void)hipFree(d->dsplitBuf); d->dsplitBuf = nullptr; d->dsplitBufCap = 0;
    if (d->dmbBuf) (void)hipFree(d->dmbBuf); d->dmbBuf = nullptr; d->dmbBufCap = 0;
    if (d->dlitBuf) (void)hipFree(d->dlitBuf); d->dlitBuf = nullptr; d->dlitBufCap = 0;
}
// before a buffer holding `have` bytes is replaced by one of `need` bytes: false when even alone it would exceed the limit
bool scratch_make_room(DevState* d, size_t have, size_t need) {
    if (!g_scratch_limit) return true;
    if (need > g_scratch_limit) return false;
    if (scratch_total(d) - have + need <= g_scratch_limit) return true;
    if (hipDeviceSynchronize() != hipSuccess) return false;      // other pipelines' kernels may still be using what is about to go
    scratch_free_all(d);
    return true;
}
// frames per slice such that `perFrame` bytes of scratch each stay inside `share` of the limit (at least 4 096: below that the
// fused kernels run, which keep their scratch per workgroup)
size_t scratch_slice(size_t perFrame, size_t dflt, size_t shareDiv) {
    if (!g_scratch_limit) return dflt;
    size_t const f = (g_scratch_limit / shareDiv) / (perFrame ? perFrame : 1);
    return f < 4096 ? 4096 : (f < dflt ? f : dflt);
}

bool ensure_staging(StageSlot* d, size_t bytes) {
    if (!d->hostK) {
        if (hipStreamCreateWithFlags(&d->hostIn, hipStreamNonBlocking) != hipSuccess || hipStreamCreateWithFlags(&d->hostK, hipStreamNonBlocking) != hipSuccess
            || hipStreamCreateWithFlags(&d->hostOut, hipStreamNonBlocking) != hipSuccess) { d->hostIn = d->hostK = d->hostOut = nullptr; return false; }
    }
    if (d->hPinnedCap < bytes) {
        if (d->hPinned) (void)hipHostFree(d->hPinned);
        if (d->dStage) (void)hipFree(d->dStage);
        d->hPinned = nullptr; d->dStage = nullptr; d->hPinnedCap = d->dStageCap = 0;
        size_t const cap = bytes + (bytes >> 2) + (1u << 20);
        if (hipHostMalloc(&d->hPinned, cap, hipHostMallocDefault) != hipSuccess) return false;
        if (hipMalloc(&d->dStage, cap) != hipSuccess) return false;
        d->hPinnedCap = d->dStageCap = cap;
    }
    return true;
}
// a free slot of the device, or the next one in turn when both are taken (held until the guard goes)
struct SlotLock {
    StageSlot* s = nullptr;
    explicit SlotLock(DevState* d) {
        for (int k = 0; k < ZJ_STAGE_SLOTS && !s; k++) if (d->slot[k]->mu.try_lock()) s = d->slot[k];
        if (!s) { s = d->slot[d->slotTicket->fetch_add(1u) % ZJ_STAGE_SLOTS]; s->mu.lock(); }
    }
    ~SlotLock() { if (s) s->mu.unlock(); }
    SlotLock(const SlotLock&) = delete; SlotLock& operator=(const SlotLock&) = delete;
};
// One host buffer through a staging slot, blocking: the slot (held until the guard goes), `total` bytes of its staging areas, and a drain of its kernel stream on
// the way out — an error return leaves copies in flight on the staging area: none when the slot is given back.  A region has the same offset on both sides.
struct StagedCall {
    SlotLock lock;
    bool const ready;                                 // false: no staging area (the caller answers ZJNI_ERROR_unsupported)
    u8* const host; u8* const dev; hipStream_t const st;
    StagedCall(DevState* d, size_t total) : lock(d), ready(ensure_staging(lock.s, total)), host(lock.s->hPinned), dev(lock.s->dStage), st(lock.s->hostK) {}
    ~StagedCall() { if (ready) (void)hipStreamSynchronize(st); }
    u64* words() const { return (u64*)host; }
    // the first k bytes (header words, source) to the device; no wait
    bool upload(size_t k) { return hipMemcpyAsync(dev, host, k, hipMemcpyHostToDevice, st) == hipSuccess; }
    // header words [w0, w0 + k) back, and a wait
    bool fetch(size_t w0, size_t k) {
        return hipMemcpyAsync(host + w0 * 8, dev + w0 * 8, k * 8, hipMemcpyDeviceToHost, st) == hipSuccess && hipStreamSynchronize(st) == hipSuccess;
    }
    // regions back into the caller's buffers behind one wait
    struct Span { void* to; size_t off, bytes; };
    bool download(std::initializer_list<Span> spans) {
        for (const Span& s : spans) if (s.bytes && hipMemcpyAsync(host + s.off, dev + s.off, s.bytes, hipMemcpyDeviceToHost, st) != hipSuccess) return false;
        if (hipStreamSynchronize(st) != hipSuccess) return false;
        for (const Span& s : spans) if (s.bytes) memcpy(s.to, host + s.off, s.bytes);
        return true;
    }
    // what the entries with one result word and one payload end on: the word's checks, then its bytes out
    size_t payload(size_t res, void* dst, size_t dstCap, size_t oDst) {
        if (zjni_isError(res) || res == 0) return res;
        if (res > dstCap) return ZJNI_ERR(ZJNI_ERROR_no_device);
        return download({{dst, oDst, res}}) ? res : ZJNI_ERR(ZJNI_ERROR_no_device);
    }
};
// Host-side copies of the host-pointer entries (caller's buffers <-> pinned staging) run on a few threads: one memcpy stream moves
// ~10 GB/s, the PCIe link 57 each way — every byte of a batch is copied once by the host on each side, so these copies, not the link,
// bound the entries unless enough threads share them.  Default: the CPUs this process may really use (scheduler affinity and the cgroup
// quota, not the processors the box shows), at most 16; ZJNI_HOST_THREADS overrides (1 = the calling thread only).
#define ZJ_HOST_SLICE ((u64)256 << 20)
static int host_threads() {
    static int const t = []() {
        if (const char* ov = zj_env("ZJNI_HOST_THREADS")) { int const v = atoi(ov); return v < 1 ? 1 : (v > 64 ? 64 : v); }
        long v = 16;
        cpu_set_t set; CPU_ZERO(&set);
        if (sched_getaffinity(0, sizeof(set), &set) == 0) { long const a = CPU_COUNT(&set); if (a >= 1 && a < v) v = a; }
        if (FILE* f = fopen("/sys/fs/cgroup/cpu.max", "r")) {                    // cgroup v2: "<quota> <period>" or "max <period>"
            char q[32]; long per = 0;
            if (fscanf(f, "%31s %ld", q, &per) == 2 && strcmp(q, "max") != 0 && per > 0) { long const c = (atol(q) + per - 1) / per; if (c >= 1 && c < v) v = c; }
            fclose(f);
        }
        return (int)(v < 1 ? 1 : v);
    }();
    return t;
}
// fn(lo, hi) over index ranges of about equal bytes; off[0..n] = byte offsets of the items; `threads` = 0: host_threads()
template <class F>
static void par_ranges(const u64* off, size_t n, F fn, int threads = 0) {
    u64 const total = off[n] - off[0];
    int T = total < ((u64)8 << 20) ? 1 : (threads > 0 ? threads : host_threads());
    if ((size_t)T > n) T = (int)(n ? n : 1);
    if (T <= 1) { fn((size_t)0, n); return; }
    std::vector<size_t> cut((size_t)T + 1, n); cut[0] = 0;
    for (int t = 1; t < T; t++) cut[(size_t)t] = (size_t)(std::lower_bound(off, off + n + 1, off[0] + total / (u64)T * (u64)t) - off);
    for (int t = 1; t <= T; t++) if (cut[(size_t)t] < cut[(size_t)t - 1]) cut[(size_t)t] = cut[(size_t)t - 1];
    std::vector<std::thread> th;
    for (int t = 1; t < T; t++) th.emplace_back([&, t]() { fn(cut[(size_t)t], cut[(size_t)t + 1]); });
    fn(cut[0], cut[1]);
    for (auto& x : th) x.join();
}

}  // namespace

// ============================================================================ C-ABI ============
extern "C" {

const char* zjni_version(void) { return ZJNI_VERSION_STRING; }
int zjni_device_count(void) { return dev_count(); }

int zjni_init(int ordinal) {
    if (dev_count() <= 0) return -(int)ZJNI_ERROR_no_device;
    DevState* d = get_state(ordinal);
    if (!d) return -(int)ZJNI_ERROR_no_device;
    t_dev = ordinal;
    return 0;
}

void zjni_shutdown(void) {
    std::lock_guard<std::mutex> lk(g_mu);
    for (auto& d : g_dev) {
        if (d.ordinal < 0) continue;
        (void)hipSetDevice(d.ordinal);
        (void)hipFree(d.counters); if (d.decStat) { (void)hipHostFree((void*)d.decStat); d.decStat = nullptr; } if (d.encStat) { (void)hipHostFree((void*)d.encStat); d.encStat = nullptr; (void)hipEventDestroy(d.evLists); } (void)hipFree(d.decScratch); (void)hipFree(d.encScratch);
        if (d.encList) (void)hipFree(d.encList);
        if (d.splitBuf) (void)hipFree(d.splitBuf);
        if (d.dsplitBuf) (void)hipFree(d.dsplitBuf);
        if (d.dmbBuf) (void)hipFree(d.dmbBuf);
        if (d.dlitBuf) (void)hipFree(d.dlitBuf);
        if (d.wideBuf) (void)hipFree(d.wideBuf);
        if (d.multiTables) (void)hipFree(d.multiTables);
        if (d.cdBuf) (void)hipFree(d.cdBuf);
        if (d.cdList) (void)hipFree(d.cdList);
        if (d.slotPart) (void)hipFree(d.slotPart);
        if (d.framesBuf) (void)hipFree(d.framesBuf);
        if (d.framesStat) (void)hipFree(d.framesStat);
        if (d.framesE) { (void)hipHostFree((void*)d.framesE); (void)hipEventDestroy(d.evFramesE); }
        for (int p = 0; p < 2; p++) { if (d.cdMatchDone[p]) (void)hipEventDestroy(d.cdMatchDone[p]); if (d.cdEncDone[p]) (void)hipEventDestroy(d.cdEncDone[p]); }
        if (d.sideStream) { (void)hipStreamDestroy(d.sideStream); (void)hipEventDestroy(d.evFork); (void)hipEventDestroy(d.evJoin); }
        if (d.clearStream) { (void)hipStreamDestroy(d.clearStream); (void)hipEventDestroy(d.evMatchDone); (void)hipEventDestroy(d.evCleared); }
        for (int k = 0; k < ZJ_STAGE_SLOTS; k++) if (StageSlot* const sl = d.slot[k]) {
            if (sl->hostIn) { (void)hipStreamDestroy(sl->hostIn); (void)hipStreamDestroy(sl->hostK); (void)hipStreamDestroy(sl->hostOut); }
            for (hipEvent_t e : sl->pipeEv) if (e) (void)hipEventDestroy(e);
            for (hipEvent_t e : sl->stageEv) if (e) (void)hipEventDestroy(e);
            if (sl->hPinned) (void)hipHostFree(sl->hPinned);
            if (sl->dStage) (void)hipFree(sl->dStage);
            delete sl;
        }
        if (d.waveStream) { (void)hipStreamDestroy(d.waveStream); (void)hipEventDestroy(d.evJoinWave); }
        d = DevState();
    }
}

unsigned zjni_isError(size_t r) { return r > ZJNI_ERR(256) ? 1u : 0u; }
int zjni_getErrorCode(size_t r) { return zjni_isError(r) ? (int)(0 - r) : 0; }
const char* zjni_getErrorName(size_t r) {
    // strings are libzstd's (N/common/error_private.c:15-65) so Java-side message checks keep passing
    switch (zjni_getErrorCode(r)) {
    case 0: return "No error detected";
    case 1: return "Error (generic)";
    case 10: return "Unknown frame descriptor";
    case 14: return "Unsupported frame parameter";
    case 16: return "Frame requires too much memory for decoding";
    case 20: return "Data corruption detected";
    case 22: return "Restored data doesn't match checksum";
    case 24: return "Header of Literals' block doesn't respect format specification";
    case 30: return "Dictionary is corrupted";
    case 32: return "Dictionary mismatch";
    case 40: return "Unsupported parameter";
    case 42: return "Parameter is out of bound";
    case 44: return "tableLog requires too much memory : unsupported";
    case 64: return "Allocation error : not enough memory";
    case 70: return "Destination buffer is too small";
    case 72: return "Src size is incorrect";
    case 200: return "zjni: no gfx950 device available";
    case 201: return "zjni: input outside the GPU path (use the CPU path)";
    default: return "Unspecified error code";
    }
}

size_t zjni_compressBound(size_t s) {
    return s + (s >> 8) + (s < (128u << 10) ? (((128u << 10) - s) >> 11) : 0);
}

unsigned long long zjni_getFrameContentSize(const void* srcv, size_t srcSize) {
    // N/decompress/zstd_decompress.c:447-557 / :588-603
    const u8* p = (const u8*)srcv;
    if (srcSize < 5) return (unsigned long long)-2;
    u32 const magic = ld32(p);
    if (magic != 0xFD2FB528u)       // a skippable frame needs its 8-byte header present (:476-478), then counts as size 0 (:596)
        return ((magic & 0xFFFFFFF0u) == 0x184D2A50u && srcSize >= 8) ? 0ull : (unsigned long long)-2;
    u32 const fhd = p[4], didc = fhd & 3, single = (fhd >> 5) & 1, fcsid = fhd >> 6;
    u32 const didSz = didc == 3 ? 4 : didc, fcsSz = fcsid == 0 ? single : (1u << fcsid);
    size_t pos = 5 + !single + didSz;
    if (srcSize < pos + fcsSz || (fhd & 8)) return (unsigned long long)-2;
    if (!single && (p[5] >> 3) + 10u > 31u) return (unsigned long long)-2;     // windowLog > ZSTD_WINDOWLOG_MAX (:517)
    if (fcsid == 0) return single ? p[pos] : (unsigned long long)-1;
    if (fcsid == 1) return ld16(p + pos) + 256;
    if (fcsid == 2) return ld32(p + pos);
    return ld64(p + pos);
}

/* debugging/profiling aid (not in the public header): copies the 32 phase-cycle counters and clears them */
int zjni_debug_read_profile(unsigned long long* out32) {
    DevState* d = cur_state();
    if (!d || !d->prof) return -1;
    if (hipMemcpy(out32, d->prof, 32 * 8, hipMemcpyDeviceToHost) != hipSuccess) return -1;
    return hipMemset(d->prof, 0, 32 * 8) == hipSuccess ? 0 : -1;
}

/* Stage durations (ms) of the last large-batch device calls on this device, from HIP events recorded on the
 * caller's stream around the kernels: out[0] match-finder kernel (compress); out[1..4] decode stages prep /
 * sequence decode / execute / fused leftovers.  Blocks until those events have completed; entries whose stage
 * did not run are -1.  A profiling aid for bench.py's roofline line, not part of the data path. */
int zjni_last_timing(float* out5) {
    DevState* d = cur_state();
    if (!d) return -(int)ZJNI_ERROR_no_device;
    for (int i = 0; i < 5; i++) out5[i] = -1.0f;
    if (d->tevCompress) { if (hipEventSynchronize(d->tev[1]) == hipSuccess) (void)hipEventElapsedTime(&out5[0], d->tev[0], d->tev[1]); }
    if (d->tevDecompress && hipEventSynchronize(d->tev[6]) == hipSuccess) {
        for (int i = 0; i < 4; i++) (void)hipEventElapsedTime(&out5[1 + i], d->tev[2 + i], d->tev[3 + i]);
    }
    return 0;
}

/* the same five durations plus out8[5] = the wide match-finder kernel (frames > 64 KiB; last slice of the call); out8[6..7] reserved (-1) */
int zjni_last_timing2(float* out8) {
    DevState* d = cur_state();
    int const r = zjni_last_timing(out8);
    if (r) return r;
    out8[5] = out8[6] = out8[7] = -1.0f;
    if (d->tevWide && hipEventSynchronize(d->tev[9]) == hipSuccess) (void)hipEventElapsedTime(&out8[5], d->tev[8], d->tev[9]);
    return 0;
}

int zjni_last_route(void) { DevState* d = cur_state(); return d ? d->lastRoute : -(int)ZJNI_ERROR_no_device; }
// The last large compress call's three lists as the classification kernel filled them — out3[0] frames of the common launch (list A: what zjni_last_route names),
// out3[1] frames of the wide launch (list B: frames above 64 KiB, zj_enc_match_wide_kernel = ZJNI_ROUTE_WIDE), out3[2] frames of the multi-block / wave-per-frame
// kernel (list C).  Waits for the device: a diagnostic for benches and tests, not for the data path.
int zjni_last_lists(unsigned* out3) {
    DevState* d = cur_state();
    if (!d || !out3) return -(int)ZJNI_ERROR_no_device;
    u32 h[8];
    if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(h, d->counters + 16, sizeof h, hipMemcpyDeviceToHost) != hipSuccess) return -(int)ZJNI_ERROR_no_device;
    out3[0] = h[0]; out3[1] = h[1]; out3[2] = h[4];
    if (d->lastRoute == ZJ_ROUTE_WAVE_HBM && d->lastPipeMax && h[4] && h[4] <= d->lastPipeMax && 2u * h[6] >= h[4]) d->lastRoute = ZJNI_ROUTE_PIPE;      // zj_pipe_route, restated for the diagnostics
    return 0;
}
// The last large decompress call: out4[0] frames of the single-block pipeline (list A), out4[1] frames the fused kernel decoded (list B: what no pipeline took, or
// handed over), out4[2] frames of the multi-block stages (list M), out4[3] their blocks.  Waits for the device (diagnostics: benches, tests).
int zjni_last_decode_lists(unsigned* out4) {
    DevState* d = cur_state();
    if (!d || !out4) return -(int)ZJNI_ERROR_no_device;
    u32 a[12], m[8];
    if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(a, d->counters + 32, sizeof a, hipMemcpyDeviceToHost) != hipSuccess
        || hipMemcpy(m, d->counters + 232, sizeof m, hipMemcpyDeviceToHost) != hipSuccess) return -(int)ZJNI_ERROR_no_device;
    out4[0] = a[8]; out4[1] = a[1]; out4[2] = m[2]; out4[3] = m[0];
    return 0;
}
// ... and out5[4]: frames of one stored (raw / RLE) block that stage 1 copied itself (round 6; they are on none of the three lists)
int zjni_last_decode_lists2(unsigned* out5) {
    DevState* d = cur_state();
    if (!d || !out5) return -(int)ZJNI_ERROR_no_device;
    int const r = zjni_last_decode_lists(out5);
    if (r) return r;
    u32 s = 0;
    if (hipMemcpy(&s, d->counters + 32 + 11, sizeof s, hipMemcpyDeviceToHost) != hipSuccess) return -(int)ZJNI_ERROR_no_device;
    out5[4] = s;
    return 0;
}
const char* zjni_route_kernel(int route) {
    switch (route) {
    case ZJNI_ROUTE_WIDE: return "zj_enc_match_wide_kernel";
    case ZJNI_ROUTE_PIPE: return "zj_encode_pipe_kernel";
    case ZJNI_ROUTE_FUSED: return "zj_encode_kernel";
    case ZJNI_ROUTE_WAVE: return "zj_enc_match_wave_kernel";
    case ZJNI_ROUTE_LANE: case ZJNI_ROUTE_HYBRID: return "zj_enc_match_kernel";
    case ZJNI_ROUTE_LANE_GATED: return "zj_enc_match_gated_kernel";
    case ZJNI_ROUTE_RUN: case ZJNI_ROUTE_RUN_FLAGS: return "zj_enc_match_run_kernel";
    case ZJNI_ROUTE_WAVE_HBM: return "zj_encode_multi_kernel";
    default: return "";
    }
}
#ifndef ZJNI_BUILD_STAMP
#define ZJNI_BUILD_STAMP "unknown"
#endif
#ifdef ZJ_TUNING_KERNELS
const char* zjni_build_stamp(void) { return ZJNI_BUILD_STAMP "+tuning"; }
#else
const char* zjni_build_stamp(void) { return ZJNI_BUILD_STAMP; }
#endif

/* ---- resource policy ---- */
size_t zjni_set_scratch_limit(size_t bytes) {
    std::lock_guard<std::mutex> lk(g_mu);
    g_scratch_limit = bytes == 0 ? 0 : (bytes < ZJ_SCRATCH_LIMIT_MIN ? ZJ_SCRATCH_LIMIT_MIN : bytes);
    return g_scratch_limit;
}
size_t zjni_scratch_bytes(void) {
    DevState* d = cur_state();
    if (!d) return 0;
    std::lock_guard<std::mutex> lk(*d->enqueueMu);
    return scratch_total(d);
}
size_t zjni_release_scratch(void) {
    DevState* d = cur_state();
    if (!d) return ZJNI_ERR(ZJNI_ERROR_no_device);
    std::lock_guard<std::mutex> lk(*d->enqueueMu);              // no batch call is being enqueued ...
    if (hipDeviceSynchronize() != hipSuccess) return ZJNI_ERR(ZJNI_ERROR_no_device);   // ... and none is still running
    scratch_free_all(d);
    if (d->framesBuf) (void)hipFree(d->framesBuf); d->framesBuf = nullptr; d->framesBufCap = 0;
    d->lastValid = false;
    return 0;
}

int zjni_kernel_info(int* decodeGrid, int* decodeLds, int* encodeGrid, int* encodeLds) {
    DevState* d = cur_state();
    if (decodeLds) *decodeLds = (int)sizeof(ZDecShared);
    if (encodeLds) *encodeLds = (int)(enc_lds_pass0(3) + sizeof(ZEncShared));
    if (!d) return -(int)ZJNI_ERROR_no_device;
    if (decodeGrid) *decodeGrid = d->decGrid;
    if (encodeGrid) *encodeGrid = d->encGrid;
    return 0;
}

struct zjni_cdict { int ordinal; u8* buf; unsigned dictID; int level; u32 strategy; };   // buf = [ZECDictDev][tagged tables][raw dictionary bytes]; level: the level word (1..3, or ZE_LW_NEG | N)
struct zjni_ddict { int ordinal; u8* buf; size_t rawSize; unsigned dictID; };   // buf = [ZDDictDev][raw dictionary bytes]

// Scratch of the multi-block stages (zj_decode_split.h): tables and records per BLOCK, claimed on the device — ZD_MB_BLOCKS blocks (4 GiB of input at 128 KiB a block)
// and a pool of ZD_MB_SEQS records (a frame whose blocks or sequences find no room goes to the fused kernel).  ZJNI_DEC_MB=0 switches the stages off (A/B runs);
// none under a scratch limit, none with a dictionary.
#define ZD_MB_BLOCKS 65536u
#define ZD_MB_SEQS ((size_t)192 << 20)
#define ZD_MB_LIT_BYTES ((size_t)2 << 30)
struct ZDMbHost { ZDMbArgs a; u64* pool; u8* litPool; u32* procFlag; bool on; };
static ZDMbHost decode_mb_scratch(DevState* d, size_t n, hipStream_t st, bool haveDict) {
    ZDMbHost h; memset(&h, 0, sizeof h);
    int const mbEnv = (zj_env("ZJNI_DEC_MB") && atoi(zj_env("ZJNI_DEC_MB")) == 0) ? 0 : 1;
    if (hipMemsetAsync(d->counters + 232, 0, 64, st) != hipSuccess) return h;      // (also when the stages stay off: zjni_last_decode_lists reads them)
    if (!mbEnv || haveDict || g_scratch_limit) return h;
    size_t const tabB = (size_t)ZD_MB_BLOCKS * ZD_SPLIT_TAB_BYTES, blkB = (size_t)ZD_MB_BLOCKS * sizeof(ZDBlk), frB = n * sizeof(ZDFrameMB), listB2 = (size_t)ZD_MB_BLOCKS * 4, lmB = n * 4;
    size_t const poolOff = (tabB + blkB + frB + 2 * listB2 + 2 * lmB + 255) & ~(size_t)255;          // (lmB x 2: list M, stage 3's "done beside stage 2" flags)
    size_t const litOff = poolOff + ZD_MB_SEQS * 8;
    size_t const need = litOff + ZD_MB_LIT_BYTES + 256;
    if (d->dmbBufCap < need) {
        if (!scratch_make_room(d, d->dmbBufCap, need)) return h;
        if (d->dmbBuf) { if (hipStreamSynchronize(st) != hipSuccess) return h; (void)hipFree(d->dmbBuf); d->dmbBuf = nullptr; d->dmbBufCap = 0; }
        if (hipMalloc(&d->dmbBuf, need) != hipSuccess) { (void)hipGetLastError(); return h; }        // no room: the fused kernel serves these frames as before
        d->dmbBufCap = need;
    }
    u32* const ctr = d->counters + 232;               // [0] blocks, [1] seq list, [2] |M|, [3] work seq, [4..5] records, [6] work exec, [8] lit list, [10..11] literal bytes, [12] work lit
    if (hipMemsetAsync(ctr, 0, 64, st) != hipSuccess) return h;
    h.a.tabs = (u16*)d->dmbBuf; h.a.blks = (ZDBlk*)(d->dmbBuf + tabB); h.a.frames = (ZDFrameMB*)(d->dmbBuf + tabB + blkB);
    h.a.seqList = (u32*)(d->dmbBuf + tabB + blkB + frB); h.a.litList = h.a.seqList + ZD_MB_BLOCKS; h.a.listM = h.a.litList + ZD_MB_BLOCKS;
    h.a.ctr = ctr; h.a.blkCap = ZD_MB_BLOCKS; h.a.seqCap = ZD_MB_SEQS; h.a.minBlocks = 1;
    // stage 3 beside stage 2 (ZJNI_DEC_MB_OVERLAP=0: behind it, as before): a flag per frame says which ones it finished there
    h.procFlag = nullptr;
    if (!(zj_tune("ZJNI_DEC_MB_OVERLAP") && atoi(zj_tune("ZJNI_DEC_MB_OVERLAP")) == 0)) {
        u32* const q = h.a.listM + n;
        if (hipMemsetAsync(q, 0, lmB, st) == hipSuccess) h.procFlag = q;
    }
    h.pool = (u64*)(d->dmbBuf + poolOff);
    int const litEnv = (zj_tune("ZJNI_DEC_MB_LIT") && atoi(zj_tune("ZJNI_DEC_MB_LIT")) == 0) ? 0 : 1;       // stage 2b of these frames off (A/B runs)
    h.a.litCap = litEnv ? ZD_MB_LIT_BYTES : 0; if (!litEnv) h.a.litList = nullptr;
    h.litPool = d->dmbBuf + litOff;
    h.on = true;
    return h;
}
// stages 2 and 3 of the multi-block frames stage 1 put on list M; frames stage 3 hands over are appended to list B (count at listBCount) for the fused kernel behind
static void decode_mb_launch(DevState* d, const ZDMbHost& h, hipStream_t st, const void* d_src, const uint64_t* d_src_off, void* d_dst, const uint64_t* d_dst_off, uint64_t* d_result,
                             u32* listB, u32* listBCount) {
    if (!h.on) return;
    // Stage 2b (literals) and — round 4 — stage 3 on the side stream BESIDE stage 2: the lane-per-block decode leaves most of every SIMD idle, and a frame's blocks
    // finish at different times (they differ 8 x in their number of sequences).  Stage 3 walks a frame's blocks in order as before, but starts each as soon as stage 2
    // has set its seqReady — a 1 MiB frame is then done about one block's execution behind its slowest block instead of eight behind the whole stage; a sweep pass
    // behind both takes the frames it gave up on (bounded waits).
    bool const lit = h.a.litList != nullptr, beside = h.procFlag != nullptr;
    bool const forked = (lit || beside) && hipEventRecord(d->evFork, st) == hipSuccess && hipStreamWaitEvent(d->sideStream, d->evFork, 0) == hipSuccess;
    hipLaunchKernelGGL(zj_dec_seq_mb_kernel, dim3((u32)d->dseqGrid), dim3(64), 0, st, (const u8*)d_src, (const u64*)d_src_off, (const u32*)h.a.seqList, (const u32*)(h.a.ctr + 1), h.a.ctr + 3,
                       (const u16*)h.a.tabs, h.pool, h.a.blks, (forked && beside) ? 1u : 0u);
    if (forked) {
        if (lit) hipLaunchKernelGGL(zj_dec_lit_mb_kernel, dim3((u32)d->dlitGrid), dim3(64), ZD_EXEC_LDS, d->sideStream, (const u8*)d_src, (const u64*)d_src_off, (const u32*)h.a.litList, (const u32*)(h.a.ctr + 8), h.a.ctr + 12,
                                    h.a.blks, h.litPool);
        if (beside)
            hipLaunchKernelGGL(zj_dec_exec_mb_kernel, dim3((u32)d->decGrid), dim3(64), 0, d->sideStream, (const u8*)d_src, (const u64*)d_src_off, (u8*)d_dst, (const u64*)d_dst_off, (u64*)d_result,
                               (const u32*)h.a.listM, (const u32*)(h.a.ctr + 2), h.a.ctr + 6, (const ZDFrameMB*)h.a.frames, (const ZDBlk*)h.a.blks, (const u64*)h.pool, d->decScratch, listB, listBCount,
                               (const u8*)(lit ? h.litPool : nullptr), 1u, h.procFlag);
        if (hipEventRecord(d->evJoin, d->sideStream) != hipSuccess || hipStreamWaitEvent(st, d->evJoin, 0) != hipSuccess) { (void)hipStreamSynchronize(d->sideStream); }
    } else if (lit) {                                   // no fork: stage 2b on the main stream
        hipLaunchKernelGGL(zj_dec_lit_mb_kernel, dim3((u32)d->dlitGrid), dim3(64), ZD_EXEC_LDS, st, (const u8*)d_src, (const u64*)d_src_off, (const u32*)h.a.litList, (const u32*)(h.a.ctr + 8), h.a.ctr + 12,
                           h.a.blks, h.litPool);
    }
    bool const swept = forked && beside;
    hipLaunchKernelGGL(zj_dec_exec_mb_kernel, dim3((u32)d->decGrid), dim3(64), 0, st, (const u8*)d_src, (const u64*)d_src_off, (u8*)d_dst, (const u64*)d_dst_off, (u64*)d_result,
                       (const u32*)h.a.listM, (const u32*)(h.a.ctr + 2), swept ? h.a.ctr + 14 : h.a.ctr + 6, (const ZDFrameMB*)h.a.frames, (const ZDBlk*)h.a.blks, (const u64*)h.pool, d->decScratch, listB, listBCount,
                       (const u8*)(lit ? h.litPool : nullptr), swept ? 2u : 0u, swept ? h.procFlag : (u32*)nullptr);
}
static size_t decompress_batch_device_impl(const void* d_src, const uint64_t* d_src_off, void* d_dst, const uint64_t* d_dst_off,
                                           uint64_t* d_result, size_t n, const zjni_ddict* ddict, void* stream) {
    DevState* d = cur_state();
    const ZDDictDev* const ddDev = ddict ? (const ZDDictDev*)ddict->buf : nullptr;
    const u8* const ddRaw = ddict ? ddict->buf + sizeof(ZDDictDev) : nullptr;
    if (!d) return ZJNI_ERR(ZJNI_ERROR_no_device);
    if (n == 0) return 0;
    if (n > 0xFFFFFFFFull) return ZJNI_ERR(72);
    hipStream_t st = (hipStream_t)stream;
    u32 const grid = (u32)(n < (size_t)d->decGrid ? n : (size_t)d->decGrid);
    // Large batches: the three-stage pipeline (tANS decode lane-per-frame); whatever is not a simple frame, and
    // anything that fails on the way, ends on list B and goes through the fused kernel.  Small batches: fused only.
    size_t splitMin = 4096;
    if (const char* ov = zj_env("ZJNI_DSPLIT_MIN")) splitMin = (size_t)atoll(ov);
    if (n >= splitMin) {
        size_t const tabBytes = n * (size_t)ZD_SPLIT_TAB_BYTES, seqBytes = n * (size_t)ZD_SPLIT_SEQ_BYTES, metaBytes = n * sizeof(ZDMeta), listBytes = n * 4;
        size_t const need = tabBytes + seqBytes + metaBytes + 4 * listBytes + 256;
        if (d->dsplitBufCap < need) {
            if (!scratch_make_room(d, d->dsplitBufCap, need)) return ZJNI_ERR(64);
            if (d->dsplitBuf) { if (hipStreamSynchronize(st) != hipSuccess) return ZJNI_ERR(ZJNI_ERROR_no_device); (void)hipFree(d->dsplitBuf); d->dsplitBuf = nullptr; d->dsplitBufCap = 0; }
            if (hipMalloc(&d->dsplitBuf, need) != hipSuccess) return ZJNI_ERR(64);
            d->dsplitBufCap = need;
        }
        u16* const tabs = (u16*)d->dsplitBuf; u64* const seqs = (u64*)(d->dsplitBuf + tabBytes);
        ZDMeta* const metas = (ZDMeta*)(d->dsplitBuf + tabBytes + seqBytes);
        u32* const listA = (u32*)(d->dsplitBuf + tabBytes + seqBytes + metaBytes); u32* const listB = listA + n;
        u32* const doneList = listB + n; u32* const procFlag = doneList + n;       // completion queue of the sequence decode, frames the side pass executed
        u32* const c = d->counters + 32;          // [0] frames the pass beside the sequence decode executed, [1] |B|, [2] work prep, [3] work seq, [4] work exec, [5] work fused, [6] queue length, [7] work of the sweep pass, [8] |A|, [9] sequences in A, [10] work of the literal pass, [11] frames of one stored block copied by stage 1
        // Stage 2b (zd_lit_frame): one literal slot per frame, as large as the budget allows (at most a block); frames whose literals do
        // not fit a slot stay with the execution kernel.  Without a dictionary only (treeless literals need the dictionary's table).
        // ZJNI_DEC_LIT=0 switches the pass off (A/B runs); ZJNI_DEC_LIT_BYTES sets the budget (default 4 GiB, nothing under a scratch limit).
        u8* litSlots = nullptr; u32 litSlot = 0;
        {   int const litEnv = (zj_env("ZJNI_DEC_LIT") && atoi(zj_env("ZJNI_DEC_LIT")) == 0) ? 0 : 1;
            if (litEnv && !ddict && !g_scratch_limit) {
                size_t budget = (size_t)4 << 30; if (const char* ov = zj_tune("ZJNI_DEC_LIT_BYTES")) { long long const v = atoll(ov); budget = v <= 0 ? 0 : ((unsigned long long)v > ((unsigned long long)64 << 30) ? (size_t)64 << 30 : (size_t)v); }
                size_t slot = budget / n; if (slot > ZD_BLOCK_MAX) slot = ZD_BLOCK_MAX; slot &= ~(size_t)4095;
                if (slot >= 16384) {
                    size_t const needL = n * slot + 64;
                    if (d->dlitBufCap < needL) {
                        if (d->dlitBuf) { if (hipStreamSynchronize(st) != hipSuccess) return ZJNI_ERR(ZJNI_ERROR_no_device); (void)hipFree(d->dlitBuf); d->dlitBuf = nullptr; d->dlitBufCap = 0; }
                        if (hipMalloc(&d->dlitBuf, needL) == hipSuccess) d->dlitBufCap = needL; else { d->dlitBuf = nullptr; (void)hipGetLastError(); }
                    }
                    if (d->dlitBuf) { litSlots = d->dlitBuf; litSlot = (u32)slot; }
                }
            }
        }
        static int const overlapEnv = zj_tune("ZJNI_DEC_NO_OVERLAP") ? 0 : 1;
        // Running the execution kernel beside the sequence decode costs two cross-stream dependencies and an extra launch per slice
        // (~0.3 ms) — worth it only for frames with many sequences (zj_dec_heavy, decided on the device).  The host skips the set-up
        // when the last slice it has statistics for was light: the statistics arrive asynchronously and are never waited for, so a
        // change of workload is followed one call late, which costs time, never correctness.
        u32 const statA = d->decStat ? d->decStat[0] : 0u, statS = d->decStat ? d->decStat[1] : 0u;
        int const overlap = overlapEnv && !(statA > 0u && statS < 512u * statA);
        if (hipMemsetAsync(c, 0, 48, st) != hipSuccess) return ZJNI_ERR(ZJNI_ERROR_no_device);
        (void)hipEventRecord(d->tev[2], st);
        ZDMbHost const mb = decode_mb_scratch(d, n, st, ddict != nullptr);       // frames that are not simple: multi-block, no content size (the stream classes')
        if (ddict) hipLaunchKernelGGL(zj_dec_prep_kernel_t<true>, dim3(grid), dim3(64), 0, st, (const u8*)d_src, (const u64*)d_src_off, (const u64*)d_dst_off,
                                      (u32)n, c + 2, tabs, metas, listA, listB, c, ddDev, overlap ? doneList : (u32*)nullptr, procFlag, mb.a, 0u, (u8*)d_dst, (u64*)d_result);
        else hipLaunchKernelGGL(zj_dec_prep_kernel, dim3(grid), dim3(64), 0, st, (const u8*)d_src, (const u64*)d_src_off, (const u64*)d_dst_off,
                                (u32)n, c + 2, tabs, metas, listA, listB, c, ddDev, overlap ? doneList : (u32*)nullptr, procFlag, mb.a, 0u, (u8*)d_dst, (u64*)d_result);
        (void)hipEventRecord(d->tev[3], st);
        u32 const waves = (u32)((n + 63) / 64);
        u32 gridX = (u32)(n < (size_t)d->dexecGrid ? n : (size_t)d->dexecGrid);
        if (const char* ov = zj_tune("ZJNI_DEXEC_PER_CU")) { int const v = atoi(ov); if (v >= 1 && (u32)(v * d->numCU) < gridX) gridX = (u32)(v * d->numCU); }      // (tuning builds: fewer execution / literal workgroups beside the sequence decode)
        // The execution kernel (literals + LZ77 copy, wave per frame) runs on a side stream BESIDE the sequence decode and takes
        // frames in the order they finish there: the lane-per-frame decode is a dependent chain per frame (one wave per SIMD, mostly
        // waiting), so the two share the CUs instead of following each other.  A sweep pass afterwards takes what the side kernel
        // did not get to (its waits are bounded): completion never depends on the two kernels being co-scheduled.
        bool const fork = overlap || litSlots;
        if (fork && (hipEventRecord(d->evFork, st) != hipSuccess || hipStreamWaitEvent(d->sideStream, d->evFork, 0) != hipSuccess)) return ZJNI_ERR(ZJNI_ERROR_no_device);
        if (litSlots) {                                 // beside the sequence decode, ahead of the mode-1 execution pass on the same side stream
            u32 gridL = (u32)(n < (size_t)d->dlitGrid ? n : (size_t)d->dlitGrid);
            if (const char* ov = zj_tune("ZJNI_DLIT_PER_CU")) { int const v = atoi(ov); if (v >= 1 && (u32)(v * d->numCU) < gridL) gridL = (u32)(v * d->numCU); }
            hipLaunchKernelGGL(zj_dec_lit_kernel, dim3(gridL), dim3(64), ZD_EXEC_LDS, d->sideStream, (const u8*)d_src, (const u64*)d_src_off, (const u32*)listA,
                               (const u32*)(c + 8), c + 10, metas, litSlots, litSlot, d->prof);
        }
        hipLaunchKernelGGL(zj_dec_seq_kernel, dim3(waves < (u32)d->dseqGrid ? waves : (u32)d->dseqGrid), dim3(64), 0, st, (const u8*)d_src,
                           (const u64*)d_src_off, (const u32*)listA, (const u32*)(c + 8), c + 3, (const u16*)tabs, seqs, metas, ddDev,
                           overlap ? doneList : (u32*)nullptr, c + 6, (u32)d->dseqHeavy);
        (void)hipEventRecord(d->tev[4], st);
        if (litSlots && !overlap && (hipEventRecord(d->evJoin, d->sideStream) != hipSuccess || hipStreamWaitEvent(st, d->evJoin, 0) != hipSuccess)) {
            (void)hipStreamSynchronize(d->sideStream); (void)hipStreamSynchronize(st);          // the side kernel must not outlive this call's claim on the scratch
            return ZJNI_ERR(ZJNI_ERROR_no_device);
        }
        for (int pass = overlap ? 1 : 0; pass <= (overlap ? 2 : 0); pass++) {
            hipStream_t const es = pass == 1 ? d->sideStream : st;
            u32* const work = pass == 2 ? c + 7 : c + 4;
            if (ddict) hipLaunchKernelGGL(zj_dec_exec_kernel_t<true>, dim3(gridX), dim3(64), ZD_SHARED_NO_FSE, es,
                               (const u8*)d_src, (const u64*)d_src_off, (u8*)d_dst, (const u64*)d_dst_off, (u64*)d_result, (const u32*)listA,
                               (const u32*)(c + 8), work, metas, (const u64*)seqs, d->decScratch, listB, c + 1, d->prof, ddDev, ddRaw, (u32)pass, (const u32*)doneList, procFlag, litSlots, litSlot, c);
            else hipLaunchKernelGGL(zj_dec_exec_kernel, dim3(gridX), dim3(64), ZD_SHARED_NO_FSE, es,
                               (const u8*)d_src, (const u64*)d_src_off, (u8*)d_dst, (const u64*)d_dst_off, (u64*)d_result, (const u32*)listA,
                               (const u32*)(c + 8), work, metas, (const u64*)seqs, d->decScratch, listB, c + 1, d->prof, ddDev, ddRaw, (u32)pass, (const u32*)doneList, procFlag, litSlots, litSlot, c);
            if (pass == 1 && (hipEventRecord(d->evJoin, d->sideStream) != hipSuccess || hipStreamWaitEvent(st, d->evJoin, 0) != hipSuccess)) {
                (void)hipStreamSynchronize(d->sideStream); (void)hipStreamSynchronize(st);          // the side kernel must not outlive this call's claim on the scratch
                return ZJNI_ERR(ZJNI_ERROR_no_device);
            }
        }
        if (d->decStat) (void)hipMemcpyAsync((void*)d->decStat, c + 8, 8, hipMemcpyDeviceToHost, st);
        decode_mb_launch(d, mb, st, d_src, d_src_off, d_dst, d_dst_off, d_result, listB, c + 1);
        (void)hipEventRecord(d->tev[5], st);
        if (ddict) hipLaunchKernelGGL(zj_decode_dict_kernel, dim3(grid < (u32)d->decDictGrid ? grid : (u32)d->decDictGrid), dim3(64), 0, st, (const u8*)d_src, (const u64*)d_src_off, (u8*)d_dst,
                           (const u64*)d_dst_off, (u64*)d_result, (u32)n, c + 5, d->decScratch, d->prof, (const u32*)listB, (const u32*)(c + 1), ddDev, ddRaw);
        else hipLaunchKernelGGL(zj_decode_kernel, dim3(grid), dim3(64), 0, st, (const u8*)d_src, (const u64*)d_src_off, (u8*)d_dst,
                           (const u64*)d_dst_off, (u64*)d_result, (u32)n, c + 5, d->decScratch, d->prof, (const u32*)listB, (const u32*)(c + 1), ddDev, ddRaw);
        (void)hipEventRecord(d->tev[6], st); d->tevDecompress = true;
        return hipGetLastError() == hipSuccess ? 0 : ZJNI_ERR(ZJNI_ERROR_no_device);
    }
    if (hipMemsetAsync(d->counters, 0, 4, st) != hipSuccess) return ZJNI_ERR(ZJNI_ERROR_no_device);
    // Small batches: frames of two blocks and more take the block stages (stage 1 in its multi-block-only mode; a frame is a chain of ~40 000 dependent steps per MiB on
    // the fused kernel, its blocks decode side by side here); everything else, and whatever the stages hand over, is the fused kernel's as before.
    if (!ddict) {
        ZDMbHost mb = decode_mb_scratch(d, n, st, false);
        size_t const lbBytes = n * 4;
        if (mb.on && d->dsplitBufCap < lbBytes + 256) {                                   // list B of this path lives at the start of the split pipeline's buffer
            if (d->dsplitBuf) { if (hipStreamSynchronize(st) != hipSuccess) return ZJNI_ERR(ZJNI_ERROR_no_device); (void)hipFree(d->dsplitBuf); d->dsplitBuf = nullptr; d->dsplitBufCap = 0; }
            if (hipMalloc(&d->dsplitBuf, lbBytes + 256) != hipSuccess) { (void)hipGetLastError(); mb.on = false; } else d->dsplitBufCap = lbBytes + 256;
        }
        if (mb.on) {
            u32* const c = d->counters + 32; u32* const listB = (u32*)d->dsplitBuf;
            if (hipMemsetAsync(c, 0, 48, st) != hipSuccess) return ZJNI_ERR(ZJNI_ERROR_no_device);
            mb.a.minBlocks = 2;
            (void)hipEventRecord(d->tev[2], st);
            hipLaunchKernelGGL(zj_dec_prep_kernel, dim3(grid), dim3(64), 0, st, (const u8*)d_src, (const u64*)d_src_off, (const u64*)d_dst_off,
                               (u32)n, c + 2, (u16*)nullptr, (ZDMeta*)nullptr, (u32*)nullptr, listB, c, (const ZDDictDev*)nullptr, (u32*)nullptr, (u32*)nullptr, mb.a, 1u, (u8*)d_dst, (u64*)d_result);
            (void)hipEventRecord(d->tev[3], st); (void)hipEventRecord(d->tev[4], st);
            decode_mb_launch(d, mb, st, d_src, d_src_off, d_dst, d_dst_off, d_result, listB, c + 1);
            (void)hipEventRecord(d->tev[5], st);
            hipLaunchKernelGGL(zj_decode_kernel, dim3(grid), dim3(64), 0, st, (const u8*)d_src, (const u64*)d_src_off, (u8*)d_dst,
                               (const u64*)d_dst_off, (u64*)d_result, (u32)n, c + 5, d->decScratch, d->prof, (const u32*)listB, (const u32*)(c + 1), (const ZDDictDev*)nullptr, (const u8*)nullptr);
            (void)hipEventRecord(d->tev[6], st); d->tevDecompress = true;
            return hipGetLastError() == hipSuccess ? 0 : ZJNI_ERR(ZJNI_ERROR_no_device);
        }
    }
    if (ddict) {
        u32 const gridD = (u32)(n < (size_t)d->decDictGrid ? n : (size_t)d->decDictGrid);
        hipLaunchKernelGGL(zj_decode_dict_kernel, dim3(gridD), dim3(64), 0, st, (const u8*)d_src, (const u64*)d_src_off, (u8*)d_dst,
                           (const u64*)d_dst_off, (u64*)d_result, (u32)n, d->counters, d->decScratch, d->prof, (const u32*)nullptr, (const u32*)nullptr, ddDev, ddRaw);
    } else
    hipLaunchKernelGGL(zj_decode_kernel, dim3(grid), dim3(64), 0, st, (const u8*)d_src, (const u64*)d_src_off, (u8*)d_dst,
                       (const u64*)d_dst_off, (u64*)d_result, (u32)n, d->counters, d->decScratch, d->prof, (const u32*)nullptr, (const u32*)nullptr, ddDev, ddRaw);
    return hipGetLastError() == hipSuccess ? 0 : ZJNI_ERR(ZJNI_ERROR_no_device);
}
// The per-frame scratch of the pipelines (176 KiB decode, 416 KiB compress) is sized per call; very large batches go
// through it in slices of ZJ_CHUNK_FRAMES on the same stream (stream order makes the reuse safe), so a batch of a
// million buffers needs no more scratch than one of 65 536.
#define ZJ_CHUNK_FRAMES 65536u
// one batch call at a time per device on the host side, and in order on the GPU side
struct BatchOrder {
    DevState* d; hipStream_t st;
    BatchOrder(DevState* dev, void* stream) : d(dev), st((hipStream_t)stream) {
        if (!d) return;
        d->enqueueMu->lock();
        if (d->lastValid) (void)hipStreamWaitEvent(st, d->lastDone, 0);
    }
    ~BatchOrder() { if (!d) return; d->lastValid = (hipEventRecord(d->lastDone, st) == hipSuccess); d->enqueueMu->unlock(); }
};
static size_t decompress_chunked_ordered(const void* d_src, const uint64_t* d_src_off, void* d_dst, const uint64_t* d_dst_off,
                                         uint64_t* d_result, size_t n, const zjni_ddict* ddict, void* stream);
static size_t decompress_chunked(const void* d_src, const uint64_t* d_src_off, void* d_dst, const uint64_t* d_dst_off,
                                 uint64_t* d_result, size_t n, const zjni_ddict* ddict, void* stream) {
    BatchOrder order(cur_state(), stream);
    return decompress_chunked_ordered(d_src, d_src_off, d_dst, d_dst_off, d_result, n, ddict, stream);
}
// (the caller holds the device's BatchOrder)
static size_t decompress_chunked_ordered(const void* d_src, const uint64_t* d_src_off, void* d_dst, const uint64_t* d_dst_off,
                                         uint64_t* d_result, size_t n, const zjni_ddict* ddict, void* stream) {
    size_t const chunk = scratch_slice((size_t)ZD_SPLIT_TAB_BYTES + ZD_SPLIT_SEQ_BYTES + sizeof(ZDMeta) + 8, ZJ_CHUNK_FRAMES, 1);
    for (size_t at = 0; at < n || at == 0; at += chunk) {
        size_t const m = n - at < chunk ? n - at : chunk;
        size_t const r = decompress_batch_device_impl(d_src, d_src_off + at, d_dst, d_dst_off + at, d_result + at, m, ddict, stream);
        if (r != 0 || n == 0) return r;
    }
    return 0;
}
size_t zjni_decompress_batch_device(const void* d_src, const uint64_t* d_src_off, void* d_dst, const uint64_t* d_dst_off,
                                    uint64_t* d_result, size_t n, void* stream) {
    return decompress_chunked(d_src, d_src_off, d_dst, d_dst_off, d_result, n, nullptr, stream);
}
size_t zjni_decompress_batch_device_usingDDict(const void* d_src, const uint64_t* d_src_off, void* d_dst, const uint64_t* d_dst_off,
                                               uint64_t* d_result, size_t n, const zjni_ddict* ddict, void* stream) {
    if (ddict && ddict->ordinal != t_dev && t_dev >= 0) return ZJNI_ERR(32);      // digested on another device
    return decompress_chunked(d_src, d_src_off, d_dst, d_dst_off, d_result, n, ddict, stream);
}

// ---- sizing a decompress batch from its frames alone (zj_frameinfo.h) ----
size_t zjni_inspect(const void* src, size_t srcSize, zjni_frame_info* out) {
    zj_frame_walk((const u8*)src, src ? (u64)srcSize : 0, out);
    return 0;
}
// One lane per buffer: the walk is a chain of dependent block-header reads, nothing for a wave to share.  Workgroups of one wave and no barrier, so a frame
// of many blocks keeps back the 63 buffers of its own wave and nobody else's.
__global__ __launch_bounds__(64) void zj_inspect_kernel(const u8* __restrict__ src, const u64* __restrict__ off, zjni_frame_info* __restrict__ info, u32 n) {
    u64 const i = (u64)blockIdx.x * 64u + threadIdx.x;
    if (i >= n) return;
    u64 const lo = off[i], hi = off[i + 1];
    zjni_frame_info fi;
    zj_frame_walk(src + lo, hi > lo ? hi - lo : 0, &fi);
    info[i] = fi;
}
// The offsets are a scan over n slots in three launches: every workgroup of 256 lanes takes 1 024 buffers (4 neighbours per lane), writes their slots to
// off[1 + i] and their sum to part[workgroup]; one workgroup scans the partial sums (n / 1 024 of them); the first kernel's grid again turns the slots into
// clamped prefix sums in place.  Additions saturate (zj_sat_add: associative, so the order of the tree does not show).
#define ZJ_SLOT_WG 256u
#define ZJ_SLOT_PER_WG 1024u
// exclusive prefix of v over the workgroup's 256 lanes, *total = their sum (Hillis-Steele in LDS)
__device__ __forceinline__ u64 zj_slot_scan256(u64 v, u64* sh, u64* total) {
    u32 const t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (u32 d = 1; d < ZJ_SLOT_WG; d <<= 1) {
        u64 const w = t >= d ? sh[t - d] : 0;
        __syncthreads();
        sh[t] = zj_sat_add(sh[t], w);
        __syncthreads();
    }
    u64 const excl = t ? sh[t - 1] : 0;
    *total = sh[ZJ_SLOT_WG - 1];
    __syncthreads();
    return excl;
}
__global__ __launch_bounds__(ZJ_SLOT_WG) void zj_slot_sizes_kernel(const zjni_frame_info* __restrict__ info, u64 n, u64 alignMask, u64 slotMax,
                                                                   u64* __restrict__ off, u64* __restrict__ part) {
    __shared__ u64 sh[ZJ_SLOT_WG];
    u64 const base = (u64)blockIdx.x * ZJ_SLOT_PER_WG + (u64)threadIdx.x * 4u;
    u64 sum = 0;
    for (u32 k = 0; k < 4; k++) {
        u64 const i = base + k;
        if (i >= n) break;
        u64 const slot = zj_info_slot(info[i].content, info[i].bound, alignMask, slotMax);
        off[i + 1] = slot;
        sum = zj_sat_add(sum, slot);
    }
    u64 total;
    (void)zj_slot_scan256(sum, sh, &total);
    if (threadIdx.x == 0) part[blockIdx.x] = total;
}
// part[0 .. m) -> its exclusive prefix sums in place, needed[0] = the total, off[0] = 0: one workgroup, a contiguous run per lane (zj_pack_offsets_kernel's shape)
__global__ __launch_bounds__(1024) void zj_slot_parts_kernel(u64* __restrict__ part, u64 m, u64* __restrict__ needed, u64* __restrict__ off) {
    __shared__ u64 sh[1024];
    u32 const t = threadIdx.x;
    u64 const per = (m + 1023u) / 1024u, lo0 = (u64)t * per, lo = lo0 < m ? lo0 : m, hi = lo + per < m ? lo + per : m;
    u64 sum = 0;
    for (u64 i = lo; i < hi; i++) sum = zj_sat_add(sum, part[i]);
    sh[t] = sum;
    __syncthreads();
    for (u32 d = 1; d < 1024u; d <<= 1) {
        u64 const v = t >= d ? sh[t - d] : 0;
        __syncthreads();
        sh[t] = zj_sat_add(sh[t], v);
        __syncthreads();
    }
    u64 run = t ? sh[t - 1] : 0;
    for (u64 i = lo; i < hi; i++) { u64 const z = part[i]; part[i] = run; run = zj_sat_add(run, z); }
    if (t == 1023u) { needed[0] = sh[1023]; off[0] = 0; }
}
__global__ __launch_bounds__(ZJ_SLOT_WG) void zj_slot_offsets_kernel(u64* __restrict__ off, u64 n, u64 cap, const u64* __restrict__ part) {
    __shared__ u64 sh[ZJ_SLOT_WG];
    u64 const base = (u64)blockIdx.x * ZJ_SLOT_PER_WG + (u64)threadIdx.x * 4u;
    u64 slot[4], sum = 0;
    for (u32 k = 0; k < 4; k++) { slot[k] = base + k < n ? off[base + k + 1] : 0; sum = zj_sat_add(sum, slot[k]); }
    u64 total;
    u64 run = zj_sat_add(part[blockIdx.x], zj_slot_scan256(sum, sh, &total));
    for (u32 k = 0; k < 4; k++) {
        if (base + k >= n) break;
        run = zj_sat_add(run, slot[k]);
        off[base + k + 1] = run < cap ? run : cap;
    }
}
static bool slot_align_ok(u64 align) { return align >= 1 && align <= 65536 && (align & (align - 1)) == 0; }
// (the caller holds the device's BatchOrder: `slotPart` is shared by the device's calls)
static size_t inspect_enqueue(DevState* d, const void* d_src, const uint64_t* d_src_off, zjni_frame_info* d_info, size_t n, hipStream_t st) {
    if (n == 0) return 0;
    if (n > 0xFFFFFFFFull) return ZJNI_ERR(72);
    hipLaunchKernelGGL(zj_inspect_kernel, dim3((u32)((n + 63) / 64)), dim3(64), 0, st, (const u8*)d_src, (const u64*)d_src_off, d_info, (u32)n);
    return hipGetLastError() == hipSuccess ? 0 : ZJNI_ERR(ZJNI_ERROR_no_device);
}
static size_t offsets_enqueue(DevState* d, const zjni_frame_info* d_info, size_t n, u64 cap, u64 align, u64 slotMax, u64* d_dst_off, u64* d_needed, hipStream_t st) {
    if (n > 0xFFFFFFFFull) return ZJNI_ERR(72);
    if (n == 0) return hipMemsetAsync(d_dst_off, 0, 8, st) == hipSuccess && hipMemsetAsync(d_needed, 0, 8, st) == hipSuccess ? 0 : ZJNI_ERR(ZJNI_ERROR_no_device);
    size_t const groups = (n + ZJ_SLOT_PER_WG - 1) / ZJ_SLOT_PER_WG;
    if (groups > d->slotPartCap) {
        size_t const want = groups < 8192 ? 8192 : groups;
        if (d->slotPart) (void)hipFree(d->slotPart);          // (drains the device: an earlier call may still be reading it)
        d->slotPart = nullptr; d->slotPartCap = 0;
        if (hipMalloc(&d->slotPart, want * 8) != hipSuccess) return ZJNI_ERR(64);
        d->slotPartCap = want;
    }
    hipLaunchKernelGGL(zj_slot_sizes_kernel, dim3((u32)groups), dim3(ZJ_SLOT_WG), 0, st, d_info, (u64)n, align - 1, slotMax, d_dst_off, d->slotPart);
    hipLaunchKernelGGL(zj_slot_parts_kernel, dim3(1), dim3(1024), 0, st, d->slotPart, (u64)groups, d_needed, d_dst_off);
    hipLaunchKernelGGL(zj_slot_offsets_kernel, dim3((u32)groups), dim3(ZJ_SLOT_WG), 0, st, d_dst_off, (u64)n, cap, (const u64*)d->slotPart);
    return hipGetLastError() == hipSuccess ? 0 : ZJNI_ERR(ZJNI_ERROR_no_device);
}
size_t zjni_inspect_batch_device(const void* d_src, const uint64_t* d_src_off, zjni_frame_info* d_info, size_t n, void* stream) {
    DevState* d = cur_state();
    if (!d) return ZJNI_ERR(ZJNI_ERROR_no_device);
    return inspect_enqueue(d, d_src, d_src_off, d_info, n, (hipStream_t)stream);      // no shared scratch: needs no place in the device's order
}
size_t zjni_decompress_offsets_device(const zjni_frame_info* d_info, size_t n, uint64_t dstCapacity, uint64_t align, uint64_t slotMax,
                                      uint64_t* d_dst_off, uint64_t* d_needed, void* stream) {
    if (!slot_align_ok(align)) return ZJNI_ERR(42);
    DevState* d = cur_state();
    if (!d) return ZJNI_ERR(ZJNI_ERROR_no_device);
    BatchOrder order(d, stream);
    return offsets_enqueue(d, d_info, n, dstCapacity, align, slotMax, d_dst_off, d_needed, (hipStream_t)stream);
}
size_t zjni_decompress_batch_device_sized(const void* d_src, const uint64_t* d_src_off, void* d_dst, uint64_t dstCapacity, uint64_t align,
                                          uint64_t slotMax, zjni_frame_info* d_info, uint64_t* d_dst_off, uint64_t* d_needed,
                                          uint64_t* d_result, size_t n, const zjni_ddict* ddict, void* stream) {
    if (!slot_align_ok(align)) return ZJNI_ERR(42);
    if (ddict && ddict->ordinal != t_dev && t_dev >= 0) return ZJNI_ERR(32);      // digested on another device
    DevState* d = cur_state();
    if (!d) return ZJNI_ERR(ZJNI_ERROR_no_device);
    BatchOrder order(d, stream);
    size_t r = inspect_enqueue(d, d_src, d_src_off, d_info, n, (hipStream_t)stream);
    if (r == 0) r = offsets_enqueue(d, d_info, n, dstCapacity, align, slotMax, d_dst_off, d_needed, (hipStream_t)stream);
    if (r != 0) return r;
    return decompress_chunked_ordered(d_src, d_src_off, d_dst, d_dst_off, d_result, n, ddict, stream);
}

// ZSTD_createDDict (N/decompress/zstd_ddict.c:36-130; ZstdDictDecompress.init, N/jni_fast_zstd.c:56-75): the raw
// dictionary goes to HBM once and one workgroup digests it there.  NULL when the device or the dictionary is bad.
zjni_ddict* zjni_createDDict(const void* dict, size_t dictSize) {
    DevState* d = cur_state();
    if (!d || !dict || dictSize == 0 || dictSize > 0x7FFFFFFFull) return nullptr;
    zjni_ddict* dd = new zjni_ddict{t_dev, nullptr, dictSize, 0};
    if (hipMalloc(&dd->buf, sizeof(ZDDictDev) + dictSize + 16) != hipSuccess) { delete dd; return nullptr; }
    ZDDictDev head;
    bool ok = hipMemcpy(dd->buf + sizeof(ZDDictDev), dict, dictSize, hipMemcpyHostToDevice) == hipSuccess;
    if (ok) {
        hipLaunchKernelGGL(zj_ddict_digest_kernel, dim3(1), dim3(64), 0, 0, (const u8*)(dd->buf + sizeof(ZDDictDev)), (u32)dictSize, (ZDDictDev*)dd->buf);
        ok = hipMemcpy(&head, dd->buf, 64, hipMemcpyDeviceToHost) == hipSuccess && head.status == 0;
    }
    if (!ok) { (void)hipFree(dd->buf); delete dd; return nullptr; }
    dd->dictID = head.dictID;
    return dd;
}
size_t zjni_freeDDict(zjni_ddict* dd) {
    if (!dd) return 0;
    (void)hipSetDevice(dd->ordinal);
    (void)hipFree(dd->buf);
    delete dd;
    return 0;
}
unsigned zjni_getDictID_fromDDict(const zjni_ddict* dd) { return dd ? dd->dictID : 0u; }

// The `checksum` argument of the advanced / dictionary entries is a flag word (include/zjni_amd.h ZJNI_FRAME_*): 1 alone is what it
// always meant; the boolean entries (zjni_compress*2) normalise their argument before they get here.
static inline void zj_dbg_sync(const char* what) {        // ZJNI_DEBUG_SYNC=1: drain the device after a launch and say so (finding the kernel that does not return)
    static int const on = zj_env("ZJNI_DEBUG_SYNC") ? 1 : 0;
    if (!on) return;
    fprintf(stderr, "[zjni] waiting for %s ...", what); fflush(stderr);
    hipError_t const e = hipDeviceSynchronize();
    fprintf(stderr, " %s\n", e == hipSuccess ? "done" : hipGetErrorString(e)); fflush(stderr);
}
// Frame-wide match-finder tables of the wave-per-frame kernels (zj_encode_multi_kernel, zj_encode_cdict_copy_kernel): 1 MiB per resident
// workgroup, allocated on first use.  Two workgroups per SIMD (8 per CU): the wave matcher of multi-block frames is a chain of round trips
// and LDS steps per frame, a second wave beside it fills the gaps (2 048 x 1 MiB frames: 656 -> 412 ms); the LDS of the entropy stage
// (18 KiB per workgroup) does not admit a third.  ZJNI_MULTI_PER_CU overrides.
static bool ensure_multi_tables(DevState* d) {
    if (d->multiTables) return true;
    int perCU = 8; if (const char* ov = zj_tune("ZJNI_MULTI_PER_CU")) { int const v = atoi(ov); if (v >= 1 && v <= 16) perCU = v; }
    int fit = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&fit, zj_encode_multi_kernel, 64, sizeof(ZEEntropy)) == hipSuccess && fit >= 1 && fit < perCU) perCU = fit;
    d->multiGrid = d->numCU * perCU; if (d->multiGrid > d->encGrid) d->multiGrid = d->encGrid;     // encScratch has one slot per resident entropy workgroup
    if (hipMalloc(&d->multiTables, (size_t)d->multiGrid * ZE_MULTI_TABLE_BYTES) != hipSuccess) { d->multiTables = nullptr; (void)hipGetLastError(); return false; }
    {   int pfit = 0; size_t const lds = sizeof(ZEEntropy) + ZJ_PIPE_LDS_P;
        d->pipeGrid = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&pfit, zj_encode_pipe_kernel, 128, lds + 16u) == hipSuccess && pfit >= 1) {
            int gp = d->numCU * pfit;
            if (gp > d->multiGrid) gp = d->multiGrid;             // a table set per workgroup
            if (gp > d->encGrid / 2) gp = d->encGrid / 2;         // two scratch slots per workgroup
            d->pipeGrid = gp;
        } else (void)hipGetLastError(); }
    return true;
}
static inline u32 zj_frame_flags(int word) { return (u32)word & ZE_FLAG_MASK; }
static size_t compress_batch_device_impl(const void* d_src, const uint64_t* d_src_off, void* d_dst, const uint64_t* d_dst_off,
                                         uint64_t* d_result, size_t n, int levelWord, u32 flags, void* stream) {
    DevState* d = cur_state();
    if (!d) return ZJNI_ERR(ZJNI_ERROR_no_device);
    int const level = (int)ZE_LW_LEVEL((u32)levelWord);       // kernels take the level word (level | hashLog << 8 | chainLog << 16)
    bool const tuned = ZE_LW_TUNED((u32)levelWord);
    bool const neg = ((u32)levelWord & ZE_LW_NEG) != 0u;      // a negative level: level 1's routes, each on its *_neg kernel (zj_encode_kernel takes both)
    if (level < 1 || level > ZJ_LEVEL_MAX) return ZJNI_ERR(42);
    if (n == 0) return 0;
    if (n > 0xFFFFFFFFull) return ZJNI_ERR(72);
    hipStream_t st = (hipStream_t)stream;
    d->lastRoute = ZJ_ROUTE_OTHER;
    bool wasCleared = d->clearedValid; d->clearedValid = false;      // whatever this call does with the scratch, the promise of the previous one ends here
    if (d->encListCap < n) {                      // grows rarely; the only synchronous step of this entry
        if (d->encList) { if (hipStreamSynchronize(st) != hipSuccess) return ZJNI_ERR(ZJNI_ERROR_no_device); (void)hipFree(d->encList); d->encList = nullptr; d->encListCap = 0; }
        size_t const cap = n + (n >> 2) + 1024;
        if (hipMalloc(&d->encList, 4 * cap * sizeof(u32)) != hipSuccess) return ZJNI_ERR(64);
        d->encListCap = cap;
    }
    u32* const ctr = d->counters + 16;            // [0] |A|, [1] |B|, [2] work A, [3] work B
    u32* const listA = d->encList; u32* const listB = d->encList + d->encListCap; u32* const listS = d->encList + 2 * d->encListCap; u32* const listC = d->encList + 3 * d->encListCap;
    if (hipMemsetAsync(ctr, 0, 32, st) != hipSuccess) return ZJNI_ERR(ZJNI_ERROR_no_device);     // [0] |A|, [1] |B|, [2] work A, [3] work B, [4] |C|, [5] work C
    if (level > 3 && tuned) return ZJNI_ERR(42);
    // Level 3, batches that cannot fill the lane pipeline: a lane of that pipeline takes ~46 000 rounds for a 64 KiB text frame whatever the batch size (a
    // floor of ~96 ms per call), while a wave of the multi-block kernel parses the same frame in ~6 000 windows (zj_match_wavex.h: ~17 ms) —
    // so below ZJNI_L3_WAVE_MAX frames (default 8 192: four rounds of the 2 048 resident waves) every frame goes there, with the level's own tables or the caller's.
    // (ZJNI_SPLIT_MIN — "the lane pipelines from this batch size on" — is honoured: with it set the wave route ends there.)
    size_t l3WaveMax = 8192; if (const char* ov = zj_env("ZJNI_L3_WAVE_MAX")) l3WaveMax = (size_t)atoll(ov);
    if (const char* ov = zj_env("ZJNI_SPLIT_MIN")) { size_t const v = (size_t)atoll(ov); if (v < l3WaveMax) l3WaveMax = v; }
    bool const l3wave = level == 3 && tuned && n < l3WaveMax && !g_scratch_limit;      // (tuned: table sizes beyond the LDS — the level's own 16 / 15 included; explicit 14 / 13 keeps the LDS matcher of small batches)
    if (l3wave) levelWord |= (int)ZE_LW_WAVE_ROUTE;
    u32 const ldsA = level > 3 ? 0u : (u32)enc_lds_pass0(level);
    hipLaunchKernelGGL(zj_enc_classify_kernel, dim3((u32)((n + 255) / 256)), dim3(256), 0, st, (const u64*)d_src_off, (u64*)d_result,
                       (u32)n, (u32)levelWord, ldsA, ctr, listA, listB, listC);
    // The wide slice (list B: frames of 64 KiB + 1 .. 128 KiB, ~1.1 MiB of tables and records per frame of a 65 536-frame slice) is allocated when a call HAS such
    // frames (rounds 1-5: by any large level 1-3 call, 72 GiB).  While it does not exist the list counts come back to pinned memory behind an event, and the call waits
    // for them where it would allocate — by then list A's kernels are queued, so the device is not kept waiting; once it exists nothing is asked.
    bool listsAsked = false;
    if (level <= 3 && d->encStat && d->wideBufCap == 0 && !l3wave)
        listsAsked = hipMemcpyAsync((void*)d->encStat, ctr, 24, hipMemcpyDeviceToHost, st) == hipSuccess && hipEventRecord(d->evLists, st) == hipSuccess;
    // levels 4-8, frames of 16-128 KiB: one lane per frame when the batch is large (below) and the scratch budget has room for a table set
    // per lane slot, else one wave per frame (here)
    // (level 4 is double-fast: its frames above 16 KiB stay on list C, where the wave matcher of zj_match_wavex.h parses them — two waves per
    //  SIMD each on its own frame beat 256 waves of one-lane parses; ZJNI_L4_LANES=1 keeps the lane-slot route selectable for A/B runs)
    bool const l4wave = level == 4 && !(zj_tune("ZJNI_L4_LANES") && atoi(zj_tune("ZJNI_L4_LANES")) == 1);
    bool const bigLanes = level > 3 && !l4wave && n >= 4096 && (!g_scratch_limit || g_scratch_limit >= ((size_t)48 << 30));
    if (!bigLanes)
    {   // list C: multi-block frames (levels 1-3) and the single-block frames of levels 4-8 above 16 KiB.  The launch is unconditional (an empty list costs an empty kernel); its tables are a fixed 1 MiB per resident workgroup.
        if (!ensure_multi_tables(d)) return ZJNI_ERR(64);
        u32 const gc = (u32)(n < (size_t)d->multiGrid ? n : (size_t)d->multiGrid);
        // blocks of multi-block frames: the wave matchers (zj_match_wavex.h: double-fast at level 3, fast at levels 1-2); ZJNI_MULTI_WAVE=0 keeps the one-lane parse selectable for A/B runs, =2 the wave matcher without staged spans
        u32 multiSerial = 0; if (const char* ov = zj_tune("ZJNI_MULTI_WAVE")) { int const v = atoi(ov); multiSerial = v == 0 ? ZE_FLAG_MULTI_SERIAL : (v == 2 ? ZE_FLAG_MULTI_NOCARRY : 0u); }
        // levels 1-2 (fast strategy): the one-lane parse unless ZJNI_MULTI_WAVE_FAST=1 — the wave version (ZWaveF) is exact but measured slower there
        // (2 048 x 512 KiB at level 1: 156 ms against 138; one 64 KiB table per frame stays in the L2 / Infinity Cache and an iteration of the one-lane loop is one short trip)
        {   const char* const ov = zj_tune("ZJNI_MULTI_WAVE_FAST"); if (!(ov && atoi(ov) == 1)) multiSerial |= ZE_FLAG_MULTI_FAST_SERIAL; }
        // Batches that leave wave slots empty (every frame resident at once and room to spare) take the pipelined kernel: a parse wave a block ahead of an entropy wave per
        // frame — 1 024 x 1 MiB: the frame's chain is the parse alone.  With the slots full the one-wave kernel does the same work in fewer wave-milliseconds.
        // ZJNI_PIPE_MAX (tuning builds): the largest batch that takes it (0: never).
        u32 pipeMax = level <= 3 ? (u32)d->pipeGrid : 0u; if (const char* ov = zj_tune("ZJNI_PIPE_MAX")) { long long const v = atoll(ov); pipeMax = v <= 0 ? 0u : ((size_t)v < (size_t)d->pipeGrid ? (u32)v : (u32)d->pipeGrid); }
        if (neg) pipeMax = 0u;                                      // negative levels: zj_encode_multi_kernel_neg, never the pipelined kernel
        d->lastPipeMax = pipeMax;
        if (pipeMax) {
            u32 const gp = (u32)(n < (size_t)pipeMax ? n : (size_t)pipeMax);
            hipLaunchKernelGGL(zj_encode_pipe_kernel, dim3(gp), dim3(128), (u32)(((sizeof(ZEEntropy) + 15u) & ~(size_t)15) + ZJ_PIPE_LDS_P), st, (const u8*)d_src, (const u64*)d_src_off, (u8*)d_dst, (const u64*)d_dst_off,
                               (u64*)d_result, (u32)levelWord, (const u32*)listC, (const u32*)(ctr + 4), ctr + 5, d->encScratch, d->multiTables, flags | multiSerial, (u32)sizeof(ZEEntropy), pipeMax);
        }
        hipLaunchKernelGGL(neg ? zj_encode_multi_kernel_neg : zj_encode_multi_kernel, dim3(gc), dim3(64), (u32)sizeof(ZEEntropy), st, (const u8*)d_src, (const u64*)d_src_off, (u8*)d_dst, (const u64*)d_dst_off,
                           (u64*)d_result, (u32)levelWord, (const u32*)listC, (const u32*)(ctr + 4), ctr + 5, d->encScratch, d->multiTables, flags | multiSerial, (u32)sizeof(ZEEntropy), pipeMax);
    }
    if (l3wave) {                                  // the whole batch was list C's
        d->lastRoute = ZJ_ROUTE_WAVE_HBM; d->tevCompress = false;
        d->clearedValid = wasCleared;              // the lane pipeline's scratch was not touched: what the previous call promised about its tables still holds
        return hipGetLastError() == hipSuccess ? 0 : ZJNI_ERR(ZJNI_ERROR_no_device);
    }
    // Everything below places something in splitBuf.  A clear the previous call queued on clearStream (24 GiB: 5-6 ms) may still be running — BatchOrder only
    // chains `st` to `st` — so EVERY user of the buffer first orders itself behind it, not only the branch that skips its own memset (levels 4-8, the LDS matcher
    // of small batches and a level 1-3 call with larger tables used to start under the running clear: records and table entries zeroed mid-parse).
    if (wasCleared && hipStreamWaitEvent(st, d->evCleared, 0) != hipSuccess) return ZJNI_ERR(ZJNI_ERROR_no_device);
    if (level > 3) {
        // list A of levels 4-8 (frames <= 16 KiB): chain parsers lane-per-frame, then the entropy kernel on their records
        u32 const maxSrcC = ZE_CHAIN_MAX_SRC;
        size_t const tablesBytes = n * (size_t)ZE_CHAIN_TABLE_BYTES, fsBytes = n * (size_t)ZE_FRAME_STRIDE(maxSrcC), metaBytes = n * 12;
        size_t const need = tablesBytes + fsBytes + metaBytes + 256;
        if (d->splitBufCap < need) {
            if (!scratch_make_room(d, d->splitBufCap, need)) return ZJNI_ERR(64);
            if (d->splitBuf) { if (hipStreamSynchronize(st) != hipSuccess) return ZJNI_ERR(ZJNI_ERROR_no_device); (void)hipFree(d->splitBuf); d->splitBuf = nullptr; d->splitBufCap = 0; wasCleared = false; }
            if (hipMalloc(&d->splitBuf, need) != hipSuccess) return ZJNI_ERR(64);
            d->splitBufCap = need;
        }
        u8* const tables = d->splitBuf; u8* const fs = d->splitBuf + tablesBytes; u32* const mt = (u32*)(fs + fsBytes);
        u32* const mctr = d->counters + 24;
        if (hipMemsetAsync(mctr, 0, 16, st) != hipSuccess || hipMemsetAsync(tables, 0, tablesBytes, st) != hipSuccess) return ZJNI_ERR(ZJNI_ERROR_no_device);
        u32 const waves = (u32)((n + 63) / 64);
        hipLaunchKernelGGL(zj_enc_match_chain_kernel, dim3(waves < (u32)d->matchGrid * 2u ? waves : (u32)d->matchGrid * 2u), dim3(64), 0, st, (const u8*)d_src, (const u64*)d_src_off,
                           (u32)levelWord, (const u32*)listA, (const u32*)ctr, mctr, tables, fs, mt);
        u32 const ldsRun = (u32)sizeof(ZEEntropy);
        u32 const gridA = (u32)(n < (size_t)d->encGridLvl[1] ? n : (size_t)d->encGridLvl[1]);
        hipLaunchKernelGGL(zj_encode_kernel, dim3(gridA), dim3(64), ldsRun, st, (const u8*)d_src, (const u64*)d_src_off, (u8*)d_dst,
                           (const u64*)d_dst_off, (u64*)d_result, (u32)levelWord, (const u32*)listA, (const u32*)ctr, ctr + 2, d->encScratch, (unsigned long long*)nullptr,
                           fs, maxSrcC, (const u32*)mt, 0u, (const u32*)nullptr, (u32*)nullptr, flags, (const ZECDictDev*)nullptr, (u32)(ldsRun), 0u, 0xFFFFFFFFu);
        if (bigLanes) {
            // list C in slices of ZJ_BIG_SLICE frames: [table set per lane slot][records per frame of the slice][meta]
            size_t bigWaves = (size_t)d->numCU;           // measured at level 5, 65 536 x 64 KiB: 128 / 256 / 512 / 1 024 waves -> 3.69 / 1.95 / 2.44 / 2.74 s (1 MiB of table per lane slot: beyond one wave per CU the rows' random requests take over)
            if (const char* ov = zj_tune("ZJNI_BIG_WAVES")) { long const v = atol(ov); if (v >= 1 && v <= 4096) bigWaves = (size_t)v; }
            size_t const slots = bigWaves * 64, tablesB = slots * ZE_MULTI_TABLE_BYTES;
            size_t const fsB = (size_t)ZJ_BIG_SLICE * ZE_FRAME_STRIDE(ZE_BLOCK_MAX), needB = tablesB + fsB + (size_t)ZJ_BIG_SLICE * 12 + 256;
            if (d->wideBufCap < needB) {
                if (!scratch_make_room(d, d->wideBufCap, needB)) return ZJNI_ERR(64);
                if (d->wideBuf) { if (hipStreamSynchronize(st) != hipSuccess) return ZJNI_ERR(ZJNI_ERROR_no_device); (void)hipFree(d->wideBuf); d->wideBuf = nullptr; d->wideBufCap = 0; }
                if (hipMalloc(&d->wideBuf, needB) != hipSuccess) return ZJNI_ERR(64);
                d->wideBufCap = needB;
            }
            u32* const tb = (u32*)d->wideBuf; u8* const fsb = d->wideBuf + tablesB; u32* const mtb = (u32*)(fsb + fsB);
            u32* const wctr = d->counters + 48;       // [2s] match work, [2s + 1] entropy work of slice s
            size_t const passes = (n + ZJ_BIG_SLICE - 1) / ZJ_BIG_SLICE;
            if (hipMemsetAsync(wctr, 0, 8 * passes, st) != hipSuccess) return ZJNI_ERR(ZJNI_ERROR_no_device);
            for (size_t sN = 0; sN < passes; sN++) {
                u32 const base = (u32)(sN * ZJ_BIG_SLICE);
                hipLaunchKernelGGL(zj_enc_match_big_kernel, dim3((u32)(slots / 64)), dim3(64), 0, st, (const u8*)d_src, (const u64*)d_src_off, (u32)levelWord,
                                   (const u32*)listC, (const u32*)(ctr + 4), wctr + 2 * sN, tb, fsb, mtb, base, (u32)ZJ_BIG_SLICE);
                u32 const gridB = (u32)(ZJ_BIG_SLICE < (size_t)d->encGridLvl[1] ? ZJ_BIG_SLICE : (size_t)d->encGridLvl[1]);
                hipLaunchKernelGGL(zj_encode_kernel, dim3(gridB), dim3(64), ldsRun, st, (const u8*)d_src, (const u64*)d_src_off, (u8*)d_dst,
                                   (const u64*)d_dst_off, (u64*)d_result, (u32)levelWord, (const u32*)listC, (const u32*)(ctr + 4), wctr + 2 * sN + 1, d->encScratch, (unsigned long long*)nullptr,
                                   fsb, (u32)ZE_BLOCK_MAX, (const u32*)mtb, 0u, (const u32*)nullptr, (u32*)nullptr, flags, (const ZECDictDev*)nullptr, (u32)(ldsRun), base, (u32)ZJ_BIG_SLICE);
            }
        }
        return hipGetLastError() == hipSuccess ? 0 : ZJNI_ERR(ZJNI_ERROR_no_device);
    }
    // Large batches: match finding goes lane-per-frame (64 frames per wave) ahead of the wave-per-frame
    // entropy stage; small batches keep the fused wave-per-frame kernel (lower latency, tables in LDS).
    size_t splitMin = 4096;
    if (const char* ov = zj_env("ZJNI_SPLIT_MIN")) splitMin = (size_t)atoll(ov);
    if (tuned) splitMin = 1;                      // explicit table sizes exist only on the lane-per-frame path (tables in HBM)
    u8* fscratch = nullptr; u32* meta = nullptr; u32 const maxSrc = 65536u;
    // Small level-3 batches: list A goes through the wave-per-frame matcher (tables in LDS, 64 positions per step) and the
    // entropy kernel instead of the fused kernel, whose match finder is one lane walking the frame (3-10x the latency).
    bool const smallWave = n < splitMin && level == 3 && !tuned && zj_tune("ZJNI_NO_OVERLAP") == nullptr && zj_tune("ZJNI_NO_WAVE") == nullptr;
    if (n >= splitMin || smallWave) {
        u32 const tableStride = ze_lane_table_stride((u32)levelWord, false);   // fast: u16 entries; dfast: 4-byte tagged entries
        size_t const tablesBytes = smallWave ? 0 : n * (size_t)tableStride, fsBytes = n * (size_t)ZE_FRAME_STRIDE(maxSrc), metaBytes = n * 12, qBytes = n * 4;
        // Level 3, large batches: the run machine (zj_match_run.h), with need flags (zj_need.h: a flag byte per position, computed BESIDE the match
        // kernel) for the frames they pay on.  ZJNI_NEED: 2 (default) = the frames zn_worth() picks — search-dense frames over a small alphabet —
        // 1 = every frame, 0 = none.  64 KiB of flags per frame slot: left out under a scratch budget (zjni_set_scratch_limit) and when the device
        // cannot spare them; the machine then runs with every flag set.  ZJNI_LANE_MACHINE=0: the previous machine (ZLaneD), for A/B runs.
        u32 needMode = 2;
        if (const char* ov = zj_env("ZJNI_NEED")) needMode = (u32)atoi(ov);
        bool const overlap = zj_tune("ZJNI_NO_OVERLAP") == nullptr;
        bool const runMachine = level == 3 && !smallWave && zj_tune("ZJNI_HYBRID") == nullptr && !(zj_tune("ZJNI_LANE_MACHINE") && atoi(zj_tune("ZJNI_LANE_MACHINE")) == 0);
        u32 const hlN = ZE_LW_HL(levelWord) ? ZE_LW_HL(levelWord) : (tuned ? 16u : (u32)ZE_L3_HASHLOG), clN = ZE_LW_CL(levelWord) ? ZE_LW_CL(levelWord) : (tuned ? 15u : (u32)ZE_L3_CHAINLOG);
        bool needGate = (needMode == 1 || needMode == 2) && level == 3 && !smallWave && !g_scratch_limit && zj_tune("ZJNI_HYBRID") == nullptr
                        && overlap && hlN <= ZN_MAX_LOG_L && clN <= ZN_MAX_LOG_S;
        if (needGate && !d->needLdsSet) {                    // more than 64 KiB of dynamic LDS has to be asked for, once per device; refused: no flags
            if (hipFuncSetAttribute((const void*)zj_enc_need_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(ZNLds)) == hipSuccess) d->needLdsSet = true;
            else { (void)hipGetLastError(); needGate = false; }
        }
        u32 const needSelective = needMode >= 2 ? 1u : 0u;
        size_t needFlagBytes = needGate ? n * (size_t)ZN_FLAG_STRIDE + 9 * n + 384 : 0;     // flags, gate bytes, ready words, pick list
        size_t need = tablesBytes + fsBytes + metaBytes + 2 * qBytes + n + 256 + needFlagBytes;
        if (d->splitBufCap < need) {
            if (!scratch_make_room(d, d->splitBufCap, need)) return ZJNI_ERR(64);
            if (d->splitBuf) { if (hipStreamSynchronize(st) != hipSuccess) return ZJNI_ERR(ZJNI_ERROR_no_device); (void)hipFree(d->splitBuf); d->splitBuf = nullptr; d->splitBufCap = 0; wasCleared = false; }
            if (hipMalloc(&d->splitBuf, need) != hipSuccess) {
                if (!needGate) return ZJNI_ERR(64);
                (void)hipGetLastError(); needGate = false; need -= needFlagBytes; needFlagBytes = 0;          // no room for the flags
                if (hipMalloc(&d->splitBuf, need) != hipSuccess) return ZJNI_ERR(64);
            }
            d->splitBufCap = need;
        }
        u8* const tables = d->splitBuf; fscratch = d->splitBuf + tablesBytes; meta = (u32*)(fscratch + fsBytes);
        u32* const doneList = (u32*)((u8*)meta + metaBytes); u32* const procFlag = doneList + n; u8* const score = (u8*)(procFlag + n);
        u8* const needFlags = needGate ? (u8*)(((uintptr_t)(score + n) + 63) & ~(uintptr_t)63) : nullptr;
        u32* const needReady = needGate ? (u32*)(needFlags + n * (size_t)ZN_FLAG_STRIDE) : nullptr;       // (ZN_FLAG_STRIDE is a multiple of 16)
        u32* const needPick = needGate ? needReady + n : nullptr;
        u8* const needGateMap = needGate ? (u8*)(needPick + n) : nullptr;
        u32* const needCtr = d->counters + 208;             // [0] flag kernel's work queue, [1] picked frames

        u32* const mctr = d->counters + 24;       // [0] match work, [1] completion-queue length, [2] work of the sweep pass
        // Experiment (ZJNI_HYBRID=1, off by default): at level 3 with the LDS-sized tables the two match
        // finders share a large batch — the list is partitioned by search density, the lane-per-frame kernel (tables in HBM,
        // bound by their random requests) takes the match-dense part, the wave-per-frame kernel (tables in LDS) the rest.
        // Measured on the metric configuration it does not pay: the wave kernel needs the LDS the entropy kernel runs in,
        // and under the lane kernel's traffic it falls to half its stand-alone rate.
        bool const hybrid = smallWave || (overlap && level == 3 && !tuned && zj_tune("ZJNI_HYBRID") != nullptr && zj_tune("ZJNI_NO_WAVE") == nullptr);
        bool const waveOnly = smallWave || (hybrid && zj_tune("ZJNI_WAVE_ONLY") != nullptr);
        unsigned long long* const work2 = (unsigned long long*)(d->counters + 192);
        const u32* listM = listA;
        if (hybrid && hipMemsetAsync(work2, 0, 32, st) != hipSuccess) return ZJNI_ERR(ZJNI_ERROR_no_device);   // split = 0: the whole list is the wave kernel's
#ifdef ZJ_TUNING_KERNELS
        if (hybrid && !waveOnly) {
            u32 const gs = (u32)(n < (size_t)d->numCU * 16 ? n : (size_t)d->numCU * 16);
            u32 threshold = 40;                       // text / JSON-like frames score 15-25, frames searched position by position 50+
            if (const char* ov = zj_tune("ZJNI_WAVE_SCORE")) threshold = (u32)atoi(ov);
            u32 share = 150;                          // permille of the batch the wave kernel takes at most
            if (const char* ov = zj_tune("ZJNI_WAVE_SHARE")) share = (u32)atoi(ov);
            hipLaunchKernelGGL(zj_enc_score_kernel, dim3(gs), dim3(64), 0, st, (const u8*)d_src, (const u64*)d_src_off, (const u32*)listA, (const u32*)ctr, score);
            hipLaunchKernelGGL(zj_enc_partition_kernel, dim3((u32)((n + 255) / 256)), dim3(256), 0, st, (const u32*)listA, (const u32*)ctr, (const u8*)score, threshold, share, work2, listS);
            hipLaunchKernelGGL(zj_enc_partition_done_kernel, dim3(1), dim3(1), 0, st, (const u32*)ctr, share, work2);
            listM = listS;
        }
#endif
        int const preclearEnv = (zj_tune("ZJNI_PRECLEAR") && atoi(zj_tune("ZJNI_PRECLEAR")) == 0) ? 0 : 1;
        if (tablesBytes) {
            if (wasCleared && d->clearedPtr == tables && d->clearedBytes >= tablesBytes) {          // the previous call left them zero: `st` already waits for evCleared (above)
            } else if (hipMemsetAsync(tables, 0, tablesBytes, st) != hipSuccess) return ZJNI_ERR(ZJNI_ERROR_no_device);
        }
        // after this call's match kernels (recorded below, at tev[1]): the same range zeroed again for the next call
        auto preclear = [&]() {
            if (!preclearEnv || !tablesBytes || g_scratch_limit) return;
            if (hipEventRecord(d->evMatchDone, st) != hipSuccess || hipStreamWaitEvent(d->clearStream, d->evMatchDone, 0) != hipSuccess) return;
            if (hipMemsetAsync(tables, 0, tablesBytes, d->clearStream) != hipSuccess || hipEventRecord(d->evCleared, d->clearStream) != hipSuccess) { (void)hipStreamSynchronize(d->clearStream); return; }
            d->clearedPtr = tables; d->clearedBytes = tablesBytes; d->clearedValid = true;
        };
        if (hipMemsetAsync(mctr, 0, 12, st) != hipSuccess) return ZJNI_ERR(ZJNI_ERROR_no_device);
        u32 const waves = (u32)((n + 63) / 64);
        u32 gridM = waves < (u32)d->matchGrid ? waves : (u32)d->matchGrid;
        if (const char* ov = zj_tune("ZJNI_MATCH_GRID")) { u32 const v = (u32)atoi(ov); if (v >= 1 && v < gridM) gridM = v; }   // experiments: fewer resident waves, more frames per lane
        // with the sequences already found the entropy kernel only needs the entropy-stage LDS (more workgroups per CU)
        u32 const ldsRun = (u32)sizeof(ZEEntropy);
        u32 const gridA = (u32)(n < (size_t)d->encGridLvl[1] ? n : (size_t)d->encGridLvl[1]);
        unsigned long long* const eprof = d->prof ? d->prof + 16 : nullptr;
        if (needGate) {      // which frames get flags: decided ahead of the fork, a few microseconds per thousand frames
            if (hipMemsetAsync(needCtr, 0, 8, st) != hipSuccess) return ZJNI_ERR(ZJNI_ERROR_no_device);
            u32 const gw = (u32)(n < (size_t)d->numCU * 8 ? n : (size_t)d->numCU * 8);
            hipLaunchKernelGGL(zj_enc_worth_kernel, dim3(gw), dim3(256), 0, st, (const u8*)d_src, (const u64*)d_src_off, (const u32*)listA, (const u32*)ctr,
                               needGateMap, needReady, needSelective, needPick, needCtr + 1);
            zj_dbg_sync("zj_enc_worth_kernel");
        }
        // an error return after work has been queued on the side streams must not leave it running over scratch the next call reuses
        auto bail = [&](size_t code) { (void)hipStreamSynchronize(d->sideStream); (void)hipStreamSynchronize(d->waveStream); (void)hipStreamSynchronize(st); return code; };
        if (overlap) {
            // The entropy kernel runs on a side stream BESIDE the match kernel and consumes its completion queue:
            // frames that parse quickly are entropy-coded while the slow ones still occupy their lanes (the match
            // kernel leaves most of every CU idle in its tail).  A sweep pass afterwards takes whatever the side
            // kernel did not get to (its waits are bounded), so completion never depends on the two kernels
            // actually being co-scheduled.
            if (hipMemsetAsync(doneList, 0xFF, qBytes, st) != hipSuccess || hipMemsetAsync(procFlag, 0, qBytes, st) != hipSuccess) return ZJNI_ERR(ZJNI_ERROR_no_device);
            if (hipEventRecord(d->evFork, st) != hipSuccess || hipStreamWaitEvent(d->sideStream, d->evFork, 0) != hipSuccess) return bail(ZJNI_ERR(ZJNI_ERROR_no_device));
            if ((hybrid || needGate) && hipStreamWaitEvent(d->waveStream, d->evFork, 0) != hipSuccess) return bail(ZJNI_ERR(ZJNI_ERROR_no_device));
            if (needGate) {      // the flag kernel on its own stream, enqueued before the entropy kernel: its workgroups take 140 KiB of LDS each (sizeof(ZNLds)), which a CU full of waiting entropy workgroups does not have
                u32 const gn = (u32)(n < (size_t)d->numCU ? n : (size_t)d->numCU);
                hipLaunchKernelGGL(zj_enc_need_kernel, dim3(gn), dim3(zj_need_threads()), sizeof(ZNLds), zj_tune("ZJNI_NEED_INLINE") ? st : d->waveStream, (const u8*)d_src, (const u64*)d_src_off, (u32)levelWord,
                                   (const u32*)listA, (const u32*)needPick, (const u32*)(needCtr + 1), needFlags, needReady, needCtr, (u32)ZN_FLAG_STRIDE);
                if (hipEventRecord(d->evJoinWave, d->waveStream) != hipSuccess) return bail(ZJNI_ERR(ZJNI_ERROR_no_device));
                zj_dbg_sync("zj_enc_need_kernel");
            }
            (void)hipEventRecord(d->tev[0], st);
            if (hybrid) {
                u32 const gw = (u32)(n < (size_t)d->waveGrid ? n : (size_t)d->waveGrid);
                hipLaunchKernelGGL(zj_enc_match_wave_kernel, dim3(gw), dim3(64), sizeof(ZWLds), d->waveStream, (const u8*)d_src, (const u64*)d_src_off, (u32)levelWord,
                                   listM, (const u32*)ctr, work2, fscratch, maxSrc, meta, doneList, mctr + 1);
                if (hipEventRecord(d->evJoinWave, d->waveStream) != hipSuccess) return bail(ZJNI_ERR(ZJNI_ERROR_no_device));
            }
            u32 lanePeriod = 0;                                    // rotation period of the double-fast lane machines (0 = the machine's own)
            if (const char* ov = zj_tune("ZJNI_LANE_PERIOD"); ov && !neg) { lanePeriod = (u32)atoi(ov) & 0xFu; if (lanePeriod && lanePeriod < 3u) lanePeriod = 3u; }     // (three non-search states take turns: a shorter rotation would never run one of them)
            if (runMachine) {
                void (*kern)(const u8*, const u64*, u32, const u32*, const u32*, u32*, u8*, u32, u8*, u32, u32*, u32*, u32*, u32, u32, const u8*, const u8*, const u32*) = zj_enc_match_run_kernel;
#ifdef ZJ_TUNING_KERNELS
                if (const char* ov = zj_tune("ZJNI_RUN_JMAX")) { int const j = atoi(ov); kern = j == 3 ? zj_enc_match_run3_kernel : j == 4 ? zj_enc_match_run4_kernel : j == 6 ? zj_enc_match_run6_kernel : j == 7 ? zj_enc_match_run7_kernel : zj_enc_match_run_kernel; }
#endif
                hipLaunchKernelGGL(kern, dim3(gridM), dim3(64), 0, st, (const u8*)d_src, (const u64*)d_src_off, (u32)levelWord | (lanePeriod << 24),
                                   listM, (const u32*)ctr, mctr, tables, tableStride, fscratch, maxSrc, meta, doneList, mctr + 1, 0u, 0xFFFFFFFFu, (const u8*)needFlags, (const u8*)needGateMap, (const u32*)needReady);
                d->lastRoute = needGate ? ZJ_ROUTE_RUN_FLAGS : ZJ_ROUTE_RUN;
            }
#ifdef ZJ_TUNING_KERNELS
            else if (needGate) {
                hipLaunchKernelGGL(zj_enc_match_gated_kernel, dim3(gridM), dim3(64), 0, st, (const u8*)d_src, (const u64*)d_src_off, (u32)levelWord | (lanePeriod << 24),
                                   listM, (const u32*)ctr, mctr, tables, tableStride, fscratch, maxSrc, meta, doneList, mctr + 1, 0u, 0xFFFFFFFFu, (const u8*)needFlags, (const u8*)needGateMap, (const u32*)needReady);
                d->lastRoute = ZJ_ROUTE_LANE_GATED;
            }
#endif
            else if (!waveOnly) {
            hipLaunchKernelGGL(neg ? zj_enc_match_kernel_neg : zj_enc_match_kernel, dim3(gridM), dim3(64), 0, st, (const u8*)d_src, (const u64*)d_src_off, (u32)levelWord | (lanePeriod << 24),
                               listM, (const u32*)ctr, mctr, tables, tableStride, fscratch, maxSrc, meta, doneList, mctr + 1, 0u, 0xFFFFFFFFu,
                               hybrid ? work2 : (unsigned long long*)nullptr);
            d->lastRoute = hybrid ? ZJ_ROUTE_HYBRID : ZJ_ROUTE_LANE;
            } else d->lastRoute = ZJ_ROUTE_WAVE;
            if (needGate && hipStreamWaitEvent(st, d->evJoinWave, 0) != hipSuccess) return bail(ZJNI_ERR(ZJNI_ERROR_no_device));
            zj_dbg_sync("match kernel");
            if (hybrid && hipStreamWaitEvent(st, d->evJoinWave, 0) != hipSuccess) return bail(ZJNI_ERR(ZJNI_ERROR_no_device));
            (void)hipEventRecord(d->tev[1], st); d->tevCompress = true;
            preclear();
            // the entropy kernel's persistent workgroups fill the LDS of every CU; the flag kernel's need 140 KiB each: the entropy kernel starts when the flags are done
            // (measured without this: whichever kernel the dispatcher places first wins, and every second call the picked frames' lanes wait out their 50 ms)
            if (needGate && !zj_tune("ZJNI_NEED_INLINE") && hipStreamWaitEvent(d->sideStream, d->evJoinWave, 0) != hipSuccess) return bail(ZJNI_ERR(ZJNI_ERROR_no_device));
            u32 gridE = gridA;                                  // (ZJNI_ENT_GRID: fewer entropy workgroups beside the match kernel — with <= 1 024 every match wave is resident from the start, profiles/r05/b_; the call's time does not move)
            if (const char* ov = zj_tune("ZJNI_ENT_GRID")) { u32 const v = (u32)atoi(ov); if (v >= 1 && v < gridE) gridE = v; }
            hipLaunchKernelGGL(zj_encode_kernel, dim3(gridE), dim3(64), ldsRun, d->sideStream, (const u8*)d_src, (const u64*)d_src_off, (u8*)d_dst,
                               (const u64*)d_dst_off, (u64*)d_result, (u32)levelWord, listM, (const u32*)ctr, ctr + 2, d->encScratch, eprof,
                               fscratch, maxSrc, (const u32*)meta, 1u, (const u32*)doneList, procFlag, flags, (const ZECDictDev*)nullptr, (u32)(ldsRun), 0u, 0xFFFFFFFFu);
            if (hipEventRecord(d->evJoin, d->sideStream) != hipSuccess || hipStreamWaitEvent(st, d->evJoin, 0) != hipSuccess) return bail(ZJNI_ERR(ZJNI_ERROR_no_device));
            hipLaunchKernelGGL(zj_encode_kernel, dim3(gridA), dim3(64), ldsRun, st, (const u8*)d_src, (const u64*)d_src_off, (u8*)d_dst,
                               (const u64*)d_dst_off, (u64*)d_result, (u32)levelWord, listM, (const u32*)ctr, mctr + 2, d->encScratch, eprof,
                               fscratch, maxSrc, (const u32*)meta, 2u, (const u32*)doneList, procFlag, flags, (const ZECDictDev*)nullptr, (u32)(ldsRun), 0u, 0xFFFFFFFFu);
        } else {
            (void)hipEventRecord(d->tev[0], st);
            d->lastRoute = runMachine ? ZJ_ROUTE_RUN : ZJ_ROUTE_LANE;
            if (runMachine)
                hipLaunchKernelGGL(zj_enc_match_run_kernel, dim3(gridM), dim3(64), 0, st, (const u8*)d_src, (const u64*)d_src_off, (u32)levelWord,
                                   (const u32*)listA, (const u32*)ctr, mctr, tables, tableStride, fscratch, maxSrc, meta, (u32*)nullptr, (u32*)nullptr, 0u, 0xFFFFFFFFu, (const u8*)nullptr, (const u8*)nullptr, (const u32*)nullptr);
            else
            hipLaunchKernelGGL(neg ? zj_enc_match_kernel_neg : zj_enc_match_kernel, dim3(gridM), dim3(64), 0, st, (const u8*)d_src, (const u64*)d_src_off, (u32)levelWord,
                               (const u32*)listA, (const u32*)ctr, mctr, tables, tableStride, fscratch, maxSrc, meta, (u32*)nullptr, (u32*)nullptr, 0u, 0xFFFFFFFFu, (unsigned long long*)nullptr);
            (void)hipEventRecord(d->tev[1], st); d->tevCompress = true;
            preclear();
            hipLaunchKernelGGL(zj_encode_kernel, dim3(gridA), dim3(64), ldsRun, st, (const u8*)d_src, (const u64*)d_src_off, (u8*)d_dst,
                               (const u64*)d_dst_off, (u64*)d_result, (u32)levelWord, (const u32*)listA, (const u32*)ctr, ctr + 2, d->encScratch, eprof,
                               fscratch, maxSrc, (const u32*)meta, 0u, (const u32*)nullptr, (u32*)nullptr, flags, (const ZECDictDev*)nullptr, (u32)(ldsRun), 0u, 0xFFFFFFFFu);
        }
    } else {
        // small batches: the fused wave-per-frame kernel (match finding on lane 0 with the tables in LDS)
        d->lastRoute = ZJ_ROUTE_FUSED;
        u32 const gridA = (u32)(n < (size_t)d->encGridLvl[level] ? n : (size_t)d->encGridLvl[level]);
        hipLaunchKernelGGL(zj_encode_kernel, dim3(gridA), dim3(64), ldsA, st, (const u8*)d_src, (const u64*)d_src_off, (u8*)d_dst,
                           (const u64*)d_dst_off, (u64*)d_result, (u32)levelWord, (const u32*)listA, (const u32*)ctr, ctr + 2, d->encScratch, d->prof ? d->prof + 16 : nullptr,
                           (u8*)nullptr, maxSrc, (const u32*)nullptr, 0u, (const u32*)nullptr, (u32*)nullptr, flags, (const ZECDictDev*)nullptr, (u32)(ldsA), 0u, 0xFFFFFFFFu);
    }
    if (n >= splitMin) {
        // List B (frames > 64 KiB, fast-strategy frames with larger tables) through the same two stages, in slices that
        // share one scratch area sized for 4-byte positions and 128 KiB frames; a slice past the end of the list is empty.
        auto bailB = [&](size_t code) { (void)hipStreamSynchronize(d->sideStream); (void)hipStreamSynchronize(d->waveStream); (void)hipStreamSynchronize(st); return code; };
        size_t sliceB = 65536;                       // as many lanes as the common path runs: 32 768 leaves half the wave slots empty (13.8 vs 18.5 GiB/s on 128 KiB frames)
        if (const char* ov = zj_env("ZJNI_WIDE_SLICE")) sliceB = (size_t)atoll(ov);
        sliceB = scratch_slice((size_t)ze_lane_table_stride((u32)levelWord, true) + ZE_FRAME_STRIDE(ZE_WIDE_MAX_SRC) + 12, sliceB, 2);   // half the budget: the common-case buffer of this call has the other half
        if (sliceB > n) sliceB = n;
        if (sliceB < 64) sliceB = 64;
        u32 const strideB = ze_lane_table_stride((u32)levelWord, true);
        size_t const tablesB = sliceB * (size_t)strideB, fsB = sliceB * (size_t)ZE_FRAME_STRIDE(ZE_WIDE_MAX_SRC), metaB = sliceB * 12, qB = sliceB * 4;
        // The entropy kernel BESIDE the match kernel, as on the common path: it takes frames off the completion queue while the slow frames still occupy
        // their lanes; a sweep pass afterwards takes what it did not get to.  ZJNI_NO_OVERLAP: one after the other (A/B runs).
        bool const besideB = zj_tune("ZJNI_NO_OVERLAP") == nullptr;
        // Level 3: need flags for the frames zj_enc_worth_kernel picks (zn_flags_frame_wide: 64 KiB + 1 .. 128 KiB) and the run machine for the slice — what the common
        // path does for frames to 64 KiB.  Only when one slice holds the whole list (a call's frames normally do), ZJNI_NEED / ZJNI_LANE_MACHINE as there;
        // ZJNI_NEED_WIDE=0 keeps the wide launch on ZLaneD without flags (A/B runs).
        u32 needModeB = 2; if (const char* ov = zj_env("ZJNI_NEED")) needModeB = (u32)atoi(ov);
        u32 const hlB = ZE_LW_HL(levelWord) ? ZE_LW_HL(levelWord) : (tuned ? 16u : (u32)ZE_L3_HASHLOG), clB = ZE_LW_CL(levelWord) ? ZE_LW_CL(levelWord) : (tuned ? 15u : (u32)ZE_L3_CHAINLOG);
        bool needW = level == 3 && (needModeB == 1 || needModeB == 2) && besideB && !g_scratch_limit && sliceB >= n && hlB <= ZN_MAX_LOG_L && clB <= ZN_MAX_LOG_S
                     && !(zj_tune("ZJNI_LANE_MACHINE") && atoi(zj_tune("ZJNI_LANE_MACHINE")) == 0) && !(zj_tune("ZJNI_NEED_WIDE") && atoi(zj_tune("ZJNI_NEED_WIDE")) == 0);
        if (needW && !d->needLdsSet) {
            if (hipFuncSetAttribute((const void*)zj_enc_need_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(ZNLds)) == hipSuccess) d->needLdsSet = true;
            else { (void)hipGetLastError(); needW = false; }
        }
        size_t flagB = needW ? sliceB * (size_t)ZN_FLAG_STRIDE_WIDE + 9 * sliceB + 384 : 0;      // flags, ready words, pick list, gate bytes
        size_t needB = tablesB + fsB + metaB + 2 * qB + 256 + flagB;
        if (d->wideBufCap < needB && listsAsked) {                 // no wide slice yet: is there a list B at all?
            if (hipEventSynchronize(d->evLists) != hipSuccess) return bailB(ZJNI_ERR(ZJNI_ERROR_no_device));
            if (d->encStat[1] == 0u) return hipGetLastError() == hipSuccess ? 0 : ZJNI_ERR(ZJNI_ERROR_no_device);
        }
        if (d->wideBufCap < needB) {
            if (!scratch_make_room(d, d->wideBufCap, needB)) return ZJNI_ERR(64);
            if (d->wideBuf) { if (hipStreamSynchronize(st) != hipSuccess) return ZJNI_ERR(ZJNI_ERROR_no_device); (void)hipFree(d->wideBuf); d->wideBuf = nullptr; d->wideBufCap = 0; }
            if (hipMalloc(&d->wideBuf, needB) != hipSuccess) {
                if (!needW) return ZJNI_ERR(64);
                (void)hipGetLastError(); needW = false; needB -= flagB; flagB = 0;                    // no room for the flags
                if (hipMalloc(&d->wideBuf, needB) != hipSuccess) return ZJNI_ERR(64);
            }
            d->wideBufCap = needB;
        }
        u8* const tb = d->wideBuf; u8* const fs = d->wideBuf + tablesB; u32* const mt = (u32*)(fs + fsB);
        u32* const doneB = (u32*)((u8*)mt + metaB); u32* const procB = doneB + sliceB;      // completion queue of a slice's match kernel, frames the side pass encoded
        u8* const flagsW = needW ? (u8*)(((uintptr_t)(procB + sliceB) + 63) & ~(uintptr_t)63) : nullptr;
        u32* const readyW = needW ? (u32*)(flagsW + sliceB * (size_t)ZN_FLAG_STRIDE_WIDE) : nullptr;
        u32* const pickW = needW ? readyW + sliceB : nullptr;
        u8* const gateW = needW ? (u8*)(pickW + sliceB) : nullptr;
        u32* const needCtrW = d->counters + 212;       // [0] flag kernel's work queue, [1] picked frames
        u32* const wctr = d->counters + 48;           // [0] match work, [1] entropy work (queue order), [2] queue length, [3] work of the sweep pass
        u32 const wavesB = (u32)((sliceB + 63) / 64);
        u32 const gridMB = wavesB < (u32)d->matchGrid ? wavesB : (u32)d->matchGrid;
        u32 const gridEB = (u32)(sliceB < (size_t)d->encGridLvl[1] ? sliceB : (size_t)d->encGridLvl[1]);
        for (size_t base = 0; base < n; base += sliceB) {
            if (hipMemsetAsync(wctr, 0, 16, st) != hipSuccess) return ZJNI_ERR(ZJNI_ERROR_no_device);
            hipLaunchKernelGGL(zj_zero_slots_kernel, dim3((u32)d->numCU * 8), dim3(256), 0, st, tb, strideB, (const u32*)(ctr + 1), (u32)base, (u32)sliceB);
            bool forked = false, flagged = false;
            if (besideB) {
                if (hipMemsetAsync(doneB, 0xFF, qB, st) != hipSuccess || hipMemsetAsync(procB, 0, qB, st) != hipSuccess) return ZJNI_ERR(ZJNI_ERROR_no_device);
                if (needW) {                               // which frames get flags: decided ahead of the fork
                    if (hipMemsetAsync(needCtrW, 0, 8, st) != hipSuccess) return ZJNI_ERR(ZJNI_ERROR_no_device);
                    u32 const gw = (u32)(n < (size_t)d->numCU * 8 ? n : (size_t)d->numCU * 8);
                    hipLaunchKernelGGL(zj_enc_worth_kernel, dim3(gw), dim3(256), 0, st, (const u8*)d_src, (const u64*)d_src_off, (const u32*)listB, (const u32*)(ctr + 1),
                                       gateW, readyW, needModeB >= 2 ? 1u : 0u, pickW, needCtrW + 1);
                }
                forked = hipEventRecord(d->evFork, st) == hipSuccess && hipStreamWaitEvent(d->sideStream, d->evFork, 0) == hipSuccess;
                if (forked && needW && hipStreamWaitEvent(d->waveStream, d->evFork, 0) == hipSuccess) {    // the flag kernel on its own stream, enqueued before the entropy kernel (its workgroups need 140 KiB of LDS each)
                    u32 const gn = (u32)(n < (size_t)d->numCU ? n : (size_t)d->numCU);
                    hipLaunchKernelGGL(zj_enc_need_kernel, dim3(gn), dim3(zj_need_threads()), sizeof(ZNLds), d->waveStream, (const u8*)d_src, (const u64*)d_src_off, (u32)levelWord,
                                       (const u32*)listB, (const u32*)pickW, (const u32*)(needCtrW + 1), flagsW, readyW, needCtrW, (u32)ZN_FLAG_STRIDE_WIDE);
                    flagged = hipEventRecord(d->evJoinWave, d->waveStream) == hipSuccess;
                    if (!flagged) { (void)hipStreamSynchronize(d->waveStream); (void)hipStreamSynchronize(d->sideStream); (void)hipStreamSynchronize(st); return ZJNI_ERR(ZJNI_ERROR_no_device); }
                }
            }
            (void)hipEventRecord(d->tev[8], st);
            hipLaunchKernelGGL(neg ? zj_enc_match_wide_kernel_neg : zj_enc_match_wide_kernel, dim3(gridMB), dim3(64), 0, st, (const u8*)d_src, (const u64*)d_src_off, (u32)levelWord,
                               (const u32*)listB, (const u32*)(ctr + 1), wctr, tb, strideB, fs, (u32)ZE_WIDE_MAX_SRC, mt, (u32)base, (u32)sliceB, forked ? doneB : (u32*)nullptr, forked ? wctr + 2 : (u32*)nullptr,
                               (const u8*)(flagged ? flagsW : nullptr), (const u8*)(flagged ? gateW : nullptr), (const u32*)(flagged ? readyW : nullptr));
            if (flagged && hipStreamWaitEvent(st, d->evJoinWave, 0) != hipSuccess) { (void)hipStreamSynchronize(d->waveStream); (void)hipStreamSynchronize(d->sideStream); (void)hipStreamSynchronize(st); return ZJNI_ERR(ZJNI_ERROR_no_device); }
            (void)hipEventRecord(d->tev[9], st); d->tevWide = true;
            if (flagged && hipStreamWaitEvent(d->sideStream, d->evJoinWave, 0) != hipSuccess) { (void)hipStreamSynchronize(d->waveStream); (void)hipStreamSynchronize(d->sideStream); (void)hipStreamSynchronize(st); return ZJNI_ERR(ZJNI_ERROR_no_device); }     // the entropy kernel's workgroups fill every CU's LDS: it starts when the flags are done
            if (forked) {
                hipLaunchKernelGGL(zj_encode_kernel, dim3(gridEB), dim3(64), (u32)sizeof(ZEEntropy), d->sideStream, (const u8*)d_src, (const u64*)d_src_off, (u8*)d_dst,
                                   (const u64*)d_dst_off, (u64*)d_result, (u32)levelWord, (const u32*)listB, (const u32*)(ctr + 1), wctr + 1, d->encScratch, d->prof ? d->prof + 16 : nullptr,
                                   fs, (u32)ZE_WIDE_MAX_SRC, (const u32*)mt, 1u, (const u32*)doneB, procB, flags, (const ZECDictDev*)nullptr, (u32)sizeof(ZEEntropy), (u32)base, (u32)sliceB);
                if (hipEventRecord(d->evJoin, d->sideStream) != hipSuccess || hipStreamWaitEvent(st, d->evJoin, 0) != hipSuccess) { (void)hipStreamSynchronize(d->sideStream); (void)hipStreamSynchronize(st); return ZJNI_ERR(ZJNI_ERROR_no_device); }
            }
            hipLaunchKernelGGL(zj_encode_kernel, dim3(gridEB), dim3(64), (u32)sizeof(ZEEntropy), st, (const u8*)d_src, (const u64*)d_src_off, (u8*)d_dst,
                               (const u64*)d_dst_off, (u64*)d_result, (u32)levelWord, (const u32*)listB, (const u32*)(ctr + 1), forked ? wctr + 3 : wctr + 1, d->encScratch, d->prof ? d->prof + 16 : nullptr,
                               fs, (u32)ZE_WIDE_MAX_SRC, (const u32*)mt, forked ? 2u : 0u, (const u32*)(forked ? doneB : nullptr), forked ? procB : (u32*)nullptr, flags, (const ZECDictDev*)nullptr, (u32)sizeof(ZEEntropy), (u32)base, (u32)sliceB);
        }
        return hipGetLastError() == hipSuccess ? 0 : ZJNI_ERR(ZJNI_ERROR_no_device);
    }
    u32 const gridB = (u32)(n < (size_t)d->encGridBig ? n : (size_t)d->encGridBig);
    hipLaunchKernelGGL(zj_encode_kernel, dim3(gridB), dim3(64), ZJ_ENC_LDS_BIG, st, (const u8*)d_src, (const u64*)d_src_off, (u8*)d_dst,
                       (const u64*)d_dst_off, (u64*)d_result, (u32)levelWord, (const u32*)listB, (const u32*)(ctr + 1), ctr + 3, d->encScratch, d->prof ? d->prof + 16 : nullptr,
                       (u8*)nullptr, maxSrc, (const u32*)nullptr, 0u, (const u32*)nullptr, (u32*)nullptr, flags, (const ZECDictDev*)nullptr, (u32)(ZJ_ENC_LDS_BIG), 0u, 0xFFFFFFFFu);
    return hipGetLastError() == hipSuccess ? 0 : ZJNI_ERR(ZJNI_ERROR_no_device);
}
// Level 3 with nothing set runs the reference's own tables (hashLog 16 / chainLog 15, N/compress/clevels.h:29-31 after ZSTD_adjustCParams): every frame is
// Zstd.compress(x, 3)'s, byte for byte, whatever the batch size — measured at the full batch the 4x larger tables cost nothing (153.6 vs 153.7 ms, the
// kernel is bound by request count, not footprint).  ZstdCompressCtx.setHashLog(14).setChainLog(13) selects the LDS-sized tables: the wave-per-frame
// matcher and the fused kernel of small batches (lower latency per call, 0.2 % smaller frames on the bench set, not the reference's default bytes).
// ZJNI_L3_TABLES=lds restores that as the default (A/B runs against round 2).
static int zj_level3_word(int lw) {
    u32 const w = (u32)lw;
    if (ZE_LW_LEVEL(w) != 3u || (ZE_LW_HL(w) | ZE_LW_CL(w))) return lw;
    static int const lds = (zj_tune("ZJNI_L3_TABLES") && !strcmp(zj_tune("ZJNI_L3_TABLES"), "lds")) ? 1 : 0;
    return lds ? lw : (int)(ZE_LW(3u, 16u, 15u) | ZE_LW_IMPLICIT | (w & ~0xFFFFFFu));
}
// (the caller holds the device's BatchOrder)
static size_t compress_chunked_ordered(const void* d_src, const uint64_t* d_src_off, void* d_dst, const uint64_t* d_dst_off,
                                       uint64_t* d_result, size_t n, int level, u32 flags, void* stream) {
    level = zj_negative_word(level);              // negative level -> level word (zj_encode.h: ZE_LW_NEG)
    level = zj_level3_word(level);
    size_t const perFrame = ZE_LW_LEVEL((u32)level) > 3u ? (size_t)ZE_CHAIN_TABLE_BYTES + ZE_FRAME_STRIDE(ZE_CHAIN_MAX_SRC) + 21
                                                          : (size_t)ze_lane_table_stride((u32)level, false) + ZE_FRAME_STRIDE(65536u) + 21;
    size_t const chunk = scratch_slice(perFrame, ZJ_CHUNK_FRAMES, 2);
    for (size_t at = 0; at < n || at == 0; at += chunk) {
        size_t const m = n - at < chunk ? n - at : chunk;
        size_t const r = compress_batch_device_impl(d_src, d_src_off + at, d_dst, d_dst_off + at, d_result + at, m, level, flags, stream);
        if (r != 0 || n == 0) return r;
    }
    return 0;
}
static size_t compress_chunked(const void* d_src, const uint64_t* d_src_off, void* d_dst, const uint64_t* d_dst_off,
                               uint64_t* d_result, size_t n, int level, u32 flags, void* stream) {
    BatchOrder order(cur_state(), stream);
    return compress_chunked_ordered(d_src, d_src_off, d_dst, d_dst_off, d_result, n, level, flags, stream);
}
size_t zjni_compress_batch_device(const void* d_src, const uint64_t* d_src_off, void* d_dst, const uint64_t* d_dst_off,
                                  uint64_t* d_result, size_t n, int level, void* stream) {
    if (level == 0) level = 3;                    // ZSTD_CLEVEL_DEFAULT, as ZSTD_c_compressionLevel = 0 means
    if (!zj_level_served(level)) return ZJNI_ERR(42);
    return compress_chunked(d_src, d_src_off, d_dst, d_dst_off, d_result, n, level, 0u, stream);
}
size_t zjni_compress_batch_device2(const void* d_src, const uint64_t* d_src_off, void* d_dst, const uint64_t* d_dst_off,
                                   uint64_t* d_result, size_t n, int level, int checksum, void* stream) {
    if (level == 0) level = 3;                    // ZSTD_CLEVEL_DEFAULT, as ZSTD_c_compressionLevel = 0 means
    if (!zj_level_served(level)) return ZJNI_ERR(42);
    return compress_chunked(d_src, d_src_off, d_dst, d_dst_off, d_result, n, level, checksum ? ZE_FLAG_CHECKSUM : 0u, stream);
}
// Test entry (include/zjni_amd.h, "introspection for tests/bench"): zj_encode_kernel in mode 0 on records the CALLER wrote, so that tests reach the wave64 code of the
// entropy stage with quantities no match finder emits on request.  Host code only: the frame slots ([records][literal offsets], as the match kernels leave them) are
// laid out on the host and copied into a buffer of this call's own; one launch for the frames to 64 KiB (the common stride), one for the wider ones, as the product's
// two entropy launches.  Synchronous, and nothing of it stays allocated.
size_t zjni_test_compress_records_batch_device(const void* d_src, const uint64_t* d_src_off, const uint32_t* h_rec, const uint64_t* h_rec_off, const uint32_t* h_meta,
                                               void* d_dst, const uint64_t* d_dst_off, uint64_t* d_result, size_t n, int level, int checksum, int stagedLds, int grid, void* stream) {
    DevState* d = cur_state();
    if (!d) return ZJNI_ERR(ZJNI_ERROR_no_device);
    if (level < 1 || level > ZJ_LEVEL_MAX || !h_rec_off || !h_meta || (!h_rec && n && h_rec_off[n])) return ZJNI_ERR(42);
    if (n == 0) return 0;
    if (n > 65536) return ZJNI_ERR(72);
    hipStream_t st = (hipStream_t)stream;
    std::vector<u64> so(n + 1);
    if (hipMemcpyAsync(so.data(), d_src_off, (n + 1) * 8, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) return ZJNI_ERR(ZJNI_ERROR_no_device);
    std::vector<u32> lists[2];                                   // [0] frames to 64 KiB, [1] wider ones
    u32 const maxSrcOf[2] = { 65536u, (u32)ZE_WIDE_MAX_SRC };
    for (size_t i = 0; i < n; i++) {
        u64 const size = so[i + 1] - so[i]; u32 const w = size > 65536u ? 1u : 0u;
        u64 const nb = h_rec_off[i + 1] - h_rec_off[i];
        if (so[i + 1] < so[i] || size > ZE_BLOCK_MAX || h_rec_off[i + 1] < h_rec_off[i] || nb != h_meta[3 * i] || nb > ZE_FRAME_MAXSEQ(maxSrcOf[w])) return ZJNI_ERR(42);
        // the kernel trusts its records (a match finder wrote them): nothing that reads or writes outside the frame may reach it
        u64 lit = 0, at = 0;
        for (u64 q = 0; q < nb; q++) {
            const u32* const s = h_rec + 4 * (h_rec_off[i] + q);                       // ll, ml, offBase, pos
            if (s[3] != at || s[1] < 3u || s[2] < 1u || (u64)s[3] + s[0] + s[1] > size) return ZJNI_ERR(42);
            lit += s[0]; at += (u64)s[0] + s[1];
        }
        if (at + h_meta[3 * i + 2] != size || lit + h_meta[3 * i + 2] != h_meta[3 * i + 1]) return ZJNI_ERR(42);
        lists[w].push_back((u32)i);
    }
    size_t off[2][3], total = 64;                                // per list: frame slots, meta, list; 64 bytes of counters in front ([0] |A|, [1] |B|, [2] work A, [3] work B)
    for (int w = 0; w < 2; w++) {
        size_t const m = lists[w].size();
        off[w][0] = total; total += m * (size_t)ZE_FRAME_STRIDE(maxSrcOf[w]);
        off[w][1] = total; total += (m * 12 + 63) & ~(size_t)63;
        off[w][2] = total; total += (m * 4 + 63) & ~(size_t)63;
    }
    std::vector<u8> image(total, (u8)0xC3);                       // (what no record covers is poisoned, as a slot a previous call used would be)
    {   u32* const c = (u32*)image.data(); memset(c, 0, 64); c[0] = (u32)lists[0].size(); c[1] = (u32)lists[1].size(); }
    for (int w = 0; w < 2; w++) {
        for (size_t k = 0; k < lists[w].size(); k++) {
            u32 const i = lists[w][k]; u32 const nb = h_meta[3 * (size_t)i];
            u8* const fs = image.data() + off[w][0] + k * (size_t)ZE_FRAME_STRIDE(maxSrcOf[w]);
            memcpy(fs, h_rec + 4 * h_rec_off[i], (size_t)nb * 16);
            u32* const litOff = (u32*)(fs + (size_t)ZE_FRAME_MAXSEQ(maxSrcOf[w]) * 16u); u32 lit = 0;
            for (u32 q = 0; q < nb; q++) { litOff[q] = lit; lit += h_rec[4 * (h_rec_off[i] + q)]; }
            memcpy(image.data() + off[w][1] + k * 12, h_meta + 3 * (size_t)i, 12);
            ((u32*)(image.data() + off[w][2]))[k] = i;
        }
    }
    BatchOrder order(d, stream);
    u8* buf = nullptr;
    if (hipMalloc(&buf, total) != hipSuccess) { (void)hipGetLastError(); return ZJNI_ERR(64); }
    size_t r = 0;
    if (hipMemcpyAsync(buf, image.data(), total, hipMemcpyHostToDevice, st) != hipSuccess) r = ZJNI_ERR(ZJNI_ERROR_no_device);
    u32 const levelWord = (u32)zj_level3_word(level), flags = checksum ? ZE_FLAG_CHECKSUM : 0u;
    // the dynamic LDS of the product's entropy launches: the stage alone (no dictionary: nothing is staged), or with room for a frame of ZE_SMALL_MAX bytes (the dictionary pipeline's launch)
    u32 const ldsRun = stagedLds ? (u32)ZE_SMALL_LDS_BYTES : (u32)sizeof(ZEEntropy);
    size_t gridMax = (size_t)(stagedLds ? d->encGridSmall : d->encGridLvl[1]);
    if (gridMax > (size_t)d->encGrid) gridMax = (size_t)d->encGrid;                 // a scratch slot per workgroup
    if (grid > 0 && (size_t)grid < gridMax) gridMax = (size_t)grid;
    for (int w = 0; w < 2 && r == 0; w++) {
        size_t const m = lists[w].size();
        if (!m) continue;
        u32* const ctr = (u32*)buf;
        hipLaunchKernelGGL(zj_encode_kernel, dim3((u32)(m < gridMax ? m : gridMax)), dim3(64), ldsRun, st, (const u8*)d_src, (const u64*)d_src_off, (u8*)d_dst,
                           (const u64*)d_dst_off, (u64*)d_result, levelWord, (const u32*)(buf + off[w][2]), (const u32*)(ctr + w), ctr + 2 + w, d->encScratch, (unsigned long long*)nullptr,
                           buf + off[w][0], maxSrcOf[w], (const u32*)(buf + off[w][1]), 0u, (const u32*)nullptr, (u32*)nullptr, flags, (const ZECDictDev*)nullptr, ldsRun, 0u, 0xFFFFFFFFu);
        if (hipGetLastError() != hipSuccess) r = ZJNI_ERR(ZJNI_ERROR_no_device);
    }
    if (hipStreamSynchronize(st) != hipSuccess && r == 0) r = ZJNI_ERR(ZJNI_ERROR_no_device);
    (void)hipFree(buf);
    return r;
}
// Stream frames (include/zjni_amd.h): n streams, each buffered whole, through zj_encode_stream_kernel.
size_t zjni_compress_stream_batch_device(const void* d_src, const uint64_t* d_src_off, void* d_dst, const uint64_t* d_dst_off, uint64_t* d_result, size_t n, int level, int checksum,
                                         const uint32_t* d_flush_at, const uint64_t* d_flush_off, const uint32_t* d_mode, void* stream) {
    if (level == 0) level = 3;
    if (level > 3) return ZJNI_ERR(42);                              // the levels whose multi-block frames the kernels make (above: the bundled library's)
    level = zj_negative_word(level);                                 // negative levels: row 0 of the unknown-size table, step N + 1, raw literals (ze_compress_stream)
    DevState* d = cur_state();
    if (!d) return ZJNI_ERR(ZJNI_ERROR_no_device);
    if (n == 0) return 0;
    if (n > 0xFFFFFFFFull) return ZJNI_ERR(72);
    BatchOrder order(d, stream);
    hipStream_t st = (hipStream_t)stream;
    if (!ensure_multi_tables(d)) return ZJNI_ERR(64);
    u32* const ctr = d->counters + 224;
    if (hipMemsetAsync(ctr, 0, 4, st) != hipSuccess) return ZJNI_ERR(ZJNI_ERROR_no_device);
    u32 const gc = (u32)(n < (size_t)d->multiGrid ? n : (size_t)d->multiGrid);
    u32 flags = checksum ? ZE_FLAG_CHECKSUM : 0u;
    if (const char* ov = zj_tune("ZJNI_MULTI_WAVE")) { int const v = atoi(ov); flags |= v == 0 ? ZE_FLAG_MULTI_SERIAL : (v == 2 ? ZE_FLAG_MULTI_NOCARRY : 0u); }
    {   const char* const ov = zj_tune("ZJNI_MULTI_WAVE_FAST"); if (!(ov && atoi(ov) == 1)) flags |= ZE_FLAG_MULTI_FAST_SERIAL; }      // levels 1-2: the one-lane parse (zj_encode_multi_kernel's default)
    hipLaunchKernelGGL(zj_encode_stream_kernel, dim3(gc), dim3(64), (u32)sizeof(ZEEntropy), st, (const u8*)d_src, (const u64*)d_src_off, (u8*)d_dst, (const u64*)d_dst_off,
                       (u64*)d_result, (u32)level, (u32)n, ctr, d->encScratch, d->multiTables, flags, (u32)sizeof(ZEEntropy), (const u32*)d_flush_at, (const u64*)d_flush_off, (const u32*)d_mode);
    return hipGetLastError() == hipSuccess ? 0 : ZJNI_ERR(ZJNI_ERROR_no_device);
}
// One stream from host pointers: what was written so far, where the caller flushed, closing or not.  Returns the bytes the frame has so far (final = 0: up to the
// last flush), or an error; 201 when the total exceeds the level's unknown-size window (the bundled library's stream takes over).
size_t zjni_compress_stream(void* dst, size_t dstCap, const void* src, size_t srcSize, int level, int checksum, const uint32_t* flushAt, size_t nFlush, int final_, int knownEmpty) {
    if (level == 0) level = 3;
    if (level > 3) return ZJNI_ERR(42);
    if (srcSize > ((size_t)1 << ze_stream_window_log(level < 0 ? 1u : (u32)level)) || srcSize > ZE_MULTI_MAX) return ZJNI_ERR(201);     // (negative levels: level 1's 512 KiB window)
    if ((srcSize && !src) || (dstCap && !dst) || (nFlush && !flushAt) || nFlush > (1u << 20)) return ZJNI_ERR(72);
    DevState* d = cur_state();
    if (!d) return ZJNI_ERR(ZJNI_ERROR_no_device);
    size_t const cap = dstCap > ((size_t)1 << 31) ? ((size_t)1 << 31) : dstCap;
    // staging layout: [srcOff 2][dstOff 2][result 1][flushOff 2][mode (4 bytes, padded to 8)][flush positions][src][dst]
    size_t const oSrcOff = 0, oDstOff = 16, oRes = 32, oFOff = 40, oMode = 56, oFlush = 64, oSrc = (oFlush + 4 * nFlush + 15) & ~(size_t)15, oDst = (oSrc + srcSize + 15) & ~(size_t)15;
    size_t const total = oDst + cap + 16;
    SlotLock slotLock(d); StageSlot* const sl = slotLock.s;
    if (!ensure_staging(sl, total)) return ZJNI_ERR(ZJNI_ERROR_unsupported);
    hipStream_t const hst = sl->hostK;
    struct Drain { hipStream_t st; ~Drain() { (void)hipStreamSynchronize(st); } } drainOnExit{hst};
    u64* const h = (u64*)sl->hPinned;
    h[0] = 0; h[1] = srcSize; h[2] = 0; h[3] = cap; h[4] = 0; h[5] = 0; h[6] = nFlush; ((u32*)(sl->hPinned + oMode))[0] = (final_ ? 1u : 0u) | (knownEmpty ? 2u : 0u); ((u32*)(sl->hPinned + oMode))[1] = 0;
    if (nFlush) memcpy(sl->hPinned + oFlush, flushAt, 4 * nFlush);
    if (srcSize) memcpy(sl->hPinned + oSrc, src, srcSize);
    if (hipMemcpyAsync(sl->dStage, sl->hPinned, oSrc + srcSize, hipMemcpyHostToDevice, hst) != hipSuccess) return ZJNI_ERR(ZJNI_ERROR_no_device);
    size_t const r = zjni_compress_stream_batch_device(sl->dStage + oSrc, (const u64*)(sl->dStage + oSrcOff), sl->dStage + oDst, (const u64*)(sl->dStage + oDstOff), (u64*)(sl->dStage + oRes), 1, level, checksum,
                                                       (const u32*)(sl->dStage + oFlush), (const u64*)(sl->dStage + oFOff), (const u32*)(sl->dStage + oMode), hst);
    if (zjni_isError(r)) return r;
    if (hipMemcpyAsync(sl->hPinned + oRes, sl->dStage + oRes, 8, hipMemcpyDeviceToHost, hst) != hipSuccess || hipStreamSynchronize(hst) != hipSuccess) return ZJNI_ERR(ZJNI_ERROR_no_device);
    size_t const out = (size_t)h[4];
    if (zjni_isError(out) || out == 0) return out;
    if (out > cap) return ZJNI_ERR(70);
    if (hipMemcpyAsync(sl->hPinned + oDst, sl->dStage + oDst, out, hipMemcpyDeviceToHost, hst) != hipSuccess || hipStreamSynchronize(hst) != hipSuccess) return ZJNI_ERR(ZJNI_ERROR_no_device);
    memcpy(dst, sl->hPinned + oDst, out);
    return out;
}
// ---- stream frames continued from device state (include/zjni_amd.h; ze_compress_stream_resume) ----
size_t zjni_cstream_state_bytes(int level) {
    if (level == 0) level = 3;
    return level > 3 ? 0 : (size_t)ze_stream_state_bytes((u32)zj_negative_word(level));
}
size_t zjni_compress_stream_continue_batch_device(const void* d_src, const uint64_t* d_src_off, void* d_dst, const uint64_t* d_dst_off, uint64_t* d_result, size_t n, int level, int checksum,
                                                  const uint32_t* d_flush_at, const uint64_t* d_flush_off, const uint32_t* d_mode, void* d_state, void* stream) {
    if (level == 0) level = 3;
    if (level > 3) return ZJNI_ERR(42);
    level = zj_negative_word(level);
    DevState* d = cur_state();
    if (!d) return ZJNI_ERR(ZJNI_ERROR_no_device);
    if (n == 0) return 0;
    if (n > 0xFFFFFFFFull || !d_state) return ZJNI_ERR(72);
    BatchOrder order(d, stream);
    hipStream_t st = (hipStream_t)stream;
    if (!d->contGrid) {                                               // resident workgroups: as zj_encode_stream_kernel's, a scratch slot each
        int perCU = 8, fit = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&fit, zj_encode_stream_continue_kernel, 64, sizeof(ZEEntropy)) == hipSuccess && fit >= 1 && fit < perCU) perCU = fit;
        d->contGrid = d->numCU * perCU; if (d->contGrid > d->encGrid) d->contGrid = d->encGrid;
    }
    u32* const ctr = d->counters + 226;
    if (hipMemsetAsync(ctr, 0, 4, st) != hipSuccess) return ZJNI_ERR(ZJNI_ERROR_no_device);
    u32 const gc = (u32)(n < (size_t)d->contGrid ? n : (size_t)d->contGrid);
    u32 flags = checksum ? ZE_FLAG_CHECKSUM : 0u;                     // the block parses: zjni_compress_stream_batch_device's choices
    if (const char* ov = zj_tune("ZJNI_MULTI_WAVE")) { int const v = atoi(ov); flags |= v == 0 ? ZE_FLAG_MULTI_SERIAL : (v == 2 ? ZE_FLAG_MULTI_NOCARRY : 0u); }
    {   const char* const ov = zj_tune("ZJNI_MULTI_WAVE_FAST"); if (!(ov && atoi(ov) == 1)) flags |= ZE_FLAG_MULTI_FAST_SERIAL; }
    hipLaunchKernelGGL(zj_encode_stream_continue_kernel, dim3(gc), dim3(64), (u32)sizeof(ZEEntropy), st, (const u8*)d_src, (const u64*)d_src_off, (u8*)d_dst, (const u64*)d_dst_off,
                       (u64*)d_result, (u32)level, (u32)n, ctr, d->encScratch, (u8*)d_state, (u64)ze_stream_state_bytes((u32)level), flags, (u32)sizeof(ZEEntropy),
                       (const u32*)d_flush_at, (const u64*)d_flush_off, (const u32*)d_mode);
    return hipGetLastError() == hipSuccess ? 0 : ZJNI_ERR(ZJNI_ERROR_no_device);
}
// The host form: one stream's handle.  Device: [meta slots][state][source so far, up to the window][new frame bytes]; pinned: [meta slots][source so far][new frame bytes].
// A meta slot serves one launch: [srcOff 2][dstOff 2][result 1][flushOff 2][mode, pad][flush position, pad] (u64 words 0-8 of its 128 bytes).
// A plain handle waits for every launch in the call that makes it and uses slot 0 only.  An eager handle (ZJNI_CSTREAM_EAGER) launches the full 128 KiB pieces from
// ZSTD_e_continue calls without waiting: launch k of a span between two waits has slot k and its own part of the frame-byte area, which comes back to the pinned
// area behind the kernel, so a later call finds its bytes there once the handle's stream is idle.
#define ZJ_CS_SLOTS 32u                        /* more than a window holds pieces (16 at level 3), and every launch consumes at least one */
#define ZJ_CS_SLOT_BYTES 128u
#define ZJ_CS_META (ZJ_CS_SLOTS * ZJ_CS_SLOT_BYTES)
struct zjni_cstream {
    int ordinal, level, checksum, eager;
    size_t window, outCap, stateBytes;
    u8* dBuf; u8* hPinned; hipStream_t st;
    size_t flushed, pending;                   // source bytes on the device (the state has consumed them, or a launch in flight will), bytes buffered in hPinned behind them
    bool touched, closed; size_t dead;         // dead: the code every call answers until the handle is reset
    // eager: the launches whose frame bytes are not handed out yet, oldest first; part k has slot k
    struct Part { size_t off, cap, size, given; } parts[ZJ_CS_SLOTS];
    u32 nParts, firstPart, inFlight;           // inFlight: the newest parts, whose sizes have not been read yet
    size_t outCursor;                          // the frame-byte area behind the newest part
};
static inline size_t zj_cstream_bound(size_t fresh, size_t flushes) { return fresh + (fresh >> 8) + 4096 + 64 * (flushes + 4); }
zjni_cstream* zjni_createCStream2(int level, int checksum, int flags) {
    DevState* d = cur_state();
    if (level == 0) level = 3;
    if (!d || level > 3 || (flags & ~ZJNI_CSTREAM_EAGER)) return nullptr;
    zjni_cstream* cs = new zjni_cstream();
    cs->ordinal = d->ordinal; cs->level = level; cs->checksum = checksum ? 1 : 0; cs->eager = (flags & ZJNI_CSTREAM_EAGER) ? 1 : 0;
    cs->window = (size_t)1 << ze_stream_window_log(level < 0 ? 1u : (u32)level);
    cs->outCap = zj_cstream_bound(cs->window, 1) + (cs->eager ? ZJ_CS_SLOTS * zj_cstream_bound(0, 1) : 0);      // (every launch's part is a bound of its own)
    cs->stateBytes = zjni_cstream_state_bytes(level);
    cs->dBuf = nullptr; cs->hPinned = nullptr; cs->st = nullptr;
    if (hipMalloc(&cs->dBuf, ZJ_CS_META + cs->stateBytes + cs->window + cs->outCap) != hipSuccess || hipHostMalloc(&cs->hPinned, ZJ_CS_META + cs->window + cs->outCap, hipHostMallocDefault) != hipSuccess
        || hipStreamCreateWithFlags(&cs->st, hipStreamNonBlocking) != hipSuccess || zjni_isError(zjni_cstream_reset(cs))) { (void)hipGetLastError(); (void)zjni_freeCStream(cs); return nullptr; }
    return cs;
}
zjni_cstream* zjni_createCStream(int level, int checksum) { return zjni_createCStream2(level, checksum, 0); }
size_t zjni_freeCStream(zjni_cstream* cs) {
    if (!cs) return 0;
    (void)hipSetDevice(cs->ordinal);
    if (cs->st) { (void)hipStreamSynchronize(cs->st); (void)hipStreamDestroy(cs->st); }       // (waits for the pieces in flight)
    if (cs->dBuf) (void)hipFree(cs->dBuf);
    if (cs->hPinned) (void)hipHostFree(cs->hPinned);
    if (t_dev >= 0) (void)hipSetDevice(t_dev);
    delete cs;
    return 0;
}
size_t zjni_cstream_reset(zjni_cstream* cs) {
    if (!cs) return ZJNI_ERR(72);
    if (cs->ordinal != t_dev && t_dev >= 0) return ZJNI_ERR(32);
    cs->flushed = 0; cs->pending = 0; cs->touched = false; cs->closed = false; cs->dead = 0;
    cs->nParts = 0; cs->firstPart = 0; cs->inFlight = 0; cs->outCursor = 0;                 // (the memset below runs behind the pieces in flight; their bytes are dropped)
    if (hipMemsetAsync(cs->dBuf + ZJ_CS_META, 0, cs->stateBytes, cs->st) != hipSuccess || hipStreamSynchronize(cs->st) != hipSuccess) return cs->dead = ZJNI_ERR(ZJNI_ERROR_no_device);
    return 0;
}
// the handle is dead from here on: nothing stays in flight, nothing stays held
static size_t zj_cstream_kill(zjni_cstream* cs, size_t code) {
    (void)hipStreamSynchronize(cs->st);
    cs->nParts = 0; cs->firstPart = 0; cs->inFlight = 0; cs->outCursor = 0;
    return cs->dead = code;
}
// Enqueue one call of the device form on the handle's stream and do not wait: the `fresh` bytes behind cs->flushed go up, meta slot `slot` describes the call, the new
// frame bytes go to [outOff, outOff + outCap) of the frame-byte area and the result to the slot's word 4 on the device.  0 or an error code.
static size_t zj_cstream_launch(zjni_cstream* cs, u32 slot, size_t fresh, u32 mode, bool flushHere, size_t outOff, size_t outCap) {
    size_t const total = cs->flushed + fresh;
    size_t const oState = ZJ_CS_META, oSrc = oState + cs->stateBytes, oDst = oSrc + cs->window;
    u64* const h = (u64*)(cs->hPinned + (size_t)slot * ZJ_CS_SLOT_BYTES);
    h[0] = 0; h[1] = total; h[2] = 0; h[3] = outCap; h[4] = 0; h[5] = 0; h[6] = flushHere ? 1 : 0;
    ((u32*)(h + 7))[0] = mode; ((u32*)(h + 7))[1] = 0; ((u32*)(h + 8))[0] = (u32)total; ((u32*)(h + 8))[1] = 0;
    u8* const dv = cs->dBuf; u8* const ds = dv + (size_t)slot * ZJ_CS_SLOT_BYTES;
    if (hipMemcpyAsync(ds, h, 72, hipMemcpyHostToDevice, cs->st) != hipSuccess) return ZJNI_ERR(ZJNI_ERROR_no_device);
    if (fresh && hipMemcpyAsync(dv + oSrc + cs->flushed, cs->hPinned + ZJ_CS_META + cs->flushed, fresh, hipMemcpyHostToDevice, cs->st) != hipSuccess) return ZJNI_ERR(ZJNI_ERROR_no_device);
    return zjni_compress_stream_continue_batch_device(dv + oSrc, (const u64*)ds, dv + oDst + outOff, (const u64*)(ds + 16), (u64*)(ds + 32), 1, cs->level, cs->checksum,
                                                      (const u32*)(ds + 64), (const u64*)(ds + 40), (const u32*)(ds + 56), dv + oState, cs->st);
}
// eager: wait for the pieces in flight and read their sizes.  0, or the code the handle is dead with.
static size_t zj_cstream_collect(zjni_cstream* cs) {
    if (!cs->inFlight) return 0;
    if (hipStreamSynchronize(cs->st) != hipSuccess) return zj_cstream_kill(cs, ZJNI_ERR(ZJNI_ERROR_no_device));
    for (u32 k = cs->nParts - cs->inFlight; k < cs->nParts; k++) {
        size_t const out = (size_t)((const u64*)(cs->hPinned + (size_t)k * ZJ_CS_SLOT_BYTES))[4];
        if (zjni_isError(out)) return zj_cstream_kill(cs, out);
        if (out > cs->parts[k].cap) return zj_cstream_kill(cs, ZJNI_ERR(70));
        cs->parts[k].size = out;
    }
    cs->inFlight = 0;
    return 0;
}
// eager: frame bytes of parts [firstPart, upTo) that have not been handed out (all of them collected)
static size_t zj_cstream_held(const zjni_cstream* cs, u32 upTo) {
    size_t held = 0;
    for (u32 k = cs->firstPart; k < upTo; k++) held += cs->parts[k].size - cs->parts[k].given;
    return held;
}
// eager: hand out what parts [firstPart, upTo) hold, oldest first, as far as dstCap allows; the rest stays held
static size_t zj_cstream_hand_out(zjni_cstream* cs, u8* dst, size_t dstCap, u32 upTo) {
    size_t at = 0;
    u8 const* const hOut = cs->hPinned + ZJ_CS_META + cs->window;
    while (cs->firstPart < upTo) {
        zjni_cstream::Part& p = cs->parts[cs->firstPart];
        size_t const n = p.size - p.given < dstCap - at ? p.size - p.given : dstCap - at;
        if (n) memcpy(dst + at, hOut + p.off + p.given, n);
        p.given += n; at += n;
        if (p.given < p.size) break;
        cs->firstPart++;
    }
    if (cs->firstPart == cs->nParts) { cs->nParts = 0; cs->firstPart = 0; cs->outCursor = 0; }       // nothing held, nothing in flight: the slots and the area start again
    return at;
}
size_t zjni_cstream_pending(const zjni_cstream* cs) {
    if (!cs || !cs->eager || cs->dead) return 0;
    if (cs->inFlight && hipStreamSynchronize(cs->st) != hipSuccess) return 0;
    size_t held = zj_cstream_held(cs, cs->nParts - cs->inFlight);
    for (u32 k = cs->nParts - cs->inFlight; k < cs->nParts; k++) {
        size_t const out = (size_t)((const u64*)(cs->hPinned + (size_t)k * ZJ_CS_SLOT_BYTES))[4];
        if (!zjni_isError(out)) held += out;
    }
    return held;
}
size_t zjni_cstream_compress(zjni_cstream* cs, void* dst, size_t dstCap, const void* src, size_t srcSize, int directive) {
    if (!cs || (srcSize && !src) || (dstCap && !dst)) return ZJNI_ERR(72);
    if (directive < 0 || directive > 2) return ZJNI_ERR(42);
    if (cs->ordinal != t_dev && t_dev >= 0) return ZJNI_ERR(32);                          // made on another device
    if (cs->dead) return cs->dead;
    if (cs->closed) return cs->dead = ZJNI_ERR(60);
    if (srcSize > cs->window || cs->flushed + cs->pending + srcSize > cs->window) return zj_cstream_kill(cs, ZJNI_ERR(201));      // beyond the window: the caller's CPU path replays the stream from byte 0, so what is held is dropped
    if (zjni_isError(zj_cstream_collect(cs))) return cs->dead;                              // eager: the work of earlier calls
    size_t const held = zj_cstream_held(cs, cs->nParts);
    if (directive != 0 && dstCap < held + zj_cstream_bound(cs->pending + srcSize, 1)) return ZJNI_ERR(70);              // (nothing was touched: the call may be made again with more room)
    bool const knownEmpty = directive == 2 && !cs->touched && srcSize == 0;
    cs->touched = true;
    if (srcSize) memcpy(cs->hPinned + ZJ_CS_META + cs->flushed + cs->pending, src, srcSize);
    cs->pending += srcSize;
    u8* const dv = cs->dBuf;
    size_t const oDst = ZJ_CS_META + cs->stateBytes + cs->window;
    u8* const hOut = cs->hPinned + ZJ_CS_META + cs->window;
    if (directive == 0) {
        if (!cs->eager) return 0;                                                           // buffered until a flush
        u32 const earlier = cs->nParts;
        size_t const full = cs->pending & ~(size_t)131071;                                  // cs->flushed stands on a piece boundary: the pieces these bytes complete go out now
        if (full) {
            size_t const cap = zj_cstream_bound(full, 1);
            if (cs->nParts == ZJ_CS_SLOTS || cs->outCursor + cap > cs->outCap) return zj_cstream_kill(cs, ZJNI_ERR(1));
            u32 const k = cs->nParts;
            u8* const ds = dv + (size_t)k * ZJ_CS_SLOT_BYTES;
            size_t const r = zj_cstream_launch(cs, k, full, 4u, false, cs->outCursor, cap);
            if (zjni_isError(r)) return zj_cstream_kill(cs, r);
            if (hipMemcpyAsync(cs->hPinned + (size_t)k * ZJ_CS_SLOT_BYTES + 32, ds + 32, 8, hipMemcpyDeviceToHost, cs->st) != hipSuccess
                || hipMemcpyAsync(hOut + cs->outCursor, dv + oDst + cs->outCursor, cap, hipMemcpyDeviceToHost, cs->st) != hipSuccess) return zj_cstream_kill(cs, ZJNI_ERR(ZJNI_ERROR_no_device));
            cs->parts[k].off = cs->outCursor; cs->parts[k].cap = cap; cs->parts[k].size = 0; cs->parts[k].given = 0;
            cs->nParts++; cs->inFlight = 1; cs->outCursor += cap;
            cs->flushed += full; cs->pending -= full;
        }
        return zj_cstream_hand_out(cs, (u8*)dst, dstCap, earlier);                          // the frame bytes of earlier calls' pieces; this call's piece is on its way
    }
    size_t const given = zj_cstream_hand_out(cs, (u8*)dst, dstCap, cs->nParts);              // eager: everything held goes first (there is room for it)
    size_t const total = cs->flushed + cs->pending;
    u64* const h = (u64*)cs->hPinned;
    auto fail = [&](size_t code) { (void)hipStreamSynchronize(cs->st); return cs->dead = code; };
    size_t const r = zj_cstream_launch(cs, 0, cs->pending, (directive == 2 ? 1u : 0u) | (knownEmpty ? 2u : 0u), directive == 1, 0, cs->outCap);
    if (zjni_isError(r)) return fail(r);
    if (hipMemcpyAsync(h + 4, dv + 32, 8, hipMemcpyDeviceToHost, cs->st) != hipSuccess || hipStreamSynchronize(cs->st) != hipSuccess) return fail(ZJNI_ERR(ZJNI_ERROR_no_device));
    size_t const out = (size_t)h[4];
    if (zjni_isError(out)) return cs->dead = out;
    if (out > dstCap - given || out > cs->outCap) return cs->dead = ZJNI_ERR(70);
    if (out && (hipMemcpyAsync(hOut, dv + oDst, out, hipMemcpyDeviceToHost, cs->st) != hipSuccess || hipStreamSynchronize(cs->st) != hipSuccess)) return fail(ZJNI_ERR(ZJNI_ERROR_no_device));
    if (out) memcpy((u8*)dst + given, hOut, out);
    cs->flushed = total; cs->pending = 0; cs->closed = directive == 2;
    return given + out;
}
// ZstdCompressCtx.setHashLog / setChainLog (ZSTD_c_hashLog / ZSTD_c_chainLog; 0 = the library's choice) on top of level + checksum.
// Honoured for level 3 (double-fast), hashLog 6..17, chainLog 6..16: with 16 / 15 the frames are the reference's plain level 3.
static size_t level_word(int level, int hashLog, int chainLog, int* out) {
    *out = level;
    if (!hashLog && !chainLog) return 0;
    if (level != 3) return ZJNI_ERR(40);
    if ((hashLog && (hashLog < 6 || hashLog > (int)ZE_HASHLOG_CAP)) || (chainLog && (chainLog < 6 || chainLog > (int)ZE_CHAINLOG_CAP))) return ZJNI_ERR(42);
    *out = (int)ZE_LW(level, hashLog, chainLog);
    return 0;
}
size_t zjni_compress_batch_device_advanced(const void* d_src, const uint64_t* d_src_off, void* d_dst, const uint64_t* d_dst_off,
                                           uint64_t* d_result, size_t n, int level, int checksum, int hashLog, int chainLog, void* stream) {
    if (level == 0) level = 3;
    int lw; size_t const e = level_word(level, hashLog, chainLog, &lw);
    if (e) return e;
    return compress_chunked(d_src, d_src_off, d_dst, d_dst_off, d_result, n, lw, zj_frame_flags(checksum), stream);
}

// ZSTD_createCDict (N/compress/zstd_compress.c:5710-5719; ZstdDictCompress.init, N/jni_fast_zstd.c:18-52): the raw dictionary
// goes to HBM once, behind its (zeroed) tagged tables, and one workgroup digests it there.  NULL when the device, the level
// or the dictionary is bad.
zjni_cdict* zjni_createCDict(const void* dict, size_t dictSize, int level) {
    DevState* d = cur_state();
    if (level == 0) level = 3;                        // ZSTD_createCDict: 0 = ZSTD_CLEVEL_DEFAULT
    if (!d || !dict || dictSize < 8 || dictSize > 0x3FFFFFFFull || level > 3) return nullptr;
    level = zj_negative_word(level);                  // negative levels (zstd's --fast=N, clamped at ZSTD_minCLevel()): the CDict keeps their word, N included
    bool const neg = ((u32)level & ZE_LW_NEG) != 0u;
    ZEParams const cp = ze_cdict_params_of((u32)level, (u32)dictSize);
    size_t const head = (sizeof(ZECDictDev) + 15) & ~(size_t)15, tablesBytes = (size_t)ze_cdict_table_entries(cp) * 4u;
    zjni_cdict* cd = new zjni_cdict{t_dev, nullptr, 0, level, cp.strategy};
    if (hipMalloc(&cd->buf, head + tablesBytes + dictSize + 16) != hipSuccess) { delete cd; return nullptr; }
    ZECDictDev hd; memset(&hd, 0, sizeof(hd));
    hd.tablesOff = (u32)head; hd.rawOff = (u32)(head + tablesBytes);
    bool ok = hipMemset(cd->buf, 0, head + tablesBytes) == hipSuccess
           && hipMemcpy(cd->buf, &hd, sizeof(hd), hipMemcpyHostToDevice) == hipSuccess
           && hipMemcpy(cd->buf + hd.rawOff, dict, dictSize, hipMemcpyHostToDevice) == hipSuccess;
    if (ok) {
        hipLaunchKernelGGL(neg ? zj_cdict_digest_kernel_neg : zj_cdict_digest_kernel, dim3(1), dim3(64), 0, 0, (u32)dictSize, (u32)level, (ZECDictDev*)cd->buf);
        ok = hipMemcpy(&hd, cd->buf, 64, hipMemcpyDeviceToHost) == hipSuccess && hd.status == 0;
    }
    if (!ok) { (void)hipFree(cd->buf); delete cd; return nullptr; }
    cd->dictID = hd.dictID;
    return cd;
}
size_t zjni_freeCDict(zjni_cdict* cd) {
    if (!cd) return 0;
    (void)hipSetDevice(cd->ordinal);
    (void)hipFree(cd->buf);
    delete cd;
    return 0;
}
unsigned zjni_getDictID_fromCDict(const zjni_cdict* cd) { return cd ? cd->dictID : 0u; }

// ZstdCompressCtx.loadDict(ZstdDictCompress) + compress, batched: lane-per-frame attach-mode search, then the
// wave-per-frame entropy stage starting from the dictionary's tables.
// Slices of 2 x ZJ_CHUNK_FRAMES: memset/classify/clear/match of slice s on the caller's stream, its entropy kernel on the side
// stream — beside slice s+1's match kernel (which leaves most of every CU idle: one wave per SIMD, waiting on memory).
// (the caller holds the device's BatchOrder; n in 1 .. 2^32 - 1, the CDict of this device)
static size_t compress_cdict_ordered(DevState* d, const void* d_src, const uint64_t* d_src_off, void* d_dst, const uint64_t* d_dst_off,
                                     uint64_t* d_result, size_t n, const zjni_cdict* cdict, u32 flags, void* stream);
size_t zjni_compress_batch_device_usingCDict(const void* d_src, const uint64_t* d_src_off, void* d_dst, const uint64_t* d_dst_off,
                                             uint64_t* d_result, size_t n, const zjni_cdict* cdict, int checksum, void* stream) {
    if (!cdict) return ZJNI_ERR(32);
    if (cdict->ordinal != t_dev && t_dev >= 0) return ZJNI_ERR(32);                       // digested on another device
    DevState* d = cur_state();
    if (!d) return ZJNI_ERR(ZJNI_ERROR_no_device);
    if (n == 0) return 0;
    if (n > 0xFFFFFFFFull) return ZJNI_ERR(72);
    BatchOrder order(d, stream);
    return compress_cdict_ordered(d, d_src, d_src_off, d_dst, d_dst_off, d_result, n, cdict, zj_frame_flags(checksum), stream);
}
static size_t compress_cdict_ordered(DevState* d, const void* d_src, const uint64_t* d_src_off, void* d_dst, const uint64_t* d_dst_off,
                                     uint64_t* d_result, size_t n, const zjni_cdict* cdict, u32 flags, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    size_t chunk = 2 * ZJ_CHUNK_FRAMES;            // 2 048 match waves = every SIMD's second wave slot as well: more table requests in flight (measured: +15 % over 65 536)
    chunk = scratch_slice((size_t)ZC_TABLE_STRIDE + 2 * ((size_t)ZE_FRAME_STRIDE(ZC_MAX_SRC) + 12), chunk, 1);
    if (const char* ov = zj_tune("ZJNI_CD_SLICE")) { size_t const v = (size_t)atoll(ov); if (v >= 64) chunk = v; }
    size_t const slice = n < chunk ? n : chunk;
    size_t const fsBytes = slice * (size_t)ZE_FRAME_STRIDE(ZC_MAX_SRC), metaBytes = (slice * 12 + 255) & ~(size_t)255, tablesBytes = slice * (size_t)ZC_TABLE_STRIDE;
    size_t const need = tablesBytes + 2 * (fsBytes + metaBytes) + 256;
    if (d->cdBufCap < need || d->cdSliceCap < slice) {
        if (!scratch_make_room(d, d->cdBufCap, need)) return ZJNI_ERR(64);
        if (d->cdBuf) { if (hipDeviceSynchronize() != hipSuccess) return ZJNI_ERR(ZJNI_ERROR_no_device); (void)hipFree(d->cdBuf); d->cdBuf = nullptr; d->cdBufCap = 0; }
        if (hipMalloc(&d->cdBuf, need) != hipSuccess) return ZJNI_ERR(64);
        d->cdBufCap = need; d->cdSliceCap = slice;
    }
    if (d->cdListCap < slice) {
        if (d->cdList) { if (hipDeviceSynchronize() != hipSuccess) return ZJNI_ERR(ZJNI_ERROR_no_device); (void)hipFree(d->cdList); d->cdList = nullptr; d->cdListCap = 0; }
        if (hipMalloc(&d->cdList, 2 * (slice + 1024) * sizeof(u32)) != hipSuccess) return ZJNI_ERR(64);
        d->cdListCap = slice;
    }
    size_t const sliceCap = d->cdSliceCap;
    size_t const fsB = sliceCap * (size_t)ZE_FRAME_STRIDE(ZC_MAX_SRC), metaB = (sliceCap * 12 + 255) & ~(size_t)255;
    u8* const tables = d->cdBuf;
    const ZECDictDev* const cd = (const ZECDictDev*)cdict->buf;
    bool const neg = ((u32)cdict->level & ZE_LW_NEG) != 0u;     // a negative level: the two searches on their *_neg kernels (the entropy kernel takes the word as it is)
    unsigned long long* const eprof = d->prof ? d->prof + 16 : nullptr;
    int pending[2] = {0, 0};
    auto bail = [&](size_t code) {                       // an error mid-way still orders the caller's stream after the entropy kernels already posted
        for (int p = 0; p < 2; p++) if (pending[p]) (void)hipStreamWaitEvent(st, d->cdEncDone[p], 0);
        return code;
    };
    size_t s = 0;
    for (size_t at = 0; at < n; at += chunk, s++) {
        size_t const m = n - at < chunk ? n - at : chunk;
        int const par = (int)(s & 1);
        u8* const fscratch = d->cdBuf + sliceCap * (size_t)ZC_TABLE_STRIDE + (size_t)par * (fsB + metaB); u32* const meta = (u32*)(fscratch + fsB);
        u32* const list = d->cdList + (size_t)par * (d->cdListCap + 1024);
        u32* const ctr = d->counters + 32 + 8 * par;              // [0] |list|, [1] unused, [2] entropy work, [4] match work
        const u64* const so = (const u64*)d_src_off + at; const u64* const dofs = (const u64*)d_dst_off + at; u64* const res = (u64*)d_result + at;
        if (pending[par]) { if (hipStreamWaitEvent(st, d->cdEncDone[par], 0) != hipSuccess) return bail(ZJNI_ERR(ZJNI_ERROR_no_device)); pending[par] = 0; }   // slice s-2 is done with this set
        if (hipMemsetAsync(ctr, 0, 32, st) != hipSuccess) return bail(ZJNI_ERR(ZJNI_ERROR_no_device));
        hipLaunchKernelGGL(zj_enc_classify_kernel, dim3((u32)((m + 255) / 256)), dim3(256), 0, st, so, res, (u32)m, 1u, 0xFFFFFFFFu, ctr, list, list, (u32*)nullptr);   // every frame <= 128 KiB is listed
        hipLaunchKernelGGL(zj_cdict_zero_tables_kernel, dim3((u32)(m < 16384 ? m : 16384)), dim3(256), 0, st, so, cd, (const u32*)list, (const u32*)ctr, tables);
        u32 const waves = (u32)((m + 63) / 64);
        u32 const gridM = waves < (u32)d->matchGrid ? waves : (u32)d->matchGrid;
        (void)hipEventRecord(d->tev[0], st);
        hipLaunchKernelGGL(neg ? zj_enc_match_dict_kernel_neg : zj_enc_match_dict_kernel, dim3(gridM), dim3(64), 0, st, (const u8*)d_src, so, cd, (const u32*)list, (const u32*)ctr, ctr + 4, tables, fscratch, meta);
        (void)hipEventRecord(d->tev[1], st); d->tevCompress = true;
        if (hipEventRecord(d->cdMatchDone[par], st) != hipSuccess || hipStreamWaitEvent(d->sideStream, d->cdMatchDone[par], 0) != hipSuccess) return bail(ZJNI_ERR(ZJNI_ERROR_no_device));
        u32 const gridA = (u32)(m < (size_t)d->encGridSmall ? m : (size_t)d->encGridSmall);
        hipLaunchKernelGGL(zj_encode_kernel, dim3(gridA), dim3(64), ZE_SMALL_LDS_BYTES, d->sideStream, (const u8*)d_src, so, (u8*)d_dst, dofs, res, (u32)cdict->level,
                           (const u32*)list, (const u32*)ctr, ctr + 2, d->encScratch, eprof, fscratch, ZC_MAX_SRC, (const u32*)meta, 0u, (const u32*)nullptr, (u32*)nullptr, flags, cd,
                           (u32)ZE_SMALL_LDS_BYTES, 0u, 0xFFFFFFFFu);
        if (hipEventRecord(d->cdEncDone[par], d->sideStream) != hipSuccess) return bail(ZJNI_ERR(ZJNI_ERROR_no_device));
        pending[par] = 1;
    }
    for (int par = 0; par < 2; par++) if (pending[par] && hipStreamWaitEvent(st, d->cdEncDone[par], 0) != hipSuccess) return bail(ZJNI_ERR(ZJNI_ERROR_no_device));
    {   // sources beyond the attach range (they got parameter_unsupported above): copy mode, if the call has any
        if (!ensure_multi_tables(d)) return ZJNI_ERR(64);
        u32* const cc = d->counters + 56;            // [0] copy-mode frames of the call, [1] work
        if (hipMemsetAsync(cc, 0, 8, st) != hipSuccess) return ZJNI_ERR(ZJNI_ERROR_no_device);
        hipLaunchKernelGGL(zj_cdict_count_copy_kernel, dim3((u32)((n + 255) / 256)), dim3(256), 0, st, (const u64*)d_src_off, (u32)n, cd, cc);
        u32 const gc = (u32)(n < (size_t)d->multiGrid ? n : (size_t)d->multiGrid);
        hipLaunchKernelGGL(neg ? zj_encode_cdict_copy_kernel_neg : zj_encode_cdict_copy_kernel, dim3(gc), dim3(64), (u32)sizeof(ZEEntropy), st, (const u8*)d_src, (const u64*)d_src_off, (u8*)d_dst, (const u64*)d_dst_off,
                           (u64*)d_result, (u32)n, cd, (const u32*)cc, cc + 1, d->encScratch, d->multiTables, flags, (u32)sizeof(ZEEntropy));
    }
    return hipGetLastError() == hipSuccess ? 0 : ZJNI_ERR(ZJNI_ERROR_no_device);
}

// The first frame of a buffer, read on the host: its compressed size (0 = not a complete plain frame) and its content size (~0 = not in the header).
// Only used to bound the destination staging of the host-pointer decompress entry: a buffer that IS one frame with a known content size needs that
// many bytes, not the caller's whole capacity (a 4 KiB frame decoded into a 64 MiB buffer would otherwise pin and move 64 MiB).  Format: zstd
// compression format 1.5.7, frame header (N/decompress/zstd_decompress.c:447-557) and block headers (ZSTD_getcBlockSize, :1-3 bytes).
static size_t host_frame_extent(const u8* p, size_t n, u64* content) {
    *content = ~(u64)0;
    if (n < 9 || ld32(p) != 0xFD2FB528u) return 0;
    u32 const fhd = p[4], didc = fhd & 3, single = (fhd >> 5) & 1, fcsid = fhd >> 6, cks = (fhd >> 2) & 1;
    if (fhd & 8) return 0;
    u32 const didSz = didc == 3 ? 4 : didc, fcsSz = fcsid == 0 ? single : (1u << fcsid);
    size_t pos = 5 + !single + didSz;
    if (n < pos + fcsSz + 3) return 0;
    if (fcsid == 0) { if (single) *content = p[pos]; } else if (fcsid == 1) *content = (u64)ld16(p + pos) + 256; else if (fcsid == 2) *content = ld32(p + pos); else *content = ld64(p + pos);
    pos += fcsSz;
    for (;;) {
        if (pos + 3 > n) return 0;
        u32 const bh = (u32)p[pos] | ((u32)p[pos + 1] << 8) | ((u32)p[pos + 2] << 16), type = (bh >> 1) & 3, bs = bh >> 3;
        if (type == 3) return 0;
        pos += 3 + (type == 1 ? 1 : bs);
        if (pos > n) return 0;
        if (bh & 1) break;
    }
    pos += cks ? 4 : 0;
    return pos <= n ? pos : 0;
}

// ZSTD_findFrameCompressedSize + ZSTD_decompressBound for ONE complete zstd frame at src (N/decompress/zstd_decompress.c:739-850): the bytes the frame occupies,
// its content size from the header (~0: not recorded) and an upper bound of what it decodes to (raw / RLE blocks exactly, compressed blocks at the block maximum).
// 0: not a complete, well-formed zstd frame (skippable frames, truncated input, reserved bits): the caller keeps the bundled library's stream.
size_t zjni_frame_extent(const void* srcv, size_t srcSize, unsigned long long* content, unsigned long long* bound) {
    const u8* const p = (const u8*)srcv; u64 c = ~(u64)0;
    size_t const ext = srcv ? host_frame_extent(p, srcSize, &c) : 0;
    if (content) *content = c;
    if (bound) *bound = 0;
    if (!ext) return 0;
    u32 const fhd = p[4], didc = fhd & 3, single = (fhd >> 5) & 1, fcsid = fhd >> 6;
    u32 const didSz = didc == 3 ? 4 : didc, fcsSz = fcsid == 0 ? single : (1u << fcsid);
    u64 blockMax = 128u << 10;
    if (!single) { u32 const wl = (p[5] >> 3) + 10u; if (wl > 31u) return 0; u64 const w = ((u64)1 << wl) + (((u64)1 << wl) >> 3) * (p[5] & 7u); if (w < blockMax) blockMax = w; }
    else if (c < blockMax) blockMax = c;
    size_t pos = 5 + !single + didSz + fcsSz; u64 b = 0;
    for (;;) {
        u32 const bh = (u32)p[pos] | ((u32)p[pos + 1] << 8) | ((u32)p[pos + 2] << 16), type = (bh >> 1) & 3, bs = bh >> 3;
        b += type == 2 ? blockMax : bs;
        pos += 3 + (type == 1 ? 1 : bs);
        if (bh & 1) break;
    }
    if (bound) *bound = (c != ~(u64)0) ? c : b;
    return ext;
}

// Host-pointer decompress as a three-stage pipeline over slices of the batch: while slice k's frames are decoded, slice k + 1's sources cross the
// link one way and slice k - 1's output the other (PCIe: 57 GB/s each way alone, 2 x 49 at once on this box: tools/micro/pcie.py), and the host
// threads gather / scatter the slices on either side.  The first slice is small (its transfer and kernels are the pipeline's lead-in), the others
// large enough for the lane-per-frame sequence decode, whose time is its longest frame's chain whatever the slice size.
static size_t host_decompress_locked(DevState* d, StageSlot* sl, const void* const* src, const size_t* srcSize, void* const* dst, const size_t* dstCap, size_t* result, size_t n,
                                     const zjni_ddict* ddict, bool exactCaps);
static size_t host_decompress(DevState* d, const void* const* src, const size_t* srcSize, void* const* dst, const size_t* dstCap, size_t* result, size_t n,
                              const zjni_ddict* ddict) {
    // One host-pointer DECOMPRESS at a time per device: the call is a three-stream pipeline over its own slices already, at the link's and the host threads' limit; a second one
    // beside it only shares both (measured: 41 GiB/s one after the other, 27 with two in flight, profiles/r05/e_).  It still runs beside a compress call's kernels.
    std::lock_guard<std::mutex> oneDecompress(*d->hostDecompMu);
    SlotLock slotLock(d);                         // one of the device's staging slots, for both passes
    size_t const r = host_decompress_locked(d, slotLock.s, src, srcSize, dst, dstCap, result, n, ddict, false);
    if (zjni_isError(r)) return r;
    // A frame that was given its header's content size as capacity and overran it is damaged; the reference, decoding into the caller's larger
    // buffer, goes on to the frame's end and answers from there (usually corruption_detected, not dstSize_tooSmall): those few again, with the caller's capacity
    std::vector<size_t> again;
    for (size_t i = 0; i < n; i++) if (result[i] == ZJNI_ERR(70)) { u64 c; if (srcSize[i] && host_frame_extent((const u8*)src[i], srcSize[i], &c) == srcSize[i] && c != ~(u64)0 && c < dstCap[i]) again.push_back(i); }
    if (again.empty()) return 0;
    size_t const m = again.size();
    std::vector<const void*> s2(m); std::vector<size_t> z2(m), c2(m), r2(m); std::vector<void*> d2(m);
    for (size_t j = 0; j < m; j++) { size_t const i = again[j]; s2[j] = src[i]; z2[j] = srcSize[i]; d2[j] = dst[i]; c2[j] = dstCap[i]; }
    size_t const rr = host_decompress_locked(d, slotLock.s, s2.data(), z2.data(), d2.data(), c2.data(), r2.data(), m, ddict, true);
    if (zjni_isError(rr)) return rr;
    for (size_t j = 0; j < m; j++) result[again[j]] = r2[j];
    return 0;
}
static size_t host_decompress_locked(DevState* d, StageSlot* sl, const void* const* src, const size_t* srcSize, void* const* dst, const size_t* dstCap, size_t* result, size_t n,
                                     const zjni_ddict* ddict, bool exactCaps) {
    size_t const offBytes = (n + 1) * 8;
    // what each buffer needs on the device: the frame's own content size when the buffer is exactly one frame that says it, else the caller's capacity
    std::vector<u64> need(n + 1, 0), srcAt(n + 1, 0);
    {   std::vector<u64> idx(n + 1); for (size_t i = 0; i <= n; i++) idx[i] = i;
        par_ranges(idx.data(), n, [&](size_t a0, size_t a1) {
            for (size_t i = a0; i < a1; i++) {
                u64 c; size_t const ext = srcSize[i] ? host_frame_extent((const u8*)src[i], srcSize[i], &c) : 0;
                need[i] = (!exactCaps && ext == srcSize[i] && c != ~(u64)0 && c <= dstCap[i]) ? c : dstCap[i];
            }
        }); }
    u64 srcTotal = 0, dstTotal = 0;
    for (size_t i = 0; i < n; i++) { u64 const c = need[i]; need[i] = dstTotal; srcAt[i] = srcTotal; dstTotal += c; srcTotal += srcSize[i]; }
    need[n] = dstTotal; srcAt[n] = srcTotal;                       // (need[] now holds destination offsets)
    // staging layout: [srcOff][dstOff][result][src blob][dst blob]
    size_t const oSrcOff = 0, oDstOff = offBytes, oRes = 2 * offBytes, oSrc = 3 * offBytes, oDst = (oSrc + (size_t)srcTotal + 15) & ~(size_t)15;
    size_t const total = oDst + (size_t)dstTotal + 16;
    if (!ensure_staging(sl, total)) return ZJNI_ERR(ZJNI_ERROR_unsupported);      // no room to stage this batch: the caller's CPU path takes it
    u64* const hs = (u64*)(sl->hPinned + oSrcOff); u64* const hd = (u64*)(sl->hPinned + oDstOff); const u64* const hr = (const u64*)(sl->hPinned + oRes);
    memcpy(hs, srcAt.data(), offBytes); memcpy(hd, need.data(), offBytes);
    u8* const hSrc = sl->hPinned + oSrc; u8* const hDst = sl->hPinned + oDst;
    // slices by destination bytes: a small first one, then up to eight of at least ZJ_HOST_SLICE
    std::vector<size_t> cuts; cuts.push_back(0);
    {   u64 const big = dstTotal / 8 > ZJ_HOST_SLICE ? dstTotal / 8 : ZJ_HOST_SLICE; u64 target = big / 4;
        for (size_t lo = 0; lo < n;) { size_t hi = lo + 1; while (hi < n && hd[hi] - hd[lo] < target) hi++; cuts.push_back(hi); lo = hi; target = big; } }
    size_t const nSlices = cuts.size() - 1;
    if (sl->pipeEv.size() < 3 * nSlices) {
        size_t const have = sl->pipeEv.size(); sl->pipeEv.resize(3 * nSlices, nullptr);
        for (size_t k = have; k < 3 * nSlices; k++) if (hipEventCreateWithFlags(&sl->pipeEv[k], hipEventDisableTiming) != hipSuccess) { sl->pipeEv.resize(k); return ZJNI_ERR(ZJNI_ERROR_no_device); }
    }
    auto drain = [&](size_t code) { (void)hipStreamSynchronize(sl->hostIn); (void)hipStreamSynchronize(sl->hostK); (void)hipStreamSynchronize(sl->hostOut); return code; };   // nothing of ours in flight when the staging lock drops
    int const T = host_threads();
    std::atomic<bool> gathering(true);               // while the sources are still being gathered the two sides share the host's threads
    auto scatter = [&](size_t lo, size_t hi) {
        par_ranges(hd + lo, hi - lo, [&](size_t a0, size_t a1) {
            for (size_t i = lo + a0; i < lo + a1; i++) {
                result[i] = (size_t)hr[i];
                if (!zjni_isError(result[i]) && result[i]) memcpy(dst[i], hDst + hd[i], result[i]);
            }
        }, gathering.load() ? (T + 1) / 2 : T);
    };
    // the returning side runs on a thread of its own: slice k is handed to the caller as soon as it is back, whatever the enqueueing side is doing.
    // With one usable CPU (or when the thread cannot be created) the calling thread returns the slices itself after the last one is enqueued.
    std::mutex qm; std::condition_variable qcv; size_t enqueued = 0; std::atomic<bool> failed(false);
    auto return_slices = [&]() {
        (void)hipSetDevice(d->ordinal);
        for (size_t k = 0; k < nSlices; k++) {
            {   std::unique_lock<std::mutex> lk(qm); qcv.wait(lk, [&] { return enqueued > k || failed.load(); }); if (enqueued <= k) return; }
            if (hipEventSynchronize(sl->pipeEv[3 * k + 2]) != hipSuccess) { failed.store(true); return; }
            scatter(cuts[k], cuts[k + 1]);
        }
    };
    std::thread returner;
    if (T > 1) { try { returner = std::thread(return_slices); } catch (const std::system_error&) { /* no thread to be had: the serial path below */ } }
    bool const threaded = returner.joinable();
    struct Joiner { std::thread& t; std::atomic<bool>& f; std::mutex& m; std::condition_variable& cv; bool ok = false;
                    ~Joiner() { if (!ok) { std::lock_guard<std::mutex> g(m); f.store(true); } cv.notify_all(); if (t.joinable()) t.join(); } } joiner{returner, failed, qm, qcv};
    if (hipMemcpyAsync(sl->dStage, sl->hPinned, 2 * offBytes, hipMemcpyHostToDevice, sl->hostIn) != hipSuccess) return drain(ZJNI_ERR(ZJNI_ERROR_no_device));
    for (size_t k = 0; k < nSlices; k++) {
        size_t const lo = cuts[k], hi = cuts[k + 1];
        hipEvent_t const evIn = sl->pipeEv[3 * k], evK = sl->pipeEv[3 * k + 1], evOut = sl->pipeEv[3 * k + 2];
        par_ranges(hs + lo, hi - lo, [&](size_t a0, size_t a1) { for (size_t i = lo + a0; i < lo + a1; i++) if (srcSize[i]) memcpy(hSrc + hs[i], src[i], srcSize[i]); }, k == 0 ? T : (T + 1) / 2);
        if (hs[hi] > hs[lo] && hipMemcpyAsync(sl->dStage + oSrc + hs[lo], hSrc + hs[lo], (size_t)(hs[hi] - hs[lo]), hipMemcpyHostToDevice, sl->hostIn) != hipSuccess) return drain(ZJNI_ERR(ZJNI_ERROR_no_device));
        if (hipEventRecord(evIn, sl->hostIn) != hipSuccess || hipStreamWaitEvent(sl->hostK, evIn, 0) != hipSuccess) return drain(ZJNI_ERR(ZJNI_ERROR_no_device));
        size_t const r = zjni_decompress_batch_device_usingDDict(sl->dStage + oSrc, (const u64*)(sl->dStage + oSrcOff) + lo, sl->dStage + oDst, (const u64*)(sl->dStage + oDstOff) + lo,
                                                                 (u64*)(sl->dStage + oRes) + lo, hi - lo, ddict, sl->hostK);
        if (zjni_isError(r)) return drain(r);
        if (hipEventRecord(evK, sl->hostK) != hipSuccess || hipStreamWaitEvent(sl->hostOut, evK, 0) != hipSuccess) return drain(ZJNI_ERR(ZJNI_ERROR_no_device));
        if (hipMemcpyAsync(sl->hPinned + oRes + lo * 8, sl->dStage + oRes + lo * 8, (hi - lo) * 8, hipMemcpyDeviceToHost, sl->hostOut) != hipSuccess) return drain(ZJNI_ERR(ZJNI_ERROR_no_device));
        if (hd[hi] > hd[lo] && hipMemcpyAsync(hDst + hd[lo], sl->dStage + oDst + hd[lo], (size_t)(hd[hi] - hd[lo]), hipMemcpyDeviceToHost, sl->hostOut) != hipSuccess) return drain(ZJNI_ERR(ZJNI_ERROR_no_device));
        if (hipEventRecord(evOut, sl->hostOut) != hipSuccess) return drain(ZJNI_ERR(ZJNI_ERROR_no_device));
        {   std::lock_guard<std::mutex> g(qm); enqueued = k + 1; }
        qcv.notify_all();
    }
    gathering.store(false);
    joiner.ok = true;
    if (threaded) returner.join(); else return_slices();
    if (failed.load()) return drain(ZJNI_ERR(ZJNI_ERROR_no_device));
    return 0;
}

// ---- host-pointer batches: pack -> H2D -> kernel -> D2H -> scatter ------------------------------
// ZJNI_HOST_TRACE=1: the phases of a host-pointer compress call on stderr, milliseconds since the process's first one (two calls in flight: which phase waits for what)
static void host_trace(const void* job, const char* what) {
    static bool const on = zj_env("ZJNI_HOST_TRACE") != nullptr;
    if (!on) return;
    static auto const t0 = std::chrono::steady_clock::now();
    fprintf(stderr, "[zjni host %p] %8.1f ms  %s\n", job, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(), what);
}
static size_t host_batch(bool compress, const void* const* src, const size_t* srcSize, void* const* dst, const size_t* dstCap,
                         size_t* result, size_t n, int level, int checksum = 0, const zjni_ddict* ddict = nullptr, const zjni_cdict* cdict = nullptr) {
    DevState* d = cur_state();
    if (!d) return ZJNI_ERR(ZJNI_ERROR_no_device);
    if (n == 0) return 0;
    size_t srcTotal = 0, dstTotal = 0;
    for (size_t i = 0; i < n; i++) {                   // one staging blob each way: its size must be representable (and allocatable)
        if (srcSize[i] > ((size_t)1 << 46) || dstCap[i] > ((size_t)1 << 46)) return ZJNI_ERR(64);
        srcTotal += srcSize[i]; dstTotal += dstCap[i];
        if (srcTotal > ((size_t)1 << 46) || dstTotal > ((size_t)1 << 46)) return ZJNI_ERR(64);
        if ((srcSize[i] && !src[i]) || (dstCap[i] && !dst[i])) return ZJNI_ERR(compress ? 72 : 72);
    }
    if (!compress) return host_decompress(d, src, srcSize, dst, dstCap, result, n, ddict);
    size_t const offBytes = (n + 1) * 8;
    // staging layout: [srcOff][dstOff][result][packedOff][src blob][dst blob][device only, compress: packed frames]
    size_t const oSrcOff = 0, oDstOff = offBytes, oRes = 2 * offBytes, oPOff = 3 * offBytes, oSrc = 4 * offBytes, oDst = (oSrc + srcTotal + 15) & ~(size_t)15;
    size_t const oPack = (oDst + dstTotal + 15) & ~(size_t)15;
    size_t const total = oPack + (compress ? dstTotal : 0) + 16;
    host_trace(result, "call");
    SlotLock slotLock(d); StageSlot* const sl = slotLock.s;      // one of the device's staging slots: a second caller stages and copies while this one's kernels run
    if (!ensure_staging(sl, total)) return ZJNI_ERR(ZJNI_ERROR_unsupported);     // no room to stage this batch: the caller's CPU path takes it
    hipStream_t const hst = sl->hostK;            // everything of this call in order on the slot's own stream
    struct Drain { hipStream_t st; ~Drain() { (void)hipStreamSynchronize(st); } } drainOnExit{hst};     // error returns below leave copies in flight on the staging area: none when the slot is given back
    u64* hs = (u64*)(sl->hPinned + oSrcOff); u64* hd = (u64*)(sl->hPinned + oDstOff); u64* hp = (u64*)(sl->hPinned + oPOff);
    size_t a = 0, b = 0;
    for (size_t i = 0; i < n; i++) { hs[i] = a; hd[i] = b; a += srcSize[i]; b += dstCap[i]; }
    hs[n] = a; hd[n] = b;
    u8* const hSrc = sl->hPinned + oSrc;
    // in slices of ~256 MiB: while the link carries slice k the host threads gather slice k + 1 into the pinned area
    if (hipMemcpyAsync(sl->dStage, sl->hPinned, oSrc, hipMemcpyHostToDevice, hst) != hipSuccess) return ZJNI_ERR(ZJNI_ERROR_no_device);
    for (size_t lo = 0; lo < n;) {
        size_t hi = lo + 1; while (hi < n && hs[hi] - hs[lo] < ZJ_HOST_SLICE) hi++;
        par_ranges(hs + lo, hi - lo, [&](size_t a0, size_t a1) { for (size_t i = lo + a0; i < lo + a1; i++) if (srcSize[i]) memcpy(hSrc + hs[i], src[i], srcSize[i]); });
        if (hs[hi] > hs[lo] && hipMemcpyAsync(sl->dStage + oSrc + hs[lo], hSrc + hs[lo], (size_t)(hs[hi] - hs[lo]), hipMemcpyHostToDevice, hst) != hipSuccess) return ZJNI_ERR(ZJNI_ERROR_no_device);
        lo = hi;
    }
    host_trace(result, "sources gathered, H2D enqueued");
    size_t r;
    if (compress && cdict)
        r = zjni_compress_batch_device_usingCDict(sl->dStage + oSrc, (const u64*)(sl->dStage + oSrcOff), sl->dStage + oDst, (const u64*)(sl->dStage + oDstOff),
                                                  (u64*)(sl->dStage + oRes), n, cdict, checksum, hst);
    else if (compress)                             // `level` may be a level word (zjni_compress_batch_advanced)
        r = compress_chunked(sl->dStage + oSrc, (const u64*)(sl->dStage + oSrcOff), sl->dStage + oDst, (const u64*)(sl->dStage + oDstOff),
                             (u64*)(sl->dStage + oRes), n, level, zj_frame_flags(checksum), hst);
    else
        r = zjni_decompress_batch_device_usingDDict(sl->dStage + oSrc, (const u64*)(sl->dStage + oSrcOff), sl->dStage + oDst, (const u64*)(sl->dStage + oDstOff),
                                                    (u64*)(sl->dStage + oRes), n, ddict, hst);
    if (zjni_isError(r)) return r;
    host_trace(result, "kernels enqueued");
    if (hipMemcpyAsync(sl->hPinned + oRes, sl->dStage + oRes, n * 8, hipMemcpyDeviceToHost, hst) != hipSuccess) return ZJNI_ERR(ZJNI_ERROR_no_device);
    const u64* hr = (const u64*)(sl->hPinned + oRes);
    const u64* from = hd;                              // where frame i's bytes start inside the returned blob
    if (compress) {
        // the destinations are compressBound-sized: pack the frames on the device and bring back only their bytes
        if (hipStreamSynchronize(hst) != hipSuccess) return ZJNI_ERR(ZJNI_ERROR_no_device);
        host_trace(result, "kernels done");
        u64 acc = 0;
        for (size_t i = 0; i < n; i++) { hp[i] = acc; if (!zjni_isError((size_t)hr[i])) acc += hr[i]; }
        hp[n] = acc;
        if (hipMemcpyAsync(sl->dStage + oPOff, hp, offBytes, hipMemcpyHostToDevice, hst) != hipSuccess) return ZJNI_ERR(ZJNI_ERROR_no_device);
        size_t const pr = zjni_pack_batch_device(sl->dStage + oDst, (const u64*)(sl->dStage + oDstOff), (const u64*)(sl->dStage + oRes),
                                                 sl->dStage + oPack, (const u64*)(sl->dStage + oPOff), n, hst);
        if (zjni_isError(pr)) return pr;
        from = hp;
    }
    // the way back in slices too: the host threads scatter slice k into the caller's buffers while the link carries slice k + 1
    u8* const dOut = sl->dStage + (compress ? oPack : oDst);
    u8* const hDst = sl->hPinned + oDst;
    std::vector<size_t> cuts; cuts.push_back(0);
    for (size_t lo = 0; lo < n;) { size_t hi = lo + 1; while (hi < n && from[hi] - from[lo] < ZJ_HOST_SLICE) hi++; cuts.push_back(hi); lo = hi; }
    size_t const nSlices = cuts.size() - 1;
    if (sl->stageEv.size() < nSlices) {
        size_t const have = sl->stageEv.size(); sl->stageEv.resize(nSlices, nullptr);
        for (size_t k = have; k < nSlices; k++) if (hipEventCreateWithFlags(&sl->stageEv[k], hipEventDisableTiming) != hipSuccess) return ZJNI_ERR(ZJNI_ERROR_no_device);
    }
    for (size_t k = 0; k < nSlices; k++) {
        size_t const lo = cuts[k], hi = cuts[k + 1];
        if (from[hi] > from[lo] && hipMemcpyAsync(hDst + from[lo], dOut + from[lo], (size_t)(from[hi] - from[lo]), hipMemcpyDeviceToHost, hst) != hipSuccess) return ZJNI_ERR(ZJNI_ERROR_no_device);
        if (hipEventRecord(sl->stageEv[k], hst) != hipSuccess) return ZJNI_ERR(ZJNI_ERROR_no_device);
    }
    host_trace(result, "D2H enqueued");
    for (size_t k = 0; k < nSlices; k++) {
        size_t const lo = cuts[k], hi = cuts[k + 1];
        if (hipEventSynchronize(sl->stageEv[k]) != hipSuccess) return ZJNI_ERR(ZJNI_ERROR_no_device);
        if (k + 1 == nSlices) host_trace(result, "last slice back");
        par_ranges(from + lo, hi - lo, [&](size_t a0, size_t a1) {
            for (size_t i = lo + a0; i < lo + a1; i++) {
                result[i] = (size_t)hr[i];
                if (!zjni_isError(result[i]) && result[i]) memcpy(dst[i], hDst + from[i], result[i]);
            }
        });
    }
    host_trace(result, "scattered: done");
    return 0;
}

size_t zjni_decompress_batch(const void* const* src, const size_t* srcSize, void* const* dst, const size_t* dstCap, size_t* result, size_t n) {
    return host_batch(false, src, srcSize, dst, dstCap, result, n, 0);
}

// ---- asynchronous host batches (include/zjni_amd.h: two in flight through the device's two staging slots) ----
struct zjni_batch_job { std::thread worker; size_t code = 0; };
static zjni_batch_job* batch_begin(bool compress, const void* const* src, const size_t* srcSize, void* const* dst, const size_t* dstCap,
                                   size_t* result, size_t n, int level, int checksum) {
    DevState* d = cur_state();
    if (!d) return nullptr;
    int const ordinal = d->ordinal;
    zjni_batch_job* job = new (std::nothrow) zjni_batch_job();
    if (!job) return nullptr;
    try {
        job->worker = std::thread([=]() {
            if (zjni_init(ordinal) != 0) { job->code = ZJNI_ERR(ZJNI_ERROR_no_device); return; }      // binds the worker to the caller's device
            job->code = compress ? zjni_compress_batch2(src, srcSize, dst, dstCap, result, n, level, checksum) : zjni_decompress_batch(src, srcSize, dst, dstCap, result, n);
        });
    } catch (const std::system_error&) { delete job; return nullptr; }
    return job;
}
zjni_batch_job* zjni_compress_batch_begin(const void* const* src, const size_t* srcSize, void* const* dst, const size_t* dstCap, size_t* result, size_t n, int level, int checksum) {
    return batch_begin(true, src, srcSize, dst, dstCap, result, n, level, checksum);
}
zjni_batch_job* zjni_decompress_batch_begin(const void* const* src, const size_t* srcSize, void* const* dst, const size_t* dstCap, size_t* result, size_t n) {
    return batch_begin(false, src, srcSize, dst, dstCap, result, n, 0, 0);
}
size_t zjni_batch_finish(zjni_batch_job* job) {
    if (!job) return ZJNI_ERR(ZJNI_ERROR_no_device);
    if (job->worker.joinable()) job->worker.join();
    size_t const code = job->code;
    delete job;
    return code;
}

// ---- one host batch over several devices of this process (SURVEY.md section 8e at the boundary a JVM has: one process) ----
// The batch is cut into contiguous index ranges of about equal source bytes, one per listed device; a thread per device binds it
// (zjni_init) and runs its range through the host-pointer path.  mode 0: every device returns its frames to the host over its
// own PCIe link (no inter-GPU traffic — the right choice when the consumer is host memory, as with JVM buffers).  mode 1
// (compress only): the devices pack their frames and send them to devices[0] over xGMI (peer copies, the gather of section 8e),
// which returns the whole batch to the host in one transfer.
static void multi_ranges(const size_t* srcSize, size_t n, int nd, std::vector<size_t>& cut) {
    size_t total = 0; for (size_t i = 0; i < n; i++) total += srcSize[i];
    cut.assign((size_t)nd + 1, n); cut[0] = 0;
    size_t acc = 0; int k = 1;
    for (size_t i = 0; i < n && k < nd; i++) {
        acc += srcSize[i];
        while (k < nd && acc * (size_t)nd >= total * (size_t)k && acc > 0) cut[(size_t)k++] = i + 1;
    }
    for (; k < nd; k++) cut[(size_t)k] = n;
    for (int j = 1; j <= nd; j++) if (cut[(size_t)j] < cut[(size_t)j - 1]) cut[(size_t)j] = cut[(size_t)j - 1];
}
static size_t multi_run(bool compress, const void* const* src, const size_t* srcSize, void* const* dst, const size_t* dstCap, size_t* result, size_t n,
                        int level, int checksum, const int* devices, int nDevices) {
    if (n == 0) return 0;
    if (!devices || nDevices < 1 || nDevices > 64) return ZJNI_ERR(42);
    for (int j = 0; j < nDevices; j++) if (devices[j] < 0 || devices[j] >= dev_count()) return ZJNI_ERR(ZJNI_ERROR_no_device);
    std::vector<size_t> cut; multi_ranges(srcSize, n, nDevices, cut);
    std::vector<size_t> rc((size_t)nDevices, 0);
    std::vector<std::thread> th;
    for (int j = 0; j < nDevices; j++) th.emplace_back([&, j]() {
        size_t const lo = cut[(size_t)j], cnt = cut[(size_t)j + 1] - lo;
        if (!cnt) return;
        if (zjni_init(devices[j]) != 0) { rc[(size_t)j] = ZJNI_ERR(ZJNI_ERROR_no_device); return; }
        rc[(size_t)j] = host_batch(compress, src + lo, srcSize + lo, dst + lo, dstCap + lo, result + lo, cnt, level, checksum);
    });
    for (auto& t : th) t.join();
    for (int j = 0; j < nDevices; j++) if (zjni_isError(rc[(size_t)j])) return rc[(size_t)j];
    return 0;
}
// mode 1: compress on every device, pack there, peer-copy the packed frames to devices[0], one D2H from there
static size_t multi_compress_gather(const void* const* src, const size_t* srcSize, void* const* dst, const size_t* dstCap, size_t* result, size_t n,
                                    int level, int checksum, const int* devices, int nDevices) {
    if (n == 0) return 0;
    if (!devices || nDevices < 1 || nDevices > 64) return ZJNI_ERR(42);
    for (int j = 0; j < nDevices; j++) if (devices[j] < 0 || devices[j] >= dev_count()) return ZJNI_ERR(ZJNI_ERROR_no_device);
    std::vector<size_t> cut; multi_ranges(srcSize, n, nDevices, cut);
    struct Part { u8* dSrc = nullptr; u8* dComp = nullptr; u8* dPacked = nullptr; u64* dOff = nullptr; u64* dCOff = nullptr; u64* dRes = nullptr; u64* dPOff = nullptr;
                  std::vector<u64> res, poff; size_t packed = 0, rc = 0; };
    std::vector<Part> parts((size_t)nDevices);
    auto phase1 = [&](int j) {
        Part& p = parts[(size_t)j]; size_t const lo = cut[(size_t)j], cnt = cut[(size_t)j + 1] - lo;
        if (!cnt) return;
        if (zjni_init(devices[j]) != 0) { p.rc = ZJNI_ERR(ZJNI_ERROR_no_device); return; }
        size_t st = 0, ct = 0; std::vector<u64> so(cnt + 1), co(cnt + 1);
        for (size_t i = 0; i < cnt; i++) { so[i] = st; co[i] = ct; st += srcSize[lo + i]; ct += dstCap[lo + i]; }
        so[cnt] = st; co[cnt] = ct;
        std::vector<u8> stage(st + 16);
        for (size_t i = 0; i < cnt; i++) if (srcSize[lo + i]) memcpy(stage.data() + so[i], src[lo + i], srcSize[lo + i]);
        bool ok = hipMalloc(&p.dSrc, st + 16) == hipSuccess && hipMalloc(&p.dComp, ct + 16) == hipSuccess && hipMalloc(&p.dOff, (cnt + 1) * 8) == hipSuccess
               && hipMalloc(&p.dCOff, (cnt + 1) * 8) == hipSuccess && hipMalloc(&p.dRes, cnt * 8) == hipSuccess && hipMalloc(&p.dPOff, (cnt + 1) * 8) == hipSuccess;
        ok = ok && hipMemcpy(p.dSrc, stage.data(), st, hipMemcpyHostToDevice) == hipSuccess && hipMemcpy(p.dOff, so.data(), (cnt + 1) * 8, hipMemcpyHostToDevice) == hipSuccess
                && hipMemcpy(p.dCOff, co.data(), (cnt + 1) * 8, hipMemcpyHostToDevice) == hipSuccess;
        if (!ok) { p.rc = ZJNI_ERR(64); return; }
        size_t const r = zjni_compress_batch_device2(p.dSrc, p.dOff, p.dComp, p.dCOff, p.dRes, cnt, level, checksum, nullptr);
        if (zjni_isError(r)) { p.rc = r; return; }
        p.res.resize(cnt); p.poff.resize(cnt + 1);
        if (hipMemcpy(p.res.data(), p.dRes, cnt * 8, hipMemcpyDeviceToHost) != hipSuccess) { p.rc = ZJNI_ERR(ZJNI_ERROR_no_device); return; }
        size_t a = 0; for (size_t i = 0; i < cnt; i++) { p.poff[i] = a; if (!zjni_isError((size_t)p.res[i])) a += p.res[i]; }
        p.poff[cnt] = a; p.packed = a;
        ok = hipMalloc(&p.dPacked, a + 16) == hipSuccess && hipMemcpy(p.dPOff, p.poff.data(), (cnt + 1) * 8, hipMemcpyHostToDevice) == hipSuccess;
        if (!ok) { p.rc = ZJNI_ERR(64); return; }
        size_t const r2 = zjni_pack_batch_device(p.dComp, p.dCOff, p.dRes, p.dPacked, p.dPOff, cnt, nullptr);
        if (zjni_isError(r2) || hipDeviceSynchronize() != hipSuccess) p.rc = ZJNI_ERR(ZJNI_ERROR_no_device);
    };
    {   std::vector<std::thread> th; for (int j = 0; j < nDevices; j++) th.emplace_back(phase1, j); for (auto& t : th) t.join(); }
    size_t rc = 0, total = 0;
    for (auto& p : parts) { if (zjni_isError(p.rc) && !rc) rc = p.rc; total += p.packed; }
    u8* gather = nullptr; std::vector<u8> host;
    if (!rc) {
        if (hipSetDevice(devices[0]) != hipSuccess || hipMalloc(&gather, total + 16) != hipSuccess) rc = ZJNI_ERR(64);
        size_t at = 0;
        for (int j = 0; j < nDevices && !rc; j++) {            // the xGMI step: every device's packed frames land behind each other on devices[0]
            Part& p = parts[(size_t)j];
            if (p.packed && hipMemcpyPeer(gather + at, devices[0], p.dPacked, devices[j], p.packed) != hipSuccess) rc = ZJNI_ERR(ZJNI_ERROR_no_device);
            at += p.packed;
        }
        host.resize(total + 16);
        if (!rc && total && hipMemcpy(host.data(), gather, total, hipMemcpyDeviceToHost) != hipSuccess) rc = ZJNI_ERR(ZJNI_ERROR_no_device);
        size_t base = 0;
        for (int j = 0; j < nDevices && !rc; j++) {
            Part& p = parts[(size_t)j]; size_t const lo = cut[(size_t)j], cnt = cut[(size_t)j + 1] - lo;
            for (size_t i = 0; i < cnt; i++) {
                result[lo + i] = (size_t)p.res[i];
                if (!zjni_isError(result[lo + i]) && result[lo + i]) memcpy(dst[lo + i], host.data() + base + p.poff[i], result[lo + i]);
            }
            base += p.packed;
        }
    }
    if (gather) { (void)hipSetDevice(devices[0]); (void)hipFree(gather); }
    for (int j = 0; j < nDevices; j++) {
        Part& p = parts[(size_t)j];
        if (!p.dSrc && !p.dComp) continue;
        (void)hipSetDevice(devices[j]);
        (void)hipFree(p.dSrc); (void)hipFree(p.dComp); (void)hipFree(p.dPacked); (void)hipFree(p.dOff); (void)hipFree(p.dCOff); (void)hipFree(p.dRes); (void)hipFree(p.dPOff);
    }
    return rc;
}
size_t zjni_compress_batch_multi(const void* const* src, const size_t* srcSize, void* const* dst, const size_t* dstCap, size_t* result, size_t n,
                                 int level, int checksum, const int* devices, int nDevices, int mode) {
    if (level == 0) level = 3;
    if (!zj_level_served(level)) return ZJNI_ERR(42);
    if (mode == 1) return multi_compress_gather(src, srcSize, dst, dstCap, result, n, level, checksum ? 1 : 0, devices, nDevices);
    return multi_run(true, src, srcSize, dst, dstCap, result, n, level, checksum ? 1 : 0, devices, nDevices);
}
size_t zjni_decompress_batch_multi(const void* const* src, const size_t* srcSize, void* const* dst, const size_t* dstCap, size_t* result, size_t n,
                                   const int* devices, int nDevices) {
    return multi_run(false, src, srcSize, dst, dstCap, result, n, 0, 0, devices, nDevices);
}
size_t zjni_compress_batch(const void* const* src, const size_t* srcSize, void* const* dst, const size_t* dstCap, size_t* result, size_t n, int level) {
    if (level == 0) level = 3;                    // ZSTD_CLEVEL_DEFAULT, as ZSTD_c_compressionLevel = 0 means
    if (!zj_level_served(level)) return ZJNI_ERR(42);
    return host_batch(true, src, srcSize, dst, dstCap, result, n, level);
}

size_t zjni_compress_batch2(const void* const* src, const size_t* srcSize, void* const* dst, const size_t* dstCap, size_t* result, size_t n, int level, int checksum) {
    if (level == 0) level = 3;                    // ZSTD_CLEVEL_DEFAULT, as ZSTD_c_compressionLevel = 0 means
    if (!zj_level_served(level)) return ZJNI_ERR(42);
    return host_batch(true, src, srcSize, dst, dstCap, result, n, level, checksum ? 1 : 0);
}

size_t zjni_compress_batch_advanced(const void* const* src, const size_t* srcSize, void* const* dst, const size_t* dstCap, size_t* result, size_t n,
                                    int level, int checksum, int hashLog, int chainLog) {
    if (level == 0) level = 3;                    // ZSTD_CLEVEL_DEFAULT, as ZSTD_c_compressionLevel = 0 means
    int lw; size_t const e = level_word(level, hashLog, chainLog, &lw);
    if (e) return e;
    if (!zj_level_served(level) || (level > 3 && (hashLog | chainLog))) return ZJNI_ERR(42);
    return host_batch(true, src, srcSize, dst, dstCap, result, n, lw, checksum);
}
// ---- cross-thread aggregation of per-buffer calls (second half) ----
// zstd-jni's per-buffer natives are called from many threads, one context each, one buffer per call; a GPU wants thousands of
// buffers per launch.  An aggregator turns concurrent blocking per-buffer calls into batches: the first caller of a kind (compress
// at a level + checksum flag, or decompress) opens a batch and waits up to maxWaitMicros for company, callers that arrive meanwhile
// join it, the opener runs the batch entry once and everybody returns with its own result.  Results are those of the batch entries
// (byte-identical frames); what changes is latency (up to the wait) against launches shared.  One device per aggregator.
struct ZjAggReq { const void* src; size_t srcSize; void* dst; size_t dstCap; size_t result; };
struct ZjAggBatch { std::vector<ZjAggReq*> reqs; bool closed = false, done = false; size_t bytes = 0; };
#define ZJ_AGG_MAX_BYTES ((size_t)2 << 30)          /* staging a batch may ask for (sources + destination capacities): a member that would push it past this opens the next batch */
struct zjni_aggregator {
    int device; size_t maxBatch; unsigned maxWaitMicros;
    std::mutex mu; std::condition_variable cv;
    std::map<int, std::shared_ptr<ZjAggBatch> > open;           // kind -> the batch that is still taking members
    unsigned long long calls = 0, batches = 0;
};
static size_t agg_run(int kind, const void* const* sp, const size_t* ss, void* const* dp, const size_t* dc, size_t* res, size_t n, int level, int checksum) {
    return kind < 0 ? zjni_decompress_batch(sp, ss, dp, dc, res, n) : zjni_compress_batch2(sp, ss, dp, dc, res, n, level, checksum);
}
static size_t agg_submit(zjni_aggregator* a, int kind, ZjAggReq& rq, int level, int checksum) {
    if (!a) return ZJNI_ERR(ZJNI_ERROR_unsupported);
    // a member's own faults are its own: checked before it joins, so that no one else's call fails for them
    if (rq.srcSize > ((size_t)1 << 46) || rq.dstCap > ((size_t)1 << 46)) return ZJNI_ERR(64);
    if ((rq.srcSize && !rq.src) || (rq.dstCap && !rq.dst)) return ZJNI_ERR(72);
    size_t const mine = rq.srcSize + rq.dstCap;
    std::unique_lock<std::mutex> lk(a->mu);
    a->calls++;
    std::shared_ptr<ZjAggBatch> b;
    auto it = a->open.find(kind);
    bool leader = false;
    if (it != a->open.end() && !it->second->closed && !it->second->reqs.empty() && it->second->bytes + mine > ZJ_AGG_MAX_BYTES) {   // would outgrow the staging: that batch goes now
        it->second->closed = true; a->cv.notify_all();
    }
    if (it == a->open.end() || it->second->closed) { b = std::make_shared<ZjAggBatch>(); a->open[kind] = b; leader = true; a->batches++; }
    else b = it->second;
    b->reqs.push_back(&rq); b->bytes += mine;
    if (b->reqs.size() >= a->maxBatch) { b->closed = true; a->cv.notify_all(); }
    if (!leader) {
        a->cv.wait(lk, [&]() { return b->done; });
        return rq.result;
    }
    // the opener: wait for company, close the batch, run it outside the lock
    a->cv.wait_for(lk, std::chrono::microseconds(a->maxWaitMicros), [&]() { return b->closed; });
    b->closed = true;
    if (a->open[kind] == b) a->open.erase(kind);
    std::vector<ZjAggReq*> reqs = b->reqs;                       // (members only join while !closed: the list is final)
    lk.unlock();
    size_t const n = reqs.size();
    std::vector<const void*> sp(n); std::vector<size_t> ss(n), dc(n), res(n); std::vector<void*> dp(n);
    for (size_t i = 0; i < n; i++) { sp[i] = reqs[i]->src; ss[i] = reqs[i]->srcSize; dp[i] = reqs[i]->dst; dc[i] = reqs[i]->dstCap; }
    size_t rc = 0;
    if (zjni_init(a->device) != 0) rc = ZJNI_ERR(ZJNI_ERROR_no_device);
    else rc = agg_run(kind, sp.data(), ss.data(), dp.data(), dc.data(), res.data(), n, level, checksum);
    if (zjni_isError(rc)) {
        // the shared launch failed as a whole (staging, a device error): every member gets its own verdict from a call of its own — what it
        // would have got without the aggregator — instead of a stranger's error
        for (size_t i = 0; i < n; i++) {
            size_t r1 = 0; size_t const rr = n == 1 ? rc : agg_run(kind, &sp[i], &ss[i], &dp[i], &dc[i], &r1, 1, level, checksum);
            res[i] = zjni_isError(rr) ? rr : r1;
        }
    }
    lk.lock();
    for (size_t i = 0; i < n; i++) reqs[i]->result = res[i];
    b->done = true;
    a->cv.notify_all();
    return rq.result;
}
zjni_aggregator* zjni_createAggregator(int device, size_t maxBatch, unsigned maxWaitMicros) {
    if (device < 0 || device >= dev_count() || maxBatch < 1) return nullptr;
    zjni_aggregator* a = new zjni_aggregator();
    a->device = device; a->maxBatch = maxBatch > 65536 ? 65536 : maxBatch; a->maxWaitMicros = maxWaitMicros;
    return a;
}
void zjni_freeAggregator(zjni_aggregator* a) { delete a; }        // no call may be in flight
size_t zjni_aggregator_compress(zjni_aggregator* a, void* dst, size_t dstCap, const void* src, size_t srcSize, int level, int checksum) {
    if (level == 0) level = 3;
    if (!zj_level_served(level)) return ZJNI_ERR(42);
    if (level < ZJ_LEVEL_MIN) level = ZJ_LEVEL_MIN;
    ZjAggReq rq = { src, srcSize, dst, dstCap, 0 };
    int const kind = (level > 0 ? level * 2 : 32 - level * 2) + (checksum ? 1 : 0);      // compress kinds: 2..17 for levels 1-8, from 34 on for negative levels; decompress is -1
    return agg_submit(a, kind, rq, level, checksum ? 1 : 0);
}
size_t zjni_aggregator_decompress(zjni_aggregator* a, void* dst, size_t dstCap, const void* src, size_t srcSize) {
    ZjAggReq rq = { src, srcSize, dst, dstCap, 0 };
    return agg_submit(a, -1, rq, 0, 0);
}
void zjni_aggregator_stats(zjni_aggregator* a, unsigned long long* calls, unsigned long long* batches) {
    std::lock_guard<std::mutex> lk(a->mu);
    if (calls) *calls = a->calls;
    if (batches) *batches = a->batches;
}

size_t zjni_compress(void* dst, size_t dstCap, const void* src, size_t srcSize, int level) {
    size_t res = 0; const void* s = src; void* dd = dst;
    size_t const r = zjni_compress_batch(&s, &srcSize, &dd, &dstCap, &res, 1, level);
    return zjni_isError(r) ? r : res;
}
size_t zjni_compress2(void* dst, size_t dstCap, const void* src, size_t srcSize, int level, int checksum) {
    size_t res = 0; const void* s = src; void* dd = dst;
    size_t const r = zjni_compress_batch2(&s, &srcSize, &dd, &dstCap, &res, 1, level, checksum);
    return zjni_isError(r) ? r : res;
}
size_t zjni_compress_batch_usingCDict(const void* const* src, const size_t* srcSize, void* const* dst, const size_t* dstCap, size_t* result, size_t n,
                                      const zjni_cdict* cdict, int checksum) {
    if (!cdict) return ZJNI_ERR(32);
    return host_batch(true, src, srcSize, dst, dstCap, result, n, cdict->level, checksum, nullptr, cdict);
}
size_t zjni_compress_usingCDict(void* dst, size_t dstCap, const void* src, size_t srcSize, const zjni_cdict* cdict) {
    size_t res = 0; const void* s = src; void* dd = dst;
    size_t const r = zjni_compress_batch_usingCDict(&s, &srcSize, &dd, &dstCap, &res, 1, cdict, 0);
    return zjni_isError(r) ? r : res;
}
size_t zjni_decompress_batch_usingDDict(const void* const* src, const size_t* srcSize, void* const* dst, const size_t* dstCap, size_t* result, size_t n,
                                        const zjni_ddict* ddict) {
    return host_batch(false, src, srcSize, dst, dstCap, result, n, 0, 0, ddict);
}
size_t zjni_decompress_usingDDict(void* dst, size_t dstCap, const void* src, size_t srcSize, const zjni_ddict* ddict) {
    size_t res = 0; const void* s = src; void* dd = dst;
    size_t const r = zjni_decompress_batch_usingDDict(&s, &srcSize, &dd, &dstCap, &res, 1, ddict);
    return zjni_isError(r) ? r : res;
}
size_t zjni_decompress(void* dst, size_t dstCap, const void* src, size_t srcSize) {
    size_t res = 0; const void* s = src; void* dd = dst;
    size_t const r = zjni_decompress_batch(&s, &srcSize, &dd, &dstCap, &res, 1);
    return zjni_isError(r) ? r : res;
}

void zjni_synth_fill_host(void* dst, size_t bufSize, uint64_t firstIndex, size_t nBuffers) {
    for (size_t i = 0; i < nBuffers; i++) zs_fill((u8*)dst + i * bufSize, (u32)bufSize, firstIndex + i);
}
size_t zjni_synth_fill_device(void* d_dst, size_t bufSize, uint64_t firstIndex, size_t nBuffers, void* stream) {
    if (!cur_state()) return ZJNI_ERR(ZJNI_ERROR_no_device);
    if (nBuffers == 0) return 0;
    hipLaunchKernelGGL(zj_synth_kernel, dim3((u32)((nBuffers + 63) / 64)), dim3(64), 0, (hipStream_t)stream, (u8*)d_dst, (u32)bufSize, firstIndex, (u32)nBuffers);
    return hipGetLastError() == hipSuccess ? 0 : ZJNI_ERR(ZJNI_ERROR_no_device);
}

// exclusive prefix sums of a batch's result sizes (error results count as 0) -> off[0 .. n]: one workgroup, a contiguous run per lane, one scan over the lanes' sums
__global__ __launch_bounds__(1024) void zj_pack_offsets_kernel(const u64* __restrict__ sizes, u64* __restrict__ off, u32 n) {
    __shared__ u64 part[1024];
    u32 const t = threadIdx.x;
    u64 const per = ((u64)n + 1023u) / 1024u, lo0 = (u64)t * per, lo = lo0 < n ? lo0 : n, hi = lo + per < n ? lo + per : n;      // (64-bit: n up to 2^32 - 1 — ADVICE r05)
    u64 sum = 0;
    for (u64 i = lo; i < hi; i++) { u64 const z = sizes[i]; sum += z > ((u64)1 << 40) ? 0 : z; }
    part[t] = sum;
    __syncthreads();
    for (u32 d = 1; d < 1024u; d <<= 1) {                // (Hillis-Steele over 1 024 sums)
        u64 const v = t >= d ? part[t - d] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    u64 run = t ? part[t - 1] : 0;
    for (u64 i = lo; i < hi; i++) { off[i] = run; u64 const z = sizes[i]; run += z > ((u64)1 << 40) ? 0 : z; }
    if (t == 1023u) off[n] = part[1023];
}
size_t zjni_pack_batch_device2(const void* d_src, const uint64_t* d_src_off, const uint64_t* d_sizes,
                               void* d_dst, uint64_t* d_packed_off, size_t n, void* stream) {
    DevState* d = cur_state();
    if (!d) return ZJNI_ERR(ZJNI_ERROR_no_device);
    if (n > 0xFFFFFFFFull) return ZJNI_ERR(64);
    if (n == 0) return hipMemsetAsync(d_packed_off, 0, 8, (hipStream_t)stream) == hipSuccess ? 0 : ZJNI_ERR(ZJNI_ERROR_no_device);
    hipLaunchKernelGGL(zj_pack_offsets_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, (const u64*)d_sizes, (u64*)d_packed_off, (u32)n);
    return zjni_pack_batch_device(d_src, d_src_off, d_sizes, d_dst, d_packed_off, n, stream);
}
size_t zjni_pack_batch_device(const void* d_src, const uint64_t* d_src_off, const uint64_t* d_sizes,
                              void* d_dst, const uint64_t* d_dst_off, size_t n, void* stream) {
    DevState* d = cur_state();
    if (!d) return ZJNI_ERR(ZJNI_ERROR_no_device);
    if (n == 0) return 0;
    u32 const grid = (u32)(n < (size_t)d->numCU * 8 ? n : (size_t)d->numCU * 8);
    hipLaunchKernelGGL(zj_pack_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const u8*)d_src, (const u64*)d_src_off,
                       (const u64*)d_sizes, (u8*)d_dst, (const u64*)d_dst_off, (u32)n);
    return hipGetLastError() == hipSuccess ? 0 : ZJNI_ERR(ZJNI_ERROR_no_device);
}

// ============================================================================ large buffers as many frames (zj_frames.h) ============
// zjni_decompress_frames_batch_device and zjni_compress_chunked_batch_device turn n large buffers into E small entries on the device, run the existing batch
// pipelines on the entries and fold the entries' answers back into one per buffer.  The pipelines take their batch size by value and size their scratch on the
// host, so the one thing the host has to know is E — eight bytes read back through pinned memory behind the count and its scan, the only host wait of either
// entry.  Everything else follows on `stream` in order.
//
// framesBuf holds, per call: the per-buffer arrays (counts, their scans, carries), the per-entry arrays and, for the chunked compress, the entries' scratch
// destinations of one slice.
//
// What every entry of this section shares is written once: frames_room and frames_read_total (framesBuf and a scan's totals, the one host wait), the range tail
// of the two range entries (RangePlan: range_plan_read, range_plan_decode, range_plan_scatter) and their finish loop (zj_range_finish_body), StagedCall for the
// blocking forms for one host buffer, packed_call for the host batch forms of the sequence entries, frames_stat_get behind the zjni_last_* getters, and the
// argument rules zj_level_arg, dict_on_this_device and grid_cap.  A new entry brings its own arithmetic and calls these.
static bool zj_level_arg(int& level) { if (level == 0) level = 3; return zj_level_served(level); }      // 0 = ZSTD_CLEVEL_DEFAULT, as ZSTD_c_compressionLevel = 0 means
static bool dict_on_this_device(int ordinal) { return ordinal == t_dev || t_dev < 0; }                  // (else: digested on another device, 32)
static u32 grid_cap(const DevState* d, size_t n) { return (u32)(n < (size_t)d->numCU * 8 ? n : (size_t)d->numCU * 8); }      // a wave or workgroup per item, eight per CU at most
static bool frames_state(DevState* d) {
    if (!d->framesStat && hipMalloc(&d->framesStat, 64) != hipSuccess) { d->framesStat = nullptr; (void)hipGetLastError(); return false; }
    if (!d->framesE) {
        void* hp = nullptr;
        if (hipHostMalloc(&hp, 64, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); return false; }
        if (hipEventCreateWithFlags(&d->evFramesE, hipEventDisableTiming) != hipSuccess) { (void)hipHostFree(hp); (void)hipGetLastError(); return false; }
        memset(hp, 0, 64); d->framesE = (volatile u64*)hp;
    }
    return true;
}
// at least `need` bytes of framesBuf; with keep != 0 the first `keep` bytes survive a move (the per-buffer arrays, written before E was known)
static size_t frames_room(DevState* d, size_t need, size_t keep, hipStream_t st) {
    if (d->framesBufCap >= need) return 0;
    if (g_scratch_limit && need > g_scratch_limit) return ZJNI_ERR(64);
    size_t const cap = need + (need >> 3) + 4096;
    u8* fresh = nullptr;
    if (hipStreamSynchronize(st) != hipSuccess) return ZJNI_ERR(ZJNI_ERROR_no_device);
    if (hipMalloc(&fresh, cap) != hipSuccess) { (void)hipGetLastError(); return ZJNI_ERR(64); }
    if (keep && hipMemcpy(fresh, d->framesBuf, keep, hipMemcpyDeviceToDevice) != hipSuccess) { (void)hipFree(fresh); return ZJNI_ERR(ZJNI_ERROR_no_device); }
    if (d->framesBuf) (void)hipFree(d->framesBuf);          // (drains the device: an earlier call may still be reading it)
    d->framesBuf = fresh; d->framesBufCap = cap;
    return 0;
}
// k consecutive words (scan totals: first[n] = E) -> out[0 .. k) on the host, and one word more from d_also, when given, -> out[k]; 8 words at most.  The entry's one host
// wait: for the count kernel and its scan only (and for whatever the stream held before them).
static size_t frames_read_total(DevState* d, const u64* d_words, size_t k, hipStream_t st, u64* out, const u64* d_also = nullptr) {
    if (hipMemcpyAsync((void*)d->framesE, d_words, k * 8, hipMemcpyDeviceToHost, st) != hipSuccess
        || (d_also && hipMemcpyAsync((void*)(d->framesE + k), d_also, 8, hipMemcpyDeviceToHost, st) != hipSuccess)
        || hipEventRecord(d->evFramesE, st) != hipSuccess || hipEventSynchronize(d->evFramesE) != hipSuccess) return ZJNI_ERR(ZJNI_ERROR_no_device);
    for (size_t i = 0; i < k + (d_also ? 1 : 0); i++) out[i] = d->framesE[i];
    return 0;
}
static inline size_t zj_up16(size_t v) { return (v + 15) & ~(size_t)15; }
// the counters of one entry (four words of framesStat from `word`) behind everything the device holds; zeros while no call has made them
static int frames_stat_get(u32 word, unsigned out4[4]) {
    DevState* d = cur_state();
    if (!d || !out4) return -(int)ZJNI_ERROR_no_device;
    u32 h[4] = {0, 0, 0, 0};
    if (hipDeviceSynchronize() != hipSuccess || (d->framesStat && hipMemcpy(h, d->framesStat + word, sizeof h, hipMemcpyDeviceToHost) != hipSuccess)) return -(int)ZJNI_ERROR_no_device;
    for (int k = 0; k < 4; k++) out4[k] = h[k];
    return 0;
}
// A host batch through one device buffer of the call's own, synchronous: `image` (packed on the host) goes to the buffer's front, run(buf) enqueues the device
// entry on the null stream, [aRes, all) — results, then payload — comes back in `back`.  One copy each way.
extern "C++" { template <class Run>      // (a template cannot have C linkage)
static size_t packed_call(const std::vector<u8>& image, size_t aRes, size_t all, std::vector<u8>& back, Run run) {
    u8* buf = nullptr;
    if (hipMalloc(&buf, all ? all : 1) != hipSuccess) { (void)hipGetLastError(); return ZJNI_ERR(64); }
    size_t r = 0;
    if (hipMemcpy(buf, image.data(), image.size(), hipMemcpyHostToDevice) != hipSuccess) r = ZJNI_ERR(ZJNI_ERROR_no_device);
    if (r == 0) r = run(buf);
    back.resize(all - aRes);
    if (r == 0 && (hipStreamSynchronize(nullptr) != hipSuccess || hipMemcpy(back.data(), buf + aRes, all - aRes, hipMemcpyDeviceToHost) != hipSuccess)) r = ZJNI_ERR(ZJNI_ERROR_no_device);
    if (hipDeviceSynchronize() != hipSuccess && r == 0) r = ZJNI_ERR(ZJNI_ERROR_no_device);       // nothing may still use `buf`
    (void)hipFree(buf);
    return r;
} }

// ---- frames from the caller's sequences: ZSTD_compressSequences for batches (zj_sequences.h) ----
// Two launches on `stream`, nothing else: the conversion (a wave per frame from a work counter) and the frame loop (a workgroup per frame from a second one).
// Records, literal offsets and block entries live in framesBuf — 20 bytes per sequence of the call and 4 per frame, counted as scratch (zjni_set_scratch_limit;
// a call whose records alone exceed the limit answers 64) — whose size is the one thing the host has to know: d_seq_off[n], eight bytes read back once through
// pinned memory, the entry's only host wait.  A frame's slice of the array is checked against that total on the device before anything of it is read.
// Without delimiters the same read-back brings d_src_off[n] too: 24 bytes a sequence (the prefix word more), 40 bytes per 64 KiB of the batch's sources and 320 per frame.
__global__ __launch_bounds__(64) void zj_seq_convert_kernel(const u64* __restrict__ srcOff, const ZSSeq* __restrict__ seqs, const u64* __restrict__ seqOff, u64 total,
                                                            ZESeq* __restrict__ rec, u32* __restrict__ lit, u32* __restrict__ nBlk, u32 n, u32 level, u32 flags, u32* workCounter) {
    GrpSeq<64> g;
    for (;;) {
        u32 const i = zj_next_index(workCounter);
        if (i >= n) break;
        u64 const q0 = zj_uni64(seqOff[i]), q1 = zj_uni64(seqOff[i + 1]), s0 = zj_uni64(srcOff[i]), s1 = zj_uni64(srcOff[i + 1]);
        // The shape of zj_seq_cut_kernel, for its reason: one way through the body and ONE place where lane 0 alone writes, with the workgroup's barrier
        // between it and the next index (a lane-0 store that `continue`s into zj_next_index lets the compiler send the other 63 lanes ahead on their own).
        u32 answer = 1u;                                                                                         // 1: convert; else the word for nBlk[i]
        if (q0 > q1 || q1 > total || q1 - q0 > 0x7FFFFFFFull || s1 < s0) answer = ZS_NO_FRAME;
        else {
            u64 const size64 = s1 - s0;
            u32 const srcSize = size64 > 0xFFFFFFFFull ? 0xFFFFFFFFu : (u32)size64;
            ZEParams const p = ze_params_of(level, srcSize);
            if (p.strategy == 0u || srcSize > ZE_MULTI_MAX) answer = 0u;                                         // the frame loop answers 201 before it looks at a slot
            else zs_convert(g, seqs + q0, (u32)(q1 - q0), srcSize, zs_ml_min(p), zs_max_nbseq(p, srcSize), (flags & ZS_FLAG_REPCODES) != 0u, rec + q0 + i, lit + q0 + i, nBlk + i);
        }
        if (answer != 1u && threadIdx.x == 0) nBlk[i] = answer;
        __syncthreads();
    }
}
// (the register budget of zj_encode_kernel, whose stage this is: three waves per SIMD)
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(3, 8))) void zj_encode_sequences_kernel(const u8* __restrict__ src, const u64* __restrict__ srcOff, const u64* __restrict__ seqOff,
                                                                 u8* __restrict__ dst, const u64* __restrict__ dstOff, u64* __restrict__ result, u32 n, u32 level, u32 flags,
                                                                 ZESeq* rec, const u32* lit, const u32* nBlk, u32* workCounter, u8* scratch, u32 ldsBytes) {
    __shared__ ZEncShared sh;
    __shared__ ZSState st;
    ZjProf pf; pf.start(nullptr);
    GrpSeq<64> g;
    if (threadIdx.x == 0) { sh.dictLoaded = 0; sh.ctDict[0] = 0; sh.ctDict[1] = 0; sh.ctDict[2] = 0; }
    __syncthreads();
    u8* const ws = scratch + (size_t)blockIdx.x * ZE_SCRATCH_BYTES;
    for (;;) {
        u32 const i = zj_next_index(workCounter);
        if (i >= n) break;
        u64 const s0 = zj_uni64(srcOff[i]), s1 = zj_uni64(srcOff[i + 1]), d0 = zj_uni64(dstOff[i]), d1 = zj_uni64(dstOff[i + 1]);
        u32 const nb = ZJ_UNI(nBlk[i]);
        u64 const q0 = nb == ZS_NO_FRAME ? 0 : zj_uni64(seqOff[i]);
        u64 const cap = d1 - d0;
        u64 r;
        if (s1 < s0 || d1 < d0) r = ZJ_ERR64(ZJ_E_SRCSIZE_WRONG);
        else if (s1 - s0 > ZE_MULTI_MAX) r = ZJ_ERR64(201);
        else r = zs_compress_frame(g, sh, st, zj_dyn_lds, src + s0, (u32)(s1 - s0), dst + d0, (u32)(cap > 0xFFFFFFFFull ? 0xFFFFFFFFull : cap), level, flags,
                                   rec + q0 + i, lit + q0 + i, nb, ws, pf, ldsBytes);
        if (threadIdx.x == 0) result[i] = r;
        __syncthreads();
    }
}
// ZJNI_SEQ_NO_DELIMITERS: the same two steps with the library cutting the blocks (zj_sequences.h, "no block delimiters").  The conversion also takes a word a sequence for
// the prefix, and frame i's slots start at zs_nd_slot_base — which places the slices apart only while both offset arrays ascend, so a frame that finds its own pair
// descending or beyond the totals the host read raises counter word 2, and the frame loop then answers srcSize_wrong (72) for every frame of the call before it reads a slot.
__global__ __launch_bounds__(64) void zj_seq_cut_kernel(const u64* __restrict__ srcOff, const ZSSeq* __restrict__ seqs, const u64* __restrict__ seqOff, u64 total, u64 totalSrc, u64 slots,
                                                        u32* __restrict__ pfx, ZESeq* __restrict__ rec, u32* __restrict__ lit, u32* __restrict__ nBlk, u32 n, u32 level, u32* workCounter, u32* badOffsets) {
    GrpSeq<64> g;
    for (;;) {
        u32 const i = zj_next_index(workCounter);
        if (i >= n) break;
        u64 const q0 = zj_uni64(seqOff[i]), q1 = zj_uni64(seqOff[i + 1]), s0 = zj_uni64(srcOff[i]), s1 = zj_uni64(srcOff[i + 1]);
        bool const descending = q0 > q1 || q1 > total || s1 < s0 || s1 > totalSrc;
        // One way through the body and ONE place where lane 0 alone writes, with the workgroup's barrier between it and the next index.  A lane-0 branch
        // that `continue`s straight into zj_next_index lets the compiler send the other 63 lanes ahead on their own: their v_readfirstlane then reads
        // lane 1's zero and they take frame 0 again — seen on the device as another frame's block count overwritten, and as a wave that never ends.
        u32 answer = 1u;                                                                                         // 1: convert; else the word for nBlk[i]
        if (descending || q1 - q0 > 0x7FFFFFFFull) answer = ZS_NO_FRAME;
        else {
            u64 const size64 = s1 - s0;
            u32 const srcSize = size64 > 0xFFFFFFFFull ? 0xFFFFFFFFu : (u32)size64;
            ZEParams const p = ze_params_of(level, srcSize);
            if (p.strategy == 0u || srcSize > ZE_MULTI_MAX) answer = 0u;                                         // the frame loop answers 201 before it looks at a slot
            else {
                u32 const cnt = (u32)(q1 - q0);
                u64 const base = zs_nd_slot_base(q0, s0, i), mine = (u64)cnt + 2u * zs_nd_max_blocks(srcSize);
                if (base + mine > slots) answer = ZS_NO_FRAME;                                                   // (cannot happen while the offsets ascend)
                else zs_convert_nodelim(g, seqs + q0, cnt, srcSize, zs_ml_min(p), p.minMatch, zs_max_nbseq(p, srcSize), pfx + q0, rec + base, lit + base, (u32)mine, nBlk + i);
            }
        }
        if (answer != 1u && threadIdx.x == 0) { nBlk[i] = answer; if (descending) atomicOr(badOffsets, 1u); }
        __syncthreads();
    }
}
// zj_encode_sequences_kernel for those slots: zs_compress_frame's no-delimiter instantiation
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(3, 8))) void zj_encode_sequences_nodelim_kernel(const u8* __restrict__ src, const u64* __restrict__ srcOff, const u64* __restrict__ seqOff,
                                                                 u8* __restrict__ dst, const u64* __restrict__ dstOff, u64* __restrict__ result, u32 n, u32 level, u32 flags,
                                                                 ZESeq* rec, const u32* lit, const u32* nBlk, u32* workCounter, const u32* badOffsets, u8* scratch, u32 ldsBytes) {
    __shared__ ZEncShared sh;
    __shared__ ZSState st;
    ZjProf pf; pf.start(nullptr);
    GrpSeq<64> g;
    if (threadIdx.x == 0) { sh.dictLoaded = 0; sh.ctDict[0] = 0; sh.ctDict[1] = 0; sh.ctDict[2] = 0; }
    __syncthreads();
    u8* const ws = scratch + (size_t)blockIdx.x * ZE_SCRATCH_BYTES;
    bool const apart = ZJ_UNI(*badOffsets) == 0u;
    for (;;) {
        u32 const i = zj_next_index(workCounter);
        if (i >= n) break;
        u64 const s0 = zj_uni64(srcOff[i]), s1 = zj_uni64(srcOff[i + 1]), d0 = zj_uni64(dstOff[i]), d1 = zj_uni64(dstOff[i + 1]);
        u32 const nb = ZJ_UNI(nBlk[i]);
        u64 const base = (nb == ZS_NO_FRAME || nb == 0u || !apart) ? 0 : zs_nd_slot_base(zj_uni64(seqOff[i]), s0, i);
        u64 const cap = d1 - d0;
        u64 r;
        if (s1 < s0 || d1 < d0 || !apart) r = ZJ_ERR64(ZJ_E_SRCSIZE_WRONG);
        else if (s1 - s0 > ZE_MULTI_MAX) r = ZJ_ERR64(201);
        else r = zs_compress_frame<GrpSeq<64>, true>(g, sh, st, zj_dyn_lds, src + s0, (u32)(s1 - s0), dst + d0, (u32)(cap > 0xFFFFFFFFull ? 0xFFFFFFFFull : cap), level, flags,
                                                     rec + base, lit + base, nb, ws, pf, ldsBytes);
        if (threadIdx.x == 0) result[i] = r;
        __syncthreads();
    }
}
static std::atomic<int> g_seq_grid(0);           // zjni_debug_sequences_grid
int zjni_debug_sequences_grid(int grid) { return g_seq_grid.exchange(grid < 0 ? 0 : grid); }
size_t zjni_sequenceBound(size_t srcSize) { return (size_t)zs_sequence_bound(srcSize); }
size_t zjni_compress_sequences_batch_device(const void* d_src, const uint64_t* d_src_off, const zjni_sequence* d_seqs, const uint64_t* d_seq_off,
                                            void* d_dst, const uint64_t* d_dst_off, uint64_t* d_result, size_t n, int level, int flags, void* stream) {
    static_assert(sizeof(zjni_sequence) == 16 && sizeof(ZSSeq) == 16 && ZJNI_SEQ_REPCODES == ZS_FLAG_REPCODES && ZJNI_FRAME_CHECKSUM == ZE_FLAG_CHECKSUM, "zjni_sequence is ZSTD_Sequence");
    static_assert(ZJNI_SEQ_NO_DELIMITERS == ZS_FLAG_NODELIM, "the flag word");
    if (flags & ~(ZJNI_FRAME_CHECKSUM | ZJNI_SEQ_REPCODES | ZJNI_SEQ_NO_DELIMITERS)) return ZJNI_ERR(42);
    if (!zj_level_arg(level)) return ZJNI_ERR(42);
    if (n == 0) return 0;
    if (n > 0x7FFFFFFFull) return ZJNI_ERR(72);
    if (!d_src_off || !d_seq_off || !d_dst_off || !d_result) return ZJNI_ERR(42);
    bool const nodelim = (flags & ZJNI_SEQ_NO_DELIMITERS) != 0;
    flags &= ZJNI_FRAME_CHECKSUM | ZJNI_SEQ_REPCODES;
    DevState* d = cur_state();
    if (!d) return ZJNI_ERR(ZJNI_ERROR_no_device);
    BatchOrder order(d, stream);
    hipStream_t st = (hipStream_t)stream;
    if (!frames_state(d)) return ZJNI_ERR(64);
    u64 totals[2] = {0, 0};                                                          // d_seq_off[n], and without delimiters d_src_off[n]: the bound on the blocks needs the batch's bytes
    {   size_t const e = frames_read_total(d, (const u64*)d_seq_off + n, 1, st, totals, nodelim ? (const u64*)d_src_off + n : nullptr); if (e) return e; }
    u64 const total = totals[0], totalSrc = totals[1];
    if (total > ((u64)1 << 40) || totalSrc > ((u64)1 << 40)) return ZJNI_ERR(64);
    if (total && !d_seqs) return ZJNI_ERR(42);
    size_t const slots = nodelim ? (size_t)zs_nd_slots(total, totalSrc, n) : (size_t)total + n;
    size_t const offNblk = 64, offLit = offNblk + zj_up16(n * 4), offRec = offLit + zj_up16(slots * 4), offPfx = offRec + slots * 16, need = offPfx + (nodelim ? (size_t)total * 4 : 0);
    {   size_t const e = frames_room(d, need, 0, st); if (e) return e; }
    u32* const ctr = (u32*)d->framesBuf;
    if (hipMemsetAsync(ctr, 0, 64, st) != hipSuccess) return ZJNI_ERR(ZJNI_ERROR_no_device);
    if (!d->seqGrid) {                                                               // resident workgroups of the frame loop, asked for once (under BatchOrder)
        int perCU = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&perCU, zj_encode_sequences_kernel, 64, sizeof(ZEEntropy)) != hipSuccess || perCU < 1) { (void)hipGetLastError(); perCU = 1; }
        d->seqGrid = d->numCU * perCU;
        if (d->seqGrid > d->encGrid) d->seqGrid = d->encGrid;                        // a scratch slot per workgroup
    }
    int grid = d->seqGrid;
    int const want = g_seq_grid.load();
    if (want > 0 && want < grid) grid = want;
    if ((size_t)grid > n) grid = (int)n;
    u32 const lw = zs_level_word(level);
    ZESeq* const rec = (ZESeq*)(d->framesBuf + offRec); u32* const lit = (u32*)(d->framesBuf + offLit); u32* const nBlk = (u32*)(d->framesBuf + offNblk);
    size_t convGrid = grid_cap(d, n); if (want > 0 && (size_t)want < convGrid) convGrid = (size_t)want;
    if (nodelim) {
        hipLaunchKernelGGL(zj_seq_cut_kernel, dim3((u32)convGrid), dim3(64), 0, st, (const u64*)d_src_off, (const ZSSeq*)d_seqs, (const u64*)d_seq_off, total, totalSrc, (u64)slots,
                           (u32*)(d->framesBuf + offPfx), rec, lit, nBlk, (u32)n, lw, ctr, ctr + 2);
        if (hipGetLastError() != hipSuccess) return ZJNI_ERR(ZJNI_ERROR_no_device);
        hipLaunchKernelGGL(zj_encode_sequences_nodelim_kernel, dim3((u32)grid), dim3(64), sizeof(ZEEntropy), st, (const u8*)d_src, (const u64*)d_src_off, (const u64*)d_seq_off, (u8*)d_dst,
                           (const u64*)d_dst_off, (u64*)d_result, (u32)n, lw, (u32)flags, rec, (const u32*)lit, (const u32*)nBlk, ctr + 1, (const u32*)(ctr + 2), d->encScratch, (u32)sizeof(ZEEntropy));
        return hipGetLastError() == hipSuccess ? 0 : ZJNI_ERR(ZJNI_ERROR_no_device);
    }
    hipLaunchKernelGGL(zj_seq_convert_kernel, dim3((u32)convGrid), dim3(64), 0, st, (const u64*)d_src_off, (const ZSSeq*)d_seqs, (const u64*)d_seq_off, total, rec, lit, nBlk, (u32)n, lw, (u32)flags, ctr);
    if (hipGetLastError() != hipSuccess) return ZJNI_ERR(ZJNI_ERROR_no_device);
    hipLaunchKernelGGL(zj_encode_sequences_kernel, dim3((u32)grid), dim3(64), sizeof(ZEEntropy), st, (const u8*)d_src, (const u64*)d_src_off, (const u64*)d_seq_off, (u8*)d_dst,
                       (const u64*)d_dst_off, (u64*)d_result, (u32)n, lw, (u32)flags, rec, (const u32*)lit, (const u32*)nBlk, ctr + 1, d->encScratch, (u32)sizeof(ZEEntropy));
    return hipGetLastError() == hipSuccess ? 0 : ZJNI_ERR(ZJNI_ERROR_no_device);
}
// Host arrays: sources, sequence arrays and destinations go through one device buffer of the call's own (packed on the host, one copy each way).  Synchronous.
size_t zjni_compress_sequences_batch(const void* const* src, const size_t* srcSize, const zjni_sequence* const* seqs, const size_t* nSeqs,
                                     void* const* dst, const size_t* dstCap, size_t* result, size_t n, int level, int flags) {
    if (flags & ~(ZJNI_FRAME_CHECKSUM | ZJNI_SEQ_REPCODES | ZJNI_SEQ_NO_DELIMITERS)) return ZJNI_ERR(42);
    if (!zj_level_arg(level)) return ZJNI_ERR(42);
    if (n == 0) return 0;
    if (n > 0x7FFFFFFFull) return ZJNI_ERR(72);
    if (!src || !srcSize || !seqs || !nSeqs || !dst || !dstCap || !result) return ZJNI_ERR(42);
    std::vector<u64> off(3 * (n + 1));
    u64* const so = off.data(); u64* const qo = so + n + 1; u64* const dof = qo + n + 1;
    so[0] = qo[0] = dof[0] = 0;
    for (size_t i = 0; i < n; i++) {
        if ((srcSize[i] && !src[i]) || (nSeqs[i] && !seqs[i]) || (dstCap[i] && !dst[i])) return ZJNI_ERR(72);
        if (srcSize[i] > ((size_t)1 << 40) || nSeqs[i] > ((size_t)1 << 36) || dstCap[i] > ((size_t)1 << 40)) return ZJNI_ERR(64);
        so[i + 1] = so[i] + srcSize[i]; qo[i + 1] = qo[i] + nSeqs[i]; dof[i + 1] = dof[i] + dstCap[i];
    }
    if (!cur_state()) return ZJNI_ERR(ZJNI_ERROR_no_device);
    size_t const aSrc = 0, aSeq = zj_up16(so[n]), aOff = aSeq + zj_up16(qo[n] * 16), inBytes = aOff + off.size() * 8;
    size_t const aRes = zj_up16(inBytes), aDst = aRes + zj_up16(n * 8), all = aDst + dof[n];
    std::vector<u8> image(inBytes);
    for (size_t i = 0; i < n; i++) {
        if (srcSize[i]) memcpy(image.data() + aSrc + so[i], src[i], srcSize[i]);
        if (nSeqs[i]) memcpy(image.data() + aSeq + qo[i] * 16, seqs[i], nSeqs[i] * 16);
    }
    memcpy(image.data() + aOff, off.data(), off.size() * 8);
    std::vector<u8> back;
    size_t const r = packed_call(image, aRes, all, back, [&](u8* buf) {
        const u64* const dOff = (const u64*)(buf + aOff);
        return zjni_compress_sequences_batch_device(buf + aSrc, dOff, (const zjni_sequence*)(buf + aSeq), dOff + n + 1, buf + aDst, dOff + 2 * (n + 1), (uint64_t*)(buf + aRes), n, level, flags, nullptr);
    });
    if (r) return r;
    const u64* const res = (const u64*)back.data();
    for (size_t i = 0; i < n; i++) {
        result[i] = (size_t)res[i];
        if (!zjni_isError((size_t)res[i]) && res[i] <= dstCap[i] && res[i]) memcpy(dst[i], back.data() + (aDst - aRes) + dof[i], (size_t)res[i]);
    }
    return 0;
}
size_t zjni_compress_sequences(void* dst, size_t dstCapacity, const zjni_sequence* seqs, size_t nSeqs, const void* src, size_t srcSize, int level, int flags) {
    if ((flags & ZJNI_SEQ_NO_DELIMITERS) && !dst) return ZJNI_ERR(42);      // the new mode's one-buffer form wants a destination: no frame fits in none (header)
    size_t res = 0; const void* s = src; void* dd = dst; const zjni_sequence* q = seqs;
    size_t const r = zjni_compress_sequences_batch(&s, &srcSize, &q, &nSeqs, &dd, &dstCapacity, &res, 1, level, flags);
    return zjni_isError(r) ? r : res;
}

// ---- the matchers' sequences out: ZSTD_generateSequences for batches (zj_generate.h) ----
// A dispatcher of its own with one route, one launch on `stream`: zj_generate_kernel, a workgroup of one wave per frame from a work counter, parse and export
// (zg_generate_frame) over the workgroup's tables (ensure_multi_tables) and scratch slot, the wave matcher's scoreboards in the dynamic LDS.  It takes every frame:
// single-block and multi-block ones, levels 1-8 and the negative ones, and the frames that only have an answer (empty, refused).  The lane pipeline's scratch is not
// touched, so what the last compress call promised about its tables still holds.  No host wait; counters (u32, 64 bytes of framesBuf): [4] work, [10] refused.
// Not here yet: the lane match kernels in their plain launch form followed by an export kernel for large batches of small frames.
__global__ __launch_bounds__(64, ZJ_MULTI_WAVES) void zj_generate_kernel(const u8* __restrict__ src, const u64* __restrict__ srcOff, ZSSeq* __restrict__ seqs, const u64* __restrict__ seqOff,
                                                                          u64* __restrict__ result, u32 level, u32 count, u32* workCounter,
                                                                          u8* scratch, u32* tables, u32* refused) {
    __shared__ ZEncShared sh;
    Grp<64> g;
    u8* const ws = scratch + (size_t)blockIdx.x * ZE_SCRATCH_BYTES;
    u32* const tb = tables + (size_t)blockIdx.x * (ZE_MULTI_TABLE_BYTES / 4u);
    for (;;) {
        u32 const i = zj_next_index(workCounter);
        if (i >= count) break;
        u64 const s0 = zj_uni64(srcOff[i]), s1 = zj_uni64(srcOff[i + 1]), q0 = zj_uni64(seqOff[i]), q1 = zj_uni64(seqOff[i + 1]);
        u64 r;
        if (s1 < s0 || q1 < q0) r = ZJ_ERR64(ZJ_E_SRCSIZE_WRONG);
        else if (s1 - s0 > ZE_MULTI_MAX) r = ZJ_ERR64(201);
        else r = zg_generate_frame(g, sh, zj_dyn_lds, src + s0, (u32)(s1 - s0), seqs + q0, q1 - q0, level, ws, tb);
        if (threadIdx.x == 0) { result[i] = r; if (r > ZJ_ERR64(256)) atomicAdd(refused, 1u); }
        __syncthreads();
    }
}
static std::atomic<int> g_gen_grid(0);           // zjni_debug_generate_grid
int zjni_debug_generate_grid(int grid) { return g_gen_grid.exchange(grid < 0 ? 0 : grid); }
int zjni_last_generate(unsigned out4[4]) {
    DevState* d = cur_state();
    if (!d || !out4) return -(int)ZJNI_ERROR_no_device;
    u32 h[16];
    const u8* const at = d->genCounters;
    if (!at || at != d->framesBuf) return -1;                                         // no generate call since the buffer last moved
    if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(h, at, sizeof h, hipMemcpyDeviceToHost) != hipSuccess) return -(int)ZJNI_ERROR_no_device;
    out4[0] = 0; out4[1] = d->genFrames; out4[2] = h[10]; out4[3] = 0;               // (no lane route yet: every frame takes the wave route)
    return 0;
}
size_t zjni_mergeBlockDelimiters(zjni_sequence* seqs, size_t nSeqs) { return seqs ? zg_merge_block_delimiters((ZSSeq*)seqs, nSeqs) : 0; }
size_t zjni_generate_sequences_batch_device(const void* d_src, const uint64_t* d_src_off, zjni_sequence* d_seqs, const uint64_t* d_seq_off,
                                            uint64_t* d_result, size_t n, int level, int flags, void* stream) {
    if (flags) return ZJNI_ERR(42);               // none is defined yet
    if (!zj_level_arg(level)) return ZJNI_ERR(42);
    if (n == 0) return 0;
    if (n > 0xFFFFFFFFull) return ZJNI_ERR(72);
    if (!d_src_off || !d_seq_off || !d_result) return ZJNI_ERR(42);
    DevState* d = cur_state();
    if (!d) return ZJNI_ERR(ZJNI_ERROR_no_device);
    BatchOrder order(d, stream);
    hipStream_t st = (hipStream_t)stream;
    u32 const lw = (u32)zj_level3_word((int)zs_level_word(level));
    {   size_t const e = frames_room(d, 64, 0, st); if (e) return e; }
    if (!ensure_multi_tables(d)) return ZJNI_ERR(64);
    u32* const ctr = (u32*)d->framesBuf;
    d->genCounters = d->framesBuf; d->genFrames = (u32)n;
    if (hipMemsetAsync(ctr, 0, 64, st) != hipSuccess) return ZJNI_ERR(ZJNI_ERROR_no_device);
    int const want = g_gen_grid.load();
    size_t grid = (size_t)d->multiGrid; if (grid > n) grid = n; if (want > 0 && (size_t)want < grid) grid = (size_t)want;
    hipLaunchKernelGGL(zj_generate_kernel, dim3((u32)grid), dim3(64), (u32)zj_up16(sizeof(ZXLds)), st, (const u8*)d_src, (const u64*)d_src_off, (ZSSeq*)d_seqs, (const u64*)d_seq_off,
                       (u64*)d_result, lw, (u32)n, ctr + 4, d->encScratch, d->multiTables, ctr + 10);
    return hipGetLastError() == hipSuccess ? 0 : ZJNI_ERR(ZJNI_ERROR_no_device);
}
// Host arrays: sources and slots go through one device buffer of the call's own (packed on the host, one copy each way).  Synchronous.
size_t zjni_generate_sequences_batch(const void* const* src, const size_t* srcSize, zjni_sequence* const* seqs, const size_t* seqCapacity, size_t* result, size_t n, int level, int flags) {
    if (flags) return ZJNI_ERR(42);
    if (!zj_level_arg(level)) return ZJNI_ERR(42);
    if (n == 0) return 0;
    if (n > 0xFFFFFFFFull) return ZJNI_ERR(72);
    if (!src || !srcSize || !seqs || !seqCapacity || !result) return ZJNI_ERR(42);
    std::vector<u64> off(2 * (n + 1));
    u64* const so = off.data(); u64* const qo = so + n + 1;
    so[0] = qo[0] = 0;
    for (size_t i = 0; i < n; i++) {
        if ((srcSize[i] && !src[i]) || (seqCapacity[i] && !seqs[i])) return ZJNI_ERR(72);
        if (srcSize[i] > ((size_t)1 << 40) || seqCapacity[i] > ((size_t)1 << 36)) return ZJNI_ERR(64);
        so[i + 1] = so[i] + srcSize[i]; qo[i + 1] = qo[i] + seqCapacity[i];
    }
    if (!cur_state()) return ZJNI_ERR(ZJNI_ERROR_no_device);
    size_t const aOff = zj_up16(so[n]), inBytes = aOff + off.size() * 8;
    size_t const aRes = zj_up16(inBytes), aSeq = aRes + zj_up16(n * 8), all = aSeq + qo[n] * 16;
    std::vector<u8> image(inBytes);
    for (size_t i = 0; i < n; i++) if (srcSize[i]) memcpy(image.data() + so[i], src[i], srcSize[i]);
    memcpy(image.data() + aOff, off.data(), off.size() * 8);
    std::vector<u8> back;
    size_t const r = packed_call(image, aRes, all, back, [&](u8* buf) {
        const u64* const dOff = (const u64*)(buf + aOff);
        return zjni_generate_sequences_batch_device(buf, dOff, (zjni_sequence*)(buf + aSeq), dOff + n + 1, (uint64_t*)(buf + aRes), n, level, flags, nullptr);
    });
    if (r) return r;
    const u64* const res = (const u64*)back.data();
    for (size_t i = 0; i < n; i++) {
        result[i] = (size_t)res[i];
        if (!zjni_isError((size_t)res[i]) && res[i] <= seqCapacity[i] && res[i]) memcpy(seqs[i], back.data() + (aSeq - aRes) + qo[i] * 16, (size_t)res[i] * 16);
    }
    return 0;
}
size_t zjni_generate_sequences(zjni_sequence* seqs, size_t seqCapacity, const void* src, size_t srcSize, int level) {
    size_t res = 0; const void* s = src; zjni_sequence* q = seqs;
    size_t const r = zjni_generate_sequences_batch(&s, &srcSize, &q, &seqCapacity, &res, 1, level, 0);
    return zjni_isError(r) ? r : res;
}
// ---- frame-parallel decompress ----
// first walk, one lane per buffer as zj_inspect_kernel walks: cnt[i] = entries of buffer i
__global__ __launch_bounds__(64) void zj_frames_count_kernel(const u8* __restrict__ src, const u64* __restrict__ off, u64* __restrict__ cnt, u32 n, u32* stat) {
    u64 const i = (u64)blockIdx.x * 64u + threadIdx.x;
    if (i >= n) return;
    u64 const lo = off[i], hi = off[i + 1];
    u32 const c = zj_frames_count(src + lo, hi > lo ? hi - lo : 0);
    cnt[i] = c;
    atomicAdd(&stat[c > 1u ? 0 : 1], 1u);
}
// second walk: the entries of buffer i at first[i]; the lane of the last buffer closes both arrays with the batch's ends
__global__ __launch_bounds__(64) void zj_frames_emit_kernel(const u8* __restrict__ src, const u64* __restrict__ off, const u64* __restrict__ dstOff, const u64* __restrict__ first,
                                                            u64* __restrict__ srcOffE, u64* __restrict__ dstOffE, u32 n) {
    u64 const i = (u64)blockIdx.x * 64u + threadIdx.x;
    if (i >= n) return;
    u64 const lo = off[i], hi = off[i + 1], dlo = dstOff[i], dhi = dstOff[i + 1], e0 = first[i], e1 = first[i + 1];
    zj_frames_emit(src + lo, hi > lo ? hi - lo : 0, lo, dlo, dhi > dlo ? dhi - dlo : 0, (u32)(e1 - e0), srcOffE + e0, dstOffE + e0);
    if (i + 1 == n) { srcOffE[e1] = hi; dstOffE[e1] = dhi; }
}
// One wave per buffer: the sum of its entries' sizes; a buffer with an entry that answered an error goes on the redo list instead.  A buffer of one entry
// (not split) takes that entry's answer as it is.
__global__ __launch_bounds__(64) void zj_frames_reduce_kernel(const u64* __restrict__ first, const u64* __restrict__ resE, u64* __restrict__ result, u32 n,
                                                              u32* __restrict__ redo, u32* stat) {
    u32 const lane = threadIdx.x;
    for (u32 i = blockIdx.x; i < n; i += gridDim.x) {
        u64 const lo = first[i], hi = first[i + 1];
        if (hi - lo == 1) { if (lane == 0) result[i] = resE[lo]; continue; }
        u64 sum = 0; u32 bad = 0;
        for (u64 e = lo + lane; e < hi; e += 64) { u64 const r = resE[e]; if (r > ((u64)1 << 40)) bad = 1; else sum += r; }
        for (u32 d = 32; d; d >>= 1) { sum += __shfl_xor(sum, (int)d, 64); bad |= __shfl_xor(bad, (int)d, 64); }
        if (lane == 0) {
            if (bad) redo[atomicAdd(&stat[2], 1u)] = i;
            else result[i] = sum;
        }
    }
}
size_t zjni_decompress_frames_batch_device(const void* d_src, const uint64_t* d_src_off, void* d_dst, const uint64_t* d_dst_off,
                                           uint64_t* d_result, size_t n, const zjni_ddict* ddict, void* stream) {
    if (ddict && !dict_on_this_device(ddict->ordinal)) return ZJNI_ERR(32);
    DevState* d = cur_state();
    if (!d) return ZJNI_ERR(ZJNI_ERROR_no_device);
    if (n > 0xFFFFFFFFull) return ZJNI_ERR(72);
    hipStream_t const st = (hipStream_t)stream;
    BatchOrder order(d, stream);
    if (!frames_state(d)) return ZJNI_ERR(64);
    if (hipMemsetAsync(d->framesStat, 0, 16, st) != hipSuccess) return ZJNI_ERR(ZJNI_ERROR_no_device);
    d->lastFramesE = 0;
    if (n == 0) return 0;
    // per buffer: [cnt n][first n + 1][redo n (u32)]
    size_t const oCnt = 0, oFirst = zj_up16(n * 8), oRedo = oFirst + zj_up16((n + 1) * 8), perBuf = oRedo + zj_up16(n * 4);
    size_t r = frames_room(d, perBuf, 0, st);
    if (r != 0) return r;
    hipLaunchKernelGGL(zj_frames_count_kernel, dim3((u32)((n + 63) / 64)), dim3(64), 0, st, (const u8*)d_src, (const u64*)d_src_off, (u64*)(d->framesBuf + oCnt), (u32)n, d->framesStat);
    hipLaunchKernelGGL(zj_pack_offsets_kernel, dim3(1), dim3(1024), 0, st, (const u64*)(d->framesBuf + oCnt), (u64*)(d->framesBuf + oFirst), (u32)n);
    u64 E = 0;
    if ((r = frames_read_total(d, (const u64*)(d->framesBuf + oFirst) + n, 1, st, &E)) != 0) return r;
    if (E > 0xFFFFFFFFull) return ZJNI_ERR(72);
    if (E < n) return ZJNI_ERR(ZJNI_ERROR_no_device);                           // (every buffer is at least one entry)
    // per entry: [srcOffE E + 1][dstOffE E + 1][resE E]
    size_t const oSrcE = perBuf, oDstE = oSrcE + zj_up16((E + 1) * 8), oResE = oDstE + zj_up16((E + 1) * 8), total = oResE + zj_up16(E * 8);
    if ((r = frames_room(d, total, perBuf, st)) != 0) return r;
    u8* const fb = d->framesBuf;
    hipLaunchKernelGGL(zj_frames_emit_kernel, dim3((u32)((n + 63) / 64)), dim3(64), 0, st, (const u8*)d_src, (const u64*)d_src_off, (const u64*)d_dst_off, (const u64*)(fb + oFirst),
                       (u64*)(fb + oSrcE), (u64*)(fb + oDstE), (u32)n);
    if (hipGetLastError() != hipSuccess) return ZJNI_ERR(ZJNI_ERROR_no_device);
    if ((r = decompress_chunked_ordered(d_src, (const u64*)(fb + oSrcE), d_dst, (const u64*)(fb + oDstE), (u64*)(fb + oResE), (size_t)E, ddict, stream)) != 0) return r;
    hipLaunchKernelGGL(zj_frames_reduce_kernel, dim3(grid_cap(d, n)), dim3(64), 0, st, (const u64*)(fb + oFirst), (const u64*)(fb + oResE), (u64*)d_result, (u32)n, (u32*)(fb + oRedo), d->framesStat);
    // the redo list: the fused kernel over the caller's own offsets, one wave per buffer; whatever it answers stands (an empty list is a launch that finds no work)
    if (ddict) {
        u32 const gridD = (u32)(n < (size_t)d->decDictGrid ? n : (size_t)d->decDictGrid);
        hipLaunchKernelGGL(zj_decode_dict_kernel, dim3(gridD), dim3(64), 0, st, (const u8*)d_src, (const u64*)d_src_off, (u8*)d_dst, (const u64*)d_dst_off, (u64*)d_result, (u32)n,
                           d->framesStat + 3, d->decScratch, d->prof, (const u32*)(fb + oRedo), (const u32*)(d->framesStat + 2), (const ZDDictDev*)ddict->buf, (const u8*)(ddict->buf + sizeof(ZDDictDev)));
    } else {
        u32 const gridD = (u32)(n < (size_t)d->decGrid ? n : (size_t)d->decGrid);
        hipLaunchKernelGGL(zj_decode_kernel, dim3(gridD), dim3(64), 0, st, (const u8*)d_src, (const u64*)d_src_off, (u8*)d_dst, (const u64*)d_dst_off, (u64*)d_result, (u32)n,
                           d->framesStat + 3, d->decScratch, d->prof, (const u32*)(fb + oRedo), (const u32*)(d->framesStat + 2), (const ZDDictDev*)nullptr, (const u8*)nullptr);
    }
    d->lastFramesE = E;
    return hipGetLastError() == hipSuccess ? 0 : ZJNI_ERR(ZJNI_ERROR_no_device);
}
int zjni_last_frames(unsigned* out4) {
    int const r = frames_stat_get(0, out4);
    if (r == 0) { out4[3] = out4[2]; out4[2] = out4[1]; out4[1] = (unsigned)cur_state()->lastFramesE; }      // the entries decoded are the host's count
    return r;
}

// ---- ranged decompress (zj_frames_range.h) ----
// per buffer: [rec n][q 5 x n][scan 5 x (n + 1)][totals 5].  The five quantities: entries of set A, entries of set B, compact source bytes of A, of B, scratch
// bytes of the edge frames.
// first walk, one lane per buffer like zj_frames_count_kernel: rules 1-4, the buffer's record and what the scans add up
__global__ __launch_bounds__(64) void zj_range_count_kernel(const u8* __restrict__ src, const u64* __restrict__ off, const u64* __restrict__ dstOff, const u64* __restrict__ range,
                                                            ZRRec* __restrict__ rec, u64* __restrict__ q, u64* __restrict__ total, u32 n) {
    u64 const i = (u64)blockIdx.x * 64u + threadIdx.x;
    if (i >= n) return;
    u64 const lo = off[i], hi = off[i + 1], dlo = dstOff[i], dhi = dstOff[i + 1];
    ZRRec r; u64 qq[5];
    zj_range_count(src + lo, hi > lo ? hi - lo : 0, range[2 * i], range[2 * i + 1], dhi > dlo ? dhi - dlo : 0, r, qq);
    rec[i] = r;
    for (u32 k = 0; k < 5; k++) q[(u64)k * n + i] = qq[k];
    if (total) total[i] = r.total;
}
// workgroup k: scan[k][0 .. n] = exclusive prefix sums of q[k][0 .. n), totals[k] = scan[k][n] (zj_pack_offsets_kernel's shape, five at once)
__global__ __launch_bounds__(1024) void zj_range_scan_kernel(const u64* __restrict__ q, u64* __restrict__ scan, u64* __restrict__ totals, u32 n) {
    __shared__ u64 part[1024];
    u32 const t = threadIdx.x;
    const u64* const in = q + (u64)blockIdx.x * n;
    u64* const out = scan + (u64)blockIdx.x * ((u64)n + 1u);
    u64 const per = ((u64)n + 1023u) / 1024u, lo0 = (u64)t * per, lo = lo0 < n ? lo0 : n, hi = lo + per < n ? lo + per : n;
    u64 sum = 0;
    for (u64 i = lo; i < hi; i++) sum += in[i];
    part[t] = sum;
    __syncthreads();
    for (u32 d = 1; d < 1024u; d <<= 1) {
        u64 const v = t >= d ? part[t - d] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    u64 run = t ? part[t - 1] : 0;
    for (u64 i = lo; i < hi; i++) { out[i] = run; run += in[i]; }
    if (t == 1023u) { out[n] = part[1023]; totals[blockIdx.x] = part[1023]; }
}
// second walk, one lane per buffer, from the recorded position of `first`: the entries of both sets and the copy runs; the lane of the last buffer closes the arrays.
// Set B's sources lie behind set A's in the compact bytes (at scan[2][n]).
__global__ __launch_bounds__(64) void zj_range_emit_kernel(const u8* __restrict__ src, const u64* __restrict__ off, const u64* __restrict__ dstOff, const ZRRec* __restrict__ rec,
                                                           const u64* __restrict__ scan, u32 n, u64* __restrict__ srcA, u64* __restrict__ dstA, u64* __restrict__ srcB,
                                                           u64* __restrict__ dstB, ZRCopy* __restrict__ in, ZRCopy* __restrict__ out) {
    u64 const i = (u64)blockIdx.x * 64u + threadIdx.x;
    if (i >= n) return;
    u64 const n1 = (u64)n + 1u;
    const u64* const fA = scan; const u64* const fB = scan + n1; const u64* const cA = scan + 2 * n1; const u64* const cB = scan + 3 * n1; const u64* const eB = scan + 4 * n1;
    u64 const lo = off[i], hi = off[i + 1], a0 = fA[i], a1 = fA[i + 1], b0 = fB[i];
    ZRRec const r = rec[i];
    ZRCopy cin[3], cout[2];
    zj_range_emit(src + lo, hi > lo ? hi - lo : 0, r, lo, dstOff[i], (u32)(a1 - a0 - 1u), cA[i], cA[n] + cB[i], eB[i], srcA + a0, dstA + a0, srcB + b0, dstB + b0, cin, cout);
    in[i] = cin[0]; in[(u64)n + 2 * i] = cin[1]; in[(u64)n + 2 * i + 1] = cin[2];
    out[2 * i] = cout[0]; out[2 * i + 1] = cout[1];
    if (i + 1 == n) { srcA[a1] = cA[n]; dstA[a1] = dstA[a1 - 1]; srcB[fB[n]] = cA[n] + cB[n]; dstB[fB[n]] = eB[n]; }
}
// The bandwidth kernel: workgroup t moves what lies in tile t of the runs' key space.  keyIsDst: the key is the destination offset (source -> compact bytes),
// otherwise the source offset (edge scratch -> the caller's slots).  16 aligned bytes per lane where both residues agree, else two 8-byte words; bytes at the ends.
__global__ __launch_bounds__(256) void zj_range_gather_kernel(const ZRCopy* __restrict__ runs, u64 D, const u8* __restrict__ srcBase, u8* __restrict__ dstBase, u32 keyIsDst, u64 keyEnd) {
    u64 const tLo = (u64)blockIdx.x * ZJ_RANGE_TILE, tHi = tLo + ZJ_RANGE_TILE < keyEnd ? tLo + ZJ_RANGE_TILE : keyEnd;
    u32 const t = threadIdx.x;
    for (u64 d = zj_range_tile_first(runs, D, tLo); d < D; d++) {
        ZRCopy const c = runs[d];
        if (c.key >= tHi) break;
        u64 at = 0;
        u64 const len = zj_range_tile_part(c, tLo, tHi, &at);
        if (!len) continue;
        const u8* const s = srcBase + (keyIsDst ? c.other : c.key) + at;
        u8* const dd = dstBase + (keyIsDst ? c.key : c.other) + at;
        ZRPlan const pl = zj_range_copy_plan((u64)(uintptr_t)s, (u64)(uintptr_t)dd, len);
        if (t < pl.head) dd[t] = s[t];
        const u8* const sb = s + pl.head; u8* const db = dd + pl.head;
        if (pl.wide) for (u64 k = t; k < pl.body; k += 256) ((uint4*)db)[k] = ((const uint4*)sb)[k];
        else for (u64 k = t; k < pl.body; k += 256) { u64 const a = ld64(sb + 16 * k), b = ld64(sb + 16 * k + 8); st64(db + 16 * k, a); st64(db + 16 * k + 8, b); }
        if (t < pl.tail) db[(pl.body << 4) + t] = sb[(pl.body << 4) + t];
    }
}
// The finish loop of both range entries.  One wave per buffer (or request): the first error over its entries in frame order (edge first, interiors, edge last),
// the result, the stats (stat[P::kStat .. + 4)); a buffer with an error gets its edge runs emptied, so the gather behind the kernel copies nothing for it.
// The policy P says what a buffer starts with (initial), and what an entry's answer counts as, 0 or an error (edge: first or last; interior: the k-th).
extern "C++" { template <class P>      // (a template cannot have C linkage)
__device__ __forceinline__ void zj_range_finish_body(const P& p, const ZRRec* __restrict__ rec, const u64* __restrict__ scan, const u64* __restrict__ resA, const u64* __restrict__ resB,
                                                     u64* __restrict__ result, u32 n, ZRCopy* __restrict__ out, u32* stat) {
    u32 const lane = threadIdx.x;
    for (u32 i = blockIdx.x; i < n; i += gridDim.x) {
        u32 const status = rec[i].status, e = rec[i].edges, frames = rec[i].frames;
        if (status != ZJ_RANGE_SELECTED) {
            if (lane == 0) { result[i] = status == ZJ_RANGE_NOTHING ? 0 : ZJ_ERR64(status); atomicAdd(&stat[P::kStat + (status == ZJ_RANGE_NOTHING ? 0 : 3)], 1u); }
            continue;
        }
        u64 const a0 = scan[i], m = scan[i + 1] - a0 - 1u, b0 = scan[(u64)n + 1u + i];
        u64 err = p.initial(i);
        if (!err && (e & 1u)) err = p.edge(i, resB[b0], false);
        for (u64 base = 0; base < m && !err; base += 64) {
            u64 const k = base + lane;
            u64 const v = k < m ? p.interior(i, k, resA[a0 + k]) : 0;
            unsigned long long const mask = __ballot(v != 0);
            if (mask) err = __shfl(v, (int)(__ffsll((long long)mask) - 1), 64);
        }
        if (!err && (e & 2u)) err = p.edge(i, resB[b0 + (e & 1u)], true);
        if (lane == 0) {
            result[i] = err ? err : rec[i].hi - rec[i].lo;
            if (err) { out[2 * (u64)i].len = 0; out[2 * (u64)i + 1].len = 0; }
            atomicAdd(&stat[P::kStat + (err ? 3 : 0)], 1u); atomicAdd(&stat[P::kStat + 1], frames); atomicAdd(&stat[P::kStat + 2], zj_range_edge_count(e));
        }
    }
} }
// the walked entry: an entry counts as the pipeline answered it
struct ZRFinishWalked {
    static constexpr u32 kStat = 4;
    __device__ u64 initial(u32) const { return 0; }
    __device__ u64 edge(u32, u64 v, bool) const { return v > ((u64)1 << 40) ? v : 0; }
    __device__ u64 interior(u32, u64, u64 v) const { return v > ((u64)1 << 40) ? v : 0; }
};
__global__ __launch_bounds__(64) void zj_range_finish_kernel(const ZRRec* __restrict__ rec, const u64* __restrict__ scan, const u64* __restrict__ resA, const u64* __restrict__ resB,
                                                             u64* __restrict__ result, u32 n, ZRCopy* __restrict__ out, u32* stat) {
    zj_range_finish_body(ZRFinishWalked{}, rec, scan, resA, resB, result, n, out, stat);
}
// The tail of both range entries.  In front of it the entry has laid out framesBuf's first `head` bytes (its per-buffer or per-request arrays, the five totals at
// oTot) and launched its count (or request) kernel and zj_range_scan_kernel over `count` buffers (or requests).
struct RangePlan {
    u64 EA, EB, CA, CB, SB;          // entries of set A, of set B, compact source bytes of A, of B, scratch bytes of the edge frames
    // per entry and per run: [srcA EA + 1][dstA EA + 1][resA EA][srcB EB + 1][dstB EB + 1][resB EB][in 3 x count][out 2 x count][compact bytes CA + CB][edge scratch SB]
    size_t oSrcA, oDstA, oResA, oSrcB, oDstB, oResB, oIn, oOut, oComp, oEdge, total;
};
static u64 range_tiles(u64 bytes) { return (bytes + ZJ_RANGE_TILE - 1) / ZJ_RANGE_TILE; }
// the entry's only host wait (the five totals in one copy of 40 bytes: the pipelines size their launches on the host), their checks, the layout, and room for it
static size_t range_plan_read(DevState* d, size_t oTot, size_t count, size_t head, hipStream_t st, RangePlan& p) {
    u64 t[5];
    size_t const r = frames_read_total(d, (const u64*)(d->framesBuf + oTot), 5, st, t);
    if (r != 0) return r;
    p.EA = t[0]; p.EB = t[1]; p.CA = t[2]; p.CB = t[3]; p.SB = t[4];
    if (p.EA > 0xFFFFFFFFull) return ZJNI_ERR(72);
    if (p.EA < count || p.EB > 2 * (u64)count) return ZJNI_ERR(ZJNI_ERROR_no_device);          // (every buffer has its closing entry and at most two edges)
    p.oSrcA = head; p.oDstA = p.oSrcA + zj_up16((p.EA + 1) * 8); p.oResA = p.oDstA + zj_up16((p.EA + 1) * 8); p.oSrcB = p.oResA + zj_up16(p.EA * 8 + 8);
    p.oDstB = p.oSrcB + zj_up16((p.EB + 1) * 8); p.oResB = p.oDstB + zj_up16((p.EB + 1) * 8); p.oIn = p.oResB + zj_up16(p.EB * 8 + 8);
    p.oOut = p.oIn + zj_up16(3 * count * sizeof(ZRCopy)); p.oComp = p.oOut + zj_up16(2 * count * sizeof(ZRCopy));
    p.oEdge = p.oComp + zj_up16(p.CA + p.CB) + 16; p.total = p.oEdge + zj_up16(p.SB) + 16;
    if (p.CA + p.CB < p.CA || p.total < p.oComp || p.total < p.SB) return ZJNI_ERR(64);
    return frames_room(d, p.total, head, st);
}
// behind the entry's emit launches: the selected source bytes into the compact area (3 x count runs), then the pipelines over set A (into the caller's slots) and
// set B (into the edge scratch)
static size_t range_plan_decode(DevState* d, const RangePlan& p, size_t count, const void* d_src, void* d_dst, const zjni_ddict* ddict, void* stream) {
    u8* const fb = d->framesBuf;
    u64 const tilesIn = range_tiles(p.CA + p.CB);
    if (tilesIn > 0x7FFFFFFFull || range_tiles(p.SB) > 0x7FFFFFFFull) return ZJNI_ERR(64);
    if (tilesIn) hipLaunchKernelGGL(zj_range_gather_kernel, dim3((u32)tilesIn), dim3(256), 0, (hipStream_t)stream, (const ZRCopy*)(fb + p.oIn), (u64)(3 * count), (const u8*)d_src, fb + p.oComp, 1u, p.CA + p.CB);
    if (hipGetLastError() != hipSuccess) return ZJNI_ERR(ZJNI_ERROR_no_device);
    size_t r = 0;
    // (a call with no interior frame has nothing but closing entries in set A: no launch)
    if (p.EA > count && (r = decompress_chunked_ordered(fb + p.oComp, (const u64*)(fb + p.oSrcA), d_dst, (const u64*)(fb + p.oDstA), (u64*)(fb + p.oResA), (size_t)p.EA, ddict, stream)) != 0) return r;
    if (p.EB && (r = decompress_chunked_ordered(fb + p.oComp, (const u64*)(fb + p.oSrcB), fb + p.oEdge, (const u64*)(fb + p.oDstB), (u64*)(fb + p.oResB), (size_t)p.EB, ddict, stream)) != 0) return r;
    return 0;
}
// behind the entry's finish launch: the edge frames' bytes from the scratch into the caller's slots (2 x count runs)
static size_t range_plan_scatter(DevState* d, const RangePlan& p, size_t count, void* d_dst, hipStream_t st) {
    u64 const tilesOut = range_tiles(p.SB);
    if (tilesOut) hipLaunchKernelGGL(zj_range_gather_kernel, dim3((u32)tilesOut), dim3(256), 0, st, (const ZRCopy*)(d->framesBuf + p.oOut), (u64)(2 * count), (const u8*)(d->framesBuf + p.oEdge), (u8*)d_dst, 0u, p.SB);
    return hipGetLastError() == hipSuccess ? 0 : ZJNI_ERR(ZJNI_ERROR_no_device);
}
size_t zjni_decompress_frames_range_batch_device(const void* d_src, const uint64_t* d_src_off, void* d_dst, const uint64_t* d_dst_off, const uint64_t* d_range,
                                                 uint64_t* d_result, uint64_t* d_total, size_t n, const zjni_ddict* ddict, void* stream) {
    if (ddict && !dict_on_this_device(ddict->ordinal)) return ZJNI_ERR(32);
    DevState* d = cur_state();
    if (!d) return ZJNI_ERR(ZJNI_ERROR_no_device);
    if (n > 0xFFFFFFFFull) return ZJNI_ERR(72);
    hipStream_t const st = (hipStream_t)stream;
    BatchOrder order(d, stream);
    if (!frames_state(d)) return ZJNI_ERR(64);
    if (hipMemsetAsync(d->framesStat + 4, 0, 16, st) != hipSuccess) return ZJNI_ERR(ZJNI_ERROR_no_device);
    if (n == 0) return 0;
    size_t const oRec = 0, oQ = zj_up16(n * sizeof(ZRRec)), oScan = oQ + zj_up16(5 * n * 8), oTot = oScan + zj_up16(5 * (n + 1) * 8), perBuf = oTot + 64;
    size_t r = frames_room(d, perBuf, 0, st);
    if (r != 0) return r;
    u32 const gridN = (u32)((n + 63) / 64);
    hipLaunchKernelGGL(zj_range_count_kernel, dim3(gridN), dim3(64), 0, st, (const u8*)d_src, (const u64*)d_src_off, (const u64*)d_dst_off, (const u64*)d_range,
                       (ZRRec*)(d->framesBuf + oRec), (u64*)(d->framesBuf + oQ), (u64*)d_total, (u32)n);
    hipLaunchKernelGGL(zj_range_scan_kernel, dim3(5), dim3(1024), 0, st, (const u64*)(d->framesBuf + oQ), (u64*)(d->framesBuf + oScan), (u64*)(d->framesBuf + oTot), (u32)n);
    RangePlan p;
    if ((r = range_plan_read(d, oTot, n, perBuf, st, p)) != 0) return r;
    u8* const fb = d->framesBuf;
    hipLaunchKernelGGL(zj_range_emit_kernel, dim3(gridN), dim3(64), 0, st, (const u8*)d_src, (const u64*)d_src_off, (const u64*)d_dst_off, (const ZRRec*)(fb + oRec),
                       (const u64*)(fb + oScan), (u32)n, (u64*)(fb + p.oSrcA), (u64*)(fb + p.oDstA), (u64*)(fb + p.oSrcB), (u64*)(fb + p.oDstB), (ZRCopy*)(fb + p.oIn), (ZRCopy*)(fb + p.oOut));
    if ((r = range_plan_decode(d, p, n, d_src, d_dst, ddict, stream)) != 0) return r;
    hipLaunchKernelGGL(zj_range_finish_kernel, dim3(grid_cap(d, n)), dim3(64), 0, st, (const ZRRec*)(fb + oRec), (const u64*)(fb + oScan), (const u64*)(fb + p.oResA), (const u64*)(fb + p.oResB),
                       (u64*)d_result, (u32)n, (ZRCopy*)(fb + p.oOut), d->framesStat);
    return range_plan_scatter(d, p, n, d_dst, st);
}
int zjni_last_frames_range(unsigned* out4) { return frames_stat_get(4, out4); }

// ---- range reads by a caller-held index (zj_index.h) ----
// The request kernel stands where zj_range_count_kernel stands, zj_range_scan_kernel runs with n := R, the entries of set A are written one lane each, and
// zj_range_emit itself (with no interior entry to walk) writes set B and the copy runs of a request.
size_t zjni_index_bytes(size_t n, size_t E) { return (size_t)zj_index_bytes(n, E); }
// One wave per buffer: lanes stride its entries, a wave-wide AND gives valid[i] (zj_pieces_count_kernel's shape).
__global__ __launch_bounds__(64) void zj_index_buffers_kernel(const u64* __restrict__ first, const u64* __restrict__ size, const u64* __restrict__ content, const u64* __restrict__ result,
                                                              u32 n, u64 E, u64* __restrict__ valid) {
    u32 const lane = threadIdx.x;
    for (u32 i = blockIdx.x; i < n; i += gridDim.x) {
        bool ok = zj_index_first_ok(first, i, E);
        u64 const f0 = first[i], f1 = first[i + 1];
        for (u64 e = f0 + lane; ok && e < f1; e += 64) ok = size[e] <= ZJ_INDEX_SIZE_MAX && content[e] <= ZJ_INDEX_SIZE_MAX;
        ok = __ballot(!ok) == 0ull;
        if (lane == 0) valid[i] = zj_index_valid(ok, result, i);
    }
}
// workgroup 0: C[0 .. E] = exclusive prefix sums of the compressed sizes; workgroup 1: U of the content sizes (zj_range_scan_kernel's shape, E items)
__global__ __launch_bounds__(ZJ_INDEX_SCAN_WG) void zj_index_scan_kernel(const u64* __restrict__ size, const u64* __restrict__ content, u64 E, u64* __restrict__ C, u64* __restrict__ U) {
    __shared__ u64 part[ZJ_INDEX_SCAN_WG];
    u32 const t = threadIdx.x;
    const u64* const in = blockIdx.x ? content : size;
    u64* const out = blockIdx.x ? U : C;
    u64 const per = (E + ZJ_INDEX_SCAN_WG - 1u) / ZJ_INDEX_SCAN_WG, lo0 = (u64)t * per, lo = lo0 < E ? lo0 : E, hi = lo + per < E ? lo + per : E;
    u64 sum = 0;
    for (u64 i = lo; i < hi; i++) sum += zj_index_term(in[i]);
    part[t] = sum;
    __syncthreads();
    for (u32 d = 1; d < ZJ_INDEX_SCAN_WG; d <<= 1) {
        u64 const v = t >= d ? part[t - d] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    u64 run = t ? part[t - 1] : 0;
    for (u64 i = lo; i < hi; i++) { out[i] = run; run += zj_index_term(in[i]); }
    if (t == ZJ_INDEX_SCAN_WG - 1u) out[E] = part[ZJ_INDEX_SCAN_WG - 1u];
}
// one lane per entry: the content size of a piece from the cuts (or the fixed grid) its compress call took; an entry no buffer owns counts nothing
__global__ __launch_bounds__(256) void zj_index_content_kernel(const u64* __restrict__ off, const u64* __restrict__ first, u32 n, u64 E, u64 chunk, const u64* __restrict__ cut,
                                                               const u64* __restrict__ cutOff, u64* __restrict__ content) {
    u64 const e = (u64)blockIdx.x * 256u + threadIdx.x;
    if (e >= E) return;
    content[e] = 0;
    if (!n) return;
    u64 const i = zj_entry_owner(first, n, e), f0 = first[i];
    if (e < f0 || e >= first[i + 1]) return;
    u64 const lo = off[i], hi = off[i + 1], size = hi > lo ? hi - lo : 0;
    const u64* list = nullptr; u64 c = 0;
    if (cut) { u64 const c0 = cutOff[i], c1 = cutOff[i + 1]; c = c1 > c0 ? c1 - c0 : 0; list = cut + c0; }
    content[e] = zj_index_piece_content(size, chunk, list, c, e - f0);
}
// (the caller holds the device's BatchOrder)
static size_t index_build_ordered(DevState* d, size_t n, const u64* d_first, const u64* d_size, const u64* d_content, const u64* d_result, size_t E, u64* d_index, hipStream_t st) {
    u64* const first = d_index; u64* const valid = d_index + n + 1; u64* const C = d_index + 2 * n + 1; u64* const U = C + E + 1;
    if (hipMemcpyAsync(first, d_first, (n + 1) * 8, hipMemcpyDeviceToDevice, st) != hipSuccess) return ZJNI_ERR(ZJNI_ERROR_no_device);
    if (n) hipLaunchKernelGGL(zj_index_buffers_kernel, dim3(grid_cap(d, n)), dim3(64), 0, st, d_first, d_size, d_content, d_result, (u32)n, (u64)E, valid);
    hipLaunchKernelGGL(zj_index_scan_kernel, dim3(2), dim3(ZJ_INDEX_SCAN_WG), 0, st, d_size, d_content, (u64)E, C, U);
    return hipGetLastError() == hipSuccess ? 0 : ZJNI_ERR(ZJNI_ERROR_no_device);
}
size_t zjni_index_from_sizes_device(size_t n, const uint64_t* d_piece_first, const uint64_t* d_piece_size, const uint64_t* d_piece_content, size_t E, void* d_index, void* stream) {
    DevState* d = cur_state();
    if (!d) return ZJNI_ERR(ZJNI_ERROR_no_device);
    if (n > 0xFFFFFFFFull || E > 0xFFFFFFFFull) return ZJNI_ERR(72);
    if (!d_index || !d_piece_first || (E && (!d_piece_size || !d_piece_content))) return ZJNI_ERR(42);
    BatchOrder order(d, stream);
    return index_build_ordered(d, n, (const u64*)d_piece_first, (const u64*)d_piece_size, (const u64*)d_piece_content, nullptr, E, (u64*)d_index, (hipStream_t)stream);
}
size_t zjni_index_from_pieces_device(const uint64_t* d_src_off, size_t n, size_t chunkSize, const uint64_t* d_cut, const uint64_t* d_cut_off, const uint64_t* d_result,
                                     const uint64_t* d_piece_first, const uint64_t* d_piece_size, size_t E, void* d_index, void* stream) {
    DevState* d = cur_state();
    if (!d) return ZJNI_ERR(ZJNI_ERROR_no_device);
    if (n > 0xFFFFFFFFull || E > 0xFFFFFFFFull) return ZJNI_ERR(72);
    if (chunkSize < 256 || chunkSize > ZJNI_BLOCKSIZE_MAX || (d_cut && !d_cut_off)) return ZJNI_ERR(42);
    if (!d_index || !d_piece_first || (n && !d_src_off) || (E && !d_piece_size)) return ZJNI_ERR(42);
    hipStream_t const st = (hipStream_t)stream;
    BatchOrder order(d, stream);
    if (!frames_state(d)) return ZJNI_ERR(64);
    size_t const r = frames_room(d, zj_up16(E * 8) + 16, 0, st);           // the content sizes, until the scan behind them has run (stream order)
    if (r != 0) return r;
    u64* const content = (u64*)d->framesBuf;
    if (E) hipLaunchKernelGGL(zj_index_content_kernel, dim3((u32)((E + 255) / 256)), dim3(256), 0, st, (const u64*)d_src_off, (const u64*)d_piece_first, (u32)n, (u64)E, (u64)chunkSize,
                              (const u64*)d_cut, (const u64*)d_cut_off, content);
    return index_build_ordered(d, n, (const u64*)d_piece_first, (const u64*)d_piece_size, content, (const u64*)d_result, E, (u64*)d_index, st);
}

// ---- the index from the frames alone: two walks over the headers with a scan between them, as the frames layer counts and emits ----
// first walk, one lane per buffer as zj_frames_count_kernel walks: cnt[i] = entries of buffer i (0: empty, or not indexable)
__global__ __launch_bounds__(64) void zj_index_walk_count_kernel(const u8* __restrict__ src, const u64* __restrict__ off, u64* __restrict__ cnt, u32 n) {
    u64 const i = (u64)blockIdx.x * 64u + threadIdx.x;
    if (i >= n) return;
    u64 const lo = off[i], hi = off[i + 1];
    u64 entries, wrote;
    (void)zj_index_walk(src + lo, hi > lo ? hi - lo : 0, 0, nullptr, nullptr, &entries, &wrote);
    cnt[i] = entries;
}
// second walk: the sizes of buffer i at first[i], inside its own extent of the E entries, and valid[i]
__global__ __launch_bounds__(64) void zj_index_walk_emit_kernel(const u8* __restrict__ src, const u64* __restrict__ off, const u64* __restrict__ first, u32 n, u64 E,
                                                                u64* __restrict__ size, u64* __restrict__ content, u64* __restrict__ valid) {
    u64 const i = (u64)blockIdx.x * 64u + threadIdx.x;
    if (i >= n) return;
    u64 const lo = off[i], hi = off[i + 1];
    valid[i] = zj_index_frames_emit(src + lo, hi > lo ? hi - lo : 0, first, i, E, size, content);
}
size_t zjni_index_count_frames_device(const void* d_src, const uint64_t* d_src_off, size_t n, uint64_t* d_piece_first, void* stream) {
    DevState* d = cur_state();
    if (!d) return ZJNI_ERR(ZJNI_ERROR_no_device);
    if (n > 0xFFFFFFFFull) return ZJNI_ERR(72);
    if (!d_piece_first || (n && !d_src_off)) return ZJNI_ERR(42);
    hipStream_t const st = (hipStream_t)stream;
    BatchOrder order(d, stream);
    if (n == 0) return hipMemsetAsync(d_piece_first, 0, 8, st) == hipSuccess ? 0 : ZJNI_ERR(ZJNI_ERROR_no_device);
    if (!frames_state(d)) return ZJNI_ERR(64);
    size_t const r = frames_room(d, zj_up16(n * 8) + 16, 0, st);           // the counts, until the scan behind them has run (stream order)
    if (r != 0) return r;
    u64* const cnt = (u64*)d->framesBuf;
    hipLaunchKernelGGL(zj_index_walk_count_kernel, dim3((u32)((n + 63) / 64)), dim3(64), 0, st, (const u8*)d_src, (const u64*)d_src_off, cnt, (u32)n);
    hipLaunchKernelGGL(zj_pack_offsets_kernel, dim3(1), dim3(1024), 0, st, (const u64*)cnt, (u64*)d_piece_first, (u32)n);
    return hipGetLastError() == hipSuccess ? 0 : ZJNI_ERR(ZJNI_ERROR_no_device);
}
size_t zjni_index_from_frames_device(const void* d_src, const uint64_t* d_src_off, size_t n, const uint64_t* d_piece_first, size_t E, void* d_index,
                                     uint64_t* d_piece_size, uint64_t* d_piece_content, void* stream) {
    DevState* d = cur_state();
    if (!d) return ZJNI_ERR(ZJNI_ERROR_no_device);
    if (n > 0xFFFFFFFFull || E > 0xFFFFFFFFull) return ZJNI_ERR(72);
    if (!d_index || !d_piece_first || (n && !d_src_off)) return ZJNI_ERR(42);
    hipStream_t const st = (hipStream_t)stream;
    BatchOrder order(d, stream);
    u64* const idx = (u64*)d_index;
    u64* const valid = idx + n + 1; u64* const C = idx + 2 * n + 1; u64* const U = C + E + 1;
    // the two arrays the walk writes and the scan reads: the caller's, or library scratch until the scan has run (stream order)
    size_t const arr = zj_up16(E * 8) + 16;
    u64* size = (u64*)d_piece_size; u64* content = (u64*)d_piece_content;
    if (E && (!size || !content)) {
        if (!frames_state(d)) return ZJNI_ERR(64);
        size_t const r = frames_room(d, 2 * arr, 0, st);
        if (r != 0) return r;
        if (!size) size = (u64*)d->framesBuf;
        if (!content) content = (u64*)(d->framesBuf + arr);
    }
    if (hipMemcpyAsync(idx, d_piece_first, (n + 1) * 8, hipMemcpyDeviceToDevice, st) != hipSuccess) return ZJNI_ERR(ZJNI_ERROR_no_device);
    // (an entry no buffer owns, which only a false d_piece_first leaves, counts nothing)
    if (E && (hipMemsetAsync(size, 0, E * 8, st) != hipSuccess || hipMemsetAsync(content, 0, E * 8, st) != hipSuccess)) return ZJNI_ERR(ZJNI_ERROR_no_device);
    if (n) hipLaunchKernelGGL(zj_index_walk_emit_kernel, dim3((u32)((n + 63) / 64)), dim3(64), 0, st, (const u8*)d_src, (const u64*)d_src_off, (const u64*)d_piece_first, (u32)n, (u64)E,
                              size, content, valid);
    hipLaunchKernelGGL(zj_index_scan_kernel, dim3(2), dim3(ZJ_INDEX_SCAN_WG), 0, st, (const u64*)size, (const u64*)content, (u64)E, C, U);
    return hipGetLastError() == hipSuccess ? 0 : ZJNI_ERR(ZJNI_ERROR_no_device);
}

// per request: [rec R][ireq R][bad R][q 5 x R][scan 5 x (R + 1)][totals 5] — the range layer's, with the request's place in the index and its mark beside the record
// one lane per request: rules 1-4 by bisection
__global__ __launch_bounds__(64) void zj_index_request_kernel(const u64* __restrict__ idx, u64 n, u64 E, const u64* __restrict__ off, const u64* __restrict__ req, const u64* __restrict__ dstOff,
                                                              ZRRec* __restrict__ rec, ZIReq* __restrict__ ireq, u32* __restrict__ bad, u64* __restrict__ q, u64* __restrict__ total, u32 R) {
    u64 const i = (u64)blockIdx.x * 64u + threadIdx.x;
    if (i >= R) return;
    u64 const dlo = dstOff[i], dhi = dstOff[i + 1];
    ZRRec r; ZIReq ir; u64 qq[5];
    zj_index_request(idx, n, E, off, req[3 * i], req[3 * i + 1], req[3 * i + 2], dhi > dlo ? dhi - dlo : 0, r, ir, qq);
    rec[i] = r; ireq[i] = ir; bad[i] = 0;
    for (u32 k = 0; k < 5; k++) q[(u64)k * R + i] = qq[k];
    if (total) total[i] = r.total;
}
// one lane per entry of set A: an interior entry whose sums do not ascend inside its request's run marks the request
__global__ __launch_bounds__(ZJ_INDEX_EMIT_WG) void zj_index_check_kernel(const u64* __restrict__ idx, u64 n, u64 E, const ZRRec* __restrict__ rec, const ZIReq* __restrict__ ireq,
                                                                          const u64* __restrict__ fA, u32 R, u64 EA, u32* __restrict__ bad) {
    u64 const g = (u64)blockIdx.x * ZJ_INDEX_EMIT_WG + threadIdx.x;
    if (g >= EA) return;
    u64 const r = zj_entry_owner(fA, R, g), j = g - fA[r], m = fA[r + 1] - fA[r] - 1u;
    if (j >= m || rec[r].status != ZJ_RANGE_SELECTED) return;
    ZIView const v = zj_index_view(idx, n, E);
    if (!zj_index_entry_ok(v.C, v.U, rec[r], ireq[r], j)) bad[r] = 1u;
}
// one lane per entry of set A, the closing entries included: the owner by bisection over the scanned counts, the offsets from C and U alone
__global__ __launch_bounds__(ZJ_INDEX_EMIT_WG) void zj_index_emit_kernel(const u64* __restrict__ idx, u64 n, u64 E, const ZRRec* __restrict__ rec, const ZIReq* __restrict__ ireq,
                                                                         const u32* __restrict__ bad, const u64* __restrict__ scan, const u64* __restrict__ dstOff, u32 R, u64 EA,
                                                                         u64* __restrict__ srcA, u64* __restrict__ dstA) {
    u64 const g = (u64)blockIdx.x * ZJ_INDEX_EMIT_WG + threadIdx.x;
    if (g >= EA) return;
    const u64* const fA = scan; const u64* const cA = scan + 2 * ((u64)R + 1u);
    u64 const r = zj_entry_owner(fA, R, g);
    ZIView const v = zj_index_view(idx, n, E);
    u64 s, dd;
    zj_index_entry(v.C, v.U, rec[r], ireq[r], bad[r] != 0u, g - fA[r], cA[r], dstOff[r], &s, &dd);
    srcA[g] = s; dstA[g] = dd;
}
// one lane per request, behind the emit kernel: set B and the copy runs as zj_range_emit writes them for a buffer with no interior entry to walk; the lane of the
// last request closes the arrays
__global__ __launch_bounds__(64) void zj_index_edges_kernel(const ZRRec* __restrict__ rec, const ZIReq* __restrict__ ireq, const u64* __restrict__ scan, const u64* __restrict__ dstOff, u32 R,
                                                            u64* __restrict__ srcA, u64* __restrict__ dstA, u64* __restrict__ srcB, u64* __restrict__ dstB,
                                                            ZRCopy* __restrict__ in, ZRCopy* __restrict__ out) {
    u64 const i = (u64)blockIdx.x * 64u + threadIdx.x;
    if (i >= R) return;
    u64 const n1 = (u64)R + 1u;
    const u64* const fA = scan; const u64* const fB = scan + n1; const u64* const cA = scan + 2 * n1; const u64* const cB = scan + 3 * n1; const u64* const eB = scan + 4 * n1;
    u64 const a1 = fA[i + 1], b0 = fB[i];
    ZRRec const r = rec[i];
    ZRCopy cin[3], cout[2];
    u64 closeSrc, closeDst;
    zj_range_emit(nullptr, 0, r, ireq[i].srcLo, dstOff[i], 0u, cA[i], cA[R] + cB[i], eB[i], &closeSrc, &closeDst, srcB + b0, dstB + b0, cin, cout);
    in[i] = cin[0]; in[(u64)R + 2 * i] = cin[1]; in[(u64)R + 2 * i + 1] = cin[2];
    out[2 * i] = cout[0]; out[2 * i + 1] = cout[1];
    if (i + 1 == R) { srcA[a1] = cA[R]; dstA[a1] = dstA[a1 - 1]; srcB[fB[R]] = cA[R] + cB[R]; dstB[fB[R]] = eB[R]; }
}
// The indexed entry's finish (zj_range_finish_body), with one rule more than the walked one: an entry that decoded without error to another size than the index
// says answers 20, as does a request an entry marked.
struct ZRFinishIndexed {
    static constexpr u32 kStat = 8;
    const ZRRec* rec; const ZIReq* ireq; const u32* bad; const u64* U;
    __device__ u64 initial(u32 i) const { return bad[i] ? ZJ_ERR64(ZJ_E_CORRUPTION) : 0; }
    __device__ u64 edge(u32 i, u64 v, bool last) const { return zj_index_verdict(v, last ? rec[i].fcsL : rec[i].fcsF); }
    __device__ u64 interior(u32 i, u64 k, u64 v) const { u64 const e = ireq[i].e0 + k; return zj_index_verdict(v, U[e + 1] - U[e]); }
};
__global__ __launch_bounds__(64) void zj_index_finish_kernel(const u64* __restrict__ idx, u64 n, u64 E, const ZRRec* __restrict__ rec, const ZIReq* __restrict__ ireq, const u32* __restrict__ bad,
                                                             const u64* __restrict__ scan, const u64* __restrict__ resA, const u64* __restrict__ resB,
                                                             u64* __restrict__ result, u32 R, ZRCopy* __restrict__ out, u32* stat) {
    zj_range_finish_body(ZRFinishIndexed{rec, ireq, bad, zj_index_view(idx, n, E).U}, rec, scan, resA, resB, result, R, out, stat);
}
size_t zjni_decompress_index_range_batch_device(const void* d_src, const uint64_t* d_src_off, size_t n, const void* d_index, size_t E, const uint64_t* d_req,
                                                void* d_dst, const uint64_t* d_dst_off, uint64_t* d_result, uint64_t* d_total, size_t R,
                                                const zjni_ddict* ddict, void* stream) {
    if (ddict && !dict_on_this_device(ddict->ordinal)) return ZJNI_ERR(32);
    DevState* d = cur_state();
    if (!d) return ZJNI_ERR(ZJNI_ERROR_no_device);
    if (n > 0xFFFFFFFFull || E > 0xFFFFFFFFull || R > 0xFFFFFFFFull) return ZJNI_ERR(72);
    hipStream_t const st = (hipStream_t)stream;
    BatchOrder order(d, stream);
    if (!frames_state(d)) return ZJNI_ERR(64);
    if (hipMemsetAsync(d->framesStat + 8, 0, 16, st) != hipSuccess) return ZJNI_ERR(ZJNI_ERROR_no_device);
    if (R == 0) return 0;
    if (!d_index) return ZJNI_ERR(42);
    const u64* const idx = (const u64*)d_index;
    size_t const oRec = 0, oReq = zj_up16(R * sizeof(ZRRec)), oBad = oReq + zj_up16(R * sizeof(ZIReq)), oQ = oBad + zj_up16(R * 4), oScan = oQ + zj_up16(5 * R * 8),
                 oTot = oScan + zj_up16(5 * (R + 1) * 8), perReq = oTot + 64;
    size_t r = frames_room(d, perReq, 0, st);
    if (r != 0) return r;
    u32 const gridR = (u32)((R + 63) / 64);
    hipLaunchKernelGGL(zj_index_request_kernel, dim3(gridR), dim3(64), 0, st, idx, (u64)n, (u64)E, (const u64*)d_src_off, (const u64*)d_req, (const u64*)d_dst_off,
                       (ZRRec*)(d->framesBuf + oRec), (ZIReq*)(d->framesBuf + oReq), (u32*)(d->framesBuf + oBad), (u64*)(d->framesBuf + oQ), (u64*)d_total, (u32)R);
    hipLaunchKernelGGL(zj_range_scan_kernel, dim3(5), dim3(1024), 0, st, (const u64*)(d->framesBuf + oQ), (u64*)(d->framesBuf + oScan), (u64*)(d->framesBuf + oTot), (u32)R);
    RangePlan p;
    if ((r = range_plan_read(d, oTot, R, perReq, st, p)) != 0) return r;
    u8* const fb = d->framesBuf;
    const ZRRec* const rec = (const ZRRec*)(fb + oRec); const ZIReq* const ireq = (const ZIReq*)(fb + oReq); u32* const bad = (u32*)(fb + oBad);
    const u64* const scan = (const u64*)(fb + oScan);
    u32 const gridA = (u32)((p.EA + ZJ_INDEX_EMIT_WG - 1u) / ZJ_INDEX_EMIT_WG);
    if (p.EA > R) hipLaunchKernelGGL(zj_index_check_kernel, dim3(gridA), dim3(ZJ_INDEX_EMIT_WG), 0, st, idx, (u64)n, (u64)E, rec, ireq, scan, (u32)R, p.EA, bad);
    hipLaunchKernelGGL(zj_index_emit_kernel, dim3(gridA), dim3(ZJ_INDEX_EMIT_WG), 0, st, idx, (u64)n, (u64)E, rec, ireq, (const u32*)bad, scan, (const u64*)d_dst_off, (u32)R, p.EA,
                       (u64*)(fb + p.oSrcA), (u64*)(fb + p.oDstA));
    hipLaunchKernelGGL(zj_index_edges_kernel, dim3(gridR), dim3(64), 0, st, rec, ireq, scan, (const u64*)d_dst_off, (u32)R, (u64*)(fb + p.oSrcA), (u64*)(fb + p.oDstA),
                       (u64*)(fb + p.oSrcB), (u64*)(fb + p.oDstB), (ZRCopy*)(fb + p.oIn), (ZRCopy*)(fb + p.oOut));
    if ((r = range_plan_decode(d, p, R, d_src, d_dst, ddict, stream)) != 0) return r;
    hipLaunchKernelGGL(zj_index_finish_kernel, dim3(grid_cap(d, R)), dim3(64), 0, st, idx, (u64)n, (u64)E, rec, ireq, (const u32*)bad, scan, (const u64*)(fb + p.oResA), (const u64*)(fb + p.oResB),
                       (u64*)d_result, (u32)R, (ZRCopy*)(fb + p.oOut), d->framesStat);
    return range_plan_scatter(d, p, R, d_dst, st);
}
int zjni_last_index_range(unsigned* out4) { return frames_stat_get(8, out4); }

// ---- chunked compress ----
size_t zjni_compressBound_chunked(size_t srcSize, size_t chunkSize) {
    if (chunkSize < 256 || chunkSize > ZJNI_BLOCKSIZE_MAX) return ZJNI_ERR(42);
    return (size_t)zj_chunk_bound_total(srcSize, chunkSize);
}
// one lane per buffer: its pieces and what their scratch destinations take
__global__ __launch_bounds__(256) void zj_chunks_count_kernel(const u64* __restrict__ off, u32 n, u64 chunk, u64* __restrict__ cnt, u64* __restrict__ btot) {
    u64 const i = (u64)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    u64 const lo = off[i], hi = off[i + 1], size = hi > lo ? hi - lo : 0;
    cnt[i] = zj_chunk_count(size, chunk);
    btot[i] = zj_chunk_bound_total(size, chunk);
}
// one lane per entry of the slice [a, a + m], its end included: where the piece begins in the source, and in the slice's scratch (relative to the slice's first)
__global__ __launch_bounds__(256) void zj_chunks_emit_kernel(const u64* __restrict__ off, const u64* __restrict__ first, const u64* __restrict__ bbase, u32 n, u64 chunk,
                                                             u64 a, u32 m, u64 E, u64* __restrict__ srcOffS, u64* __restrict__ dstOffS) {
    u64 const j = (u64)blockIdx.x * 256u + threadIdx.x;
    if (j > m) return;
    u64 const ia = zj_entry_owner(first, n, a), dstA = zj_chunk_dst(bbase[ia], chunk, a - first[ia]);
    u64 const e = a + j;
    if (e >= E) { srcOffS[j] = off[n]; dstOffS[j] = bbase[n] - dstA; return; }
    u64 const i = zj_entry_owner(first, n, e), k = e - first[i];
    srcOffS[j] = zj_chunk_src(off[i], chunk, k);
    dstOffS[j] = zj_chunk_dst(bbase[i], chunk, k) - dstA;
}
// One wave per buffer, the entries it has in the slice [a, a + m): a running sum of the frame sizes (carried from slice to slice) places every frame in the caller's
// slot; a frame moves only when it ends inside the slot, so nothing is written outside it; the first entry that answered an error is remembered.
__global__ __launch_bounds__(64) void zj_chunks_place_kernel(const u64* __restrict__ first, const u64* __restrict__ dstOff, u32 n, u64 a, u32 m, const u64* __restrict__ resS,
                                                             u64* __restrict__ carry, u64* __restrict__ ferr, u64* __restrict__ packSize, u64* __restrict__ packDst) {
    u32 const lane = threadIdx.x;
    for (u32 i = blockIdx.x; i < n; i += gridDim.x) {
        u64 const f0 = first[i], f1 = first[i + 1], lo = f0 > a ? f0 : a, hi = f1 < a + m ? f1 : a + m;
        if (lo >= hi) continue;
        u64 const dlo = dstOff[i], dhi = dstOff[i + 1], cap = dhi > dlo ? dhi - dlo : 0;
        u64 run = carry[i], err = ferr[i];
        for (u64 base = lo; base < hi; base += 64) {
            u64 const e = base + lane;
            bool const in = e < hi;
            u64 const r = in ? resS[e - a] : 0;
            bool const bad = r > ((u64)1 << 40);
            u64 const sz = bad ? 0 : r;
            u64 incl = sz;
            for (u32 d = 1; d < 64; d <<= 1) { u64 const v = __shfl_up(incl, d, 64); if (lane >= d) incl += v; }
            u64 const pos = run + (incl - sz);
            if (in) { packSize[e - a] = (!bad && pos + sz <= cap) ? sz : ~(u64)0; packDst[e - a] = dlo + (pos < cap ? pos : cap); }
            unsigned long long const mask = __ballot(bad);
            if (mask && !err) err = __shfl(r, (int)(__ffsll((long long)mask) - 1), 64);
            run += __shfl(incl, 63, 64);
        }
        if (lane == 0) { carry[i] = run; ferr[i] = err; }
    }
}
__global__ __launch_bounds__(256) void zj_chunks_verdict_kernel(const u64* __restrict__ dstOff, u32 n, const u64* __restrict__ carry, const u64* __restrict__ ferr, u64* __restrict__ result) {
    u64 const i = (u64)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    u64 const dlo = dstOff[i], dhi = dstOff[i + 1], cap = dhi > dlo ? dhi - dlo : 0;
    result[i] = ferr[i] ? ferr[i] : (carry[i] > cap ? ZJ_ERR64(ZJ_E_DSTSIZE_TOO_SMALL) : carry[i]);
}
size_t zjni_compress_chunked_batch_device(const void* d_src, const uint64_t* d_src_off, void* d_dst, const uint64_t* d_dst_off,
                                          uint64_t* d_result, size_t n, int level, int checksum, size_t chunkSize, void* stream) {
    if (!zj_level_arg(level)) return ZJNI_ERR(42);
    if (chunkSize < 256 || chunkSize > ZJNI_BLOCKSIZE_MAX) return ZJNI_ERR(42);
    DevState* d = cur_state();
    if (!d) return ZJNI_ERR(ZJNI_ERROR_no_device);
    if (n > 0xFFFFFFFFull) return ZJNI_ERR(72);
    if (n == 0) return 0;
    hipStream_t const st = (hipStream_t)stream;
    BatchOrder order(d, stream);
    if (!frames_state(d)) return ZJNI_ERR(64);
    // per buffer: [cnt n][btot n][first n + 1][bbase n + 1][carry n][ferr n]
    size_t const nb = zj_up16((n + 1) * 8), oCnt = 0, oBtot = nb, oFirst = 2 * nb, oBbase = 3 * nb, oCarry = 4 * nb, oFerr = 5 * nb, perBuf = 6 * nb;
    size_t r = frames_room(d, perBuf, 0, st);
    if (r != 0) return r;
    u32 const gridN = (u32)((n + 255) / 256);
    hipLaunchKernelGGL(zj_chunks_count_kernel, dim3(gridN), dim3(256), 0, st, (const u64*)d_src_off, (u32)n, (u64)chunkSize, (u64*)(d->framesBuf + oCnt), (u64*)(d->framesBuf + oBtot));
    hipLaunchKernelGGL(zj_pack_offsets_kernel, dim3(1), dim3(1024), 0, st, (const u64*)(d->framesBuf + oCnt), (u64*)(d->framesBuf + oFirst), (u32)n);
    hipLaunchKernelGGL(zj_pack_offsets_kernel, dim3(1), dim3(1024), 0, st, (const u64*)(d->framesBuf + oBtot), (u64*)(d->framesBuf + oBbase), (u32)n);
    if (hipMemsetAsync(d->framesBuf + oCarry, 0, 2 * nb, st) != hipSuccess) return ZJNI_ERR(ZJNI_ERROR_no_device);
    u64 E = 0;
    if ((r = frames_read_total(d, (const u64*)(d->framesBuf + oFirst) + n, 1, st, &E)) != 0) return r;
    if (E > 0xFFFFFFFFull) return ZJNI_ERR(72);
    if (E < n) return ZJNI_ERR(ZJNI_ERROR_no_device);
    // per slice of S entries: [srcOffS S + 1][dstOffS S + 1][resS S][packSize S][packDst S][scratch destinations: S x zjni_compressBound(chunk)]
    size_t const bound = (size_t)zj_compress_bound(chunkSize);
    size_t S = scratch_slice(bound + 48, ZJ_CHUNK_FRAMES, 4);
    if (S > E) S = (size_t)E;
    size_t const ns = zj_up16((S + 1) * 8), oSrcS = perBuf, oDstS = oSrcS + ns, oResS = oDstS + ns, oPSize = oResS + ns, oPDst = oPSize + ns, oOut = oPDst + ns;
    size_t const total = oOut + zj_up16(S * bound) + 16;
    if ((r = frames_room(d, total, perBuf, st)) != 0) return r;
    u8* const fb = d->framesBuf;
    u32 const gridW = grid_cap(d, n);
    for (u64 a = 0; a < E; a += S) {
        u32 const m = (u32)(E - a < S ? E - a : S);
        hipLaunchKernelGGL(zj_chunks_emit_kernel, dim3(m / 256 + 1), dim3(256), 0, st, (const u64*)d_src_off, (const u64*)(fb + oFirst), (const u64*)(fb + oBbase), (u32)n, (u64)chunkSize,
                           a, m, E, (u64*)(fb + oSrcS), (u64*)(fb + oDstS));
        if (hipGetLastError() != hipSuccess) return ZJNI_ERR(ZJNI_ERROR_no_device);
        if ((r = compress_chunked_ordered(d_src, (const u64*)(fb + oSrcS), fb + oOut, (const u64*)(fb + oDstS), (u64*)(fb + oResS), m, level, checksum ? ZE_FLAG_CHECKSUM : 0u, stream)) != 0) return r;
        hipLaunchKernelGGL(zj_chunks_place_kernel, dim3(gridW), dim3(64), 0, st, (const u64*)(fb + oFirst), (const u64*)d_dst_off, (u32)n, a, m, (const u64*)(fb + oResS),
                           (u64*)(fb + oCarry), (u64*)(fb + oFerr), (u64*)(fb + oPSize), (u64*)(fb + oPDst));
        hipLaunchKernelGGL(zj_pack_kernel, dim3(grid_cap(d, m)), dim3(256), 0, st, (const u8*)(fb + oOut), (const u64*)(fb + oDstS), (const u64*)(fb + oPSize), (u8*)d_dst, (const u64*)(fb + oPDst), m);
    }
    hipLaunchKernelGGL(zj_chunks_verdict_kernel, dim3(gridN), dim3(256), 0, st, (const u64*)d_dst_off, (u32)n, (const u64*)(fb + oCarry), (const u64*)(fb + oFerr), (u64*)d_result);
    return hipGetLastError() == hipSuccess ? 0 : ZJNI_ERR(ZJNI_ERROR_no_device);
}

// ---- pieces: chunked compress with a dictionary, the caller's cuts and the frame sizes out ----
size_t zjni_compressBound_pieces(size_t srcSize, size_t nPieces) { return (size_t)zj_pieces_bound(srcSize, nPieces); }
// One wave per buffer: lanes stride the cut list, a wave-wide AND gives its legality.  idx[i] = the entries buffer i owns in the caller's index (0 for an illegal list),
// cnt[i] = the entries it is walked as inside the call (zj_pieces_walked), ferr[i] = 0 or the 42 of an illegal list, which the place kernel's first-error rule then keeps.
__global__ __launch_bounds__(64) void zj_pieces_count_kernel(const u64* __restrict__ off, u32 n, u64 chunk, const u64* __restrict__ cut, const u64* __restrict__ cutOff,
                                                             u64* __restrict__ cnt, u64* __restrict__ idx, u64* __restrict__ ferr) {
    u32 const lane = threadIdx.x;
    for (u32 i = blockIdx.x; i < n; i += gridDim.x) {
        u64 const lo = off[i], hi = off[i + 1], size = hi > lo ? hi - lo : 0;
        bool ok = true; u64 pieces = zj_chunk_count(size, chunk);
        if (cut) {                                                      // (uniform over the wave, as i and c are: every lane reaches the ballot)
            u64 const c0 = cutOff[i], c1 = cutOff[i + 1], c = c1 > c0 ? c1 - c0 : 0;
            ok = c1 >= c0 && (c || zj_cut_none_ok(size, chunk));
            for (u64 k = lane; ok && k < c; k += 64) ok = zj_cut_ok(cut + c0, c, k, size, chunk);
            ok = __ballot(!ok) == 0ull;
            pieces = c + 1;
        }
        if (lane == 0) { cnt[i] = zj_pieces_walked(ok, pieces, size, chunk); idx[i] = ok ? pieces : 0; ferr[i] = ok ? 0 : ZJ_ERR64(42); }
    }
}
// one lane per entry of the slice [a, a + m], its end included: where the piece begins in the source; its scratch destination is its place in the slice x bound
__global__ __launch_bounds__(256) void zj_pieces_emit_kernel(const u64* __restrict__ off, const u64* __restrict__ first, const u64* __restrict__ idx, u32 n, u64 chunk, u64 bound,
                                                             const u64* __restrict__ cut, const u64* __restrict__ cutOff, u64 a, u32 m, u64 E,
                                                             u64* __restrict__ srcOffS, u64* __restrict__ dstOffS) {
    u64 const j = (u64)blockIdx.x * 256u + threadIdx.x;
    if (j > m) return;
    dstOffS[j] = j * bound;
    u64 const e = a + j;
    if (e >= E) { srcOffS[j] = off[n]; return; }
    u64 const i = zj_entry_owner(first, n, e);
    srcOffS[j] = zj_piece_src(off[i], chunk, (cut && idx[i]) ? cut + cutOff[i] : nullptr, e - first[i]);
}
// one lane per entry of the slice [a, a + m), behind its compress call: the entry's size goes to the caller's index; an entry of a buffer with an illegal list
// answers that buffer's 42 instead of its frame's size, so the place kernel moves nothing of it
__global__ __launch_bounds__(256) void zj_pieces_sizes_kernel(const u64* __restrict__ first, const u64* __restrict__ ifirst, const u64* __restrict__ idx, u32 n, u64 a, u32 m,
                                                              u64* __restrict__ resS, u64* __restrict__ pieceSize, u64 pieceCap) {
    u64 const j = (u64)blockIdx.x * 256u + threadIdx.x;
    if (j >= m) return;
    u64 const e = a + j, i = zj_entry_owner(first, n, e);
    if (!idx[i]) { resS[j] = ZJ_ERR64(42); return; }
    u64 const p = ifirst[i] + (e - first[i]);
    if (pieceSize && p < pieceCap) pieceSize[p] = resS[j];
}
size_t zjni_compress_pieces_batch_device(const void* d_src, const uint64_t* d_src_off, void* d_dst, const uint64_t* d_dst_off, uint64_t* d_result, size_t n,
                                         int level, int flags, size_t chunkSize, const uint64_t* d_cut, const uint64_t* d_cut_off, const zjni_cdict* cdict,
                                         uint64_t* d_piece_first, uint64_t* d_piece_size, size_t pieceCap, void* stream) {
    if ((u32)flags & ZE_FLAG_NO_FCS) return ZJNI_ERR(42);          // a frame without a content size can be neither split nor range-read afterwards
    if (!cdict && !zj_level_arg(level)) return ZJNI_ERR(42);
    if (chunkSize < 256 || chunkSize > ZJNI_BLOCKSIZE_MAX) return ZJNI_ERR(42);
    if (d_cut && !d_cut_off) return ZJNI_ERR(42);
    if (cdict && !dict_on_this_device(cdict->ordinal)) return ZJNI_ERR(32);       // zjni_compress_batch_device_usingCDict's answer
    DevState* d = cur_state();
    if (!d) return ZJNI_ERR(ZJNI_ERROR_no_device);
    if (n > 0xFFFFFFFFull) return ZJNI_ERR(72);
    hipStream_t const st = (hipStream_t)stream;
    if (n == 0) {
        if (d_piece_first && hipMemsetAsync(d_piece_first, 0, 8, st) != hipSuccess) return ZJNI_ERR(ZJNI_ERROR_no_device);
        return 0;
    }
    u32 const fl = cdict ? (zj_frame_flags(flags) & ~ZE_FLAG_NO_FCS) : (((u32)flags & 1u) ? ZE_FLAG_CHECKSUM : 0u);
    BatchOrder order(d, stream);
    if (!frames_state(d)) return ZJNI_ERR(64);
    // per buffer: [cnt n][idx n][first n + 1][ifirst n + 1][carry n][ferr n]
    size_t const nb = zj_up16((n + 1) * 8), oCnt = 0, oIdx = nb, oFirst = 2 * nb, oIfirst = 3 * nb, oCarry = 4 * nb, oFerr = 5 * nb, perBuf = 6 * nb;
    size_t r = frames_room(d, perBuf, 0, st);
    if (r != 0) return r;
    u32 const gridN = (u32)((n + 255) / 256);
    u32 const gridW = grid_cap(d, n);
    hipLaunchKernelGGL(zj_pieces_count_kernel, dim3(gridW), dim3(64), 0, st, (const u64*)d_src_off, (u32)n, (u64)chunkSize, (const u64*)d_cut, (const u64*)d_cut_off,
                       (u64*)(d->framesBuf + oCnt), (u64*)(d->framesBuf + oIdx), (u64*)(d->framesBuf + oFerr));
    hipLaunchKernelGGL(zj_pack_offsets_kernel, dim3(1), dim3(1024), 0, st, (const u64*)(d->framesBuf + oCnt), (u64*)(d->framesBuf + oFirst), (u32)n);
    hipLaunchKernelGGL(zj_pack_offsets_kernel, dim3(1), dim3(1024), 0, st, (const u64*)(d->framesBuf + oIdx), (u64*)(d->framesBuf + oIfirst), (u32)n);
    if (hipMemsetAsync(d->framesBuf + oCarry, 0, nb, st) != hipSuccess) return ZJNI_ERR(ZJNI_ERROR_no_device);
    // the one host wait: E (the entries walked) and, eight bytes beside it, the entries of the caller's index — they differ by the walks of illegal lists
    u64 both[2];
    if ((r = frames_read_total(d, (const u64*)(d->framesBuf + oFirst) + n, 1, st, both, (const u64*)(d->framesBuf + oIfirst) + n)) != 0) return r;
    u64 const E = both[0], EI = both[1];
    if (E > 0xFFFFFFFFull || EI > 0xFFFFFFFFull) return ZJNI_ERR(72);
    if (E < n || EI > E) return ZJNI_ERR(ZJNI_ERROR_no_device);
    if (d_piece_size && EI > pieceCap) return ZJNI_ERR(70);
    if (d_piece_first && hipMemcpyAsync(d_piece_first, d->framesBuf + oIfirst, (n + 1) * 8, hipMemcpyDeviceToDevice, st) != hipSuccess) return ZJNI_ERR(ZJNI_ERROR_no_device);
    // per slice of S entries: [srcOffS S + 1][dstOffS S + 1][resS S][packSize S][packDst S][scratch destinations: S x zjni_compressBound(chunk)]
    size_t const bound = (size_t)zj_compress_bound(chunkSize);
    size_t S = scratch_slice(bound + 48, ZJ_CHUNK_FRAMES, 4);
    if (S > E) S = (size_t)E;
    size_t const ns = zj_up16((S + 1) * 8), oSrcS = perBuf, oDstS = oSrcS + ns, oResS = oDstS + ns, oPSize = oResS + ns, oPDst = oPSize + ns, oOut = oPDst + ns;
    size_t const total = oOut + zj_up16(S * bound) + 16;
    if ((r = frames_room(d, total, perBuf, st)) != 0) return r;
    u8* const fb = d->framesBuf;
    for (u64 a = 0; a < E; a += S) {
        u32 const m = (u32)(E - a < S ? E - a : S);
        hipLaunchKernelGGL(zj_pieces_emit_kernel, dim3(m / 256 + 1), dim3(256), 0, st, (const u64*)d_src_off, (const u64*)(fb + oFirst), (const u64*)(fb + oIdx), (u32)n, (u64)chunkSize,
                           (u64)bound, (const u64*)d_cut, (const u64*)d_cut_off, a, m, E, (u64*)(fb + oSrcS), (u64*)(fb + oDstS));
        if (hipGetLastError() != hipSuccess) return ZJNI_ERR(ZJNI_ERROR_no_device);
        r = cdict ? compress_cdict_ordered(d, d_src, (const u64*)(fb + oSrcS), fb + oOut, (const u64*)(fb + oDstS), (u64*)(fb + oResS), m, cdict, fl, stream)
                  : compress_chunked_ordered(d_src, (const u64*)(fb + oSrcS), fb + oOut, (const u64*)(fb + oDstS), (u64*)(fb + oResS), m, level, fl, stream);
        if (r != 0) return r;
        hipLaunchKernelGGL(zj_pieces_sizes_kernel, dim3((m + 255) / 256), dim3(256), 0, st, (const u64*)(fb + oFirst), (const u64*)(fb + oIfirst), (const u64*)(fb + oIdx), (u32)n, a, m,
                           (u64*)(fb + oResS), (u64*)d_piece_size, (u64)pieceCap);
        hipLaunchKernelGGL(zj_chunks_place_kernel, dim3(gridW), dim3(64), 0, st, (const u64*)(fb + oFirst), (const u64*)d_dst_off, (u32)n, a, m, (const u64*)(fb + oResS),
                           (u64*)(fb + oCarry), (u64*)(fb + oFerr), (u64*)(fb + oPSize), (u64*)(fb + oPDst));
        hipLaunchKernelGGL(zj_pack_kernel, dim3(grid_cap(d, m)), dim3(256), 0, st, (const u8*)(fb + oOut), (const u64*)(fb + oDstS), (const u64*)(fb + oPSize), (u8*)d_dst, (const u64*)(fb + oPDst), m);
    }
    hipLaunchKernelGGL(zj_chunks_verdict_kernel, dim3(gridN), dim3(256), 0, st, (const u64*)d_dst_off, (u32)n, (const u64*)(fb + oCarry), (const u64*)(fb + oFerr), (u64*)d_result);
    return hipGetLastError() == hipSuccess ? 0 : ZJNI_ERR(ZJNI_ERROR_no_device);
}

// ---- blocking forms for one host buffer, staged like zjni_compress2 / zjni_decompress: [srcOff 2][dstOff 2][result 1][pad][src][dst] in one staging slot ----
static size_t host_one_buffer(bool compress, void* dst, size_t dstCap, const void* src, size_t srcSize, int level, int checksum, size_t chunkSize, const zjni_ddict* ddict = nullptr) {
    DevState* d = cur_state();
    if (!d) return ZJNI_ERR(ZJNI_ERROR_no_device);
    if (srcSize > ((size_t)1 << 46) || dstCap > ((size_t)1 << 46)) return ZJNI_ERR(64);
    if ((srcSize && !src) || (dstCap && !dst)) return ZJNI_ERR(72);
    size_t const oSrc = 64, oDst = oSrc + zj_up16(srcSize), total = oDst + dstCap + 16;
    StagedCall sc(d, total);
    if (!sc.ready) return ZJNI_ERR(ZJNI_ERROR_unsupported);
    u64* const h = sc.words();
    h[0] = 0; h[1] = srcSize; h[2] = 0; h[3] = dstCap; h[4] = 0;
    if (srcSize) memcpy(sc.host + oSrc, src, srcSize);
    if (!sc.upload(oSrc + srcSize)) return ZJNI_ERR(ZJNI_ERROR_no_device);
    u64* const dW = (u64*)sc.dev;
    size_t const r = compress ? zjni_compress_chunked_batch_device(sc.dev + oSrc, dW, sc.dev + oDst, dW + 2, dW + 4, 1, level, checksum, chunkSize, sc.st)
                              : zjni_decompress_frames_batch_device(sc.dev + oSrc, dW, sc.dev + oDst, dW + 2, dW + 4, 1, ddict, sc.st);
    if (zjni_isError(r)) return r;
    if (!sc.fetch(4, 1)) return ZJNI_ERR(ZJNI_ERROR_no_device);
    return sc.payload((size_t)h[4], dst, dstCap, oDst);
}
size_t zjni_compress_chunked(void* dst, size_t dstCap, const void* src, size_t srcSize, int level, int checksum, size_t chunkSize) {
    return host_one_buffer(true, dst, dstCap, src, srcSize, level, checksum, chunkSize);
}
size_t zjni_decompress_frames(void* dst, size_t dstCap, const void* src, size_t srcSize) {
    return host_one_buffer(false, dst, dstCap, src, srcSize, 0, 0, 0);
}
size_t zjni_decompress_frames_usingDDict(void* dst, size_t dstCap, const void* src, size_t srcSize, const zjni_ddict* ddict) {
    return host_one_buffer(false, dst, dstCap, src, srcSize, 0, 0, 0, ddict);
}
// zjni_compress_pieces_batch_device for one host buffer: [srcOff 2][dstOff 2][result 1][cutOff 2][pad][pieceFirst 2][pad] fill the slot's first 128 bytes, then
// [src][cuts][piece sizes][dst]
size_t zjni_compress_pieces(void* dst, size_t dstCap, const void* src, size_t srcSize, int level, int flags, size_t chunkSize, const uint64_t* cut, size_t nCut,
                            const zjni_cdict* cdict, uint64_t* pieceSize, size_t pieceCap, size_t* nPieces) {
    DevState* d = cur_state();
    if (!d) return ZJNI_ERR(ZJNI_ERROR_no_device);
    if (srcSize > ((size_t)1 << 46) || dstCap > ((size_t)1 << 46) || nCut > ((size_t)1 << 32) || pieceCap > ((size_t)1 << 32)) return ZJNI_ERR(64);
    if ((srcSize && !src) || (dstCap && !dst)) return ZJNI_ERR(72);
    if (!cut) nCut = 0;
    if (!pieceSize) pieceCap = 0;
    size_t const oSrc = 128, oCut = oSrc + zj_up16(srcSize), oPs = oCut + zj_up16(nCut * 8), oDst = oPs + zj_up16(pieceCap * 8), total = oDst + dstCap + 16;
    StagedCall sc(d, total);
    if (!sc.ready) return ZJNI_ERR(ZJNI_ERROR_unsupported);
    u64* const h = sc.words();
    memset(h, 0, 128);
    h[1] = srcSize; h[3] = dstCap; h[6] = nCut;
    if (srcSize) memcpy(sc.host + oSrc, src, srcSize);
    if (nCut) memcpy(sc.host + oCut, cut, nCut * 8);
    if (!sc.upload(oPs)) return ZJNI_ERR(ZJNI_ERROR_no_device);
    u64* const dW = (u64*)sc.dev;
    size_t const r = zjni_compress_pieces_batch_device(sc.dev + oSrc, dW, sc.dev + oDst, dW + 2, dW + 4, 1, level, flags, chunkSize,
                                                       cut ? (const u64*)(sc.dev + oCut) : nullptr, cut ? dW + 5 : nullptr, cdict,
                                                       dW + 8, pieceSize ? (u64*)(sc.dev + oPs) : nullptr, pieceCap, sc.st);
    if (zjni_isError(r)) return r;
    if (!sc.fetch(4, 6)) return ZJNI_ERR(ZJNI_ERROR_no_device);                // the result and, in [8 .. 10), pieceFirst; the device left the words between as they were sent
    size_t const res = (size_t)h[4], E = (size_t)h[9];
    if (nPieces) *nPieces = E;
    if (zjni_isError(res)) return res;
    if (res > dstCap || (pieceSize && E > pieceCap)) return ZJNI_ERR(ZJNI_ERROR_no_device);
    // the frame's bytes and the piece sizes behind one wait
    return sc.download({{dst, oDst, res}, {pieceSize, oPs, pieceSize ? E * 8 : 0}}) ? res : ZJNI_ERR(ZJNI_ERROR_no_device);
}

// the ranged form: [srcOff 2][dstOff 2][result 1][range 2][total 1] fill the slot's first 64 bytes; the slot is as large as the range can get, not as the buffer
size_t zjni_decompress_frames_range(void* dst, size_t dstCap, const void* src, size_t srcSize, unsigned long long lo, unsigned long long len, unsigned long long* total) {
    return zjni_decompress_frames_range_usingDDict(dst, dstCap, src, srcSize, lo, len, total, nullptr);
}
size_t zjni_decompress_frames_range_usingDDict(void* dst, size_t dstCap, const void* src, size_t srcSize, unsigned long long lo, unsigned long long len, unsigned long long* total,
                                               const zjni_ddict* ddict) {
    DevState* d = cur_state();
    if (!d) return ZJNI_ERR(ZJNI_ERROR_no_device);
    if ((u64)dstCap > len) dstCap = (size_t)len;
    if (srcSize > ((size_t)1 << 46) || dstCap > ((size_t)1 << 46)) return ZJNI_ERR(64);
    if ((srcSize && !src) || (dstCap && !dst)) return ZJNI_ERR(72);
    size_t const oSrc = 64, oDst = oSrc + zj_up16(srcSize), all = oDst + dstCap + 16;
    StagedCall sc(d, all);
    if (!sc.ready) return ZJNI_ERR(ZJNI_ERROR_unsupported);
    u64* const h = sc.words();
    h[0] = 0; h[1] = srcSize; h[2] = 0; h[3] = dstCap; h[4] = 0; h[5] = lo; h[6] = len; h[7] = 0;
    if (srcSize) memcpy(sc.host + oSrc, src, srcSize);
    if (!sc.upload(oSrc + srcSize)) return ZJNI_ERR(ZJNI_ERROR_no_device);
    u64* const dW = (u64*)sc.dev;
    size_t const r = zjni_decompress_frames_range_batch_device(sc.dev + oSrc, dW, sc.dev + oDst, dW + 2, dW + 5, dW + 4, dW + 7, 1, ddict, sc.st);
    if (zjni_isError(r)) return r;
    if (!sc.fetch(4, 4)) return ZJNI_ERR(ZJNI_ERROR_no_device);
    if (total) *total = h[7];
    return sc.payload((size_t)h[4], dst, dstCap, oDst);
}

// The indexed form for one host buffer: rules 1-4 run here, on the host, with the functions the request kernel runs; only the selected entries' bytes and their slice
// of the index cross the link, and the device entry answers the range shifted by the content before the first selected entry.  The slot's first 64 bytes are
// [srcOff 2][dstOff 2][result 1][request 3], then [index of 1 buffer and m entries][the selected source bytes][dst].
size_t zjni_decompress_index_range(void* dst, size_t dstCap, const void* src, size_t srcSize, unsigned long long lo, unsigned long long len,
                                   const uint64_t* pieceSize, const uint64_t* pieceContent, size_t nPieces, unsigned long long* total, const zjni_ddict* ddict) {
    DevState* d = cur_state();
    if (!d) return ZJNI_ERR(ZJNI_ERROR_no_device);
    if (total) *total = ZJ_FI_ERROR;
    if ((u64)dstCap > len) dstCap = (size_t)len;
    if (srcSize > ((size_t)1 << 46) || dstCap > ((size_t)1 << 46) || nPieces > 0xFFFFFFFFull) return ZJNI_ERR(64);
    if ((srcSize && !src) || (dstCap && !dst) || (nPieces && (!pieceSize || !pieceContent))) return ZJNI_ERR(72);
    // the whole buffer's index in host memory: one buffer, nPieces entries
    std::vector<u64> hidx((size_t)zj_index_words(1, nPieces));
    u64* const C = hidx.data() + 3; u64* const U = C + nPieces + 1;
    bool legal = true;
    hidx[0] = 0; hidx[1] = nPieces; C[0] = U[0] = 0;
    for (size_t e = 0; e < nPieces; e++) {
        legal = legal && pieceSize[e] <= ZJ_INDEX_SIZE_MAX && pieceContent[e] <= ZJ_INDEX_SIZE_MAX;
        C[e + 1] = C[e] + zj_index_term(pieceSize[e]); U[e + 1] = U[e] + zj_index_term(pieceContent[e]);
    }
    hidx[2] = zj_index_valid(legal, nullptr, 0);
    u64 const hoff[2] = {0, (u64)srcSize};
    ZRRec rec; ZIReq ir; u64 q[5];
    zj_index_request(hidx.data(), 1, nPieces, hoff, 0, lo, len, dstCap, rec, ir, q);
    if (total) *total = rec.total;
    if (rec.status == ZJ_RANGE_NOTHING) return 0;
    if (rec.status != ZJ_RANGE_SELECTED) return ZJNI_ERR(rec.status);
    u64 const eF = ir.e0 - (rec.edges & 1u), m = rec.frames, cLo = C[eF], bytes = C[eF + m] - cLo, uLo = U[eF], want = rec.hi - rec.lo;
    size_t const idxBytes = (size_t)zj_index_bytes(1, m), oIdx = 64, oSrc = oIdx + idxBytes, oDst = oSrc + zj_up16(bytes), all = oDst + want + 16;
    StagedCall sc(d, all);
    if (!sc.ready) return ZJNI_ERR(ZJNI_ERROR_unsupported);
    u64* const h = sc.words();
    h[0] = 0; h[1] = bytes; h[2] = 0; h[3] = want; h[4] = 0; h[5] = 0; h[6] = rec.lo - uLo; h[7] = want;
    u64* const hi = (u64*)(sc.host + oIdx);
    hi[0] = 0; hi[1] = m; hi[2] = 0;
    for (u64 k = 0; k <= m; k++) { hi[3 + k] = C[eF + k] - cLo; hi[3 + m + 1 + k] = U[eF + k] - uLo; }
    memcpy(sc.host + oSrc, (const u8*)src + cLo, bytes);
    if (!sc.upload(oSrc + bytes)) return ZJNI_ERR(ZJNI_ERROR_no_device);
    u64* const dW = (u64*)sc.dev;
    size_t const r = zjni_decompress_index_range_batch_device(sc.dev + oSrc, dW, 1, sc.dev + oIdx, (size_t)m, dW + 5, sc.dev + oDst, dW + 2, dW + 4, nullptr, 1, ddict, sc.st);
    if (zjni_isError(r)) return r;
    if (!sc.fetch(4, 1)) return ZJNI_ERR(ZJNI_ERROR_no_device);
    return sc.payload((size_t)h[4], dst, dstCap, oDst);
}

// The walk on the host, no device: the arrays zjni_decompress_index_range takes, from the bytes alone, by the function both device walks run.
size_t zjni_index_from_frames(const void* src, size_t srcSize, uint64_t* pieceSize, uint64_t* pieceContent, size_t capacity, size_t* nPieces) {
    if (nPieces) *nPieces = 0;
    if ((srcSize && !src) || (capacity && (!pieceSize || !pieceContent))) return ZJNI_ERR(72);
    u64 entries = 0, wrote = 0;
    u32 const verdict = zj_index_walk((const u8*)src, (u64)srcSize, (u64)capacity, (u64*)pieceSize, (u64*)pieceContent, &entries, &wrote);
    if (verdict) return ZJNI_ERR(verdict);
    if (nPieces) *nPieces = (size_t)entries;
    return entries > capacity ? ZJNI_ERR(70) : 0;
}

}  // extern "C"
