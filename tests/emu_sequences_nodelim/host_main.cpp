// tests/emu_sequences_nodelim/host_main.cpp — the no-delimiter passes and frame loop as a stand-alone program for the host sanitizers:
// `make -C tests/emu_sequences_nodelim asan` builds it with g++ -fsanitize=address,undefined around the lane-serial build (emu_sequences_nodelim.cpp, included) and runs
// it over hand-made arrays that take every branch of the cut, each buffer an exact-size heap block.  (The host parts of the entries are entries_main.cpp, which the
// same target builds with zj_kernels.hip and runs behind this one.)  TEST INFRASTRUCTURE ONLY.
#include "../../include/zjni_amd.h"
#include "emu_sequences_nodelim.cpp"
#include <stdio.h>
#include <vector>

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); failures++; } } while (0)

static unsigned long long emu(const std::vector<unsigned char>& src, const std::vector<zjni_sequence>& q, int level, unsigned flags, unsigned* blocks, std::vector<unsigned char>* out = nullptr) {
    std::vector<unsigned char> dst(src.size() + (src.size() >> 8) + 512);
    unsigned long long const r = emu_compress_sequences_nodelim(src.data(), (unsigned)src.size(), (const unsigned*)q.data(), (unsigned)q.size(), dst.data(), (unsigned)dst.size(), level, flags, blocks);
    if (out && r < dst.size()) out->assign(dst.begin(), dst.begin() + r);
    return r;
}

int main() {
    unsigned long long const e107 = 0ull - 107, e70 = 0ull - 70, e201 = 0ull - 201;
    unsigned nb = 0;
    // ---- the passes and the frame loop, lane-serial ----
    std::vector<unsigned char> text(400000), run(1u << 20, (unsigned char)'e');
    for (size_t i = 0; i < text.size(); i++) text[i] = (unsigned char)("etaoinsh"[(i * 7 + i / 5 + i / 977) & 7]);
    std::vector<unsigned char> small(text.begin(), text.begin() + 408), tiny(text.begin(), text.begin() + 6), twenty(text.begin(), text.begin() + 20);
    CHECK(emu(text, {}, 3, 0, &nb) < text.size() + 64 && nb == 4);                                              // no sequences: literals only, four blocks
    CHECK(emu(run, { { 1, 2, (1u << 20) - 1, 0 } }, 3, 1, &nb) < 200 && nb == 8);                              // one match split seven times, the last edge moved back
    CHECK(emu(run, { { 1, 2, (1u << 20) - 1, 0 } }, 1, 0, &nb) == e201);                                        // beyond the level's window
    CHECK(emu(text, { { 8, 131068, 200000, 0 } }, 3, 0, &nb) < text.size() + 64 && nb == 4);                   // first half of 4: the block ends in front of the match
    CHECK(emu(text, { { 8, 131064, 200000, 0 } }, 1, 0, &nb) < text.size() + 64 && nb == 4);                   // first half of 8: split
    CHECK(emu(text, { { 8, 1000, 131072, 0 } }, 3, 0, &nb) < text.size() + 64 && nb == 5);                     // a match of exactly 128 KiB is not split
    CHECK(emu(text, { { 8, 280000, 50, 0 }, { 3, 10, 0xFFFFFF00u, 0 } }, -5, 1, &nb) < text.size() + 64 && nb == 4);     // the edge in literals twice, then a match past the source
    CHECK(emu(small, { { 4, 8, 402, 0 } }, 3, 0, &nb) == 7 + 3 + 8 && nb == 1);                                 // a shortened last block ends the frame
    CHECK(emu(small, { { 4, 8, 5000, 0 } }, 3, 0, &nb) < 408 + 32);
    CHECK(emu(small, { { 0, 0, 8, 0 }, { 0, 5, 8, 0 } }, 3, 0, &nb) < 408 + 32);                                 // offset 0 is an offset
    CHECK(emu(small, { { 2, 4, 2, 0 } }, 1, 0, &nb) == e107 && emu(small, { { 13, 4, 8, 0 } }, 3, 0, &nb) == e107 && emu(small, { { 12, 4, 8, 0 } }, 3, 0, &nb) < 440);
    CHECK(emu(small, { { 1, 0xFFFFFFF0u, 0x20, 0 } }, 3, 0, &nb) == e107 && emu(small, { { 3, 10, 8, 0 }, { 1, 0x80000000u, 0x80000000u, 0 } }, 3, 0, &nb) == e107);      // lengths that wrap
    CHECK(emu(small, { { 3, 400, 8, 0 }, { 0xFFFFFFFFu, 0xFFFFFFFFu, 1, 7 } }, 3, 0, &nb) < 440);                // ... behind the end of the source: never read
    CHECK(emu(small, { { 0xFFFFFFFDu, 4, 8, 0 } }, 3, 0, &nb) == e107);                                          // offBase 0
    CHECK(emu(twenty, { { 4, 5, 20, 0 } }, 3, 0, &nb) < 64 && nb == 2);                                          // a last block under 7 bytes does not end the loop
    CHECK(emu(tiny, { { 4, 3, 10, 0 } }, 3, 0, &nb) == e70 && nb == 2);                                          // nothing left to consume: the reference fills the destination
    CHECK(emu(std::vector<unsigned char>(text.begin(), text.begin() + 131075), { { 1, 1, 140000, 0 } }, 3, 0, &nb) == e107);      // a block inside a match with 3 bytes left: undefined in the reference
    {   std::vector<zjni_sequence> many;                                                                          // more sequences than a tile, a repcode flag that changes nothing
        for (unsigned i = 0; i < 700; i++) many.push_back({ 1 + i % 3, 3 + i % 2, 4 + i % 3, 0 });
        std::vector<unsigned char> a, b;
        unsigned long long const ra = emu(text, many, 3, 1, &nb, &a), rb = emu(text, many, 3, 1 | 8, &nb, &b);
        CHECK(ra == rb && ra < text.size() + 64 && a == b && !a.empty());
    }
    printf(failures ? "host_main: %d FAILED\n" : "host_main: ok\n", failures);
    return failures ? 1 : 0;
}
