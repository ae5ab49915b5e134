// tests/emu_sequences_nodelim/entries_main.cpp — the host parts of the sequence entries with ZJNI_SEQ_NO_DELIMITERS (flag check, the host forms' packing) as a
// stand-alone program for the host sanitizers: `make -C tests/emu_sequences_nodelim asan` links it with zj_kernels.hip built with -Xarch_host
// -fsanitize=address,undefined and runs it.  It needs no GPU: without a device the entries answer 200 (no_device) AFTER their host-side work; with one they
// compress, and the answers are checked against what the arguments deserve either way.  TEST INFRASTRUCTURE ONLY.
#include "../../include/zjni_amd.h"
#include <stdio.h>
#include <vector>

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); failures++; } } while (0)

int main() {
    size_t const bad = (size_t)0 - 42, noDevice = (size_t)0 - ZJNI_ERROR_no_device;
    std::vector<unsigned char> small(408);
    for (size_t i = 0; i < small.size(); i++) small[i] = (unsigned char)("etaoinsh"[(i * 7 + i / 5) & 7]);
    CHECK(zjni_compress_sequences(nullptr, 0, nullptr, 0, nullptr, 0, 3, 32) == bad && zjni_compress_sequences(nullptr, 0, nullptr, 0, nullptr, 0, 3, 16 | 64) == bad);
    CHECK(zjni_compress_sequences(nullptr, 0, nullptr, 0, nullptr, 0, 3, 16) == bad);                        // the one-buffer form wants a destination in this mode
    CHECK(zjni_compress_sequences_batch(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 3, 16) == 0);
    CHECK(zjni_compress_sequences_batch_device(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, -5, 16 | 8 | 1, nullptr) == 0);
    CHECK(zjni_compress_sequences_batch_device(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 3, 3, 16, nullptr) == bad);
    size_t res[3] = { 7, 7, 7 };
    std::vector<zjni_sequence> q1 = { { 3, 40, 8, 0 }, { 11, 60, 9, 0 } }, q2 = { { 2, 4, 2, 0 } };
    std::vector<unsigned char> d0(32), d1(512), d2(512);
    const void* src[3] = { nullptr, small.data(), small.data() };
    size_t srcSize[3] = { 0, small.size(), small.size() };
    const zjni_sequence* seqs[3] = { nullptr, q1.data(), q2.data() };
    size_t nSeqs[3] = { 0, q1.size(), q2.size() };
    void* dst[3] = { d0.data(), d1.data(), d2.data() };
    size_t cap[3] = { d0.size(), d1.size(), d2.size() };
    size_t const r = zjni_compress_sequences_batch(src, srcSize, seqs, nSeqs, dst, cap, res, 3, 3, ZJNI_FRAME_CHECKSUM | ZJNI_SEQ_NO_DELIMITERS);
    if (r == noDevice) printf("no device: the host forms packed their arguments and stopped at the device\n");
    else {
        CHECK(r == 0);
        CHECK(res[0] == 6 + 3 + 4 && !zjni_isError(res[1]) && res[1] < 408 && res[2] == (size_t)0 - 107);
        CHECK(d1[0] == 0x28 && d1[1] == 0xB5 && d1[2] == 0x2F && d1[3] == 0xFD);
    }
    size_t const r1 = zjni_compress_sequences(d1.data(), d1.size(), q1.data(), q1.size(), small.data(), small.size(), 1, ZJNI_SEQ_NO_DELIMITERS);
    CHECK(r1 == noDevice || (!zjni_isError(r1) && r1 < 408));
    printf(failures ? "entries_main: %d FAILED\n" : "entries_main: ok\n", failures);
    return failures ? 1 : 0;
}
