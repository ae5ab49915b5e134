// tests/emu_sequences/host_main.cpp — the host parts of the sequence entries (argument checks, the host forms' packing of sources, sequence arrays and
// offsets) as a stand-alone program for the host sanitizers: `make -C tests/emu_sequences asan` links it with zj_kernels.hip built with
// -Xarch_host -fsanitize=address,undefined and runs it.  It needs no GPU: without a device the entries answer 200 (no_device) AFTER their host-side work;
// with one they compress, and the answers are checked against what the arguments deserve either way.  TEST INFRASTRUCTURE ONLY.
#include "../../include/zjni_amd.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); failures++; } } while (0)

int main() {
    size_t const bad = (size_t)0 - 42, noDevice = (size_t)0 - ZJNI_ERROR_no_device;
    CHECK(zjni_sequenceBound(0) == 2 && zjni_sequenceBound(1) == 2 && zjni_sequenceBound(1023) == 343 && zjni_sequenceBound(131072) == 43690 + 1 + 128 + 1);
    CHECK(zjni_compress_sequences(nullptr, 0, nullptr, 0, nullptr, 0, 3, 16) == bad);
    CHECK(zjni_compress_sequences(nullptr, 0, nullptr, 0, nullptr, 0, 9, 0) == bad);
    size_t res[4] = { 7, 7, 7, 7 };
    CHECK(zjni_compress_sequences_batch(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 3, 0) == 0);
    CHECK(zjni_compress_sequences_batch(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, res, 1, 3, 0) == bad);
    CHECK(zjni_compress_sequences_batch_device(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, -5, 9, nullptr) == 0);
    CHECK(zjni_compress_sequences_batch_device(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 3, 3, 0, nullptr) == bad);
    // four frames in exact-size heap blocks: an empty source, a lone delimiter, a block of three sequences, an array with no delimiter
    std::vector<unsigned char> s1(64), s2(300);
    for (size_t i = 0; i < s1.size(); i++) s1[i] = (unsigned char)("etaoinsh"[(i * 7 + i / 5) & 7]);
    for (size_t i = 0; i < s2.size(); i++) s2[i] = (unsigned char)("etaoinsh"[(i * 5 + i / 3) & 7]);
    std::vector<zjni_sequence> q1 = { { 0, 64, 0, 0 } }, q2 = { { 3, 40, 8, 0 }, { 11, 60, 9, 0 }, { 5, 30, 12, 0 }, { 0, 141, 0, 0 } }, q3 = { { 3, 40, 8, 0 } };
    std::vector<unsigned char> d0(32), d1(128), d2(400), d3(400);
    const void* src[4] = { nullptr, s1.data(), s2.data(), s2.data() };
    size_t srcSize[4] = { 0, s1.size(), s2.size(), s2.size() };
    const zjni_sequence* seqs[4] = { nullptr, q1.data(), q2.data(), q3.data() };
    size_t nSeqs[4] = { 0, q1.size(), q2.size(), q3.size() };
    void* dst[4] = { d0.data(), d1.data(), d2.data(), d3.data() };
    size_t cap[4] = { d0.size(), d1.size(), d2.size(), d3.size() };
    size_t const r = zjni_compress_sequences_batch(src, srcSize, seqs, nSeqs, dst, cap, res, 4, 3, ZJNI_FRAME_CHECKSUM | ZJNI_SEQ_REPCODES);
    if (r == noDevice) printf("no device: the host forms packed their arguments and stopped at the device\n");
    else {
        CHECK(r == 0);
        CHECK(res[0] == 6 + 3 + 4 && res[1] == 6 + 3 + 64 + 4 && !zjni_isError(res[2]) && res[2] < 300 && res[3] == (size_t)0 - 107);
        CHECK(d1[0] == 0x28 && d1[1] == 0xB5 && d1[2] == 0x2F && d1[3] == 0xFD);
    }
    void* null_dst[1] = { nullptr }; size_t one[1] = { 1 };
    CHECK(zjni_compress_sequences_batch(src + 1, srcSize + 1, seqs + 1, nSeqs + 1, null_dst, one, res, 1, 3, 0) == (size_t)0 - 72);
    size_t const r1 = zjni_compress_sequences(d2.data(), d2.size(), q2.data(), q2.size(), s2.data(), s2.size(), 1, 0);
    CHECK(r1 == noDevice || (!zjni_isError(r1) && r1 < 300));
    printf(failures ? "host_main: %d FAILED\n" : "host_main: ok\n", failures);
    return failures ? 1 : 0;
}
