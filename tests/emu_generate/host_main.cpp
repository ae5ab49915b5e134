// tests/emu_generate/host_main.cpp — the host parts of the generate entries (argument checks, the host form's packing of sources and slots, the merge of
// block delimiters) as a stand-alone program for the host sanitizers: `make -C tests/emu_generate asan` links it with zj_kernels.hip built with
// -Xarch_host -fsanitize=address,undefined and runs it.  It needs no GPU: without a device the entries answer 200 (no_device) AFTER their host-side work;
// with one they parse, and the answers are checked against what the arguments deserve either way.  TEST INFRASTRUCTURE ONLY.
#include "../../include/zjni_amd.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); failures++; } } while (0)

int main() {
    size_t const bad = (size_t)0 - 42, noDevice = (size_t)0 - ZJNI_ERROR_no_device;
    CHECK(zjni_generate_sequences(nullptr, 0, nullptr, 0, 9) == bad);
    size_t res[4] = { 7, 7, 7, 7 };
    CHECK(zjni_generate_sequences_batch(nullptr, nullptr, nullptr, nullptr, nullptr, 0, 3, 0) == 0);
    CHECK(zjni_generate_sequences_batch(nullptr, nullptr, nullptr, nullptr, res, 1, 3, 0) == bad);
    CHECK(zjni_generate_sequences_batch(nullptr, nullptr, nullptr, nullptr, res, 1, 3, 1) == bad);
    CHECK(zjni_generate_sequences_batch_device(nullptr, nullptr, nullptr, nullptr, nullptr, 0, -5, 0, nullptr) == 0);
    CHECK(zjni_generate_sequences_batch_device(nullptr, nullptr, nullptr, nullptr, nullptr, 3, 3, 0, nullptr) == bad);
    CHECK(zjni_generate_sequences_batch_device(nullptr, nullptr, nullptr, nullptr, nullptr, ((size_t)1 << 32) + 1, 3, 0, nullptr) == (size_t)0 - 72);
    // the merge, in an exact-size heap block: a trailing delimiter, two adjacent ones, none, an empty array
    {   std::vector<zjni_sequence> a = { { 5, 3, 4, 0 }, { 0, 2, 0, 0 }, { 0, 7, 0, 0 }, { 9, 1, 6, 1 }, { 0, 9, 0, 0 } };
        CHECK(zjni_mergeBlockDelimiters(a.data(), a.size()) == 2 && a[0].litLength == 3 && a[1].offset == 9 && a[1].litLength == 10 && a[1].rep == 1);
        std::vector<zjni_sequence> b = { { 5, 3, 4, 0 }, { 7, 0, 5, 2 } };
        CHECK(zjni_mergeBlockDelimiters(b.data(), b.size()) == 2 && b[1].offset == 7);
        std::vector<zjni_sequence> c = { { 0, 4, 0, 0 } };
        CHECK(zjni_mergeBlockDelimiters(c.data(), c.size()) == 0 && zjni_mergeBlockDelimiters(nullptr, 0) == 0); }
    // four frames in exact-size heap blocks: an empty source, one under 7 bytes, a text, one whose slots are too few
    std::vector<unsigned char> s1(5, 'x'), s2(3000);
    for (size_t i = 0; i < s2.size(); i++) s2[i] = (unsigned char)("etaoinsh"[(i * 5 + i / 3) & 7]);
    std::vector<zjni_sequence> q0(2), q1(4), q2(zjni_sequenceBound(s2.size())), q3(1);
    const void* src[4] = { nullptr, s1.data(), s2.data(), s2.data() };
    size_t srcSize[4] = { 0, s1.size(), s2.size(), s2.size() };
    zjni_sequence* seqs[4] = { q0.data(), q1.data(), q2.data(), q3.data() };
    size_t cap[4] = { q0.size(), q1.size(), q2.size(), q3.size() };
    size_t const r = zjni_generate_sequences_batch(src, srcSize, seqs, cap, res, 4, 3, 0);
    if (r == noDevice) printf("no device: the host form packed its arguments and stopped at the device\n");
    else {
        CHECK(r == 0);
        CHECK(res[0] == 0 && res[1] == (size_t)0 - 106 && !zjni_isError(res[2]) && res[2] >= 2 && res[2] <= q2.size() && res[3] == (size_t)0 - 70);
        if (!zjni_isError(res[2])) CHECK(q2[res[2] - 1].offset == 0 && q2[res[2] - 1].matchLength == 0);
    }
    zjni_sequence* null_seqs[1] = { nullptr }; size_t one[1] = { 1 };
    CHECK(zjni_generate_sequences_batch(src + 2, srcSize + 2, null_seqs, one, res, 1, 3, 0) == (size_t)0 - 72);
    size_t const r1 = zjni_generate_sequences(q2.data(), q2.size(), s2.data(), s2.size(), 1);
    CHECK(r1 == noDevice || (!zjni_isError(r1) && r1 >= 2));
    printf(failures ? "host_main: %d FAILED\n" : "host_main: ok\n", failures);
    return failures ? 1 : 0;
}
