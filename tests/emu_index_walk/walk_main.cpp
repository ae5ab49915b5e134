// tests/emu_index_walk/walk_main.cpp — the host form of the index walk as a stand-alone program for the host sanitizers (address, undefined): reads a file of
// length-prefixed buffers (uint64 little endian, then the bytes), walks each on an exact-size malloc copy with exact-size output arrays — the counting call, the
// call with a capacity one too small, the filling call — and prints one line a buffer:  <code> <count> <count at capacity - 1> | sizes | contents.
// For tests/test_emu_index_walk.py.  TEST INFRASTRUCTURE ONLY: never linked into libzjni_amd.so.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

typedef unsigned long long ull;
extern "C" ull emu_walk_host(const unsigned char* src, ull srcSize, ull* pieceSize, ull* pieceContent, ull capacity, ull* nPieces);

static unsigned code_of(ull r) { return r > ~0ull - 120 ? (unsigned)(0 - r) : 0u; }

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: walk_main FILE\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    for (;;) {
        ull len = 0;
        if (fread(&len, 8, 1, f) != 1) break;
        unsigned char* buf = len ? (unsigned char*)malloc((size_t)len) : nullptr;
        if (len && fread(buf, 1, (size_t)len, f) != len) { fprintf(stderr, "short file\n"); return 2; }
        ull count = 0, again = 0, shortCount = 0;
        ull const r0 = emu_walk_host(buf, len, nullptr, nullptr, 0, &count);
        if (code_of(r0) != 0 && code_of(r0) != 70) { printf("%u 0 0 | |\n", code_of(r0)); free(buf); continue; }
        if (count) {                                          // one entry too few: 70, the count needed, and no write beyond the capacity
            ull* s1 = (ull*)malloc((size_t)(count - 1) * 8 + (count == 1)); ull* c1 = (ull*)malloc((size_t)(count - 1) * 8 + (count == 1));
            ull const r1 = emu_walk_host(buf, len, s1, c1, count - 1, &shortCount);
            if (code_of(r1) != 70) { fprintf(stderr, "capacity - 1 answered %u\n", code_of(r1)); return 1; }
            free(s1); free(c1);
        }
        ull* size = (ull*)malloc((size_t)count * 8 + !count); ull* content = (ull*)malloc((size_t)count * 8 + !count);
        ull const r2 = emu_walk_host(buf, len, size, content, count, &again);
        if (r2 != 0 || again != count) { fprintf(stderr, "the filling call answered %llu, %llu entries\n", r2, again); return 1; }
        printf("0 %llu %llu |", count, shortCount);
        for (ull k = 0; k < count; k++) printf(" %llu", size[k]);
        printf(" |");
        for (ull k = 0; k < count; k++) printf(" %llu", content[k]);
        printf("\n");
        free(size); free(content); free(buf);
    }
    fclose(f);
    return 0;
}
