// Stand-alone check of the host side of the variable block-Jacobi layout (new_cg_variants_amd/csrc/prcg_bjvar.h): built with
// -fsanitize=address,undefined and run on the CPU by tests/test_block_jacobi_var.py.  For every edge partition: the tiling's
// invariants, lay -> unlay is the identity on the packed blocks, and no slot of the layout is written twice.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "prcg_bjvar.h"

using namespace prcg;

static int failures = 0;
#define EXPECT(cond)                                                                 \
    do {                                                                             \
        if (!(cond)) { std::printf("FAILED %s (line %d, case %s)\n", #cond, __LINE__, current); ++failures; } \
    } while (0)
static const char* current = "";

static std::vector<int64_t> from_sizes(const std::vector<int>& sizes) {
    std::vector<int64_t> ptr(1, 0);
    for (int m : sizes) ptr.push_back(ptr.back() + m);
    return ptr;
}

static void check(const char* name, const std::vector<int>& sizes, int64_t want_tiles) {
    current = name;
    const std::vector<int64_t> ptr = from_sizes(sizes);
    const int64_t nb = (int64_t)sizes.size(), n = ptr.back();
    int64_t k = -1, m = -1;
    EXPECT(bjvar_check(n, nb, ptr.data(), &k, &m) == 0);
    BjVarPlan P;
    bjvar_plan(n, nb, ptr.data(), P);
    EXPECT(P.ntiles == want_tiles);
    EXPECT((int64_t)P.tiles.size() == P.ntiles * kBjvTileWords);
    EXPECT((int64_t)P.code.size() == P.ntiles * kBjvLanes && P.bidx.size() == P.code.size());
    int64_t rows = 0, lines = 0, blocks = 0;
    for (int64_t T = 0; T < P.ntiles; ++T) {
        const int64_t* tw = P.tiles.data() + T * kBjvTileWords;
        EXPECT(tw[0] == rows && tw[1] == lines && tw[2] == blocks);
        int live = 0, L = 0, starts = 0;
        for (int t = 0; t < kBjvLanes; ++t) {
            const uint8_t cd = P.code[T * kBjvLanes + t];
            if (cd & kBjvDead) continue;
            EXPECT(live == t);                            // live lanes come first, without a gap
            ++live;
            const int a = cd & 7, bm = ((cd >> 3) & 7) + 1;
            EXPECT(a < bm && t - a >= 0 && t - a + bm <= kBjvLanes);
            if (a == 0) ++starts;
            EXPECT(P.bidx[T * kBjvLanes + t] == starts - 1);
            const int64_t kb = tw[2] + starts - 1;
            EXPECT(kb < nb && ptr[kb] == tw[0] + t - a && ptr[kb + 1] - ptr[kb] == bm);
            if (bm > L) L = bm;
        }
        EXPECT(live >= 1 && live <= kBjvLanes && tw[3] == L);
        if (T + 1 < P.ntiles) EXPECT(live + (ptr[blocks + starts + 1] - ptr[blocks + starts]) > kBjvLanes);   // closed because the next block did not fit
        rows += live; lines += L; blocks += starts;
    }
    EXPECT(rows == n && lines == P.lines && blocks == nb);
    int64_t count = 0;
    for (int s : sizes) count += (int64_t)s * s;
    std::vector<double> packed((size_t)count), laid((size_t)P.doubles(), -1.0), back((size_t)count, -2.0);
    for (int64_t q = 0; q < count; ++q) packed[(size_t)q] = 1.0 + (double)q;       // distinct, never 0
    bjvar_lay(P, ptr.data(), packed.data(), laid.data());
    int64_t nonzero = 0;
    for (double v : laid) { EXPECT(v >= 0.0); if (v != 0.0) ++nonzero; }
    EXPECT(nonzero == count);                             // every packed entry has a slot of its own, every other slot holds 0.0
    EXPECT(bjvar_unlay(P, ptr.data(), laid.data(), back.data()) == count);
    EXPECT(back == packed);
}

int main() {
    check("n = 1", {1}, 1);
    check("one block of 5", {5}, 1);
    check("600 of size 1", std::vector<int>(600, 1), 3);
    check("70 of size 8", std::vector<int>(70, 8), 3);
    {
        std::vector<int> s(85, 3);                        // 255 rows, then a block of 8 that does not fit
        s.push_back(8);
        check("255 rows of size 3, then 8", s, 2);
    }
    {
        std::mt19937 g(7);
        std::vector<int> s;
        for (int q = 0; q < 340; ++q) s.push_back(1 + (int)(g() % 8));
        int64_t tiles = 1, fill = 0;                      // the greedy tiles, counted independently
        for (int m : s) { if (fill + m > kBjvLanes) { ++tiles; fill = 0; } fill += m; }
        check("seeded mix of 1..8", s, tiles);
    }
    check("empty", {}, 0);
    // refusals
    current = "refusals";
    int64_t k = -1, m = -1;
    const int64_t a[] = {1, 4}, b[] = {0, 3}, c[] = {0, 2, 2, 4}, d[] = {0, 2, 11, 12};
    EXPECT(bjvar_check(4, 1, a, &k, &m) == 1);
    EXPECT(bjvar_check(4, 1, b, &k, &m) == 2);
    EXPECT(bjvar_check(4, -1, b, &k, &m) == 2);
    EXPECT(bjvar_check(4, 3, c, &k, &m) == 3 && k == 1 && m == 0);
    EXPECT(bjvar_check(12, 3, d, &k, &m) == 3 && k == 1 && m == 9);
    if (failures) { std::printf("%d checks failed\n", failures); return 1; }
    std::printf("bjvar layout ok\n");
    return 0;
}
