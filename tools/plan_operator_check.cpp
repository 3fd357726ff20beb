// Stand-alone check of the operator decision (csrc/prcg_plan.cpp: plan_operator) under AddressSanitizer / UBSan: host code
// only, its own main, no GPU and nothing loaded into Python.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer tools/plan_operator_check.cpp
//       new_cg_variants_amd/csrc/prcg_plan.cpp -lpthread -o plan_operator_check && ./plan_operator_check
//
// Three operators built here -- a 5-point Laplacian, a 15-diagonal band whose outermost columns are ghosts, a ragged
// block matrix with three unknowns per node -- are planned with the default options and with PRCG_WIN=0 (which forces the
// CSR-adaptive tiles with their narrow column codes and value dictionary).  Exit status 0 iff every invariant holds:
//   * the tile tables cover rows 0..n exactly once, interior tiles first;
//   * every 16-bit / 8-bit column code plus its tile's base reproduces the column;
//   * every vdict[vdesc.first + vidx] reproduces the value's bits.
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../new_cg_variants_amd/csrc/prcg_plan.h"

using namespace prcg;

struct Csr {
    int64_t n = 0, g = 0;
    std::vector<int32_t> ip{0}, col;
    std::vector<double> val;
    void push(int32_t c, double v) { col.push_back(c); val.push_back(v); }
    void end_row() { ip.push_back((int32_t)col.size()); ++n; }
};

static Csr laplace_2d(int nx, int ny) {
    Csr A;
    for (int j = 0; j < ny; ++j)
        for (int i = 0; i < nx; ++i) {
            const int r = j * nx + i;
            if (j > 0) A.push(r - nx, -1.0);
            if (i > 0) A.push(r - 1, -1.0);
            A.push(r, 4.0);
            if (i + 1 < nx) A.push(r + 1, -1.0);
            if (j + 1 < ny) A.push(r + nx, -1.0);
            A.end_row();
        }
    return A;
}

// rows [lo, lo + n) of an infinite band: columns left of the block are ghosts n .. n+6, right of it n+7 .. n+13
static Csr band_with_ghosts(int n) {
    Csr A;
    A.g = 14;
    for (int r = 0; r < n; ++r) {
        for (int d = -7; d <= 7; ++d) {
            const int c = r + d;
            const double v = d == 0 ? 2.5 : 1e-4 * (1 + (d < 0 ? -d : d));
            A.push(c < 0 ? n + 7 + c : (c >= n ? n + 7 + (c - n) : c), v);
        }
        A.end_row();
    }
    return A;
}

// nodes with 3 unknowns each; a node couples to itself and to a ragged set of neighbours through full 3 x 3 blocks
static Csr ragged_blocks(int nodes) {
    Csr A;
    std::mt19937 rng(7);
    for (int a = 0; a < nodes; ++a) {
        std::vector<int> nb{a};
        const int extra = (int)(rng() % 14);
        for (int e = 0; e < extra; ++e) {
            const int b = a + (int)(rng() % 41) - 20;
            if (b >= 0 && b < nodes) nb.push_back(b);
        }
        for (int i = 0; i < 3; ++i) {
            for (int b : nb)
                for (int j = 0; j < 3; ++j) A.push(3 * b + j, b == a && i == j ? 9.0 : -0.125 * (1 + (int)(rng() % 40)));
            A.end_row();
        }
    }
    return A;
}

static int failures = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { ++failures; fprintf(stderr, "FAIL %s: ", name); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); return; } } while (0)

static void check(const char* name, const Csr& A, const Options& o, bool expect_classic) {
    OperatorPlan pl;
    std::string err;
    const int64_t nnz = (int64_t)A.col.size();
    EXPECT(plan_operator(o, A.n, A.g, nnz, A.ip.data(), A.col.data(), A.val.data(), pl, err), "plan_operator: %s", err.c_str());
    EXPECT(!(pl.win && pl.sell), "two families at once");
    if (expect_classic) EXPECT(!pl.win && !pl.sell, "PRCG_WIN=0 / PRCG_SELL=0 did not select the CSR-adaptive tiles");
    // tile table: classes in order, rows covered once
    EXPECT((int64_t)pl.tiles.size() == (int64_t)pl.nt_int + pl.nt_bnd, "tile counts");
    std::vector<int> seen((size_t)A.n, 0);
    for (const Tile& t : pl.tiles) {
        EXPECT(t.row_begin >= 0 && t.row_begin <= t.row_end && t.row_end <= A.n, "tile rows [%d,%d)", t.row_begin, t.row_end);
        EXPECT(t.nnz_begin == A.ip[(size_t)t.row_begin] && t.nnz_end == A.ip[(size_t)t.row_end], "tile nonzeros");
        for (int r = t.row_begin; r < t.row_end; ++r) ++seen[(size_t)r];
    }
    for (int64_t r = 0; r < A.n; ++r) EXPECT(seen[(size_t)r] == 1, "row %lld in %d tiles", (long long)r, seen[(size_t)r]);
    if (pl.win) {
        EXPECT((int64_t)pl.wtiles.size() == (int64_t)pl.nwt_int + pl.nwt_bnd && !pl.wrel.empty(), "window tile counts");
        EXPECT(pl.win_pat ? !pl.pats.empty() : (pl.win_geom >= 2 ? !pl.wcw16.empty() : !pl.wcw8.empty()), "window index images");
    }
    if (pl.sell) EXPECT((int64_t)pl.sslices.size() == (int64_t)pl.nst_int + pl.nst_bnd && !pl.sp.val.empty(), "slice counts");
    // narrow column codes and the value dictionary of the CSR-adaptive tiles
    const int cap = tile_cap_nnz(pl.steps);
    EXPECT(pl.tbase.size() == pl.tiles.size() + 1, "tile bases");
    for (size_t ti = 0; ti < pl.tiles.size(); ++ti) {
        const Tile& t = pl.tiles[ti];
        const bool interior = (int)ti < pl.nt_int;
        if (t.nnz_end - t.nnz_begin > cap || t.nnz_end == t.nnz_begin) continue;       // long row / empty: not streamed
        const bool c16 = interior ? pl.c16_int : pl.c16_bnd, c8 = interior ? pl.c8_int : pl.c8_bnd, vd = interior ? pl.vd_int : pl.vd_bnd;
        if (c16) EXPECT(pl.c16.size() == (size_t)nnz + 8, "16-bit stream size");
        if (c8) EXPECT(pl.c8.size() == (size_t)nnz + 8, "8-bit stream size");
        if (vd) EXPECT(pl.vidx.size() == (size_t)nnz + 8 && pl.vdesc.size() == 2 * (pl.tiles.size() + 1), "dictionary sizes");
        for (int32_t q = t.nnz_begin; q < t.nnz_end; ++q) {
            if (c16) EXPECT((int32_t)pl.c16[(size_t)q] + pl.tbase[ti] == A.col[(size_t)q], "c16 of nonzero %d", q);
            if (c8) EXPECT((int32_t)pl.c8[(size_t)q] + pl.tbase[ti] == A.col[(size_t)q], "c8 of nonzero %d", q);
            if (vd) {
                const int32_t first = pl.vdesc[2 * ti], count = pl.vdesc[2 * ti + 1];
                EXPECT(count >= 1 && count <= kDictMax && pl.vidx[(size_t)q] < count && (size_t)first + count <= pl.vdict.size(), "dictionary of tile %zu", ti);
                EXPECT(memcmp(&pl.vdict[(size_t)first + pl.vidx[(size_t)q]], &A.val[(size_t)q], sizeof(double)) == 0, "value of nonzero %d", q);
            }
        }
    }
    if (expect_classic && A.n > 0) EXPECT(pl.c16_int && pl.vd_int, "the CSR-adaptive encodings were not built (c16 %d, dictionary %d)", pl.c16_int, pl.vd_int);
    printf("ok   %-28s family %d  tiles %d+%d  c16 %d/%d c8 %d/%d dict %d/%d  bytes %lld\n", name, pl.win ? 1 : (pl.sell ? 2 : 0), pl.nt_int, pl.nt_bnd,
           pl.c16_int, pl.c16_bnd, pl.c8_int, pl.c8_bnd, pl.vd_int, pl.vd_bnd, (long long)pl.bytes());
}

int main() {
    const Csr lap = laplace_2d(70, 45), band = band_with_ghosts(5000), blocks = ragged_blocks(900);
    Options def, classic;
    if (!apply_option(classic, "PRCG_WIN", "0") || !apply_option(classic, "PRCG_SELL", "0") || apply_option(classic, "PRCG_NO_SUCH", "1")) {
        fprintf(stderr, "FAIL apply_option\n");
        return 1;
    }
    check("laplace_2d", lap, def, false);
    check("laplace_2d PRCG_WIN=0", lap, classic, true);
    check("band+ghosts", band, def, false);
    check("band+ghosts PRCG_WIN=0", band, classic, true);
    check("ragged blocks", blocks, def, false);
    check("ragged blocks PRCG_WIN=0", blocks, classic, true);
    if (failures) { fprintf(stderr, "%d check(s) failed\n", failures); return 1; }
    return 0;
}
