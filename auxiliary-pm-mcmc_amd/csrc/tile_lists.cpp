// The tile lists every factorisation's trailing-update launches run over, one list entry per
// workgroup and chain (plain C++: built on the host, uploaded once per launch shape by
// host_chol64.cpp). All three cover the tiles (i, j) with i in [i0, R), j0 <= j <= min(i, jend-1),
// each exactly once. Packed entry formats:
//   tiles        (i << 16) | j                       one 64x64 tile (k_chol_update, k_chol_update32)
//   super-tiles  (i << 18) | (j << 4) | rv0 | rv1 << 1 | cv0 << 2 | cv1 << 3
//                rows i, i+1 and columns j, j+1 (tile units) with per-half validity; tile
//                (i+a, j+c) is written iff rv_a && cv_c && j+c <= i+a (k_chol_update_t128,
//                k_chol_update32_t128, k_rhs_row_update32)
//   quads        (I << 20) | (J << 8) | rmask << 4 | cmask
//                row tiles I .. I+3 and column tiles J .. J+3 with per-tile validity; tile
//                (I+a, J+c) is written iff rmask bit a, cmask bit c and J+c <= I+a
//                (k_chol_update32_q256)
#include "tile_lists.h"

#include <algorithm>

// tiles in super-tile order (SxS tiles, super-rows top-down, super-columns left-right, row-major
// inside), the rows of the gap [glo, ghi) left out
std::vector<unsigned> build_update_tiles(int i0, int R, int j0, int jend, int glo, int ghi) {
    std::vector<unsigned> v;
    const int S = 8;
    for (int I = i0; I < R; I += S)
        for (int J = j0; J < jend; J += S)
            for (int i = I; i < std::min(I + S, R); ++i) {
                if (i >= glo && i < ghi) continue;
                for (int j = J; j < std::min(J + S, jend); ++j)
                    if (j <= i) v.push_back(((unsigned)i << 16) | (unsigned)j);
            }
    return v;
}

// 128x128 super-tiles, the rows of the gap [glo, ghi) left out, in 4x4-super-tile blocks (the L2
// locality of build_update_tiles); super-tile rows start at i0, columns at j0; row tile solo (if
// >= 0) is never paired with another. Entries without any valid tile are omitted.
std::vector<unsigned> build_update_supertiles(int i0, int R, int j0, int jend, int glo, int ghi,
                                              int solo) {
    std::vector<unsigned> v;
    auto rowv = [&](int i) { return i < R && !(i >= glo && i < ghi); };
    const int S = 4;  // super-tiles per block edge (8x8 tiles, as build_update_tiles)
    std::vector<int> rows;  // first row tile of each super-tile row; rows[p] + 1 valid iff paired
    std::vector<bool> pair;
    for (int i = i0; i < R;) {
        const bool two = i != solo && i + 1 != solo;
        rows.push_back(i);
        pair.push_back(two);
        i += two ? 2 : 1;
    }
    const int nr = (int)rows.size(), nc = (jend - j0 + 1) / 2;
    for (int P = 0; P < nr; P += S)
        for (int Q = 0; Q < nc; Q += S)
            for (int p = P; p < std::min(P + S, nr); ++p)
                for (int q = Q; q < std::min(Q + S, nc); ++q) {
                    const int i = rows[p], j = j0 + 2 * q;
                    const bool rv0 = rowv(i), rv1 = pair[p] && rowv(i + 1);
                    const bool cv0 = j < jend, cv1 = j + 1 < jend;
                    bool any = false;
                    for (int a = 0; a < 2; ++a)
                        for (int c = 0; c < 2; ++c)
                            any |= (a ? rv1 : rv0) && (c ? cv1 : cv0) && j + c <= i + a;
                    if (!any) continue;
                    v.push_back(((unsigned)i << 18) | ((unsigned)j << 4) | (rv0 ? 1u : 0u) |
                                (rv1 ? 2u : 0u) | (cv0 ? 4u : 0u) | (cv1 ? 8u : 0u));
                }
    return v;
}

// 256x256 quad tiles in 2x2-quad blocks (8x8 tiles, the L2 locality of build_update_supertiles)
std::vector<unsigned> build_update_quads(int i0, int R, int j0, int jend) {
    std::vector<unsigned> v;
    const int nr = (R - i0 + 3) / 4, nc = (jend - j0 + 3) / 4, S = 2;
    for (int P = 0; P < nr; P += S)
        for (int Q = 0; Q < nc; Q += S)
            for (int p = P; p < std::min(P + S, nr); ++p)
                for (int q = Q; q < std::min(Q + S, nc); ++q) {
                    const int I = i0 + 4 * p, Jq = j0 + 4 * q;
                    unsigned rm = 0, cm = 0;
                    for (int a = 0; a < 4; ++a) {
                        if (I + a < R) rm |= 1u << a;
                        if (Jq + a < jend) cm |= 1u << a;
                    }
                    bool any = false;
                    for (int a = 0; a < 4; ++a)
                        for (int c = 0; c < 4; ++c)
                            any |= ((rm >> a) & 1) && ((cm >> c) & 1) && Jq + c <= I + a;
                    if (!any) continue;
                    v.push_back(((unsigned)I << 20) | ((unsigned)Jq << 8) | (rm << 4) | cm);
                }
    return v;
}
