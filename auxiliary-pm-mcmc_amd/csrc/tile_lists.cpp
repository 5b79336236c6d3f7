// The tile lists every factorisation's trailing-update launches run over, one list entry per
// workgroup and chain (plain C++: built on the host, uploaded once per launch shape by
// host_chol64.cpp). All three cover the tiles (i, j) with i in [i0, R), j0 <= j <= min(i, jend-1),
// each exactly once. The packed entry formats (Tile64, SuperTile, QuadTile) and which tiles an
// entry writes: update_item.h.
#include "tile_lists.h"

#include <algorithm>

#include "update_item.h"

template <class Entry>
static bool writes_any(const Entry& e) {
    for (int a = 0; a < Entry::E; ++a)
        for (int c = 0; c < Entry::E; ++c)
            if (e.writes(a, c)) return true;
    return false;
}

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
                    if (j <= i) v.push_back(Tile64::pack(i, j));
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
                    const SuperTile e(SuperTile::pack(i, j, rowv(i), pair[p] && rowv(i + 1),
                                                      j < jend, j + 1 < jend));
                    if (writes_any(e)) v.push_back(e.e);
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
                    const QuadTile e(QuadTile::pack(I, Jq, rm, cm));
                    if (writes_any(e)) v.push_back(e.e);
                }
    return v;
}
