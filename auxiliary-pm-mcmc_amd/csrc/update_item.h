// The entries of the trailing updates' lists (tile_lists.cpp) and the order in which a launch
// deals its work items to workgroups: what the host packs, the kernels unpack and a fused launch
// decodes, once. Plain C++ as well as HIP (tests/test_tile_lists_host.py and
// tests/test_update_item_host.py compile it with the host compiler). The checks of UPD_HOST_CHECK
// exist in host code only.
#pragma once
#include "apm_hd.h"

#ifdef __HIP_DEVICE_COMPILE__
#define UPD_HOST_CHECK(x) ((void)0)
#else
#include <assert.h>
#define UPD_HOST_CHECK(x) assert(x)
#endif
// (always inlined, as the kernels' own copies of these functions were)
#define UPD_HD APM_HD inline __attribute__((always_inline))

// Work item L of `total` -> its place in the XCD-aware order: workgroups are dealt round-robin
// over the 8 XCDs (MI355X_MICROARCH.md, dispatch), so XCD x = L % 8 is given the contiguous work
// range [x*q+min(x,r), ...) (bijective for any count). Consecutive work items are consecutive tiles
// of one chain in the host-built super-tile order (8x8 tiles: 8 row panels + 8 column panels =
// 2 MiB of operands per super-tile), so the operand panels a workgroup needs are in its XCD's L2.
UPD_HD long xcd_remap(long L, long total) {
    const long xcd = L & 7, q = total >> 3, r = total & 7;
    const long base = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
    return base + (L >> 3);
}

// The work item (chain b, list entry t) of workgroup `block` of an update launch of ntiles x
// nchains workgroups. fused_enabled: workgroups 0 .. nchains-1 (dispatched first) take entry 0,
// the diagonal tile (d, d) of chain b, and factor it after updating it (fused_diag, diag.h); the
// others take the remaining ntiles - 1 entries of every chain, XCD-aware. With ntiles == 1 every
// workgroup of the grid is a fused one and the other branch (nt = 0) is not evaluated.
struct UpdateItem {
    bool fused;
    int b, t;
};
UPD_HD UpdateItem update_item(long block, bool fused_enabled, int ntiles, int nchains) {
    if (fused_enabled && (int)block < nchains) return UpdateItem{true, (int)block, 0};
    const int nt = fused_enabled ? ntiles - 1 : ntiles;
    UPD_HOST_CHECK(nt > 0);
    const long w = xcd_remap(block - (fused_enabled ? nchains : 0), (long)nt * nchains);
    return UpdateItem{false, (int)(w / nt), (int)(w % nt) + (fused_enabled ? 1 : 0)};
}

// The packed entry formats, tile units throughout. Each entry names E x E tiles (row tiles
// i .. i+E-1, column tiles j .. j+E-1) of which it writes those with writes(a, c); an operand
// tile of an invalid row or column is replaced by a valid one of the same entry (no out-of-range
// reads), and what is computed from it is dropped.

// (i << 16) | j, 16 bits each: one 64x64 tile (k_chol_update, k_chol_update32)
struct Tile64 {
    static constexpr int E = 1;
    unsigned e;
    UPD_HD explicit Tile64(unsigned packed) : e(packed) {}
    UPD_HD static unsigned pack(int i, int j) {
        UPD_HOST_CHECK(0 <= i && i < (1 << 16) && 0 <= j && j < (1 << 16));
        return ((unsigned)i << 16) | (unsigned)j;
    }
    UPD_HD int i() const { return (int)(e >> 16); }
    UPD_HD int j() const { return (int)(e & 0xffff); }
    UPD_HD bool writes(int, int) const { return true; }
};

// (i << 18) | (j << 4) | rv0 | rv1 << 1 | cv0 << 2 | cv1 << 3, i and j 14 bits each: the 128x128
// super-tile of rows i, i+1 and columns j, j+1 with per-half validity (k_chol_update_t128,
// k_chol_update32_t128, k_rhs_row_update32)
struct SuperTile {
    static constexpr int E = 2;
    unsigned e;
    UPD_HD explicit SuperTile(unsigned packed) : e(packed) {}
    UPD_HD static unsigned pack(int i, int j, bool rv0, bool rv1, bool cv0, bool cv1) {
        UPD_HOST_CHECK(0 <= i && i < (1 << 14) && 0 <= j && j < (1 << 14));
        return ((unsigned)i << 18) | ((unsigned)j << 4) | (rv0 ? 1u : 0u) | (rv1 ? 2u : 0u) |
               (cv0 ? 4u : 0u) | (cv1 ? 8u : 0u);
    }
    UPD_HD int i() const { return (int)(e >> 18); }
    UPD_HD int j() const { return (int)((e >> 4) & 0x3fff); }
    UPD_HD bool rv(int a) const { return e & (1u << a); }
    UPD_HD bool cv(int c) const { return e & (4u << c); }
    UPD_HD bool writes(int a, int c) const { return rv(a) && cv(c) && j() + c <= i() + a; }
    // operand row tiles of the two row halves and of the two column halves
    UPD_HD int ra0() const { return rv(0) ? i() : i() + 1; }
    UPD_HD int ra1() const { return rv(1) ? i() + 1 : i(); }
    UPD_HD int cb0() const { return cv(0) ? j() : j() + 1; }
    UPD_HD int cb1() const { return cv(1) ? j() + 1 : j(); }
};

// (i << 20) | (j << 8) | rm << 4 | cm, i and j 12 bits each, rm / cm one validity bit per row /
// column tile: the 256x256 quad tile of rows i .. i+3 and columns j .. j+3 (k_chol_update32_q256)
struct QuadTile {
    static constexpr int E = 4;
    unsigned e;
    UPD_HD explicit QuadTile(unsigned packed) : e(packed) {}
    UPD_HD static unsigned pack(int i, int j, unsigned rm, unsigned cm) {
        UPD_HOST_CHECK(0 <= i && i < (1 << 12) && 0 <= j && j < (1 << 12) && rm < 16 && cm < 16);
        return ((unsigned)i << 20) | ((unsigned)j << 8) | (rm << 4) | cm;
    }
    UPD_HD int i() const { return (int)(e >> 20); }
    UPD_HD int j() const { return (int)((e >> 8) & 0xfff); }
    UPD_HD int rm() const { return (e >> 4) & 15; }
    UPD_HD int cm() const { return e & 15; }
    UPD_HD bool rv(int a) const { return (rm() >> a) & 1; }
    UPD_HD bool cv(int c) const { return (cm() >> c) & 1; }
    UPD_HD bool writes(int a, int c) const { return rv(a) && cv(c) && j() + c <= i() + a; }
    // operand tile of row a / column c
    UPD_HD int rt(int a) const { return rv(a) ? i() + a : i(); }
    UPD_HD int ct(int c) const { return cv(c) ? j() + c : j(); }
};
