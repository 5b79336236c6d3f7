// The fp64 two-level Cholesky schedule over 64 x 64 tiles (chol.hip), in its two forms, and the
// device-resident update lists every factorisation's trailing updates launch over.
#include "apm_host.h"

namespace apm_host {

double update_flops(int i0, int R, int j0, int jend, int kc, Gap g, bool syrk_lower) {
    double f = 0.0;
    for (int i = i0; i < R; ++i) {
        if (i >= g.lo && i < g.hi) continue;
        const int jmax = std::min(i, jend - 1);
        for (int j = j0; j <= jmax; ++j) {
            const int k = syrk_lower ? std::min(kc, j + 1) : kc;  // plus == 2: k <= j only
            f += (i == j) ? 64.0 * 65.0 * 64.0 * k : 2.0 * 64.0 * 64.0 * 64.0 * k;
        }
    }
    return f;
}

// ---- update lists per launch shape: looked up by key, else built, uploaded once
// (synchronously) and kept for the context's lifetime
namespace {
template <class Map, class Build>
DevList cached_list(apm_ctx* c, Map& lists, const typename Map::key_type& key, Build build) {
    auto it = lists.find(key);
    if (it != lists.end()) return it->second;
    const std::vector<unsigned> v = build();
    unsigned* d = dalloc<unsigned>(c, v.size());  // (an empty list still gets an element)
    if (!v.empty())
        HIPC(hipMemcpy(d, v.data(), sizeof(unsigned) * v.size(), hipMemcpyHostToDevice));
    return lists[key] = DevList(d, (int)v.size());
}
}  // namespace

DevList tile_list(apm_ctx* c, int i0, int R, int j0, int jend, Gap g) {
    return cached_list(c, c->tile_lists, std::make_tuple(i0, R, j0, jend, g.lo, g.hi),
                       [&] { return build_update_tiles(i0, R, j0, jend, g.lo, g.hi); });
}

DevList super_list(apm_ctx* c, int i0, int R, int j0, int jend, Gap g, int solo) {
    return cached_list(c, solo >= 0 ? c->super_lists_solo : c->super_lists,
                       std::make_tuple(i0, R, j0, jend, g.lo, g.hi), [&] {
                           return build_update_supertiles(i0, R, j0, jend, g.lo, g.hi, solo);
                       });
}

// the super-tiles of (i0, R, j0, jend) with row tile rhs alone, followed by that row's super-tiles
// of the columns [jend, jext): the next panel's columns of a lookahead update and the right-hand
// side row's far columns in one launch
DevList super_list_ext(apm_ctx* c, int i0, int R, int j0, int jend, int rhs, int jext) {
    return cached_list(c, c->super_lists_ext, std::make_tuple(i0, R, j0, jend, rhs, jext), [&] {
        std::vector<unsigned> v = build_update_supertiles(i0, R, j0, jend, 0, 0, rhs);
        const std::vector<unsigned> e =
            build_update_supertiles(rhs, rhs + 1, jend, jext, 0, 0, rhs);
        v.insert(v.end(), e.begin(), e.end());
        return v;
    });
}

DevList quad_list(apm_ctx* c, int i0, int R, int j0, int jend) {
    return cached_list(c, c->quad_lists, std::make_tuple(i0, R, j0, jend),
                       [&] { return build_update_quads(i0, R, j0, jend); });
}

// Trailing update of tiles (i, j), i in [i0, R) minus the gap, j in [j0, min(i, jend-1)], by
// columns [k0, k0+kc). fuse_k >= 0: the launch also factors diagonal tile (fuse_k, fuse_k), which
// must be its first tile (i0 == j0 == fuse_k; the super-tile order starts there).
void tracked_update(apm_ctx* c, MatB M, int k0, int kc, int i0, int R, int j0, int jend, Gap g,
                    int plus, int count, int fuse_k, int fail_code, const Exec* ex,
                    const MatB* src) {
    const Exec E = ex ? *ex : main_exec(c);
    if (i0 < j0) i0 = j0;
    if (update_tile_count(i0, R, j0, jend) <= 0) return;
    const bool t128 = kc >= 2 && jend - j0 >= 2 && (fuse_k < 0 || (i0 == fuse_k && j0 == fuse_k));
    if (src && (!t128 || plus == 2))  // (theta_eval_impl enables it only where it holds)
        throw HipError{"out-of-place update needs the fp64 t128 path"};
    const auto tl = tile_list(c, i0, R, j0, jend, g);
    if (tl.second <= 0) return;
    FusedDiag<double> fd{0, nullptr, 0, nullptr, 0, 0};
    if (fuse_k >= 0) fd = FusedDiag<double>{1, E.Dinv, c->dstride, E.ldet, c->lstride, fail_code};
    const double fl = c->prof ? update_flops(i0, R, j0, jend, kc, g, plus == 2) * E.live_n : 0.0;
    ProfScope ps(c, APM_PROF_CHOL_UPDATE, fl, E.s);
    ProfScope ps_outer(c, kc >= 2 && jend - j0 >= 2 ? APM_PROF_CHOL_UPDATE_OUTER : -1, fl, E.s);
    if (t128) {
        const auto sl = super_list(c, i0, R, j0, jend, g);
        launch_chol_update_t128(M, k0, kc, sl.first, sl.second, plus, E.lv, count, E.s, fd,
                                src ? *src : MatB{nullptr, 0, 0});
    } else {
        if (plus == 2) throw HipError{"identity-initialised update needs the t128 path"};
        launch_chol_update(M, k0, kc, tl.first, tl.second, plus != 0, E.lv, count, E.s, fd);
    }
}

// Two-level Cholesky over tile columns [k0, k1) of rows < R (tile units), the trailing matrix
// spanning columns < Cb. Outer panels of `outer` tiles are factored with 64-wide diag / panel /
// in-panel update steps; the rest of the matrix then receives one update of depth 64 * outer per
// outer panel (`outer` times less read-modify-write traffic than rank-64 steps). Inside a panel the schedule is
// left-looking: column k receives all of the panel's earlier columns in ONE update (depth
// (k-K)*64, one read-modify-write of its tiles instead of k-K). Every diagonal tile after the
// first is factored inside the update launch that completes it, as that launch's first tile
// (fused diag: its one-wave latency hides under that launch instead of idling the GPU between
// launches).
void chol_factor(apm_ctx* c, MatB M, int k0, int k1, int R, int Cb, int fail_code, int count,
                 const FactorOpts& o) {
    const Exec E = o.ex ? *o.ex : main_exec(c);
    bool have_diag = false;  // tile (K, K) already factored by the previous outer update
    for (int K = k0; K < k1; K += c->outer) {
        const int Kend = std::min(K + c->outer, k1);
        for (int k = K; k < Kend; ++k) {
            const Gap g = o.gap(k, c->nb);
            if (k > K)
                tracked_update(c, M, K, k - K, k, R, k, k + 1, g, false, count, k, fail_code, &E);
            else if (!have_diag)
                launch_chol_diag(M, k, E.Dinv, c->dstride, E.ldet, c->lstride, E.lv, fail_code,
                                 count, E.s);
            launch_chol_panel(M, k, k + 1, R, g.lo, g.hi, E.Dinv, c->dstride, E.lv, count, E.s);
        }
        if (o.after_panel) o.after_panel(K, Kend);
        have_diag = Kend < k1;
        tracked_update(c, M, K, Kend - K, Kend, R, Kend, Cb, o.gap(Kend - 1, c->nb), false, count,
                       have_diag ? Kend : -1, fail_code, &E, K == k0 ? o.first_src : nullptr);
    }
}

// The same schedule's solve-only form: the rows [row_start, R) against the existing factor in
// tile columns [0, k1), k1 <= row_start (L_kk and inv(L_kk) are reused: the top-left of an
// augmented matrix is already factored). Per column a panel solve and the rank-64 update of
// the rows' remaining columns of the outer panel, per outer panel one update of the rows'
// columns [Kend, Cb). Nothing is factored, so nothing can fail.
void chol_solve_rows(apm_ctx* c, MatB M, int k1, int row_start, int R, int Cb, int count,
                     const SolveOpts& o) {
    const Exec E = o.ex ? *o.ex : main_exec(c);
    for (int K = 0; K < k1; K += c->outer) {
        const int Kend = std::min(K + c->outer, k1);
        for (int k = K; k < Kend; ++k) {
            const Gap g = o.gap(k, c->nb);
            launch_chol_panel(M, k, row_start, R, g.lo, g.hi, E.Dinv, c->dstride, E.lv, count,
                              E.s);
            tracked_update(c, M, k, 1, row_start, R, k + 1, Kend, g, false, count, -1, 0, &E);
        }
        tracked_update(c, M, K, Kend - K, row_start, R, Kend, Cb, o.gap(Kend - 1, c->nb), false,
                       count, -1, 0, &E);
    }
}

}  // namespace apm_host
