// Internal launcher interface between the kernel translation units and the host orchestration
// (host_*.cpp, capi.cpp; their shared declarations are in apm_host.h).
// Nothing here is part of the public C-ABI (include/apm.h).
#pragma once
#include <string>

#include "apm_common.h"
#include "tile_lists.h"  // the update lists the launchers below run over (plain C++)
#include "tri_index.h"   // lower_tri_index (plain C++ as well)
#include "update_item.h"  // the lists' entry formats and the work-item order (plain C++ as well)

// A batched fp64 matrix: chain b's element (r, c) lives at base[b*cstride + r*ld + c].
struct MatB {
    double* base;
    int64_t ld;
    int64_t cstride;
};

// The same for fp32 (the fp32 factorisations: chol32_panel.hip, chol32_update.hip).
struct MatF {
    float* base;
    int64_t ld;
    int64_t cstride;
};

// Per-chain liveness: a kernel does work for chain b iff active[b] != 0 && status[b] == 0.
struct Live {
    const int* active;
    int* status;
};
__device__ __forceinline__ bool live_chain(const Live& lv, int b) {
    return lv.active[b] != 0 && lv.status[b] == 0;
}

// ---- chol.hip -------------------------------------------------------------------------------
// Blocked right-looking Cholesky building blocks over TB x TB tiles (lower triangle).
// diag:   factor tile (k,k) in place, write its inverse to Dinv[b][k] and sum(log diag) to
//         ldet[b][k]; a non-positive pivot sets status[b] = fail_code.
// panel:  tiles (i,k), i in [i0, R):  A_ik <- A_ik * inv(L_kk)^T     (f64 MFMA)
// update: tiles (i,j), i in [i0, R), j0 <= j <= min(i, jend-1):
//         A_ij -= sum_{q<kc} A_{i,k0+q} A_{j,k0+q}^T  (f64 MFMA, rank 64*kc)
void launch_chol_diag(MatB A, int k, double* Dinv, int64_t dstride, double* ldet, int64_t lstride,
                      Live live, int fail_code, int nchains, hipStream_t s);
// panel rows [i0, R) minus the row tiles [glo, ghi) (pass glo = ghi = R for none)
void launch_chol_panel(MatB A, int k, int i0, int R, int glo, int ghi, const double* Dinv,
                       int64_t dstride, Live live, int nchains, hipStream_t s);
// Optional diag step fused into an update launch (the launch's tiles[0] is the diagonal tile
// (d, d); Dinv / ldet / status are written as by launch_chol_diag for k = d).
template <class TS>
struct FusedDiag {
    int enabled;
    TS* Dinv;
    int64_t dstride;
    double* ldet;
    int64_t lstride;
    int fail_code;
};
// tiles: device list built by build_update_tiles (tile_lists.cpp)
// plus = true adds instead of subtracting (SYRK of the UL factorisation, postcov.hip)
void launch_chol_update(MatB A, int k0, int kc, const unsigned* tiles, int ntiles, bool plus,
                        Live live, int nchains, hipStream_t s,
                        FusedDiag<double> fd = FusedDiag<double>{0, nullptr, 0, nullptr, 0, 0});
// the same with one 128x128 super-tile per workgroup (tiles from build_update_supertiles)
// plus: 0 A -= ..., 1 A += ..., 2 A = I + Y Y^T for lower-triangular Y (depth per tile column
// truncated to the nonzero blocks; the old tile is not read). S.base: the old tiles are read from
// S (same tile coordinates, own ld / chain stride) instead of A - an out-of-place update
void launch_chol_update_t128(MatB A, int k0, int kc, const unsigned* tiles, int ntiles, int plus,
                             Live live, int nchains, hipStream_t s,
                             FusedDiag<double> fd = FusedDiag<double>{0, nullptr, 0, nullptr, 0, 0},
                             MatB S = MatB{nullptr, 0, 0});
long update_tile_count(int i0, int R, int j0, int jend);
// launch_chol_diag on an fp32 matrix: the first diagonal tile of an fp32 factorisation
void launch_chol_diag32(MatF A, int k, float* Dinv, int64_t dstride, double* ldet,
                        int64_t lstride, Live live, int fail_code, int nchains, hipStream_t s);
// one step (block J) of the backward solve L^T z = r, r stored in row `rrow` of A (in place),
// z written to z[b*zstride + ...]
void launch_trsv_lt_step(MatB A, int J, int64_t rrow, const double* Dinv, int64_t dstride,
                         double* z, int64_t zstride, Live live, int nchains, hipStream_t s);
// empty kernel k_apm_marker<id> (trace bracketing, apm_prof_marker)
void launch_marker(int id, hipStream_t s);
// test hook: C(64x64) = A(64x64) * B(64x64)^T through the MFMA tile path
void launch_tile_nt_test(const double* A, const double* B, double* C, hipStream_t s);
void launch_philox_test(const uint32_t* in, uint32_t* out, int64_t n, hipStream_t s);

// ---- the fp32 factorisations and the mixed-precision Newton solve: shared types -------------
// Bounded in-launch hand-overs of the Newton solve (k_chol_panel_df32, k_trsv32_mw). HIP promises
// no dispatch order, so a workgroup's logical index is the ticket it draws from a monotonic
// arrival counter when it starts (a ticket exists only for a workgroup that is running): a
// dataflow row then waits only on rows that have arrived, and of the TRSV's chains only the one
// holding the newest ticket can wait on a workgroup that has not. Every wait is bounded by
// `limit` polls; a bounded exit is counted in *timeouts and fails its chain (the Newton loop
// reruns it in fp64), so it can cost time but never a value.
struct SpinCtl {
    unsigned long long* ticket;    // arrival counter, shared by the launches of one stream
    unsigned long long base;       // its value before this launch (host-side running total)
    unsigned long long* timeouts;  // bounded-spin exits (APM_PROF_DF / _TRSV_TIMEOUTS)
    int limit;                     // polls before a wait gives up
};
// fp16x3 operand planes of one outer panel of the Newton matrix (tile32.h): for each 32-column
// slice s of the panel and row r < rows, hi = fp16(x) and lo = fp16(x - hi) of the row's 32
// entries (64 bytes each), hi at base + b * cstride + (s * rows + r) * 32 and lo at + lo (fp16
// bit patterns). Written by the dataflow panel kernel for the rows below the panel's diagonal
// block; the trailing update then stages them into LDS with DMA instead of splitting fp32
// operands in registers. base == nullptr: no planes.
struct Planes16 {
    unsigned short* base;
    int64_t cstride;
    int64_t lo;
    int rows;
};

// ---- chol32_panel.hip: in-panel steps of the fp32 factorisations ----------------------------
// tile columns [K, K+ncols) of an outer panel (diagonal tile (K, K) already factored) in one
// dataflow launch (per-(chain, row) progress words prog[b * pstride + row], monotonic
// base per factorisation and panel); returns the launch's workgroup count (its tickets), 0 when
// nothing was launched, -1 for a panel wider than the progress word allows. pl.base != nullptr:
// the rows below the diagonal block (row tiles < pl.rows / 64) also write the panel's planes.
// inv_skip (per chain): that chain's rows below the diagonal block return at once (its
// explicit-inverse panel follows)
long launch_chol_panel_df32(MatF A, int K, int ncols, int R, FusedDiag<float> fd, Live live,
                            int nchains, int hlim, const int* h3ok, unsigned long long* prog,
                            int64_t pstride, unsigned long long base, SpinCtl sc, hipStream_t s,
                            Planes16 pl = Planes16{nullptr, 0, 0, 0}, int rhs_as = -1,
                            const int* inv_skip = nullptr);
// explicit-inverse panel of the Newton factorisation, after a dataflow launch over
// the diagonal block [K, K+8) and the right-hand-side row (rhs_as): Z = inv(L_D) of the 512x512
// diagonal block as fp16x3 planes (zpl, 512 rows), by recursive doubling over fp32 scratch (zt:
// 3 x 512 x 512 per chain, zstride floats apart); then every row tile i in [K+8, nb) becomes
// X_i = A_i Z^T in one fp16x3 GEMM (in place, plus the panel's planes pl). Only the chains
// flagged in `ok` (the host's invok: 1 + K_ii < 2^15, so the split Schur-complement entries fit
// fp16's range).
void launch_panel_inv32(MatF A, int K, int nb, const float* Dinv, int64_t dstride, float* zt,
                        int64_t zstride, Planes16 zpl, Planes16 pl, Live live, int nchains,
                        const int* h3ok, hipStream_t s);
// rows [row0, R) of an outer panel [K, K+ncols) whose diagonal block is final (fd.Dinv: its
// inverses), each row a left-looking walk over the panel's columns with no waits; zrow > 0: row
// tile i is zero in the tile columns < zrow - 1 - i (postcov.hip's fp32 bottom block)
void launch_chol_panel_bulk32(MatF A, int K, int ncols, int row0, int R, int zrow,
                              FusedDiag<float> fd, Live live, int nchains, int hlim,
                              const int* h3ok, hipStream_t s,
                              Planes16 pl = Planes16{nullptr, 0, 0, 0});

// ---- chol32_update.hip: trailing updates of the fp32 factorisations -------------------------
void launch_chol_update32(MatF A, int k0, int kc, const unsigned* tiles, int ntiles, Live live,
                          int nchains, hipStream_t s,
                          FusedDiag<float> fd = FusedDiag<float>{0, nullptr, 0, nullptr, 0, 0},
                          int hlim = 0, const int* h3ok = nullptr);
// the same update with one 128x128 super-tile per workgroup (tiles from build_update_supertiles);
// hlim > 0: fp16x3 operands for super-tiles whose rows lie below row tile hlim, in the chains b
// with h3ok[b] != 0 (h3ok == nullptr: every chain); the others take fp32 operands.
// rhs >= 0: row tile rhs is the appended right-hand side whose first row alone is data (its
// super-tiles must hold it alone: build_update_supertiles(..., solo = rhs)); it is updated as a
// row-vector product (fp64 accumulation) instead of a 64-row tile product.
// role: which launch population this is (the kernel's ROLE: each has its own instantiation and so
// its own profiler figures). The caller states it; pl (k0's panel's planes) goes with
// UPD32_NEWTON_PLANES and with no other role, else the launcher throws.
enum {
    UPD32_NEWTON = 0,         // the Newton factorisation, fp16x3 operands split while staged
    UPD32_POST = 1,           // the posterior factor's bottom block (same code)
    UPD32_NEWTON_PLANES = 2,  // the Newton factorisation, fp16x3 operands from the planes
};
void launch_chol_update32_t128(MatF A, int k0, int kc, const unsigned* tiles, int ntiles,
                               Live live, int nchains, hipStream_t s,
                               FusedDiag<float> fd = FusedDiag<float>{0, nullptr, 0, nullptr, 0, 0},
                               int hlim = 0, const int* h3ok = nullptr, int rhs = -1,
                               int role = UPD32_NEWTON, Planes16 pl = Planes16{nullptr, 0, 0, 0});
// the far trailing updates of the fp32 factorisations on 256x256 quad tiles: fp16x3 operands
// from the planes only, rows below the appended right-hand side, chains with h3ok set
// (role: UPD32_NEWTON or UPD32_POST). npan > 1 (UPD32_NEWTON only): the depth is that of npan
// consecutive outer panels of kc tiles, pl the first one's planes and the next ones' pstep
// entries further on each
void launch_chol_update32_q256(MatF A, int k0, int kc, const unsigned* quads, int nq, Live live,
                               int nchains, hipStream_t s, const int* h3ok, Planes16 pl,
                               int role = UPD32_NEWTON, int npan = 1, int64_t pstep = 0);
// the appended right-hand-side row beside the quad tiles, whose lists stop above it: tiles = the
// super-tiles of row tile rhs alone (build_update_supertiles(rhs, rhs + 1, ..., solo = rhs))
void launch_rhs_row_update32(MatF A, int k0, int kc, const unsigned* tiles, int ntiles, Live live,
                             int nchains, hipStream_t s);

// ---- newton_solve.hip: K b, TRSV and fp64 refinement of the mixed-precision Newton solve ----
// y = K x from K's lower tiles (part: nb*nb*64 doubles per chain of partials); Bf.base != null
// also forms the fp32 Newton matrix I + W^1/2 K W^1/2 and its right-hand-side block (x = b)
void launch_symv(MatB K, const double* x, int64_t xstride, double* y, int64_t ystride,
                 double* part, int64_t pstride, int np, MatF Bf, const double* Ws,
                 int64_t wstride, Live live, int nchains, hipStream_t s, int symv_tpw = 1);
void launch_row32(MatF Bf, int64_t row, int np, double* out, int64_t ostride, Live live,
                  int nchains, hipStream_t s);
// blocked TRSV steps with fp32 tiles / inverses and fp64 vectors (r updated in place)
void launch_trsv_fwd32(MatF A, int J, int nb, const float* Dinv, int64_t dstride, double* r,
                       double* y, int64_t vstride, Live live, int nchains, hipStream_t s);
void launch_trsv_bwd32(MatF A, int J, const float* Dinv, int64_t dstride, double* r, double* z,
                       int64_t vstride, Live live, int nchains, hipStream_t s);
// the whole solve in one launch over TRM_G workgroups per chain (k_trsv32_mw; NaN-fills `out`
// first; fp64 r -> out, r kept); needs np <= 8192 (trsv32_mw_ok), else the per-block steps above
bool trsv32_mw_ok(int np);
void trsv32_mw_init();  // per device, once the device is current (apm_create)
// returns the launch's workgroup count (its tickets)
long launch_trsv32_mw(bool fwd, MatF A, int nb, const float* Dinv, int64_t dstride,
                      const double* r, double* out, int64_t vstride, Live live, int nchains,
                      int fail_code, SpinCtl sc, hipStream_t s);
// refinement vector ops (mode 0: out = Ws x; 1: out = Ws Kb - x - Ws Kt; 2: x += out)
// acceptance of refinement step `step` on the chains with refining[b] != 0 && status[b] == 0:
// accepted chains leave the mask; with last = true the others get status = fail_code
void launch_refine_check(const double* x, const double* d, int64_t vstride, int np, double tol,
                         int fail_code, int step, bool last, double* prev, int* refining,
                         const int* status, int nchains, hipStream_t s);
// refining[b] = chain b live
void launch_refine_mask(Live live, int* refining, int nchains, hipStream_t s);
void launch_refine(int mode, const double* Ws, const double* Kb, double* x, const double* Kt,
                   double* out, int64_t vstride, int np, Live live, int nchains, hipStream_t s);

// ---- covariance kinds -----------------------------------------------------------------------
// The one place that reads an APM_KERNEL_* value of include/apm.h: a kind the device builds is a
// (family, iso / ARD) pair; everything else (APM_KERNEL_PRECOMPUTED, unknown values) is not.
//   SE          S = s exp(-r^2 / 2)                                G = S
//   Matern 3/2  S = s (1 + sqrt3 r) exp(-sqrt3 r)                  G = 3 s exp(-sqrt3 r)
//   Matern 5/2  S = s (1 + sqrt5 r + 5/3 r^2) exp(-sqrt5 r)        G = 5/3 s (1 + sqrt5 r) exp(-sqrt5 r)
// with r^2 = sum_k ((x_ik - x_jk)/tau_k)^2, s = exp(theta_0), tau_k = exp(theta_{k+1}) (ARD) or
// exp(theta_1) for every k (iso); dK/dtheta_{k+1} = G ((x_ik - x_jk)/tau_k)^2 (gradient.hip).
// APM_COV_BIAS (16) OR-ed onto one of the six: K = S + beta 1 1^T + eps I on the data pairs, beta =
// exp of theta's last entry; dK/dtheta_{P-1} = beta on every data pair.
// APM_COV_LINEAR (64) OR-ed onto an SE kind, with or without the bias: K = S [+ beta] + lambda x x^T
// + eps I on the data pairs (the raw inputs' dot products), lambda = exp of theta's last entry and
// beta = exp of the one before it; dK/dtheta_{P-1} = lambda x_i . x_j.
enum { APM_FAM_SE = 0, APM_FAM_M32 = 1, APM_FAM_M52 = 2 };
struct KernelKind {
    int family;  // APM_FAM_*, -1: not built on the device
    int iso;     // one length scale (theta has 2 entries) instead of d (d + 1 entries)
    int bias;    // the constant term: one more theta entry (the last, or the one before lambda's)
    int linear;  // the linear term (SE only): one more theta entry, the last
    bool on_device() const { return family >= 0; }
    int64_t theta_len(int64_t d) const {
        return family < 0 ? 0 : (iso ? 2 : d + 1) + bias + linear;
    }
};
inline KernelKind kernel_kind_of(int kind) {
    const int bias = (kind & 16) ? 1 : 0;    // APM_COV_BIAS
    const int linear = (kind & 64) ? 1 : 0;  // APM_COV_LINEAR
    switch (kind & ~(16 | 64)) {
        case 0: return KernelKind{APM_FAM_SE, 1, bias, linear};  // APM_KERNEL_ISO
        case 1: return KernelKind{APM_FAM_SE, 0, bias, linear};  // APM_KERNEL_ARD
        default: break;
    }
    if (linear) return KernelKind{-1, 0, 0, 0};  // (a Matern kind has no linear instantiation)
    switch (kind & ~16) {
        case 3: return KernelKind{APM_FAM_M32, 1, bias, 0};  // APM_KERNEL_M32_ISO
        case 4: return KernelKind{APM_FAM_M32, 0, bias, 0};  // APM_KERNEL_M32_ARD
        case 5: return KernelKind{APM_FAM_M52, 1, bias, 0};  // APM_KERNEL_M52_ISO
        case 6: return KernelKind{APM_FAM_M52, 0, bias, 0};  // APM_KERNEL_M52_ARD
        // APM_KERNEL_PRECOMPUTED (with or without a flag) and unknown values
        default: return KernelKind{-1, 0, 0, 0};
    }
}
// the launchers' dispatch on the family, the constant and the linear term (template parameters of
// k_gram, k_gram_cross and k_grad_reduce: their epilogues differ, everything else is shared). The
// linear term exists for the SE family only: inside a Matern case LIN is false whatever the flag.
#define APM_FAMILY_DISPATCH(family, ...)                                           \
    switch (family) {                                                              \
        case APM_FAM_M32: { constexpr int FAM = APM_FAM_M32; __VA_ARGS__; } break; \
        case APM_FAM_M52: { constexpr int FAM = APM_FAM_M52; __VA_ARGS__; } break; \
        default: { constexpr int FAM = APM_FAM_SE; __VA_ARGS__; } break;           \
    }
#define APM_BIAS_DISPATCH(bias, ...)                        \
    if (bias) { constexpr bool BIAS = true; __VA_ARGS__; }  \
    else { constexpr bool BIAS = false; __VA_ARGS__; }
#define APM_LINEAR_DISPATCH(linear, ...)                                       \
    if (linear) { constexpr bool LIN = FAM == APM_FAM_SE; __VA_ARGS__; }       \
    else { constexpr bool LIN = false; __VA_ARGS__; }
#ifdef __HIPCC__
// the covariance function of the pair's scaled squared distance r2, family FAM
template <int FAM>
__device__ __forceinline__ double cov_S(double sigma, double r2) {
    if constexpr (FAM == APM_FAM_SE) {
        return sigma * exp(-0.5 * r2);
    } else if constexpr (FAM == APM_FAM_M32) {
        const double t = 1.7320508075688772 * sqrt(r2);
        return sigma * ((1.0 + t) * exp(-t));
    } else {
        const double t = 2.23606797749979 * sqrt(r2);
        return sigma * ((1.0 + t + (5.0 / 3.0) * r2) * exp(-t));
    }
}
// the Matern families' length-scale weight G (the SE family's is S itself)
template <int FAM>
__device__ __forceinline__ double cov_G(double sigma, double r2) {
    static_assert(FAM == APM_FAM_M32 || FAM == APM_FAM_M52, "SE: G = S");
    if constexpr (FAM == APM_FAM_M32) {
        const double t = 1.7320508075688772 * sqrt(r2);
        return (3.0 * sigma) * exp(-t);
    } else {
        const double t = 2.23606797749979 * sqrt(r2);
        return ((5.0 / 3.0) * sigma) * ((1.0 + t) * exp(-t));
    }
}
#endif

// ---- gram.hip -------------------------------------------------------------------------------
// K[b] (np x np, identity-padded beyond n) from X (n x d, row-major, ldx) and theta[b]
// kind: an APM_KERNEL_* value with kernel_kind_of(kind).on_device() (SE: kernels.pyx:12-49, :52-90)
// both: write both triangles (else K's lower tiles only); K2.base: the lower tiles of tile
// columns < k2cols also to K2 (direct-form distances on the fp64 VALU, k_gram)
void launch_gram(MatB K, const double* X, int64_t ldx, int n, int d, const double* theta,
                 int64_t tstride, int kind, double eps, int np, Live live, int nchains,
                 hipStream_t s, bool both, MatB K2 = MatB{nullptr, 0, 0}, int k2cols = 1 << 30);

// ---- predict.hip: Laplace predictive at test inputs -----------------------
// Cross-covariance of the ms test points Xs (row-major, ld = d) against the n training points,
// k*_rc = s exp(-1/2 sum_k ((xs_rk - x_ck)/tau_k)^2) (no epsilon: kernels.pyx adds it for i == j
// of one point set only; s = sig[b] = exp(theta_0) computed by the host), for the 64-row tiles [0, mb) of the block, k_gram's arithmetic.
// plain == 0 (the predictive path): chain b's A rows [row0, row0 + 64 mb), columns [0, 64 nb),
// <- k*_rc Ws[c], exact zeros for rows >= ms and columns >= n; part[b * pstride + tj * 64 mb + r]
// <- sum of k*_rc a_c over the columns of tile column tj (summed in order by k_predict_reduce).
// plain != 0 (apm_gram_cross): out.base[r * out.ld + c] <- k*_rc for r < ms, c < n, one chain,
// nothing else is touched (Ws, a, part, live may be null).
// A biased kind adds bet[b] = exp(theta_{P-1}), the host's as sig[b] is, to every k*_rc with
// r < ms, c < n (bet is not read otherwise and may be null). A kind with the linear term adds
// lam[b] xs_r . x_c (lam[b] the host's exp of theta's last entry; not read otherwise, may be null).
void launch_gram_cross(MatB out, int64_t row0, const double* Xs, int ms, int mb, const double* X,
                       int64_t ldx, int n, int d, int nb, const double* theta, int64_t tstride,
                       const double* sig, const double* bet, const double* lam, int kind,
                       const double* Ws, const double* a, int64_t vstride, double* part,
                       int64_t pstride, Live live, int plain, int nchains, hipStream_t s);
// per chain and test row r < ms: mean = sum_tj part[tj][r] (in order), var = sig[b] - |row r of V^T|^2
// over columns [0, 64 nb) of A's rows [row0, ..), prob = Phi(mean / sqrt(1 + var)); each output
// out[b * ostride + r]. Nothing is clamped. sig[b] is the prior variance k** here (and in
// launch_is_rows): s, or s + beta of a biased kind. lam != null (a kind with the linear term):
// k** = sig[b] + lam[b] xsn[r], xsn the test rows' squared norms; a null lam reads neither.
// lik (APM_LIK_*): the logit's prob is the Gauss-Hermite average of sigma (gh_table.h)
void launch_predict_reduce(int lik, MatB A, int64_t row0, int ms, int mb, int nb,
                           const double* sig, const double* lam, const double* xsn,
                           const double* part, int64_t pstride, double* mean, double* var,
                           double* prob, int64_t ostride, Live live, int nchains, hipStream_t s);

// ---- predict_joint.hip: joint Laplace / EP predictive at test inputs --------
// The block: chain b's A rows and columns [row0, row0 + 64 mb), the free rows behind the factor.
// Its lower tiles <- the test-test Gram of the ms staged test inputs Xs (row-major, ld = d), k**
// on the diagonal, no epsilon; the identity beyond ms. sig / bet / lam as launch_gram_cross.
void launch_gram_test(MatB A, int64_t row0, const double* Xs, int ms, int mb, int d,
                      const double* theta, int64_t tstride, const double* sig, const double* bet,
                      const double* lam, int kind, Live live, int nchains, hipStream_t s);
// eps onto the block's ms real diagonal entries
void launch_joint_eps(MatB A, int64_t row0, int ms, double eps, Live live, int nchains,
                      hipStream_t s);
// xi[b * xstride + r * ldx + j] <- element j S + r of the normal stream (seeds[b], counters[b]),
// r < S, j < ms (philox.h); nothing else is written
void launch_joint_normal(double* xi, int64_t xstride, int64_t ldx, const uint64_t* seeds,
                         const uint64_t* counters, int ms, int S, Live live, int nchains,
                         hipStream_t s);
// f[r][j] = mean[b * mstride + j] + sum_k xi[r][k] L[j][k], L the block's lower factor (zeros above
// the diagonal), xi sp = 64 ceil(S / 64) rows of ldx >= 64 mb doubles with zeros beyond (S, ms):
// draws[b * dstride + r * ms + j] <- f (r < S, j < ms) unless null; with labels ys (ms, +-1)
// part[b * pstride + tj * sp + r] <- sum over the columns j < ms of tile tj of log p(ys_j | f[r][j])
// (lik: APM_LIK_*), else part is not written
void launch_joint_draw(int lik, MatB A, int64_t row0, int ms, int mb, const double* xi,
                       int64_t xstride, int64_t ldx, int S, int sp, const double* mean,
                       int64_t mstride, const double* ys, double* draws, int64_t dstride,
                       double* part, int64_t pstride, Live live, int nchains, hipStream_t s);
// out[b] = logsumexp_{r < S} sum_{tj < mb} part[b * pstride + tj * sp + r] - log S (is_lme)
void launch_joint_lme(const double* part, int64_t pstride, int mb, int S, int sp, double* out,
                      Live live, int nchains, hipStream_t s);

// ---- gradient.hip: gradient of the Laplace LML w.r.t. theta ---------------
// per chain and row r < 64 nb: dS = K_rr - |row np + r of A over columns [0, 64 nb)|^2,
// g = y phi(f)/Phi(y f), s2 = 1/2 dS d3 (third derivative of log p at f); zeros for r >= n.
// Each output out[b * gstride + r]; f per chain with stride vstride. lik (APM_LIK_*): g and d3
// are the likelihood's (lik_grad_d3, apm_common.h)
void launch_grad_rows(int lik, MatB A, MatB K, int n, int nb, const double* f, const double* y,
                      int64_t vstride, double* dS, double* g, double* s2, int64_t gstride,
                      Live live, int nchains, hipStream_t s);
// A's rows [np, 2np) x columns [0, np) <- diag(Ws) (whole tiles), and zeros in the lower tiles of
// the bottom-right block
void launch_grad_fill(MatB A, const double* Ws, int64_t vstride, int nb, Live live, int nchains,
                      hipStream_t s);
// q = s2 + u for rows < n, zero beyond
void launch_grad_q(const double* s2, const double* u, double* q, int64_t gstride, int n, int np,
                   Live live, int nchains, hipStream_t s);
// part[b * pstride + t * P + j] <- super-tile t's share of sum_ik M_ik (dK/dtheta_j)_ik with
// M = 1/2 a a^T + 1/2 Rn + 1/2 (q g^T + g q^T) (Rn = -R, lower tiles) and S from K's lower tiles
// off the diagonal, exp(theta_0) on it; t over the ns (ns + 1) / 2 lower super-tiles, ns =
// ceil(nb / 2). launch_grad_sum adds them in tile order into grad[b * P + j]. A biased kind's K
// tiles hold S + beta: its SE instantiation forms S from the pair's own r^2, its Matern ones take
// K - beta; both write beta sum_ik M_ik as entry P - 1. A kind with the linear term (SE only) takes
// the biased SE route, writes beta's entry at P - 2 and lambda sum_ik M_ik x_i . x_k as entry
// P - 1 from a kernel of its own (k_grad_lin).
void launch_grad_reduce(MatB K, MatB Rn, const double* X, int64_t ldx, int n, int d, int nb,
                        const double* theta, int64_t tstride, int kind, const double* a,
                        int64_t vstride, const double* q, const double* g, int64_t gstride,
                        double* part, int64_t pstride, int P, Live live, int nchains,
                        hipStream_t s);
void launch_grad_sum(const double* part, int64_t pstride, int nst, int P, double* grad, Live live,
                     int nchains, hipStream_t s);

// ---- newton.hip -----------------------------------------------------------------------------
struct NewtonVecs {     // all per chain, stride vstride (>= np)
    double* f;          // current mode estimate
    double* fnew;
    double* W;          // W_diag
    double* Ws;         // W_diag^1/2
    double* b;          // W f + grad
    double* Kb;         // K b, later reused
    double* a;          // b - W^1/2 z
    double* z;          // TRSV result
    int64_t vstride;
};
// lik (APM_LIK_*, apm_common.h): the likelihood whose grad / W / log p the launch evaluates
void launch_newton_prep(int lik, NewtonVecs v, const double* y, int n, int np, Live live,
                        int nchains, hipStream_t s);
void launch_gemv(MatB M, const double* x, int64_t xstride, double* out, int64_t ostride, int np,
                 Live live, int nchains, hipStream_t s);
void launch_form_B(MatB K, MatB A, NewtonVecs v, int np, Live live, int nchains, hipStream_t s);
void launch_newton_update(NewtonVecs v, int np, Live live, int nchains, hipStream_t s);
void launch_newton_check(NewtonVecs v, int n, int np, double tol, int* active, const int* status,
                         int* n_iter, int nchains, hipStream_t s);
void launch_copy_lower(MatB src, MatB dst, int np, Live live, int nchains, hipStream_t s);
void launch_form_aug(MatB K, MatB A, NewtonVecs v, int np, Live live, int nchains,
                     hipStream_t s, bool lower_only = false);
// per chain: out[b] = -0.5 a.f + sum_n log p(y|f) - 0.5*sum(ldet[0..nb))*2
void launch_laplace_lml(int lik, NewtonVecs v, const double* y, int n, const double* ldet,
                        int64_t lstride, int nb, double* out, Live live, int nchains,
                        hipStream_t s);

// ---- ep.hip: parallel expectation propagation for the probit ----------------
struct EpVecs {         // all per chain, stride `stride` (>= np), but logz (one per chain)
    double* tau;        // site precisions tau~ (zero for rows >= n)
    double* nu;         // site precision-means nu~
    double* ctau;       // the damped candidates of the current sweep
    double* cnu;
    double* var;        // marginal variances sigma^2 of the current sweep
    double* lz;         // the rows' terms of log Z_EP
    double* dm;         // (mu - mu_prev)^2
    double* logz;       // log Z_EP of a converged chain
    int* bad;           // the row's cavity precision was <= 0 or not finite
    int64_t stride;
};
// W = tau~, W^1/2 = sqrt(tau~) and b = nu~ into the Newton vectors
void launch_ep_prep(EpVecs e, NewtonVecs v, int np, Live live, int nchains, hipStream_t s);
// per chain and row r < n, from row np + r of A over columns [0, 64 nb) (the solved row of V^T),
// K_rr, mu = v.fnew and mu_prev = v.f: var, the damped candidate sites, lz, dm and bad
void launch_ep_sites(MatB A, MatB K, int n, int nb, NewtonVecs v, const double* y, EpVecs e,
                     double damping, Live live, int nchains, hipStream_t s);
// launch_ep_sites with the tilted moments of likelihood lik (APM_LIK_*) by the quadrature rule
// of ep_quad.h: lz carries log Z^ for log Phi(z), and bad is also set at a site
// outside the rule's covered region
void launch_ep_sites_q(int lik, MatB A, MatB K, int n, int nb, NewtonVecs v, const double* y,
                       EpVecs e, double damping, Live live, int nchains, hipStream_t s);
// per live chain: n_iter += 1; a bad cavity -> status = fail_code; from the second sweep on
// mean(dm) < diff_tol -> logz = sum lz - sum ldet[0, nb), active = 0; else the candidates become
// the sites; v.f <- v.fnew
void launch_ep_chain(EpVecs e, NewtonVecs v, int n, int np, const double* ldet, int64_t lstride,
                     int nb, double diff_tol, int fail_code, int* active, int* status,
                     int* n_iter, int nchains, hipStream_t s);
// per live chain after the stop sweep, for the IS theta-call's posterior factor and slot writer:
// v.f <- v.fnew (mu) and exact zeros in rows [n, np) of v.f, v.W, v.Ws and v.a
void launch_ep_handoff(NewtonVecs v, int n, int np, Live live, int nchains, hipStream_t s);

// cache slot: fp32 factor with an extra TB-row block (row np holds g^T for apm_slot_read; the
// estimate does not use it), plus fp64 vectors of the self-consistent epilogue (ugemm.hip)
struct SlotSet {
    float* L;           // (np + TB) x np, ld = np
    double* fpost64;    // np: f_post
    double* W64;        // np: W of the last Newton iteration (0 for PriorMC)
    double* z64;        // np: z = C^-1 f_post = a + W f_post (0 for PriorMC)
    double* cst;        // 1 per slot: 1/2 f_post^T z - 1/2 log|B|  (0 for PriorMC)
    int64_t lstride, vstride;
    // wide slots (trace of the factor's Gram L L^T above APM_WIDE_Q, ugemm.hip): the factor is
    // also kept in fp64 and their u-path runs on f64 MFMA
    double* const* L64; // per slot: np x np, ld = np, or null - buffers are attached by the host
                        // to the slots that become wide (rare), not allocated per slot
    double* rowq;       // np per slot: squared row norms of the factor (k_slot_write_L)
    int* wide;          // 1 per slot
    int* chain_wide;    // 1 per chain of the call (read back with the theta-call's results)
    double wide_q;      // the threshold (APM_WIDE_Q, overridable by the environment variable)
    double post_q;      // trace(C) above which an fp32 bottom block is recomputed in fp64
                        // (APM_POST32_Q; postcov.hip)
    const double* icm_thr;  // per chain: trace(C) below which bit 3 of chain_wide asks the host
                            // for the reference-route check of chol(C) (host_theta.cpp icm_check)
};
// trace(L L^T) above which a slot's u-path runs in fp64: the fp32 L.U moves
// log f by ~1e-10 x trace (11 nats at trace 1.15e11, sigma = e^18.5; < 1e-6 nats at the trace
// ~1e3 of typical thetas), so this keeps the fp32 rounding of L and U below ~1e-4 nats
#define APM_WIDE_Q 1.0e6
// trace(C) above which the posterior factor's bottom block is recomputed in fp64 (postcov.hip):
// its fp32 TRSM moves log f by ~1e-9 x trace(C) (tools/postcov_precision_study.py)
#define APM_POST32_Q 1.0e5
// write slot slots[b] from the factored work matrix. mode 1 = PriorMC (K_chol at (0,0), g = 0),
// mode 2 = IS via chol(K) (postcov.hip: chol(C) J at rows [np, 2np) cols [0, np), g in v.Kb),
// mode 3 = the same with chol(C) J in the fp32 bottom block of S32 (rows [np, 2np)); its chains
// with trace(C) > S.post_q get bit 1 of S.chain_wide (the host recomputes them in fp64, mode 2).
// Only chains with live.active[b] && !live.status[b] are written.
void launch_slot_write(MatB A, NewtonVecs v, const double* ldet, int64_t lstride, int nb,
                       SlotSet S, const int64_t* slots, int mode, int n, int np, Live live,
                       int nchains, hipStream_t s, MatF S32 = MatF{nullptr, 0, 0},
                       double* rowe = nullptr);
// the fp64 factor alone, for the call's wide slots that have a buffer attached (mode 1 or 2)
void launch_slot_write_L64(MatB A, SlotSet S, const int64_t* slots, int mode, int np, Live live,
                           int nchains, hipStream_t s);

// ---- postcov.hip ----------------------------------------------------------------------------
void launch_set_rhs(MatB A, int64_t row0, int ncols, const double* vec, int64_t vstride,
                    Live live, int nchains, hipStream_t s);
void launch_get_row(MatB A, int64_t row, int n, double* out, int64_t ostride, Live live,
                    int nchains, hipStream_t s);
// dst (from column dcol0) <- Y2 = J (W^1/2 L)^T J, and L <- L J in place, in one pass. Upper
// tiles of Y2 are zeroed: all of them (zero_all), or only the first super-diagonal, the only
// ones the single-launch SYRK (k_chol_update_t128, plus == 2) reads
void launch_form_y2_rev(MatB L, MatB dst, int64_t dcol0, const double* Ws, int64_t vstride,
                        int np, Live live, int nchains, hipStream_t s, bool zero_all);
void launch_identity_lower(MatB M, int np, Live live, int nchains, hipStream_t s);
// out = L^T x (L lower), or with rev g = J L^T J h; tile-parallel through nb*nb*64 partials per chain
void launch_trmv_tiles(bool rev, MatB L, const double* x, double* out, int64_t vstride, int np,
                       double* part, int64_t pstride, Live live, int nchains, hipStream_t s);
// fp32 working copy of the posterior factor for its bottom block (postcov.hip): S32's top rows
// <- the lower tiles of the fp64 top factor L' (rows [0, np) of A) in tile columns [k0, k1), its
// diagonal-tile inverses D32 <- D64 for those columns; bottom: S32's rows [np, 2np) <- L_K J
// (rows [np, 2np) of A) from the outer panel of each row's first nonzero tile on (the zero
// tiles the bottom's updates read included)
void launch_post32_convert(MatB A, MatF S32, const double* D64, int64_t d64stride, float* D32,
                           int64_t d32stride, int nb, int outer, int k0, int k1, bool bottom,
                           Live live, int nchains, hipStream_t s,
                           Planes16 pl = Planes16{nullptr, 0, 0, 0});
// status[b] = code where other[b] != 0 (chol(K) failure of the concurrent factorisation wins)
void launch_merge_status(int* status, const int* other, int code, int nchains, hipStream_t s);

// ---- newton.hip: read-back of up to three small device arrays (4-byte words) into mapped
// pinned host memory, back to back at dst (device address of the host buffer)
struct Export {
    const unsigned* src[4];
    int words[4];
    unsigned* dst;
};
void launch_export(const Export& e, hipStream_t s);

// ---- ugemm.hip ------------------------------------------------------------------------------
struct UPool {
    double* base;       // each buffer: np x sp fp64, ld = sp, zero padded (device normals are
                        // fp32 values; host uploads keep their fp64 values for the wide path)
    int64_t stride;
    int sp;
    float* base32;      // the same buffers rounded to fp32 (same layout), written with them: the
                        // operand k_ugemm reads (half the bytes of converting the fp64 ones there)
};
void launch_u_convert(const double* U64, int64_t ldu, int n, int S, UPool P, int64_t ubuf,
                      hipStream_t s);
void launch_u_normal(UPool P, const int64_t* ubufs, const uint64_t* seeds,
                     const uint64_t* counters, int n, int S, int nchains, hipStream_t s);
void launch_u_combine(UPool P, const int64_t* dst, const int64_t* a, const int64_t* b,
                      const double* ca, const double* cb, int n, int S, int nchains,
                      hipStream_t s);
// partial[b][i][s] = sum over rows of row-block i of t(n,s) (i < nb), partial[b][nb][s] = g^T u_s
// wide: also launch the f64 MFMA twin for the call's wide slots (k_ugemm64)
void launch_ugemm(int lik, SlotSet S, const int64_t* slots, UPool P, const int64_t* ubufs,
                  const double* y, int n, int np, double* partial, int64_t pstride,
                  const int* status, int nchains, bool wide, hipStream_t s);
void launch_lme(const double* partial, int64_t pstride, int nb, int S, int sp, SlotSet Sl,
                const int64_t* slots, double* out, const int* status, int nchains,
                hipStream_t s);

// ---- is_diag.hip: block estimates and weight diagnostics of the IS estimate --
// per chain b and block j < nblk of B samples of `partial` (k_ugemm's per-sample sums, log w_s as
// is_weights.h forms it): logf, ess and wmax at out[q * qstride + b * ostride + off + j], q = 0, 1, 2;
// chains with status != 0 are skipped
void launch_lme_blocks(const double* partial, int64_t pstride, int nb, int B, int nblk, int sp,
                       const double* cst, const int64_t* slots, double* out, int64_t qstride,
                       int64_t ostride, int64_t off, const int* status, int nchains,
                       hipStream_t s);

// ---- is_predict.hip: importance-sampling predictive at test inputs ----------
// wbar[b * sp + s] = the self-normalised weight of sample s < S from the per-sample sums the
// theta-call's k_ugemm left in `partial` (is_weights.h), exact zeros for s in [S, sp);
// ess[b] = 1 / sum_s wbar_s^2
void launch_is_weights(const double* partial, int64_t pstride, int nb, int S, int sp,
                       const double* cst, const int64_t* slots, double* wbar, double* ess,
                       Live live, int nchains, hipStream_t s);
// Ut[b][s][k] = U[ubufs[b]][np - 1 - k][s] (sp x np per chain); the U buffers are only read
void launch_is_ut(UPool P, const int64_t* ubufs, int np, double* Ut, Live live, int nchains,
                  hipStream_t s);
// per chain and row r < 64 mb of the solved rows p_r^T in A's rows [row0, ..) x columns
// [0, 64 nb): vstar = sig[b] - |p_r|^2, cvec = sum_tj part[tj][r] in order (0 for r >= ms), each at
// out[b * ostride + r], and p_r^T J into columns [64 nb, 128 nb) of the same row
void launch_is_rows(MatB A, int64_t row0, int ms, int mb, int nb, const double* sig,
                    const double* lam, const double* xsn,
                    const double* part, int64_t pstride, double* vstar, double* cvec,
                    int64_t ostride, Live live, int nchains, hipStream_t s);
// per (chain, row tile < mb, sample tile < sp / 64): the h-rows (A's rows [row0, ..), columns
// [col0, col0 + np)) times Ut on the f64 MFMA, m = cvec + acc, the link (lik: APM_LIK_*) and the
// weighted sums over the tile's samples into pp[((b 3 + q) npr + row) (sp / 64) + tile], q = 0: wbar
// link, 1: wbar m, 2: wbar m^2
void launch_is_pred_gemm(int lik, MatB A, int64_t row0, int64_t col0, int np, int mb,
                         const double* Ut, int sp, const double* wbar, const double* vstar,
                         const double* cvec, int64_t ostride, double* pp, int64_t npr, Live live,
                         int nchains, hipStream_t s);
// the sample-tile partials in order -> prob, mean, var = vstar + sum wbar m^2 - mean^2 (r < ms)
void launch_is_finish(const double* pp, int64_t npr, int nst, int ms, const double* vstar,
                      double* mean, double* var, double* prob, int64_t ostride, Live live,
                      int nchains, hipStream_t s);

// ---- is_loo.hip: leave-one-out predictive densities from the IS samples ------
// logw[b * sp + s] = log of the self-normalised weight of sample s < S (is_weights.h, from
// `partial`), -inf for s in [S, sp); ess[b] = k_is_weights' value; chains with status != 0 skipped
void launch_is_logw(const double* partial, int64_t pstride, int nb, int S, int sp,
                    const double* cst, const int64_t* slots, double* logw, double* ess,
                    const int* status, int nchains, hipStream_t s);
// per (chain, row block, sample tile): C_chol U as launch_ugemm forms it (wide: the f64 twin for
// the call's wide slots too), f = f_post + acc, t = log wbar - log p(y_row | f) (-inf where log
// wbar is) and one of two epilogues on the rows < n. store: every t at out[(b np + row) sp + s],
// rows [n, np) left alone. Else the tile's five log-space sums of t and t' = log wbar + log p at
// out[((b 5 + q) np + row) (sp / 64) + tile], q = 0: max t, 1: sum e^(t - max), 2: sum e^(2 (t -
// max)), 3: max t', 4: sum e^(t' - max')
void launch_is_row_gemm(int lik, bool store, SlotSet S, const int64_t* slots, UPool P,
                        const int64_t* ubufs, const double* y, int n, int np, const double* logw,
                        double* out, const int* status, int nchains, bool wide, hipStream_t s);
// the sample tiles in order -> loo, lpd, ess_loo, and the cavity density gauss from the slot's
// rowq, W64, z64 and fpost64, at out[q * qstride + b * npr + row], q = 0 .. 3 (row < n)
void launch_is_loo_finish(int lik, const double* pp, int64_t npr, int nst, int n, SlotSet S,
                          const int64_t* slots, const double* y, double* out, int64_t qstride,
                          const int* status, int nchains, hipStream_t s);

// ---- is_psis.hip: Pareto-smoothed leave-one-out densities and k-hat ----------
// per (chain, row < n) of T (chain stride tstride, row stride sp, the first S columns): the tail
// fit and the smoothed sum into out[b npr + row] (loo_psis) and out[qstride + b npr + row] (khat);
// per chain the fit on logw[b sp ..] into khat_w[b]. S <= APM_PSIS_MAX_SAMPLES.
void launch_psis_rows(const double* T, int64_t tstride, int sp, const double* logw, int S, int n,
                      double* out, int64_t npr, int64_t qstride, double* khat_w,
                      const int* status, int nchains, hipStream_t s);

// chol(K) retry of the chains with fail[b] == code, unblocked in LAPACK's dpotf2 order (chol.hip,
// DESIGN.md §3.4): K's lower triangle into A, L in place, per-tile log-diagonal sums into ldet;
// success clears fail[b]. Returns false (nothing launched) for np > 512.
bool launch_chol_unblocked(MatB K, MatB A, int np, int* fail, int code, double* ldet,
                           int64_t lstride, int nchains, hipStream_t s);

// ---- the guard (newton.hip) --------------------------------------------------
// G[k * B + b]: 0: 1/2 log|B| of the last Newton factor, 1: 1/2 log|K|, 2..5: residuals r1..r4
// (rowe: the slot writer's per-row residuals of C_chol g = f_post, B x np)
void launch_guard_save(const double* ldet, int64_t lstride, int off, int nb, double* G, int B,
                       int k, Live live, int nchains, hipStream_t s);
void launch_guard_check(const double* ldet, int64_t lstride, int nb, const double* gvec,
                        int64_t gstride, SlotSet S, const int64_t* slots, double* G, int B,
                        double t1, double t2, double t3, double t4, const double* rowe,
                        const double* fvec, int fail_code, Live live, int nchains,
                        hipStream_t s);

// ---- launching (stream skew: tests only; host_ctx.cpp skew_point, APM_SKEW) ----------------
// Every launch goes through APM_LAUNCH, which first lets skew_point enqueue a delay kernel on the
// launch's stream when the calling thread's context asked for it (a cross-stream edge without
// its wait then reads stale data deterministically instead of by chance), and which throws a
// HipError when the launch is refused: the C-ABI entry point that enqueued it returns APM_E_HIP.
struct __attribute__((visibility("hidden"))) HipError {
    std::string msg;
};
static inline void throw_if_launch_failed() {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) throw HipError{std::string("kernel launch: ") + hipGetErrorString(e)};
}
#ifdef APM_TOOL_NO_SKEW  // stand-alone development benches that include a .hip file directly
inline void skew_point(hipStream_t) {}
#else
void skew_point(hipStream_t s);
#endif
void launch_delay(int us, hipStream_t s);  // (skew_point's own kernel: launched without it)
#define APM_LAUNCH(kern, grid, block, lds, st, ...)                      \
    do {                                                                 \
        skew_point(st);                                                  \
        hipLaunchKernelGGL(kern, grid, block, lds, st, __VA_ARGS__);     \
        throw_if_launch_failed();                                        \
    } while (0)
