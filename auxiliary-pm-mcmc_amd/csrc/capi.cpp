// The C-ABI (include/apm.h): argument checks, the per-call staging of the host's inputs, the
// translation of a HipError into APM_E_HIP and the NaN rows of failed chains, each frame written
// once (ctx_call, cached_call, check_theta_call, check_u_call, finish_rows). The orchestration
// behind the entry points is in the host_*.cpp units (apm_host.h): a batched theta-call here names
// its fit and its tail there and launches nothing itself. What still launches from this file is one
// kernel behind a staged copy (the U-buffer calls, apm_gram, apm_gram_cross, the self-tests, the
// marker).
#include <cmath>
#include <limits>
#include <mutex>
#include <optional>

#include "apm_host.h"

#define APM_VERSION 3

using namespace apm_host;

namespace {

thread_local std::string g_err;

int fail(apm_ctx* c, int code, const std::string& m) {
    if (c) c->err = m;
    g_err = m;
    return code;
}

bool check_idx(apm_ctx* c, int64_t count, const int64_t* idx, int64_t lim, const char* what) {
    for (int64_t i = 0; i < count; ++i)
        if (idx[i] < 0 || idx[i] >= lim) {
            fail(c, APM_E_INVALID, std::string(what) + " index out of range");
            return false;
        }
    return true;
}

// stand-alone calls reuse one context per (device, n, kind) shape
std::mutex g_mu;
std::map<std::tuple<int, int64_t, int64_t, int>, apm_ctx*> g_cache;

// A context entry point: its launches belong to c (the SkewScope, where the entry point opens
// one), on c's device, and a HipError of the body becomes APM_E_HIP. The body returns nothing; an
// early `return` in it ends the call with APM_SUCCESS.
enum Skew { NO_SKEW, SKEW };
template <class Body>
int ctx_call(apm_ctx* c, Skew skew, Body body) {
    std::optional<SkewScope> scope;
    if (skew == SKEW) scope.emplace(c);
    try {
        HIPC(hipSetDevice(c->device));
        body();
    } catch (const HipError& e) {
        return fail(c, APM_E_HIP, e.msg);
    }
    return APM_SUCCESS;
}

// A stand-alone call on the cached context of its (device, n, d, kind) shape; the body creates or
// refreshes it (c is null at the shape's first call). A HipError frees the context and forgets it.
template <class Body>
int cached_call(int device, int64_t n, int64_t d, int kind, Body body) {
    std::lock_guard<std::mutex> lk(g_mu);
    apm_ctx*& c = g_cache[std::make_tuple(device, n, d, kind)];
    try {
        body(c);
    } catch (const HipError& e) {
        if (c) {
            free_ctx(c);
            c = nullptr;
        }
        return fail(nullptr, APM_E_HIP, e.msg);
    }
    return APM_SUCCESS;
}

// ---- the batched theta-calls (apm_predict, apm_laplace_grad, apm_ep_eval, apm_ep_predict,
// apm_ep_grad, apm_is_predict): at most max_batch rows of theta, a fit, a tail on the chains that
// are OK, NaN rows for the others (the source map, says what a new one supplies)

// What such a call has checked, in the one order all of them keep: the context, `early`, the
// likelihood, the covariance kind, m, count, ldo, ldt, ldg, and last whatever else the entry point
// names (rest_bad: evaluated only with a context).
struct ThetaArgs {
    const char* early = nullptr;  // a refusal that needs no context (apm_is_predict's est)
    bool probit_only = false;     // (unless the context's EP moments come by quadrature)
    const char* device_why = "";  // why a PRECOMPUTED context is refused: "needs ... (...)"
    bool batch = false;           // count in [1, max_batch]
    int64_t count = 0;
    bool rows = false;            // m > 0 and ldo >= m, a message each
    int64_t m = 0, ldo = 0;
    bool lds = false;             // ldt, ldg >= theta length, a message each
    int64_t ldt = 0, ldg = 0;
    const char* rest_msg = "bad arguments";
};
template <class Rest>
int check_theta_call(apm_ctx* c, const char* who, const ThetaArgs& a, Rest rest_bad) {
    const auto no = [&](apm_ctx* cc, const char* m) {
        return fail(cc, APM_E_INVALID, std::string(who) + ": " + m);
    };
    if (!c) return no(nullptr, "null context");
    if (a.early) return no(c, a.early);
    if (a.probit_only && c->lik != APM_LIK_PROBIT && !c->ep_quad)
        return no(c, "probit only (the logit's tilted moments need quadrature)");
    if (c->kind == APM_KERNEL_PRECOMPUTED) return no(c, a.device_why);
    if (a.rows && a.m <= 0) return no(c, "m <= 0");
    if (a.batch && (a.count <= 0 || a.count > c->max_batch))
        return no(c, "count outside [1, max_batch]");
    if (a.rows && a.ldo < a.m) return no(c, "ldo < m");
    if (a.lds && a.ldt < c->P) return no(c, "ldt < theta length");
    if (a.lds && a.ldg < c->P) return no(c, "ldg < theta length");
    if (rest_bad()) return no(c, a.rest_msg);
    return APM_SUCCESS;
}

// ---- the cached u-calls with outputs of their own (apm_u_eval_diag, apm_is_spread, apm_is_loo,
// apm_is_loo_psis): what each has checked, in the one order all of them keep - the context, count,
// the pointers every such call needs and the entry point's further ones (more_null), the entry
// point's own checks (own: the first message that applies or null, evaluated only with a context),
// and last the two index lists. apm_u_eval keeps its single message.
template <class Own>
int check_u_call(apm_ctx* c, const char* who, int64_t count, const int64_t* slots,
                 const int64_t* ubufs, const int* status, bool more_null, Own own) {
    const auto no = [&](apm_ctx* cc, const char* m) {
        return fail(cc, APM_E_INVALID, std::string(who) + ": " + m);
    };
    if (!c) return no(nullptr, "null context");
    if (count <= 0 || count > c->max_batch) return no(c, "count outside [1, max_batch]");
    if (!slots || !ubufs || !status || more_null) return no(c, "bad arguments");
    if (const char* m = own()) return no(c, m);
    if (!check_idx(c, count, slots, c->n_slots, "slot") ||
        !check_idx(c, count, ubufs, c->n_ubufs, "ubuf"))
        return APM_E_INVALID;
    return APM_SUCCESS;
}

// NaN where the chain's status is not OK: in its row of each (pointer, row stride, width), a null
// pointer skipped, and in its entry of the per-chain scalars
struct Rows {
    double* p;
    int64_t ld, width;
};
void finish_rows(int64_t count, const int* status, std::initializer_list<Rows> rows,
                 std::initializer_list<double*> scalars = {}) {
    const double nan = std::numeric_limits<double>::quiet_NaN();
    for (int64_t b = 0; b < count; ++b) {
        if (status[b] == APM_STATUS_OK) continue;
        for (const Rows& r : rows)
            if (r.p) std::fill(r.p + b * r.ld, r.p + b * r.ld + r.width, nan);
        for (double* s : scalars)
            if (s) s[b] = nan;
    }
}

// an EP fit's statuses and sweep counts to the caller (after the sync behind ep_*fit*)
void ep_report(const EpFit& f, int64_t count, int* status, int64_t* n_sweeps) {
    for (int64_t b = 0; b < count; ++b) {
        status[b] = f.st[b];
        if (n_sweeps) n_sweeps[b] = f.sweeps[b];
    }
}

// count staged rows of `width` doubles -> the caller's rows (row stride ld), if asked for
void rows_out(double* dst, int64_t ld, const std::vector<double>& src, int64_t count,
              int64_t width) {
    if (dst)
        for (int64_t b = 0; b < count; ++b)
            std::copy(src.begin() + b * width, src.begin() + (b + 1) * width, dst + b * ld);
}

}  // namespace

// =============================================================================== C-ABI
extern "C" {

int apm_version(void) { return APM_VERSION; }

int apm_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

const char* apm_global_error(void) { return g_err.c_str(); }

apm_ctx* apm_create(int device, int kernel_kind, const double* X, int64_t n, int64_t d,
                    int64_t ldx, const double* y, double epsilon, int64_t n_imp,
                    int64_t max_batch, int64_t n_slots, int64_t n_ubufs) {
    if (n <= 0 || d < 0 || n_imp <= 0 || max_batch <= 0 || n_slots <= 0 || n_ubufs <= 0 ||
        (kernel_kind != APM_KERNEL_PRECOMPUTED && !kernel_kind_of(kernel_kind).on_device()) ||
        (kernel_kind != APM_KERNEL_PRECOMPUTED && !X) ||
        n_imp > 1 << 20) {
        g_err = "apm_create: invalid arguments";
        return nullptr;
    }
    apm_ctx* c = new apm_ctx();
    try {
        init_ctx(c, device, kernel_kind, X, n, d, ldx, y, epsilon, n_imp, max_batch, n_slots,
                 n_ubufs);
    } catch (const HipError& e) {
        g_err = "apm_create: " + e.msg;
        free_ctx(c);
        return nullptr;
    }
    return c;
}

void apm_destroy(apm_ctx* ctx) { free_ctx(ctx); }

const char* apm_last_error(const apm_ctx* ctx) { return ctx ? ctx->err.c_str() : g_err.c_str(); }

int64_t apm_padded_n(const apm_ctx* ctx) { return ctx ? ctx->np : -1; }

int64_t apm_theta_len(const apm_ctx* ctx) { return ctx ? ctx->P : -1; }

int apm_set_newton(apm_ctx* ctx, double diff_f_tol, int64_t max_iters) {
    if (!ctx || max_iters < 0) return fail(ctx, APM_E_INVALID, "apm_set_newton: bad arguments");
    ctx->tol = diff_f_tol;
    ctx->max_iters = max_iters;
    return APM_SUCCESS;
}

int apm_set_likelihood(apm_ctx* ctx, int lik) {
    if (!ctx || (lik != APM_LIK_PROBIT && lik != APM_LIK_LOGIT))
        return fail(ctx, APM_E_INVALID, "apm_set_likelihood: bad arguments");
    ctx->lik = lik;
    return APM_SUCCESS;
}

int apm_likelihood(const apm_ctx* ctx) { return ctx ? ctx->lik : APM_E_INVALID; }

void* apm_stream(apm_ctx* ctx) { return ctx ? (void*)ctx->stream : nullptr; }

int apm_u_upload(apm_ctx* c, int64_t ubuf, const double* U, int64_t ldu) {
    if (!c || !U || ubuf < 0 || ubuf >= c->n_ubufs || ldu < c->S)
        return fail(c, APM_E_INVALID, "apm_u_upload: bad arguments");
    return ctx_call(c, SKEW, [&] {
        HIPC(hipMemcpy2DAsync(c->U64, sizeof(double) * c->S, U, sizeof(double) * ldu,
                              sizeof(double) * c->S, c->n, hipMemcpyHostToDevice, c->stream));
        launch_u_convert(c->U64, c->S, c->n, c->S, c->Up, ubuf, c->stream);
        sync(c);
    });
}

int apm_u_download(apm_ctx* c, int64_t ubuf, double* U, int64_t ldu) {
    if (!c || !U || ubuf < 0 || ubuf >= c->n_ubufs || ldu < c->S)
        return fail(c, APM_E_INVALID, "apm_u_download: bad arguments");
    return ctx_call(c, NO_SKEW, [&] {
        std::vector<double> h((size_t)c->np * c->sp);
        HIPC(hipMemcpyAsync(h.data(), c->Up.base + ubuf * c->Up.stride, sizeof(double) * h.size(),
                            hipMemcpyDeviceToHost, c->stream));
        sync(c);
        for (int i = 0; i < c->n; ++i)
            for (int s = 0; s < c->S; ++s) U[(int64_t)i * ldu + s] = h[(size_t)i * c->sp + s];
    });
}

int apm_u_normal(apm_ctx* c, int64_t count, const int64_t* ubufs, const uint64_t* seeds,
                 const uint64_t* counters) {
    if (!c || count <= 0 || count > c->max_batch || !ubufs || !seeds || !counters)
        return fail(c, APM_E_INVALID, "apm_u_normal: bad arguments");
    if (!check_idx(c, count, ubufs, c->n_ubufs, "ubuf")) return APM_E_INVALID;
    return ctx_call(c, SKEW, [&] {
        std::memcpy(blk_field(c, BLK_I3), ubufs, sizeof(int64_t) * count);
        std::memcpy(blk_field(c, BLK_SEEDS), seeds, sizeof(uint64_t) * count);
        std::memcpy(blk_field(c, BLK_CTRS), counters, sizeof(uint64_t) * count);
        HIPC(hipMemcpyAsync(c->d_i3, c->hblk, sizeof(int64_t) * BLK_FIELDS * c->max_batch,
                            hipMemcpyHostToDevice, c->stream));
        launch_u_normal(c->Up, c->d_i3, c->d_seeds, c->d_ctrs, c->n, c->S, (int)count,
                        c->stream);
        sync(c);
    });
}

int apm_u_combine(apm_ctx* c, int64_t count, const int64_t* dst, const int64_t* a,
                  const int64_t* b, const double* ca, const double* cb) {
    if (!c || count <= 0 || count > c->max_batch || !dst || !a || !b || !ca || !cb)
        return fail(c, APM_E_INVALID, "apm_u_combine: bad arguments");
    if (!check_idx(c, count, dst, c->n_ubufs, "dst") || !check_idx(c, count, a, c->n_ubufs, "a") ||
        !check_idx(c, count, b, c->n_ubufs, "b"))
        return APM_E_INVALID;
    return ctx_call(c, SKEW, [&] {
        const int64_t B = c->max_batch;
        std::memcpy(blk_field(c, BLK_I3), dst, sizeof(int64_t) * count);
        std::memcpy(blk_field(c, BLK_A), a, sizeof(int64_t) * count);
        std::memcpy(blk_field(c, BLK_B), b, sizeof(int64_t) * count);
        std::memcpy(blk_field(c, BLK_CA), ca, sizeof(double) * count);
        std::memcpy(blk_field(c, BLK_CB), cb, sizeof(double) * count);
        HIPC(hipMemcpyAsync(c->d_i3, c->hblk, sizeof(int64_t) * BLK_SEEDS * B,  // (up to cb)
                            hipMemcpyHostToDevice, c->stream));
        launch_u_combine(c->Up, c->d_i3, c->d_i3 + BLK_A * B, c->d_i3 + BLK_B * B, c->d_ca,
                         c->d_cb, c->n, c->S, (int)count, c->stream);
        sync(c);
    });
}

int apm_theta_eval(apm_ctx* c, int est, int64_t count, const double* thetas, int64_t ldt,
                   const int64_t* ubufs, const int64_t* slots, double* out_logf, int* status,
                   int64_t* nops) {
    if (!c || count <= 0 || count > c->max_batch || !thetas || !out_logf || !status ||
        est < 0 || est > APM_EST_IS_EP || c->kind == APM_KERNEL_PRECOMPUTED || ldt < c->P)
        return fail(c, APM_E_INVALID, "apm_theta_eval: bad arguments");
    if (est == APM_EST_IS_EP && c->lik != APM_LIK_PROBIT && !c->ep_quad)
        return fail(c, APM_E_INVALID, "apm_theta_eval: APM_EST_IS_EP is probit only (the logit's "
                                      "tilted moments need quadrature)");
    if (est != APM_EST_LAPLACE) {
        if (!ubufs || !slots) return fail(c, APM_E_INVALID, "apm_theta_eval: ubufs/slots required");
        if (!check_idx(c, count, slots, c->n_slots, "slot") ||
            !check_idx(c, count, ubufs, c->n_ubufs, "ubuf"))
            return APM_E_INVALID;
    }
    return ctx_call(c, SKEW, [&] {
        const double* th = upload_thetas(c, count, thetas, ldt);
        // fp16x3 Newton updates need |L_ij| <= sqrt(1 + K_ii) < 65504 (chol32_update.hip): per chain;
        // the posterior bottom block's operands |L'_ij| <= sqrt(1 + n K_ii) (postcov.hip).
        // K_ii = s + beta + eps; "theta_0 < 19" is the bound s < e^19 on K_ii, which a constant
        // term shares (beta = 0 leaves every flag what it was). With the linear term K_ii differs
        // by row: the bounds take its largest value, s + beta + lambda max|x|^2 + eps, and the
        // ICM threshold its sum, trace(K); without the flag every expression is
        // what it was
        const bool lin = kernel_kind_of(c->kind).linear != 0;
        for (int64_t b = 0; b < count; ++b) {
            const double beta = cov_beta(c->kind, c->P, th + b * c->P);
            double sb = std::exp(th[b * c->P]) + beta;
            double tr = 0.0;
            if (lin) {
                const double lam = cov_lambda(c->kind, c->P, th + b * c->P);
                tr = c->n * (sb + c->eps) + lam * c->x2sum;
                sb += lam * c->x2max;
            }
            const double kii = sb + c->eps;
            pin_h3(c)[b] = c->h3 && (beta == 0.0 && !lin ? th[b * c->P] < 19.0 : std::log(sb) < 19.0);
            pin_inv(c)[b] = 1.0 + sb + c->eps < 32768.0;
            pin_h3post(c)[b] = c->h3 && 1.0 + c->n * kii < 4e8;
            pin_icm(c)[b] = (lin ? tr : c->n * kii) / std::max(c->icm_q, 1.0);
        }
        upload_h3(c, (int)count);
        if (est != APM_EST_LAPLACE) upload_idx(c, (int)count, slots, ubufs);
        theta_eval_impl(c, est, (int)count, true, out_logf, status, nops);
    });
}

int apm_theta_eval_K(apm_ctx* c, int est, const double* K, int64_t ldk, int64_t ubuf,
                     int64_t slot, double* out_logf, int* status, int64_t* nops) {
    if (!c || !K || ldk < c->n || !out_logf || !status || est < 0 || est > APM_EST_IS_EP)
        return fail(c, APM_E_INVALID, "apm_theta_eval_K: bad arguments");
    if (est == APM_EST_IS_EP && c->lik != APM_LIK_PROBIT && !c->ep_quad)
        return fail(c, APM_E_INVALID, "apm_theta_eval_K: APM_EST_IS_EP is probit only (the "
                                      "logit's tilted moments need quadrature)");
    if (est != APM_EST_LAPLACE &&
        (slot < 0 || slot >= c->n_slots || ubuf < 0 || ubuf >= c->n_ubufs))
        return fail(c, APM_E_INVALID, "apm_theta_eval_K: slot/ubuf out of range");
    return ctx_call(c, SKEW, [&] {
        std::vector<double> Kp;  // (alive until theta_eval_impl's syncs)
        const double kmax = upload_padded_K(c, K, ldk, Kp);
        pin_h3(c)[0] = c->h3 && kmax < 1.8e8;  // sqrt(1 + K_ii) < 1.4e4 (chol32_update.hip)
        pin_inv(c)[0] = 1.0 + kmax < 32768.0;
        pin_h3post(c)[0] = c->h3 && 1.0 + c->n * kmax < 4e8;
        pin_icm(c)[0] = c->n * kmax / std::max(c->icm_q, 1.0);
        upload_h3(c, 1);
        upload_idx(c, 1, &slot, &ubuf);  // (the pinned copy is the slot the read-back marks)
        theta_eval_impl(c, est, 1, false, out_logf, status, nops);
    });
}

int apm_u_eval(apm_ctx* c, int64_t count, const int64_t* slots, const int64_t* ubufs,
               double* out_logf, int* status) {
    if (!c || count <= 0 || count > c->max_batch || !slots || !ubufs || !out_logf || !status)
        return fail(c, APM_E_INVALID, "apm_u_eval: bad arguments");
    if (!check_idx(c, count, slots, c->n_slots, "slot") ||
        !check_idx(c, count, ubufs, c->n_ubufs, "ubuf"))
        return APM_E_INVALID;
    return ctx_call(c, SKEW, [&] {
        u_call_open(c, (int)count, slots, ubufs);
        read_back(c, {RB{c->out, (int)sizeof(double) * (int)count, out_logf},
                      RB{c->status, (int)sizeof(int) * (int)count, status}});
        // u_call_close's rule for the one scalar here: a slot whose last theta-call failed was
        // never written, and c->out keeps an earlier call's value where k_lme wrote nothing
        for (int b = 0; b < (int)count; ++b)
            if (status[b] != 0 || c->slot_failed[slots[b]])
                out_logf[b] = std::numeric_limits<double>::quiet_NaN();
    });
}

// ---- block estimates and weight diagnostics of the IS estimate (host_is_diag.cpp) ------------
namespace {

// what apm_u_eval_diag and apm_is_spread share (draws: the latter's seeds / counters)
int is_diag_call(apm_ctx* c, const char* who, int64_t count, const int64_t* slots,
                 const int64_t* ubufs, bool draws, const uint64_t* seeds, const uint64_t* counters,
                 int64_t n_rep, int64_t block, double* logf, double* ess, double* wmax,
                 int64_t ldo, int* status) {
    const int rc = check_u_call(c, who, count, slots, ubufs, status,
                                draws && (!seeds || !counters), [&]() -> const char* {
        if (block < 1 || block > c->S) return "block outside [1, n_imp]";
        if (n_rep < 1) return "n_rep < 1";
        const int64_t nblk = c->S / block;
        if (n_rep > APM_SPREAD_MAX_BLOCKS || n_rep * nblk > APM_SPREAD_MAX_BLOCKS)
            return "n_rep * nblk above APM_SPREAD_MAX_BLOCKS";
        return ldo < n_rep * nblk ? "ldo < n_rep * nblk" : nullptr;
    });
    if (rc != APM_SUCCESS) return rc;
    return ctx_call(c, SKEW, [&] {
        is_diag_run(c, (int)count, slots, ubufs, draws ? seeds : nullptr, counters, n_rep, block,
                    logf, ess, wmax, ldo, status);
    });
}

}  // namespace

int apm_u_eval_diag(apm_ctx* c, int64_t count, const int64_t* slots, const int64_t* ubufs,
                    int64_t block, double* logf, double* ess, double* wmax, int64_t ldo,
                    int* status) {
    return is_diag_call(c, "apm_u_eval_diag", count, slots, ubufs, false, nullptr, nullptr, 1,
                        block, logf, ess, wmax, ldo, status);
}

int apm_is_spread(apm_ctx* c, int64_t count, const int64_t* slots, const int64_t* ubufs,
                  const uint64_t* seeds, const uint64_t* counters, int64_t n_rep, int64_t block,
                  double* logf, double* ess, double* wmax, int64_t ldo, int* status) {
    return is_diag_call(c, "apm_is_spread", count, slots, ubufs, true, seeds, counters, n_rep,
                        block, logf, ess, wmax, ldo, status);
}

// ---- leave-one-out predictive densities from the IS samples (host_is_loo.cpp) -----------------
int apm_is_loo(apm_ctx* c, int64_t count, const int64_t* slots, const int64_t* ubufs,
               double* out_logf, double* loo, double* lpd, double* ess_loo, double* gauss,
               int64_t ldo, double* ess, int* status) {
    const int rc = check_u_call(c, "apm_is_loo", count, slots, ubufs, status, false, [&] {
        return (loo || lpd || ess_loo || gauss) && ldo < c->n ? "ldo < n" : nullptr;
    });
    if (rc != APM_SUCCESS) return rc;
    return ctx_call(c, SKEW, [&] {
        is_loo_run(c, (int)count, slots, ubufs, out_logf, loo, lpd, ess_loo, gauss, ldo, ess,
                   status);
    });
}

// ---- their Pareto-smoothed form and the Pareto k-hat diagnostics (host_is_psis.cpp) ------------
int apm_is_loo_psis(apm_ctx* c, int64_t count, const int64_t* slots, const int64_t* ubufs,
                    double* out_logf, double* loo_psis, double* khat, int64_t ldo, double* khat_w,
                    double* logratio, int64_t ldr, int* status) {
    const int rc = check_u_call(c, "apm_is_loo_psis", count, slots, ubufs, status, false,
                                [&]() -> const char* {
        if (c->S > APM_PSIS_MAX_SAMPLES) return "n_imp above APM_PSIS_MAX_SAMPLES";
        if ((loo_psis || khat) && ldo < c->n) return "ldo < n";
        return logratio && ldr < (int64_t)c->n * c->S ? "ldr < n*n_imp" : nullptr;
    });
    if (rc != APM_SUCCESS) return rc;
    return ctx_call(c, SKEW, [&] {
        is_psis_run(c, (int)count, slots, ubufs, out_logf, loo_psis, khat, ldo, khat_w, logratio,
                    ldr, status);
    });
}

// ---- cache-slot lifetimes (samplers.py:563-584: an MH sampler holds the current state's cache
// and the proposal's at once; on accept the proposal's becomes current and the old one is dropped).
// Host bookkeeping only: a slot's contents are immutable between theta-calls into it, so a copy
// of the handle is another owner of the same state, as a second reference to the reference's
// (K_chol, C_chol, f_post) tuple is.
int apm_cache_acquire(apm_ctx* c, int64_t* slot) {
    if (!c || !slot) return fail(c, APM_E_INVALID, "apm_cache_acquire: bad arguments");
    for (int i = 0; i < c->n_slots; ++i)
        if (c->slot_refs[i] == 0) {
            c->slot_refs[i] = 1;
            *slot = i;
            return APM_SUCCESS;
        }
    return fail(c, APM_E_NOMEM, "apm_cache_acquire: every cache slot is owned (raise n_slots)");
}

int apm_cache_copy(apm_ctx* c, int64_t slot) {
    if (!c || slot < 0 || slot >= c->n_slots || c->slot_refs[slot] <= 0)
        return fail(c, APM_E_INVALID, "apm_cache_copy: slot not acquired");
    ++c->slot_refs[slot];
    return APM_SUCCESS;
}

int apm_cache_release(apm_ctx* c, int64_t slot) {
    if (!c || slot < 0 || slot >= c->n_slots || c->slot_refs[slot] <= 0)
        return fail(c, APM_E_INVALID, "apm_cache_release: slot not acquired");
    --c->slot_refs[slot];
    return APM_SUCCESS;
}

int64_t apm_cache_refcount(const apm_ctx* c, int64_t slot) {
    if (!c || slot < 0 || slot >= c->n_slots) return APM_E_INVALID;
    return c->slot_refs[slot];
}

int apm_slot_read(apm_ctx* c, int64_t slot, double* L, int64_t ldl, double* f_post, double* g,
                  double* cst) {
    if (!c || slot < 0 || slot >= c->n_slots) return fail(c, APM_E_INVALID, "apm_slot_read: bad slot");
    return ctx_call(c, NO_SKEW, [&] {
        const int64_t np = c->np;
        if (L || g) {
            std::vector<float> h((size_t)((np + 64) * np));
            HIPC(hipMemcpyAsync(h.data(), c->Sl.L + slot * c->Sl.lstride, sizeof(float) * h.size(),
                                hipMemcpyDeviceToHost, c->stream));
            sync(c);
            if (L)  // (the slot keeps row i only up to its diagonal tile)
                for (int i = 0; i < c->n; ++i)
                    for (int j = 0; j < c->n; ++j)
                        L[(int64_t)i * ldl + j] = j <= i ? h[(size_t)i * np + j] : 0.0;
            if (g)
                for (int j = 0; j < c->n; ++j) g[j] = h[(size_t)np * np + j];
        }
        if (f_post) {
            HIPC(hipMemcpyAsync(f_post, c->Sl.fpost64 + slot * c->Sl.vstride, sizeof(double) * c->n,
                                hipMemcpyDeviceToHost, c->stream));
        }
        if (cst)
            HIPC(hipMemcpyAsync(cst, c->Sl.cst + slot, sizeof(double), hipMemcpyDeviceToHost,
                                c->stream));
        sync(c);
    });
}

int apm_gram(int device, int kind, const double* X, int64_t n, int64_t d, int64_t ldx,
             const double* theta, int64_t n_theta, double eps, double* K, int64_t ldk) {
    if (n <= 0 || d <= 0 || !X || !theta || !K || ldk < n || ldx < d ||
        !kernel_kind_of(kind).on_device())
        return fail(nullptr, APM_E_INVALID, "apm_gram: bad arguments");
    const int64_t P = kernel_kind_of(kind).theta_len(d);
    if (n_theta < P) return fail(nullptr, APM_E_INVALID, "apm_gram: theta too short");
    return cached_call(device, n, d, kind + 16, [&](apm_ctx*& c) {
        if (!c) {
            c = new apm_ctx();
            init_ctx(c, device, kind, X, n, d, ldx, nullptr, eps, 1, 1, 1, 1);
        } else {
            HIPC(hipSetDevice(device));
            std::vector<double> Xc((size_t)(n * d));
            for (int64_t i = 0; i < n; ++i)
                for (int64_t k = 0; k < d; ++k) Xc[i * d + k] = X[i * ldx + k];
            HIPC(hipMemcpyAsync(c->X, Xc.data(), sizeof(double) * n * d, hipMemcpyHostToDevice,
                                c->stream));
        }
        HIPC(hipMemcpyAsync(c->theta, theta, sizeof(double) * P, hipMemcpyHostToDevice, c->stream));
        HIPC(hipMemsetD32Async(c->active, 1, 1, c->stream));
        HIPC(hipMemsetAsync(c->status, 0, sizeof(int), c->stream));
        launch_gram(c->K, c->X, d, (int)n, (int)d, c->theta, P, kind, eps, c->np, live_of(c), 1,
                    c->stream, true);
        HIPC(hipMemcpy2DAsync(K, sizeof(double) * ldk, c->K.base, sizeof(double) * c->np,
                              sizeof(double) * n, n, hipMemcpyDeviceToHost, c->stream));
        sync(c);
    });
}

int apm_gram_cross(int device, int kind, const double* Xs, int64_t m, const double* X, int64_t n,
                   int64_t d, int64_t ldx, const double* theta, int64_t n_theta, double* Ks,
                   int64_t ldk) {
    if (m <= 0 || n <= 0 || d <= 0 || !Xs || !X || !theta || !Ks || ldk < n || ldx < d ||
        m > (1 << 24) || n > (1 << 24) || !kernel_kind_of(kind).on_device())
        return fail(nullptr, APM_E_INVALID, "apm_gram_cross: bad arguments");
    const int64_t P = kernel_kind_of(kind).theta_len(d);
    if (n_theta < P) return fail(nullptr, APM_E_INVALID, "apm_gram_cross: theta too short");
    double* dev = nullptr;  // [X: n x d][Xs: m x d][theta: P][s][beta][lambda][Ks: m x n]
    try {
        HIPC(hipSetDevice(device));
        std::vector<double> h((size_t)((n + m) * d + P + 3));  // (+ s = exp(theta_0), beta, lambda)
        for (int64_t i = 0; i < n + m; ++i)  // both point sets take the row stride ldx
            for (int64_t k = 0; k < d; ++k)
                h[i * d + k] = i < n ? X[i * ldx + k] : Xs[(i - n) * ldx + k];
        for (int64_t p = 0; p < P; ++p) h[(n + m) * d + p] = theta[p];
        h[(n + m) * d + P] = std::exp(theta[0]);
        h[(n + m) * d + P + 1] = cov_beta(kind, (int)P, theta);
        h[(n + m) * d + P + 2] = cov_lambda(kind, (int)P, theta);
        HIPC(hipMalloc(reinterpret_cast<void**>(&dev), sizeof(double) * (h.size() + m * n)));
        HIPC(hipMemcpy(dev, h.data(), sizeof(double) * h.size(), hipMemcpyHostToDevice));
        double* dK = dev + h.size();
        launch_gram_cross(MatB{dK, n, 0}, 0, dev + n * d, (int)m, (int)((m + 63) / 64), dev, d,
                          (int)n, (int)d, (int)((n + 63) / 64), dev + (n + m) * d, 0,
                          dev + (n + m) * d + P, dev + (n + m) * d + P + 1,
                          dev + (n + m) * d + P + 2, kind, nullptr, nullptr, 0, nullptr, 0,
                          Live{nullptr, nullptr}, 1, 1, nullptr);
        HIPC(hipMemcpy2D(Ks, sizeof(double) * ldk, dK, sizeof(double) * n, sizeof(double) * n, m,
                         hipMemcpyDeviceToHost));
        HIPC(hipFree(dev));
    } catch (const HipError& e) {
        if (dev) (void)hipFree(dev);
        return fail(nullptr, APM_E_HIP, e.msg);
    }
    return APM_SUCCESS;
}

int apm_predict(apm_ctx* c, int64_t count, const double* thetas, int64_t ldt, const double* Xs,
                int64_t m, int64_t ldxs, double* mean, double* var, double* prob, int64_t ldo,
                int* status, int64_t* n_iter) {
    ThetaArgs a;
    a.device_why = "needs an ISO or ARD context (the cross-covariance is built on the device)";
    a.batch = a.rows = true;
    a.count = count, a.m = m, a.ldo = ldo;
    const int rc = check_theta_call(c, "apm_predict", a, [&] {
        return !thetas || !Xs || !status || ldt < c->P || ldxs < c->d;
    });
    if (rc != APM_SUCCESS) return rc;
    return ctx_call(c, SKEW, [&] {
        upload_thetas(c, count, thetas, ldt);
        std::vector<double> lml((size_t)count);
        if (laplace_then_live(c, (int)count, lml.data(), status, n_iter))
            predict_all(c, count, thetas, ldt, Xs, m, ldxs, mean, var, prob, ldo);
        finish_rows(count, status, {{mean, ldo, m}, {var, ldo, m}, {prob, ldo, m}});
    });
}

int apm_is_predict(apm_ctx* c, int est, int64_t count, const double* thetas, int64_t ldt,
                   const int64_t* ubufs, const int64_t* slots, const double* Xs, int64_t m,
                   int64_t ldxs, double* out_logf, double* prob, double* mean, double* var,
                   int64_t ldo, double* ess, int* status, int64_t* nops) {
    ThetaArgs a;
    if (est != APM_EST_IS && est != APM_EST_IS_EP) a.early = "APM_EST_IS or APM_EST_IS_EP only";
    a.device_why = "needs a context whose covariance is built on the device (the cross-"
                   "covariance is)";
    a.rest_msg = "bad test inputs or ldo < m";
    int rc = check_theta_call(c, "apm_is_predict", a, [&] {
        return m <= 0 || ldo < m || !Xs || ldxs < c->d;
    });
    // the theta-call itself: apm_theta_eval's checks (count, the logit's IS_EP refusal, indices),
    // staging and values
    if (rc == APM_SUCCESS)
        rc = apm_theta_eval(c, est, count, thetas, ldt, ubufs, slots, out_logf, status, nops);
    if (rc != APM_SUCCESS) return rc;
    return ctx_call(c, SKEW, [&] {
        int ok = 0;
        for (int64_t b = 0; b < count; ++b) ok += status[b] == APM_STATUS_OK;
        if (ok)
            is_predict_tail(c, (int)count, thetas, ldt, status, Xs, m, ldxs, prob, mean, var, ldo,
                            ess);
        finish_rows(count, status, {{mean, ldo, m}, {var, ldo, m}, {prob, ldo, m}}, {ess});
        // the tail's chol(K) and chol(J M J); the row solves count as apm_predict's do: not at all
        for (int64_t b = 0; nops && b < count; ++b) nops[b] += status[b] == APM_STATUS_OK ? 2 : 0;
    });
}

int apm_laplace_grad(apm_ctx* c, int64_t count, const double* thetas, int64_t ldt, double* lml,
                     double* grad, int64_t ldg, int* status, int64_t* n_iter) {
    ThetaArgs a;
    a.device_why = "needs an ISO or ARD context (dK/dtheta is built on the device)";
    a.batch = a.lds = true;
    a.count = count, a.ldt = ldt, a.ldg = ldg;
    const int rc = check_theta_call(c, "apm_laplace_grad", a,
                                    [&] { return !thetas || !grad || !status; });
    if (rc != APM_SUCCESS) return rc;
    return ctx_call(c, SKEW, [&] {
        upload_thetas(c, count, thetas, ldt);
        std::vector<double> val((size_t)count), gh((size_t)count * c->P);
        if (laplace_then_live(c, (int)count, val.data(), status, n_iter)) {
            grad_buffers(c);
            grad_block(c, (int)count);
            HIPC(hipMemcpyAsync(gh.data(), c->gout, sizeof(double) * count * c->P,
                                hipMemcpyDeviceToHost, c->stream));
            sync(c);
        }
        rows_out(lml, 1, val, count, 1);
        rows_out(grad, ldg, gh, count, c->P);
        finish_rows(count, status, {{grad, ldg, c->P}}, {lml});
    });
}

int apm_laplace(int device, const double* K, int64_t n, int64_t ldk, const double* y,
                int calc_cov, int calc_lml, double diff_f_tol, int64_t max_iters, double* f_out,
                double* C_out, int64_t ldc, double* lml_out, int64_t* n_iter_out, int* status) {
    return apm_laplace_lik(device, APM_LIK_PROBIT, K, n, ldk, y, calc_cov, calc_lml, diff_f_tol,
                           max_iters, f_out, C_out, ldc, lml_out, n_iter_out, status);
}

int apm_laplace_lik(int device, int lik, const double* K, int64_t n, int64_t ldk, const double* y,
                    int calc_cov, int calc_lml, double diff_f_tol, int64_t max_iters,
                    double* f_out, double* C_out, int64_t ldc, double* lml_out,
                    int64_t* n_iter_out, int* status) {
    if (!K || !y || n <= 0 || ldk < n || !f_out || !status || max_iters < 0 ||
        (calc_cov && (!C_out || ldc < n)) || (calc_lml && !lml_out) ||
        (lik != APM_LIK_PROBIT && lik != APM_LIK_LOGIT))
        return fail(nullptr, APM_E_INVALID, "apm_laplace: bad arguments");
    return cached_call(device, n, 0, APM_KERNEL_PRECOMPUTED, [&](apm_ctx*& c) {
        standalone_ctx(c, device, n, y);
        c->tol = diff_f_tol;
        c->max_iters = max_iters;
        c->lik = lik;  // (the shape's cached context serves both likelihoods)
        laplace_on_K(c, K, ldk, f_out, calc_cov ? C_out : nullptr, ldc,
                     calc_lml ? lml_out : nullptr, n_iter_out, status);
    });
}

// ---- expectation propagation (host_ep.cpp) -----------------------------------
namespace {

bool ep_settings_ok(double damping, double diff_tol, int64_t max_sweeps) {
    return damping > 0.0 && damping <= 1.0 && diff_tol >= 0.0 && max_sweeps >= 1;
}

}  // namespace

int apm_set_ep(apm_ctx* ctx, double damping, double diff_tol, int64_t max_sweeps) {
    if (!ctx || !ep_settings_ok(damping, diff_tol, max_sweeps))
        return fail(ctx, APM_E_INVALID, "apm_set_ep: bad arguments");
    if (ctx->lik != APM_LIK_PROBIT && !ctx->ep_quad)
        return fail(ctx, APM_E_INVALID, "apm_set_ep: probit only (the logit's tilted moments need "
                                        "quadrature)");
    ctx->ep_damping = damping;
    ctx->ep_tol = diff_tol;
    ctx->ep_max_sweeps = max_sweeps;
    return APM_SUCCESS;
}

int apm_set_ep_quadrature(apm_ctx* ctx, int on) {
    if (!ctx || (on != 0 && on != 1))
        return fail(ctx, APM_E_INVALID, "apm_set_ep_quadrature: bad arguments");
    ctx->ep_quad = on;
    return APM_SUCCESS;
}

int apm_ep_quadrature(const apm_ctx* ctx) { return ctx ? ctx->ep_quad : APM_E_INVALID; }

int apm_ep_eval(apm_ctx* c, int64_t count, const double* thetas, int64_t ldt, double* logz,
                double* mu, double* var, double* tau, double* nu, int64_t ldo, int* status,
                int64_t* n_sweeps) {
    ThetaArgs a;
    a.probit_only = a.batch = true;
    a.device_why = "needs an ISO or ARD context (apm_ep takes a K of the caller's)";
    a.count = count;
    const int rc = check_theta_call(c, "apm_ep_eval", a, [&] {
        return !thetas || !status || ldt < c->P || ((mu || var || tau || nu) && ldo < c->n);
    });
    if (rc != APM_SUCCESS) return rc;
    return ctx_call(c, SKEW, [&] {
        EpFit fit;
        ep_gram_fit(c, count, thetas, ldt, fit);
        std::vector<double> lz((size_t)count);
        HIPC(hipMemcpyAsync(lz.data(), c->ep.logz, sizeof(double) * count, hipMemcpyDeviceToHost,
                            c->stream));
        ep_fetch(c, mu, ldo, c->v.f, c->v.vstride, count);
        ep_fetch(c, var, ldo, c->ep.var, c->ep.stride, count);
        ep_fetch(c, tau, ldo, c->ep.tau, c->ep.stride, count);
        ep_fetch(c, nu, ldo, c->ep.nu, c->ep.stride, count);
        sync(c);
        ep_report(fit, count, status, n_sweeps);
        rows_out(logz, 1, lz, count, 1);
        finish_rows(count, status,
                    {{mu, ldo, c->n}, {var, ldo, c->n}, {tau, ldo, c->n}, {nu, ldo, c->n}}, {logz});
    });
}

int apm_ep_predict(apm_ctx* c, int64_t count, const double* thetas, int64_t ldt, const double* Xs,
                   int64_t m, int64_t ldxs, double* mean, double* var, double* prob, int64_t ldo,
                   int* status, int64_t* n_sweeps) {
    ThetaArgs a;
    a.probit_only = a.batch = a.rows = true;
    a.device_why = "needs an ISO or ARD context (the cross-covariance is built on the device)";
    a.count = count, a.m = m, a.ldo = ldo;
    const int rc = check_theta_call(c, "apm_ep_predict", a, [&] {
        return !thetas || !Xs || !status || ldt < c->P || ldxs < c->d;
    });
    if (rc != APM_SUCCESS) return rc;
    return ctx_call(c, SKEW, [&] {
        EpFit fit;
        ep_gram_fit(c, count, thetas, ldt, fit);
        sync(c);
        ep_report(fit, count, status, n_sweeps);
        // predict_block reads S^1/2 (v.Ws), a and the factor of each chain's last sweep
        if (fit.ok) predict_all(c, count, thetas, ldt, Xs, m, ldxs, mean, var, prob, ldo);
        finish_rows(count, status, {{mean, ldo, m}, {var, ldo, m}, {prob, ldo, m}});
    });
}

int apm_predict_joint(apm_ctx* c, int approx, int64_t count, const double* thetas, int64_t ldt,
                      const double* Xs, int64_t m, int64_t ldxs, double* mean, int64_t ldo,
                      double* cov, int64_t ldc, int64_t n_draws, const uint64_t* seeds,
                      const uint64_t* counters, double* draws, const double* ys,
                      double* joint_lpd, int* status, int64_t* n_iter) {
    ThetaArgs a;
    if (approx != APM_JOINT_LAPLACE && approx != APM_JOINT_EP)
        a.early = "APM_JOINT_LAPLACE or APM_JOINT_EP only";
    a.probit_only = approx == APM_JOINT_EP;
    a.device_why = "needs an ISO or ARD context (the cross-covariance is built on the device)";
    a.batch = true;
    a.count = count;
    a.rest_msg = "bad arguments, m outside [1, apm_padded_n] or n_draws outside [0, "
                 "APM_JOINT_MAX_DRAWS]";
    const int rc = check_theta_call(c, "apm_predict_joint", a, [&] {
        const bool sampled = draws || joint_lpd;
        return !thetas || !Xs || !status || ldt < c->P || ldxs < c->d || m < 1 || m > c->np ||
               (mean && ldo < m) || (cov && ldc < m) || n_draws < 0 ||
               n_draws > APM_JOINT_MAX_DRAWS || (sampled && (n_draws == 0 || !seeds || !counters)) ||
               (joint_lpd && !ys);
    });
    if (rc != APM_SUCCESS) return rc;
    return ctx_call(c, SKEW, [&] {
        int ok = 0;
        EpFit fit;  // (alive until the tail's synchronisation)
        if (approx == APM_JOINT_EP) {
            ep_gram_fit(c, count, thetas, ldt, fit);
            sync(c);
            ep_report(fit, count, status, n_iter);
            ok = fit.ok;
        } else {
            upload_thetas(c, count, thetas, ldt);
            std::vector<double> lml((size_t)count);
            ok = laplace_then_live(c, (int)count, lml.data(), status, n_iter);
        }
        if (ok)
            predict_joint_tail(c, (int)count, thetas, ldt, status, Xs, m, ldxs, mean, ldo, cov, ldc,
                               n_draws, seeds, counters, draws, ys, joint_lpd);
        finish_rows(count, status, {{mean, ldo, m}, {draws, n_draws * m, n_draws * m}},
                    {joint_lpd});
        for (int64_t b = 0; cov && b < count; ++b)  // (a block's rows are ldc apart, m wide)
            for (int64_t r = 0; status[b] != APM_STATUS_OK && r < m; ++r)
                std::fill(cov + (b * m + r) * ldc, cov + (b * m + r) * ldc + m,
                          std::numeric_limits<double>::quiet_NaN());
    });
}

int apm_ep_grad(apm_ctx* c, int64_t count, const double* thetas, int64_t ldt, double* logz,
                double* grad, int64_t ldg, int* status, int64_t* n_sweeps) {
    ThetaArgs a;
    a.probit_only = a.batch = a.lds = true;
    a.device_why = "needs an ISO or ARD context (dK/dtheta is built on the device)";
    a.count = count, a.ldt = ldt, a.ldg = ldg;
    const int rc =
        check_theta_call(c, "apm_ep_grad", a, [&] { return !thetas || !grad || !status; });
    if (rc != APM_SUCCESS) return rc;
    return ctx_call(c, SKEW, [&] {
        EpFit fit;
        ep_gram_fit(c, count, thetas, ldt, fit);
        std::vector<double> lz((size_t)count), gh((size_t)count * c->P);
        HIPC(hipMemcpyAsync(lz.data(), c->ep.logz, sizeof(double) * count, hipMemcpyDeviceToHost,
                            c->stream));
        if (fit.ok) {  // S^1/2 (v.Ws), a and the factor of each chain's last sweep are in place
            grad_buffers(c);
            ep_grad_block(c, (int)count);
            HIPC(hipMemcpyAsync(gh.data(), c->gout, sizeof(double) * count * c->P,
                                hipMemcpyDeviceToHost, c->stream));
        }
        sync(c);
        ep_report(fit, count, status, n_sweeps);
        rows_out(logz, 1, lz, count, 1);
        rows_out(grad, ldg, gh, count, c->P);
        finish_rows(count, status, {{grad, ldg, c->P}}, {logz});
    });
}

int apm_ep(int device, const double* K, int64_t n, int64_t ldk, const double* y, int calc_cov,
           double damping, double diff_tol, int64_t max_sweeps, double* mu_out, double* var_out,
           double* tau_out, double* nu_out, double* C_out, int64_t ldc, double* logz_out,
           int64_t* n_sweeps_out, int* status) {
    return apm_ep_lik(device, APM_LIK_PROBIT, K, n, ldk, y, calc_cov, damping, diff_tol,
                      max_sweeps, mu_out, var_out, tau_out, nu_out, C_out, ldc, logz_out,
                      n_sweeps_out, status);
}

int apm_ep_lik(int device, int lik, const double* K, int64_t n, int64_t ldk, const double* y,
               int calc_cov, double damping, double diff_tol, int64_t max_sweeps, double* mu_out,
               double* var_out, double* tau_out, double* nu_out, double* C_out, int64_t ldc,
               double* logz_out, int64_t* n_sweeps_out, int* status) {
    if (!K || !y || n <= 0 || ldk < n || !status || !ep_settings_ok(damping, diff_tol, max_sweeps) ||
        (calc_cov && (!C_out || ldc < n)) || (lik != APM_LIK_PROBIT && lik != APM_LIK_LOGIT))
        return fail(nullptr, APM_E_INVALID, "apm_ep: bad arguments");
    // (apm_laplace's cached context of the shape)
    return cached_call(device, n, 0, APM_KERNEL_PRECOMPUTED, [&](apm_ctx*& c) {
        standalone_ctx(c, device, n, y);
        c->ep_damping = damping;
        c->ep_tol = diff_tol;
        c->ep_max_sweeps = max_sweeps;
        c->lik = lik;  // (augmented() and the shared kernels read it)
        // the probit's moments are closed form, the logit's come by the rule
        c->ep_quad = lik == APM_LIK_LOGIT;
        std::vector<double> Kp;  // (alive until the syncs below)
        upload_padded_K(c, K, ldk, Kp);
        EpFit fit;
        ep_fit_counted(c, 1, fit);
        sync(c);
        ep_report(fit, 1, status, n_sweeps_out);
        finish_rows(1, status, {{mu_out, n, n}, {var_out, n, n}, {tau_out, n, n}, {nu_out, n, n}},
                    {logz_out});
        if (*status != APM_STATUS_OK) return;
        if (logz_out)
            HIPC(hipMemcpyAsync(logz_out, c->ep.logz, sizeof(double), hipMemcpyDeviceToHost,
                                c->stream));
        ep_fetch(c, mu_out, n, c->v.f, c->v.vstride, 1);
        ep_fetch(c, var_out, n, c->ep.var, c->ep.stride, 1);
        ep_fetch(c, tau_out, n, c->ep.tau, c->ep.stride, 1);
        ep_fetch(c, nu_out, n, c->ep.nu, c->ep.stride, 1);
        if (calc_cov) covariance_out(c, C_out, ldc);
        sync(c);
    });
}

int apm_selftest_tile(int device, const double* A, const double* B, double* C) {
    if (!A || !B || !C) return fail(nullptr, APM_E_INVALID, "apm_selftest_tile: null pointer");
    double* d = nullptr;
    try {
        HIPC(hipSetDevice(device));
        HIPC(hipMalloc(&d, sizeof(double) * 3 * 4096));
        HIPC(hipMemcpy(d, A, sizeof(double) * 4096, hipMemcpyHostToDevice));
        HIPC(hipMemcpy(d + 4096, B, sizeof(double) * 4096, hipMemcpyHostToDevice));
        HIPC(hipMemcpy(d + 8192, C, sizeof(double) * 4096, hipMemcpyHostToDevice));
        launch_tile_nt_test(d, d + 4096, d + 8192, nullptr);
        HIPC(hipMemcpy(C, d + 8192, sizeof(double) * 4096, hipMemcpyDeviceToHost));
        HIPC(hipFree(d));
    } catch (const HipError& e) {
        if (d) (void)hipFree(d);
        return fail(nullptr, APM_E_HIP, e.msg);
    }
    return APM_SUCCESS;
}

int apm_selftest_philox(int device, int64_t n, const uint32_t* in, uint32_t* out) {
    if (!in || !out || n <= 0 || n > (1 << 24))
        return fail(nullptr, APM_E_INVALID, "apm_selftest_philox: bad arguments");
    uint32_t* d = nullptr;
    try {
        HIPC(hipSetDevice(device));
        HIPC(hipMalloc(&d, sizeof(uint32_t) * 10 * n));
        HIPC(hipMemcpy(d, in, sizeof(uint32_t) * 6 * n, hipMemcpyHostToDevice));
        launch_philox_test(d, d + 6 * n, n, nullptr);
        HIPC(hipMemcpy(out, d + 6 * n, sizeof(uint32_t) * 4 * n, hipMemcpyDeviceToHost));
        HIPC(hipFree(d));
    } catch (const HipError& e) {
        if (d) (void)hipFree(d);
        return fail(nullptr, APM_E_HIP, e.msg);
    }
    return APM_SUCCESS;
}

int apm_guard_read(apm_ctx* c, int64_t count, double* r) {
    if (!c || !r || count <= 0 || count > c->max_batch)
        return fail(c, APM_E_INVALID, "apm_guard_read: bad arguments");
    return ctx_call(c, NO_SKEW, [&] {
        std::vector<double> h((size_t)4 * c->max_batch);
        HIPC(hipMemcpyAsync(h.data(), c->guard + 2 * c->max_batch, sizeof(double) * h.size(),
                            hipMemcpyDeviceToHost, c->stream));
        sync(c);
        for (int64_t b = 0; b < count; ++b)
            for (int k = 0; k < 4; ++k) r[4 * b + k] = h[(size_t)k * c->max_batch + b];
    });
}

int apm_prof_enable(apm_ctx* c, int on) {
    if (!c) return fail(c, APM_E_INVALID, "apm_prof_enable: null ctx");
    c->prof = on < 0 ? 0 : (on > 2 ? 2 : on);
    return APM_SUCCESS;
}

int apm_prof_marker(apm_ctx* c, int id) {
    if (!c || id < 0 || id > 3) return fail(c, APM_E_INVALID, "apm_prof_marker: bad arguments");
    return ctx_call(c, NO_SKEW, [&] {
        launch_marker(id, c->stream);
    });
}

int apm_prof_read(apm_ctx* c, int kind, double* total_ms, int64_t* launches, double* work,
                  int reset) {
    if (!c || kind < 0 || kind >= APM_PROF_NKINDS)
        return fail(c, APM_E_INVALID, "apm_prof_read: bad arguments");
    return ctx_call(c, NO_SKEW, [&] {
        sync(c);
        if (kind == APM_PROF_DF_TIMEOUTS || kind == APM_PROF_TRSV_TIMEOUTS) {
            unsigned long long* d = spin_words(c) + (kind == APM_PROF_TRSV_TIMEOUTS ? 1 : 0);
            unsigned long long h = 0;
            HIPC(hipMemcpy(&h, d, sizeof(h), hipMemcpyDeviceToHost));
            if (total_ms) *total_ms = 0.0;
            if (launches) *launches = (int64_t)h;
            if (work) *work = 0.0;
            if (reset) HIPC(hipMemset(d, 0, sizeof(h)));
            return;
        }
        if (kind == APM_PROF_POST64_RERUNS) {
            if (total_ms) *total_ms = 0.0;
            if (launches) *launches = c->n_post64;
            if (work) *work = 0.0;
            if (reset) c->n_post64 = 0;
            return;
        }
        if (kind == APM_PROF_ICM_CHECKS || kind == APM_PROF_GUARD) {
            int64_t& n = kind == APM_PROF_GUARD ? c->n_guard : c->n_icm_check;
            if (total_ms) *total_ms = 0.0;
            if (launches) *launches = n;
            if (work) *work = 0.0;
            if (reset) n = 0;
            return;
        }
        if (kind == APM_PROF_STATS) {
            if (total_ms) *total_ms = 0.0;
            if (launches) *launches = c->n_fp64_rerun;
            if (work) *work = (double)c->n_refine_steps;
            if (reset) c->n_fp64_rerun = c->n_refine_steps = 0;
            return;
        }
        double ms = 0.0, wk = 0.0;
        int64_t cnt = 0;
        for (const ProfRec& r : c->recs) {
            if (r.kind != kind) continue;
            float e = 0.f;
            HIPC(hipEventElapsedTime(&e, r.a, r.b));
            ms += e;
            wk += r.work;
            ++cnt;
        }
        if (total_ms) *total_ms = ms;
        if (launches) *launches = cnt;
        if (work) *work = wk;
        if (reset) {
            c->recs.clear();
            c->evnext = 0;
        }
    });
}

}  // extern "C"
