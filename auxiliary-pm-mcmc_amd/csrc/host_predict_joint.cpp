// The joint Laplace / EP predictive at test inputs (predict_joint.hip): what
// follows the fit on its last factor, for one block of m <= np test inputs. predict_block leaves
// V^T = (W^1/2 . k*)^T L^-T in the free rows [np, np + 64 mb) of A; with the test-test Gram seeded
// behind them its trailing updates leave Sigma = K** - V V^T in the lower tiles of A[np.., np..],
// which is copied out, given epsilon and factored in place by the fp64 schedule; the draws are the
// product of that factor with the normals.
#include "apm_host.h"

namespace apm_host {

namespace {

void release(apm_ctx* c, double*& p) {
    if (!p) return;
    c->allocs.erase(std::find(c->allocs.begin(), c->allocs.end(), (void*)p));
    HIPC(hipFree(p));
    p = nullptr;
}

// the draw buffers, for sp (a multiple of 64) rows of normals per chain
void joint_buffers(apm_ctx* c, int64_t sp, bool want_draws) {
    const int64_t np = c->np, B = c->max_batch;
    if (!c->jn_ys) {
        c->jn_ys = dalloc<double>(c, np);
        c->jn_keys = dalloc<uint64_t>(c, 2 * B);
    }
    if (sp > c->jn_cap) {
        sync(c);  // (nothing of an earlier call is in flight: every call ends synchronised)
        release(c, c->jn_xi);
        release(c, c->jn_part);
        release(c, c->jn_draws);
        c->jn_cap = sp;
    }
    if (!c->jn_xi) {
        c->jn_xi = dalloc<double>(c, B * c->jn_cap * np);
        c->jn_part = dalloc<double>(c, B * c->nb * c->jn_cap);
    }
    if (want_draws && !c->jn_draws) c->jn_draws = dalloc<double>(c, B * c->jn_cap * np);
}

}  // namespace

void predict_joint_tail(apm_ctx* c, int count, const double* thetas, int64_t ldt, int* st_h,
                        const double* Xs, int64_t m, int64_t ldxs, double* mean, int64_t ldo,
                        double* cov, int64_t ldc, int64_t n_draws, const uint64_t* seeds,
                        const uint64_t* counters, double* draws, const double* ys,
                        double* joint_lpd) {
    const Live lv = live_of(c);
    const int nb = c->nb;
    const int64_t np = c->np;
    TestInputs in(c, count, thetas, ldt, Xs, m, ldxs);
    const int ms = in.upload(0), mb = (ms + 63) / 64;
    launch_gram_test(c->A, np, c->pxs, ms, mb, c->d, c->theta, c->P, c->psig, c->pbet, c->plam,
                     c->kind, lv, count, c->stream);
    predict_block(c, count, ms, /*with_cov=*/true);
    in.rows_back(0, ms, nullptr, mean, nullptr, nullptr, ldo);
    if (cov)  // Sigma as the device has it, into the caller's blocks: the lower triangle counts
        for (int b = 0; b < count; ++b)
            if (st_h[b] == APM_STATUS_OK)
                HIPC(hipMemcpy2DAsync(cov + (int64_t)b * m * ldc, sizeof(double) * ldc,
                                      c->A.base + b * c->A.cstride + np * c->A.ld + np,
                                      sizeof(double) * c->A.ld, sizeof(double) * ms, ms,
                                      hipMemcpyDeviceToHost, c->stream));
    std::vector<int> st_d((size_t)count, 0);
    std::vector<double> lpd((size_t)count);
    if (draws || joint_lpd) {
        const int S = (int)n_draws, sp = (S + 63) / 64 * 64;
        const int64_t B = c->max_batch, ldx = 64 * mb, xstride = (int64_t)sp * ldx;
        joint_buffers(c, sp, draws != nullptr);
        launch_joint_eps(c->A, np, ms, c->eps, lv, count, c->stream);
        chol_factor(c, c->A, /*k0=*/nb, /*k1=*/nb + mb, /*R=*/nb + mb, /*Cb=*/nb + mb,
                    APM_STATUS_CHOL_C, count);
        HIPC(hipMemcpyAsync(c->jn_keys, seeds, sizeof(uint64_t) * count, hipMemcpyHostToDevice,
                            c->stream));
        HIPC(hipMemcpyAsync(c->jn_keys + B, counters, sizeof(uint64_t) * count,
                            hipMemcpyHostToDevice, c->stream));
        if (joint_lpd)
            HIPC(hipMemcpyAsync(c->jn_ys, ys, sizeof(double) * ms, hipMemcpyHostToDevice,
                                c->stream));
        HIPC(hipMemsetAsync(c->jn_xi, 0, sizeof(double) * count * xstride, c->stream));
        launch_joint_normal(c->jn_xi, xstride, ldx, c->jn_keys, c->jn_keys + B, ms, S, lv, count,
                            c->stream);
        const int64_t dstride = (int64_t)S * ms, pstride = (int64_t)mb * sp;
        launch_joint_draw(c->lik, c->A, np, ms, mb, c->jn_xi, xstride, ldx, S, sp, c->pmean, np,
                          joint_lpd ? c->jn_ys : nullptr, draws ? c->jn_draws : nullptr, dstride,
                          c->jn_part, pstride, lv, count, c->stream);
        if (joint_lpd) {
            launch_joint_lme(c->jn_part, pstride, mb, S, sp, c->out, lv, count, c->stream);
            HIPC(hipMemcpyAsync(lpd.data(), c->out, sizeof(double) * count, hipMemcpyDeviceToHost,
                                c->stream));
        }
        if (draws)
            for (int b = 0; b < count; ++b)
                if (st_h[b] == APM_STATUS_OK)
                    HIPC(hipMemcpyAsync(draws + b * dstride, c->jn_draws + b * dstride,
                                        sizeof(double) * dstride, hipMemcpyDeviceToHost,
                                        c->stream));
        HIPC(hipMemcpyAsync(st_d.data(), c->status, sizeof(int) * count, hipMemcpyDeviceToHost,
                            c->stream));
    }
    sync(c);
    for (int b = 0; b < count; ++b) {
        if (st_h[b] != APM_STATUS_OK) continue;
        if (st_d[b] != APM_STATUS_OK) {  // (the factor of Sigma + eps I alone can fail here)
            st_h[b] = st_d[b];
            continue;
        }
        if (joint_lpd) joint_lpd[b] = lpd[b];
        if (!cov) continue;
        double* Cb = cov + (int64_t)b * m * ldc;  // the mirror, in blocks that stay in cache
        for (int64_t i0 = 0; i0 < ms; i0 += 32)
            for (int64_t j0 = 0; j0 <= i0; j0 += 32)
                for (int64_t i = i0; i < std::min<int64_t>(i0 + 32, ms); ++i)
                    for (int64_t j = j0; j < std::min(j0 + 32, i); ++j)
                        Cb[j * ldc + i] = Cb[i * ldc + j];
    }
}

}  // namespace apm_host
