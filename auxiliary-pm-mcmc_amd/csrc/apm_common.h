// Shared definitions for the MI355X (gfx950) APM hot path.
//
// Layout conventions:
//   * every matrix is row-major, fp64 unless stated, padded to Np = ceil(N/64)*64 so kernels
//     need no bounds checks; padded rows/cols are the identity (matrices) or zero (vectors);
//   * the lower triangle is the meaningful part of every factor; TB = 64 is the tile edge;
//   * batched objects carry an explicit per-chain stride and a `chain` grid dimension.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define APM_TB 64

typedef double d4_t __attribute__((ext_vector_type(4)));
typedef float f4_t __attribute__((ext_vector_type(4)));
typedef float f2_t __attribute__((ext_vector_type(2)));
typedef double d2_t __attribute__((ext_vector_type(2)));
// operands of __builtin_amdgcn_global_load_lds (LDS-DMA staging)
typedef __attribute__((address_space(3))) void lds_void_t;
typedef __attribute__((address_space(1))) void glb_void_t;

// per-chain status codes (mirrored in gpdemo/_native.py)
enum {
    APM_OK = 0,
    APM_ERR_CHOL_K = 1,        // chol(K) failed           -> numpy.linalg.LinAlgError
    APM_ERR_CHOL_B = 2,        // chol(B) failed (Newton)  -> numpy.linalg.LinAlgError
    APM_ERR_CHOL_C = 3,        // chol(C) failed           -> InvalidCovarianceMatrixError
    APM_ERR_MAXITER = 4,       // Newton did not converge  -> MaximumIterationsExceededError
};

// ---------------------------------------------------------------------------------------------
// log Phi(z) = log_ndtr(z), accurate over the whole real line (scipy.special.log_ndtr semantics):
//   z <  0 : log(erfcx(-z/sqrt2)/2) - z^2/2      (no underflow for very negative z)
//   z >= 0 : log1p(-erfc(z/sqrt2)/2)
__device__ __forceinline__ double log_ndtr_d(double z) {
    const double rs2 = 0.70710678118654752440;
    if (z < 0.0) return log(0.5 * erfcx(-z * rs2)) - 0.5 * z * z;
    return log1p(-0.5 * erfc(z * rs2));
}

__device__ __forceinline__ float log_ndtr_f(float z) {
    const float rs2 = 0.70710678118654752440f;
    if (z < 0.0f) return __logf(0.5f * erfcxf(-z * rs2)) - 0.5f * z * z;
    return log1pf(-0.5f * erfcf(z * rs2));
}

// log Phi(z) with the -z^2/2 of the negative branch in fp64 and the O(log|z|) remainder in fp32
// (the u-path epilogue, ugemm.hip: the large terms of the per-sample sum cancel in fp64; the
// fp32 part is bounded by ~1 + log|z| in magnitude, so its rounding stays below 1e-6 per entry)
__device__ __forceinline__ double log_ndtr_mixed(double z) {
    const float rs2 = 0.70710678118654752440f;
    const float zf = (float)z;
    if (z < 0.0) return (double)__logf(0.5f * erfcxf(-zf * rs2)) - 0.5 * z * z;
    return (double)log1pf(-0.5f * erfcf(zf * rs2));
}

// ---------------------------------------------------------------------------------------------
// The likelihood p(y | f) of a latent value, y in {-1, +1}: a template parameter
// LIK of the five kernels that evaluate it (k_newton_prep, k_laplace_lml, k_grad_rows, the u-path
// epilogue of k_ugemm / k_ugemm64, k_predict_reduce) and a launch-time switch of their launchers,
// as the covariance family FAM is. The values are include/apm.h's.
//   probit  p = Phi(y f)          v = phi(f)/Phi(y f), grad = y v, W = v^2 + grad f
//   logit   p = sigma(y f)        t = y f, grad = y sigma(-t), W = sigma(t) sigma(-t) in (0, 1/4]
#define APM_LIK_PROBIT 0
#define APM_LIK_LOGIT 1
#define APM_LIK_DISPATCH(lik, ...)                                                    \
    switch (lik) {                                                                    \
        case APM_LIK_LOGIT: { constexpr int LIK = APM_LIK_LOGIT; __VA_ARGS__; } break; \
        default: { constexpr int LIK = APM_LIK_PROBIT; __VA_ARGS__; } break;          \
    }

// sigma(u) = 1/(1 + e^-u) without overflow or cancellation on the whole line
__device__ __forceinline__ double sigmoid_d(double u) {
    const double e = exp(-fabs(u));
    const double r = 1.0 / (1.0 + e);
    return u >= 0.0 ? r : e * r;
}

// log sigma(t): -log1p(e^-t) for t >= 0, t - log1p(e^t) for t < 0 (accurate on the whole line,
// as log_ndtr_d)
__device__ __forceinline__ double log_sigmoid_d(double t) {
    if (t < 0.0) return t - log1p(exp(t));
    return -log1p(exp(-t));
}

// log sigma(t) with the linear part t of the negative branch in fp64 and the remainder
// log1p(e^-|t|) in (0, log 2] in fp32 (log_ndtr_mixed's twin for the u-path epilogue)
__device__ __forceinline__ double log_sigmoid_mixed(double t) {
    const float tf = (float)t;
    if (t < 0.0) return t - (double)log1pf(expf(tf));
    return -(double)log1pf(expf(-tf));
}

// log p(y | f) at t = y f
template <int LIK>
__device__ __forceinline__ double lik_logp(double t) {
    if constexpr (LIK == APM_LIK_LOGIT) return log_sigmoid_d(t);
    else return log_ndtr_d(t);
}
template <int LIK>
__device__ __forceinline__ double lik_logp_mixed(double t) {
    if constexpr (LIK == APM_LIK_LOGIT) return log_sigmoid_mixed(t);
    else return log_ndtr_mixed(t);
}

// grad = d log p / df and W = -d^2 log p / df^2 at f (lpa.py:86-88 for the probit). The logit's
// sigma(-t) is 1/(1 + e^t) itself, never 1 - sigma(t).
struct LikGW {
    double grad, W;
};
template <int LIK>
__device__ __forceinline__ LikGW lik_grad_W(double f, double yi) {
    if constexpr (LIK == APM_LIK_LOGIT) {
        const double t = yi * f;
        const double sm = sigmoid_d(-t);
        return LikGW{yi * sm, sigmoid_d(t) * sm};
    } else {
        const double vv = exp(-0.5 * f * f - log_ndtr_d(yi * f) - 0.91893853320467274178);
        const double grad = vv * yi;
        return LikGW{grad, vv * vv + grad * f};
    }
}

// grad and the third derivative d3 = d^3 log p / df^3 = -dW/df at f (gradient.hip); the logit's
// 1 - 2 sigma(t) is formed as sigma(-t) - sigma(t)
struct LikGD3 {
    double grad, d3;
};
template <int LIK>
__device__ __forceinline__ LikGD3 lik_grad_d3(double fi, double yi) {
    if constexpr (LIK == APM_LIK_LOGIT) {
        const double t = yi * fi;
        const double sp = sigmoid_d(t), sm = sigmoid_d(-t);
        return LikGD3{yi * sm, -yi * (sp * sm) * (sm - sp)};
    } else {
        const double v = exp(-0.5 * fi * fi - log_ndtr_d(yi * fi) - 0.91893853320467274178);
        const double d3 = -((2.0 * v + yi * fi) * (-fi * v - yi * v * v) + yi * v);
        return LikGD3{yi * v, d3};
    }
}

// wave64 reductions
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// |row[0 .. ncols)|^2 on every lane of a wave, in one order for every kernel that takes it
// (k_grad_rows, k_ep_sites, k_predict_reduce, k_is_rows): 16-byte pieces, lane l the pieces at
// columns 2l, 2l + 128, .. in order (fma on x, then on y), then the wave's butterfly. piece(c, v)
// sees every piece the lane loads (k_is_rows stores it reversed).
template <class F>
__device__ __forceinline__ double row_sqnorm_d2(const double* row, int ncols, int lane, F&& piece) {
    double s = 0.0;
    for (int c = 2 * lane; c < ncols; c += 128) {
        const d2_t v = *reinterpret_cast<const d2_t*>(row + c);
        s = fma(v.x, v.x, s);
        s = fma(v.y, v.y, s);
        piece(c, v);
    }
    return wave_sum_d(s);
}
__device__ __forceinline__ double row_sqnorm_d2(const double* row, int ncols, int lane) {
    return row_sqnorm_d2(row, ncols, lane, [](int, d2_t) {});
}
// pb[0] + pb[stride] + .. + pb[(nb - 1) stride] in order: a row's mu* from the partials that
// k_gram_cross leaves per tile column
__device__ __forceinline__ double sum_tile_partials(const double* pb, int nb, int64_t stride) {
    double s = 0.0;
    for (int tj = 0; tj < nb; ++tj) s += pb[tj * stride];
    return s;
}
__device__ __forceinline__ double wave_max_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    return v;
}

// block (<=1024 threads) sum into every thread; `red` needs blockDim/64 doubles of LDS
__device__ __forceinline__ double block_sum_d(double v, double* red) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    v = wave_sum_d(v);
    __syncthreads();
    if (lane == 0) red[w] = v;
    __syncthreads();
    double s = 0.0;
    for (int i = 0; i < nw; ++i) s += red[i];
    return s;
}
__device__ __forceinline__ double block_max_d(double v, double* red) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    v = wave_max_d(v);
    __syncthreads();
    if (lane == 0) red[w] = v;
    __syncthreads();
    double s = -INFINITY;
    for (int i = 0; i < nw; ++i) s = fmax(s, red[i]);
    return s;
}
