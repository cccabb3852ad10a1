// lr_dense.h -- the host side of the dense NUTS metric (include/logreg_hip_dense.h): the factorisation of the inverse metric and the
// image of it the kernel reads (lr_nuts_dense.h).  Host code only, no device call: lr_api.hip and tests/host/dense_harness.cpp include it.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdio>
#include <vector>

namespace lr {

constexpr int kDenseMaxP = 32;

// s, R, A of include/logreg_hip_dense.h "Factorisation" (each [p] / [p][p], may be null).  -> 0, or -1 with the reason in `why`.
inline int dense_factor(int p, const double* sigma, double* s_out, double* R_out, double* A_out, char* why, size_t why_len) {
#pragma clang fp contract(off)
    if (p < 1 || p > kDenseMaxP) {
        std::snprintf(why, why_len, "p must be in 1..%d (got %d)", kDenseMaxP, p);
        return -1;
    }
    double s[kDenseMaxP], R[kDenseMaxP][kDenseMaxP], L[kDenseMaxP][kDenseMaxP], A[kDenseMaxP][kDenseMaxP];
    for (int i = 0; i < p; ++i)
        for (int j = 0; j <= i; ++j)
            if (!std::isfinite(sigma[i * p + j])) {
                std::snprintf(why, why_len, "inv_metric[%d][%d] is not finite", i, j);
                return -1;
            }
    for (int j = 0; j < p; ++j) {
        if (!(sigma[j * p + j] > 0)) {
            std::snprintf(why, why_len, "inv_metric[%d][%d] = %g must be > 0", j, j, sigma[j * p + j]);
            return -1;
        }
        s[j] = std::sqrt(sigma[j * p + j]);
    }
    for (int i = 0; i < p; ++i) {
        for (int j = 0; j < i; ++j) {
            const double d = s[i] * s[j];
            R[i][j] = R[j][i] = sigma[i * p + j] / d;
        }
        R[i][i] = 1.0;
    }
    for (int i = 0; i < p; ++i)
        for (int j = 0; j < p; ++j) L[i][j] = A[i][j] = 0.0;
    for (int i = 0; i < p; ++i)
        for (int j = 0; j <= i; ++j) {
            double t = R[i][j];
            for (int k = 0; k < j; ++k) {
                const double q = L[i][k] * L[j][k];
                t = t - q;
            }
            if (i == j) {
                if (!(t > 0) || !std::isfinite(t)) {
                    std::snprintf(why, why_len, "inv_metric is not positive definite: pivot %d of its correlation matrix is %g", i, t);
                    return -1;
                }
                L[i][i] = std::sqrt(t);
            } else {
                L[i][j] = t / L[j][j];
            }
        }
    for (int c = 0; c < p; ++c)
        for (int i = c; i >= 0; --i) {
            double t = i == c ? 1.0 : 0.0;
            for (int k = i + 1; k <= c; ++k) {
                const double q = L[k][i] * A[k][c];
                t = t - q;
            }
            A[i][c] = t / L[i][i];
        }
    for (int i = 0; i < p; ++i) {
        if (s_out) s_out[i] = s[i];
        for (int j = 0; j < p; ++j) {
            if (R_out) R_out[i * p + j] = R[i][j];
            if (A_out) A_out[i * p + j] = A[i][j];
        }
    }
    return 0;
}

// what the kernel reads: (T) s | (T)(1 / s) | (T) R [P][P] | (T) A [P][P], zero in padded rows and columns
template <typename T, int P> void dense_factor_image(int p, const double* s, const double* R, const double* A, std::vector<unsigned char>* img) {
    std::vector<T> f((size_t)2 * P + (size_t)2 * P * P, T(0));
    for (int i = 0; i < p; ++i) {
        f[i] = (T)s[i];
        f[P + i] = (T)(1.0 / s[i]);
        for (int j = 0; j < p; ++j) {
            f[2 * P + (size_t)i * P + j] = (T)R[i * p + j];
            f[2 * P + (size_t)P * P + (size_t)i * P + j] = (T)A[i * p + j];
        }
    }
    img->assign(reinterpret_cast<const unsigned char*>(f.data()), reinterpret_cast<const unsigned char*>(f.data()) + f.size() * sizeof(T));
}

}  // namespace lr
