// Gauss-Hermite nodes and weights (weight exp(-x^2)) on the host, for the quadrature of bean_importance_marg.hpp.
// Plain C++, no device code.
//
// The nodes are the eigenvalues of the Jacobi matrix of the Hermite recurrence (zero diagonal, off-diagonal
// sqrt(k / 2), k = 1 .. Q - 1): bisection on its Sturm sequence brackets the i-th largest to a few ulps - no initial
// guesses to get wrong - and two Newton steps on the orthonormal recurrence
//     p_0 = pi^(-1/4),  p_(k+1) = x sqrt(2 / (k + 1)) p_k - sqrt(k / (k + 1)) p_(k-1),  p_Q' = sqrt(2 Q) p_(Q-1)
// polish it in long double.  The weights are the Christoffel numbers w_i = 1 / sum_(k < Q) p_k(x_i)^2.
// The rule is symmetric; only the Q / 2 positive nodes (Q even) are returned, ascending, with
//     lw_i = log w_i + x_i^2,
// so that  int f(u) du ~ sqrt(2) sigma sum_i exp(lw_i) [f(m + sqrt(2) sigma x_i) + f(m - sqrt(2) sigma x_i)].
#pragma once

#include <cmath>

namespace bean {

inline void gauss_hermite_half(int Q, double* x_out, double* lw_out) {
    const int H = Q / 2;
    for (int i = 0; i < H; ++i) {
        // the (H + 1 + i)-th smallest eigenvalue: the i-th positive one
        const int want = H + i;  // eigenvalues strictly below the root
        long double lo = 0.0L, hi = 2.0L * sqrtl((long double)Q) + 1.0L;
        for (int it = 0; it < 200 && hi - lo > 1e-18L * hi; ++it) {
            const long double mid = 0.5L * (lo + hi);
            // Sturm count: the eigenvalues below mid
            int below = 0;
            long double q = -mid;
            if (q < 0) ++below;
            for (int k = 1; k < Q; ++k) {
                if (q == 0.0L) q = 1e-300L;
                q = -mid - (0.5L * k) / q;
                if (q < 0) ++below;
            }
            if (below > want) hi = mid;
            else lo = mid;
        }
        long double x = 0.5L * (lo + hi), sum = 0.0L;
        for (int pass = 0; pass < 3; ++pass) {
            long double pm = 0.0L, p = 0.75112554446494248286L;  // pi^(-1/4)
            sum = p * p;
            for (int k = 0; k < Q; ++k) {
                const long double pn = x * sqrtl(2.0L / (k + 1)) * p - sqrtl((long double)k / (k + 1)) * pm;
                pm = p;
                p = pn;
                if (k + 1 < Q) sum += p * p;
            }
            if (pass < 2) x -= p / (sqrtl(2.0L * Q) * pm);
        }
        x_out[i] = (double)x;
        lw_out[i] = (double)(-logl(sum) + x * x);
    }
}

}  // namespace bean
