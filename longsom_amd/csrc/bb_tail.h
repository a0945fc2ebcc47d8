// The beta-binomial upper tail and Python's round(x, 4), shared by the step-1 call (call.hip) and the per-cell verdict (cellgeno.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace lsg {

// log of the beta-binomial pmf at m (scipy betabinom._logpmf written with lgamma)
__device__ __noinline__ double bb_logpmf(double m, double n, double a, double b) {
    return lgamma(n + 1.0) - lgamma(m + 1.0) - lgamma(n - m + 1.0) + lgamma(m + a) + lgamma(n - m + b) - lgamma(n + a + b) +
           lgamma(a + b) - lgamma(a) - lgamma(b);
}

// P(X >= k) for X ~ BetaBinomial(n, a, b), integer k.  pm0 = pmf(0), shared by the alts of one cell type.
__device__ __noinline__ double bb_upper_tail(uint32_t k, uint32_t n, double a, double b, double pm0, double lgcn) {
    if (k == 0) return 1.0;
    if (k > n) return 0.0;                         // 1 - sum of the whole pmf; canonical 0.0
    const double dn = (double)n;
    if ((uint64_t)k <= (uint64_t)n - k + 1) {      // lower side is shorter: 1 - sum_{m<k} pmf(m)
        double sum = pm0, pm = pm0;
        for (uint32_t m = 1; m < k; ++m) {
            if ((m & 1023u) == 0) pm = exp(bb_logpmf((double)m, dn, a, b));
            else { const double mm = (double)(m - 1); pm *= (dn - mm) * (mm + a) / ((mm + 1.0) * (dn - mm - 1.0 + b)); }
            sum += pm;
        }
        return 1.0 - sum;
    }
    // upper side: sum_{m=k}^{n} pmf(m), descending from pmf(n) = G(n+a) G(a+b) / (G(n+a+b) G(a))
    double pm = exp(lgamma(dn + a) - lgamma(dn + a + b) + lgcn);
    double sum = pm;
    uint32_t cnt = 1;
    for (uint32_t m = n; m > k;) {
        --m;
        if ((cnt & 1023u) == 0) pm = exp(bb_logpmf((double)m, dn, a, b));
        else { const double mm = (double)m; pm *= (mm + 1.0) * (dn - mm - 1.0 + b) / ((dn - mm) * (mm + a)); }
        sum += pm;
        ++cnt;
    }
    return sum;
}
__device__ __noinline__ double bb_pm0(uint32_t n, double a, double b, double lgc0) {
    const double dn = (double)n;                   // pmf(0) = G(n+b) G(a+b) / (G(n+a+b) G(b))
    return exp(lgamma(dn + b) - lgamma(dn + a + b) + lgc0);
}

// Python round(x, 4) * 10^4 as an integer: half-even on the exact binary value of x.
__device__ __forceinline__ int32_t round4(double x) {
    if (!(x > 0.0)) return 0;                      // negative fp noise and -0.0 print as 0.0 (canonical)
    const double hi = x * 1e4;
    const double lo = fma(x, 1e4, -hi);
    double k = rint(hi);                           // half-even
    const double d = (hi - k) + lo;                // exact distance to k unless |lo| is absorbed (then irrelevant)
    if (d > 0.5) k += 1.0;
    else if (d < -0.5) k -= 1.0;
    else if (d == 0.5 && (hi - k) != 0.5) { if (fmod(k, 2.0) != 0.0) k += 1.0; }
    else if (d == -0.5 && (hi - k) != -0.5) { if (fmod(k, 2.0) != 0.0) k -= 1.0; }
    return (int32_t)k;
}

} // namespace lsg
