// BnpC's sampler for the model with fixed error rates (CellClustering/libs/CRP.py:17-410, libs/MCMC.py:200-388): Gibbs assignment sweeps,
// the Escobar-West concentration update and the parameter Metropolis-Hastings, every chain of a run in every kernel.  The stream, the
// variates and the order of a step are defined in longsom_amd/bnpc_sampler.py's docstring; its numpy twin is what these kernels are held
// to.  See include/longsom_hip.h, lsg_bnpcs_*.  Everything is fp64 except theta.
#include "lsg_ctx.h"
#include <algorithm>
#include <cmath>

namespace lsg {

constexpr double S_TMIN = 1e-5, S_TMAX = 1 - 1e-5;
constexpr double S_EPS = 1e-15;                       // np.finfo(np.float64).resolution
constexpr int S_TRIES = 64;                           // Marsaglia-Tsang tries before the mean is written and an error counted
enum { P_PERM = 1, P_CHOICE, P_BIRTH, P_BIRTH_B, P_DPA, P_ETA, P_ETA_B, P_ALPHA, P_MH, P_INIT_LABEL, P_INIT_THETA };
constexpr int LT = 16;                                // k_bnpcs_ll: cells x columns per workgroup
constexpr int REC = 5;                                // doubles recorded per chain and step: ML, the CRP prior sum, the beta prior sum, live clusters, alpha

// what every kernel reads: the shape, the constants and where the state lies.  Per chain c: lab, size, colof, live, prow at c * N (prow:
// c * (N + 1)); theta, L1, L0, n1, n0 at c * N * M; LL at c * N * ll_pitch.
struct SDev {
    int32_t N, M, W, C, steps1, ll_pitch;
    int64_t arena_rows;
    double FN, FP, omFN, omFP, p, q, g0, g1, dpa_prob, new1, new0, betaln;
    int32_t uniform;
    const uint64_t *one, *zero, *seeds;
    const int32_t* pop;                               // [N][2]: ones, zeros
    int32_t *lab, *size, *colof, *live, *nlive, *hi, *order, *rec_lab, *err;
    float *theta, *arena;
    double *L1, *L0, *LL, *alpha, *prow, *rowml, *rowb, *rec_sc;
    uint32_t *n1, *n0;
    uint64_t* keys;
};

// ---- the stream ----------------------------------------------------------------------------------------------------------------
__host__ __device__ inline void philox4x32(uint64_t key, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t w[4]) {
    uint32_t k0 = (uint32_t)key, k1 = (uint32_t)(key >> 32);
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    w[0] = c0; w[1] = c1; w[2] = c2; w[3] = c3;
}

__host__ __device__ inline double to_double(uint32_t lo, uint32_t hi) { return ((double)((((uint64_t)hi << 32) | lo) >> 12) + 0.5) * 0x1p-52; }

__device__ inline void doubles(uint64_t key, uint32_t index, uint32_t step, uint32_t purpose, uint32_t attempt, double& a, double& b) {
    uint32_t w[4];
    philox4x32(key, index, step, purpose, attempt, w);
    a = to_double(w[0], w[1]); b = to_double(w[2], w[3]);
}

// ---- the variates ----------------------------------------------------------------------------------------------------------------
__device__ double gamma_variate(uint64_t key, uint32_t index, uint32_t step, uint32_t purpose, double a, int32_t* err) {
    const double a1 = a < 1.0 ? a + 1.0 : a, d = a1 - 1.0 / 3.0, c = 1.0 / sqrt(9.0 * d);
    for (int t = 0; t < S_TRIES; ++t) {
        double u1, u2, u3, u4;
        doubles(key, index, step, purpose, 2u * t, u1, u2);
        doubles(key, index, step, purpose, 2u * t + 1u, u3, u4);
        const double x = sqrt(-2.0 * log(u1)) * cos(2.0 * M_PI * u2);
        const double base = 1.0 + c * x, v = base * base * base;
        if (v > 0.0 && log(u3) < 0.5 * x * x + d - d * v + d * log(v)) {
            double g = d * v;
            if (a < 1.0) g *= pow(u4, 1.0 / a);
            return g;
        }
    }
    atomicAdd(err, 1);
    return a;
}

__device__ double beta_variate(uint64_t key, uint32_t index, uint32_t step, uint32_t purpose, double a, double b, int32_t* err) {
    const double x = gamma_variate(key, index, step, purpose, a, err), y = gamma_variate(key, index, step, purpose + 1u, b, err);
    const double s = x + y;
    return s > 0.0 ? x / s : 0.5;
}

__device__ inline double f32diff(float bound, float x) { return (double)(bound - x); }

__device__ inline float truncnorm_variate(double u, float old, double sd) {
    const double pa = normcdf(f32diff((float)S_TMIN, old) / sd), pb = normcdf(f32diff((float)S_TMAX, old) / sd);
    return (float)((double)old + sd * normcdfinv(pa + u * (pb - pa)));
}

__device__ inline double truncnorm_logpdf(float x, float loc, double sd) {
    const double pa = normcdf(f32diff((float)S_TMIN, loc) / sd), pb = normcdf(f32diff((float)S_TMAX, loc) / sd);
    const double z = (double)(x - loc) / sd;
    return -0.5 * z * z - 0.5 * log(2.0 * M_PI) - log(sd) - log(pb - pa);
}

__device__ inline void log_terms(const SDev& d, float theta, double& l1, double& l0) {
    const double th = (double)theta, om = (double)(1.0f - theta);
    l1 = log(th * d.omFN + om * d.FP);
    l0 = log(th * d.FN + om * d.omFP);
}

__device__ inline double beta_logpdf(const SDev& d, float theta) {
    const double x = (double)theta;
    return (d.q - 1.0) * log1p(-x) + (d.p - 1.0) * log(x) - d.betaln;
}

// ---- reductions over a workgroup of 256 (four waves): every lane gets the result; sh holds 4 -------------------------------------
__device__ inline double block_max(double v, double* sh) {
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    v = fmax(fmax(sh[0], sh[1]), fmax(sh[2], sh[3]));
    __syncthreads();
    return v;
}

__device__ inline double block_sum(double v, double* sh) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    v = (sh[0] + sh[1]) + (sh[2] + sh[3]);
    __syncthreads();
    return v;
}

__device__ inline int block_min_int(int v, int* sh) {
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    v = min(min(sh[0], sh[1]), min(sh[2], sh[3]));
    __syncthreads();
    return v;
}

// ---- counts: n1 / n0 [chain][cluster][mutation] from the masks and the labels (zeroed before).  A lane per cell. ------------------------
__global__ __launch_bounds__(256) void k_bnpcs_counts(SDev d) {
    const int c = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= d.N) return;
    const int32_t l = d.lab[(size_t)c * d.N + i];
    uint32_t* n1 = d.n1 + ((size_t)c * d.N + l) * d.M;
    uint32_t* n0 = d.n0 + ((size_t)c * d.N + l) * d.M;
    for (int w = 0; w < d.W; ++w) {
        uint64_t o = d.one[(size_t)i * d.W + w], z = d.zero[(size_t)i * d.W + w];
        while (o) { const int b = __ffsll((unsigned long long)o) - 1; atomicAdd(&n1[w * 64 + b], 1u); o &= o - 1; }
        while (z) { const int b = __ffsll((unsigned long long)z) - 1; atomicAdd(&n0[w * 64 + b], 1u); z &= z - 1; }
    }
}

// ---- tables: L1 / L0 of every live cluster, and per cluster the likelihood sum_m n1 L1 + n0 L0 and the beta prior's log density of its
// parameters.  A wave per (cluster, chain). -----------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_bnpcs_tables(SDev d) {
    const int c = blockIdx.y, k = blockIdx.x;
    const size_t row = (size_t)c * d.N + k;
    double ml = 0.0, bp = 0.0;
    if (d.size[row] > 0)
        for (int m = threadIdx.x; m < d.M; m += 64) {
            const float th = d.theta[row * d.M + m];
            double l1, l0;
            log_terms(d, th, l1, l0);
            d.L1[row * d.M + m] = l1; d.L0[row * d.M + m] = l0;
            ml += (double)d.n1[row * d.M + m] * l1 + (double)d.n0[row * d.M + m] * l0;
            if (!d.uniform) bp += beta_logpdf(d, th);
        }
    for (int o = 32; o > 0; o >>= 1) { ml += __shfl_xor(ml, o, 64); bp += __shfl_xor(bp, o, 64); }
    if (threadIdx.x == 0) { d.rowml[row] = ml; d.rowb[row] = bp; }
}

// ---- live: the clusters alive, ascending (live[j]), their column (colof[cluster], -1 for a free id), their number and hi = the largest + 1.
// A workgroup per chain; a lane owns a run of ids. ----------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_bnpcs_live(SDev d) {
    __shared__ int cnt[256];
    const int c = blockIdx.x, t = threadIdx.x;
    const int32_t* size = d.size + (size_t)c * d.N;
    const int ch = (d.N + 255) / 256, k0 = min(t * ch, d.N), k1 = min(k0 + ch, d.N);
    int n = 0;
    for (int k = k0; k < k1; ++k) n += size[k] > 0;
    cnt[t] = n;
    __syncthreads();
    int at = 0;
    for (int j = 0; j < t; ++j) at += cnt[j];
    for (int k = k0; k < k1; ++k) {
        if (size[k] > 0) { d.live[(size_t)c * d.N + at] = k; d.colof[(size_t)c * d.N + k] = at; ++at; }
        else d.colof[(size_t)c * d.N + k] = -1;
    }
    if (t == 255) d.nlive[c] = at;
    __syncthreads();
    if (t == 0) { const int K = d.nlive[c]; d.hi[c] = K ? d.live[(size_t)c * d.N + K - 1] + 1 : 0; }
}

// ---- likelihood: LL[chain][cell][column] = sum_m one L1 + zero L0 against the clusters alive at the sweep's start.  16 cells x 16 columns
// per workgroup; the tables of 64 mutations at a time go through LDS ([mutation][column], padded), a lane walks its cell's two mask words.
__global__ __launch_bounds__(256) void k_bnpcs_ll(SDev d) {
    __shared__ double s1[64][LT + 1], s0[64][LT + 1];
    const int c = blockIdx.z, K = d.nlive[c];
    const int col0 = blockIdx.x * LT, cell0 = blockIdx.y * LT;
    if (col0 >= K) return;
    const int tx = threadIdx.x & (LT - 1), ty = threadIdx.x >> 4;
    const int cell = cell0 + ty, col = col0 + tx;
    double acc = 0.0;
    for (int w = 0; w < d.W; ++w) {
        __syncthreads();
        for (int e = threadIdx.x; e < LT * 64; e += 256) {
            const int cc = e >> 6, m = e & 63, mm = w * 64 + m;
            double a = 0.0, b = 0.0;
            if (col0 + cc < K && mm < d.M) {
                const size_t at = ((size_t)c * d.N + d.live[(size_t)c * d.N + col0 + cc]) * d.M + mm;
                a = d.L1[at]; b = d.L0[at];
            }
            s1[m][cc] = a; s0[m][cc] = b;
        }
        __syncthreads();
        const uint64_t o = cell < d.N ? d.one[(size_t)cell * d.W + w] : 0, z = cell < d.N ? d.zero[(size_t)cell * d.W + w] : 0;
#pragma unroll 8
        for (int m = 0; m < 64; ++m) acc += ((o >> m) & 1) ? s1[m][tx] : ((z >> m) & 1) ? s0[m][tx] : 0.0;
    }
    if (cell < d.N && col < K) d.LL[((size_t)c * d.N + cell) * d.ll_pitch + col] = acc;
}

// ---- the permutation of the cells: ascending by (64-bit draw, index).  keys first, then each cell's rank by counting. -----------------------
__global__ __launch_bounds__(256) void k_bnpcs_keys(SDev d, uint32_t step) {
    const int c = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= d.N) return;
    uint32_t w[4];
    philox4x32(d.seeds[c], (uint32_t)i, step, P_PERM, 0, w);
    d.keys[(size_t)c * d.N + i] = ((uint64_t)w[1] << 32) | w[0];
}

__global__ __launch_bounds__(256) void k_bnpcs_perm(SDev d) {
    __shared__ uint64_t tile[256];
    const int c = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    const uint64_t* keys = d.keys + (size_t)c * d.N;
    const uint64_t mine = i < d.N ? keys[i] : 0;
    int rank = 0;
    for (int j0 = 0; j0 < d.N; j0 += 256) {
        __syncthreads();
        tile[threadIdx.x] = j0 + (int)threadIdx.x < d.N ? keys[j0 + threadIdx.x] : ~0ull;
        __syncthreads();
        const int n = min(256, d.N - j0);
        for (int j = 0; j < n; ++j) rank += (tile[j] < mine) || (tile[j] == mine && j0 + j < i);
    }
    if (i < d.N) d.order[(size_t)c * d.N + rank] = i;
}

// a cell against one cluster from the cluster's own tables: a masked sum over the mutations
__device__ inline double ll_direct(const SDev& d, int c, int cell, int k) {
    const double* l1 = d.L1 + ((size_t)c * d.N + k) * d.M;
    const double* l0 = d.L0 + ((size_t)c * d.N + k) * d.M;
    double acc = 0.0;
    for (int w = 0; w < d.W; ++w) {
        uint64_t o = d.one[(size_t)cell * d.W + w], z = d.zero[(size_t)cell * d.W + w];
        while (o) { acc += l1[w * 64 + __ffsll((unsigned long long)o) - 1]; o &= o - 1; }
        while (z) { acc += l0[w * 64 + __ffsll((unsigned long long)z) - 1]; z &= z - 1; }
    }
    return acc;
}

// ---- the sweep: one workgroup per chain walks the permuted cells (update_assignments_Gibbs, CRP.py:254-288), then the concentration
// update (update_DP_alpha, :386-410).  No workgroup waits for another.  A lane owns a run of cluster ids, so the running sum of the
// probabilities keeps the ids' order.  A cluster alive at the sweep's start reads its column of LL; one born in the sweep, or an id that
// emptied and was issued again, has colof = -1 and is evaluated from its own tables (the stale-column rule).
__global__ __launch_bounds__(256) void k_bnpcs_scan(SDev d, uint32_t step) {
    __shared__ double shd[4];
    __shared__ int shi[4];
    __shared__ double pref[4];
    __shared__ int s_pick;
    const int c = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6, N = d.N;
    const uint64_t key = d.seeds[c];
    int32_t* lab = d.lab + (size_t)c * N; int32_t* size = d.size + (size_t)c * N; int32_t* colof = d.colof + (size_t)c * N;
    const int32_t* order = d.order + (size_t)c * N;
    double* prow = d.prow + (size_t)c * (N + 1);
    const double alpha = d.alpha[c], lden = log((double)(N - 1) + alpha), lnew = log(alpha) - lden, log_eps = log(S_EPS);
    int hi = d.hi[c];
    for (int n = 0; n < N; ++n) {
        const int cell = order[n];
        const int old = lab[cell];
        __syncthreads();
        if (t == 0) { const int sz = size[old] - 1; size[old] = sz; if (sz == 0) colof[old] = -1; s_pick = hi; }
        __syncthreads();
        // slots 0 .. hi-1 are cluster ids, slot hi is the new cluster
        const int ch = (hi + 1 + 255) / 256, k0 = min(t * ch, hi + 1), k1 = min(k0 + ch, hi + 1);
        double mx = -INFINITY;
        for (int k = k0; k < k1; ++k) {
            double lp = -INFINITY;
            if (k == hi) lp = ((double)d.pop[2 * cell] * d.new1 + (double)d.pop[2 * cell + 1] * d.new0) + lnew;
            else {
                const int sz = size[k];
                if (sz > 0) {
                    const int col = colof[k];
                    const double ll = col >= 0 ? d.LL[((size_t)c * N + cell) * d.ll_pitch + col] : ll_direct(d, c, cell, k);
                    lp = ll + (log((double)sz) - lden);
                }
            }
            prow[k] = lp;
            mx = fmax(mx, lp);
        }
        mx = block_max(mx, shd);
        double sum = 0.0;
        for (int k = k0; k < k1; ++k) { const double lp = prow[k]; if (lp != -INFINITY) sum += exp(lp - mx); }
        sum = block_sum(sum, shd);
        const double lz = log1p(sum - 1.0);                       // the maximum's own term is exactly 1 (_normalize_log_probs leaves it out)
        double ps = 0.0;
        for (int k = k0; k < k1; ++k) {
            const double lp = prow[k];
            const double p = lp != -INFINITY ? exp(fmin(fmax(lp - mx - lz, log_eps), 0.0)) : 0.0;
            prow[k] = p; ps += p;
        }
        // running sum over the lanes in id order: within a wave, then over the four waves
        double inc = ps;
        for (int o = 1; o < 64; o <<= 1) { const double up = __shfl_up(inc, o, 64); if (lane >= o) inc += up; }
        if (lane == 63) pref[wave] = inc;
        __syncthreads();
        double before = inc - ps;
        for (int w = 0; w < wave; ++w) before += pref[w];
        const double total = ((pref[0] + pref[1]) + pref[2]) + pref[3];
        double u, u_unused;
        doubles(key, (uint32_t)cell, step, P_CHOICE, 0, u, u_unused);
        double run = before;
        for (int k = k0; k < k1; ++k) {
            const double p = prow[k];
            if (p == 0.0) continue;
            run += p;
            if (run / total > u) { atomicMin(&s_pick, k); break; }
        }
        __syncthreads();
        const int pick = s_pick;
        if (pick >= hi) {
            // a new cluster: the smallest free id, its parameters drawn from the cell (_init_cl_params_new), its tables made here
            int fr = hi;
            for (int k = k0; k < k1 && k < hi; ++k) if (size[k] == 0) { fr = k; break; }
            const int slot = block_min_int(fr, shi);
            const size_t row = (size_t)c * N + slot;
            for (int m = t; m < d.M; m += 256) {
                const int w = m >> 6, b = m & 63;
                const double a1 = d.p + (double)((d.one[(size_t)cell * d.W + w] >> b) & 1), b1 = d.q + (double)((d.zero[(size_t)cell * d.W + w] >> b) & 1);
                const double x = beta_variate(key, (uint32_t)m, step, (uint32_t)P_BIRTH | ((uint32_t)cell << 8), a1, b1, d.err + c);
                const float th = (float)fmin(fmax(x, S_TMIN), S_TMAX);
                double l1, l0;
                log_terms(d, th, l1, l0);
                d.theta[row * d.M + m] = th; d.L1[row * d.M + m] = l1; d.L0[row * d.M + m] = l0;
            }
            if (t == 0) { size[slot] = 1; colof[slot] = -1; lab[cell] = slot; }
            hi = max(hi, slot + 1);
        } else if (t == 0) { size[pick] += 1; lab[cell] = pick; }
    }
    __syncthreads();
    // the concentration update
    const int chn = (N + 255) / 256;
    double kk = 0.0;
    for (int k = min(t * chn, N); k < min(t * chn + chn, N); ++k) kk += size[k] > 0;
    kk = block_sum(kk, shd);
    if (t == 0) {
        double u0, u1;
        doubles(key, 0, step, P_DPA, 0, u0, u1);
        if (u0 < d.dpa_prob) {
            const double eta = beta_variate(key, 0, step, P_ETA, alpha + 1.0, (double)N, d.err + c);
            const double scale = d.g1 - log(eta);
            const double w = (d.g0 + kk - 1.0) / ((double)N * scale);
            const double pi_eta = w / (1.0 + w);
            const double g = gamma_variate(key, 0, step, P_ALPHA, u1 < pi_eta ? d.g0 + kk : d.g0 + kk - 1.0, d.err + c);
            d.alpha[c] = fmax(1.0 + S_EPS, g * scale);
        }
    }
}

// ---- the parameter move (MH_cluster_params / _get_log_A, :314-383): a lane per (mutation, live cluster, chain) ------------------------------
__global__ __launch_bounds__(64) void k_bnpcs_mh(SDev d, uint32_t step) {
    const int c = blockIdx.z, j = blockIdx.y, m = blockIdx.x * 64 + threadIdx.x;
    if (j >= d.nlive[c] || m >= d.M) return;
    const int k = d.live[(size_t)c * d.N + j];
    const size_t at = ((size_t)c * d.N + k) * d.M + m;
    const uint64_t key = d.seeds[c];
    const uint32_t pw = (uint32_t)P_MH | ((uint32_t)k << 8);
    double u, v;
    doubles(key, (uint32_t)m, step, pw, 0, u, v);
    uint32_t w[4];
    philox4x32(key, (uint32_t)m, step, pw, 1, w);
    const uint32_t pick = w[0] % 3u;
    const double sd = pick == 0 ? 0.1 : pick == 1 ? 0.25 : 0.5;
    const float old = d.theta[at];
    const float nw = truncnorm_variate(u, old, sd);
    const double n1 = (double)d.n1[at], n0 = (double)d.n0[at];
    double nl1, nl0, ol1, ol0;
    log_terms(d, nw, nl1, nl0);
    log_terms(d, old, ol1, ol0);
    const double new_ll = n1 * nl1 + n0 * nl0, old_ll = n1 * ol1 + n0 * ol0;
    const double new_prior = d.uniform ? 0.0 : beta_logpdf(d, nw), old_prior = d.uniform ? 0.0 : beta_logpdf(d, old);
    const double new_p = truncnorm_logpdf(nw, old, sd), old_p = truncnorm_logpdf(old, nw, sd);
    const double A = new_ll + new_prior - old_ll - old_prior + old_p - new_p;
    if (log(v) < A) d.theta[at] = nw;
}

// ---- record (Chain.update_results, MCMC.py:242-282): ML, the two prior sums, the labels, and after burn-in the live clusters' parameters
// in ascending id into the arena.  A workgroup per chain. ------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_bnpcs_record(SDev d, int32_t step, int32_t keep, const int64_t* used) {
    __shared__ double shd[4];
    const int c = blockIdx.x, t = threadIdx.x, N = d.N, K = d.nlive[c];
    const int32_t* live = d.live + (size_t)c * N;
    const double alpha = d.alpha[c], lden = log((double)(N - 1) + alpha);
    const int ch = (K + 255) / 256;
    double ml = 0.0, crp = 0.0, bp = 0.0;
    for (int j = min(t * ch, K); j < min(t * ch + ch, K); ++j) {
        const size_t row = (size_t)c * N + live[j];
        ml += d.rowml[row]; bp += d.rowb[row];
        crp += log((double)d.size[row]) - lden;
    }
    ml = block_sum(ml, shd); crp = block_sum(crp, shd); bp = block_sum(bp, shd);
    if (t == 0) {
        double* r = d.rec_sc + ((size_t)c * d.steps1 + step) * REC;
        r[0] = ml; r[1] = crp; r[2] = bp; r[3] = (double)K; r[4] = alpha;
    }
    for (int i = t; i < N; i += 256) d.rec_lab[((size_t)c * d.steps1 + step) * N + i] = d.lab[(size_t)c * N + i];
    if (keep) {
        float* dst = d.arena + ((size_t)c * d.arena_rows + used[c]) * d.M;
        for (int64_t e = t; e < (int64_t)K * d.M; e += 256) {
            const int j = (int)(e / d.M), m = (int)(e - (int64_t)j * d.M);
            dst[e] = d.theta[((size_t)c * N + live[j]) * d.M + m];
        }
    }
}

// ---- test support: the stream and the variates as the kernels see them -----------------------------------------------------------------
__global__ void k_bnpcs_test_stream(uint64_t key, int64_t n, const uint32_t* ctr, uint32_t* words, double* dbl) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t w[4];
    philox4x32(key, ctr[4 * i], ctr[4 * i + 1], ctr[4 * i + 2], ctr[4 * i + 3], w);
    for (int k = 0; k < 4; ++k) words[4 * i + k] = w[k];
    dbl[2 * i] = to_double(w[0], w[1]); dbl[2 * i + 1] = to_double(w[2], w[3]);
}

__global__ void k_bnpcs_test_variates(uint64_t key, int32_t kind, int64_t n, double a, double b, double* out, int32_t* err) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (kind == 0) out[i] = beta_variate(key, (uint32_t)i, 0, P_BIRTH, a, b, err);
    else if (kind == 1) { double u, v; doubles(key, (uint32_t)i, 0, P_MH, 0, u, v); out[i] = (double)truncnorm_variate(u, (float)a, b); }
    else out[i] = gamma_variate(key, (uint32_t)i, 0, P_ALPHA, a, err);
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------
static int sync_check(lsg_ctx* c, const char* who) {
    hipError_t e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = hipGetLastError();
    if (e != hipSuccess) { set_error("%s: kernel failed: %s", who, hipGetErrorString(e)); return -1; }
    return 0;
}

static SDev dev_of(const Bnpcs& b) {
    SDev d{};
    d.N = b.n_cells; d.M = b.n_muts; d.W = b.n_words; d.C = b.n_chains; d.steps1 = b.steps1; d.ll_pitch = b.ll_pitch; d.arena_rows = b.arena_rows;
    d.FN = b.cfg[0]; d.FP = b.cfg[1]; d.omFN = 1 - b.cfg[0]; d.omFP = 1 - b.cfg[1]; d.p = b.cfg[2]; d.q = b.cfg[3]; d.g0 = b.cfg[4]; d.g1 = b.cfg[5]; d.dpa_prob = b.cfg[6];
    d.uniform = d.p == 1.0 && d.q == 1.0;
    d.new1 = b.cfg[7]; d.new0 = b.cfg[8]; d.betaln = b.cfg[9];
    d.one = b.one.as<uint64_t>(); d.zero = b.zero.as<uint64_t>(); d.seeds = b.seeds.as<uint64_t>(); d.pop = b.pop.as<int32_t>();
    d.lab = b.lab.as<int32_t>(); d.size = b.size.as<int32_t>(); d.colof = b.colof.as<int32_t>(); d.live = b.live.as<int32_t>(); d.nlive = b.nlive.as<int32_t>();
    d.hi = b.hi.as<int32_t>(); d.order = b.order.as<int32_t>(); d.rec_lab = b.rec_lab.as<int32_t>(); d.err = b.err.as<int32_t>();
    d.theta = b.theta.as<float>(); d.arena = b.arena.as<float>();
    d.L1 = b.L1.as<double>(); d.L0 = b.L0.as<double>(); d.LL = b.LL.as<double>(); d.alpha = b.alpha.as<double>(); d.prow = b.prow.as<double>();
    d.rowml = b.rowml.as<double>(); d.rowb = b.rowb.as<double>(); d.rec_sc = b.rec_sc.as<double>();
    d.n1 = b.n1.as<uint32_t>(); d.n0 = b.n0.as<uint32_t>(); d.keys = b.keys.as<uint64_t>();
    return d;
}

static int need(lsg_ctx* c, const char* who) {
    if (!c) { set_error("%s: NULL handle", who); return -2; }
    if (hipSetDevice(c->device) != hipSuccess) { set_error("%s: hipSetDevice failed", who); return -1; }
    if (!c->bnpcs.valid) { set_error("%s: no sampler (lsg_bnpcs_create first)", who); return -2; }
    return 0;
}

// the live list and its count on the host
static int fetch_live(lsg_ctx* c, const char* who) {
    Bnpcs& b = c->bnpcs;
    hipLaunchKernelGGL(k_bnpcs_live, dim3(b.n_chains), dim3(256), 0, c->stream, dev_of(b));
    LSG_HIP(hipMemcpyAsync(b.h_k.data(), b.nlive.p, (size_t)b.n_chains * 4, hipMemcpyDeviceToHost, c->stream));
    if (sync_check(c, who)) return -1;
    b.k_max = *std::max_element(b.h_k.begin(), b.h_k.end());
    return 0;
}

static int launch_counts_tables(lsg_ctx* c) {
    Bnpcs& b = c->bnpcs;
    const size_t cells = (size_t)b.n_chains * b.n_cells * b.n_muts;
    LSG_HIP(hipMemsetAsync(b.n1.p, 0, cells * 4, c->stream));
    LSG_HIP(hipMemsetAsync(b.n0.p, 0, cells * 4, c->stream));
    const SDev d = dev_of(b);
    hipLaunchKernelGGL(k_bnpcs_counts, dim3((b.n_cells + 255) / 256, b.n_chains), dim3(256), 0, c->stream, d);
    hipLaunchKernelGGL(k_bnpcs_tables, dim3(b.n_cells, b.n_chains), dim3(64), 0, c->stream, d);
    return 0;
}

// after lsg_bnpcs_set_state: the sizes are the caller's labels'; the live list, the counts and the tables follow
static int prepare(lsg_ctx* c, const char* who) {
    Bnpcs& b = c->bnpcs;
    if (b.prepared) return 0;
    if (fetch_live(c, who)) return -1;
    if (int rc = launch_counts_tables(c)) return rc;
    b.prepared = true;
    return 0;
}

static int launch_sweep(lsg_ctx* c, uint32_t step) {
    Bnpcs& b = c->bnpcs;
    b.ll_pitch = std::max(b.k_max, 1);
    if (b.LL.reserve((size_t)b.n_chains * b.n_cells * b.ll_pitch * 8)) return -1;
    const SDev d = dev_of(b);
    hipLaunchKernelGGL(k_bnpcs_ll, dim3((b.ll_pitch + LT - 1) / LT, (b.n_cells + LT - 1) / LT, b.n_chains), dim3(256), 0, c->stream, d);
    hipLaunchKernelGGL(k_bnpcs_keys, dim3((b.n_cells + 255) / 256, b.n_chains), dim3(256), 0, c->stream, d, step);
    hipLaunchKernelGGL(k_bnpcs_perm, dim3((b.n_cells + 255) / 256, b.n_chains), dim3(256), 0, c->stream, d);
    hipLaunchKernelGGL(k_bnpcs_scan, dim3(b.n_chains), dim3(256), 0, c->stream, d, step);
    return 0;
}

static int launch_mh(lsg_ctx* c, uint32_t step) {
    Bnpcs& b = c->bnpcs;
    hipLaunchKernelGGL(k_bnpcs_mh, dim3((b.n_muts + 63) / 64, std::max(b.k_max, 1), b.n_chains), dim3(64), 0, c->stream, dev_of(b), step);
    return 0;
}

} // namespace lsg

using namespace lsg;

int lsg_bnpcs_create(lsg_ctx* c, int32_t n_cells, int32_t n_muts, int32_t n_chains, int32_t n_steps, const uint64_t* one, const uint64_t* zero, const double* cfg,
                     const uint64_t* seeds, int64_t arena_rows) {
    const char* who = "lsg_bnpcs_create";
    if (!c) { set_error("%s: NULL handle", who); return -2; }
    LSG_HIP(hipSetDevice(c->device));
    Bnpcs& b = c->bnpcs;
    b.valid = b.prepared = false;
    if (n_cells < 2 || n_cells > 65535) { set_error("%s: %d cells (2 .. 65535: the estimate keeps 16-bit labels)", who, n_cells); return -2; }
    if (n_muts < 1 || n_chains < 1 || n_steps < 1 || arena_rows < 1 || !one || !zero || !cfg || !seeds) { set_error("%s: bad arguments", who); return -2; }
    if (!(cfg[0] > 0 && cfg[0] < 1 && cfg[1] > 0 && cfg[1] < 1 && cfg[2] > 0 && cfg[3] > 0 && cfg[4] > 0)) { set_error("%s: error rates in (0, 1) and positive prior parameters are needed", who); return -2; }
    const size_t N = n_cells, M = n_muts, C = n_chains, W = (M + 63) / 64, S1 = (size_t)n_steps + 1;
    const double bytes = (double)C * N * M * (4 + 8 + 8 + 4 + 4) + (double)C * S1 * N * 4 + (double)C * arena_rows * M * 4;
    if (bytes > 64e9) { set_error("%s: %d chains x %d cells x %d mutations x %d steps need %.0f GB of state", who, n_chains, n_cells, n_muts, n_steps, bytes / 1e9); return -2; }
    if (b.one.reserve(N * W * 8) || b.zero.reserve(N * W * 8) || b.pop.reserve(N * 8) || b.seeds.reserve(C * 8) || b.lab.reserve(C * N * 4) || b.size.reserve(C * N * 4) ||
        b.colof.reserve(C * N * 4) || b.live.reserve(C * N * 4) || b.nlive.reserve(C * 4) || b.hi.reserve(C * 4) || b.theta.reserve(C * N * M * 4) || b.L1.reserve(C * N * M * 8) ||
        b.L0.reserve(C * N * M * 8) || b.alpha.reserve(C * 8) || b.prow.reserve(C * (N + 1) * 8) || b.n1.reserve(C * N * M * 4) || b.n0.reserve(C * N * M * 4) ||
        b.rowml.reserve(C * N * 8) || b.rowb.reserve(C * N * 8) || b.order.reserve(C * N * 4) || b.keys.reserve(C * N * 8) || b.rec_lab.reserve(C * S1 * N * 4) ||
        b.rec_sc.reserve(C * S1 * REC * 8) || b.arena.reserve(C * (size_t)arena_rows * M * 4) || b.err.reserve(C * 4 + 8 * C + 8)) return -1;
    std::vector<int32_t> pop(2 * N);
    const uint64_t tail = M % 64 ? ((1ull << (M % 64)) - 1) : ~0ull;
    for (size_t i = 0; i < N; ++i) {
        int p1 = 0, p0 = 0;
        for (size_t w = 0; w < W; ++w) {
            const uint64_t o = one[i * W + w], z = zero[i * W + w];
            if ((o & z) || (w == W - 1 && ((o | z) & ~tail))) { set_error("%s: cell %zu: a mutation is both 1 and 0, or a bit lies past the last mutation", who, i); return -2; }
            p1 += __builtin_popcountll(o); p0 += __builtin_popcountll(z);
        }
        pop[2 * i] = p1; pop[2 * i + 1] = p0;
    }
    hipStream_t st = c->stream;
    LSG_HIP(hipMemcpyAsync(b.one.p, one, N * W * 8, hipMemcpyHostToDevice, st));
    LSG_HIP(hipMemcpyAsync(b.zero.p, zero, N * W * 8, hipMemcpyHostToDevice, st));
    LSG_HIP(hipMemcpyAsync(b.pop.p, pop.data(), N * 8, hipMemcpyHostToDevice, st));
    LSG_HIP(hipMemcpyAsync(b.seeds.p, seeds, C * 8, hipMemcpyHostToDevice, st));
    LSG_HIP(hipMemsetAsync(b.lab.p, 0, C * N * 4, st));
    LSG_HIP(hipMemsetAsync(b.size.p, 0, C * N * 4, st));
    LSG_HIP(hipMemsetAsync(b.theta.p, 0, C * N * M * 4, st));
    LSG_HIP(hipMemsetAsync(b.alpha.p, 0, C * 8, st));
    LSG_HIP(hipMemsetAsync(b.err.p, 0, C * 4 + 8 * C, st));
    LSG_HIP(hipMemsetAsync(b.rec_lab.p, 0, C * S1 * N * 4, st));
    LSG_HIP(hipMemsetAsync(b.rec_sc.p, 0, C * S1 * REC * 8, st));
    LSG_HIP(hipStreamSynchronize(st));
    b.n_cells = n_cells; b.n_muts = n_muts; b.n_words = (int32_t)W; b.n_chains = n_chains; b.steps1 = (int32_t)S1; b.arena_rows = arena_rows;
    b.k_max = 0; b.ll_pitch = 1; b.pending = -1; b.next_step = 0;
    std::copy(cfg, cfg + 10, b.cfg);
    b.h_k.assign(C, 0); b.h_used.assign(C, 0);
    b.valid = true;
    return 0;
}

int lsg_bnpcs_set_state(lsg_ctx* c, int32_t chain, const int32_t* labels, const float* theta, double dp_alpha) {
    const char* who = "lsg_bnpcs_set_state";
    if (int rc = need(c, who)) return rc;
    Bnpcs& b = c->bnpcs;
    if (chain < 0 || chain >= b.n_chains || !labels || !theta || !(dp_alpha > 0)) { set_error("%s: bad arguments", who); return -2; }
    const size_t N = b.n_cells, M = b.n_muts;
    std::vector<int32_t> size(N, 0);
    for (size_t i = 0; i < N; ++i) {
        if (labels[i] < 0 || labels[i] >= b.n_cells) { set_error("%s: labels[%zu] = %d is not in [0, %d)", who, i, labels[i], b.n_cells); return -2; }
        ++size[labels[i]];
    }
    for (size_t k = 0; k < N; ++k)
        if (size[k])
            for (size_t m = 0; m < M; ++m) {
                const float t = theta[k * M + m];
                if (!(t > 0.0f && t < 1.0f)) { set_error("%s: theta[%zu][%zu] = %g of a live cluster is not inside (0, 1)", who, k, m, (double)t); return -2; }
            }
    hipStream_t st = c->stream;
    LSG_HIP(hipMemcpyAsync(b.lab.as<int32_t>() + chain * N, labels, N * 4, hipMemcpyHostToDevice, st));
    LSG_HIP(hipMemcpyAsync(b.size.as<int32_t>() + chain * N, size.data(), N * 4, hipMemcpyHostToDevice, st));
    LSG_HIP(hipMemcpyAsync(b.theta.as<float>() + chain * N * M, theta, N * M * 4, hipMemcpyHostToDevice, st));
    LSG_HIP(hipMemcpyAsync(b.alpha.as<double>() + chain, &dp_alpha, 8, hipMemcpyHostToDevice, st));
    LSG_HIP(hipStreamSynchronize(st));
    b.prepared = false;
    return 0;
}

int lsg_bnpcs_get_state(lsg_ctx* c, int32_t chain, int32_t* labels, float* theta, double* dp_alpha) {
    const char* who = "lsg_bnpcs_get_state";
    if (int rc = need(c, who)) return rc;
    Bnpcs& b = c->bnpcs;
    if (chain < 0 || chain >= b.n_chains || !labels || !theta || !dp_alpha) { set_error("%s: bad arguments", who); return -2; }
    const size_t N = b.n_cells, M = b.n_muts;
    hipStream_t st = c->stream;
    LSG_HIP(hipMemcpyAsync(labels, b.lab.as<int32_t>() + chain * N, N * 4, hipMemcpyDeviceToHost, st));
    LSG_HIP(hipMemcpyAsync(theta, b.theta.as<float>() + chain * N * M, N * M * 4, hipMemcpyDeviceToHost, st));
    LSG_HIP(hipMemcpyAsync(dp_alpha, b.alpha.as<double>() + chain, 8, hipMemcpyDeviceToHost, st));
    return sync_check(c, who);
}

int lsg_bnpcs_run(lsg_ctx* c, int32_t first_step, int32_t n_steps, int32_t burn_in, int32_t* done) {
    const char* who = "lsg_bnpcs_run";
    if (int rc = need(c, who)) return rc;
    Bnpcs& b = c->bnpcs;
    if (!done || n_steps < 0 || burn_in < 0) { set_error("%s: bad arguments", who); return -2; }
    *done = 0;
    if (first_step != b.next_step || first_step + n_steps > b.steps1) {
        set_error("%s: steps %d .. %d asked, the next step is %d of %d", who, first_step, first_step + n_steps - 1, b.next_step, b.steps1 - 1);
        return -2;
    }
    if (int rc = prepare(c, who)) return rc;
    int64_t* d_used = reinterpret_cast<int64_t*>(b.err.as<int32_t>() + b.n_chains + (b.n_chains & 1));
    for (int32_t s = first_step; s < first_step + n_steps; ++s) {
        if (s > 0 && b.pending != s) {
            if (int rc = launch_sweep(c, (uint32_t)s)) return rc;
            if (fetch_live(c, who)) return -1;
            if (int rc = launch_counts_tables(c)) return rc;
            if (int rc = launch_mh(c, (uint32_t)s)) return rc;
            hipLaunchKernelGGL(k_bnpcs_tables, dim3(b.n_cells, b.n_chains), dim3(64), 0, c->stream, dev_of(b));
        }
        b.pending = s;
        const bool keep = s >= burn_in;
        if (keep)
            for (int32_t k = 0; k < b.n_chains; ++k)
                if (b.h_used[k] + b.h_k[k] > b.arena_rows) {
                    if (b.h_used[k] == 0) { set_error("%s: step %d has %d clusters, the arena holds %lld rows", who, s, b.h_k[k], (long long)b.arena_rows); return -2; }
                    return sync_check(c, who);                    // full: the caller fetches and goes on at this step
                }
        LSG_HIP(hipMemcpyAsync(d_used, b.h_used.data(), (size_t)b.n_chains * 8, hipMemcpyHostToDevice, c->stream));
        hipLaunchKernelGGL(k_bnpcs_record, dim3(b.n_chains), dim3(256), 0, c->stream, dev_of(b), s, keep ? 1 : 0, d_used);
        if (sync_check(c, who)) return -1;                        // (h_used is read by the copy until here)
        if (keep) for (int32_t k = 0; k < b.n_chains; ++k) b.h_used[k] += b.h_k[k];
        b.pending = -1; b.next_step = s + 1; ++*done;
    }
    return 0;
}

int lsg_bnpcs_fetch(lsg_ctx* c, int32_t* labels, double* scalars, float* arena, int64_t* arena_used, int32_t* errors) {
    const char* who = "lsg_bnpcs_fetch";
    if (int rc = need(c, who)) return rc;
    Bnpcs& b = c->bnpcs;
    if (!labels || !scalars || !arena || !arena_used || !errors) { set_error("%s: bad arguments", who); return -2; }
    const size_t N = b.n_cells, M = b.n_muts, C = b.n_chains, S1 = b.steps1;
    hipStream_t st = c->stream;
    LSG_HIP(hipMemcpyAsync(labels, b.rec_lab.p, C * S1 * N * 4, hipMemcpyDeviceToHost, st));
    LSG_HIP(hipMemcpyAsync(scalars, b.rec_sc.p, C * S1 * REC * 8, hipMemcpyDeviceToHost, st));
    for (size_t k = 0; k < C; ++k)
        if (b.h_used[k])
            LSG_HIP(hipMemcpyAsync(arena + k * (size_t)b.arena_rows * M, b.arena.as<float>() + k * (size_t)b.arena_rows * M, (size_t)b.h_used[k] * M * 4, hipMemcpyDeviceToHost, st));
    LSG_HIP(hipMemcpyAsync(errors, b.err.p, C * 4, hipMemcpyDeviceToHost, st));
    if (sync_check(c, who)) return -1;
    for (size_t k = 0; k < C; ++k) { arena_used[k] = b.h_used[k]; b.h_used[k] = 0; }
    return 0;
}

int lsg_bnpcs_destroy(lsg_ctx* c) {
    if (!c) { set_error("lsg_bnpcs_destroy: NULL handle"); return -2; }
    LSG_HIP(hipSetDevice(c->device));
    c->bnpcs.release();
    return 0;
}

// ---- test support (include/longsom_synth.h) ----------------------------------------------------------------------------------------------
int lsg_bnpcs_test_stream(lsg_ctx* c, uint64_t key, int64_t n, const uint32_t* counters, uint32_t* words, double* dbl) {
    const char* who = "lsg_bnpcs_test_stream";
    if (!c || n < 1 || !counters || !words || !dbl) { set_error("%s: bad arguments", who); return -2; }
    LSG_HIP(hipSetDevice(c->device));
    DevBuf in, w, d;
    int rc = -1;
    if (!in.reserve((size_t)n * 16) && !w.reserve((size_t)n * 16) && !d.reserve((size_t)n * 16) &&
        hipMemcpyAsync(in.p, counters, (size_t)n * 16, hipMemcpyHostToDevice, c->stream) == hipSuccess) {
        hipLaunchKernelGGL(k_bnpcs_test_stream, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, key, n, in.as<uint32_t>(), w.as<uint32_t>(), d.as<double>());
        if (hipMemcpyAsync(words, w.p, (size_t)n * 16, hipMemcpyDeviceToHost, c->stream) == hipSuccess &&
            hipMemcpyAsync(dbl, d.p, (size_t)n * 16, hipMemcpyDeviceToHost, c->stream) == hipSuccess) rc = sync_check(c, who);
    }
    in.release(); w.release(); d.release();
    return rc;
}

int lsg_bnpcs_test_variates(lsg_ctx* c, uint64_t key, int32_t kind, int64_t n, double a, double b, double* out, int32_t* errors) {
    const char* who = "lsg_bnpcs_test_variates";
    if (!c || n < 1 || kind < 0 || kind > 2 || !out || !errors) { set_error("%s: bad arguments", who); return -2; }
    LSG_HIP(hipSetDevice(c->device));
    DevBuf o;
    int rc = -1;
    if (!o.reserve((size_t)n * 8 + 8) && hipMemsetAsync(o.p, 0, (size_t)n * 8 + 8, c->stream) == hipSuccess) {
        int32_t* d_err = reinterpret_cast<int32_t*>(o.as<double>() + n);
        hipLaunchKernelGGL(k_bnpcs_test_variates, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, key, kind, n, a, b, o.as<double>(), d_err);
        if (hipMemcpyAsync(out, o.p, (size_t)n * 8, hipMemcpyDeviceToHost, c->stream) == hipSuccess &&
            hipMemcpyAsync(errors, d_err, 4, hipMemcpyDeviceToHost, c->stream) == hipSuccess) rc = sync_check(c, who);
    }
    o.release();
    return rc;
}

int lsg_bnpcs_test_counts(lsg_ctx* c, int32_t chain, uint32_t* n1, uint32_t* n0) {
    const char* who = "lsg_bnpcs_test_counts";
    if (int rc = need(c, who)) return rc;
    Bnpcs& b = c->bnpcs;
    if (chain < 0 || chain >= b.n_chains || !n1 || !n0) { set_error("%s: bad arguments", who); return -2; }
    if (int rc = prepare(c, who)) return rc;
    const size_t NM = (size_t)b.n_cells * b.n_muts;
    LSG_HIP(hipMemcpyAsync(n1, b.n1.as<uint32_t>() + chain * NM, NM * 4, hipMemcpyDeviceToHost, c->stream));
    LSG_HIP(hipMemcpyAsync(n0, b.n0.as<uint32_t>() + chain * NM, NM * 4, hipMemcpyDeviceToHost, c->stream));
    return sync_check(c, who);
}

int lsg_bnpcs_test_ll(lsg_ctx* c, int32_t chain, double* ll, int32_t* clusters, int32_t* n_clusters) {
    const char* who = "lsg_bnpcs_test_ll";
    if (int rc = need(c, who)) return rc;
    Bnpcs& b = c->bnpcs;
    if (chain < 0 || chain >= b.n_chains || !ll || !clusters || !n_clusters) { set_error("%s: bad arguments", who); return -2; }
    if (int rc = prepare(c, who)) return rc;
    b.ll_pitch = std::max(b.k_max, 1);
    if (b.LL.reserve((size_t)b.n_chains * b.n_cells * b.ll_pitch * 8)) return -1;
    hipLaunchKernelGGL(k_bnpcs_ll, dim3((b.ll_pitch + LT - 1) / LT, (b.n_cells + LT - 1) / LT, b.n_chains), dim3(256), 0, c->stream, dev_of(b));
    const int32_t K = b.h_k[chain];
    const size_t N = b.n_cells;
    LSG_HIP(hipMemcpy2DAsync(ll, (size_t)K * 8, b.LL.as<double>() + chain * N * b.ll_pitch, (size_t)b.ll_pitch * 8, (size_t)K * 8, N, hipMemcpyDeviceToHost, c->stream));
    LSG_HIP(hipMemcpyAsync(clusters, b.live.as<int32_t>() + chain * N, (size_t)K * 4, hipMemcpyDeviceToHost, c->stream));
    *n_clusters = K;
    return sync_check(c, who);
}

int lsg_bnpcs_test_move(lsg_ctx* c, int32_t what, int32_t step) {
    const char* who = "lsg_bnpcs_test_move";
    if (int rc = need(c, who)) return rc;
    Bnpcs& b = c->bnpcs;
    if (what < 0 || what > 1 || step < 0) { set_error("%s: bad arguments", who); return -2; }
    if (int rc = prepare(c, who)) return rc;
    if (what == 0) {
        if (int rc = launch_sweep(c, (uint32_t)step)) return rc;
        if (fetch_live(c, who)) return -1;
        if (int rc = launch_counts_tables(c)) return rc;
    } else {
        if (int rc = launch_mh(c, (uint32_t)step)) return rc;
        hipLaunchKernelGGL(k_bnpcs_tables, dim3(b.n_cells, b.n_chains), dim3(64), 0, c->stream, dev_of(b));
    }
    return sync_check(c, who);
}
