// BnpC's sampler (CellClustering/libs/CRP.py:17-820, libs/CRP_learning_errors.py, libs/MCMC.py:200-388): Gibbs assignment sweeps, the
// non-conjugate split-merge move, the Escobar-West concentration update, the parameter Metropolis-Hastings and the Metropolis-Hastings
// updates of the error rates, every chain of a run in every kernel.  A chain has error rates of its own (Rates): with the updates off
// they are the run's for every chain, with them on they move between steps.  A run with a fixed assignment makes only the parameter move
// and the error update.  The stream, the variates and the order of a step are defined in longsom_amd/bnpc_sampler.py's docstring; its numpy
// twin is what these kernels are held to.  See include/longsom_hip.h, lsg_bnpcs_*.  Everything is fp64 except theta.
#include "lsg_ctx.h"
#include "philox.h"
#include <algorithm>
#include <cmath>

namespace lsg {

constexpr double S_TMIN = 1e-5, S_TMAX = 1 - 1e-5;
constexpr double S_EPS = 1e-15;                       // np.finfo(np.float64).resolution
constexpr int S_TRIES = 64;                           // Marsaglia-Tsang tries before the mean is written and an error counted
enum { P_PERM = 1, P_CHOICE, P_BIRTH, P_BIRTH_B, P_DPA, P_ETA, P_ETA_B, P_ALPHA, P_MH, P_INIT_LABEL, P_INIT_THETA,
       P_SM, P_SM_PERM, P_SM_CHOICE, P_SM_BETA, P_SM_BETA_B, P_SM_MH, P_SM_SD, P_ERR, P_ERR_FP, P_ERR_FN, P_INIT_ASSIGN, P_INIT_ASSIGN_B };
constexpr int ERR_OUT = 21;                           // doubles of an error update's outcome: whether it was made, then ten per rate (lsg_bnpcs_test_error_outcome)
constexpr int SM_OUT = 12;                            // doubles of a move's outcome: code, the clusters, the anchors, A, its four terms, ln v, |S|
constexpr int SM_MAX_SCANS = 1 << 20;                 // 4 scan + row must fit the 24 bits of `sub`
constexpr int LT = 16;                                // k_bnpcs_ll: cells x columns per workgroup
constexpr int REC = 5;                                // doubles recorded per chain and step: ML, the CRP prior sum, the beta prior sum, live clusters, alpha

// what every kernel reads: the shape, the constants and where the state lies.  Per chain c: lab, size, colof, live, prow at c * N (prow:
// c * (N + 1)); theta, L1, L0, n1, n0 at c * N * M; LL at c * N * ll_pitch.
// a chain's error rates and what follows from them: the new cluster's two log terms (get_lpost_single_new_cluster, CRP.py:230-234) and the
// six logs of _rg_init_split's likelihood, [anchor 1, 0, missing][cell 1, 0]
struct Rates {
    double FP, FN, omFP, omFN, new1, new0, sm_anchor[6];
};

// the four numbers log_terms reads: enough for a likelihood under trial rates (err_ll)
__host__ __device__ inline void rates_set(Rates& r, double FP, double FN) { r.FP = FP; r.FN = FN; r.omFP = 1 - FP; r.omFN = 1 - FN; }

__host__ __device__ inline void rates_fill(Rates& r, double FP, double FN, double mix0, double mix1) {
    rates_set(r, FP, FN);
    r.new1 = log(mix1 * (1 - FN) + mix0 * FP); r.new0 = log(mix1 * FN + mix0 * (1 - FP));
    const double v[6] = {1 - FN, FN, FP, 1 - FP, mix0 * (1 - FN) + (1 - mix0) * FP, mix0 * FN + (1 - mix0) * (1 - FP)};
    for (int k = 0; k < 6; ++k) r.sm_anchor[k] = log(v[k]);
}

struct SDev {
    int32_t N, M, W, C, steps1, ll_pitch;
    int64_t arena_rows;
    double p, q, g0, g1, dpa_prob, betaln, mix0, mix1;
    // the error-rate update: a step makes it with probability err_prob; the priors' (mean, sd) of FP and of FN.  rates [chain]; rec_err
    // [chain][steps1][2]: FP, FN per step; err_cnt [chain][4]: FP accepted, declined, FN accepted, declined; err_out [chain][ERR_OUT]
    double err_prob, err_mean[2], err_sd[2];
    Rates* rates;
    double *rec_err, *err_out;
    int32_t* err_cnt;
    int32_t uniform;
    const uint64_t *one, *zero, *seeds;
    const int32_t* pop;                               // [N][2]: ones, zeros
    int32_t *lab, *size, *colof, *live, *nlive, *hi, *order, *rec_lab, *err;
    float *theta, *arena;
    double *L1, *L0, *LL, *alpha, *prow, *rowml, *rowb, *rec_sc;
    uint32_t *n1, *n0;
    uint64_t* keys;
    // the split-merge move: a step takes it with probability sm_prob, a split with sm_edge = r0 / (r0 + r1).  Per chain: sm_i 5 N (the cells of cluster i, of cluster j, S, the
    // assignment of S, the walk's picks), sm_d sm_d_size(N, M) doubles (ll [N][2], u [N], the same in walk order, the rows' L1 / L0, the outcome),
    // sm_c 6 M (the rows' n1 / n0), sm_t 3 M (the rows), rec_sm steps1 (the codes of sm_moves)
    double sm_prob, sm_edge;
    int32_t sm_scans;
    int32_t *sm_i, *rec_sm;
    double* sm_d;
    uint32_t* sm_c;
    float* sm_t;
};

// ---- the stream ----------------------------------------------------------------------------------------------------------------
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

// the density truncated to [lo, hi]: (float)S_TMIN, (float)S_TMAX as the proposals are, but _rg_get_split_prob passes (0 - theta) / sd and
// (1 - theta) / sd (CRP.py:779-780).  The differences are formed in float32, as the twin forms them
__device__ inline double truncnorm_logpdf(float x, float loc, double sd, float lo, float hi) {
    const double pa = normcdf(f32diff(lo, loc) / sd), pb = normcdf(f32diff(hi, loc) / sd);
    const double z = (double)(x - loc) / sd;
    return -0.5 * z * z - 0.5 * log(2.0 * M_PI) - log(sd) - log(pb - pa);
}

// under the rates of the chain (a kernel copies its chain's row of SDev::rates once)
__device__ inline void log_terms(const Rates& r, float theta, double& l1, double& l0) {
    const double th = (double)theta, om = (double)(1.0f - theta);
    l1 = log(th * r.omFN + om * r.FP);
    l0 = log(th * r.FN + om * r.omFP);
}

__device__ inline double beta_logpdf(const SDev& d, float theta) {
    const double x = (double)theta;
    return (d.q - 1.0) * log1p(-x) + (d.p - 1.0) * log(x) - d.betaln;
}

// ---- reductions over a workgroup of 256 (four waves): every lane gets the result; sh holds 4 -------------------------------------
// The order is fixed: the butterfly within a wave, then (wave 0 . wave 1) . (wave 2 . wave 3)
template <class T, class Op> __device__ inline T block_reduce(T v, T* sh, Op op) {
    for (int o = 32; o > 0; o >>= 1) v = op(v, __shfl_xor(v, o, 64));
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    v = op(op(sh[0], sh[1]), op(sh[2], sh[3]));
    __syncthreads();
    return v;
}

__device__ inline double block_max(double v, double* sh) { return block_reduce(v, sh, [](double a, double b) { return fmax(a, b); }); }
__device__ inline double block_sum(double v, double* sh) { return block_reduce(v, sh, [](double a, double b) { return a + b; }); }
__device__ inline int block_min_int(int v, int* sh) { return block_reduce(v, sh, [](int a, int b) { return min(a, b); }); }

// a lane's run of the ids 0 .. n-1 in a workgroup of 256: k0 .. k1-1, the lanes' runs adjacent and ascending.  Every running sum and every
// compaction here relies on that: going through the lanes in their order goes through the ids in theirs.
struct Run { int k0, k1; };
__device__ inline Run lane_run(int n) {
    const int ch = (n + 255) / 256, k0 = min((int)threadIdx.x * ch, n);
    return {k0, min(k0 + ch, n)};
}

// the smallest id below `bound` whose cluster is empty (get_empty_cluster), `bound` if there is none; every lane gets it
__device__ inline int first_free(const int32_t* size, int bound, int* shi) {
    const auto [k0, k1] = lane_run(bound);
    int fr = bound;
    for (int k = k0; k < k1; ++k) if (size[k] == 0) { fr = k; break; }
    return block_min_int(fr, shi);
}

// a masked sum over the mutations: a cell against one row of tables (a cluster's own, or a row of the split-merge move)
__device__ inline double masked_ll(const SDev& d, int cell, const double* l1, const double* l0) {
    double acc = 0.0;
    for (int w = 0; w < d.W; ++w) {
        uint64_t o = d.one[(size_t)cell * d.W + w], z = d.zero[(size_t)cell * d.W + w];
        while (o) { acc += l1[w * 64 + __ffsll((unsigned long long)o) - 1]; o &= o - 1; }
        while (z) { acc += l0[w * 64 + __ffsll((unsigned long long)z) - 1]; z &= z - 1; }
    }
    return acc;
}

// a cell's ones and zeros counted into a row of n1 / n0: integer atomics, exact in any order
__device__ inline void count_cell(const SDev& d, int cell, uint32_t* n1, uint32_t* n0) {
    for (int w = 0; w < d.W; ++w) {
        uint64_t o = d.one[(size_t)cell * d.W + w], z = d.zero[(size_t)cell * d.W + w];
        while (o) { atomicAdd(&n1[w * 64 + __ffsll((unsigned long long)o) - 1], 1u); o &= o - 1; }
        while (z) { atomicAdd(&n0[w * 64 + __ffsll((unsigned long long)z) - 1], 1u); z &= z - 1; }
    }
}

// which of its three sds a proposal takes: word 0 of the block at `attempt`, modulo 3
__device__ inline uint32_t sd_pick(uint64_t key, uint32_t index, uint32_t step, uint32_t purpose, uint32_t attempt) {
    uint32_t w[4];
    philox4x32(key, index, step, purpose, attempt, w);
    return w[0] % 3u;
}

__device__ const double PROPOSAL_SD[3] = {0.1, 0.25, 0.5};     // param_proposal_sd (CRP.py:65): the parameter proposals' three, by sd_pick

// _get_log_A (:347-383) of one entry, not clipped; unit: the forward density's bounds are 0 and 1 (_rg_get_split_prob)
__device__ inline double log_A(const SDev& d, const Rates& er, float nw, float old, double n1, double n0, double sd, bool unit) {
    double nl1, nl0, ol1, ol0;
    log_terms(er, nw, nl1, nl0);
    log_terms(er, old, ol1, ol0);
    const double new_ll = n1 * nl1 + n0 * nl0, old_ll = n1 * ol1 + n0 * ol0;
    const double new_prior = d.uniform ? 0.0 : beta_logpdf(d, nw), old_prior = d.uniform ? 0.0 : beta_logpdf(d, old);
    const float lo = (float)S_TMIN, hi = (float)S_TMAX;
    const double new_p = unit ? truncnorm_logpdf(nw, old, sd, 0.0f, 1.0f) : truncnorm_logpdf(nw, old, sd, lo, hi), old_p = truncnorm_logpdf(old, nw, sd, lo, hi);
    return new_ll + new_prior - old_ll - old_prior + old_p - new_p;
}

// ---- counts: n1 / n0 [chain][cluster][mutation] from the masks and the labels (zeroed before).  A lane per cell. ------------------------
__global__ __launch_bounds__(256) void k_bnpcs_counts(SDev d) {
    const int c = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= d.N) return;
    const size_t row = ((size_t)c * d.N + d.lab[(size_t)c * d.N + i]) * d.M;
    count_cell(d, i, d.n1 + row, d.n0 + row);
}

// ---- tables: L1 / L0 of every live cluster, and per cluster the likelihood sum_m n1 L1 + n0 L0 and the beta prior's log density of its
// parameters.  A wave per (cluster, chain). -----------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_bnpcs_tables(SDev d) {
    const int c = blockIdx.y, k = blockIdx.x;
    const size_t row = (size_t)c * d.N + k;
    const Rates er = d.rates[c];
    double ml = 0.0, bp = 0.0;
    if (d.size[row] > 0)
        for (int m = threadIdx.x; m < d.M; m += 64) {
            const float th = d.theta[row * d.M + m];
            double l1, l0;
            log_terms(er, th, l1, l0);
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
    const auto [k0, k1] = lane_run(d.N);
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

// the rank of keys[i] among keys[0 .. n-1], by counting; every lane of the workgroup calls it (one with i >= n for the others' sake).  tile: 256 words of LDS
__device__ inline int block_rank(const uint64_t* keys, int n, int i, uint64_t* tile) {
    const uint64_t mine = i < n ? keys[i] : 0;
    int rank = 0;
    for (int j0 = 0; j0 < n; j0 += 256) {
        __syncthreads();
        tile[threadIdx.x] = j0 + (int)threadIdx.x < n ? keys[j0 + threadIdx.x] : ~0ull;
        __syncthreads();
        const int cnt = min(256, n - j0);
        for (int j = 0; j < cnt; ++j) rank += (tile[j] < mine) || (tile[j] == mine && j0 + j < i);
    }
    return rank;
}

__global__ __launch_bounds__(256) void k_bnpcs_perm(SDev d) {
    __shared__ uint64_t tile[256];
    const int c = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    const int rank = block_rank(d.keys + (size_t)c * d.N, d.N, i, tile);
    if (i < d.N) d.order[(size_t)c * d.N + rank] = i;
}

// ---- the concentration update (update_DP_alpha, :386-410) that follows a chain's sweep or its split-merge move: the whole workgroup calls it
// once the chain's sizes are final
__device__ void alpha_update(const SDev& d, int c, uint32_t step, const int32_t* size, double alpha, double* shd) {
    const int t = threadIdx.x, N = d.N;
    const uint64_t key = d.seeds[c];
    const auto [k0, k1] = lane_run(N);
    double kk = 0.0;
    for (int k = k0; k < k1; ++k) kk += size[k] > 0;
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

// ---- the sweep: one workgroup per chain walks the permuted cells (update_assignments_Gibbs, CRP.py:254-288), then the concentration
// update (update_DP_alpha, :386-410).  No workgroup waits for another.  A lane owns a run of cluster ids (lane_run), so the running sum of the
// probabilities keeps the ids' order.  A cluster alive at the sweep's start reads its column of LL; one born in the sweep, or an id that
// emptied and was issued again, has colof = -1 and is evaluated from its own tables (the stale-column rule).  With `decide` a chain whose
// step is a split-merge move (Chain.do_step, MCMC.py:322) leaves here at once: k_bnpcs_sm moves it and makes its concentration update.
__global__ __launch_bounds__(256) void k_bnpcs_scan(SDev d, uint32_t step, int decide) {
    __shared__ double shd[4];
    __shared__ int shi[4];
    __shared__ double pref[4];
    __shared__ int s_pick;
    const int c = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6, N = d.N;
    const uint64_t key = d.seeds[c];
    if (decide) {
        double u0, u1;
        doubles(key, 0, step, P_SM, 0, u0, u1);
        if (u0 < d.sm_prob) return;
    }
    int32_t* lab = d.lab + (size_t)c * N; int32_t* size = d.size + (size_t)c * N; int32_t* colof = d.colof + (size_t)c * N;
    const int32_t* order = d.order + (size_t)c * N;
    double* prow = d.prow + (size_t)c * (N + 1);
    const double alpha = d.alpha[c], lden = log((double)(N - 1) + alpha), lnew = log(alpha) - lden, log_eps = log(S_EPS);
    const Rates er = d.rates[c];
    int hi = d.hi[c];
    for (int n = 0; n < N; ++n) {
        const int cell = order[n];
        const int old = lab[cell];
        __syncthreads();
        if (t == 0) { const int sz = size[old] - 1; size[old] = sz; if (sz == 0) colof[old] = -1; s_pick = hi; }
        __syncthreads();
        // slots 0 .. hi-1 are cluster ids, slot hi is the new cluster
        const auto [k0, k1] = lane_run(hi + 1);
        double mx = -INFINITY;
        for (int k = k0; k < k1; ++k) {
            double lp = -INFINITY;
            if (k == hi) lp = ((double)d.pop[2 * cell] * er.new1 + (double)d.pop[2 * cell + 1] * er.new0) + lnew;
            else {
                const int sz = size[k];
                if (sz > 0) {
                    const int col = colof[k];
                    const size_t own = ((size_t)c * N + k) * d.M;
                    const double ll = col >= 0 ? d.LL[((size_t)c * N + cell) * d.ll_pitch + col] : masked_ll(d, cell, d.L1 + own, d.L0 + own);
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
            const int slot = first_free(size, hi, shi);
            const size_t row = (size_t)c * N + slot;
            for (int m = t; m < d.M; m += 256) {
                const int w = m >> 6, b = m & 63;
                const double a1 = d.p + (double)((d.one[(size_t)cell * d.W + w] >> b) & 1), b1 = d.q + (double)((d.zero[(size_t)cell * d.W + w] >> b) & 1);
                const double x = beta_variate(key, (uint32_t)m, step, (uint32_t)P_BIRTH | ((uint32_t)cell << 8), a1, b1, d.err + c);
                const float th = (float)fmin(fmax(x, S_TMIN), S_TMAX);
                double l1, l0;
                log_terms(er, th, l1, l0);
                d.theta[row * d.M + m] = th; d.L1[row * d.M + m] = l1; d.L0[row * d.M + m] = l0;
            }
            if (t == 0) { size[slot] = 1; colof[slot] = -1; lab[cell] = slot; }
            hi = max(hi, slot + 1);
        } else if (t == 0) { size[pick] += 1; lab[cell] = pick; }
    }
    __syncthreads();
    alpha_update(d, c, step, size, alpha, shd);
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
    const double sd = PROPOSAL_SD[sd_pick(key, (uint32_t)m, step, pw, 1)];
    const float old = d.theta[at];
    const float nw = truncnorm_variate(u, old, sd);
    const Rates er = d.rates[c];
    if (log(v) < log_A(d, er, nw, old, (double)d.n1[at], (double)d.n0[at], sd, false)) d.theta[at] = nw;
}

// ---- the split-merge move (update_assignments_split_merge and what it calls, CRP.py:417-820; the stream and the order of the draws are in
// longsom_amd/bnpc_sampler.py's docstring).  One workgroup per chain, as the sweep: no workgroup waits for another and every loop is bounded.
// The lanes share the compaction of the move's cells, the launch assignment, the rows' counts, Beta draws and tables, the parameter moves,
// the cells' likelihoods and every sum of the acceptance ratio (block_sum: a fixed order); only the assignment walk is serial, over
// records laid out in walk order.  The rows' tables stay in global memory: they are read once per scan, the dense part does not bound a step.
struct SmBuf {
    int32_t *A, *B, *S, *asg, *pick;
    double *ll, *u, *wll, *wu, *L1, *L0, *out;
    uint32_t *n1, *n0;
    float* th;
};

// a chain's doubles of sm_d, and where the outcome (SmBuf::out) lies among them: behind ll, u, wll, wu (6 N) and the rows' L1, L0 (6 M)
__host__ __device__ inline size_t sm_d_out(size_t N, size_t M) { return 6 * N + 6 * M; }
__host__ __device__ inline size_t sm_d_size(size_t N, size_t M) { return sm_d_out(N, M) + SM_OUT; }

__device__ inline SmBuf sm_buf(const SDev& d, int c) {
    const size_t N = d.N, M = d.M;
    SmBuf b;
    int32_t* pi = d.sm_i + (size_t)c * 5 * N;
    b.A = pi; b.B = pi + N; b.S = pi + 2 * N; b.asg = pi + 3 * N; b.pick = pi + 4 * N;
    double* pd = d.sm_d + (size_t)c * sm_d_size(N, M);
    b.ll = pd; b.u = pd + 2 * N; b.wll = pd + 3 * N; b.wu = pd + 5 * N; b.L1 = pd + 6 * N; b.L0 = b.L1 + 3 * M; b.out = pd + sm_d_out(N, M);
    b.n1 = d.sm_c + (size_t)c * 6 * M; b.n0 = b.n1 + 3 * M;
    b.th = d.sm_t + (size_t)c * 3 * M;
    return b;
}

// a move as its phases see it: the chain, then what sm_choose decides.  Every lane holds the same values
struct Sm {
    int c, K;
    uint32_t step;
    uint64_t key;
    double alpha;
    Rates er;
    SmBuf b;
    int32_t *lab, *size;
    const int32_t* live;
    bool split;
    int cli, clj;                                     // the clusters; a split's clj is the smallest free id, which the new cluster takes if the move is accepted
    int ai, aj, nS;                                   // the anchors; |S|: the clusters' cells without the anchors
    float *th_i, *th_j;                               // the clusters' parameters in the chain's state
    double size_data;                                 // ltrans_prob_size (:454-456) of a split, cluster_size_data (:505-507) of a merge
};

// the kernel's LDS: what the reductions, the compactions and the rank count need, and what lane 0 hands to the others
struct SmLds {
    double shd[4], val[2];
    uint64_t tile[256];
    int shi[4], cnt[256], pick[5];
};

// the cells labelled a or b, without the cells xi and xj, in ascending id into out; every lane gets their number.  cnt: 256 ints of LDS
__device__ int sm_compact(const int32_t* lab, int N, int a, int b, int xi, int xj, int32_t* out, int* cnt) {
    const int t = threadIdx.x;
    const auto [k0, k1] = lane_run(N);
    int n = 0;
    for (int k = k0; k < k1; ++k) { const int l = lab[k]; n += (l == a || l == b) && k != xi && k != xj; }
    __syncthreads();
    cnt[t] = n;
    __syncthreads();
    int at = 0, total = 0;
    for (int j = 0; j < 256; ++j) { const int v = cnt[j]; total += v; if (j < t) at += v; }
    for (int k = k0; k < k1; ++k) { const int l = lab[k]; if ((l == a || l == b) && k != xi && k != xj) out[at++] = k; }
    __syncthreads();
    return total;
}

// do_split_move (:434-462) / do_merge_move (:480-510) up to run_rg_nc: the kind of move, the clusters, the anchors and S
__device__ inline void sm_choose(const SDev& d, Sm& m, double u_kind, SmLds& L) {
    const int t = threadIdx.x, N = d.N, K = m.K;
    const int32_t* size = m.size; const int32_t* live = m.live;
    const int free_id = first_free(size, N, L.shi);                // N if there is none: then every cluster has one cell and the move is a merge
    if (t == 0) {
        double c0, c1;
        doubles(m.key, 0, m.step, P_SM, 1, c0, c1);
        const bool split = K == 1 ? true : K == N ? false : u_kind < d.sm_edge;
        int cli = -1, clj = -1;
        double size_data;
        if (split) {
            // once from the clusters of two cells or more: the re-draw loop's own distribution (:441-445)
            long long tot = 0, cum = 0;
            for (int j = 0; j < K; ++j) { const int sz = size[live[j]]; if (sz >= 2) tot += sz; }
            for (int j = 0; j < K; ++j) { const int sz = size[live[j]]; if (sz >= 2) { cum += sz; cli = live[j]; if ((double)cum / (double)tot > c0) break; } }
            const double sz = (double)size[cli];
            size_data = log(sz / (double)N) - log(sz) - log(sz - 1.0);                   // the unrestricted share (:454-456)
        } else {
            double tot = 0.0, cum = 0.0;
            for (int j = 0; j < K; ++j) tot += 1.0 / (double)size[live[j]];
            int ji = 0, jj = 0;
            for (int j = 0; j < K; ++j) { cum += 1.0 / (double)size[live[j]]; ji = j; if (cum / tot > c0) break; }
            double tot2 = 0.0;
            for (int j = 0; j < K; ++j) if (j != ji) tot2 += 1.0 / (double)size[live[j]];
            cum = 0.0;
            for (int j = 0; j < K; ++j) if (j != ji) { cum += 1.0 / (double)size[live[j]]; jj = j; if (cum / tot2 > c1) break; }
            cli = live[ji]; clj = live[jj];
            const double si = (double)size[cli], sj = (double)size[clj];
            size_data = (log(1.0 / si / tot) + log(1.0 / sj / tot)) - (log(si) + log(sj));           // :505-507
        }
        L.pick[0] = split; L.pick[1] = cli; L.pick[2] = clj; L.val[0] = size_data;
    }
    __syncthreads();
    m.split = L.pick[0] != 0; m.cli = L.pick[1]; m.clj = m.split ? free_id : L.pick[2]; m.size_data = L.val[0];
    m.th_i = d.theta + ((size_t)m.c * N + m.cli) * d.M; m.th_j = d.theta + ((size_t)m.c * N + m.clj) * d.M;
    const int nA = sm_compact(m.lab, N, m.cli, m.cli, -1, -1, m.b.A, L.cnt);
    const int nB = m.split ? 0 : sm_compact(m.lab, N, m.clj, m.clj, -1, -1, m.b.B, L.cnt);
    if (t == 0) {
        double a0, a1;
        doubles(m.key, 0, m.step, P_SM, 2, a0, a1);
        const int ii = min((int)(a0 * (double)nA), nA - 1);
        int aj;
        if (m.split) { int jj = min((int)(a1 * (double)(nA - 1)), nA - 2); jj += jj >= ii; aj = m.b.A[jj]; }
        else aj = m.b.B[min((int)(a1 * (double)nB), nB - 1)];
        L.pick[3] = m.b.A[ii]; L.pick[4] = aj;
    }
    __syncthreads();
    m.ai = L.pick[3]; m.aj = L.pick[4];
    m.nS = sm_compact(m.lab, N, m.cli, m.split ? m.cli : m.clj, m.ai, m.aj, m.b.S, L.cnt);
}

// _rg_init_split's likelihood of a cell under an anchor's data as parameters (:557-560): popcounts times the six constants, in their order
__device__ inline double sm_anchor_ll(const SDev& d, const Rates& er, int cell, int anchor) {
    int n[6] = {0, 0, 0, 0, 0, 0};
    for (int w = 0; w < d.W; ++w) {
        const uint64_t co = d.one[(size_t)cell * d.W + w], cz = d.zero[(size_t)cell * d.W + w];
        const uint64_t ao = d.one[(size_t)anchor * d.W + w], az = d.zero[(size_t)anchor * d.W + w], am = ~(ao | az);
        n[0] += __popcll(co & ao); n[1] += __popcll(cz & ao); n[2] += __popcll(co & az); n[3] += __popcll(cz & az); n[4] += __popcll(co & am); n[5] += __popcll(cz & am);
    }
    double ll = 0.0;
#pragma unroll
    for (int k = 0; k < 6; ++k) ll = ll + (double)n[k] * er.sm_anchor[k];
    return ll;
}

// n1 / n0 of rows 0 and 1 from the assignment of S and the two anchors, and row 2 as their sum
__device__ void sm_count(const SDev& d, const Sm& m) {
    const int M = d.M, nS = m.nS, ai = m.ai, aj = m.aj;           // by value: a choice between two members of m is one between their addresses, and keeps m in memory
    const SmBuf& b = m.b;
    for (int e = threadIdx.x; e < 2 * M; e += 256) { b.n1[e] = 0; b.n0[e] = 0; }
    __syncthreads();
    for (int s = threadIdx.x; s < nS + 2; s += 256) {
        const int cell = s < nS ? b.S[s] : s == nS ? ai : aj, r = s < nS ? b.asg[s] : s - nS;
        count_cell(d, cell, b.n1 + r * M, b.n0 + r * M);
    }
    __syncthreads();
    for (int k = threadIdx.x; k < M; k += 256) { b.n1[2 * M + k] = b.n1[k] + b.n1[M + k]; b.n0[2 * M + k] = b.n0[k] + b.n0[M + k]; }
    __syncthreads();
}

__device__ void sm_tables(const SDev& d, const Sm& m, int r0, int r1) {
    for (int e = r0 * d.M + threadIdx.x; e < r1 * d.M; e += 256) { double l1, l0; log_terms(m.er, m.b.th[e], l1, l0); m.b.L1[e] = l1; m.b.L0[e] = l0; }
    __syncthreads();
}

// _rg_init_split (:547-568), the launch state of run_rg_nc (:527-544): S assigned by the anchors, the rows' counts, Beta draws and tables
__device__ inline void sm_launch(const SDev& d, const Sm& m) {
    const int t = threadIdx.x, M = d.M;
    const SmBuf& b = m.b;
    for (int s = t; s < m.nS; s += 256) { const int cell = b.S[s]; b.asg[s] = sm_anchor_ll(d, m.er, cell, m.aj) > sm_anchor_ll(d, m.er, cell, m.ai) ? 1 : 0; }
    __syncthreads();
    sm_count(d, m);
    for (int e = t; e < 3 * M; e += 256) {
        const int r = e / M, k = e - r * M;
        const double x = beta_variate(m.key, (uint32_t)k, m.step, (uint32_t)P_SM_BETA | ((uint32_t)r << 8), d.p + (double)b.n1[e], d.q + (double)b.n0[e], d.err + m.c);
        b.th[e] = (float)fmin(fmax(x, S_TMIN), S_TMAX);
    }
    __syncthreads();
    sm_tables(d, m, 0, 3);
}

// MH_cluster_params(trans_prob=True) (:314-342) of rows r0 .. r1-1 at scan `scan`, a lane per (row, mutation); sums[r] gets the row's
// transition probability in every lane, and the moved rows' tables are made again
__device__ void sm_move_rows(const SDev& d, const Sm& m, int scan, int r0, int r1, double* sums, double* shd) {
    const int M = d.M;
    const SmBuf& b = m.b;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0;
    for (int e = r0 * M + threadIdx.x; e < r1 * M; e += 256) {
        const int r = e / M, k = e - r * M;
        const uint32_t pw = (uint32_t)P_SM_MH | ((uint32_t)(4 * scan + r) << 8);
        double u, v;
        doubles(m.key, (uint32_t)k, m.step, pw, 0, u, v);
        const double sd = PROPOSAL_SD[sd_pick(m.key, (uint32_t)k, m.step, pw, 1)];
        const float old = b.th[e];
        const float nw = truncnorm_variate(u, old, sd);
        const double A = fmin(log_A(d, m.er, nw, old, (double)b.n1[e], (double)b.n0[e], sd, false), 0.0);
        double share;
        if (log(v) < A) { b.th[e] = nw; share = A; }
        else share = log(-expm1(A));
        if (r == 0) a0 += share; else if (r == 1) a1 += share; else a2 += share;
    }
    sums[0] = block_sum(a0, shd); sums[1] = block_sum(a1, shd); sums[2] = block_sum(a2, shd);
    sm_tables(d, m, r0, r1);
}

// _rg_scan_assign (:609-632) of S over rows 0 and 1 with its transition probability, and the rows' counts under the assignment it leaves;
// with `back` the in-order walk of _rg_get_split_prob (:803-818) over the two clusters' own tables, which assigns the original cluster
// instead of drawing.  The likelihoods of all cells of S under the two rows are taken once; the walk's records are laid out in walk order,
// lane 0 walks them, the lanes scatter its picks.  Every lane gets the sum; 0 without a walk for an empty S (:571-572)
__device__ double sm_scan(const SDev& d, const Sm& m, int scan, bool back, SmLds& L) {
    const int t = threadIdx.x, nS = m.nS, clj = back ? m.clj : -1;
    if (nS == 0) return 0.0;
    const SmBuf& b = m.b;
    const size_t M = d.M, own = (size_t)m.c * d.N * M;
    const double* l1a = back ? d.L1 + own + m.cli * M : b.L1; const double* l0a = back ? d.L0 + own + m.cli * M : b.L0;
    const double* l1b = back ? d.L1 + own + m.clj * M : b.L1 + M; const double* l0b = back ? d.L0 + own + m.clj * M : b.L0 + M;
    uint64_t* keys = d.keys + (size_t)m.c * d.N;
    int32_t* pos = d.order + (size_t)m.c * d.N;
    for (int s = t; s < nS; s += 256) {
        const int cell = b.S[s];
        b.ll[2 * s] = masked_ll(d, cell, l1a, l0a); b.ll[2 * s + 1] = masked_ll(d, cell, l1b, l0b);
        if (clj < 0) {
            uint32_t w[4];
            philox4x32(m.key, (uint32_t)cell, m.step, (uint32_t)P_SM_PERM | ((uint32_t)scan << 8), 0, w);
            keys[s] = ((uint64_t)w[1] << 32) | w[0];
            double u, u_unused;
            doubles(m.key, (uint32_t)cell, m.step, (uint32_t)P_SM_CHOICE | ((uint32_t)scan << 8), 0, u, u_unused);
            b.u[s] = u;
        }
    }
    __syncthreads();
    for (int base = 0; base < nS; base += 256) {
        const int s = base + t;
        // the rank of the cell's key among the keys of S: ties go by the position in S, which is the order of the ids
        const int rank = clj < 0 ? block_rank(keys, nS, s, L.tile) : s;
        if (s < nS) {
            pos[rank] = s;
            b.wll[2 * rank] = b.ll[2 * s]; b.wll[2 * rank + 1] = b.ll[2 * s + 1];
            b.wu[rank] = clj < 0 ? b.u[s] : 0.0;
            b.pick[rank] = clj < 0 ? b.asg[s] : (b.asg[s] | ((m.lab[b.S[s]] == clj ? 1 : 0) << 1));      // bit 0: where it is, bit 1: where it goes
        }
    }
    __syncthreads();
    if (t == 0) {
        const int nn = nS + 2;
        const double lden = log((double)(nn - 1) + m.alpha);
        int on_j = 0;
        for (int r = 0; r < nS; ++r) on_j += b.pick[r] & 1;
        double prob = 0.0;
        for (int r = 0; r < nS; ++r) {
            const int was = b.pick[r];
            const int others = on_j - (was & 1), n_j = others + 1, n_i = nn - n_j - 1;
            const double lp0 = b.wll[2 * r] + (log((double)n_i) - lden), lp1 = b.wll[2 * r + 1] + (log((double)n_j) - lden);
            // _normalize_log (:104-116): the tables are finite, so its FloatingPointError branch is never met
            double o0, o1;
            if (lp0 >= lp1) { const double z = log1p(exp(lp1 - lp0)); o0 = 0.0 - z; o1 = (lp1 - lp0) - z; }
            else { const double z = log1p(exp(lp0 - lp1)); o0 = (lp0 - lp1) - z; o1 = 0.0 - z; }
            int nw;
            if (clj < 0) { const double p0 = exp(o0), p1 = exp(o1); nw = p0 / (p0 + p1) > b.wu[r] ? 0 : 1; }
            else nw = was >> 1;
            b.pick[r] = nw;
            on_j = others + nw;
            prob += nw ? o1 : o0;
        }
        L.val[1] = prob;
    }
    __syncthreads();
    for (int r = t; r < nS; r += 256) b.asg[pos[r]] = b.pick[r];
    __syncthreads();
    sm_count(d, m);
    return L.val[1];
}

// the way from rows r0 .. r1-1 back to the clusters' own parameters (row 1: cluster j's) under fresh sds: the sum of their clipped log A
// (_get_trans_prob_ratio_split, :672-676; _rg_get_split_prob with unit bounds, :783-797)
__device__ inline double sm_way_back(const SDev& d, const Sm& m, int r0, int r1, bool unit, double* shd) {
    const int M = d.M;
    double acc = 0.0;
    for (int e = r0 * M + threadIdx.x; e < r1 * M; e += 256) {
        const int r = e / M, k = e - r * M;
        const double sd = PROPOSAL_SD[sd_pick(m.key, (uint32_t)k, m.step, (uint32_t)P_SM_SD | ((uint32_t)r << 8), 0)];
        acc += fmin(log_A(d, m.er, r == 1 ? m.th_j[k] : m.th_i[k], m.b.th[e], (double)m.b.n1[e], (double)m.b.n0[e], sd, unit), 0.0);
    }
    return block_sum(acc, shd);
}

// _do_rg_split_MH's proposal (:641-645), one more scan and move of rows 0 and 1, and _get_trans_prob_ratio_split (:668-682) of it
__device__ inline double sm_split_proposal(const SDev& d, const Sm& m, SmLds& L) {
    double sums[3];
    const double prob_cl = sm_scan(d, m, d.sm_scans, false, L);
    sm_move_rows(d, m, d.sm_scans, 0, 2, sums, L.shd);
    const double gs_split = prob_cl + (sums[0] + sums[1]);
    return sm_way_back(d, m, 2, 3, false, L.shd) - gs_split;
}

// _do_rg_merge_MH's proposal (:656-660), one more move of row 2, and _get_trans_prob_ratio_merge (:685-692) of it: _rg_get_split_prob
// (:777-820) walks S in order to the two clusters' cells, so the assignment and the rows' counts are the original ones afterwards (:817)
__device__ inline double sm_merge_proposal(const SDev& d, const Sm& m, SmLds& L) {
    double sums[3];
    sm_move_rows(d, m, d.sm_scans, 2, 3, sums, L.shd);
    const double par = sm_way_back(d, m, 0, 2, true, L.shd);
    const double prob_assign = sm_scan(d, m, d.sm_scans, true, L);
    return (par + prob_assign) - sums[2];
}

// sum over a row's mutations of n1 L1 + n0 L0: the likelihood of the row's cells under the row
__device__ inline double sm_ll_of_row(const SDev& d, const SmBuf& b, int r, double* shd) {
    double acc = 0.0;
    for (int k = threadIdx.x; k < d.M; k += 256) { const int e = r * d.M + k; acc += (double)b.n1[e] * b.L1[e] + (double)b.n0[e] * b.L0[e]; }
    return block_sum(acc, shd);
}

// the ratio's terms behind the transition's into t[1 .. 3], from the state the proposal leaves (_do_rg_split_MH :646-653, _do_rg_merge_MH
// :661-665): _get_lprior_ratio_split / _merge (:695-713, :736-754) of the rows proposed (a split's 0 and 1, a merge's 2) against the clusters'
// own parameters, _get_ll_ratio (:716-733), _get_ltrans_prob_size_ratio_split / _merge (:757-774).  Returns how many cells of S are on the j side
__device__ inline int sm_ratio_terms(const SDev& d, const Sm& m, double* shd, double* t) {
    const int tx = threadIdx.x, M = d.M, nn = m.nS + 2;
    double cj = 0.0, pa = 0.0, pb = 0.0, inv = 0.0;
    for (int s = tx; s < m.nS; s += 256) cj += m.b.asg[s];
    const int on_j = (int)block_sum(cj, shd);
    const double n_j = (double)(on_j + 1), n_i = (double)nn - n_j;
    const double ll0 = sm_ll_of_row(d, m.b, 0, shd), ll1 = sm_ll_of_row(d, m.b, 1, shd), ll2 = sm_ll_of_row(d, m.b, 2, shd);
    if (!d.uniform && m.split) for (int k = tx; k < M; k += 256) { pa += beta_logpdf(d, m.b.th[k]) + beta_logpdf(d, m.b.th[M + k]); pb += beta_logpdf(d, m.th_i[k]); }
    if (!d.uniform && !m.split) {
        for (int e = tx; e < 2 * M; e += 256) pb += beta_logpdf(d, e < M ? m.th_i[e] : m.th_j[e - M]);
        for (int k = tx; k < M; k += 256) pa += beta_logpdf(d, m.b.th[2 * M + k]);
    }
    pa = block_sum(pa, shd); pb = block_sum(pb, shd);
    if (m.split) {
        for (int j = tx; j < m.K; j += 256) if (m.live[j] != m.cli) inv += 1.0 / (double)m.size[m.live[j]];
        inv = block_sum(inv, shd);
        t[1] = (log(m.alpha) - lgamma((double)nn)) + lgamma(n_j);    // :702-706
        t[1] += lgamma(n_i);
        t[2] = ll0 + ll1 - ll2;
        const double norm = inv + 1.0 / n_i + 1.0 / n_j;             // :762-764
        t[3] = log(1.0 / n_i / norm) + log(1.0 / n_j / norm) - m.size_data;
    } else {
        t[1] = -(log(m.alpha) - lgamma((double)nn)) - lgamma(n_j);   // :743-747
        t[1] -= lgamma(n_i);
        t[2] = ll2 - ll0 - ll1;
        // log(|S| - 1) raises for |S| of 0 or 1 under the reference's np.seterr, and the term falls back (:769-773)
        t[3] = (m.nS > 1 ? -log((double)d.N) - log((double)(m.nS - 1)) : -log((double)d.N)) - m.size_data;
    }
    if (!d.uniform) t[1] += pa - pb;
    return on_j;
}

// an accepted move on the chain's state (:465-477, :513-520): the rows become the clusters' parameters, the j side's cells change cluster
__device__ inline void sm_apply(const SDev& d, const Sm& m, int on_j) {
    const int t = threadIdx.x, M = d.M, to = m.split ? m.clj : m.cli;
    for (int k = t; k < M; k += 256) {
        if (m.split) { m.th_i[k] = m.b.th[k]; m.th_j[k] = m.b.th[M + k]; }
        else m.th_i[k] = m.b.th[2 * M + k];
    }
    for (int s = t; s < m.nS; s += 256) if (m.b.asg[s]) m.lab[m.b.S[s]] = to;
    if (t == 0) {
        m.lab[m.aj] = to;
        if (m.split) { m.size[m.clj] = on_j + 1; m.size[m.cli] -= on_j + 1; }
        else { m.size[m.cli] += m.size[m.clj]; m.size[m.clj] = 0; }
    }
}

__global__ __launch_bounds__(256) void k_bnpcs_sm(SDev d, uint32_t step, int force) {
    __shared__ SmLds L;
    const int c = blockIdx.x, t = threadIdx.x;
    Sm m;
    m.c = c; m.step = step; m.key = d.seeds[c];
    double u0, u_kind;
    doubles(m.key, 0, step, P_SM, 0, u0, u_kind);
    if (!force && !(u0 < d.sm_prob)) return;                       // this chain's step is a sweep: k_bnpcs_scan has made it
    m.K = d.nlive[c]; m.alpha = d.alpha[c]; m.er = d.rates[c]; m.b = sm_buf(d, c);
    m.lab = d.lab + (size_t)c * d.N; m.size = d.size + (size_t)c * d.N; m.live = d.live + (size_t)c * d.N;
    sm_choose(d, m, u_kind, L);
    sm_launch(d, m);
    double sums[3], term[4];
    for (int sc = 0; sc < d.sm_scans; ++sc) {                      // run_rg_nc's restricted scans (:537-542)
        sm_scan(d, m, sc, false, L);
        sm_move_rows(d, m, sc, 0, 3, sums, L.shd);
    }
    term[0] = m.split ? sm_split_proposal(d, m, L) : sm_merge_proposal(d, m, L);
    const int on_j = sm_ratio_terms(d, m, L.shd, term);
    const double A = ((term[0] + term[1]) + term[2]) + term[3];
    double v, v_unused;
    doubles(m.key, 0, step, P_SM, 3, v, v_unused);
    const bool refused = m.split && m.nS > 0 && (on_j == 0 || on_j == m.nS);   // np.unique(rg_assignment).size == 1 (:647)
    const bool accept = !refused && log(v) < A;
    const int code = m.split ? (accept ? 2 : 1) : (accept ? 4 : 3);
    if (accept) sm_apply(d, m, on_j);
    if (t == 0) {
        double* o = m.b.out;
        o[0] = (double)code; o[1] = (double)m.cli; o[2] = (double)m.clj; o[3] = (double)m.ai; o[4] = (double)m.aj; o[5] = A;
        o[6] = term[0]; o[7] = term[1]; o[8] = term[2]; o[9] = term[3]; o[10] = log(v); o[11] = (double)m.nS;
        if ((int)step < d.steps1) d.rec_sm[(size_t)c * d.steps1 + step] = code;
    }
    __syncthreads();
    alpha_update(d, c, step, m.size, m.alpha, L.shd);
}

// ---- the error-rate update (update_error_rates / MH_error_rates, CRP_learning_errors.py:52-111; Chain.do_step, MCMC.py:339-342; the draws
// are in longsom_amd/bnpc_sampler.py's docstring).  One workgroup per chain, after the parameter move and its tables: the FP move, then
// the FN move, which sees the FP move's result.  get_ll_full_error (:58-63) under the trial rates is sum_k sum_m n1 L1' + n0 L0' over the live
// clusters: the lanes stride over clusters x mutations, block_sum adds in a fixed order.  The scalar terms are the same in every lane.
// An accepted move rewrites the chain's Rates; the host makes the tables again behind this kernel.
// The rates' own density, apart from truncnorm_logpdf: a rate and its bounds 0 and 1 are doubles and the differences are formed in double,
// where a parameter's are formed in float32
__device__ inline double unit_truncnorm_logpdf(double x, double loc, double sd) {
    const double pa = normcdf((0.0 - loc) / sd), pb = normcdf((1.0 - loc) / sd);
    const double z = (x - loc) / sd;
    return -0.5 * z * z - 0.5 * log(2.0 * M_PI) - log(sd) - log(pb - pa);
}

__device__ double err_ll(const SDev& d, int c, int K, double FP, double FN, double* shd) {
    const int32_t* live = d.live + (size_t)c * d.N;
    Rates trial;
    rates_set(trial, FP, FN);
    double acc = 0.0;
    for (int64_t e = threadIdx.x; e < (int64_t)K * d.M; e += 256) {
        const int j = (int)(e / d.M), m = (int)(e - (int64_t)j * d.M);
        const size_t at = ((size_t)c * d.N + live[j]) * d.M + m;
        double l1, l0;
        log_terms(trial, d.theta[at], l1, l0);
        acc += (double)d.n1[at] * l1 + (double)d.n0[at] * l0;
    }
    return block_sum(acc, shd);
}

__global__ __launch_bounds__(256) void k_bnpcs_err(SDev d, uint32_t step) {
    __shared__ double shd[4];
    const int c = blockIdx.x, t = threadIdx.x, N = d.N, K = d.nlive[c];
    const uint64_t key = d.seeds[c];
    double* out = d.err_out + (size_t)c * ERR_OUT;
    double u0, u_unused;
    doubles(key, 0, step, P_ERR, 0, u0, u_unused);
    if (!(u0 < d.err_prob)) { if (t == 0) out[0] = 0.0; return; }
    const int32_t* live = d.live + (size_t)c * N;
    double rate[2] = {d.rates[c].FP, d.rates[c].FN};
    // the likelihood under the current rates: the sum of the tables' rows, as the record takes it
    const auto [j0, j1] = lane_run(K);
    double old_ll = 0.0;
    for (int j = j0; j < j1; ++j) old_ll += d.rowml[(size_t)c * N + live[j]];
    old_ll = block_sum(old_ll, shd);
    bool moved = false;
    for (int e = 0; e < 2; ++e) {
        const uint32_t purpose = e == 0 ? P_ERR_FP : P_ERR_FN;
        double u, v;
        doubles(key, 0, step, purpose, 0, u, v);
        constexpr double of_prior[3] = {0.5, 1.0, 1.5};                // FP_sd, FN_sd (CRP_learning_errors.py:26, 32): three, times the prior's sd
        const uint32_t pick = sd_pick(key, 0, step, purpose, 1);
        const double psd = d.err_sd[e], sd = psd * of_prior[pick];
        const double old = rate[e];
        const double pa = normcdf((0.0 - old) / sd), pb = normcdf((1.0 - old) / sd);
        const double nw = old + sd * normcdfinv(pa + u * (pb - pa));
        const bool inside = nw > 0.0 && nw < 1.0;                    // rounding can put it on an end: declined, and counted as a variate error
        const double trial = inside ? nw : old;
        const double new_ll = err_ll(d, c, K, e == 0 ? trial : rate[0], e == 0 ? rate[1] : trial, shd);
        const double new_p = unit_truncnorm_logpdf(trial, old, sd), old_p = unit_truncnorm_logpdf(old, trial, sd);
        const double new_prior = unit_truncnorm_logpdf(trial, d.err_mean[e], psd), old_prior = unit_truncnorm_logpdf(old, d.err_mean[e], psd);
        const double A = new_ll + new_prior - old_ll - old_prior + old_p - new_p;
        const double lv = log(v);
        const bool accept = inside && lv < A;
        if (t == 0) {
            double* o = out + 1 + 10 * e;
            o[0] = (double)pick; o[1] = nw; o[2] = new_ll; o[3] = old_ll; o[4] = new_prior - old_prior; o[5] = new_p; o[6] = old_p; o[7] = A; o[8] = lv;
            o[9] = accept ? 1.0 : inside ? 0.0 : -1.0;
            d.err_cnt[4 * c + 2 * e + (accept ? 0 : 1)] += 1;
            if (!inside) atomicAdd(d.err + c, 1);
        }
        if (accept) { rate[e] = nw; old_ll = new_ll; moved = true; }
    }
    if (t == 0) {
        out[0] = 1.0;
        if (moved) rates_fill(d.rates[c], rate[0], rate[1], d.mix0, d.mix1);
    }
}

// ---- record (Chain.update_results, MCMC.py:242-282): ML, the two prior sums, the labels, and after burn-in the live clusters' parameters
// in ascending id into the arena.  A workgroup per chain. ------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_bnpcs_record(SDev d, int32_t step, int32_t keep, const int64_t* used) {
    __shared__ double shd[4];
    const int c = blockIdx.x, t = threadIdx.x, N = d.N, K = d.nlive[c];
    const int32_t* live = d.live + (size_t)c * N;
    const double alpha = d.alpha[c], lden = log((double)(N - 1) + alpha);
    const auto [j0, j1] = lane_run(K);
    double ml = 0.0, crp = 0.0, bp = 0.0;
    for (int j = j0; j < j1; ++j) {
        const size_t row = (size_t)c * N + live[j];
        ml += d.rowml[row]; bp += d.rowb[row];
        crp += log((double)d.size[row]) - lden;
    }
    ml = block_sum(ml, shd); crp = block_sum(crp, shd); bp = block_sum(bp, shd);
    if (t == 0) {
        double* r = d.rec_sc + ((size_t)c * d.steps1 + step) * REC;
        r[0] = ml; r[1] = crp; r[2] = bp; r[3] = (double)K; r[4] = alpha;
        double* e = d.rec_err + ((size_t)c * d.steps1 + step) * 2;
        e[0] = d.rates[c].FP; e[1] = d.rates[c].FN;
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

// ---- lsg_bnpcs_extend: the records [chain][steps1][rec] moved to rows of a larger steps1.  rec, old_row and new_row in 32-bit words
// (every record is a whole number of them); only the `used` words of a row that hold records made so far are moved. -----------------------
__global__ __launch_bounds__(256) void k_bnpcs_restride(uint32_t* dst, const uint32_t* src, size_t old_row, size_t new_row, size_t used, int32_t C) {
    for (int c = blockIdx.y; c < C; c += gridDim.y) {
        const uint32_t* s = src + (size_t)c * old_row;
        uint32_t* o = dst + (size_t)c * new_row;
        for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < used; i += (size_t)gridDim.x * 256) o[i] = s[i];
    }
}

// ---- lsg_bnpcs_psrf: what the lugsail batch-means PSRF (utils.get_lugsail_batch_means_est, utils.py:427-467) needs of a chain's ML
// records first .. last - 1: n, the mean, the sample variance, tau(b) and tau(b // 3), tau(b) = b / (a - 1) sum (batch mean - mean)^2
// over the a = n / b whole batches.  All sums are of x - x[first] (the ML is about -1e4 with a spread of a few units), in two passes: the
// mean first, then the deviations.  A workgroup per chain; a wave sums a batch.  par [chain][3]: first, b, b // 3; out [chain][5]. -------
__device__ inline double psrf_tau(const double* x, double pivot, double mean, int32_t n, int32_t b, double* shd) {
    const int t = threadIdx.x, lane = t & 63, a = n / b;
    double acc = 0.0;
    for (int j = t >> 6; j < a; j += 4) {
        double s = 0.0;
        for (int i = lane; i < b; i += 64) s += x[((size_t)j * b + i) * REC] - pivot;
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        const double dev = s / (double)b - mean;
        if (lane == 0) acc += dev * dev;
    }
    return (double)b / (double)(a - 1) * block_sum(acc, shd);
}

__global__ __launch_bounds__(256) void k_bnpcs_psrf(SDev d, const int32_t* par, int32_t last, double* out) {
    __shared__ double shd[4];
    const int c = blockIdx.x, t = threadIdx.x;
    const int32_t first = par[3 * c], b = par[3 * c + 1], b3 = par[3 * c + 2], n = last - first;
    double* o = out + 5 * (size_t)c;
    if (n < 1) {                                                      // no record is read
        if (t < 5) o[t] = 0.0;
        return;
    }
    const double* x = d.rec_sc + ((size_t)c * d.steps1 + first) * REC;      // x[i * REC]: the ML of step first + i
    const double pivot = x[0];
    double s = 0.0;
    for (int i = t; i < n; i += 256) s += x[(size_t)i * REC] - pivot;
    const double mean = block_sum(s, shd) / (double)n;
    double q = 0.0;
    for (int i = t; i < n; i += 256) { const double e = (x[(size_t)i * REC] - pivot) - mean; q += e * e; }
    q = block_sum(q, shd);
    const bool whole = n >= 9 && b >= 3 && b3 >= 1;                   // fewer than 9 values: b // 3 is 0 and the estimate is inf (utils.py:435)
    const double tau = whole ? psrf_tau(x, pivot, mean, n, b, shd) : 0.0;
    const double tau3 = whole ? psrf_tau(x, pivot, mean, n, b3, shd) : 0.0;
    if (t == 0) {
        o[0] = (double)n; o[1] = pivot + mean; o[2] = n > 1 ? q / (double)(n - 1) : 0.0; o[3] = tau; o[4] = tau3;
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
    d.p = b.p; d.q = b.q; d.g0 = b.g0; d.g1 = b.g1; d.dpa_prob = b.dpa_prob;
    d.uniform = d.p == 1.0 && d.q == 1.0;
    d.betaln = b.betaln; d.mix0 = b.mix[0]; d.mix1 = b.mix[1];
    d.err_prob = b.err_prob; d.err_mean[0] = b.err_prior[0]; d.err_sd[0] = b.err_prior[1]; d.err_mean[1] = b.err_prior[2]; d.err_sd[1] = b.err_prior[3];
    d.rates = b.rates.as<Rates>(); d.rec_err = b.rec_err.as<double>(); d.err_out = b.err_out.as<double>(); d.err_cnt = b.err_cnt.as<int32_t>();
    d.one = b.one.as<uint64_t>(); d.zero = b.zero.as<uint64_t>(); d.seeds = b.seeds.as<uint64_t>(); d.pop = b.pop.as<int32_t>();
    d.lab = b.lab.as<int32_t>(); d.size = b.size.as<int32_t>(); d.colof = b.colof.as<int32_t>(); d.live = b.live.as<int32_t>(); d.nlive = b.nlive.as<int32_t>();
    d.hi = b.hi.as<int32_t>(); d.order = b.order.as<int32_t>(); d.rec_lab = b.rec_lab.as<int32_t>(); d.err = b.err.as<int32_t>();
    d.theta = b.theta.as<float>(); d.arena = b.arena.as<float>();
    d.L1 = b.L1.as<double>(); d.L0 = b.L0.as<double>(); d.LL = b.LL.as<double>(); d.alpha = b.alpha.as<double>(); d.prow = b.prow.as<double>();
    d.rowml = b.rowml.as<double>(); d.rowb = b.rowb.as<double>(); d.rec_sc = b.rec_sc.as<double>();
    d.n1 = b.n1.as<uint32_t>(); d.n0 = b.n0.as<uint32_t>(); d.keys = b.keys.as<uint64_t>();
    d.sm_prob = b.sm_prob; d.sm_edge = b.sm_ratio[0] / (b.sm_ratio[0] + b.sm_ratio[1]); d.sm_scans = b.sm_scans;
    d.sm_i = b.sm_i.as<int32_t>(); d.rec_sm = b.rec_sm.as<int32_t>(); d.sm_d = b.sm_d.as<double>(); d.sm_c = b.sm_c.as<uint32_t>(); d.sm_t = b.sm_t.as<float>();
    return d;
}

static int need(lsg_ctx* c, const char* who) {
    if (!c) { set_error("%s: NULL handle", who); return -2; }
    if (hipSetDevice(c->device) != hipSuccess) { set_error("%s: hipSetDevice failed", who); return -1; }
    if (!c->bnpcs.valid) { set_error("%s: no sampler (lsg_bnpcs_create first)", who); return -2; }
    return 0;
}

// the tables under the chains' parameters and rates as they are now
static void launch_tables(lsg_ctx* c) {
    Bnpcs& b = c->bnpcs;
    hipLaunchKernelGGL(k_bnpcs_tables, dim3(b.n_cells, b.n_chains), dim3(64), 0, c->stream, dev_of(b));
}

// what follows a change of the assignment: the live list and its count on the host, then the clusters' counts and tables
static int refresh_clusters(lsg_ctx* c, const char* who) {
    Bnpcs& b = c->bnpcs;
    hipLaunchKernelGGL(k_bnpcs_live, dim3(b.n_chains), dim3(256), 0, c->stream, dev_of(b));
    LSG_HIP(hipMemcpyAsync(b.h_k.data(), b.nlive.p, (size_t)b.n_chains * 4, hipMemcpyDeviceToHost, c->stream));
    if (sync_check(c, who)) return -1;
    b.k_max = *std::max_element(b.h_k.begin(), b.h_k.end());
    const size_t cells = (size_t)b.n_chains * b.n_cells * b.n_muts;
    LSG_HIP(hipMemsetAsync(b.n1.p, 0, cells * 4, c->stream));
    LSG_HIP(hipMemsetAsync(b.n0.p, 0, cells * 4, c->stream));
    hipLaunchKernelGGL(k_bnpcs_counts, dim3((b.n_cells + 255) / 256, b.n_chains), dim3(256), 0, c->stream, dev_of(b));
    launch_tables(c);
    return 0;
}

// after lsg_bnpcs_set_state: the sizes are the caller's labels'; the live list, the counts and the tables follow
static int prepare(lsg_ctx* c, const char* who) {
    Bnpcs& b = c->bnpcs;
    if (b.prepared) return 0;
    if (int rc = refresh_clusters(c, who)) return rc;
    b.prepared = true;
    return 0;
}

// the likelihood matrix against the clusters alive now, a column each
static int launch_ll(lsg_ctx* c) {
    Bnpcs& b = c->bnpcs;
    b.ll_pitch = std::max(b.k_max, 1);
    if (b.LL.reserve((size_t)b.n_chains * b.n_cells * b.ll_pitch * 8)) return -1;
    hipLaunchKernelGGL(k_bnpcs_ll, dim3((b.ll_pitch + LT - 1) / LT, (b.n_cells + LT - 1) / LT, b.n_chains), dim3(256), 0, c->stream, dev_of(b));
    return 0;
}

// ---- the three phases of a step (Chain.do_step, MCMC.py:316-342), in its order.  Each leaves the tables right for the next. -------------
// The assignment: with `sweep` and `move` each chain draws which of the two its step is, as a run has it; with one of them every chain
// makes that one; with neither (a fixed assignment) none.  Then what follows a change of the assignment
static int step_assign(lsg_ctx* c, const char* who, uint32_t step, bool sweep, bool move) {
    Bnpcs& b = c->bnpcs;
    if (sweep) {
        if (int rc = launch_ll(c)) return rc;
        const SDev d = dev_of(b);
        hipLaunchKernelGGL(k_bnpcs_keys, dim3((b.n_cells + 255) / 256, b.n_chains), dim3(256), 0, c->stream, d, step);
        hipLaunchKernelGGL(k_bnpcs_perm, dim3((b.n_cells + 255) / 256, b.n_chains), dim3(256), 0, c->stream, d);
        hipLaunchKernelGGL(k_bnpcs_scan, dim3(b.n_chains), dim3(256), 0, c->stream, d, step, move ? 1 : 0);
    }
    if (move) hipLaunchKernelGGL(k_bnpcs_sm, dim3(b.n_chains), dim3(256), 0, c->stream, dev_of(b), step, sweep ? 0 : 1);
    return refresh_clusters(c, who);
}

// the parameter move
static void step_params(lsg_ctx* c, uint32_t step) {
    Bnpcs& b = c->bnpcs;
    hipLaunchKernelGGL(k_bnpcs_mh, dim3((b.n_muts + 63) / 64, std::max(b.k_max, 1), b.n_chains), dim3(64), 0, c->stream, dev_of(b), step);
    launch_tables(c);
}

// the error-rate update of the chains whose draw says so
static void step_errors(lsg_ctx* c, uint32_t step) {
    Bnpcs& b = c->bnpcs;
    hipLaunchKernelGGL(k_bnpcs_err, dim3(b.n_chains), dim3(256), 0, c->stream, dev_of(b), step);
    launch_tables(c);
}

// the state's size, which the chains' parameters, tables and counts, the label records and the arena make up; refused past 64 GB
static int check_state_size(const char* who, const char* verb, size_t C, size_t N, size_t M, size_t S1, int64_t arena_rows) {
    const double bytes = (double)C * N * M * (4 + 8 + 8 + 4 + 4) + (double)C * S1 * N * 4 + (double)C * arena_rows * M * 4;
    if (bytes <= 64e9) return 0;
    set_error("%s: %zu chains x %zu cells x %zu mutations x %zu steps %s %.0f GB of state", who, C, N, M, S1 - 1, verb, bytes / 1e9);
    return -2;
}

// every chain's rates become r
static int upload_rates(lsg_ctx* c, const Rates& r) {
    Bnpcs& b = c->bnpcs;
    const std::vector<Rates> all((size_t)b.n_chains, r);
    LSG_HIP(hipMemcpyAsync(b.rates.p, all.data(), all.size() * sizeof(Rates), hipMemcpyHostToDevice, c->stream));
    LSG_HIP(hipStreamSynchronize(c->stream));                      // (`all` is read by the copy until here)
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
    if (int rc = check_state_size(who, "need", C, N, M, S1, arena_rows)) return rc;
    // the state's buffers and their bytes; the second list is of those that start as zeros
    const struct { DevBuf* buf; size_t bytes; } plain[] = {
        {&b.one, N * W * 8}, {&b.zero, N * W * 8}, {&b.pop, N * 8}, {&b.seeds, C * 8}, {&b.colof, C * N * 4}, {&b.live, C * N * 4}, {&b.nlive, C * 4}, {&b.hi, C * 4},
        {&b.L1, C * N * M * 8}, {&b.L0, C * N * M * 8}, {&b.prow, C * (N + 1) * 8}, {&b.n1, C * N * M * 4}, {&b.n0, C * N * M * 4}, {&b.rowml, C * N * 8}, {&b.rowb, C * N * 8},
        {&b.order, C * N * 4}, {&b.keys, C * N * 8}, {&b.arena, C * (size_t)arena_rows * M * 4}, {&b.used, C * 8}, {&b.sm_i, C * 5 * N * 4}, {&b.sm_c, C * 6 * M * 4},
        {&b.sm_t, C * 3 * M * 4}, {&b.rates, C * sizeof(Rates)}},
      zeroed[] = {
        {&b.lab, C * N * 4}, {&b.size, C * N * 4}, {&b.theta, C * N * M * 4}, {&b.alpha, C * 8}, {&b.err, C * 4}, {&b.rec_lab, C * S1 * N * 4}, {&b.rec_sc, C * S1 * REC * 8},
        {&b.rec_sm, C * S1 * 4}, {&b.sm_d, C * sm_d_size(N, M) * 8}, {&b.rec_err, C * S1 * 2 * 8}, {&b.err_cnt, C * 4 * 4}, {&b.err_out, C * ERR_OUT * 8}};
    for (const auto& x : plain) if (x.buf->reserve(x.bytes)) return -1;
    for (const auto& x : zeroed) if (x.buf->reserve(x.bytes)) return -1;
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
    for (const auto& x : zeroed) LSG_HIP(hipMemsetAsync(x.buf->p, 0, x.bytes, st));
    b.n_cells = n_cells; b.n_muts = n_muts; b.n_words = (int32_t)W; b.n_chains = n_chains; b.steps1 = (int32_t)S1; b.arena_rows = arena_rows;
    b.k_max = 0; b.ll_pitch = 1; b.pending = -1; b.next_step = 0; b.test_ml_end = 0;
    // cfg by name: FN, FP, p, q, DP_a_gamma, the concentration update's probability, the new cluster's two log terms, betaln(p, q)
    const double FN = cfg[0], FP = cfg[1], p = cfg[2], q = cfg[3];
    b.p = p; b.q = q; b.g0 = cfg[4]; b.g1 = cfg[5]; b.dpa_prob = cfg[6]; b.betaln = cfg[9];
    // every chain starts with cfg's rates: the new cluster's log terms as cfg gives them, _beta_mix_const (CRP.py:42-44) and the six
    // values a likelihood term takes under an anchor's data as parameters (:557-560)
    const double m0 = std::tgamma(p) * std::tgamma(q + 1) / std::tgamma(p + q + 1), m1 = std::tgamma(p + 1) * std::tgamma(q) / std::tgamma(p + q + 1);
    b.mix[0] = m0 / (m0 + m1); b.mix[1] = m1 / (m0 + m1);
    Rates r;
    rates_fill(r, FP, FN, b.mix[0], b.mix[1]);
    r.new1 = cfg[7]; r.new0 = cfg[8];
    if (int rc = upload_rates(c, r)) return rc;
    b.sm_prob = 0.0; b.sm_ratio[0] = 0.75; b.sm_ratio[1] = 0.25; b.sm_scans = 3;
    b.err_prob = 0.0; b.learn = b.fixed_assign = false; std::fill(b.err_prior, b.err_prior + 4, 0.0);
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
    for (int32_t s = first_step; s < first_step + n_steps; ++s) {
        if (s > 0 && b.pending != s) {
            if (int rc = step_assign(c, who, (uint32_t)s, !b.fixed_assign, !b.fixed_assign && b.sm_prob > 0)) return rc;
            step_params(c, (uint32_t)s);
            if (b.learn) step_errors(c, (uint32_t)s);
        }
        b.pending = s;
        const bool keep = s >= burn_in;
        if (keep)
            for (int32_t k = 0; k < b.n_chains; ++k)
                if (b.h_used[k] + b.h_k[k] > b.arena_rows) {
                    if (b.h_used[k] == 0) { set_error("%s: step %d has %d clusters, the arena holds %lld rows", who, s, b.h_k[k], (long long)b.arena_rows); return -2; }
                    return sync_check(c, who);                    // full: the caller fetches and goes on at this step
                }
        LSG_HIP(hipMemcpyAsync(b.used.p, b.h_used.data(), (size_t)b.n_chains * 8, hipMemcpyHostToDevice, c->stream));
        hipLaunchKernelGGL(k_bnpcs_record, dim3(b.n_chains), dim3(256), 0, c->stream, dev_of(b), s, keep ? 1 : 0, b.used.as<int64_t>());
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

int lsg_bnpcs_set_split_merge(lsg_ctx* c, double prob, double ratio_split, double ratio_merge, int32_t scans) {
    const char* who = "lsg_bnpcs_set_split_merge";
    if (int rc = need(c, who)) return rc;
    if (!(prob >= 0 && prob <= 1) || !(ratio_split > 0) || !(ratio_merge > 0) || !(std::fabs(ratio_split + ratio_merge - 1) <= 1e-9) || scans < 0 || scans > SM_MAX_SCANS) {
        set_error("%s: the probability must lie in [0, 1], the ratios be positive and sum to 1 and the scans be in [0, %d], got %g, %g, %g and %d", who, SM_MAX_SCANS, prob,
                  ratio_split, ratio_merge, scans);
        return -2;
    }
    Bnpcs& b = c->bnpcs;
    b.sm_prob = prob; b.sm_ratio[0] = ratio_split; b.sm_ratio[1] = ratio_merge; b.sm_scans = scans;
    return 0;
}

int lsg_bnpcs_fetch_moves(lsg_ctx* c, int8_t* moves) {
    const char* who = "lsg_bnpcs_fetch_moves";
    if (int rc = need(c, who)) return rc;
    Bnpcs& b = c->bnpcs;
    if (!moves) { set_error("%s: bad arguments", who); return -2; }
    std::vector<int32_t> codes((size_t)b.n_chains * b.steps1);
    LSG_HIP(hipMemcpyAsync(codes.data(), b.rec_sm.p, codes.size() * 4, hipMemcpyDeviceToHost, c->stream));
    if (sync_check(c, who)) return -1;
    for (size_t k = 0; k < codes.size(); ++k) moves[k] = (int8_t)codes[k];
    return 0;
}

int lsg_bnpcs_set_error_learning(lsg_ctx* c, double prob, double fp_mean, double fp_sd, double fn_mean, double fn_sd) {
    const char* who = "lsg_bnpcs_set_error_learning";
    if (int rc = need(c, who)) return rc;
    const double v[4] = {fp_mean, fp_sd, fn_mean, fn_sd};
    bool ok = prob >= 0 && prob <= 1;
    for (double x : v) ok = ok && x > 0 && x < 1;
    if (!ok) {
        set_error("%s: the probability must lie in [0, 1], the means and the sds inside (0, 1), got %g and FP (%g, %g), FN (%g, %g)", who, prob, fp_mean, fp_sd, fn_mean, fn_sd);
        return -2;
    }
    Bnpcs& b = c->bnpcs;
    Rates r;
    rates_fill(r, fp_mean, fn_mean, b.mix[0], b.mix[1]);
    if (int rc = upload_rates(c, r)) return rc;
    b.err_prob = prob; std::copy(v, v + 4, b.err_prior); b.learn = true; b.prepared = false;
    return 0;
}

int lsg_bnpcs_set_error_rates(lsg_ctx* c, int32_t chain, double fp, double fn) {
    const char* who = "lsg_bnpcs_set_error_rates";
    if (int rc = need(c, who)) return rc;
    Bnpcs& b = c->bnpcs;
    if (chain < 0 || chain >= b.n_chains) { set_error("%s: bad arguments", who); return -2; }
    if (!(fp > 0 && fp < 1 && fn > 0 && fn < 1)) { set_error("%s: the rates must lie inside (0, 1), got FP %g and FN %g", who, fp, fn); return -2; }
    Rates r;
    rates_fill(r, fp, fn, b.mix[0], b.mix[1]);
    LSG_HIP(hipMemcpyAsync(b.rates.as<Rates>() + chain, &r, sizeof(Rates), hipMemcpyHostToDevice, c->stream));
    LSG_HIP(hipStreamSynchronize(c->stream));
    b.prepared = false;
    return 0;
}

int lsg_bnpcs_fetch_error_rates(lsg_ctx* c, double* rates, int32_t* counts) {
    const char* who = "lsg_bnpcs_fetch_error_rates";
    if (int rc = need(c, who)) return rc;
    Bnpcs& b = c->bnpcs;
    if (!rates || !counts) { set_error("%s: bad arguments", who); return -2; }
    LSG_HIP(hipMemcpyAsync(rates, b.rec_err.p, (size_t)b.n_chains * b.steps1 * 2 * 8, hipMemcpyDeviceToHost, c->stream));
    LSG_HIP(hipMemcpyAsync(counts, b.err_cnt.p, (size_t)b.n_chains * 4 * 4, hipMemcpyDeviceToHost, c->stream));
    return sync_check(c, who);
}

int lsg_bnpcs_set_fixed_assignment(lsg_ctx* c, int32_t on) {
    const char* who = "lsg_bnpcs_set_fixed_assignment";
    if (int rc = need(c, who)) return rc;
    c->bnpcs.fixed_assign = on != 0;
    return 0;
}

int lsg_bnpcs_extend(lsg_ctx* c, int32_t add_steps) {
    const char* who = "lsg_bnpcs_extend";
    if (int rc = need(c, who)) return rc;
    Bnpcs& b = c->bnpcs;
    if (add_steps < 1) { set_error("%s: %d steps to add (at least 1)", who, add_steps); return -2; }
    const size_t N = b.n_cells, M = b.n_muts, C = b.n_chains, old1 = b.steps1, S1 = old1 + (size_t)add_steps;
    if (S1 > (size_t)INT32_MAX) { set_error("%s: %zu steps are more than a run can number", who, S1 - 1); return -2; }
    if (int rc = check_state_size(who, "would need", C, N, M, S1, b.arena_rows)) return rc;
    // the four records, each [chain][steps1][words]: new buffers first, so that a refused allocation leaves the run as it was
    DevBuf* rec[4] = {&b.rec_lab, &b.rec_sc, &b.rec_sm, &b.rec_err};
    const size_t words[4] = {N, (size_t)REC * 2, 1, 4};
    DevBuf grown[4];
    for (int k = 0; k < 4; ++k)
        if (grown[k].reserve(C * S1 * words[k] * 4)) { for (DevBuf& g : grown) g.release(); return -1; }
    hipStream_t st = c->stream;
    // a step that waits for room in the arena (pending) has made its move and written its code of rec_sm, though nothing else of its record
    const int32_t made = std::max(std::max(b.next_step, b.pending + 1), b.test_ml_end);
    for (int k = 0; k < 4; ++k) {
        const size_t used = (size_t)made * words[k];
        hipError_t e = hipMemsetAsync(grown[k].p, 0, C * S1 * words[k] * 4, st);
        if (e == hipSuccess && used) {
            const unsigned gx = (unsigned)std::min<size_t>((used + 255) / 256, 4096), gy = (unsigned)std::min<size_t>(C, 65535);
            hipLaunchKernelGGL(k_bnpcs_restride, dim3(gx, gy), dim3(256), 0, st, grown[k].as<uint32_t>(), rec[k]->as<uint32_t>(), old1 * words[k], S1 * words[k], used, (int32_t)C);
            e = hipGetLastError();
        }
        if (e != hipSuccess) {
            (void)hipStreamSynchronize(st);
            for (DevBuf& g : grown) g.release();
            set_error("%s: moving the records failed: %s", who, hipGetErrorString(e));
            return -1;
        }
    }
    if (sync_check(c, who)) { for (DevBuf& g : grown) g.release(); return -1; }
    for (int k = 0; k < 4; ++k) { rec[k]->release(); *rec[k] = grown[k]; }
    b.steps1 = (int32_t)S1;
    return 0;
}

int lsg_bnpcs_psrf(lsg_ctx* c, const int32_t* first, int32_t last, double* stats) {
    const char* who = "lsg_bnpcs_psrf";
    if (int rc = need(c, who)) return rc;
    Bnpcs& b = c->bnpcs;
    if (!first || !stats) { set_error("%s: bad arguments", who); return -2; }
    const int32_t made = std::max(b.next_step, b.test_ml_end);
    if (last < 0 || last > made) { set_error("%s: records up to %d asked, %d are made", who, last, made); return -2; }
    const size_t C = b.n_chains;
    std::vector<int32_t> par(3 * C);
    for (size_t k = 0; k < C; ++k) {
        if (first[k] < 0 || first[k] > last) { set_error("%s: chain %zu: records %d .. %d asked", who, k, first[k], last - 1); return -2; }
        const int32_t bsz = (int32_t)std::pow((double)(last - first[k]), 0.5);      // int(n ** 0.5), as utils.py:439 forms it
        par[3 * k] = first[k]; par[3 * k + 1] = bsz; par[3 * k + 2] = bsz / 3;
    }
    if (b.psrf.reserve(3 * C * 4) || b.psrf_out.reserve(C * 5 * 8)) return -1;
    LSG_HIP(hipMemcpyAsync(b.psrf.p, par.data(), 3 * C * 4, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_bnpcs_psrf, dim3(b.n_chains), dim3(256), 0, c->stream, dev_of(b), b.psrf.as<int32_t>(), last, b.psrf_out.as<double>());
    LSG_HIP(hipMemcpyAsync(stats, b.psrf_out.p, C * 5 * 8, hipMemcpyDeviceToHost, c->stream));
    return sync_check(c, who);                                        // (`par` is read by the copy until here)
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
    if (int rc = launch_ll(c)) return rc;
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
    if (what < 0 || what > 3 || step < 0) { set_error("%s: bad arguments", who); return -2; }
    if (what == 3 && !b.learn) { set_error("%s: no error-rate update (lsg_bnpcs_set_error_learning first)", who); return -2; }
    if (int rc = prepare(c, who)) return rc;
    if (what == 0 || what == 2) { if (int rc = step_assign(c, who, (uint32_t)step, what == 0, what == 2)) return rc; }
    else if (what == 1) step_params(c, (uint32_t)step);
    else step_errors(c, (uint32_t)step);
    return sync_check(c, who);
}

// what a chain's last split-merge move left (SM_OUT doubles), or its last error update (ERR_OUT)
static int fetch_outcome(lsg_ctx* c, const char* who, int32_t chain, bool move, double* outcome) {
    if (int rc = need(c, who)) return rc;
    Bnpcs& b = c->bnpcs;
    if (chain < 0 || chain >= b.n_chains || !outcome) { set_error("%s: bad arguments", who); return -2; }
    const size_t N = b.n_cells, M = b.n_muts;
    const double* src = move ? b.sm_d.as<double>() + chain * sm_d_size(N, M) + sm_d_out(N, M) : b.err_out.as<double>() + (size_t)chain * ERR_OUT;
    LSG_HIP(hipMemcpyAsync(outcome, src, (move ? SM_OUT : ERR_OUT) * 8, hipMemcpyDeviceToHost, c->stream));
    return sync_check(c, who);
}

int lsg_bnpcs_test_move_outcome(lsg_ctx* c, int32_t chain, double* outcome) { return fetch_outcome(c, "lsg_bnpcs_test_move_outcome", chain, true, outcome); }
int lsg_bnpcs_test_error_outcome(lsg_ctx* c, int32_t chain, double* outcome) { return fetch_outcome(c, "lsg_bnpcs_test_error_outcome", chain, false, outcome); }

int lsg_bnpcs_test_set_ml(lsg_ctx* c, int32_t chain, int32_t first, int32_t n, const double* values) {
    const char* who = "lsg_bnpcs_test_set_ml";
    if (int rc = need(c, who)) return rc;
    Bnpcs& b = c->bnpcs;
    if (chain < 0 || chain >= b.n_chains || first < 0 || n < 1 || !values) { set_error("%s: bad arguments", who); return -2; }
    if ((int64_t)first + n > b.steps1) { set_error("%s: records %d .. %lld asked, there is room for %d", who, first, (long long)first + n - 1, b.steps1); return -2; }
    double* dst = b.rec_sc.as<double>() + ((size_t)chain * b.steps1 + first) * REC;
    LSG_HIP(hipMemcpy2DAsync(dst, REC * 8, values, 8, 8, (size_t)n, hipMemcpyHostToDevice, c->stream));
    if (sync_check(c, who)) return -1;
    b.test_ml_end = std::max(b.test_ml_end, first + n);
    return 0;
}
