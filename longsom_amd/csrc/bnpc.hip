// BnpC's posterior estimate (CellClustering/libs/utils.py:90-192) over resident posterior samples: the co-clustering distance of
// every cell pair (get_dist), the three integer sums _calc_MPEAR is made of for many candidate cuts at once, and the mean parameters
// of a final assignment's clusters (get_mean_hierarchy_assignment).  See include/longsom_hip.h, lsg_bnpc_*.
#include "lsg_ctx.h"
#include <algorithm>

namespace lsg {

constexpr int BT = 64;              // cells per tile edge: a workgroup owns the pairs (row tile) x (column tile) of the upper triangle
constexpr int BSC = 64;             // samples per chunk: two strips of BSC x 64 labels (16 KB) in LDS
constexpr int BCUTS = 128;          // candidate cuts scored per launch of k_bnpc_mpear (two strips of 128 x 64 labels: 32 KB of LDS)
constexpr uint32_t BNONE = 0xFFFFu; // no cluster (labels and clusters are < 65535)

__host__ __device__ inline int64_t pair_index(int64_t i, int64_t j, int64_t n) { return i * n - i * (i + 1) / 2 + (j - i - 1); }      // pdist's condensed order, i < j

// int32 labels [S][N] -> 16-bit [S][pitch] (pitch: N rounded up to the tile, the pad 0); bad[0] = the smallest index whose label is outside [0, N)
__global__ void k_bnpc_pack(const int32_t* __restrict__ src, int64_t n_samples, int32_t n_cells, int32_t pitch, uint16_t* __restrict__ dst, unsigned long long* bad) {
    const int64_t total = n_samples * (int64_t)pitch;
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < total; k += (int64_t)gridDim.x * blockDim.x) {
        const int64_t s = k / pitch; const int32_t i = (int32_t)(k - s * pitch);
        uint16_t v = 0;
        if (i < n_cells) {
            const int32_t l = src[s * n_cells + i];
            if (l < 0 || l >= n_cells) atomicMin(bad, (unsigned long long)(s * n_cells + i)); else v = (uint16_t)l;
        }
        dst[k] = v;
    }
}

// rows [n][64] of a 16-bit array with row pitch `pitch`, columns tile*64 .. +63, into an LDS strip: 16 bytes per thread and turn
__device__ inline void load_strip(uint16_t* strip, const uint16_t* __restrict__ lab, int64_t row0, int n, int32_t pitch, int tile) {
    for (int k = threadIdx.x; k < n * 8; k += 256) {
        const int r = k >> 3, q = k & 7;
        reinterpret_cast<uint4*>(strip)[k] = *reinterpret_cast<const uint4*>(lab + (row0 + r) * pitch + tile * BT + q * 8);
    }
}

// D[pair] = number of samples in which the pair's two labels differ.  One workgroup (256 threads) per 64 x 64 tile with column tile >=
// row tile; thread (ty, tx) counts the 4 x 4 pairs rows 4 ty .. +3 by columns 4 tx .. +3 in registers: per sample two 8-byte LDS reads
// (the row one a broadcast over 16 lanes) and 16 compare-and-adds.  The tile is written once, pairs with i >= j or a cell >= N left out.
__global__ __launch_bounds__(256) void k_bnpc_codist(const uint16_t* __restrict__ lab, int64_t n_samples, int32_t n_cells, int32_t pitch, uint32_t* __restrict__ dist) {
    const int bi = blockIdx.y, bj = blockIdx.x;
    if (bj < bi) return;
    __shared__ __attribute__((aligned(16))) uint16_t sa[BSC * BT];
    __shared__ __attribute__((aligned(16))) uint16_t sb[BSC * BT];
    const int ty = threadIdx.x >> 4, tx = threadIdx.x & 15;
    uint32_t cnt[4][4] = {};
    for (int64_t s0 = 0; s0 < n_samples; s0 += BSC) {
        const int ns = (int)(n_samples - s0 < BSC ? n_samples - s0 : BSC);
        __syncthreads();
        load_strip(sa, lab, s0, ns, pitch, bi);
        load_strip(sb, lab, s0, ns, pitch, bj);
        __syncthreads();
#pragma unroll 4
        for (int s = 0; s < ns; ++s) {
            const uint2 a = *reinterpret_cast<const uint2*>(sa + s * BT + ty * 4);
            const uint2 b = *reinterpret_cast<const uint2*>(sb + s * BT + tx * 4);
            const uint32_t av[4] = {a.x & 0xFFFFu, a.x >> 16, a.y & 0xFFFFu, a.y >> 16};
            const uint32_t bv[4] = {b.x & 0xFFFFu, b.x >> 16, b.y & 0xFFFFu, b.y >> 16};
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int c = 0; c < 4; ++c) cnt[r][c] += (av[r] != bv[c]) ? 1u : 0u;
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int64_t i = (int64_t)bi * BT + ty * 4 + r;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int64_t j = (int64_t)bj * BT + tx * 4 + c;
            if (i < j && j < n_cells) dist[pair_index(i, j, n_cells)] = cnt[r][c];
        }
    }
}

__device__ inline unsigned long long wave_sum(unsigned long long v) {
    for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d, 64);
    return v;
}

// One pass over the tile's 4 x 4 pairs per thread for n_cuts (<= BCUTS) candidate cuts: out[2 k] += pairs whose two labels of cut k are
// equal, out[2 k + 1] += the sum of (S - D) over them; *dsum += the sum of D (only where dsum is given: once per scoring).  Exact
// integers: a wave's sums meet in LDS, a workgroup's in one 64-bit atomic per cut.
__global__ __launch_bounds__(256) void k_bnpc_mpear(const uint32_t* __restrict__ dist, const uint16_t* __restrict__ cuts, int n_cuts, int64_t n_samples, int32_t n_cells,
                                                    int32_t pitch, unsigned long long* out, unsigned long long* dsum) {
    const int bi = blockIdx.y, bj = blockIdx.x;
    if (bj < bi) return;
    __shared__ __attribute__((aligned(16))) uint16_t sa[BCUTS * BT];
    __shared__ __attribute__((aligned(16))) uint16_t sb[BCUTS * BT];
    __shared__ unsigned long long acc[2 * BCUTS + 1];
    for (int k = threadIdx.x; k < 2 * BCUTS + 1; k += 256) acc[k] = 0;
    load_strip(sa, cuts, 0, n_cuts, pitch, bi);
    load_strip(sb, cuts, 0, n_cuts, pitch, bj);
    const int ty = threadIdx.x >> 4, tx = threadIdx.x & 15, lane = threadIdx.x & 63;
    uint32_t sim[4][4]; bool live[4][4];
    unsigned long long dsum_t = 0;
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int64_t i = (int64_t)bi * BT + ty * 4 + r, j = (int64_t)bj * BT + tx * 4 + c;
            live[r][c] = i < j && j < n_cells;
            const uint32_t d = live[r][c] ? dist[pair_index(i, j, n_cells)] : 0u;
            sim[r][c] = (uint32_t)n_samples - d;
            dsum_t += d;
        }
    __syncthreads();
    if (dsum) { dsum_t = wave_sum(dsum_t); if (lane == 0) atomicAdd(&acc[2 * BCUTS], dsum_t); }
    for (int k = 0; k < n_cuts; ++k) {
        const uint2 a = *reinterpret_cast<const uint2*>(sa + k * BT + ty * 4);
        const uint2 b = *reinterpret_cast<const uint2*>(sb + k * BT + tx * 4);
        const uint32_t av[4] = {a.x & 0xFFFFu, a.x >> 16, a.y & 0xFFFFu, a.y >> 16};
        const uint32_t bv[4] = {b.x & 0xFFFFu, b.x >> 16, b.y & 0xFFFFu, b.y >> 16};
        unsigned long long np = 0, ss = 0;
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (live[r][c] && av[r] == bv[c]) { np += 1; ss += sim[r][c]; }
        np = wave_sum(np); ss = wave_sum(ss);
        if (lane == 0) { atomicAdd(&acc[2 * k], np); atomicAdd(&acc[2 * k + 1], ss); }
    }
    __syncthreads();
    for (int k = threadIdx.x; k < 2 * n_cuts; k += 256)
        if (acc[k]) atomicAdd(&out[k], acc[k]);
    if (dsum && threadIdx.x == 0 && acc[2 * BCUTS]) atomicAdd(dsum, acc[2 * BCUTS]);
}

// Per sample (a workgroup takes samples blockIdx.x, + gridDim.x, ...), against a final assignment given as cluster[cell] and first[c] (the
// first cell of cluster c):
//   rank[s][i]   the number of distinct labels of sample s smaller than cell i's: its row in the sample's parameters
//   flags[c][s]  bit 0 "same": every cell of c carries the label F of c's first cell; bit 1 "no others": no cell outside c carries F
// owner[F] = a cluster whose first cell carries F (any of them), per workgroup in global scratch.  A cell of cluster c with label L whose
// owner o is another cluster has F_o = L outside o: o has others; and if L = F_c as well, o's first cell carries F_c outside c: c has others.
__global__ __launch_bounds__(256) void k_bnpc_criteria(const uint16_t* __restrict__ lab, int64_t n_samples, int32_t n_cells, int32_t pitch, const uint16_t* __restrict__ cluster,
                                                       const int32_t* __restrict__ first, int32_t n_clusters, uint16_t* __restrict__ owner_all, uint16_t* __restrict__ rank,
                                                       uint8_t* __restrict__ flags) {
    __shared__ uint32_t present[2048], notsame[2048], others[2048], pre[2048], part[256];
    uint16_t* owner = owner_all + (size_t)blockIdx.x * pitch;
    for (int64_t s = blockIdx.x; s < n_samples; s += gridDim.x) {
        const uint16_t* row = lab + s * pitch;
        __syncthreads();
        for (int w = threadIdx.x; w < 2048; w += 256) { present[w] = 0; notsame[w] = 0; others[w] = 0; }
        for (int l = threadIdx.x; l < n_cells; l += 256) owner[l] = (uint16_t)BNONE;
        __syncthreads();
        for (int c = threadIdx.x; c < n_clusters; c += 256) owner[row[first[c]]] = (uint16_t)c;
        __syncthreads();
        for (int i = threadIdx.x; i < n_cells; i += 256) {
            const uint32_t l = row[i], c = cluster[i], f = row[first[c]], o = owner[l];
            atomicOr(&present[l >> 5], 1u << (l & 31));
            if (l != f) atomicOr(&notsame[c >> 5], 1u << (c & 31));
            if (o != BNONE && o != c) {
                atomicOr(&others[o >> 5], 1u << (o & 31));
                if (l == f) atomicOr(&others[c >> 5], 1u << (c & 31));
            }
        }
        __syncthreads();
        uint32_t sum = 0;
        for (int k = 0; k < 8; ++k) sum += __popc(present[threadIdx.x * 8 + k]);
        part[threadIdx.x] = sum;
        __syncthreads();
        if (threadIdx.x == 0) { uint32_t run = 0; for (int t = 0; t < 256; ++t) { const uint32_t v = part[t]; part[t] = run; run += v; } }
        __syncthreads();
        sum = part[threadIdx.x];
        for (int k = 0; k < 8; ++k) { pre[threadIdx.x * 8 + k] = sum; sum += __popc(present[threadIdx.x * 8 + k]); }
        __syncthreads();
        for (int i = threadIdx.x; i < n_cells; i += 256) {
            const uint32_t l = row[i];
            rank[s * pitch + i] = (uint16_t)(pre[l >> 5] + __popc(present[l >> 5] & ((1u << (l & 31)) - 1u)));
        }
        for (int c = threadIdx.x; c < n_clusters; c += 256) {
            const bool same = !((notsame[c >> 5] >> (c & 31)) & 1u), alone = !((others[c >> 5] >> (c & 31)) & 1u);
            flags[(size_t)c * n_samples + s] = (uint8_t)((same ? 1 : 0) | (same && alone ? 2 : 0));
        }
    }
}

// per cluster: samples with both criteria, samples with the first -> branch (0 both, 1 first only, 2 neither, 3 a one-cell cluster), n_used and the flag bits a used sample carries
__global__ __launch_bounds__(256) void k_bnpc_branch(const uint8_t* __restrict__ flags, int64_t n_samples, const int32_t* __restrict__ csize, uint8_t* __restrict__ branch,
                                                     uint8_t* __restrict__ picks, int32_t* __restrict__ n_used) {
    __shared__ unsigned long long acc[2];
    const int c = blockIdx.x;
    if (threadIdx.x < 2) acc[threadIdx.x] = 0;
    __syncthreads();
    unsigned long long both = 0, same = 0;
    for (int64_t s = threadIdx.x; s < n_samples; s += 256) { const uint8_t f = flags[(size_t)c * n_samples + s]; same += f & 1; both += (f >> 1) & 1; }
    both = wave_sum(both); same = wave_sum(same);
    if ((threadIdx.x & 63) == 0) { atomicAdd(&acc[0], both); atomicAdd(&acc[1], same); }
    __syncthreads();
    if (threadIdx.x == 0) {
        const int b = acc[0] ? 0 : acc[1] ? 1 : 2;
        n_used[c] = (int32_t)(acc[0] ? acc[0] : acc[1] ? acc[1] : (unsigned long long)n_samples);
        branch[c] = (uint8_t)(csize[c] == 1 ? 3 : b);
        picks[c] = (uint8_t)(acc[0] ? 3 : 1);
    }
}

// A lane per (cluster, mutation).  Branches 0 / 1 / 3 (blockIdx.z = 0 alone): the selected samples' rows params[s][rank of the cluster's
// label] added as doubles in ascending sample order, then one division: numpy's += loop (utils.py:177-181) bit for bit.  Branch 2: every
// sample, every cell of the cluster (cells[coff[c] .. coff[c + 1])) (:184-189); its samples are split over blockIdx.z, the partial sums
// go to part[ordinal of c among the branch-2 clusters][z][m] and k_bnpc_mean_finish adds them in the order of z.
__global__ __launch_bounds__(64) void k_bnpc_mean(const float* __restrict__ params, int32_t k_max, int32_t n_muts, const uint16_t* __restrict__ rank, const uint8_t* __restrict__ flags,
                                                  int64_t n_samples, int32_t pitch, const int32_t* __restrict__ first, const int32_t* __restrict__ cells, const int32_t* __restrict__ coff,
                                                  const uint8_t* __restrict__ branch, const uint8_t* __restrict__ picks, const int32_t* __restrict__ n_used, const int32_t* __restrict__ ord2,
                                                  double* __restrict__ part, double* __restrict__ out, int32_t* __restrict__ bad_rank) {
    const int c = blockIdx.y, m = blockIdx.x * 64 + threadIdx.x, z = blockIdx.z, n_split = gridDim.z;
    if (m >= n_muts) return;
    const int b = branch[c];
    double acc = 0.0;
    if (b != 2) {
        if (z) return;
        const uint8_t pick = picks[c];                             // the flag bits a sample needs: both criteria when some sample has both, else the first
        const int32_t f = first[c];
        for (int64_t s = 0; s < n_samples; ++s) {
            if ((flags[(size_t)c * n_samples + s] & pick) != pick) continue;
            const int32_t r = rank[s * pitch + f];
            if (r >= k_max) { *bad_rank = 1; continue; }
            acc += (double)params[((size_t)s * k_max + r) * n_muts + m];
        }
        out[(size_t)c * n_muts + m] = acc / (double)n_used[c];
    } else {
        const int64_t per = (n_samples + n_split - 1) / n_split, s0 = z * per, s1 = s0 + per < n_samples ? s0 + per : n_samples;
        const int32_t i0 = coff[c], i1 = coff[c + 1];
        for (int64_t s = s0; s < s1; ++s)
            for (int32_t k = i0; k < i1; ++k) {
                const int32_t r = rank[s * pitch + cells[k]];
                if (r >= k_max) { *bad_rank = 1; continue; }
                acc += (double)params[((size_t)s * k_max + r) * n_muts + m];
            }
        part[((size_t)ord2[c] * n_split + z) * n_muts + m] = acc;
    }
}

__global__ __launch_bounds__(64) void k_bnpc_mean_finish(const uint8_t* __restrict__ branch, const int32_t* __restrict__ ord2, const double* __restrict__ part, int n_split, int32_t n_muts,
                                                         int64_t n_samples, const int32_t* __restrict__ coff, double* __restrict__ out) {
    const int c = blockIdx.y, m = blockIdx.x * 64 + threadIdx.x;
    if (m >= n_muts || branch[c] != 2) return;
    double acc = 0.0;
    for (int z = 0; z < n_split; ++z) acc += part[((size_t)ord2[c] * n_split + z) * n_muts + m];
    out[(size_t)c * n_muts + m] = acc / (double)(n_samples * (int64_t)(coff[c + 1] - coff[c]));
}

static int sync_check(lsg_ctx* c, const char* who) {
    hipError_t e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = hipGetLastError();
    if (e != hipSuccess) { set_error("%s: kernel failed: %s", who, hipGetErrorString(e)); return -1; }
    return 0;
}

int run_bnpc_load(lsg_ctx* c, int64_t n_samples, int32_t n_cells, const int32_t* assign, int32_t k_max, int32_t n_muts, const float* params) {
    const char* who = "lsg_bnpc_load_samples";
    Bnpc& b = c->bnpc;
    b.valid = b.dist_valid = b.tree_valid = false;
    if (n_cells < 2 || n_cells > 65535) { set_error("%s: %d cells (2 .. 65535)", who, n_cells); return -2; }
    if (n_samples < 1 || n_samples > 0xFFFFFFFFll) { set_error("%s: %lld samples (at least 1)", who, (long long)n_samples); return -2; }
    if (!assign) { set_error("%s: assign is NULL", who); return -2; }
    if (params && (k_max < 1 || n_muts < 1)) { set_error("%s: params of %d clusters x %d mutations", who, k_max, n_muts); return -2; }
    const int32_t pitch = (n_cells + BT - 1) / BT * BT;
    const size_t n_lab = (size_t)n_samples * n_cells;
    hipStream_t st = c->stream;
    if (b.lab.reserve((size_t)n_samples * pitch * 2) || b.raw.reserve(n_lab * 4) || b.small.reserve(64)) return -1;
    unsigned long long* bad = b.small.as<unsigned long long>();
    LSG_HIP(hipMemsetAsync(bad, 0xFF, 8, st));
    LSG_HIP(hipMemcpyAsync(b.raw.p, assign, n_lab * 4, hipMemcpyHostToDevice, st));
    const int64_t total = n_samples * (int64_t)pitch;
    unsigned blocks = (unsigned)std::min<int64_t>((total + 255) / 256, (int64_t)c->n_cus * 32);
    hipLaunchKernelGGL(k_bnpc_pack, dim3(blocks), dim3(256), 0, st, b.raw.as<int32_t>(), n_samples, n_cells, pitch, b.lab.as<uint16_t>(), bad);
    unsigned long long h_bad = 0;
    LSG_HIP(hipMemcpyAsync(&h_bad, bad, 8, hipMemcpyDeviceToHost, st));
    if (sync_check(c, who)) return -1;
    b.raw.release();
    if (h_bad != ~0ull) {
        set_error("%s: assign[%lld, %lld] = %d is not a label in [0, %d)", who, (long long)(h_bad / n_cells), (long long)(h_bad % n_cells), assign[h_bad], n_cells);
        return -2;
    }
    b.has_params = params != nullptr;
    if (params) {
        const size_t bytes = (size_t)n_samples * k_max * n_muts * 4;
        if (b.params.reserve(bytes)) return -1;
        LSG_HIP(hipMemcpyAsync(b.params.p, params, bytes, hipMemcpyHostToDevice, st));
        LSG_HIP(hipStreamSynchronize(st));
    } else b.params.release();
    b.n_samples = n_samples; b.n_cells = n_cells; b.pitch = pitch; b.k_max = params ? k_max : 0; b.n_muts = params ? n_muts : 0;
    b.valid = true;
    return 0;
}

int run_bnpc_codist(lsg_ctx* c) {
    const char* who = "lsg_bnpc_codist";
    Bnpc& b = c->bnpc;
    if (!b.valid) { set_error("%s: no samples resident (lsg_bnpc_load_samples first)", who); return -2; }
    b.tree_valid = false;
    const int64_t pairs = (int64_t)b.n_cells * (b.n_cells - 1) / 2;
    if (b.dist.reserve((size_t)pairs * 4)) return -1;
    const unsigned t = (unsigned)(b.pitch / BT);
    hipLaunchKernelGGL(k_bnpc_codist, dim3(t, t), dim3(256), 0, c->stream, b.lab.as<uint16_t>(), b.n_samples, b.n_cells, b.pitch, b.dist.as<uint32_t>());
    if (sync_check(c, who)) return -1;
    b.dist_valid = true;
    return 0;
}

int run_bnpc_fetch_dist(lsg_ctx* c, uint32_t* out, int64_t capacity) {
    const char* who = "lsg_bnpc_fetch_dist";
    Bnpc& b = c->bnpc;
    if (!b.valid || !b.dist_valid) { set_error("%s: no distances resident (lsg_bnpc_codist first)", who); return -2; }
    const int64_t pairs = (int64_t)b.n_cells * (b.n_cells - 1) / 2;
    if (!out || capacity < pairs) { set_error("%s: room for %lld of %lld pairs", who, (long long)capacity, (long long)pairs); return -2; }
    LSG_HIP(hipMemcpyAsync(out, b.dist.p, (size_t)pairs * 4, hipMemcpyDeviceToHost, c->stream));
    LSG_HIP(hipStreamSynchronize(c->stream));
    return 0;
}

// a host label array [rows][n_cells] with every value in [0, n_cells) -> 16-bit rows of the tile pitch on the device
static int put_labels16(lsg_ctx* c, const char* who, const char* what, DevBuf& buf, const int32_t* src, int64_t rows, int32_t n_cells, int32_t pitch) {
    std::vector<uint16_t> h((size_t)rows * pitch, 0);
    for (int64_t r = 0; r < rows; ++r)
        for (int32_t i = 0; i < n_cells; ++i) {
            const int32_t l = src[r * n_cells + i];
            if (l < 0 || l >= n_cells) { set_error("%s: %s[%lld, %d] = %d is not in [0, %d)", who, what, (long long)r, i, l, n_cells); return -2; }
            h[(size_t)r * pitch + i] = (uint16_t)l;
        }
    if (h.empty()) return 0;
    if (buf.reserve(h.size() * 2)) return -1;
    LSG_HIP(hipMemcpyAsync(buf.p, h.data(), h.size() * 2, hipMemcpyHostToDevice, c->stream));
    LSG_HIP(hipStreamSynchronize(c->stream));      // (h leaves scope)
    return 0;
}

int run_bnpc_mpear(lsg_ctx* c, int32_t n_cuts, const int32_t* labels, uint64_t* same_pairs, uint64_t* same_sim, uint64_t* dist_sum) {
    const char* who = "lsg_bnpc_mpear";
    Bnpc& b = c->bnpc;
    if (!b.valid || !b.dist_valid) { set_error("%s: no distances resident (lsg_bnpc_load_samples and lsg_bnpc_codist first)", who); return -2; }
    if (n_cuts < 0 || (n_cuts > 0 && (!labels || !same_pairs || !same_sim))) { set_error("%s: bad arguments", who); return -2; }
    if (int rc = put_labels16(c, who, "labels", b.cuts, labels, n_cuts, b.n_cells, b.pitch)) return rc;
    const size_t words = (size_t)2 * n_cuts + 1;
    if (b.sums.reserve(words * 8)) return -1;
    unsigned long long* sums = b.sums.as<unsigned long long>();
    LSG_HIP(hipMemsetAsync(sums, 0, words * 8, c->stream));
    const unsigned t = (unsigned)(b.pitch / BT);
    for (int32_t k0 = 0; k0 < n_cuts || k0 == 0; k0 += BCUTS) {                        // (no cut at all: dist_sum alone)
        const int n = std::min(BCUTS, n_cuts - k0);
        hipLaunchKernelGGL(k_bnpc_mpear, dim3(t, t), dim3(256), 0, c->stream, b.dist.as<uint32_t>(), b.cuts.as<uint16_t>() + (size_t)k0 * b.pitch, n, b.n_samples, b.n_cells, b.pitch,
                           sums + 2 * (size_t)k0, k0 == 0 ? sums + 2 * (size_t)n_cuts : nullptr);
    }
    std::vector<unsigned long long> h(words);
    LSG_HIP(hipMemcpyAsync(h.data(), sums, words * 8, hipMemcpyDeviceToHost, c->stream));
    if (sync_check(c, who)) return -1;
    for (int32_t k = 0; k < n_cuts; ++k) { same_pairs[k] = h[2 * (size_t)k]; same_sim[k] = h[2 * (size_t)k + 1]; }
    if (dist_sum) *dist_sum = h[2 * (size_t)n_cuts];
    return 0;
}

int run_bnpc_mean_params(lsg_ctx* c, const int32_t* final_assign, int32_t n_clusters, double* params, uint8_t* branch, int32_t* n_used) {
    const char* who = "lsg_bnpc_mean_params";
    Bnpc& b = c->bnpc;
    if (!b.valid) { set_error("%s: no samples resident (lsg_bnpc_load_samples first)", who); return -2; }
    if (!b.has_params) { set_error("%s: the samples were loaded without parameters", who); return -2; }
    if (!final_assign || !params) { set_error("%s: bad arguments", who); return -2; }
    const int32_t n = b.n_cells;
    // clusters: the distinct values of final_assign, ascending; cells grouped by cluster in cell order
    std::vector<int32_t> vals(final_assign, final_assign + n);
    std::sort(vals.begin(), vals.end());
    vals.erase(std::unique(vals.begin(), vals.end()), vals.end());
    if ((int32_t)vals.size() != n_clusters) { set_error("%s: final_assign has %d distinct values, n_clusters is %d", who, (int)vals.size(), n_clusters); return -2; }
    std::vector<uint16_t> cluster(n);
    std::vector<int32_t> coff(n_clusters + 1, 0), cells(n), first(n_clusters, -1), csize(n_clusters, 0);
    for (int32_t i = 0; i < n; ++i) {
        const int32_t k = (int32_t)(std::lower_bound(vals.begin(), vals.end(), final_assign[i]) - vals.begin());
        cluster[i] = (uint16_t)k; ++csize[k];
        if (first[k] < 0) first[k] = i;
    }
    for (int32_t k = 0; k < n_clusters; ++k) coff[k + 1] = coff[k] + csize[k];
    { std::vector<int32_t> at(coff.begin(), coff.end() - 1); for (int32_t i = 0; i < n; ++i) cells[at[cluster[i]]++] = i; }

    const unsigned blocks = (unsigned)std::min<int64_t>(b.n_samples, (int64_t)c->n_cus * 4);
    const size_t host_words = (size_t)n + 3 * (size_t)n_clusters + 1;                       // cells, first, csize, coff as int32
    if (b.rank.reserve((size_t)b.n_samples * b.pitch * 2) || b.flags.reserve((size_t)n_clusters * b.n_samples) || b.owner.reserve((size_t)blocks * b.pitch * 2) ||
        b.cl16.reserve((size_t)n * 2) || b.idx.reserve(host_words * 4) || b.mean.reserve((size_t)n_clusters * b.n_muts * 8) || b.small.reserve(64 + (size_t)n_clusters * 6 + 8)) return -1;
    hipStream_t st = c->stream;
    int32_t* d_cells = b.idx.as<int32_t>(); int32_t* d_first = d_cells + n; int32_t* d_csize = d_first + n_clusters; int32_t* d_coff = d_csize + n_clusters;
    int32_t* d_bad = b.small.as<int32_t>(); int32_t* d_used = d_bad + 16; uint8_t* d_branch = reinterpret_cast<uint8_t*>(d_used + n_clusters);
    LSG_HIP(hipMemcpyAsync(b.cl16.p, cluster.data(), (size_t)n * 2, hipMemcpyHostToDevice, st));
    LSG_HIP(hipMemcpyAsync(d_cells, cells.data(), (size_t)n * 4, hipMemcpyHostToDevice, st));
    LSG_HIP(hipMemcpyAsync(d_first, first.data(), (size_t)n_clusters * 4, hipMemcpyHostToDevice, st));
    LSG_HIP(hipMemcpyAsync(d_csize, csize.data(), (size_t)n_clusters * 4, hipMemcpyHostToDevice, st));
    LSG_HIP(hipMemcpyAsync(d_coff, coff.data(), (size_t)(n_clusters + 1) * 4, hipMemcpyHostToDevice, st));
    LSG_HIP(hipMemsetAsync(d_bad, 0, 4, st));
    hipLaunchKernelGGL(k_bnpc_criteria, dim3(blocks), dim3(256), 0, st, b.lab.as<uint16_t>(), b.n_samples, n, b.pitch, b.cl16.as<uint16_t>(), d_first, n_clusters, b.owner.as<uint16_t>(),
                       b.rank.as<uint16_t>(), b.flags.as<uint8_t>());
    hipLaunchKernelGGL(k_bnpc_branch, dim3((unsigned)n_clusters), dim3(256), 0, st, b.flags.as<uint8_t>(), b.n_samples, d_csize, d_branch, d_branch + n_clusters, d_used);
    // which clusters take the branch-2 path: they get a slot for their partial sums
    std::vector<int32_t> h_used(n_clusters), ord2(n_clusters, 0); std::vector<uint8_t> h_branch(n_clusters);
    LSG_HIP(hipMemcpyAsync(h_branch.data(), d_branch, (size_t)n_clusters, hipMemcpyDeviceToHost, st));
    if (sync_check(c, who)) return -1;
    int32_t n2 = 0;
    for (int32_t k = 0; k < n_clusters; ++k) if (h_branch[k] == 2) ord2[k] = n2++;
    const int n_split = n2 ? (int)std::min<int64_t>(b.n_samples, 64) : 1;
    if (b.part.reserve((size_t)std::max(n2, 1) * n_split * b.n_muts * 8) || b.ord2.reserve((size_t)n_clusters * 4)) return -1;
    LSG_HIP(hipMemcpyAsync(b.ord2.p, ord2.data(), (size_t)n_clusters * 4, hipMemcpyHostToDevice, st));
    const dim3 grid((unsigned)((b.n_muts + 63) / 64), (unsigned)n_clusters, (unsigned)n_split);
    hipLaunchKernelGGL(k_bnpc_mean, grid, dim3(64), 0, st, b.params.as<float>(), b.k_max, b.n_muts, b.rank.as<uint16_t>(), b.flags.as<uint8_t>(), b.n_samples, b.pitch, d_first, d_cells,
                       d_coff, d_branch, d_branch + n_clusters, d_used, b.ord2.as<int32_t>(), b.part.as<double>(), b.mean.as<double>(), d_bad);
    if (n2)
        hipLaunchKernelGGL(k_bnpc_mean_finish, dim3(grid.x, grid.y), dim3(64), 0, st, d_branch, b.ord2.as<int32_t>(), b.part.as<double>(), n_split, b.n_muts, b.n_samples, d_coff,
                           b.mean.as<double>());
    int32_t h_bad = 0;
    LSG_HIP(hipMemcpyAsync(&h_bad, d_bad, 4, hipMemcpyDeviceToHost, st));
    LSG_HIP(hipMemcpyAsync(h_used.data(), d_used, (size_t)n_clusters * 4, hipMemcpyDeviceToHost, st));
    LSG_HIP(hipMemcpyAsync(params, b.mean.p, (size_t)n_clusters * b.n_muts * 8, hipMemcpyDeviceToHost, st));
    if (sync_check(c, who)) return -1;
    if (h_bad) { set_error("%s: a sample has more distinct labels than the %d parameter rows loaded", who, b.k_max); return -2; }
    if (branch) std::copy(h_branch.begin(), h_branch.end(), branch);
    if (n_used) std::copy(h_used.begin(), h_used.end(), n_used);
    return 0;
}

int run_bnpc_unload(lsg_ctx* c) { c->bnpc.release(); return 0; }

} // namespace lsg
