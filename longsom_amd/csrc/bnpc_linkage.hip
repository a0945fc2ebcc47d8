// The ward tree of BnpC's posterior estimate over the resident pair distances (scipy's linkage(y, "ward"): the nearest-neighbour chain),
// the labels of its cuts (scipy's cut_tree) and the cluster count that sets the cut range (utils.py:106-111).  See include/longsom_hip.h,
// lsg_bnpc_linkage / _cut_tree / _cluster_counts; longsom_amd/bnpc.py's ward_linkage_host and cut_tree_host are the numpy twins.
#include "lsg_ctx.h"
#include <algorithm>
#include <climits>
#include <cmath>
#include <numeric>

namespace lsg {

constexpr int WT = 1024;            // threads of the one workgroup that walks the chain: lane t owns the cells t, t + 1024, ...
constexpr int WW = WT / 64;         // its waves
constexpr int LIVE_WORDS = 2048;    // a bit per cell (n_cells <= 65535) in LDS: the clusters still alive
constexpr int CC_WORDS = 4096;      // two bits per label value (< 65536) in LDS: k_bnpc_cluster_counts' saturating counters

// The working copy: W[i][j] = double(D[pair]) / double(S) (the bits of numpy's uint32 / int), square so that a scan reads one contiguous row
__global__ __launch_bounds__(256) void k_bnpc_ward_fill(const uint32_t* __restrict__ dist, int64_t n_samples, int32_t n_cells, double* __restrict__ W) {
    const int64_t n = n_cells, total = n * n;
    const double s = (double)n_samples;
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < total; k += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = k / n, c = k - r * n, i = r < c ? r : c, j = r < c ? c : r;
        W[k] = i == j ? 0.0 : (double)dist[i * n - i * (i + 1) / 2 + (j - i - 1)] / s;
    }
}

__device__ inline bool lower(double v, int i, double bv, int bi) { return v < bv || (v == bv && i < bi); }

// scipy's nn_chain for method "ward", the whole walk in one workgroup.  What is parallel is a scan (the nearest live neighbour of the
// chain's top x: every lane the strict minimum over its ascending cells of row x, then the minimum of (value, cell) over the lanes, then
// the element below the top wins on <=) and an update (row and column y of W by the ward formula, evaluated left to right without
// contraction: the reference's bits).  Every thread carries the chain's top, the element below it and its length in registers; thread 0
// keeps the chain in memory for the pops.  One barrier per scan (the lanes' minima alternate between two LDS buffers), one per merge; the
// loop makes at most 3 (n - 1) scans (each pushes, at most 2 (n - 1) times since a merge pops two, or merges) and never waits on anything.
// No pointer is __restrict__: the threads talk through W, size and chain, across the barriers.
// rec[k] = (x, y, height, size x + size y) of merge k in the chain's order; *err: 0, 1 the scan bound was reached, 2 a scan found no cell
__global__ __launch_bounds__(WT) void k_bnpc_ward(double* W, int32_t n, int32_t* size, int32_t* chain, double* rec, int32_t* err) {
#pragma clang fp contract(off)
    __shared__ uint32_t live[LIVE_WORDS];
    __shared__ double part_v[2][WW];
    __shared__ int part_i[2][WW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int w = tid; w < LIVE_WORDS; w += WT) {
        const int lo = w * 32;
        live[w] = lo + 32 <= n ? ~0u : lo < n ? (1u << (n - lo)) - 1u : 0u;
    }
    for (int i = tid; i < n; i += WT) size[i] = 1;
    __syncthreads();
    int len = 0, lowest = 0, x = 0, below = -1, merges = 0, status = 0;
    const int64_t max_scans = 3 * (int64_t)(n - 1);
    for (int64_t scan = 0; scan < max_scans && merges < n - 1; ++scan) {
        if (len == 0) {                                                           // the lowest live cell: it only ever moves up
            while (lowest < n && !((live[lowest >> 5] >> (lowest & 31)) & 1u)) ++lowest;
            if (lowest >= n) { status = 2; break; }
            x = lowest; below = -1; len = 1;
            if (tid == 0) chain[0] = x;
        }
        const double* row = W + (size_t)x * n;
        double bv = INFINITY; int bi = INT_MAX;
        for (int i = tid; i < n; i += WT) {
            if (i == x || !((live[i >> 5] >> (i & 31)) & 1u)) continue;
            const double v = row[i];
            if (v < bv) { bv = v; bi = i; }
        }
        const double dbelow = below >= 0 ? row[below] : 0.0;
        for (int d = 32; d > 0; d >>= 1) {
            const double ov = __shfl_down(bv, d, 64); const int oi = __shfl_down(bi, d, 64);
            if (lower(ov, oi, bv, bi)) { bv = ov; bi = oi; }
        }
        const int buf = (int)(scan & 1);
        if (lane == 0) { part_v[buf][wave] = bv; part_i[buf][wave] = bi; }
        __syncthreads();
        bv = part_v[buf][0]; bi = part_i[buf][0];
        for (int w = 1; w < WW; ++w)
            if (lower(part_v[buf][w], part_i[buf][w], bv, bi)) { bv = part_v[buf][w]; bi = part_i[buf][w]; }
        int y = bi; double cur = bv;
        if (below >= 0 && dbelow <= bv) { y = below; cur = dbelow; }
        if (y == INT_MAX) { status = 2; break; }
        if (y != below) {                                                         // not mutual yet: the chain grows
            if (len >= n) { status = 2; break; }
            if (tid == 0) chain[len] = y;
            below = x; x = y; ++len;
            continue;
        }
        const int a = x < y ? x : y, b = x < y ? y : x;                           // a ends here, b carries the union
        const int na = size[a], nb = size[b];
        const double* ra = W + (size_t)a * n; double* rb = W + (size_t)b * n;
        for (int i = tid; i < n; i += WT) {
            if (i == a || i == b) continue;
            const int ni = size[i];
            if (ni == 0) continue;
            const double t = 1.0 / (double)(na + nb + ni);
            const double da = ra[i], db = rb[i];
            const double v = __dsqrt_rn((double)(ni + na) * t * da * da + (double)(ni + nb) * t * db * db - (double)ni * t * cur * cur);
            rb[i] = v;
            W[(size_t)i * n + b] = v;
        }
        if (tid == 0) {
            live[a >> 5] &= ~(1u << (a & 31));
            double* r = rec + 4 * (size_t)merges;
            r[0] = (double)a; r[1] = (double)b; r[2] = cur; r[3] = (double)(na + nb);
        }
        __syncthreads();
        if (tid == 0) { size[a] = 0; size[b] = na + nb; }                        // (read next by an update, behind the next scan's barrier)
        ++merges; len -= 2;
        if (len >= 1) { x = chain[len - 1]; below = len > 1 ? chain[len - 2] : -1; }
    }
    if (tid == 0) *err = status ? status : merges < n - 1 ? 1 : 0;
}

// Per sample (a workgroup takes samples blockIdx.x, + gridDim.x, ...): the labels that more than two cells carry, counted with a counter
// of two bits per label value that stops at 3; *sum += that number, over all samples.  A counter's word changes at most 48 times a sample
// (16 counters, 3 steps each), which bounds the compare-and-swap loop.
__global__ __launch_bounds__(256) void k_bnpc_cluster_counts(const uint16_t* __restrict__ lab, int64_t n_samples, int32_t n_cells, int32_t pitch, unsigned long long* sum) {
    __shared__ uint32_t cnt[CC_WORDS];
    __shared__ unsigned long long acc;
    const int words = (n_cells + 15) / 16;
    if (threadIdx.x == 0) acc = 0;
    unsigned long long mine = 0;
    for (int64_t s = blockIdx.x; s < n_samples; s += gridDim.x) {
        const uint16_t* row = lab + s * pitch;
        __syncthreads();
        for (int w = threadIdx.x; w < words; w += 256) cnt[w] = 0;
        __syncthreads();
        for (int i = threadIdx.x; i < n_cells; i += 256) {
            const uint32_t l = row[i], w = l >> 4, sh = (l & 15) * 2;
            uint32_t old = cnt[w];
            for (int tries = 0; tries < 49 && ((old >> sh) & 3u) != 3u; ++tries) {
                const uint32_t seen = atomicCAS(&cnt[w], old, old + (1u << sh));
                if (seen == old) break;
                old = seen;
            }
        }
        __syncthreads();
        for (int w = threadIdx.x; w < words; w += 256) mine += __popc(cnt[w] & (cnt[w] >> 1) & 0x55555555u);
    }
    for (int d = 32; d > 0; d >>= 1) mine += __shfl_down(mine, d, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(&acc, mine);
    __syncthreads();
    if (threadIdx.x == 0 && acc) atomicAdd(sum, acc);
}

static int sync_check(lsg_ctx* c, const char* who) {
    hipError_t e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = hipGetLastError();
    if (e != hipSuccess) { set_error("%s: kernel failed: %s", who, hipGetErrorString(e)); return -1; }
    return 0;
}

// scipy's label(): rows in the sorted order name the roots of their two sides, the smaller first; row k makes node n + k, whose size is
// the union's at that point.  Then the order in which cut_tree applies the nodes: ascending height, equal heights in the reverse of a
// breadth-first visit from the root that queues the right child before the left.
static void label_and_order(Bnpc& b, const std::vector<double>& rec) {
    const int32_t n = b.n_cells;
    std::vector<int32_t> by(n - 1);
    std::iota(by.begin(), by.end(), 0);
    std::stable_sort(by.begin(), by.end(), [&](int32_t p, int32_t q) { return rec[4 * (size_t)p + 2] < rec[4 * (size_t)q + 2]; });
    std::vector<int32_t> parent(2 * (size_t)n - 1), members(2 * (size_t)n - 1, 1);
    std::iota(parent.begin(), parent.end(), 0);
    auto find = [&](int32_t v) {
        int32_t root = v;
        while (parent[root] != root) root = parent[root];
        while (parent[v] != root) { const int32_t up = parent[v]; parent[v] = root; v = up; }
        return root;
    };
    b.Z.assign(4 * (size_t)(n - 1), 0.0);
    for (int32_t k = 0; k < n - 1; ++k) {
        const double* r = &rec[4 * (size_t)by[k]];
        const int32_t p = find((int32_t)r[0]), q = find((int32_t)r[1]);
        parent[p] = parent[q] = n + k;
        members[n + k] = members[p] + members[q];
        double* z = &b.Z[4 * (size_t)k];
        z[0] = (double)std::min(p, q); z[1] = (double)std::max(p, q); z[2] = r[2]; z[3] = (double)members[n + k];
    }
    std::vector<int32_t> visit(n - 1, 0), queue;
    queue.reserve(2 * (size_t)n - 1);
    queue.push_back(2 * n - 2);
    for (size_t at = 0; at < queue.size(); ++at) {
        const int32_t node = queue[at];
        if (node < n) continue;
        visit[node - n] = (int32_t)at;
        queue.push_back((int32_t)b.Z[4 * (size_t)(node - n) + 1]);
        queue.push_back((int32_t)b.Z[4 * (size_t)(node - n)]);
    }
    b.cut_order.resize(n - 1);
    std::iota(b.cut_order.begin(), b.cut_order.end(), 0);
    std::sort(b.cut_order.begin(), b.cut_order.end(), [&](int32_t p, int32_t q) {
        const double hp = b.Z[4 * (size_t)p + 2], hq = b.Z[4 * (size_t)q + 2];
        return hp < hq || (hp == hq && visit[p] > visit[q]);
    });
}

int run_bnpc_linkage(lsg_ctx* c, double* Z) {
    const char* who = "lsg_bnpc_linkage";
    Bnpc& b = c->bnpc;
    if (!b.valid || !b.dist_valid) { set_error("%s: no distances resident (lsg_bnpc_load_samples and lsg_bnpc_codist first)", who); return -2; }
    const int32_t n = b.n_cells;
    b.tree_valid = false;
    {
        const size_t bytes = (size_t)n * n * 8;
        if (bytes > b.work.cap) {
            size_t free_b = 0, total_b = 0;
            LSG_HIP(hipMemGetInfo(&free_b, &total_b));
            const size_t need = bytes + bytes / 16 + ((size_t)1 << 20);                 // (the buffer's slack and the small arrays)
            if (need > free_b + b.work.cap) {
                set_error("%s: the working matrix of %d cells takes %llu bytes, %llu bytes of device memory are free", who, n, (unsigned long long)bytes, (unsigned long long)(free_b + b.work.cap));
                return -2;
            }
        }
        if (b.work.reserve(bytes) || b.wsmall.reserve((size_t)n * 8 + 64) || b.rec.reserve((size_t)(n - 1) * 32)) return -1;
        hipStream_t st = c->stream;
        int32_t* d_err = b.wsmall.as<int32_t>(); int32_t* d_size = d_err + 16; int32_t* d_chain = d_size + n;
        const unsigned blocks = (unsigned)std::min<int64_t>(((int64_t)n * n + 255) / 256, (int64_t)c->n_cus * 32);
        hipLaunchKernelGGL(k_bnpc_ward_fill, dim3(blocks), dim3(256), 0, st, b.dist.as<uint32_t>(), b.n_samples, n, b.work.as<double>());
        hipLaunchKernelGGL(k_bnpc_ward, dim3(1), dim3(WT), 0, st, b.work.as<double>(), n, d_size, d_chain, b.rec.as<double>(), d_err);
        std::vector<double> rec(4 * (size_t)(n - 1));
        int32_t h_err = -1;
        LSG_HIP(hipMemcpyAsync(&h_err, d_err, 4, hipMemcpyDeviceToHost, st));
        LSG_HIP(hipMemcpyAsync(rec.data(), b.rec.p, rec.size() * 8, hipMemcpyDeviceToHost, st));
        if (sync_check(c, who)) return -1;
        if (h_err) {
            set_error(h_err == 1 ? "%s: the chain did not end within its 3 (n_cells - 1) scans" : "%s: a scan found no nearest cell (a distance that is no number)", who);
            return -1;
        }
        label_and_order(b, rec);
        b.tree_valid = true;
    }
    if (Z) std::copy(b.Z.begin(), b.Z.end(), Z);
    return 0;
}

int run_bnpc_cut_tree(lsg_ctx* c, int32_t n_cuts, const int32_t* n_clusters, int32_t* labels) {
    const char* who = "lsg_bnpc_cut_tree";
    Bnpc& b = c->bnpc;
    if (!b.valid || !b.dist_valid) { set_error("%s: no distances resident (lsg_bnpc_load_samples and lsg_bnpc_codist first)", who); return -2; }
    if (n_cuts < 1 || !n_clusters || !labels) { set_error("%s: %d cuts (at least 1, with n_clusters and labels given)", who, n_cuts); return -2; }
    const int32_t n = b.n_cells;
    for (int32_t k = 0; k < n_cuts; ++k)
        if (n_clusters[k] < 1 || n_clusters[k] > n - 1) {
            set_error("%s: n_clusters[%d] = %d is outside 1 .. %d (n_cells - 1; scipy's cut_tree answers n_cells itself with zeros)", who, k, n_clusters[k], n - 1);
            return -2;
        }
    if (!b.tree_valid)
        if (int rc = run_bnpc_linkage(c, nullptr)) return rc;
    std::vector<int32_t> by(n_cuts);                                                     // the cuts by the nodes they apply, ascending
    std::iota(by.begin(), by.end(), 0);
    std::stable_sort(by.begin(), by.end(), [&](int32_t p, int32_t q) { return n_clusters[p] > n_clusters[q]; });
    std::vector<int32_t> root(n), low(2 * (size_t)n - 1), id(n);                          // root: towards a cluster's lowest leaf; low: a node's lowest leaf
    std::iota(root.begin(), root.end(), 0);
    std::iota(low.begin(), low.begin() + n, 0);
    auto find = [&](int32_t v) {
        int32_t r = v;
        while (root[r] != r) r = root[r];
        while (root[v] != r) { const int32_t up = root[v]; root[v] = r; v = up; }
        return r;
    };
    int32_t applied = 0;
    for (int32_t k : by) {
        for (; applied < n - n_clusters[k]; ++applied) {
            const int32_t node = b.cut_order[applied];
            const int32_t p = low[(int32_t)b.Z[4 * (size_t)node]], q = low[(int32_t)b.Z[4 * (size_t)node + 1]];
            low[n + node] = std::min(p, q);
            root[std::max(p, q)] = std::min(p, q);
        }
        int32_t* out = labels + (size_t)k * n;
        int32_t next = 0;
        for (int32_t i = 0; i < n; ++i) {                                                // a cluster's label: its rank by its lowest leaf
            const int32_t r = find(i);
            if (r == i) id[i] = next++;
            out[i] = id[r];
        }
    }
    return 0;
}

int run_bnpc_cluster_counts(lsg_ctx* c, int64_t* sum_over_samples) {
    const char* who = "lsg_bnpc_cluster_counts";
    Bnpc& b = c->bnpc;
    if (!b.valid) { set_error("%s: no samples resident (lsg_bnpc_load_samples first)", who); return -2; }
    if (!sum_over_samples) { set_error("%s: sum_over_samples is NULL", who); return -2; }
    if (b.small.reserve(64)) return -1;
    unsigned long long* d_sum = b.small.as<unsigned long long>();
    LSG_HIP(hipMemsetAsync(d_sum, 0, 8, c->stream));
    const unsigned blocks = (unsigned)std::min<int64_t>(b.n_samples, (int64_t)c->n_cus * 8);
    hipLaunchKernelGGL(k_bnpc_cluster_counts, dim3(blocks), dim3(256), 0, c->stream, b.lab.as<uint16_t>(), b.n_samples, b.n_cells, b.pitch, d_sum);
    unsigned long long h = 0;
    LSG_HIP(hipMemcpyAsync(&h, d_sum, 8, hipMemcpyDeviceToHost, c->stream));
    if (sync_check(c, who)) return -1;
    *sum_over_samples = (int64_t)h;
    return 0;
}

} // namespace lsg
