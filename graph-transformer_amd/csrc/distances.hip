// Shortest-path distances on the device, from the one-hop structure u2gnn_graph_structure (hops = NULL etype): a
// batch's pair types (attention="graphs" with distances=H) and the expansion of the H-hop structure (attention="edges"
// with hops=H).  Integers only; the host builders (batching.hop_lists, GraphStore.distances) are the oracle and every
// result equals theirs value for value.
//
// Pair distances: one wave (a 64-thread block) owns one source row i of one graph of the batch.  The row lives as bytes
// in LDS, cap everywhere and 0 at i.  Level-synchronous sweeps in pull form: in sweep h an unset node u (row[u] == cap)
// takes h if one of its in-neighbours (the structure's transposed list of u) holds h - 1.  A sweep writes only the
// thread's own elements, and a value written during sweep h (h) is never mistaken for h - 1 (nor is cap, h - 1 <
// cap), so the result does not depend on the order of the threads.  The sweeps stop when one sets nothing; the row
// then leaves coalesced, as int32 (the batch's etype) or as bytes (the dense blocks the expansion reads).
//
// Expansion: from the dense blocks D (cap H + 1) of a chunk of graphs.  Rows: a wave per row compacts the columns
// with D <= H in ascending order by 64-bit ballot and popcount (count, then fill col / etype and the rank of each
// kept pair inside its row, uint16).  Columns: a thread per column walks the rows in ascending order (consecutive
// threads read consecutive bytes), counts, then fills t_src / t_eid, the entry id being the row's first entry inside
// the graph plus the stored rank.  The prefix sums between counting and filling are the caller's.
//
// Determinism: no atomics; every output element is written by exactly one thread.
//
// Indices: any content of the device arrays is memory-safe.  A slot stays inside [0, B); its rows must lie inside
// [0, N), hold between 1 and max_nodes nodes and its block inside [0, n_pairs), else nothing of it is written; a graph
// id is checked against [0, G) before node_start is read, the graph's nodes against [0, V) and the slot's node count
// before t_rowptr is, an entry against [0, E) before t_src is, a t_src value against [0, n) before it indexes the row,
// an output position against [0, E) before it is written.  A row that fails a check is written as type 0 and *err is
// set.
#include "u2gnn_common.h"

#include <climits>

namespace {

constexpr int DIST_WAVE = 64;
constexpr int COL_THREADS = 256;

__device__ __forceinline__ int64_t wadd(int64_t a, int64_t b) { return (int64_t)((uint64_t)a + (uint64_t)b); }
__device__ __forceinline__ int64_t wsub(int64_t a, int64_t b) { return (int64_t)((uint64_t)a - (uint64_t)b); }

// what every kernel here knows of its batch (or chunk): B slots, N rows, n_pairs dense elements
struct Batch {
    const int64_t *row_off, *pair_off;   // [B+1] each
    int B, max_n;
    int64_t N, n_pairs;
};

struct Slot {
    int b, n, i;        // slot, its node count, the row inside it
    int64_t lo, po;     // the slot's first row and first dense element
    bool ok;
};

// the slot of row r: the last b in [0, B) with row_off[b] <= r, and whether everything derived from it is in range
__device__ __forceinline__ Slot slot_of(const Batch &t, int64_t r) {
    int lo = 0, hi = t.B - 1;
    while (lo < hi) {
        const int mid = lo + (hi - lo + 1) / 2;             // in [1, B - 1]
        if (t.row_off[mid] <= r) lo = mid;
        else hi = mid - 1;
    }
    Slot s;
    s.b = lo;
    s.lo = t.row_off[lo];
    s.po = t.pair_off[lo];
    const int64_t n = wsub(t.row_off[lo + 1], s.lo), i = wsub(r, s.lo);
    s.ok = n >= 1 && n <= t.max_n && i >= 0 && i < n && s.lo >= 0 && s.lo <= t.N - n && s.po >= 0 &&
           s.po <= t.n_pairs - n * n;                       // n <= 4096: n * n cannot overflow
    s.n = (int)n, s.i = (int)i;
    return s;
}

struct DistArgs {
    u2gnn_graph_structure S;
    const int64_t *gid;
    Batch t;
    int cap;
    int32_t *err;
};

template <typename OutT>
__global__ __launch_bounds__(DIST_WAVE) void pair_distances_kernel(const DistArgs a, OutT *__restrict__ out) {
    extern __shared__ uint8_t row[];
    const u2gnn_graph_structure &S = a.S;
    const int lane = threadIdx.x;
    const Slot s = slot_of(a.t, blockIdx.x);
    if (!s.ok) {
        if (lane == 0) *a.err = 1;
        return;
    }
    const int n = s.n;
    OutT *__restrict__ dst = out + s.po + (int64_t)s.i * n;
    const int64_t g = a.gid[s.b];
    bool ok = g >= 0 && g < S.G;
    int64_t v0 = 0;
    if (ok) {
        v0 = S.node_start[g];
        const int64_t v1 = S.node_start[g + 1];
        ok = v0 >= 0 && v1 <= S.V && wsub(v1, v0) == n;
    }
    if (!ok) {
        for (int j = lane; j < n; j += DIST_WAVE) dst[j] = 0;
        if (lane == 0) *a.err = 1;
        return;
    }
    const int cap = a.cap;
    for (int j = lane; j < n; j += DIST_WAVE) row[j] = (uint8_t)(j == s.i ? 0 : cap);
    __syncthreads();
    int bad = 0;
    for (int h = 1; h < cap; ++h) {
        int set = 0;
        for (int u = lane; u < n; u += DIST_WAVE) {
            if (row[u] != cap) continue;
            const int64_t e0 = S.t_rowptr[v0 + u], e1 = S.t_rowptr[v0 + u + 1];
            if (e0 < 0 || e1 > S.E || e0 > e1) {
                bad = 1;
                continue;
            }
            for (int64_t e = e0; e < e1; ++e) {
                const uint32_t src = (uint32_t)S.t_src[e];
                if (src >= (uint32_t)n) {
                    bad = 1;
                    continue;
                }
                if (row[src] == h - 1) {
                    row[u] = (uint8_t)h;
                    set = 1;
                    break;
                }
            }
        }
        if (!__syncthreads_or(set)) break;                  // the barrier between two sweeps, and the early exit
    }
    bad = __syncthreads_or(bad);
    for (int j = lane; j < n; j += DIST_WAVE) dst[j] = bad ? (OutT)0 : (OutT)row[j];
    if (bad && lane == 0) *a.err = 1;
}

__device__ __forceinline__ int wave_max_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
    return v;
}

// per slot: ecc = max over its pairs of min(D, cap - 1), fin = the largest D below cap
__global__ __launch_bounds__(COL_THREADS) void distance_extents_kernel(const uint8_t *__restrict__ D, const Batch t,
                                                                       int cap, int32_t *__restrict__ ecc,
                                                                       int32_t *__restrict__ fin, int32_t *err) {
    __shared__ int s_e[COL_THREADS / 64], s_f[COL_THREADS / 64];
    const int b = blockIdx.x;
    const int64_t lo = t.row_off[b], n = wsub(t.row_off[b + 1], lo), po = t.pair_off[b];
    const bool ok = n >= 1 && n <= t.max_n && po >= 0 && po <= t.n_pairs - n * n;
    int e = 0, f = 0;
    if (ok) {
        const int64_t nn = n * n;
        for (int64_t p = threadIdx.x; p < nn; p += COL_THREADS) {
            const int v = D[po + p];
            e = max(e, min(v, cap - 1));
            if (v < cap) f = max(f, v);
        }
    }
    e = wave_max_i(e), f = wave_max_i(f);
    if ((threadIdx.x & 63) == 0) s_e[threadIdx.x >> 6] = e, s_f[threadIdx.x >> 6] = f;
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < COL_THREADS / 64; ++w) e = max(e, s_e[w]), f = max(f, s_f[w]);
        ecc[b] = e, fin[b] = f;
        if (!ok && n != 0) *err = 1;                        // a graph without nodes owns nothing: 0, 0
    }
}

struct ExpArgs {
    const uint8_t *D;
    Batch t;
    int H;
    int64_t *cnt, *t_cnt;                   // count: [N] each
    uint16_t *L;                            // fill: the rank of each kept pair inside its row, laid out as D
    const int64_t *rowptr, *t_rowptr;       // fill: [N] each, the chunk's part of the new row pointers
    int64_t E;                              // fill: the entries of the whole dataset (col .. t_eid hold E each)
    int32_t *col, *t_src, *t_eid;
    uint8_t *etype;
    int32_t *err;
};

template <bool FILL>
__global__ __launch_bounds__(DIST_WAVE) void hop_rows_kernel(const ExpArgs a) {
    const int lane = threadIdx.x;
    const int64_t r = blockIdx.x;
    const Slot s = slot_of(a.t, r);
    if (!s.ok) {
        if (lane == 0) {
            *a.err = 1;
            if (!FILL) a.cnt[r] = 0;
        }
        return;
    }
    const int n = s.n;
    const int64_t at = s.po + (int64_t)s.i * n;
    const uint8_t *__restrict__ d = a.D + at;
    const int64_t base = FILL ? a.rowptr[r] : 0;
    int run = 0;
    for (int j0 = 0; j0 < n; j0 += DIST_WAVE) {
        const int j = j0 + lane;
        const int v = j < n ? d[j] : 255;
        const bool in = v <= a.H;
        const unsigned long long m = __ballot(in);
        if (FILL && in) {
            const int rank = run + __popcll(m & ((1ull << lane) - 1));
            const int64_t pos = wadd(base, rank);
            if (pos >= 0 && pos < a.E) {
                a.col[pos] = j;
                a.etype[pos] = (uint8_t)v;
            } else {
                *a.err = 1;
            }
            a.L[at + j] = (uint16_t)rank;
        }
        run += __popcll(m);
    }
    if (!FILL && lane == 0) a.cnt[r] = run;
}

template <bool FILL>
__global__ __launch_bounds__(COL_THREADS) void hop_cols_kernel(const ExpArgs a) {
    const int64_t c = (int64_t)blockIdx.x * COL_THREADS + threadIdx.x;
    if (c >= a.t.N) return;
    const Slot s = slot_of(a.t, c);                         // s.i: the column inside its graph
    if (!s.ok) {
        *a.err = 1;
        if (!FILL) a.t_cnt[c] = 0;
        return;
    }
    const int n = s.n;
    const uint8_t *__restrict__ d = a.D + s.po + s.i;
    const uint16_t *__restrict__ l = a.L + s.po + s.i;
    const int64_t base = FILL ? a.t_rowptr[c] : 0;
    const int64_t first = FILL ? a.rowptr[s.lo] : 0;        // the graph's first entry
    int k = 0;
    for (int i = 0; i < n; ++i) {
        if (d[(int64_t)i * n] > a.H) continue;
        if (FILL) {
            const int64_t pos = wadd(base, k);
            if (pos >= 0 && pos < a.E) {
                a.t_src[pos] = i;
                a.t_eid[pos] = (int32_t)wadd(wsub(a.rowptr[s.lo + i], first), l[(int64_t)i * n]);
            } else {
                *a.err = 1;
            }
        }
        ++k;
    }
    if (!FILL) a.t_cnt[c] = k;
}

bool misaligned(const void *p, uintptr_t mask) { return ((uintptr_t)p & mask) != 0; }

// the checks every entry point shares: 0, or the code to return before anything is launched
int check_batch(const int64_t *row_off, const int64_t *pair_off, int32_t B, int64_t N, int64_t n_pairs,
                int32_t max_nodes, const int32_t *err) {
    if (!row_off || !pair_off || !err || B < 1 || N < 1 || n_pairs < 1 || max_nodes < 1) return U2GNN_E_ARG;
    if (max_nodes > U2GNN_DIST_NODES_MAX || N > INT_MAX) return U2GNN_E_SHAPE;
    if (misaligned(row_off, 7) || misaligned(pair_off, 7) || misaligned(err, 3)) return U2GNN_E_ALIGN;
    return 0;
}

Batch batch_of(const int64_t *row_off, const int64_t *pair_off, int32_t B, int64_t N, int64_t n_pairs,
               int32_t max_nodes) {
    Batch t;
    t.row_off = row_off, t.pair_off = pair_off, t.B = B, t.max_n = max_nodes, t.N = N, t.n_pairs = n_pairs;
    return t;
}

template <typename OutT>
int pair_distances(const u2gnn_graph_structure *S, const int64_t *gid, const int64_t *row_off, const int64_t *pair_off,
                   int32_t B, int64_t N, int64_t n_pairs, int32_t max_nodes, int32_t cap, int32_t cap_max, OutT *out,
                   int32_t *err, void *stream) {
    if (!S || !S->node_start || !S->t_rowptr || !S->t_src || S->G < 1 || S->V < 1 || S->E < 1 || !gid || !out)
        return U2GNN_E_ARG;
    if (const int rc = check_batch(row_off, pair_off, B, N, n_pairs, max_nodes, err)) return rc;
    if (cap < 1 || cap > cap_max) return U2GNN_E_SHAPE;
    if (misaligned(S->node_start, 7) || misaligned(S->t_rowptr, 7) || misaligned(S->t_src, 3) || misaligned(gid, 7) ||
        misaligned(out, sizeof(OutT) - 1))
        return U2GNN_E_ALIGN;
    DistArgs a;
    a.S = *S;
    a.gid = gid;
    a.t = batch_of(row_off, pair_off, B, N, n_pairs, max_nodes);
    a.cap = cap, a.err = err;
    hipLaunchKernelGGL(pair_distances_kernel<OutT>, dim3((unsigned)N), dim3(DIST_WAVE), (size_t)((max_nodes + 15) & ~15),
                       u2gnn_stream(stream), a, out);
    return u2gnn_launch_status();
}

}  // namespace

extern "C" {

int u2gnn_pair_distances(const u2gnn_graph_structure *S, const int64_t *gid, const int64_t *row_off,
                         const int64_t *pair_off, int32_t B, int64_t N, int64_t n_pairs, int32_t max_nodes, int32_t H,
                         int32_t *etype, int32_t *err, void *stream) {
    return pair_distances<int32_t>(S, gid, row_off, pair_off, B, N, n_pairs, max_nodes, H, U2GNN_BIAS_TYPES_MAX - 1,
                                   etype, err, stream);
}

int u2gnn_pair_distances_u8(const u2gnn_graph_structure *S, const int64_t *gid, const int64_t *row_off,
                            const int64_t *pair_off, int32_t B, int64_t N, int64_t n_pairs, int32_t max_nodes,
                            int32_t cap, uint8_t *D, int32_t *err, void *stream) {
    return pair_distances<uint8_t>(S, gid, row_off, pair_off, B, N, n_pairs, max_nodes, cap, U2GNN_BIAS_TYPES_MAX, D,
                                   err, stream);
}

int u2gnn_distance_extents(const uint8_t *D, const int64_t *row_off, const int64_t *pair_off, int32_t B, int64_t N,
                           int64_t n_pairs, int32_t max_nodes, int32_t cap, int32_t *ecc, int32_t *fin, int32_t *err,
                           void *stream) {
    if (!D || !ecc || !fin) return U2GNN_E_ARG;
    if (const int rc = check_batch(row_off, pair_off, B, N, n_pairs, max_nodes, err)) return rc;
    if (cap < 1 || cap > U2GNN_BIAS_TYPES_MAX) return U2GNN_E_SHAPE;
    if (misaligned(ecc, 3) || misaligned(fin, 3)) return U2GNN_E_ALIGN;
    hipLaunchKernelGGL(distance_extents_kernel, dim3((unsigned)B), dim3(COL_THREADS), 0, u2gnn_stream(stream), D,
                       batch_of(row_off, pair_off, B, N, n_pairs, max_nodes), cap, ecc, fin, err);
    return u2gnn_launch_status();
}

int u2gnn_hop_expand_count(const uint8_t *D, const int64_t *row_off, const int64_t *pair_off, int32_t B, int64_t N,
                           int64_t n_pairs, int32_t max_nodes, int32_t H, int64_t *cnt, int64_t *t_cnt, int32_t *err,
                           void *stream) {
    if (!D || !cnt || !t_cnt) return U2GNN_E_ARG;
    if (const int rc = check_batch(row_off, pair_off, B, N, n_pairs, max_nodes, err)) return rc;
    if (H < 1 || H > U2GNN_BIAS_TYPES_MAX - 1) return U2GNN_E_SHAPE;
    if (misaligned(cnt, 7) || misaligned(t_cnt, 7)) return U2GNN_E_ALIGN;
    ExpArgs a = {};
    a.D = D, a.t = batch_of(row_off, pair_off, B, N, n_pairs, max_nodes), a.H = H, a.cnt = cnt, a.t_cnt = t_cnt;
    a.err = err;
    hipLaunchKernelGGL(hop_rows_kernel<false>, dim3((unsigned)N), dim3(DIST_WAVE), 0, u2gnn_stream(stream), a);
    hipLaunchKernelGGL(hop_cols_kernel<false>, dim3((unsigned)((N + COL_THREADS - 1) / COL_THREADS)), dim3(COL_THREADS),
                       0, u2gnn_stream(stream), a);
    return u2gnn_launch_status();
}

int u2gnn_hop_expand_fill(const uint8_t *D, uint16_t *L, const int64_t *row_off, const int64_t *pair_off, int32_t B,
                          int64_t N, int64_t n_pairs, int32_t max_nodes, int32_t H, const int64_t *rowptr,
                          const int64_t *t_rowptr, int64_t E, int32_t *col, uint8_t *etype, int32_t *t_src,
                          int32_t *t_eid, int32_t *err, void *stream) {
    if (!D || !L || !rowptr || !t_rowptr || !col || !etype || !t_src || !t_eid || E < 1) return U2GNN_E_ARG;
    if (const int rc = check_batch(row_off, pair_off, B, N, n_pairs, max_nodes, err)) return rc;
    if (H < 1 || H > U2GNN_BIAS_TYPES_MAX - 1) return U2GNN_E_SHAPE;
    if (misaligned(L, 1) || misaligned(rowptr, 7) || misaligned(t_rowptr, 7) || misaligned(col, 3) ||
        misaligned(t_src, 3) || misaligned(t_eid, 3))
        return U2GNN_E_ALIGN;
    ExpArgs a = {};
    a.D = D, a.t = batch_of(row_off, pair_off, B, N, n_pairs, max_nodes), a.H = H, a.L = L;
    a.rowptr = rowptr, a.t_rowptr = t_rowptr, a.E = E;
    a.col = col, a.etype = etype, a.t_src = t_src, a.t_eid = t_eid, a.err = err;
    hipLaunchKernelGGL(hop_rows_kernel<true>, dim3((unsigned)N), dim3(DIST_WAVE), 0, u2gnn_stream(stream), a);
    hipLaunchKernelGGL(hop_cols_kernel<true>, dim3((unsigned)((N + COL_THREADS - 1) / COL_THREADS)), dim3(COL_THREADS),
                       0, u2gnn_stream(stream), a);
    return u2gnn_launch_status();
}

}  // extern "C"
