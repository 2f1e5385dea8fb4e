// Per-graph ("graphs" mode) attention of U2GNN: every node attends over the nodes of its own graph, so the
// attention matrix of a mini-batch is block-diagonal -- the fork's node-axis encoder (pytorch_U2GNN_Sup.py:19-21,35)
// applied to every graph on its own, batched.  Graph g owns the consecutive rows seg_offsets[g] ..
// seg_offsets[g+1]-1 of QKV [rows_pad, 3*dp] = [Q/sqrt(d) | K | V] (what the in-projection epilogue writes).
//
// The work, 2 * sum_g n_g^2 * dp FLOP per product, is small and ragged (C4: 64 graphs of ~75 nodes), far from the
// 256x128 MFMA tiles of the node-axis path: exact fp32 on the vector ALUs under every precision policy, as the
// window kernel and the d <= 32 kernels.  Flash-style: a block owns a tile of TQ rows and walks tiles of TK rows of
// the other side through LDS, so no [n_g, n_g] image goes to HBM and no LDS bound applies to n_g.  The forward
// keeps the running (max, sum) per row and saves (max, 1 / sum); the backward recomputes P from them.
//
// Determinism: no atomics.  The backward is two launches: one over query tiles (delta = rowsum(dO * O) and dQ), one
// over key tiles (dK, dV); every output element is one fixed-order fp32 chain.
//
// Segments: the offsets live on the device only.  Every row finds its segment by binary search, every bound is
// clamped to [0, N], a row covered by no segment gets zero output, and a tile that straddles segments walks the
// union of its rows' ranges and masks per row.
//
// BIAS (u2gnn_segment_attn_*_bias): an additive term per (query, key) pair of a segment on the score before the
// softmax -- the model's learned scalar per shortest-path distance.  Segment g's n_g^2 pairs are the floats
// bias[pair_off[g] ..], row-major [query][key]; the entry id of a pair is formed from the row's clamped range, and
// an id outside [0, n_pairs) reads 0 and writes nothing, so any pair_off content is memory-safe as the offsets are.
// The query-tile backward also stores dS per pair (dL/dbias): every pair once, no atomics.  A compile-time flag of
// the three kernels; the instantiations without it are the kernels as they were.
#include <mutex>
#include <set>
#include <utility>

#include "u2gnn_common.h"

#include <algorithm>
#include <climits>

namespace {

constexpr int SEG_THREADS = 256;
constexpr size_t SEG_LDS_LIMIT = 160 * 1024;

// LDS images are [T][dp + 4]: consecutive rows 4 banks apart, so the float4 reads of 16 different rows at one
// column (ds_read_b128 is served 16 lanes at a time) cover the 64 banks once (dp is a multiple of 64)
__host__ __device__ __forceinline__ int seg_ld(int dp) { return dp + 4; }

// the key range [lo, hi) of row i: the segment g with off[g] <= i < off[g+1] (the last such g, so empty segments
// are skipped), bounds clamped to [0, N]; lo = hi = 0 when no segment covers the row.  g: that segment's index
__device__ __forceinline__ void seg_range(const int64_t *off, int n_seg, int64_t i, int64_t N, int &lo, int &hi,
                                          int &g) {
    lo = hi = g = 0;
    if (i >= N || off[0] > i) return;
    int a = 0, b = n_seg;   // off[a] <= i; the answer is in [a, b)
    while (b - a > 1) {
        const int mid = (a + b) >> 1;
        if (off[mid] <= i) a = mid;
        else b = mid;
    }
    const int64_t s = min(max(off[a], (int64_t)0), N), e = min(max(off[a + 1], (int64_t)0), N);
    if (i < s || i >= e) return;
    lo = (int)s, hi = (int)e, g = a;
}

// the ranges of the block's T rows into rlo / rhi (LDS).  BIAS: also the row's part of its pairs' entry ids into
// rpb, so that the pair of query i and key j of a segment [lo, hi) of n rows at pair base pb is entry
//   pb + (i - lo) n + (j - lo) = rpb[i] + j      with the block's rows as queries (COL false), or
//                              = rpb[j] + i n    with the block's rows as keys (COL true).
// Unsigned arithmetic: a wild pair_off wraps instead of overflowing, and seg_pair_bias refuses the id
template <bool BIAS, bool COL>
__device__ __forceinline__ void seg_tile_ranges(const int64_t *off, int n_seg, int64_t row0, int T, int64_t N, int *rlo,
                                                int *rhi, const int64_t *pair_off, uint64_t *rpb) {
    if ((int)threadIdx.x < T) {
        int lo, hi, g;
        seg_range(off, n_seg, row0 + threadIdx.x, N, lo, hi, g);
        rlo[threadIdx.x] = lo, rhi[threadIdx.x] = hi;
        if constexpr (BIAS) {
            const uint64_t r = (uint64_t)(row0 + threadIdx.x) - (uint64_t)lo, n = (uint64_t)(hi - lo);
            uint64_t b = 0;
            if (hi > lo) b = (uint64_t)pair_off[g] + (COL ? r - (uint64_t)lo * n : r * n - (uint64_t)lo);
            rpb[threadIdx.x] = b;
        }
    }
}

// the bias of entry e, 0 for an id outside [0, n_pairs)
__device__ __forceinline__ float seg_pair_bias(const float *bias, uint64_t e, int64_t n_pairs) {
    return e < (uint64_t)n_pairs ? bias[e] : 0.f;
}

// the union of the rows' ranges (after a barrier): [beg, end), empty when no row is covered
__device__ __forceinline__ void seg_union(const int *rlo, const int *rhi, int T, int &beg, int &end) {
    beg = INT_MAX, end = 0;
    for (int i = 0; i < T; ++i)
        if (rhi[i] > rlo[i]) beg = min(beg, rlo[i]), end = max(end, rhi[i]);
    if (end == 0) beg = 0;
}

// rows row0 .. row0+T-1 (rows >= rlim: zeros) of a [rows][ld] operand at column offset col -> a [T][dp + 4] image
__device__ __forceinline__ void seg_stage(const float *src, int64_t ld, int64_t row0, int64_t rlim, int col, int T,
                                          int dp, float *img) {
    const int dq = dp / 4, LD = seg_ld(dp);
    // element e = i * dq + c of the image, e = tid, tid + 256, ...: (i, c) advanced without a division per element
    const int di = SEG_THREADS / dq, dc = SEG_THREADS - di * dq;
    int i = threadIdx.x / dq, c = threadIdx.x - i * dq;
    while (i < T) {
        const int64_t r = row0 + i;
        *reinterpret_cast<float4 *>(img + i * LD + 4 * c) =
            r < rlim ? *reinterpret_cast<const float4 *>(src + r * ld + col + 4 * c) : make_float4(0.f, 0.f, 0.f, 0.f);
        i += di, c += dc;
        if (c >= dq) c -= dq, ++i;
    }
}

// The walked tiles go through registers: seg_fetch issues a tile's global loads (SEG_PF float4 per thread, so
// T * dp / 4 <= 256 * SEG_PF: seg_tiles bounds TK by it), seg_put stores them into the LDS image later -- the loads
// of the next tile fly while this tile computes instead of standing in front of it.  The same element walk as
// seg_stage; rows >= rlim are zeros.
constexpr int SEG_PF = 16;
__device__ __forceinline__ void seg_fetch(const float *src, int64_t ld, int64_t row0, int64_t rlim, int col, int T,
                                          int dp, float4 (&r)[SEG_PF]) {
    const int dq = dp / 4;
    const int di = SEG_THREADS / dq, dc = SEG_THREADS - di * dq;
    int i = threadIdx.x / dq, c = threadIdx.x - i * dq;
#pragma unroll
    for (int q = 0; q < SEG_PF; ++q) {
        const int64_t row = row0 + i;
        r[q] = (i < T && row < rlim) ? *reinterpret_cast<const float4 *>(src + row * ld + col + 4 * c)
                                     : make_float4(0.f, 0.f, 0.f, 0.f);
        i += di, c += dc;
        if (c >= dq) c -= dq, ++i;
    }
}
__device__ __forceinline__ void seg_put(float *img, int T, int dp, const float4 (&r)[SEG_PF]) {
    const int dq = dp / 4, LD = seg_ld(dp);
    const int di = SEG_THREADS / dq, dc = SEG_THREADS - di * dq;
    int i = threadIdx.x / dq, c = threadIdx.x - i * dq;
#pragma unroll
    for (int q = 0; q < SEG_PF; ++q) {
        if (i < T) *reinterpret_cast<float4 *>(img + i * LD + 4 * c) = r[q];
        i += di, c += dc;
        if (c >= dq) c -= dq, ++i;
    }
}

// X[i][j] = A_i . B_j (i < TA, TA % 4 == 0; j < TB, a power of two) into X[TA][TB + 1].  A thread takes one B row
// against NR A rows (the B float4 is read once for 4 NR fma; the A reads are wave-wide broadcasts); four partial
// sums per pair by column residue, combined as (s0 + s1) + (s2 + s3) -- a fixed order, the same for every NR
template <int NR>
__device__ __forceinline__ void seg_dots_nr(const float *A, const float *B, int TA, int TB, int dp, float *X) {
    const int LD4 = seg_ld(dp) / 4, dq = dp / 4, sh = __ffs(TB) - 1;
    for (int e = threadIdx.x; e < (TA / NR) * TB; e += SEG_THREADS) {
        const int g = e >> sh, j = e & (TB - 1), i0 = g * NR;
        const float4 *b = reinterpret_cast<const float4 *>(B) + j * LD4;
        const float4 *a = reinterpret_cast<const float4 *>(A) + i0 * LD4;
        float s[NR][4];
#pragma unroll
        for (int r = 0; r < NR; ++r) s[r][0] = s[r][1] = s[r][2] = s[r][3] = 0.f;
#pragma unroll 2
        for (int c = 0; c < dq; ++c) {
            const float4 y = b[c];
#pragma unroll
            for (int r = 0; r < NR; ++r) {
                const float4 x = a[r * LD4 + c];
                s[r][0] = fmaf(x.x, y.x, s[r][0]);
                s[r][1] = fmaf(x.y, y.y, s[r][1]);
                s[r][2] = fmaf(x.z, y.z, s[r][2]);
                s[r][3] = fmaf(x.w, y.w, s[r][3]);
            }
        }
#pragma unroll
        for (int r = 0; r < NR; ++r) X[(i0 + r) * (TB + 1) + j] = (s[r][0] + s[r][1]) + (s[r][2] + s[r][3]);
    }
}
// four rows per thread when that still occupies the block's 256 threads, else two
__device__ __forceinline__ void seg_dots(const float *A, const float *B, int TA, int TB, int dp, float *X) {
    if ((TA / 4) * TB >= SEG_THREADS) seg_dots_nr<4>(A, B, TA, TB, dp, X);
    else seg_dots_nr<2>(A, B, TA, TB, dp, X);
}

// acc[r] += sum_{j < jn} C[i0 + r][j] * M[j][4 c4 ..] in j order: the thread's float4 column group of its RB rows
template <int RB>
__device__ __forceinline__ void seg_accum(const float *C, int ldc, const float *M, int dp, int i0, int c4, int jn,
                                          float4 (&acc)[RB]) {
    const int LD4 = seg_ld(dp) / 4;
    const float4 *M4 = reinterpret_cast<const float4 *>(M) + c4;
    const float *Ci = C + i0 * ldc;
    for (int j = 0; j < jn; ++j) {
        const float4 m = M4[j * LD4];
        float cf[RB];
#pragma unroll
        for (int r = 0; r < RB; ++r) cf[r] = Ci[r * ldc + j];
#pragma unroll
        for (int r = 0; r < RB; ++r) {
            acc[r].x = fmaf(cf[r], m.x, acc[r].x);
            acc[r].y = fmaf(cf[r], m.y, acc[r].y);
            acc[r].z = fmaf(cf[r], m.z, acc[r].z);
            acc[r].w = fmaf(cf[r], m.w, acc[r].w);
        }
    }
}

// sum / max over the tpr (a power of two <= 64) consecutive lanes that share a row; every lane gets the result
__device__ __forceinline__ float seg_row_sum(float v, int tpr) {
    for (int o = tpr >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float seg_row_max(float v, int tpr) {
    for (int o = tpr >> 1; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// Forward.  Block = TQ query rows; per key tile: K -> scores -> (V staged over K beside) the online softmax and
// dropout -> O accumulators rescaled and advanced.  The accumulators' owner thread holds a float4 column group of
// RB rows (dq * TQ / RB <= 256 threads).
template <int RB, bool BIAS>
__global__ void __launch_bounds__(SEG_THREADS)
    segment_attn_fwd_kernel(const float *QKV, int64_t ldq, int dp, const int64_t *off, int n_seg, float *O, int64_t ldo,
                            float *stats, float p, uint64_t seed, const uint64_t *seed_epoch, int64_t N,
                            int64_t rows_pad, int TQ, int TK, const float *bias, const int64_t *pair_off,
                            int64_t n_pairs) {
    seed = u2gnn_seed(seed, seed_epoch);
    extern __shared__ __align__(16) float seg_sm[];
    const int LD = seg_ld(dp), dq = dp / 4, ldc = TK + 1, tid = threadIdx.x;
    float *Qs = seg_sm, *KV = Qs + TQ * LD, *S = KV + TK * LD, *alpha = S + TQ * ldc;
    int *rlo = reinterpret_cast<int *>(alpha + TQ), *rhi = rlo + TQ;
    uint64_t *rpb = reinterpret_cast<uint64_t *>(rhi + TQ);   // BIAS only (seg_lds)
    const int64_t row0 = (int64_t)blockIdx.x * TQ;
    seg_tile_ranges<BIAS, false>(off, n_seg, row0, TQ, N, rlo, rhi, pair_off, rpb);
    seg_stage(QKV, ldq, row0, N, 0, TQ, dp, Qs);
    __syncthreads();
    int kbeg, kend;
    seg_union(rlo, rhi, TQ, kbeg, kend);
    // softmax role: tpr consecutive lanes per row, each holding the row's running (max, sum)
    const int tpr = SEG_THREADS / TQ, si = tid / tpr, sub = tid - si * tpr;
    const int my_lo = rlo[si], my_hi = rhi[si];
    uint64_t my_pb = 0;   // the row's pairs: entry my_pb + key (the lanes of a row read consecutive floats)
    if constexpr (BIAS) my_pb = rpb[si];
    const uint32_t rkey = u2gnn_row_key(seed, (uint32_t)(row0 + si)), thr = u2gnn_keep_thr(p);
    const float ks = p > 0.f ? 1.f / (1.f - p) : 1.f;
    float m_run = -INFINITY, l_run = 0.f;
    // accumulator role
    const bool active = tid < dq * (TQ / RB);
    const int c4 = active ? tid % dq : 0, i0 = active ? (tid / dq) * RB : 0;
    float4 acc[RB];
#pragma unroll
    for (int r = 0; r < RB; ++r) acc[r] = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 pf[SEG_PF];
    if (kbeg < kend) seg_fetch(QKV, ldq, kbeg, kend, dp, TK, dp, pf);   // the first tile's K
    for (int k0 = kbeg; k0 < kend; k0 += TK) {
        seg_put(KV, TK, dp, pf);                                  // K
        seg_fetch(QKV, ldq, k0, kend, 2 * dp, TK, dp, pf);        // this tile's V: in flight during the scores
        __syncthreads();
        seg_dots(Qs, KV, TQ, TK, dp, S);
        __syncthreads();
        seg_put(KV, TK, dp, pf);                                  // V over K
        if (k0 + TK < kend) seg_fetch(QKV, ldq, k0 + TK, kend, dp, TK, dp, pf);   // the next K: during softmax and P.V
        float *srow = S + si * ldc;
        float tmax = -INFINITY;
        for (int j = sub; j < TK; j += tpr) {
            const int kj = k0 + j;
            if constexpr (BIAS) {   // the biased score replaces the product: the second sweep reads it back
                if (kj >= my_lo && kj < my_hi) {
                    const float s = srow[j] + seg_pair_bias(bias, my_pb + (uint64_t)kj, n_pairs);
                    srow[j] = s;
                    tmax = fmaxf(tmax, s);
                }
            } else {
                if (kj >= my_lo && kj < my_hi) tmax = fmaxf(tmax, srow[j]);
            }
        }
        tmax = seg_row_max(tmax, tpr);
        const float m_new = fmaxf(m_run, tmax);
        const float a = m_new == -INFINITY ? 1.f : expf(m_run - m_new);
        float sum = 0.f;
        for (int j = sub; j < TK; j += tpr) {
            const int kj = k0 + j;
            float pv = 0.f;
            if (kj >= my_lo && kj < my_hi) pv = expf(srow[j] - m_new);
            sum += pv;
            srow[j] = (p > 0.f) ? (u2gnn_keep_rk(rkey, (uint32_t)kj, thr) ? pv * ks : 0.f) : pv;
        }
        sum = seg_row_sum(sum, tpr);
        l_run = l_run * a + sum;
        m_run = m_new;
        if (sub == 0) alpha[si] = a;
        __syncthreads();
        if (active) {
#pragma unroll
            for (int r = 0; r < RB; ++r) {
                const float al = alpha[i0 + r];
                acc[r].x *= al, acc[r].y *= al, acc[r].z *= al, acc[r].w *= al;
            }
            seg_accum<RB>(S, ldc, KV, dp, i0, c4, min(TK, kend - k0), acc);
        }
        __syncthreads();   // the next tile overwrites KV, S and alpha
    }
    if (sub == 0) {
        const float inv = l_run > 0.f ? 1.f / l_run : 0.f;
        alpha[si] = inv;
        const int64_t row = row0 + si;
        if (row < rows_pad) *reinterpret_cast<float2 *>(stats + 2 * row) = make_float2(l_run > 0.f ? m_run : 0.f, inv);
    }
    __syncthreads();
    if (active) {
#pragma unroll
        for (int r = 0; r < RB; ++r) {
            const int64_t row = row0 + i0 + r;
            const float inv = alpha[i0 + r];
            if (row < rows_pad)
                *reinterpret_cast<float4 *>(O + row * ldo + 4 * c4) =
                    make_float4(acc[r].x * inv, acc[r].y * inv, acc[r].z * inv, acc[r].w * inv);
        }
    }
}

// Backward over query tiles: delta_i = rowsum(dO_i * O_i) (kept in delta_ws for the key-tile launch), then per key
// tile S = Qs K^T and dPd = dO V^T, dS = P o (keep dPd / (1-p) - delta) with P recomputed from the saved row
// statistics, dQ += dS K.  dQKV[:, 0:dp] = q_scale * dQ.
template <int RB, bool BIAS>
__global__ void __launch_bounds__(SEG_THREADS)
    segment_attn_bwd_q_kernel(const float *QKV, int64_t ldq, int dp, const int64_t *off, int n_seg, const float *O,
                              const float *dO, int64_t ldo, const float *stats, float p, uint64_t seed,
                              const uint64_t *seed_epoch, float q_scale, float *dQKV, int64_t ldg, float *delta_ws,
                              int64_t N, int64_t rows_pad, int TQ, int TK, const float *bias, const int64_t *pair_off,
                              int64_t n_pairs, float *dbias) {
    seed = u2gnn_seed(seed, seed_epoch);
    extern __shared__ __align__(16) float seg_sm[];
    const int LD = seg_ld(dp), dq = dp / 4, ldc = TK + 1, tid = threadIdx.x;
    float *Qs = seg_sm, *dOs = Qs + TQ * LD, *Ks = dOs + TQ * LD, *Vs = Ks + TK * LD;
    float *S = Vs + TK * LD, *dP = S + TQ * ldc;
    float *rm = dP + TQ * ldc, *rinv = rm + TQ, *rdel = rinv + TQ;
    int *rlo = reinterpret_cast<int *>(rdel + TQ), *rhi = rlo + TQ;
    uint64_t *rpb = reinterpret_cast<uint64_t *>(rhi + TQ);   // BIAS only (seg_lds)
    const int64_t row0 = (int64_t)blockIdx.x * TQ;
    seg_tile_ranges<BIAS, false>(off, n_seg, row0, TQ, N, rlo, rhi, pair_off, rpb);
    seg_stage(QKV, ldq, row0, N, 0, TQ, dp, Qs);
    seg_stage(dO, ldo, row0, N, 0, TQ, dp, dOs);
    {   // delta and the saved statistics of the tile's rows (zeros for rows >= N)
        const int tpr = SEG_THREADS / TQ, si = tid / tpr, sub = tid - si * tpr;
        const int64_t row = row0 + si;
        float d = 0.f;
        if (row < N)
            for (int c = sub; c < dq; c += tpr) {
                const float4 x = *reinterpret_cast<const float4 *>(dO + row * ldo + 4 * c);
                const float4 y = *reinterpret_cast<const float4 *>(O + row * ldo + 4 * c);
                d += (x.x * y.x + x.y * y.y) + (x.z * y.z + x.w * y.w);
            }
        d = seg_row_sum(d, tpr);
        if (sub == 0) {
            rdel[si] = d;
            rm[si] = row < N ? stats[2 * row] : 0.f;
            rinv[si] = row < N ? stats[2 * row + 1] : 0.f;
            if (row < rows_pad) delta_ws[row] = d;
        }
    }
    __syncthreads();
    int kbeg, kend;
    seg_union(rlo, rhi, TQ, kbeg, kend);
    const float ks = p > 0.f ? 1.f / (1.f - p) : 1.f;
    const int tk_sh = __ffs(TK) - 1;   // TK is a power of two
    const bool active = tid < dq * (TQ / RB);
    const int c4 = active ? tid % dq : 0, i0 = active ? (tid / dq) * RB : 0;
    float4 acc[RB];
#pragma unroll
    for (int r = 0; r < RB; ++r) acc[r] = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 pfk[SEG_PF], pfv[SEG_PF];
    if (kbeg < kend) {
        seg_fetch(QKV, ldq, kbeg, kend, dp, TK, dp, pfk);
        seg_fetch(QKV, ldq, kbeg, kend, 2 * dp, TK, dp, pfv);
    }
    for (int k0 = kbeg; k0 < kend; k0 += TK) {
        seg_put(Ks, TK, dp, pfk);
        seg_put(Vs, TK, dp, pfv);
        if (k0 + TK < kend) {   // the next tile's K and V: in flight during this tile's work
            seg_fetch(QKV, ldq, k0 + TK, kend, dp, TK, dp, pfk);
            seg_fetch(QKV, ldq, k0 + TK, kend, 2 * dp, TK, dp, pfv);
        }
        __syncthreads();
        seg_dots(Qs, Ks, TQ, TK, dp, S);
        seg_dots(dOs, Vs, TQ, TK, dp, dP);
        __syncthreads();
        for (int e = tid; e < TQ * TK; e += SEG_THREADS) {
            const int i = e >> tk_sh, j = e & (TK - 1), kj = k0 + j;
            float ds = 0.f;
            if (kj >= rlo[i] && kj < rhi[i]) {
                float s = S[i * ldc + j];
                uint64_t pe = 0;
                if constexpr (BIAS) {
                    pe = rpb[i] + (uint64_t)kj;
                    s += seg_pair_bias(bias, pe, n_pairs);
                }
                const float pv = expf(s - rm[i]) * rinv[i];
                const bool keep = p > 0.f ? u2gnn_keep(seed, (uint32_t)(row0 + i), (uint32_t)kj, p) : true;
                ds = pv * ((keep ? dP[i * ldc + j] * ks : 0.f) - rdel[i]);
                if constexpr (BIAS) {   // dL/dbias of the pair: each (i, kj) is formed here exactly once
                    if (dbias && pe < (uint64_t)n_pairs) dbias[pe] = ds;
                }
            }
            S[i * ldc + j] = ds;
        }
        __syncthreads();
        if (active) seg_accum<RB>(S, ldc, Ks, dp, i0, c4, min(TK, kend - k0), acc);
        __syncthreads();
    }
    if (active) {
#pragma unroll
        for (int r = 0; r < RB; ++r) {
            const int64_t row = row0 + i0 + r;
            if (row < rows_pad)
                *reinterpret_cast<float4 *>(dQKV + row * ldg + 4 * c4) =
                    make_float4(acc[r].x * q_scale, acc[r].y * q_scale, acc[r].z * q_scale, acc[r].w * q_scale);
        }
    }
}

// Backward over key tiles: the block owns TQ key rows (K, V images) and walks the query tiles of their segments
// (Q, dO images, the queries' statistics and delta): S^T = K Qs^T, dPd^T = V dO^T, then dK += dS^T Qs and
// dV += Pd^T dO.  dQKV[:, dp:3dp] = [dK | dV].
template <int RB, bool BIAS>
__global__ void __launch_bounds__(SEG_THREADS)
    segment_attn_bwd_kv_kernel(const float *QKV, int64_t ldq, int dp, const int64_t *off, int n_seg, const float *dO,
                               int64_t ldo, const float *stats, float p, uint64_t seed, const uint64_t *seed_epoch,
                               float *dQKV, int64_t ldg, const float *delta_ws, int64_t N, int64_t rows_pad, int TQ,
                               int TK, const float *bias, const int64_t *pair_off, int64_t n_pairs) {
    seed = u2gnn_seed(seed, seed_epoch);
    extern __shared__ __align__(16) float seg_sm[];
    const int LD = seg_ld(dp), dq = dp / 4, ldc = TK + 1, tid = threadIdx.x;
    float *Ks = seg_sm, *Vs = Ks + TQ * LD, *Qs = Vs + TQ * LD, *dOs = Qs + TK * LD;
    float *C1 = dOs + TK * LD, *C2 = C1 + TQ * ldc;   // dS^T, Pd^T: [own key][query]
    float *om = C2 + TQ * ldc, *oinv = om + TK, *odel = oinv + TK;
    int *rlo = reinterpret_cast<int *>(odel + TK), *rhi = rlo + TQ;
    uint64_t *rpb = reinterpret_cast<uint64_t *>(rhi + TQ);   // BIAS only (seg_lds)
    const int64_t row0 = (int64_t)blockIdx.x * TQ;
    seg_tile_ranges<BIAS, true>(off, n_seg, row0, TQ, N, rlo, rhi, pair_off, rpb);
    seg_stage(QKV, ldq, row0, N, dp, TQ, dp, Ks);
    seg_stage(QKV, ldq, row0, N, 2 * dp, TQ, dp, Vs);
    __syncthreads();
    int qbeg, qend;
    seg_union(rlo, rhi, TQ, qbeg, qend);
    const float ks = p > 0.f ? 1.f / (1.f - p) : 1.f;
    const int tk_sh = __ffs(TK) - 1;   // TK is a power of two
    const bool active = tid < dq * (TQ / RB);
    const int c4 = active ? tid % dq : 0, i0 = active ? (tid / dq) * RB : 0;
    float4 accK[RB], accV[RB];
#pragma unroll
    for (int r = 0; r < RB; ++r) accK[r] = accV[r] = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 pfq[SEG_PF], pfo[SEG_PF];
    if (qbeg < qend) {
        seg_fetch(QKV, ldq, qbeg, qend, 0, TK, dp, pfq);
        seg_fetch(dO, ldo, qbeg, qend, 0, TK, dp, pfo);
    }
    for (int q0 = qbeg; q0 < qend; q0 += TK) {
        seg_put(Qs, TK, dp, pfq);
        seg_put(dOs, TK, dp, pfo);
        if (q0 + TK < qend) {   // the next tile's Q and dO: in flight during this tile's work
            seg_fetch(QKV, ldq, q0 + TK, qend, 0, TK, dp, pfq);
            seg_fetch(dO, ldo, q0 + TK, qend, 0, TK, dp, pfo);
        }
        if (tid < TK) {
            const int64_t qi = (int64_t)q0 + tid;
            const bool in = qi < qend;
            om[tid] = in ? stats[2 * qi] : 0.f;
            oinv[tid] = in ? stats[2 * qi + 1] : 0.f;
            odel[tid] = in ? delta_ws[qi] : 0.f;
        }
        __syncthreads();
        seg_dots(Ks, Qs, TQ, TK, dp, C1);
        seg_dots(Vs, dOs, TQ, TK, dp, C2);
        __syncthreads();
        for (int e = tid; e < TQ * TK; e += SEG_THREADS) {
            const int j = e >> tk_sh, t = e & (TK - 1), qi = q0 + t;   // own key row j, query column t
            float ds = 0.f, pd = 0.f;
            if (qi >= rlo[j] && qi < rhi[j]) {
                float s = C1[j * ldc + t];
                if constexpr (BIAS)   // down a column of the segment's block: the lanes' queries are n floats apart
                    s += seg_pair_bias(bias, rpb[j] + (uint64_t)qi * (uint64_t)(rhi[j] - rlo[j]), n_pairs);
                const float pv = expf(s - om[t]) * oinv[t];
                const bool keep = p > 0.f ? u2gnn_keep(seed, (uint32_t)qi, (uint32_t)(row0 + j), p) : true;
                pd = keep ? pv * ks : 0.f;
                ds = pv * ((keep ? C2[j * ldc + t] * ks : 0.f) - odel[t]);
            }
            C1[j * ldc + t] = ds;
            C2[j * ldc + t] = pd;
        }
        __syncthreads();
        if (active) {
            const int tn = min(TK, qend - q0);
            seg_accum<RB>(C1, ldc, Qs, dp, i0, c4, tn, accK);
            seg_accum<RB>(C2, ldc, dOs, dp, i0, c4, tn, accV);
        }
        __syncthreads();
    }
    if (active) {
#pragma unroll
        for (int r = 0; r < RB; ++r) {
            const int64_t row = row0 + i0 + r;
            if (row < rows_pad) {
                *reinterpret_cast<float4 *>(dQKV + row * ldg + dp + 4 * c4) = accK[r];
                *reinterpret_cast<float4 *>(dQKV + row * ldg + 2 * dp + 4 * c4) = accV[r];
            }
        }
    }
}

// Tile heights by width, within the 160 KiB of LDS the window kernel documents: TQ rows of the block's own side (8
// above dp = 512, else 16), TK rows of the walked side: the largest of 64, 32, 16, 8 whose images fit.
// forward:  (TQ + TK) images + S;  backward: 2 (TQ + TK) images + two score matrices (the larger of the two launches)
struct SegTiles {
    int tq, tk, rb;
    size_t lds;
};
// BIAS adds the rows' entry bases (one uint64 per own row) and moves no tile choice: the tiles are chosen as without
// it, so a zero bias walks the same tiles in the same order and gives the plain kernels' bits
size_t seg_lds(int dp, int tq, int tk, bool bwd, bool bias = false) {
    const size_t LD = (size_t)seg_ld(dp);
    const size_t fl = bwd ? 2 * (size_t)(tq + tk) * LD + 2 * (size_t)tq * (tk + 1) + 3 * (size_t)std::max(tq, tk) + 2 * tq
                          : (size_t)(tq + tk) * LD + (size_t)tq * (tk + 1) + 3 * (size_t)tq;
    return (fl + (bias ? 2 * (size_t)tq : 0)) * sizeof(float);
}
SegTiles seg_tiles(int dp, bool bwd, bool bias = false) {
    SegTiles t;
    t.tq = dp > 512 ? 8 : 16;
    t.tk = 64;
    while (t.tk > 8 && seg_lds(dp, t.tq, t.tk, bwd) > SEG_LDS_LIMIT) t.tk >>= 1;
    // two blocks per CU hide each other's staging latency: a 32-row walked tile when that makes them fit
    if (t.tk == 64 && seg_lds(dp, t.tq, 64, bwd) > SEG_LDS_LIMIT / 2 && seg_lds(dp, t.tq, 32, bwd) <= SEG_LDS_LIMIT / 2)
        t.tk = 32;
    while (t.tk > 8 && t.tk * (dp / 4) > SEG_PF * SEG_THREADS) t.tk >>= 1;   // a walked tile fits the prefetch registers
    t.lds = seg_lds(dp, t.tq, t.tk, bwd, bias);
    // accumulator rows per thread: dq column groups x tq / rb row blocks within the block's 256 threads
    const int per = std::max(1, SEG_THREADS / (dp / 4));
    t.rb = 1;
    while (t.rb * per < t.tq) t.rb <<= 1;
    return t;
}

// dynamic LDS above 64 KiB is opted into per kernel and device (as window_attn.hip)
int seg_lds_optin(const void *kern) {
    static std::mutex mu;
    static std::set<std::pair<int, const void *>> done;
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return (int)e;
    std::lock_guard<std::mutex> lk(mu);
    if (done.count({dev, kern})) return U2GNN_OK;
    e = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)SEG_LDS_LIMIT);
    if (e != hipSuccess) return (int)e;
    done.insert({dev, kern});
    return U2GNN_OK;
}

int seg_check(const void *a, const void *b, const void *c, const void *d, int32_t dp, int32_t n_seg, float p, int64_t N,
              int64_t rows_pad) {
    if (!a || !b || !c || !d || n_seg < 1 || dp < 64 || (dp % 64) || !(p >= 0.f && p < 1.f)) return U2GNN_E_ARG;
    if (N < 1 || rows_pad < N || rows_pad > INT_MAX) return U2GNN_E_ARG;
    if (dp > 1024) return U2GNN_E_SHAPE;   // the executor's widest layer
    return U2GNN_OK;
}

// a bias needs its pair offsets and at least one pair, its gradient needs the bias
bool seg_bias_ok(const float *bias, const int64_t *pair_off, int64_t n_pairs, const float *dbias) {
    if (!bias) return dbias == nullptr;
    return pair_off && n_pairs >= 1;
}

#define U2GNN_TRY_SEG(x)                 \
    do {                                 \
        const int rc_ = (x);             \
        if (rc_ != U2GNN_OK) return rc_; \
    } while (0)

// one instantiation per accumulator row count, with and without the bias
#define SEG_DISPATCH_RB(rb, LAUNCH, B) \
    switch (rb) {                      \
        case 1: LAUNCH(1, B); break;   \
        case 2: LAUNCH(2, B); break;   \
        case 4: LAUNCH(4, B); break;   \
        case 8: LAUNCH(8, B); break;   \
        default: return U2GNN_E_SHAPE; \
    }
#define SEG_DISPATCH(rb, with_bias, LAUNCH)       \
    if (with_bias) {                              \
        SEG_DISPATCH_RB(rb, LAUNCH, true)         \
    } else {                                      \
        SEG_DISPATCH_RB(rb, LAUNCH, false)        \
    }

}  // namespace

extern "C" {

int u2gnn_segment_attn_fwd_bias(const float *QKV, int64_t ldq, int32_t dp, const int64_t *seg_offsets, int32_t n_seg,
                                const int64_t *pair_off, int64_t n_pairs, const float *bias, float *O, int64_t ldo,
                                float *stats, float p, uint64_t seed, int64_t N, int64_t rows_pad, void *stream) {
    U2GNN_TRY_SEG(seg_check(QKV, seg_offsets, O, stats, dp, n_seg, p, N, rows_pad));
    if (!seg_bias_ok(bias, pair_off, n_pairs, nullptr)) return U2GNN_E_ARG;
    if ((ldq & 3) || (ldo & 3) || ldq < 3 * (int64_t)dp || ldo < dp) return U2GNN_E_ARG;
    if (((uintptr_t)QKV & 15) || ((uintptr_t)O & 15) || ((uintptr_t)stats & 7)) return U2GNN_E_ALIGN;
    if (bias && (((uintptr_t)bias & 3) || ((uintptr_t)pair_off & 7))) return U2GNN_E_ALIGN;
    const SegTiles t = seg_tiles(dp, false, bias != nullptr);
    if (t.lds > SEG_LDS_LIMIT) return U2GNN_E_SHAPE;
    const unsigned grid = (unsigned)((rows_pad + t.tq - 1) / t.tq);
#define SEG_FWD(R, B)                                                                                               \
    do {                                                                                                            \
        auto kern = segment_attn_fwd_kernel<R, B>;                                                                  \
        U2GNN_TRY_SEG(seg_lds_optin(reinterpret_cast<const void *>(kern)));                                         \
        hipLaunchKernelGGL(kern, dim3(grid), dim3(SEG_THREADS), t.lds, u2gnn_stream(stream), QKV, ldq, (int)dp,      \
                           seg_offsets, (int)n_seg, O, ldo, stats, p, seed, u2gnn_cur_epoch(), N, rows_pad, t.tq, t.tk, \
                           bias, pair_off, n_pairs);                                                                \
    } while (0)
    SEG_DISPATCH(t.rb, bias != nullptr, SEG_FWD)
#undef SEG_FWD
    return u2gnn_launch_status();
}

int u2gnn_segment_attn_fwd(const float *QKV, int64_t ldq, int32_t dp, const int64_t *seg_offsets, int32_t n_seg,
                           float *O, int64_t ldo, float *stats, float p, uint64_t seed, int64_t N, int64_t rows_pad,
                           void *stream) {
    return u2gnn_segment_attn_fwd_bias(QKV, ldq, dp, seg_offsets, n_seg, nullptr, 0, nullptr, O, ldo, stats, p, seed, N,
                                       rows_pad, stream);
}

int u2gnn_segment_attn_bwd_bias(const float *QKV, int64_t ldq, int32_t dp, const int64_t *seg_offsets, int32_t n_seg,
                                const int64_t *pair_off, int64_t n_pairs, const float *bias, const float *O,
                                const float *dO, int64_t ldo, const float *stats, float p, uint64_t seed, float q_scale,
                                float *dQKV, int64_t ldg, float *delta_ws, float *dbias, int64_t N, int64_t rows_pad,
                                void *stream) {
    U2GNN_TRY_SEG(seg_check(QKV, seg_offsets, O, stats, dp, n_seg, p, N, rows_pad));
    if (!dO || !dQKV || !delta_ws || !seg_bias_ok(bias, pair_off, n_pairs, dbias)) return U2GNN_E_ARG;
    if ((ldq & 3) || (ldo & 3) || (ldg & 3) || ldq < 3 * (int64_t)dp || ldo < dp || ldg < 3 * (int64_t)dp)
        return U2GNN_E_ARG;
    if (((uintptr_t)QKV & 15) || ((uintptr_t)O & 15) || ((uintptr_t)dO & 15) || ((uintptr_t)dQKV & 15))
        return U2GNN_E_ALIGN;
    if (bias && (((uintptr_t)bias & 3) || ((uintptr_t)dbias & 3) || ((uintptr_t)pair_off & 7))) return U2GNN_E_ALIGN;
    const SegTiles t = seg_tiles(dp, true, bias != nullptr);
    if (t.lds > SEG_LDS_LIMIT) return U2GNN_E_SHAPE;
    const unsigned grid = (unsigned)((rows_pad + t.tq - 1) / t.tq);
#define SEG_BWD(R, B)                                                                                                \
    do {                                                                                                             \
        auto kq = segment_attn_bwd_q_kernel<R, B>;                                                                   \
        auto kkv = segment_attn_bwd_kv_kernel<R, B>;                                                                 \
        U2GNN_TRY_SEG(seg_lds_optin(reinterpret_cast<const void *>(kq)));                                            \
        U2GNN_TRY_SEG(seg_lds_optin(reinterpret_cast<const void *>(kkv)));                                           \
        hipLaunchKernelGGL(kq, dim3(grid), dim3(SEG_THREADS), t.lds, u2gnn_stream(stream), QKV, ldq, (int)dp,         \
                           seg_offsets, (int)n_seg, O, dO, ldo, stats, p, seed, u2gnn_cur_epoch(), q_scale, dQKV, ldg, \
                           delta_ws, N, rows_pad, t.tq, t.tk, bias, pair_off, n_pairs, dbias);                       \
        U2GNN_TRY_SEG(u2gnn_launch_status());                                                                        \
        hipLaunchKernelGGL(kkv, dim3(grid), dim3(SEG_THREADS), t.lds, u2gnn_stream(stream), QKV, ldq, (int)dp,        \
                           seg_offsets, (int)n_seg, dO, ldo, stats, p, seed, u2gnn_cur_epoch(), dQKV, ldg,           \
                           (const float *)delta_ws, N, rows_pad, t.tq, t.tk, bias, pair_off, n_pairs);               \
    } while (0)
    SEG_DISPATCH(t.rb, bias != nullptr, SEG_BWD)
#undef SEG_BWD
    return u2gnn_launch_status();
}

int u2gnn_segment_attn_bwd(const float *QKV, int64_t ldq, int32_t dp, const int64_t *seg_offsets, int32_t n_seg,
                           const float *O, const float *dO, int64_t ldo, const float *stats, float p, uint64_t seed,
                           float q_scale, float *dQKV, int64_t ldg, float *delta_ws, int64_t N, int64_t rows_pad,
                           void *stream) {
    return u2gnn_segment_attn_bwd_bias(QKV, ldq, dp, seg_offsets, n_seg, nullptr, 0, nullptr, O, dO, ldo, stats, p, seed,
                                       q_scale, dQKV, ldg, delta_ws, nullptr, N, rows_pad, stream);
}

}  // extern "C"
