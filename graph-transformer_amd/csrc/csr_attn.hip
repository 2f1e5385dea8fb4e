// Neighbour ("edges" mode) attention of U2GNN: node i attends over {i} and its graph neighbours, so the attention
// matrix of a mini-batch is its adjacency plus the diagonal, given as a CSR over the batch's rows: row i attends
// over the columns colidx[rowptr[i] .. rowptr[i+1]) of QKV [rows_pad, 3*dp] = [Q/sqrt(d) | K | V] (what the
// in-projection epilogue writes).
//
// The work, 2 * nnz * dp FLOP per product, is a gather: every entry (i, j) reads row j of K and of V once and
// nothing is reused between the entries of a row.  Exact fp32 on the vector ALUs under every precision policy, as
// the segment and window kernels.
//
// Shape: a group of 16 lanes owns one row (4 rows per wave, one wave per block), so the short rows of molecule
// graphs (degree 2-3) do not idle a wave.  A lane holds the columns 64 c + 4 ln .. + 3 (c < dp / 64) of its row's
// Q and accumulators in registers; a neighbour's K or V row is read as one float4 per lane and chunk (256
// contiguous bytes per group and instruction); a score is 16 partial sums combined by four DPP adds inside the
// group.  The walk takes U entries at a time, their loads issued together and the next step's indices loaded one
// step ahead.  Online softmax: any degree is legal and nothing is staged by degree.  The forward saves
// (max, 1 / sum exp) per row; the backward recomputes P from them.
//
// Determinism: no atomics.  The backward is two launches: one per query row (delta = rowsum(dO * O), the entries'
// Pd and dS into edge_ws, dQ), one per key row over the transposed lists (dK, dV); every output element is one
// fixed-order fp32 chain.
//
// Indices: the arrays live on the device only and any content is memory-safe: list bounds are clamped to
// [0, nnz], and an entry whose column, source row or entry id is out of range is skipped.  A column listed twice
// in a row counts twice.
//
// BIAS instantiations (u2gnn_csr_attn_*_bias): the score of entry e is Qs_i . K_j + bias[e], one float per entry in
// colidx order (a learned per-distance bias, expanded by bias_expand_kernel below), loaded with the column indices one
// step ahead; the backward's dS_e is dL/dbias[e] and also goes to dbias.  bias is indexed by the entry ids the walk
// already clamps, so any nnz floats are memory-safe.  The instantiations without BIAS are the kernels as they were.
#include "u2gnn_common.h"

#include <climits>

namespace {

constexpr int CSR_THREADS = 64;                          // one wave per block: the finest unit the dispatcher balances
constexpr int CSR_GROUP = 16;                            // lanes per row
constexpr int CSR_ROWS = CSR_THREADS / CSR_GROUP;        // rows per block

// the sum over the 16 lanes of a row group, left in every lane of it (all of them reach this together: the walk is
// uniform per group).  A group is one DPP row, so the four steps are VALU adds with a DPP operand -- lanes 1 and 2
// apart inside each quad (quad_perm), then the mirrored half row and the mirrored row, whose quads already hold
// their sums -- instead of the four LDS-crossbar round trips __shfl_xor compiles to (ds_bpermute_b32)
template <int CTRL>
__device__ __forceinline__ float dpp_add(float v) {
    return v + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, true));
}
__device__ __forceinline__ float grp_sum(float v) {
    static_assert(CSR_GROUP == 16, "one DPP row per group");
    v = dpp_add<0xB1>(v);    // quad_perm:[1,0,3,2]
    v = dpp_add<0x4E>(v);    // quad_perm:[2,3,0,1]
    v = dpp_add<0x141>(v);   // row_half_mirror
    return dpp_add<0x140>(v);   // row_mirror
}

__device__ __forceinline__ float dot4(const float4 &a, const float4 &b, float s) {
    s = fmaf(a.x, b.x, s);
    s = fmaf(a.y, b.y, s);
    s = fmaf(a.z, b.z, s);
    return fmaf(a.w, b.w, s);
}

__device__ __forceinline__ void axpy4(float a, const float4 &x, float4 &y) {
    y.x = fmaf(a, x.x, y.x);
    y.y = fmaf(a, x.y, y.y);
    y.z = fmaf(a, x.z, y.z);
    y.w = fmaf(a, x.w, y.w);
}

__device__ __forceinline__ float4 ld4(const float *p) { return *reinterpret_cast<const float4 *>(p); }
__device__ __forceinline__ void st4(float *p, const float4 &v) { *reinterpret_cast<float4 *>(p) = v; }

// the list [beg, end) of row r < n of a pointer array, clamped to [0, nnz]; empty for r >= n
__device__ __forceinline__ void csr_list(const int64_t *ptr, int r, int n, int64_t nnz, int64_t &beg, int64_t &end) {
    beg = end = 0;
    if (r >= n) return;
    beg = min(max(ptr[r], (int64_t)0), nnz);
    end = min(max(ptr[r + 1], (int64_t)0), nnz);
    if (end < beg) end = beg;
}

// MAXC: the register chunks per lane (nc = dp / 64 <= MAXC of them are live); U: entries per step of the walk
template <int MAXC, int U, bool BIAS>
__global__ __launch_bounds__(CSR_THREADS) void csr_attn_fwd_kernel(
    const float *__restrict__ QKV, int64_t ldq, int nc, const int64_t *__restrict__ rowptr,
    const int64_t *__restrict__ colidx, const float *__restrict__ bias, int64_t nnz, float *__restrict__ O, int64_t ldo, float *__restrict__ stats,
    float p, uint64_t seed, const uint64_t *seed_epoch, int N, int rows_pad) {
    const int ln = threadIdx.x & (CSR_GROUP - 1);
    const int i = blockIdx.x * CSR_ROWS + (threadIdx.x / CSR_GROUP);
    if (i >= rows_pad) return;
    const int dp = nc * 64;
    int64_t beg, end;
    csr_list(rowptr, i, N, nnz, beg, end);
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 q[MAXC], o[MAXC];
#pragma unroll
    for (int c = 0; c < MAXC; ++c) {
        o[c] = zero;
        q[c] = (c < nc && beg < end) ? ld4(QKV + (int64_t)i * ldq + 64 * c + 4 * ln) : zero;
    }
    seed = u2gnn_seed(seed, seed_epoch);
    const uint32_t rkey = u2gnn_row_key(seed, (uint32_t)i), thr = u2gnn_keep_thr(p);
    const bool drop = p > 0.f;
    const float inv_keep = drop ? 1.f / (1.f - p) : 1.f;
    float m_run = -INFINITY, l_run = 0.f;
    int64_t jn[U];   // the columns of the next step: loaded one step ahead, so a step waits for one round trip, not two
    float bn[U];     // BIAS: their biases, loaded with them
#pragma unroll
    for (int u = 0; u < U; ++u) {
        jn[u] = beg + u < end ? colidx[beg + u] : (int64_t)-1;
        if constexpr (BIAS) bn[u] = beg + u < end ? bias[beg + u] : 0.f;
    }
    for (int64_t e = beg; e < end; e += U) {
        int j[U];
        bool ok[U];
        float b[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            ok[u] = jn[u] >= 0 && jn[u] < N;
            j[u] = ok[u] ? (int)jn[u] : 0;
            if constexpr (BIAS) b[u] = bn[u];
        }
        float4 k[U][MAXC], v[U][MAXC];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const float *kr = QKV + (int64_t)j[u] * ldq + dp + 4 * ln;
#pragma unroll
            for (int c = 0; c < MAXC; ++c) {
                const bool live = c < nc && ok[u];
                k[u][c] = live ? ld4(kr + 64 * c) : zero;
                v[u][c] = live ? ld4(kr + dp + 64 * c) : zero;
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            jn[u] = e + U + u < end ? colidx[e + U + u] : (int64_t)-1;
            if constexpr (BIAS) bn[u] = e + U + u < end ? bias[e + U + u] : 0.f;
        }
        float s[U], tmax = -INFINITY;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            float t = 0.f;
#pragma unroll
            for (int c = 0; c < MAXC; ++c)
                if (c < nc) t = dot4(q[c], k[u][c], t);
            t = grp_sum(t);
            if constexpr (BIAS) t += b[u];
            s[u] = ok[u] ? t : -INFINITY;
            tmax = fmaxf(tmax, s[u]);
        }
        const float m_new = fmaxf(m_run, tmax);
        if (m_new == -INFINITY) continue;   // nothing legal so far (uniform over the group)
        const float a = m_run == -INFINITY ? 0.f : expf(m_run - m_new);
        l_run *= a;
#pragma unroll
        for (int c = 0; c < MAXC; ++c) o[c].x *= a, o[c].y *= a, o[c].z *= a, o[c].w *= a;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const float pv = ok[u] ? expf(s[u] - m_new) : 0.f;
            l_run += pv;
            const float pd = (drop && !u2gnn_keep_rk(rkey, (uint32_t)j[u], thr)) ? 0.f : pv * inv_keep;
#pragma unroll
            for (int c = 0; c < MAXC; ++c)
                if (c < nc) axpy4(pd, v[u][c], o[c]);
        }
        m_run = m_new;
    }
    const float rinv = l_run > 0.f ? 1.f / l_run : 0.f;
#pragma unroll
    for (int c = 0; c < MAXC; ++c)
        if (c < nc)
            st4(O + (int64_t)i * ldo + 64 * c + 4 * ln,
                make_float4(o[c].x * rinv, o[c].y * rinv, o[c].z * rinv, o[c].w * rinv));
    if (ln == 0) {
        stats[2 * (int64_t)i] = l_run > 0.f ? m_run : 0.f;
        stats[2 * (int64_t)i + 1] = rinv;
    }
}

// backward, launch 1: one group per query row.  delta_i, then per entry e = (i, j): P from the statistics,
// edge_ws[e] = Pd_e, edge_ws[nnz + e] = dS_e = P_e (keep dPd_e / (1-p) - delta_i), dQ_i += dS_e K_j.  BIAS: P with the
// forward's bias, and dbias[e] = dS_e when dbias is given
template <int MAXC, int U, bool BIAS>
__global__ __launch_bounds__(CSR_THREADS) void csr_attn_bwd_q_kernel(
    const float *__restrict__ QKV, int64_t ldq, int nc, const int64_t *__restrict__ rowptr,
    const int64_t *__restrict__ colidx, const float *__restrict__ bias, int64_t nnz, const float *__restrict__ O,
    const float *__restrict__ dO, int64_t ldo, const float *__restrict__ stats, float p, uint64_t seed,
    const uint64_t *seed_epoch, float q_scale, float *__restrict__ dQKV, int64_t ldg, float *__restrict__ edge_ws,
    float *__restrict__ dbias, int N, int rows_pad) {
    const int ln = threadIdx.x & (CSR_GROUP - 1);
    const int i = blockIdx.x * CSR_ROWS + (threadIdx.x / CSR_GROUP);
    if (i >= rows_pad) return;
    const int dp = nc * 64;
    int64_t beg, end;
    csr_list(rowptr, i, N, nnz, beg, end);
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 q[MAXC], g[MAXC], dq[MAXC];
    float delta = 0.f;
#pragma unroll
    for (int c = 0; c < MAXC; ++c) {
        const bool live = c < nc && beg < end;
        dq[c] = zero;
        q[c] = live ? ld4(QKV + (int64_t)i * ldq + 64 * c + 4 * ln) : zero;
        g[c] = live ? ld4(dO + (int64_t)i * ldo + 64 * c + 4 * ln) : zero;
        if (live) delta = dot4(g[c], ld4(O + (int64_t)i * ldo + 64 * c + 4 * ln), delta);
    }
    delta = grp_sum(delta);
    float rm = 0.f, rinv = 0.f;
    if (beg < end) rm = stats[2 * (int64_t)i], rinv = stats[2 * (int64_t)i + 1];
    seed = u2gnn_seed(seed, seed_epoch);
    const uint32_t rkey = u2gnn_row_key(seed, (uint32_t)i), thr = u2gnn_keep_thr(p);
    const bool drop = p > 0.f;
    const float inv_keep = drop ? 1.f / (1.f - p) : 1.f;
    int64_t jn[U];   // the columns of the next step: loaded one step ahead, so a step waits for one round trip, not two
    float bn[U];     // BIAS: their biases, loaded with them
#pragma unroll
    for (int u = 0; u < U; ++u) {
        jn[u] = beg + u < end ? colidx[beg + u] : (int64_t)-1;
        if constexpr (BIAS) bn[u] = beg + u < end ? bias[beg + u] : 0.f;
    }
    for (int64_t e = beg; e < end; e += U) {
        int j[U];
        bool ok[U];
        float b[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            ok[u] = jn[u] >= 0 && jn[u] < N;
            j[u] = ok[u] ? (int)jn[u] : 0;
            if constexpr (BIAS) b[u] = bn[u];
        }
        float4 k[U][MAXC], v[U][MAXC];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const float *kr = QKV + (int64_t)j[u] * ldq + dp + 4 * ln;
#pragma unroll
            for (int c = 0; c < MAXC; ++c) {
                const bool live = c < nc && ok[u];
                k[u][c] = live ? ld4(kr + 64 * c) : zero;
                v[u][c] = live ? ld4(kr + dp + 64 * c) : zero;
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            jn[u] = e + U + u < end ? colidx[e + U + u] : (int64_t)-1;
            if constexpr (BIAS) bn[u] = e + U + u < end ? bias[e + U + u] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            float s = 0.f, t = 0.f;
#pragma unroll
            for (int c = 0; c < MAXC; ++c)
                if (c < nc) s = dot4(q[c], k[u][c], s), t = dot4(g[c], v[u][c], t);
            s = grp_sum(s);
            t = grp_sum(t);
            if constexpr (BIAS) s += b[u];
            const float pv = ok[u] ? expf(s - rm) * rinv : 0.f;
            const bool keep = !drop || u2gnn_keep_rk(rkey, (uint32_t)j[u], thr);
            const float pd = keep ? pv * inv_keep : 0.f;
            const float ds = pv * ((keep ? t * inv_keep : 0.f) - delta);
            if (ln == 0 && e + u < end) {
                edge_ws[e + u] = pd, edge_ws[nnz + e + u] = ds;
                if constexpr (BIAS)
                    if (dbias) dbias[e + u] = ds;
            }
#pragma unroll
            for (int c = 0; c < MAXC; ++c)
                if (c < nc) axpy4(ds, k[u][c], dq[c]);
        }
    }
#pragma unroll
    for (int c = 0; c < MAXC; ++c)
        if (c < nc)
            st4(dQKV + (int64_t)i * ldg + 64 * c + 4 * ln,
                make_float4(dq[c].x * q_scale, dq[c].y * q_scale, dq[c].z * q_scale, dq[c].w * q_scale));
}

// backward, launch 2: one group per key row j over the transposed list: dK_j = sum dS_e Qs_src(e),
// dV_j = sum Pd_e dO_src(e)
template <int MAXC, int U>
__global__ __launch_bounds__(CSR_THREADS) void csr_attn_bwd_kv_kernel(
    const float *__restrict__ QKV, int64_t ldq, int nc, const int64_t *__restrict__ t_rowptr,
    const int64_t *__restrict__ t_src, const int64_t *__restrict__ t_eid, int64_t nnz, const float *__restrict__ dO,
    int64_t ldo, float *__restrict__ dQKV, int64_t ldg, const float *__restrict__ edge_ws, int N, int rows_pad) {
    const int ln = threadIdx.x & (CSR_GROUP - 1);
    const int jr = blockIdx.x * CSR_ROWS + (threadIdx.x / CSR_GROUP);
    if (jr >= rows_pad) return;
    const int dp = nc * 64;
    int64_t beg, end;
    csr_list(t_rowptr, jr, N, nnz, beg, end);
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 dk[MAXC], dv[MAXC];
#pragma unroll
    for (int c = 0; c < MAXC; ++c) dk[c] = dv[c] = zero;
    int64_t sn[U], en[U];   // the next step's source rows and entry ids, loaded one step ahead
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const bool in = beg + u < end;
        sn[u] = in ? t_src[beg + u] : (int64_t)-1, en[u] = in ? t_eid[beg + u] : (int64_t)-1;
    }
    for (int64_t t = beg; t < end; t += U) {
        int src[U];
        float ds[U], pd[U];
        bool ok[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t ss = sn[u], ee = en[u];
            ok[u] = ss >= 0 && ss < N && ee >= 0 && ee < nnz;
            src[u] = ok[u] ? (int)ss : 0;
            pd[u] = ok[u] ? edge_ws[ee] : 0.f;
            ds[u] = ok[u] ? edge_ws[nnz + ee] : 0.f;
        }
        float4 qs[U][MAXC], g[U][MAXC];
#pragma unroll
        for (int u = 0; u < U; ++u) {
#pragma unroll
            for (int c = 0; c < MAXC; ++c) {
                const bool live = c < nc && ok[u];
                qs[u][c] = live ? ld4(QKV + (int64_t)src[u] * ldq + 64 * c + 4 * ln) : zero;
                g[u][c] = live ? ld4(dO + (int64_t)src[u] * ldo + 64 * c + 4 * ln) : zero;
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const bool in = t + U + u < end;
            sn[u] = in ? t_src[t + U + u] : (int64_t)-1, en[u] = in ? t_eid[t + U + u] : (int64_t)-1;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
#pragma unroll
            for (int c = 0; c < MAXC; ++c)
                if (c < nc) axpy4(ds[u], qs[u][c], dk[c]), axpy4(pd[u], g[u][c], dv[c]);
        }
    }
#pragma unroll
    for (int c = 0; c < MAXC; ++c)
        if (c < nc) {
            st4(dQKV + (int64_t)jr * ldg + dp + 64 * c + 4 * ln, dk[c]);
            st4(dQKV + (int64_t)jr * ldg + 2 * dp + 64 * c + 4 * ln, dv[c]);
        }
}

// ---- the learned hop bias around the kernels above: tables [R][n_types] (one table per encoder layer, n_types =
// hops + 1 distances) <-> per-entry values [R][ld >= nnz] through etype [nnz] (the entry's shortest-path distance).
// Both directions are deterministic and atomic-free.
constexpr int BIAS_THREADS = 256;
constexpr int BIAS_GROUPS = 4;                                     // float4 groups per thread and block of stage one
constexpr int BIAS_CHUNK = BIAS_THREADS * BIAS_GROUPS * 4;         // entries per block of stage one
constexpr int BIAS_COMBINE_CHAIN = 128 - BIAS_GROUPS * 4;          // stage two: partials per thread (128 adds in all)

// out[r][e] = tables[r][etype[e]], 0 for a type outside [0, n_types)
__global__ __launch_bounds__(BIAS_THREADS) void bias_expand_kernel(const float *__restrict__ tables, int R, int n_types,
                                                                   const int32_t *__restrict__ etype, int64_t nnz,
                                                                   float *__restrict__ out, int64_t ld) {
    const int64_t e = (int64_t)blockIdx.x * BIAS_THREADS + threadIdx.x;
    if (e >= nnz) return;
    const int t = etype[e];
    const bool ok = t >= 0 && t < n_types;
    for (int r = 0; r < R; ++r) out[(int64_t)r * ld + e] = ok ? tables[r * n_types + t] : 0.f;
}

// acc[t][BIAS_THREADS] -> acc[t][0] = the sum over the threads, a fixed tree of 8 levels (all threads call it)
__device__ __forceinline__ void bias_tree(float *acc, int n_types) {
    for (int s = BIAS_THREADS / 2; s >= 1; s >>= 1) {
        __syncthreads();
        if ((int)threadIdx.x < s)
            for (int t = 0; t < n_types; ++t) acc[t * BIAS_THREADS + threadIdx.x] += acc[t * BIAS_THREADS + threadIdx.x + s];
    }
    __syncthreads();
}

// stage one: block (b, r) sums the entries [b * BIAS_CHUNK, + BIAS_CHUNK) of dbias row r per type: every thread walks
// its 4 float4 groups in order (a chain of 16 adds at most per type), then the tree; partial[(r * nblk + b)][t]
__global__ __launch_bounds__(BIAS_THREADS) void bias_table_grad_partial_kernel(
    const float *__restrict__ dbias, int64_t ld, int n_types, const int32_t *__restrict__ etype, int64_t nnz,
    float *__restrict__ partial) {
    __shared__ float acc[U2GNN_BIAS_TYPES_MAX * BIAS_THREADS];
    const int tid = threadIdx.x, r = blockIdx.y;
    for (int t = 0; t < n_types; ++t) acc[t * BIAS_THREADS + tid] = 0.f;
    const float *row = dbias + (int64_t)r * ld;
#pragma unroll
    for (int g = 0; g < BIAS_GROUPS; ++g) {
        const int64_t e = (int64_t)blockIdx.x * BIAS_CHUNK + ((int64_t)g * BIAS_THREADS + tid) * 4;
        if (e + 4 <= nnz) {
            const float4 v = ld4(row + e);
            const int4 ty = *reinterpret_cast<const int4 *>(etype + e);
            const float vv[4] = {v.x, v.y, v.z, v.w};
            const int tt[4] = {ty.x, ty.y, ty.z, ty.w};
#pragma unroll
            for (int x = 0; x < 4; ++x)
                if (tt[x] >= 0 && tt[x] < n_types) acc[tt[x] * BIAS_THREADS + tid] += vv[x];
        } else {
            for (int64_t x = e; x < nnz; ++x) {   // the last, partial group
                const int t = etype[x];
                if (t >= 0 && t < n_types) acc[t * BIAS_THREADS + tid] += row[x];
            }
        }
    }
    bias_tree(acc, n_types);
    if (tid < n_types) partial[((int64_t)r * gridDim.x + blockIdx.x) * n_types + tid] = acc[tid * BIAS_THREADS];
}

// stage two: block r sums its nblk partials per type: thread i takes the blocks i, i + 256, ... in order (at most
// BIAS_COMBINE_CHAIN of them), then the tree; dtables[r][t], every t < n_types written
__global__ __launch_bounds__(BIAS_THREADS) void bias_table_grad_combine_kernel(const float *__restrict__ partial,
                                                                              int64_t nblk, int n_types,
                                                                              float *__restrict__ dtables) {
    __shared__ float acc[U2GNN_BIAS_TYPES_MAX * BIAS_THREADS];
    const int tid = threadIdx.x, r = blockIdx.x;
    for (int t = 0; t < n_types; ++t) {
        float v = 0.f;
        for (int64_t b = tid; b < nblk; b += BIAS_THREADS) v += partial[((int64_t)r * nblk + b) * n_types + t];
        acc[t * BIAS_THREADS + tid] = v;
    }
    bias_tree(acc, n_types);
    if (tid < n_types) dtables[r * n_types + tid] = acc[tid * BIAS_THREADS];
}

// blocks of stage one; 0: a bad argument or more entries than the chain bound allows
int64_t bias_grad_blocks(int32_t R, int32_t n_types, int64_t nnz) {
    if (R < 1 || R > 65535 || n_types < 1 || n_types > U2GNN_BIAS_TYPES_MAX || nnz < 1) return 0;
    const int64_t nblk = (nnz + BIAS_CHUNK - 1) / BIAS_CHUNK;
    return nblk <= (int64_t)BIAS_COMBINE_CHAIN * BIAS_THREADS ? nblk : 0;
}

int csr_check(const void *a, const void *b, const void *c, int32_t dp, float p, int64_t N, int64_t rows_pad) {
    if (!a || !b || !c || dp < 64 || (dp % 64) || !(p >= 0.f && p < 1.f)) return U2GNN_E_ARG;
    if (N < 1 || rows_pad < N || rows_pad > INT_MAX) return U2GNN_E_ARG;
    if (dp > 1024) return U2GNN_E_SHAPE;   // the executor's widest layer
    return U2GNN_OK;
}

#define U2GNN_TRY_CSR(x)                 \
    do {                                 \
        const int rc_ = (x);             \
        if (rc_ != U2GNN_OK) return rc_; \
    } while (0)

// one instantiation per register-chunk bound (the smallest that holds dp / 64); wider rows walk fewer entries per
// step, so the loads in flight stay within the register file
#define CSR_DISPATCH(nc, LAUNCH, B)          \
    do {                                     \
        if ((nc) <= 1) LAUNCH(1, 4, B);      \
        else if ((nc) <= 2) LAUNCH(2, 4, B); \
        else if ((nc) <= 4) LAUNCH(4, 2, B); \
        else if ((nc) <= 6) LAUNCH(6, 2, B); \
        else if ((nc) <= 8) LAUNCH(8, 2, B); \
        else LAUNCH(16, 1, B);               \
    } while (0)

}  // namespace

extern "C" {

int u2gnn_csr_attn_fwd_bias(const float *QKV, int64_t ldq, int32_t dp, const u2gnn_csr_attn *A, const float *bias,
                            float *O, int64_t ldo, float *stats, float p, uint64_t seed, int64_t N, int64_t rows_pad,
                            void *stream) {
    U2GNN_TRY_CSR(csr_check(QKV, O, stats, dp, p, N, rows_pad));
    if (!A || !A->rowptr || !A->colidx || A->nnz < 1) return U2GNN_E_ARG;
    if ((ldq & 3) || (ldo & 3) || ldq < 3 * (int64_t)dp || ldo < dp) return U2GNN_E_ARG;
    if (((uintptr_t)QKV & 15) || ((uintptr_t)O & 15) || ((uintptr_t)stats & 7) || ((uintptr_t)bias & 3))
        return U2GNN_E_ALIGN;
    const unsigned grid = (unsigned)((rows_pad + CSR_ROWS - 1) / CSR_ROWS);
    const int nc = dp / 64;
#define CSR_FWD(C, UU, B)                                                                                           \
    hipLaunchKernelGGL((csr_attn_fwd_kernel<C, UU, B>), dim3(grid), dim3(CSR_THREADS), 0, u2gnn_stream(stream), QKV, \
                       ldq, nc, A->rowptr, A->colidx, bias, A->nnz, O, ldo, stats, p, seed, u2gnn_cur_epoch(),       \
                       (int)N, (int)rows_pad)
    if (bias) CSR_DISPATCH(nc, CSR_FWD, true);
    else CSR_DISPATCH(nc, CSR_FWD, false);
#undef CSR_FWD
    return u2gnn_launch_status();
}

int u2gnn_csr_attn_fwd(const float *QKV, int64_t ldq, int32_t dp, const u2gnn_csr_attn *A, float *O, int64_t ldo,
                       float *stats, float p, uint64_t seed, int64_t N, int64_t rows_pad, void *stream) {
    return u2gnn_csr_attn_fwd_bias(QKV, ldq, dp, A, nullptr, O, ldo, stats, p, seed, N, rows_pad, stream);
}

int u2gnn_csr_attn_bwd_bias(const float *QKV, int64_t ldq, int32_t dp, const u2gnn_csr_attn *A, const float *bias,
                            const float *O, const float *dO, int64_t ldo, const float *stats, float p, uint64_t seed,
                            float q_scale, float *dQKV, int64_t ldg, float *edge_ws, float *dbias, int64_t N,
                            int64_t rows_pad, void *stream) {
    U2GNN_TRY_CSR(csr_check(QKV, O, stats, dp, p, N, rows_pad));
    if (!dO || !dQKV || !edge_ws || (dbias && !bias)) return U2GNN_E_ARG;
    if (!A || !A->rowptr || !A->colidx || !A->t_rowptr || !A->t_src || !A->t_eid || A->nnz < 1) return U2GNN_E_ARG;
    if ((ldq & 3) || (ldo & 3) || (ldg & 3) || ldq < 3 * (int64_t)dp || ldo < dp || ldg < 3 * (int64_t)dp)
        return U2GNN_E_ARG;
    if (((uintptr_t)QKV & 15) || ((uintptr_t)O & 15) || ((uintptr_t)dO & 15) || ((uintptr_t)dQKV & 15) ||
        ((uintptr_t)edge_ws & 3) || ((uintptr_t)bias & 3) || ((uintptr_t)dbias & 3))
        return U2GNN_E_ALIGN;
    const unsigned grid = (unsigned)((rows_pad + CSR_ROWS - 1) / CSR_ROWS);
    const int nc = dp / 64;
#define CSR_BWD_Q(C, UU, B)                                                                                          \
    hipLaunchKernelGGL((csr_attn_bwd_q_kernel<C, UU, B>), dim3(grid), dim3(CSR_THREADS), 0, u2gnn_stream(stream), QKV, \
                       ldq, nc, A->rowptr, A->colidx, bias, A->nnz, O, dO, ldo, stats, p, seed, u2gnn_cur_epoch(),    \
                       q_scale, dQKV, ldg, edge_ws, dbias, (int)N, (int)rows_pad)
    if (bias) CSR_DISPATCH(nc, CSR_BWD_Q, true);
    else CSR_DISPATCH(nc, CSR_BWD_Q, false);
#undef CSR_BWD_Q
    U2GNN_TRY_CSR(u2gnn_launch_status());
#define CSR_BWD_KV(C, UU, B)                                                                                         \
    hipLaunchKernelGGL((csr_attn_bwd_kv_kernel<C, UU>), dim3(grid), dim3(CSR_THREADS), 0, u2gnn_stream(stream), QKV,   \
                       ldq, nc, A->t_rowptr, A->t_src, A->t_eid, A->nnz, dO, ldo, dQKV, ldg,                          \
                       (const float *)edge_ws, (int)N, (int)rows_pad)
    CSR_DISPATCH(nc, CSR_BWD_KV, false);
#undef CSR_BWD_KV
    return u2gnn_launch_status();
}

int u2gnn_csr_attn_bwd(const float *QKV, int64_t ldq, int32_t dp, const u2gnn_csr_attn *A, const float *O,
                       const float *dO, int64_t ldo, const float *stats, float p, uint64_t seed, float q_scale,
                       float *dQKV, int64_t ldg, float *edge_ws, int64_t N, int64_t rows_pad, void *stream) {
    return u2gnn_csr_attn_bwd_bias(QKV, ldq, dp, A, nullptr, O, dO, ldo, stats, p, seed, q_scale, dQKV, ldg, edge_ws,
                                   nullptr, N, rows_pad, stream);
}

int u2gnn_bias_expand(const float *tables, int32_t R, int32_t n_types, const int32_t *etype, int64_t nnz, float *out,
                      int64_t ld_out, void *stream) {
    if (!tables || !etype || !out || R < 1 || n_types < 1 || n_types > U2GNN_BIAS_TYPES_MAX || nnz < 1 || ld_out < nnz)
        return U2GNN_E_ARG;
    if (nnz > (int64_t)INT_MAX * BIAS_THREADS) return U2GNN_E_SHAPE;
    if (((uintptr_t)tables & 3) || ((uintptr_t)etype & 3) || ((uintptr_t)out & 3)) return U2GNN_E_ALIGN;
    const unsigned grid = (unsigned)((nnz + BIAS_THREADS - 1) / BIAS_THREADS);
    hipLaunchKernelGGL(bias_expand_kernel, dim3(grid), dim3(BIAS_THREADS), 0, u2gnn_stream(stream), tables, (int)R,
                       (int)n_types, etype, nnz, out, ld_out);
    return u2gnn_launch_status();
}

int64_t u2gnn_bias_table_grad_ws_floats(int32_t R, int32_t n_types, int64_t nnz) {
    const int64_t nblk = bias_grad_blocks(R, n_types, nnz);
    return nblk ? (int64_t)R * nblk * n_types : -1;
}

int u2gnn_bias_table_grad(const float *dbias, int64_t ld, int32_t R, int32_t n_types, const int32_t *etype, int64_t nnz,
                          float *dtables, float *ws, int64_t ws_floats, void *stream) {
    if (!dbias || !etype || !dtables || !ws || R < 1 || R > 65535 || n_types < 1 || n_types > U2GNN_BIAS_TYPES_MAX ||
        nnz < 1 || ld < nnz || (ld & 3))
        return U2GNN_E_ARG;
    const int64_t nblk = bias_grad_blocks(R, n_types, nnz);
    if (!nblk) return U2GNN_E_SHAPE;   // more entries than the 128-add chain bound covers
    if (ws_floats < (int64_t)R * nblk * n_types) return U2GNN_E_ARG;
    if (((uintptr_t)dbias & 15) || ((uintptr_t)etype & 15) || ((uintptr_t)dtables & 3) || ((uintptr_t)ws & 3))
        return U2GNN_E_ALIGN;
    hipLaunchKernelGGL(bias_table_grad_partial_kernel, dim3((unsigned)nblk, (unsigned)R), dim3(BIAS_THREADS), 0,
                       u2gnn_stream(stream), dbias, ld, (int)n_types, etype, nnz, ws);
    U2GNN_TRY_CSR(u2gnn_launch_status());
    hipLaunchKernelGGL(bias_table_grad_combine_kernel, dim3((unsigned)R), dim3(BIAS_THREADS), 0, u2gnn_stream(stream),
                       (const float *)ws, nblk, (int)n_types, dtables);
    return u2gnn_launch_status();
}

}  // extern "C"
