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
template <int MAXC, int U>
__global__ __launch_bounds__(CSR_THREADS) void csr_attn_fwd_kernel(
    const float *__restrict__ QKV, int64_t ldq, int nc, const int64_t *__restrict__ rowptr,
    const int64_t *__restrict__ colidx, int64_t nnz, float *__restrict__ O, int64_t ldo, float *__restrict__ stats,
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
#pragma unroll
    for (int u = 0; u < U; ++u) jn[u] = beg + u < end ? colidx[beg + u] : (int64_t)-1;
    for (int64_t e = beg; e < end; e += U) {
        int j[U];
        bool ok[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            ok[u] = jn[u] >= 0 && jn[u] < N;
            j[u] = ok[u] ? (int)jn[u] : 0;
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
        for (int u = 0; u < U; ++u) jn[u] = e + U + u < end ? colidx[e + U + u] : (int64_t)-1;
        float s[U], tmax = -INFINITY;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            float t = 0.f;
#pragma unroll
            for (int c = 0; c < MAXC; ++c)
                if (c < nc) t = dot4(q[c], k[u][c], t);
            t = grp_sum(t);
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
// edge_ws[e] = Pd_e, edge_ws[nnz + e] = dS_e = P_e (keep dPd_e / (1-p) - delta_i), dQ_i += dS_e K_j
template <int MAXC, int U>
__global__ __launch_bounds__(CSR_THREADS) void csr_attn_bwd_q_kernel(
    const float *__restrict__ QKV, int64_t ldq, int nc, const int64_t *__restrict__ rowptr,
    const int64_t *__restrict__ colidx, int64_t nnz, const float *__restrict__ O, const float *__restrict__ dO,
    int64_t ldo, const float *__restrict__ stats, float p, uint64_t seed, const uint64_t *seed_epoch, float q_scale,
    float *__restrict__ dQKV, int64_t ldg, float *__restrict__ edge_ws, int N, int rows_pad) {
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
#pragma unroll
    for (int u = 0; u < U; ++u) jn[u] = beg + u < end ? colidx[beg + u] : (int64_t)-1;
    for (int64_t e = beg; e < end; e += U) {
        int j[U];
        bool ok[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            ok[u] = jn[u] >= 0 && jn[u] < N;
            j[u] = ok[u] ? (int)jn[u] : 0;
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
        for (int u = 0; u < U; ++u) jn[u] = e + U + u < end ? colidx[e + U + u] : (int64_t)-1;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            float s = 0.f, t = 0.f;
#pragma unroll
            for (int c = 0; c < MAXC; ++c)
                if (c < nc) s = dot4(q[c], k[u][c], s), t = dot4(g[c], v[u][c], t);
            s = grp_sum(s);
            t = grp_sum(t);
            const float pv = ok[u] ? expf(s - rm) * rinv : 0.f;
            const bool keep = !drop || u2gnn_keep_rk(rkey, (uint32_t)j[u], thr);
            const float pd = keep ? pv * inv_keep : 0.f;
            const float ds = pv * ((keep ? t * inv_keep : 0.f) - delta);
            if (ln == 0 && e + u < end) edge_ws[e + u] = pd, edge_ws[nnz + e + u] = ds;
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
#define CSR_DISPATCH(nc, LAUNCH)          \
    do {                                  \
        if ((nc) <= 1) LAUNCH(1, 4);      \
        else if ((nc) <= 2) LAUNCH(2, 4); \
        else if ((nc) <= 4) LAUNCH(4, 2); \
        else if ((nc) <= 6) LAUNCH(6, 2); \
        else if ((nc) <= 8) LAUNCH(8, 2); \
        else LAUNCH(16, 1);               \
    } while (0)

}  // namespace

extern "C" {

int u2gnn_csr_attn_fwd(const float *QKV, int64_t ldq, int32_t dp, const u2gnn_csr_attn *A, float *O, int64_t ldo,
                       float *stats, float p, uint64_t seed, int64_t N, int64_t rows_pad, void *stream) {
    U2GNN_TRY_CSR(csr_check(QKV, O, stats, dp, p, N, rows_pad));
    if (!A || !A->rowptr || !A->colidx || A->nnz < 1) return U2GNN_E_ARG;
    if ((ldq & 3) || (ldo & 3) || ldq < 3 * (int64_t)dp || ldo < dp) return U2GNN_E_ARG;
    if (((uintptr_t)QKV & 15) || ((uintptr_t)O & 15) || ((uintptr_t)stats & 7)) return U2GNN_E_ALIGN;
    const unsigned grid = (unsigned)((rows_pad + CSR_ROWS - 1) / CSR_ROWS);
    const int nc = dp / 64;
#define CSR_FWD(C, UU)                                                                                              \
    hipLaunchKernelGGL((csr_attn_fwd_kernel<C, UU>), dim3(grid), dim3(CSR_THREADS), 0, u2gnn_stream(stream), QKV, ldq, \
                       nc, A->rowptr, A->colidx, A->nnz, O, ldo, stats, p, seed, u2gnn_cur_epoch(), (int)N,         \
                       (int)rows_pad)
    CSR_DISPATCH(nc, CSR_FWD);
#undef CSR_FWD
    return u2gnn_launch_status();
}

int u2gnn_csr_attn_bwd(const float *QKV, int64_t ldq, int32_t dp, const u2gnn_csr_attn *A, const float *O,
                       const float *dO, int64_t ldo, const float *stats, float p, uint64_t seed, float q_scale,
                       float *dQKV, int64_t ldg, float *edge_ws, int64_t N, int64_t rows_pad, void *stream) {
    U2GNN_TRY_CSR(csr_check(QKV, O, stats, dp, p, N, rows_pad));
    if (!dO || !dQKV || !edge_ws) return U2GNN_E_ARG;
    if (!A || !A->rowptr || !A->colidx || !A->t_rowptr || !A->t_src || !A->t_eid || A->nnz < 1) return U2GNN_E_ARG;
    if ((ldq & 3) || (ldo & 3) || (ldg & 3) || ldq < 3 * (int64_t)dp || ldo < dp || ldg < 3 * (int64_t)dp)
        return U2GNN_E_ARG;
    if (((uintptr_t)QKV & 15) || ((uintptr_t)O & 15) || ((uintptr_t)dO & 15) || ((uintptr_t)dQKV & 15) ||
        ((uintptr_t)edge_ws & 3))
        return U2GNN_E_ALIGN;
    const unsigned grid = (unsigned)((rows_pad + CSR_ROWS - 1) / CSR_ROWS);
    const int nc = dp / 64;
#define CSR_BWD_Q(C, UU)                                                                                             \
    hipLaunchKernelGGL((csr_attn_bwd_q_kernel<C, UU>), dim3(grid), dim3(CSR_THREADS), 0, u2gnn_stream(stream), QKV,    \
                       ldq, nc, A->rowptr, A->colidx, A->nnz, O, dO, ldo, stats, p, seed, u2gnn_cur_epoch(), q_scale, \
                       dQKV, ldg, edge_ws, (int)N, (int)rows_pad)
    CSR_DISPATCH(nc, CSR_BWD_Q);
#undef CSR_BWD_Q
    U2GNN_TRY_CSR(u2gnn_launch_status());
#define CSR_BWD_KV(C, UU)                                                                                            \
    hipLaunchKernelGGL((csr_attn_bwd_kv_kernel<C, UU>), dim3(grid), dim3(CSR_THREADS), 0, u2gnn_stream(stream), QKV,   \
                       ldq, nc, A->t_rowptr, A->t_src, A->t_eid, A->nnz, dO, ldo, dQKV, ldg,                          \
                       (const float *)edge_ws, (int)N, (int)rows_pad)
    CSR_DISPATCH(nc, CSR_BWD_KV);
#undef CSR_BWD_KV
    return u2gnn_launch_status();
}

}  // extern "C"
