// A batch's attention pattern (u2gnn_csr_attn: rowptr, colidx, the transpose, the entry types) assembled on the
// device from the per-dataset structure u2gnn_graph_structure (include/u2gnn_hip.h): the adjacency of a batch is
// block-diagonal, so each of its arrays is the concatenation of its graphs' pieces, an entry moved by its slot's row
// offset (columns, source rows) or entry offset (row pointers, entry ids).  A segmented copy-with-offset: 13 bytes
// read and 28 written per entry, nothing reused.
//
// Shape: one launch.  The first blocks take ADJ_CHUNK consecutive batch entries each, the last ones ADJ_CHUNK
// consecutive batch rows (the N + 1 row pointers); thread t of a block handles the elements t, t + 256, ... of the
// chunk, so every load of the source arrays and every store is one contiguous run per wave.  The slot (graph of the
// batch) of a chunk's first element is found once per block by a binary search over ent_off / row_off; a thread
// reaches the slots of its own elements by stepping forward from there (its elements ascend, so it passes each slot
// of the chunk at most once -- no search per element).
//
// Determinism: no atomics; every output element is written by exactly one thread.
//
// Indices: every array lives on the device and any content is memory-safe.  A slot index stays inside [0, B); a
// graph id is checked against [0, G) before node_start / ent_start are read, a node against [0, V) and a source
// entry against [0, E) before the structure's arrays are.  An element that fails a check is written as -1 (entries)
// or as its slot's clamped offset (row pointers) and sets *err; every row pointer is clamped to [0, nnz].
#include "u2gnn_common.h"

#include <climits>

namespace {

constexpr int ADJ_THREADS = 256;
constexpr int ADJ_PER = 4;                                  // elements per thread
constexpr int ADJ_CHUNK = ADJ_THREADS * ADJ_PER;            // elements per block

struct AdjArgs {
    u2gnn_graph_structure S;
    const int64_t *gid, *row_off, *ent_off;
    int B;
    int64_t N, nnz;
    int64_t *rowptr, *colidx, *t_rowptr, *t_src, *t_eid;
    int32_t *etype, *err;
    unsigned ent_blocks;
};

// a + b without signed overflow (garbage offsets must stay defined behaviour; valid ones never wrap)
__device__ __forceinline__ int64_t wadd(int64_t a, int64_t b) { return (int64_t)((uint64_t)a + (uint64_t)b); }
__device__ __forceinline__ int64_t wsub(int64_t a, int64_t b) { return (int64_t)((uint64_t)a - (uint64_t)b); }
__device__ __forceinline__ int64_t clamp64(int64_t x, int64_t hi) { return x < 0 ? 0 : (x > hi ? hi : x); }

// the last slot b in [0, B) with off[b] <= x (0 when there is none); off: B + 1 values, ascending when valid
__device__ __forceinline__ int adj_slot(const int64_t *__restrict__ off, int B, int64_t x) {
    int lo = 0, hi = B - 1;
    while (lo < hi) {
        const int mid = lo + (hi - lo + 1) / 2;             // in [1, B - 1]
        if (off[mid] <= x) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// the slot of element x for a thread that stood at slot b: forward while the next slot starts at or before x
__device__ __forceinline__ int adj_advance(const int64_t *__restrict__ off, int B, int b, int64_t x) {
    while (b + 1 < B && off[b + 1] <= x) ++b;
    return b;
}

__global__ __launch_bounds__(ADJ_THREADS) void adjacency_assemble_kernel(const AdjArgs a) {
    __shared__ int s_slot;
    const u2gnn_graph_structure &S = a.S;
    const bool entries = blockIdx.x < a.ent_blocks;
    const int64_t base = (int64_t)(entries ? blockIdx.x : blockIdx.x - a.ent_blocks) * ADJ_CHUNK;
    const int64_t *__restrict__ off = entries ? a.ent_off : a.row_off;
    if (threadIdx.x == 0) s_slot = adj_slot(off, a.B, base);
    __syncthreads();
    int b = s_slot;
    if (entries) {
#pragma unroll
        for (int i = 0; i < ADJ_PER; ++i) {
            const int64_t e = base + i * ADJ_THREADS + threadIdx.x;
            if (e >= a.nnz) break;
            b = adj_advance(off, a.B, b, e);
            const int64_t eo = a.ent_off[b], ro = a.row_off[b], g = a.gid[b];
            int64_t c = -1, ts = -1, te = -1;
            int32_t ty = 0;
            bool ok = g >= 0 && g < S.G;
            int64_t s = 0;
            if (ok) {
                s = wadd(S.ent_start[g], wsub(e, eo));
                ok = s >= 0 && s < S.E;
            }
            if (ok) {
                c = wadd(S.col[s], ro);
                ts = wadd(S.t_src[s], ro);
                te = wadd(S.t_eid[s], eo);
                if (S.etype) ty = S.etype[s];
            } else {
                *a.err = 1;
            }
            a.colidx[e] = c;
            a.t_src[e] = ts;
            a.t_eid[e] = te;
            if (a.etype) a.etype[e] = ty;
        }
    } else {
#pragma unroll
        for (int i = 0; i < ADJ_PER; ++i) {
            const int64_t r = base + i * ADJ_THREADS + threadIdx.x;
            if (r > a.N) break;
            if (r == a.N) {
                a.rowptr[r] = a.nnz;
                a.t_rowptr[r] = a.nnz;
                break;
            }
            b = adj_advance(off, a.B, b, r);
            const int64_t eo = a.ent_off[b], g = a.gid[b];
            int64_t rp = eo, trp = eo;
            bool ok = g >= 0 && g < S.G;
            int64_t v = 0;
            if (ok) {
                v = wadd(S.node_start[g], wsub(r, a.row_off[b]));
                ok = v >= 0 && v < S.V;
            }
            if (ok) {
                const int64_t es = S.ent_start[g];
                rp = wadd(eo, wsub(S.rowptr[v], es));
                trp = wadd(eo, wsub(S.t_rowptr[v], es));
            } else {
                *a.err = 1;
            }
            a.rowptr[r] = clamp64(rp, a.nnz);
            a.t_rowptr[r] = clamp64(trp, a.nnz);
        }
    }
}

}  // namespace

extern "C" {

int u2gnn_adjacency_assemble(const u2gnn_graph_structure *S, const int64_t *gid, const int64_t *row_off,
                             const int64_t *ent_off, int32_t B, int64_t N, int64_t nnz, int64_t *rowptr,
                             int64_t *colidx, int64_t *t_rowptr, int64_t *t_src, int64_t *t_eid, int32_t *etype,
                             int32_t *err, void *stream) {
    if (!S || !S->node_start || !S->ent_start || !S->rowptr || !S->t_rowptr || !S->col || !S->t_src || !S->t_eid)
        return U2GNN_E_ARG;
    if (S->G < 1 || S->V < 1 || S->E < 1 || !gid || !row_off || !ent_off || B < 1 || N < 1 || nnz < 1) return U2GNN_E_ARG;
    if (!rowptr || !colidx || !t_rowptr || !t_src || !t_eid || !err || (etype && !S->etype)) return U2GNN_E_ARG;
    const int64_t ent_blocks = (nnz + ADJ_CHUNK - 1) / ADJ_CHUNK, row_blocks = (N + 1 + ADJ_CHUNK - 1) / ADJ_CHUNK;
    if (ent_blocks > INT_MAX || row_blocks > INT_MAX || ent_blocks + row_blocks > INT_MAX) return U2GNN_E_SHAPE;
    const void *p8[] = {S->node_start, S->ent_start, S->rowptr, S->t_rowptr, gid, row_off, ent_off, rowptr, colidx,
                        t_rowptr, t_src, t_eid};
    for (const void *p : p8)
        if ((uintptr_t)p & 7) return U2GNN_E_ALIGN;
    const void *p4[] = {S->col, S->t_src, S->t_eid, etype, err};
    for (const void *p : p4)
        if ((uintptr_t)p & 3) return U2GNN_E_ALIGN;
    AdjArgs a;
    a.S = *S;
    a.gid = gid, a.row_off = row_off, a.ent_off = ent_off;
    a.B = B, a.N = N, a.nnz = nnz;
    a.rowptr = rowptr, a.colidx = colidx, a.t_rowptr = t_rowptr, a.t_src = t_src, a.t_eid = t_eid;
    a.etype = etype, a.err = err;
    a.ent_blocks = (unsigned)ent_blocks;
    hipLaunchKernelGGL(adjacency_assemble_kernel, dim3((unsigned)(ent_blocks + row_blocks)), dim3(ADJ_THREADS), 0,
                       u2gnn_stream(stream), a);
    return u2gnn_launch_status();
}

}  // extern "C"
