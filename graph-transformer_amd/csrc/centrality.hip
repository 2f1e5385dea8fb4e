// The centrality encoding (a learned vector per node degree added to the stack's input) on gfx950:
//   u2gnn_gather_rows_emb   the stack's first gather with the table row of each gathered node added on the way
//                           (the kernels of u2gnn_gather_rows with their EMB flag set: gather_rows.h);
//   u2gnn_class_rows_grad   the table's gradient: the rows of layer (0, 0)'s input gradient summed per degree class,
//                           deterministic and atomic-free.
//
// u2gnn_class_rows_grad, two launches (RB = U2GNN_CLASS_ROWS_CHUNK = 256):
//   stage one   block (b, q) takes the RB consecutive rows [b RB, (b + 1) RB) x the 64 columns [64 q, 64 q + 64).
//               256 threads = 4 waves x 64 columns: wave w walks the rows b RB + w, + 4, + 8, ... in order (a row's
//               class is wave-uniform: one index and one degree load, broadcast), thread (w, c) adds its column of the
//               row into its own LDS cell acc[w][class][c] -- a chain of RB / 4 = 64 adds at most per cell, no cell
//               shared between threads, lane-consecutive addresses (no bank conflict).  Then per (class, column) the
//               fixed tree (acc[0] + acc[1]) + (acc[2] + acc[3]) (2 levels) -> ws[b][class][column].
//               LDS: 4 x n_classes x 64 floats = n_classes KB (dynamic; 64 KB at 64 classes: why n_classes <= 64, and
//               2 blocks of 4 waves per CU of the 160 KB there; the typical table of 17 classes leaves 8 blocks).
//   stage two   block (x, class) takes 16 columns: 256 threads = 16 lanes x 16 columns, lane l sums the chunks l, l + 16,
//               ... of its column in order (ceil(nchunks / 16) adds), then a fixed tree of 4 levels over the lanes ->
//               demb[class][column].  Every one of the n_classes x d outputs is stored (0 for a class without rows).
// A value therefore passes through at most K(n_rows) = 64 + 2 + ceil(ceil(n_rows / 256) / 16) + 4 sequential adds and
// tree levels (U2GNN_CLASS_ROWS_K; 71 up to 4096 rows, 87 at 68 374 rows), in an order fixed by the shapes alone.
#include "gather_rows.h"

namespace {

constexpr int RB = U2GNN_CLASS_ROWS_CHUNK;
constexpr int CR_LANES = 16;    // stage two: chunk lanes per column
constexpr int CR_FLIGHT = 16;   // stage one: rows of a wave whose loads are issued before the first add

template <int MODE>
__global__ void __launch_bounds__(256) gather_rows_emb_kernel(const float *__restrict__ src, int64_t ld_src,
                                                              int64_t src_rows, const int64_t *__restrict__ idx,
                                                              int64_t idx_stride, float *__restrict__ dst,
                                                              int64_t ld_dst, int64_t n_rows, int64_t n_rows_pad,
                                                              int64_t d, int64_t d_pad, int32_t *err,
                                                              const int32_t *__restrict__ deg,
                                                              const float *__restrict__ emb, int64_t ld_emb,
                                                              int n_classes) {
    gather_rows_body<MODE, true>(src, ld_src, src_rows, idx, idx_stride, dst, ld_dst, n_rows, n_rows_pad, d, d_pad, err,
                                 deg, emb, ld_emb, n_classes);
}

template <int GR_RPW, bool WIDE, bool XCD>
__global__ void __launch_bounds__(256) gather_rows_emb_multi_kernel(const float *__restrict__ src, int64_t ld_src,
                                                                    int64_t src_rows, const int64_t *__restrict__ idx,
                                                                    int64_t idx_stride, float *__restrict__ dst,
                                                                    int64_t ld_dst, int64_t n_rows, int64_t n_rows_pad,
                                                                    int64_t d, int64_t d_pad, int32_t *err,
                                                                    const int32_t *__restrict__ deg,
                                                                    const float *__restrict__ emb, int64_t ld_emb,
                                                                    int n_classes) {
    gather_rows_multi_body<GR_RPW, WIDE, XCD, true>(src, ld_src, src_rows, idx, idx_stride, dst, ld_dst, n_rows,
                                                    n_rows_pad, d, d_pad, err, deg, emb, ld_emb, n_classes);
}

// stage one (see the head of the file); ws [gridDim.x][n_classes][d]
__global__ void __launch_bounds__(256) class_rows_partial_kernel(const float *__restrict__ dX, int64_t ld,
                                                                 int64_t n_rows, int d,
                                                                 const int64_t *__restrict__ idx, int64_t idx_stride,
                                                                 const int32_t *__restrict__ deg, int64_t src_rows,
                                                                 int n_classes, float *__restrict__ ws) {
    extern __shared__ float acc[];   // [4][n_classes][64]
    const int w = threadIdx.x >> 6, c = threadIdx.x & 63;
    const int col = blockIdx.y * 64 + c;
    float *mine = acc + (int64_t)w * n_classes * 64 + c;
    for (int k = 0; k < n_classes; ++k) mine[k * 64] = 0.f;
    const int64_t row0 = (int64_t)blockIdx.x * RB;
    const int rows = (int)(n_rows - row0 < RB ? n_rows - row0 : RB);
    // CR_FLIGHT rows of the wave in flight, added in row order.  Every load is issued unconditionally at a clamped,
    // in-range address and the result selected afterwards: index -> degree is a chain of dependent loads, and a branch
    // per row made each row wait for the one before (the launch was latency-bound: 23 us whatever the shape)
    const int lc = col < d ? col : d - 1;
    for (int i = w; i < rows; i += 4 * CR_FLIGHT) {
        float v[CR_FLIGHT];
        int64_t s[CR_FLIGHT];
        int k[CR_FLIGHT];
#pragma unroll
        for (int u = 0; u < CR_FLIGHT; ++u) {
            const int r = i + 4 * u < rows ? i + 4 * u : rows - 1;
            s[u] = idx[(row0 + r) * idx_stride];
            v[u] = dX[(row0 + r) * ld + lc];
        }
#pragma unroll
        for (int u = 0; u < CR_FLIGHT; ++u) {
            const bool ok = i + 4 * u < rows && s[u] >= 0 && s[u] < src_rows;
            const int g = deg[ok ? s[u] : 0];
            k[u] = ok ? (g < 0 ? 0 : (g >= n_classes ? n_classes - 1 : g)) : -1;
        }
#pragma unroll
        for (int u = 0; u < CR_FLIGHT; ++u)
            if (k[u] >= 0 && col < d) mine[k[u] * 64] += v[u];
    }
    __syncthreads();
    const int cells = n_classes * 64, plane = n_classes * 64;
    float *out = ws + (int64_t)blockIdx.x * n_classes * d;
    for (int cell = threadIdx.x; cell < cells; cell += 256) {
        const int cc = blockIdx.y * 64 + (cell & 63);
        if (cc < d)
            out[(int64_t)(cell >> 6) * d + cc] =
                (acc[cell] + acc[plane + cell]) + (acc[2 * plane + cell] + acc[3 * plane + cell]);
    }
}

// stage two (see the head of the file)
__global__ void __launch_bounds__(256) class_rows_combine_kernel(const float *__restrict__ ws, int64_t nchunks, int d,
                                                                 int n_classes, float *__restrict__ demb,
                                                                 int64_t ld_demb) {
    __shared__ float part[CR_LANES][16];
    const int l = threadIdx.x >> 4, c = threadIdx.x & 15;
    const int col = blockIdx.x * 16 + c, k = blockIdx.y;
    float v = 0.f;
    if (col < d)
        for (int64_t b = l; b < nchunks; b += CR_LANES) v += ws[(b * n_classes + k) * d + col];
    part[l][c] = v;
    for (int s = CR_LANES / 2; s >= 1; s >>= 1) {
        __syncthreads();
        if (l < s) part[l][c] += part[l + s][c];
    }
    if (l == 0 && col < d) demb[(int64_t)k * ld_demb + col] = part[0][c];
}

inline int64_t class_rows_chunks(int64_t n_rows) { return (n_rows + RB - 1) / RB; }

}  // namespace

extern "C" {

int u2gnn_gather_rows_emb(const float *src, int64_t ld_src, int64_t src_rows, const int64_t *idx, int64_t idx_stride,
                          float *dst, int64_t ld_dst, int64_t n_rows, int64_t n_rows_pad, int64_t d, int64_t d_pad,
                          const int32_t *deg, const float *emb, int64_t ld_emb, int32_t n_classes, int32_t *err,
                          void *stream) {
    if (!dst || (n_rows > 0 && (!src || !idx || !deg)) || n_rows > n_rows_pad || d > d_pad) return U2GNN_E_ARG;
    if (!emb || n_classes < 1 || ld_emb < d) return U2GNN_E_ARG;
    if (n_rows_pad == 0) return U2GNN_OK;
    const int64_t blocks = (n_rows_pad + 3) / 4;
    if (blocks > (1 << 30)) return U2GNN_E_SHAPE;
    const dim3 grid((unsigned)blocks);
    hipStream_t st = u2gnn_stream(stream);
    const bool emb16 = (reinterpret_cast<uintptr_t>(emb) & 15) == 0 && (ld_emb & 3) == 0;
    const int route = gather_rows_route(src, ld_src, dst, ld_dst, d_pad, emb16);
#define EMB_ARGS src, ld_src, src_rows, idx, idx_stride, dst, ld_dst, n_rows, n_rows_pad, d, d_pad, err, deg, emb, \
                 ld_emb, (int)n_classes
    if (route == 1)
        hipLaunchKernelGGL(gather_rows_emb_kernel<1>, grid, dim3(256), 0, st, EMB_ARGS);
    else if (route >= 3) {
        // gridDim.x a multiple of 8 for the XCD order (surplus blocks find no rows and return)
        const dim3 g8(((unsigned)blocks + 7u) / 8u * 8u);
        if (route == 3)
            hipLaunchKernelGGL((gather_rows_emb_multi_kernel<1, false, true>), g8, dim3(256), 0, st, EMB_ARGS);
        else
            hipLaunchKernelGGL((gather_rows_emb_multi_kernel<1, true, true>), g8, dim3(256), 0, st, EMB_ARGS);
    } else if (route == 2)
        hipLaunchKernelGGL(gather_rows_emb_kernel<2>, grid, dim3(256), 0, st, EMB_ARGS);
    else
        hipLaunchKernelGGL(gather_rows_emb_kernel<0>, grid, dim3(256), 0, st, EMB_ARGS);
#undef EMB_ARGS
    return u2gnn_launch_status();
}

int64_t u2gnn_class_rows_grad_ws_floats(int64_t n_rows, int64_t d, int32_t n_classes) {
    if (n_rows < 0 || d < 1 || d > INT32_MAX || n_classes < 1 || n_classes > U2GNN_CLASS_ROWS_MAX) return -1;
    return class_rows_chunks(n_rows) * n_classes * d;
}

int u2gnn_class_rows_grad(const float *dX, int64_t ld, int64_t n_rows, int64_t d, const int64_t *idx,
                          int64_t idx_stride, const int32_t *deg, int64_t src_rows, int32_t n_classes, float *demb,
                          int64_t ld_demb, float *ws, int64_t ws_floats, void *stream) {
    if (!dX || !idx || !deg || !demb || !ws) return U2GNN_E_ARG;
    if (n_classes < 1 || n_classes > U2GNN_CLASS_ROWS_MAX || d < 1 || d > INT32_MAX || ld < d || ld_demb < d ||
        n_rows < 0 || src_rows < 0)
        return U2GNN_E_ARG;
    const int64_t nchunks = class_rows_chunks(n_rows);
    if (ws_floats < nchunks * n_classes * d) return U2GNN_E_ARG;
    if (nchunks > INT32_MAX || (d + 63) / 64 > 65535) return U2GNN_E_SHAPE;
    hipStream_t st = u2gnn_stream(stream);
    const int64_t nlive = src_rows > 0 ? nchunks : 0;   // no source row: every index is out of range, all sums are 0
    if (nlive > 0) {
        hipLaunchKernelGGL(class_rows_partial_kernel, dim3((unsigned)nchunks, (unsigned)((d + 63) / 64)), dim3(256),
                           (size_t)n_classes * 4 * 64 * sizeof(float), st, dX, ld, n_rows, (int)d, idx, idx_stride,
                           deg, src_rows, (int)n_classes, ws);
        const int rc = u2gnn_launch_status();
        if (rc != U2GNN_OK) return rc;
    }
    hipLaunchKernelGGL(class_rows_combine_kernel, dim3((unsigned)((d + 15) / 16), (unsigned)n_classes), dim3(256), 0,
                       st, (const float *)ws, nlive, (int)d, (int)n_classes, demb, ld_demb);
    return u2gnn_launch_status();
}

}  // extern "C"
