// The bodies of the a2 row gather, shared by u2gnn_gather_rows (encoder_ops.hip) and u2gnn_gather_rows_emb
// (centrality.hip).  EMB = false is the plain gather; EMB = true adds, to every real column of a row gathered from source
// row s, emb[clamp(deg[s], 0, n_classes - 1)][column] -- one IEEE add per element, padding and out-of-range rows stay
// zero.  The extra arguments are read under `if constexpr (EMB)` only, so the EMB = false instantiations compile to
// what they were before the flag existed (profiles/r12/gather_resource_usage.txt).
#pragma once
#include "u2gnn_common.h"

// the row of the table a source row takes (EMB only); deg: int32 [src_rows]
__device__ __forceinline__ const float *gather_emb_row(const int32_t *__restrict__ deg, const float *__restrict__ emb,
                                                       int64_t ld_emb, int n_classes, int64_t s) {
    int c = deg[s];
    c = c < 0 ? 0 : (c >= n_classes ? n_classes - 1 : c);
    return emb + (int64_t)c * ld_emb;
}

// ------------------------------------------------------------------------------------------
// a2 neighbour gather (pytorch_U2GNN_Sup.py:32,39): one wave per destination row, every source
// load of the row issued before its stores (restrict pointers, unrolled).  MODE 1: 16-byte
// source rows and destination rows, a float4 of columns per lane in each 256-column chunk (EMB: the table's rows
// 16-byte aligned too).  MODE 2: 4-byte-aligned source rows (X_concat with d = 367 starts rows at arbitrary 4-byte
// offsets): lane-consecutive 4-byte loads and stores, 16 columns per lane in flight.  Both need
// d_pad <= 1024.  MODE 0: the plain per-column loop for anything else.
// ------------------------------------------------------------------------------------------
template <int MODE, bool EMB>
__device__ __forceinline__ void gather_rows_body(const float *__restrict__ src, int64_t ld_src, int64_t src_rows,
                                                 const int64_t *__restrict__ idx, int64_t idx_stride,
                                                 float *__restrict__ dst, int64_t ld_dst, int64_t n_rows,
                                                 int64_t n_rows_pad, int64_t d, int64_t d_pad, int32_t *err,
                                                 const int32_t *__restrict__ deg, const float *__restrict__ emb,
                                                 int64_t ld_emb, int n_classes) {
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= n_rows_pad) return;
    float *o = dst + row * ld_dst;
    int64_t s = -1;
    if (row < n_rows) {
        s = idx[row * idx_stride];
        if (s < 0 || s >= src_rows) {
            if (lane == 0 && err) atomicExch(err, 1);
            s = -1;
        }
    }
    const float *in = src + (s < 0 ? 0 : s) * ld_src;
    const float *e = nullptr;
    if constexpr (EMB) e = s < 0 ? emb : gather_emb_row(deg, emb, ld_emb, n_classes, s);
    (void)e;
    if constexpr (MODE == 1) {
        float4 v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int c = 256 * j + 4 * lane;
            v[j] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (s < 0 || c >= d) continue;
            if (c + 3 < d) {
                v[j] = *reinterpret_cast<const float4 *>(in + c);
                if constexpr (EMB) {
                    const float4 t = *reinterpret_cast<const float4 *>(e + c);
                    v[j].x += t.x, v[j].y += t.y, v[j].z += t.z, v[j].w += t.w;
                }
            } else {
                v[j].x = in[c];
                if (c + 1 < d) v[j].y = in[c + 1];
                if (c + 2 < d) v[j].z = in[c + 2];
                if constexpr (EMB) {
                    v[j].x += e[c];
                    if (c + 1 < d) v[j].y += e[c + 1];
                    if (c + 2 < d) v[j].z += e[c + 2];
                }
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int c = 256 * j + 4 * lane;
            if (c < d_pad) *reinterpret_cast<float4 *>(o + c) = v[j];
        }
    } else if constexpr (MODE == 2) {
        float v[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int c = 64 * j + lane;
            if constexpr (EMB) v[j] = (s >= 0 && c < d) ? in[c] + e[c] : 0.f;
            else v[j] = (s >= 0 && c < d) ? in[c] : 0.f;
        }
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int c = 64 * j + lane;
            if (c < d_pad) o[c] = v[j];
        }
    } else {
        for (int64_t c = lane; c < d_pad; c += 64) {
            if constexpr (EMB) o[c] = (s >= 0 && c < d) ? in[c] + e[c] : 0.f;
            else o[c] = (s >= 0 && c < d) ? in[c] : 0.f;
        }
    }
}

// a2 gather for 4-byte-aligned source rows, d_pad <= 512 (X_concat, d = 367): GR_RPW rows per wave
// (their index loads, then all their source loads in flight), XCD-aware block order and, for WIDE,
// 16-byte stores -- each wave transposes its rows through a private LDS image (lane-consecutive
// 4-byte ds_write, ds_read_b128 of 4 consecutive columns per lane; both conflict-free), so a row
// leaves as 16-byte pieces instead of 6 x 256-B dword stores.  ld_dst % 4 == 0 and dst 16-byte
// aligned (checked by the caller); WIDE also needs d_pad % 4 == 0.
// Measured on one C4 batch (68374 x 367 -> [68608, 384], tools/gather_ab.py, profiles/r02/gather_ab.txt):
// one wave per row (MODE 2) 29.4 us; 2 rows/wave 24.7; + XCD order 21.6; + wide stores 18.6;
// 1 row/wave + XCD + wide 17.8 us (= 6.3 TB/s algorithmic; a 105 MB fill_ takes 14.8 us).  Wide stores
// alone, without the XCD order, lose (27.1 vs 26.2 us at 4 rows/wave); non-temporal stores lose too.
template <int GR_RPW, bool WIDE, bool XCD, bool EMB>
__device__ __forceinline__ void gather_rows_multi_body(const float *__restrict__ src, int64_t ld_src, int64_t src_rows,
                                                       const int64_t *__restrict__ idx, int64_t idx_stride,
                                                       float *__restrict__ dst, int64_t ld_dst, int64_t n_rows,
                                                       int64_t n_rows_pad, int64_t d, int64_t d_pad, int32_t *err,
                                                       const int32_t *__restrict__ deg,
                                                       const float *__restrict__ emb, int64_t ld_emb,
                                                       int n_classes) {
    __shared__ __attribute__((aligned(16))) float img[4][WIDE ? GR_RPW : 1][WIDE ? 512 : 4];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    // XCD: blocks are dealt round-robin to the 8 XCDs; remap so XCD x walks one contiguous eighth of
    // the rows (gridDim.x % 8 == 0) -- a graph's neighbour rows then stay in one XCD's L2
    const int64_t blk = XCD ? (int64_t)(blockIdx.x & 7) * (gridDim.x >> 3) + (blockIdx.x >> 3) : blockIdx.x;
    const int64_t row0 = (blk * 4 + w) * GR_RPW;
    if (row0 >= n_rows_pad) return;
    int64_t s[GR_RPW];
#pragma unroll
    for (int i = 0; i < GR_RPW; ++i) {
        const int64_t row = row0 + i;
        s[i] = -1;
        if (row < n_rows) {
            const int64_t t = idx[row * idx_stride];
            if (t < 0 || t >= src_rows) {
                if (lane == 0 && err) atomicExch(err, 1);
            } else {
                s[i] = t;
            }
        }
    }
    float v[GR_RPW][8];
#pragma unroll
    for (int i = 0; i < GR_RPW; ++i) {
        const float *in = src + (s[i] < 0 ? 0 : s[i]) * ld_src;
        if constexpr (EMB) {
            const float *e = s[i] < 0 ? emb : gather_emb_row(deg, emb, ld_emb, n_classes, s[i]);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int c = 64 * j + lane;
                v[i][j] = (s[i] >= 0 && c < d) ? in[c] + e[c] : 0.f;
            }
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int c = 64 * j + lane;
                v[i][j] = (s[i] >= 0 && c < d) ? in[c] : 0.f;
            }
        }
    }
    if constexpr (WIDE) {
#pragma unroll
        for (int i = 0; i < GR_RPW; ++i)
#pragma unroll
            for (int j = 0; j < 8; ++j) img[w][i][64 * j + lane] = v[i][j];
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int i = 0; i < GR_RPW; ++i) {
            const int64_t row = row0 + i;
            if (row >= n_rows_pad) break;
            float *o = dst + row * ld_dst;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int c = 256 * j + 4 * lane;
                if (c < d_pad) *reinterpret_cast<float4 *>(o + c) = *reinterpret_cast<const float4 *>(&img[w][i][c]);
            }
        }
    } else {
#pragma unroll
        for (int i = 0; i < GR_RPW; ++i) {
            const int64_t row = row0 + i;
            if (row >= n_rows_pad) break;
            float *o = dst + row * ld_dst;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int c = 64 * j + lane;
                if (c < d_pad) o[c] = v[i][j];
            }
        }
    }
}

// the route u2gnn_gather_rows takes for its arguments (u2gnn_gather_rows_emb: the same rule, MODE 1 also needing the
// table's rows 16-byte aligned): 1 = MODE 1; 3 / 4 = the multi-row XCD-ordered kernel with dword / wide stores;
// 2 = MODE 2; 0 = MODE 0
static inline int gather_rows_route(const void *src, int64_t ld_src, const void *dst, int64_t ld_dst, int64_t d_pad,
                                    bool emb_al16 = true) {
    auto al16 = [](const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
    const bool small = d_pad <= 1024;
    if (small && (d_pad & 3) == 0 && (ld_dst & 3) == 0 && al16(dst) && (ld_src & 3) == 0 && al16(src) && emb_al16)
        return 1;
    if (d_pad <= 512 && (ld_dst & 3) == 0 && al16(dst)) return (d_pad & 3) ? 3 : 4;
    return small ? 2 : 0;
}
