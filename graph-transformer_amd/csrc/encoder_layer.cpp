// Native executor of one U2GNN encoder layer (torch TransformerEncoderLayer(d, nhead=1, ff,
// dropout), post-LN, slot-0 rows) — forward and backward issued from C++ straight onto HIP
// streams, one C-ABI call per layer instead of ~40 Python-side launches.
//
// Reference: pytorch_U2GNN_Sup.py:19-21,35 (UnSup: pytorch_U2GNN_UnSup.py:37-40,57) reach this
// through torch.nn.TransformerEncoder.  u2gnn_hip/engine.py issues the same kernels from Python, one call per
// launch, and takes every tile, split count and threshold from layer_plan / split_plan below
// (u2gnn_layer_plan, u2gnn_gemm_split_plan), hence bit-identical results: tests/test_native_layer_gpu.py.
//
// Memory: every buffer is caller-allocated.  The forward writes the tensors saved for the
// backward into a "ctx" arena and uses a scratch workspace for S and split-K slabs; the backward
// carves all of its temporaries from one workspace with a bump allocator that never reuses a
// byte within a call, so work left running on the side stream cannot be overwritten by the main
// stream.  Sizes come from the same code run in planning mode (no launches).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <algorithm>
#include <atomic>
#include <vector>

#include "u2gnn_hip.h"

namespace {

inline int64_t rup(int64_t x, int64_t m) { return (x + m - 1) / m * m; }

// padded rows: multiples of 256 from 1024 rows on (the N^2 products always get 256x128 blocks), else of 128
inline int64_t rows_pad(int64_t N) { return N >= 1024 ? rup(N, 256) : rup(N, 128); }

// the kernels that run a layer's attention core: make_dims decides, carve_ctx / layer_fwd / layer_bwd switch on it
enum class Attn {
    window,       // within each node's window of W rows (window_attn.hip)
    segments,     // per-graph: every row over the rows of its own segment (segment_attn.hip), exact fp32
    csr,          // neighbour attention: every row over the columns of its CSR row (csr_attn.hip), exact fp32
    // node attention, every row over all N rows:
    small,        // d <= 32, on the vector ALUs (u2gnn_attn_small_*, small_layer.hip): every precision, no N x N
                  // image -- the matrix-core products would be >= 50 % padding (dp = 64)
    fused,        // S = Q K^T, then one softmax -> dropout -> P.V pass (u2gnn_attn_softmax_pv, attn_fused.hip)
    three_pass,   // scores, softmax + dropout, P.V (fp32 parity path, dp > 384, few rows)
};

struct Dims {
    int64_t N, d, ff, Np, dp, ffp;
    int prec;
    int prec_ab;   // dS, dQ, dK products (U2GNN_LAYER_ATTN_BWD_BF16: plain bf16)
    int prec_fwd;  // forward products (U2GNN_LAYER_FWD_F32: exact fp32; U2GNN_LAYER_FWD_X6: bf16x6)
    bool deep_wgrad;
    int window;   // 0: attention over all N rows; W: within windows of W rows (N % W == 0)
    // per-graph attention (u2gnn_layer_*_seg): n_seg > 0 consecutive row segments, offsets on the device (null
    // while planning: the sizes depend on n_seg > 0 only)
    const int64_t *seg = nullptr;
    int n_seg = 0;
    // neighbour attention (u2gnn_layer_*_csr): csr_nnz > 0 entries of a CSR over the rows, arrays on the device (csr
    // null while planning: the sizes depend on csr_nnz only)
    const u2gnn_csr_attn *csr = nullptr;
    int64_t csr_nnz = 0;
    // its per-entry additive bias (u2gnn_layer_*_csrb): csr_nnz device floats, and where the backward leaves dL/dbias;
    // both caller-owned, null: none
    const float *csr_bias = nullptr;
    float *csr_dbias = nullptr;
    // the segments' per-pair additive bias (u2gnn_layer_*_segb): n_pairs device floats, segment g's pairs from
    // pair_off[g] (device), and where the backward leaves dL/dbias; caller-owned, null: none
    const int64_t *pair_off = nullptr;
    int64_t n_pairs = 0;
    const float *seg_bias = nullptr;
    float *seg_dbias = nullptr;
    Attn attn;   // set by make_dims; meaningful once pattern_ok has passed the pattern
};

// The attention pattern of a call (n_seg row segments, a CSR of nnz entries, or neither: the node-axis or window
// layer).  Segments: offsets and count, both or neither.  CSR: none, or a complete one with at least one entry.  Never
// the two together, and neither with window mode.  A bias only with a CSR, its gradient only with the bias.  The planning form (u2gnn_layer_sizes_*) has counts only and no
// pointers.  A per-pair bias only with segments, its pair offsets and at least one pair; its gradient only with it.
bool pattern_ok(const Dims &D, bool plan) {
    const bool segs = D.seg || D.n_seg, csr = D.csr || D.csr_nnz;
    if (D.n_seg < 0 || D.csr_nnz < 0 || (segs && csr) || ((segs || csr) && D.window != 0)) return false;
    if ((D.csr_bias && !csr) || (D.csr_dbias && !D.csr_bias)) return false;
    if ((D.seg_bias && !(segs && D.pair_off && D.n_pairs >= 1)) || (D.seg_dbias && !D.seg_bias)) return false;
    if (plan) return true;
    if (segs && !(D.seg && D.n_seg >= 1)) return false;
    const u2gnn_csr_attn *A = D.csr;
    return !csr || (A && A->rowptr && A->colidx && A->t_rowptr && A->t_src && A->t_eid && D.csr_nnz >= 1);
}

// the fused attention forward (u2gnn_attn_softmax_pv): node-axis attention in the matrix-core precisions with
// dp <= 384 and at least kFusedMinNp padded rows
// (f16x3 -- the fwdh policy -- runs fused: V as fp16 x2 rows from the in-projection, 3.024 vs 3.052 ms three-pass,
// profiles/r06/h3g_fused_ab.txt; bf16x6 -- the fwd6 policy -- keeps the three-pass form: its fused kernel, ran
// the C4 step at 3.42 / 3.43 ms against 3.40 unfused, and its exp2-based probabilities moved one boundary ReLU unit
// of the test seed's step across 0).  Few rows (C2's IMDBBINARY batches, Np = 128: ONE
// workgroup walks every key) run the three-pass form, whose GEMM tiles spread over more CUs: C2 fwdh 0.424 ms
// three-pass (r6h) vs 0.460 fused (r6i)
constexpr int64_t kFusedMinNp = 1024;

// a: checked by dims_ok; the pattern: to be checked by pattern_ok
Dims make_dims(const u2gnn_layer_dims *a, const int64_t *seg, int32_t n_seg, const u2gnn_csr_attn *csr, int64_t nnz,
               const float *bias = nullptr, float *dbias = nullptr) {
    Dims D;
    D.seg = seg, D.n_seg = n_seg, D.csr = csr, D.csr_nnz = nnz, D.csr_bias = bias, D.csr_dbias = dbias;
    D.N = a->N;
    D.d = a->d;
    D.ff = a->ff;
    D.Np = rows_pad(a->N);
    D.dp = rup(a->d, 64);
    D.ffp = rup(a->ff, 64);
    D.prec = a->precision;
    D.prec_ab = (a->precision == U2GNN_PREC_BF16X3 && (a->flags & U2GNN_LAYER_ATTN_BWD_BF16)) ? U2GNN_PREC_BF16
                                                                                             : a->precision;
    D.prec_fwd = a->precision;
    if (a->precision == U2GNN_PREC_BF16X3 && (a->flags & U2GNN_LAYER_FWD_F32)) D.prec_fwd = U2GNN_PREC_F32;
    if (a->precision == U2GNN_PREC_BF16X3 && (a->flags & U2GNN_LAYER_FWD_X6)) D.prec_fwd = U2GNN_PREC_BF16X6;
    if (a->precision == U2GNN_PREC_BF16X3 && (a->flags & U2GNN_LAYER_FWD_H3)) D.prec_fwd = U2GNN_PREC_F16X3;
    D.deep_wgrad = (a->flags & U2GNN_LAYER_DEEP_WGRAD) != 0;
    D.window = a->window;
    const bool fused = D.Np >= kFusedMinNp && D.prec_fwd != U2GNN_PREC_F32 && D.prec_fwd != U2GNN_PREC_BF16X6 &&
                       D.dp <= 384;
    if (D.window) D.attn = Attn::window;
    else if (n_seg) D.attn = Attn::segments;
    else if (nnz) D.attn = Attn::csr;
    else if (D.d <= 32) D.attn = Attn::small;
    else D.attn = fused ? Attn::fused : Attn::three_pass;
    return D;
}

// bump allocator over a caller buffer; plan mode (base == nullptr) only counts
struct Arena {
    char *base;
    int64_t used = 0, cap;
    bool overflow = false;
    Arena(void *b, int64_t c) : base(static_cast<char *>(b)), cap(c) {}
    template <typename T>
    T *take(int64_t n) {
        const int64_t bytes = rup(n * (int64_t)sizeof(T), 256);
        T *p = base ? reinterpret_cast<T *>(base + used) : nullptr;
        used += bytes;
        if (base && used > cap) overflow = true;
        return p;
    }
    bool plan() const { return base == nullptr; }
};

// U2GNN_DEBUG=1 in the environment names the failing call on stderr
bool debug_on() {
    static const int on = [] {
        const char *e = std::getenv("U2GNN_DEBUG");
        return e && e[0] == '1' ? 1 : 0;
    }();
    return on != 0;
}

#define U2GNN_TRY(x)                                                                                \
    do {                                                                                            \
        const int rc_ = (x);                                                                        \
        if (rc_ != U2GNN_OK) {                                                                      \
            if (debug_on()) std::fprintf(stderr, "u2gnn: %s:%d: %s -> %d\n", __FILE__, __LINE__, #x, rc_); \
            return rc_;                                                                             \
        }                                                                                           \
    } while (0)

struct Ctx {   // tensors saved by the forward for the backward
    // Pd: with dropout the signed probability image (P/(1-p) where kept, -P where dropped), else P
    float *QKV, *Pd, *O, *Z1, *X1, *mean1, *rstd1, *Hd, *Z2, *mean2, *rstd2;
    float *Psave;   // window mode: [N/W, W, W] probabilities
    // small-width node attention (d <= 32): its context (row statistics + compact Q, K, V); per-graph attention:
    // the rows' (max, 1 / sum exp) pairs, [Np][2]
    float *stats;
};

bool small_attn(const Dims &D) { return D.attn == Attn::small; }
bool fused_attn(const Dims &D) { return D.attn == Attn::fused; }
// node attention through the N x N image (fused or three-pass)
bool image_attn(const Dims &D) { return D.attn == Attn::fused || D.attn == Attn::three_pass; }
// the forward tail (a3.3 + a3.4) of a mid-width layer with few rows as one row-block kernel + the slab LayerNorm
// (mid_layer.hip; C2: 2 launches instead of 5)
bool mid_tail(const Dims &D) { return image_attn(D) && D.dp <= 256 && D.Np <= 512; }

Ctx carve_ctx(Arena &A, const Dims &D) {
    Ctx c;
    // the small-width path projects straight into its compact attention context: no [Np][3 dp] image
    c.QKV = small_attn(D) ? nullptr : A.take<float>(D.Np * 3 * D.dp);
    c.Pd = c.Psave = c.stats = nullptr;
    switch (D.attn) {
    case Attn::window: c.Psave = A.take<float>(D.N * D.window); break;
    case Attn::segments:
    case Attn::csr: c.stats = A.take<float>(2 * D.Np); break;
    case Attn::small: c.stats = A.take<float>(u2gnn_attn_small_ctx_floats(D.Np, D.d)); break;
    case Attn::fused:
    case Attn::three_pass: c.Pd = A.take<float>(D.Np * D.Np); break;
    }
    c.O = A.take<float>(D.Np * D.dp);
    c.Z1 = A.take<float>(D.Np * D.dp);
    c.X1 = A.take<float>(D.Np * D.dp);
    c.mean1 = A.take<float>(D.Np);
    c.rstd1 = A.take<float>(D.Np);
    c.Hd = A.take<float>(D.Np * D.ffp);
    c.Z2 = A.take<float>(D.Np * D.dp);
    c.mean2 = A.take<float>(D.Np);
    c.rstd2 = A.take<float>(D.Np);
    return c;
}

// live launch timing of one role (u2gnn_probe_arm / u2gnn_probe_collect): a diagnostic of the bench, the one
// piece of process-wide state of the executor.  Every access holds g_probe_mu (arm, mark and collect may come
// from different host threads); an unarmed probe costs one relaxed atomic load per mark.
struct Probe {
    int role = 0, cap = 0, n = 0;
    hipEvent_t *ev = nullptr;   // [2 * cap]: start, end
};
Probe g_probe;
std::mutex g_probe_mu;
std::atomic<int> g_probe_role{0};

void probe_mark(int role, bool end, hipStream_t st, bool plan) {
    if (plan || g_probe_role.load(std::memory_order_relaxed) != role) return;
    std::lock_guard<std::mutex> lk(g_probe_mu);
    if (g_probe.role != role || g_probe.n >= g_probe.cap) return;
    (void)hipEventRecord(g_probe.ev[2 * g_probe.n + (end ? 1 : 0)], st);
    if (end) ++g_probe.n;
}

// f16x3 operand pre-scale exponents (u2gnn_hip.h h3_exp_a / h3_exp_b): activations and weights (typical magnitudes
// 2^-5 .. 2^0) by 2^6; the probability image (entries ~1/N, at most 1/(1-p)) by 2^(15 - ceil(log2(1/(1-p)))), so
// that its largest entry stays below fp16's 65504 and its typical ones keep 22 bits
constexpr int32_t kH3Exp = 6;
int32_t h3_prob_exp(float pd) {
    int32_t e = 15;
    for (float m = 1.f / (1.f - pd); m > 1.f; m *= 0.5f) --e;
    return e;
}

struct G {   // one GEMM product (defaults = plain store): the launch arguments and what gemm_split reads beside them
    u2gnn_gemm_args a;
    int probe_role = 0;        // U2GNN_ROLE_*: the launch is bracketed by the probe's events
    bool accumulate = false;   // gemm_split: C += the product
    bool deep_k = false;       // gemm_split: weight gradient (split_plan: 16-deep K step, capped slabs)
    const int64_t *rblk = nullptr, *cblk = nullptr;   // gemm_split: {padded, real} block of C's rows / columns
    G(const float *A, const float *B, float *C, int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldb,
      int64_t ldc, int prec) {
        std::memset(&a, 0, sizeof(a));
        a.A = A, a.B = B, a.C = C, a.M = M, a.N = N, a.K = K, a.lda = lda, a.ldb = ldb, a.ldc = ldc;
        a.epilogue = U2GNN_EPI_STORE;
        a.split_k = 1;
        a.alpha = 1.f;
        a.precision = prec;
        if (prec == U2GNN_PREC_F16X3) a.h3_exp_a = a.h3_exp_b = kH3Exp;
    }
    G &ta() { a.trans_a = 1; return *this; }
    G &tb() { a.trans_b = 1; return *this; }
    G &epi(int e) { a.epilogue = e; return *this; }
    G &tile(int t) { a.tile = t; return *this; }
    G &alpha(float x) { a.alpha = x; return *this; }
    G &clamp(bool on) { a.clamp_a = on; return *this; }   // A elements below +0 read as 0 (the signed image as Pd)
    // f16x3 pre-scale exponent of A when it is not an activation (the probability image: h3_prob_exp)
    G &h3_a(int32_t e) { if (a.precision == U2GNN_PREC_F16X3) a.h3_exp_a = e; return *this; }
    G &role(int r) { probe_role = r; return *this; }
    G &accum() { accumulate = true; return *this; }
    G &deep() { deep_k = true; return *this; }
    G &blocks(const int64_t *r, const int64_t *c) { rblk = r, cblk = c; return *this; }
    int run(hipStream_t st, bool plan) {
        if (plan) return U2GNN_OK;
        if (probe_role) probe_mark(probe_role, false, st, plan);
        const int rc = u2gnn_gemm(&a, st);
        if (probe_role) probe_mark(probe_role, true, st, plan);
        return rc;
    }
};

// Reductions (and weight-gradient products) held back to the end of a latency-bound layer's backward,
// where they go out as one grouped GEMM launch and one u2gnn_reduce_batch call (<= 2 launches) instead
// of 12-16 launches of a few microseconds each (layer_bwd says which stream each list is flushed on).
// Every job computes the same bits as its immediate launch (u2gnn_hip.h, ABI v11).
struct Defer {
    std::vector<u2gnn_reduce_job> red;
    std::vector<u2gnn_gemm_args> gemm;
    std::vector<int> role;   // probe role of each held-back GEMM
    void hold(const G &g) { gemm.push_back(g.a), role.push_back(g.probe_role); }
};

int flush(Defer *df, Arena &W, hipStream_t st) {
    const bool plan = W.plan();
    for (size_t o = 0; o < df->gemm.size(); o += 8) {
        const size_t n = std::min<size_t>(8, df->gemm.size() - o);
        // a grouped launch is timed as a whole under each role it carries (u2gnn_probe_arm)
        int probed = 0;
        for (size_t i = o; i < o + n; ++i)
            if (df->role[i] && df->role[i] != probed) probed = df->role[i], probe_mark(probed, false, st, plan);
        if (!plan) U2GNN_TRY(u2gnn_gemm_group(df->gemm.data() + o, (int32_t)n, st));
        probed = 0;
        for (size_t i = o; i < o + n; ++i)
            if (df->role[i] && df->role[i] != probed) probed = df->role[i], probe_mark(probed, true, st, plan);
    }
    const int64_t wsf = u2gnn_reduce_batch_ws_floats(df->red.data(), (int32_t)df->red.size());
    if (wsf < 0) return U2GNN_E_ARG;
    float *ws = W.take<float>(wsf > 0 ? wsf : 1);
    if (!plan && !df->red.empty())
        U2GNN_TRY(u2gnn_reduce_batch(df->red.data(), (int32_t)df->red.size(), ws, wsf, st));
    df->red.clear();
    df->gemm.clear();
    df->role.clear();
    return U2GNN_OK;
}

u2gnn_reduce_job rjob(int kind) {
    u2gnn_reduce_job j;
    std::memset(&j, 0, sizeof(j));
    j.kind = kind;
    j.alpha = 1.f;
    return j;
}

struct Slabs {   // split-K partial sums left to their consumer (p null: the product was completed)
    float *p = nullptr;
    int64_t n = 0;
};
struct To {   // where a gemm_split product goes (defaults = launched and completed on st)
    hipStream_t st;
    Defer *held = nullptr;    // non-null: the launch and its slab reduce join this list's flush instead
    Slabs *slabs = nullptr;   // non-null: a split product leaves its slabs here instead of reducing them
    bool grouped = false;     // one of two products that share the grouped launch (dQ, dK)
    explicit To(hipStream_t s) : st(s) {}
    To &hold(Defer *df) { held = df; return *this; }
    To &pair() { grouped = true; return *this; }
    To &leave_slabs(Slabs *s) { slabs = s; return *this; }
};

// How gemm_split runs one product C[M,N] (+)= op(A) op(B) of depth Kd (u2gnn_hip.h u2gnn_split_plan): when the tile
// grid alone would leave most of the 256 CUs idle (skinny outputs with a deep node dimension: P.V, Pd^T.dO, dS.K,
// dS^T.Q, the weight gradients, dH.W1, dQKV.W_in) the depth is cut into fp32 slabs of >= 4 K steps.  Block targets:
// 448 for 64 / 128 tiles, 240 for 256x128 tiles (round-2 sweeps: 224 / 896 within noise, 120 / 300 / 460 slower on
// the 256x128 products).
struct SplitPlan {
    bool direct;
    int tile, launch_tile;
    int64_t split;
};
constexpr int64_t kSplitTarget = 448, kSplitTarget256 = 240;

SplitPlan split_plan(int64_t M, int64_t N, int64_t Kd, int prec, bool accumulate, bool deep, bool mapped, bool grouped,
                     bool deep_wgrad, bool held) {
    const bool f32 = prec == U2GNN_PREC_F32;
    const int64_t bk = f32 ? 16 : 32;
    // (tiny: an accumulating product of at most 16 tiles and 16 K steps -- C2's dX += dQKV W_in, 4 tiles --
    // runs as one short launch instead of 3 split-K blocks + a reduce launch)
    const bool tiny = accumulate && Kd <= 512 && (M / 64) * (N / 64) <= 16;
    if (!f32 && !deep && !mapped && Kd <= 2048 && M % 64 == 0 && N % 64 == 0 &&
        ((M / 64) * (N / 64) >= 256 || tiny)) {
        // shallow K (dH.W1, dQKV.W_in) with enough 64x64 tiles to fill the chip: no split, the
        // epilogue accumulates straight into C (no slabs, no reduce pass)
        const bool big = M % 256 == 0 && N % 128 == 0 && (M / 256) * (N / 128) >= U2GNN_BIG_TILE_BLOCKS;
        return {true, big ? 256 : 64, big ? 256 : 64, 1};
    }
    int t;
    int64_t tiles, target = kSplitTarget;
    if (!f32 && M % 256 == 0 && N % 128 == 0 && (M / 256) * (N / 128) >= 32) {
        // 256x128 blocks (8 waves, one block per CU): the skinny attention products
        t = 256, tiles = (M / 256) * (N / 128), target = kSplitTarget256;
        // dQ and dK go out as ONE grouped launch: half the block target each, so the launch holds ~240 blocks
        // (C4: split 2, 228 blocks instead of split 4 and 456; 3.016-3.017 vs 3.054-3.065 ms per step in one
        // session, profiles/r04/ab_sched.txt; split 1 and 128x128 tiles at split 2 were slower)
        if (grouped) target = kSplitTarget256 / 2;
    } else {
        t = (M % 128 == 0 && N % 128 == 0) ? 128 : 64;
        tiles = (M / t) * (N / t);
    }
    int64_t split = std::max<int64_t>(1, std::min(target / std::max<int64_t>(tiles, 1), Kd / (4 * bk)));
    if (deep && deep_wgrad && !f32 && t == 128) {
        // weight gradients (a few dozen 128x128 output tiles, K = the rows): the 16-deep K step runs 3 blocks per
        // CU.  Slab cap: at node-sized depths 8 slabs move half the bytes of 16 beside the main stream (C4 3.236 /
        // 3.238 vs 3.251 / 3.260 ms; 12: 3.26, 4: 3.27); token-sized depths (neighbour mode, K = N(k+1) rows) keep
        // 16 (8: 15.2 vs 13.9 ms)
        t = 129;
        split = std::max<int64_t>(1, std::min<int64_t>(target / std::max<int64_t>(tiles, 1), Kd <= 8192 ? 8 : 16));
    }
    // a held-back product joins its layer's grouped launch, whose kernels are the 64x64, 16-deep 128x128 and
    // 256x128 ones: a 128x128 job runs there as four 64x64 tiles (the split is chosen above, so the sums and
    // bits are the same; C2's dV, dQ, dK: one launch instead of three)
    // A launch of fewer than 64 blocks of 128x128 runs them as 64x64 tiles too (4x the blocks for the same
    // sums; C2's dX1 = dH W1: 8 blocks of a 4-step K loop, 8.6 us)
    // (bf16 precisions, whose 64x64 and 128x128 kernels form the same k-ordered sums)
    const bool lower = !f32 && t == 128 && (held || (M / 128) * (N / 128) * split < 64);
    return {false, t, lower ? 64 : t, split};
}

// deterministic split-K into fp32 slabs + one reduce pass (alpha, accumulate, padded->real block map), as
// split_plan decides.  g describes the finished product (its C, ldc, alpha and accumulate are the result's;
// deep = weight gradient), `to` where it goes.
int gemm_split(Arena &W, const Dims &D, G g, const To &to) {
    const int64_t M = g.a.M, N = g.a.N;
    const bool accumulate = g.accumulate, mapped = g.rblk != nullptr;
    hipStream_t st = to.st;
    Defer *df = to.held;
    const bool plan = W.plan();
    const SplitPlan sp = split_plan(M, N, g.a.K, g.a.precision, accumulate, g.deep_k, mapped, to.grouped, D.deep_wgrad,
                                    df != nullptr);
    const int64_t split = sp.split;
    g.epi(accumulate ? U2GNN_EPI_ACCUM : U2GNN_EPI_STORE);   // (the slab exit stores; its reduce accumulates)
    g.tile(sp.launch_tile);
    if (sp.direct) return g.run(st, plan);
    if (split == 1 && !mapped) {
        if (df && !accumulate) {
            df->hold(g);
            return U2GNN_OK;
        }
        return g.run(st, plan);
    }
    // split-K: the GEMM stores plain partial sums into slabs; alpha, accumulate and the block map are the reduce's
    float *slabs = W.take<float>(split * M * N);
    u2gnn_reduce_job j = rjob(U2GNN_RJOB_SLAB);
    j.src = slabs, j.n_slab = (int32_t)split, j.slab_stride = M * N, j.rows = M, j.cols = N, j.ld_src = N;
    j.rblk_pad = g.rblk ? g.rblk[0] : M, j.rblk_real = g.rblk ? g.rblk[1] : M;
    j.cblk_pad = g.cblk ? g.cblk[0] : N, j.cblk_real = g.cblk ? g.cblk[1] : N;
    j.dst = g.a.C, j.ld_dst = g.a.ldc, j.alpha = g.a.alpha, j.accumulate = accumulate ? 1 : 0;
    g.a.C = slabs, g.a.ldc = N, g.a.split_k = (int32_t)split, g.a.slab_stride = M * N;
    g.epi(U2GNN_EPI_STORE).alpha(1.f);
    if (df) {   // the GEMM and its slab reduce at the layer's flush
        df->hold(g);
        df->red.push_back(j);
        return U2GNN_OK;
    }
    U2GNN_TRY(g.run(st, plan));
    if (to.slabs) {   // the consumer sums the slabs itself (u2gnn_layernorm_bwd_delta_slabs)
        to.slabs->p = slabs, to.slabs->n = split;
        return U2GNN_OK;
    }
    if (plan) return U2GNN_OK;
    return u2gnn_slab_reduce(slabs, j.n_slab, j.slab_stride, M, N, N, j.rblk_pad, j.rblk_real, j.cblk_pad, j.cblk_real,
                             j.dst, j.ld_dst, j.alpha, j.accumulate, st);
}

// dst(real) = unpack(dY^T X), held back to df's flush
int wgrad(Arena &W, const Dims &D, const float *dY, int64_t ld_dy, const float *X, int64_t ld_x, int64_t m_pad,
          int64_t n_pad, float *dst, int64_t ld_dst, const int64_t *rblk, const int64_t *cblk, hipStream_t st,
          Defer *df) {
    G g(dY, X, dst, m_pad, n_pad, D.Np, ld_dy, ld_x, ld_dst, D.prec);
    return gemm_split(W, D, g.ta().blocks(rblk, cblk).deep(), To(st).hold(df));
}

// a column sum of dY as a job of the layer's flush
void bias_grad(Defer *df, const float *dY, int64_t rows, int64_t cols_pad, int64_t ld, int64_t cb0, int64_t cb1,
               float *out) {
    u2gnn_reduce_job j = rjob(U2GNN_RJOB_COLSUM);
    j.src = dY, j.rows = rows, j.cols = cols_pad, j.ld_src = ld, j.cblk_pad = cb0, j.cblk_real = cb1, j.dst = out;
    df->red.push_back(j);
}

// Fork / join events come from a per-device ring of pre-created events.  Re-recording an event is
// safe once the waits on its previous record are enqueued (a wait binds the record current at the
// call), and a ring of 256 is far longer than the hand-offs of one layer in flight.

// The hand-offs order work of ONE device: no system-scope fence when an event is recorded (the producing
// kernels' own releases make their stores visible to the other queue's kernels).  The record then stops
// holding back the next kernel of the recording stream: dO -> dS gap 13 -> 4.7 us, C4 step 2.963 / 2.958 vs
// 2.987 / 2.978 ms (device-scope release instead: 2.979 / 2.961; profiles/r04/ab_event_fence.txt)
// SAME-DEVICE ONLY: a pooled event may order only two streams of the device it was drawn for (the pools
// are per device, the main and side streams of one layer call share that device).  A cross-device or
// host-visible hand-off must use its own event without hipEventDisableSystemFence.
constexpr unsigned kForkEventFlags = hipEventDisableTiming | hipEventDisableSystemFence;

hipEvent_t pooled_event() {
    constexpr size_t kRing = 256;
    static std::mutex mu;
    static std::map<int, std::pair<std::vector<hipEvent_t>, size_t>> pools;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    std::lock_guard<std::mutex> lk(mu);
    auto &p = pools[dev];
    if (p.first.empty()) {
        p.first.resize(kRing, nullptr);
        for (auto &ev : p.first)
            if (hipEventCreateWithFlags(&ev, kForkEventFlags) != hipSuccess) {
                for (auto &x : p.first)
                    if (x) (void)hipEventDestroy(x);
                p.first.clear();
                return nullptr;
            }
    }
    return p.first[p.second++ % kRing];
}

// side-stream hand-off: the side stream waits for everything issued on main so far
struct Side {
    hipStream_t main, side;
    bool plan;
    int fork() {
        if (plan || side == main) return U2GNN_OK;
        hipEvent_t ev = pooled_event();
        if (!ev) return U2GNN_E_ARG;
        hipError_t e = hipEventRecord(ev, main);
        if (e == hipSuccess) e = hipStreamWaitEvent(side, ev, 0);
        return e == hipSuccess ? U2GNN_OK : (int)e;
    }
    // an event at the side stream's current position (joined later by wait(); nullptr when there
    // is no separate side stream)
    int mark(hipEvent_t *ev) {
        *ev = nullptr;
        if (plan || side == main) return U2GNN_OK;
        *ev = pooled_event();
        if (!*ev) return U2GNN_E_ARG;
        const hipError_t e = hipEventRecord(*ev, side);
        return e == hipSuccess ? U2GNN_OK : (int)e;
    }
    // the main stream waits for a mark() event
    int wait(hipEvent_t ev) {
        if (!ev) return U2GNN_OK;
        const hipError_t e = hipStreamWaitEvent(main, ev, 0);
        return e == hipSuccess ? U2GNN_OK : (int)e;
    }
};

// u2gnn_layernorm_bwd_params as a job of the layer's flush
void ln_params(Defer *df, const float *dY, const float *Z, const float *mean, const float *rstd, const float *dZd,
               int64_t ld, int64_t rows, int64_t d, int64_t dp, float *dgamma, float *dbeta, float *dbias) {
    u2gnn_reduce_job j = rjob(U2GNN_RJOB_LNPARAMS);
    j.src = dY, j.ld_src = ld, j.Z = Z, j.ldz = ld, j.mean = mean, j.rstd = rstd, j.dZdrop = dZd, j.lddrop = ld;
    j.rows = rows, j.d = d, j.cols = dp, j.dst = dgamma, j.dbeta = dbeta, j.dbias = dbias;
    df->red.push_back(j);
}

// Schedule decisions (each measured in rounds 1-2; the A/B switches are gone):
//  * dV = Pd^T dO runs on the side stream beside the dS -> dQ -> dK chain (-1.4 % step time);
//  * LayerNorm forward is fused into the bias-dropout-residual epilogue when one 64-column tile holds
//    whole rows (d <= 64, matrix-core precisions);
//  * delta = rowsum(dO * O) of the attention backward comes from LayerNorm1's backward
//    (u2gnn_layernorm_bwd_delta: sum_c dA * ((Z1 - X)(1-p) - b_o)) in the matrix-core precisions; the
//    fp32 parity path keeps u2gnn_rowdot, whose error does not grow with |X|.
void set_ln(u2gnn_gemm_args &a, const float *gamma, const float *beta, float *y, int64_t ldy, float *mean, float *rstd,
            int64_t d, int64_t rows) {
    a.ln_gamma = gamma, a.ln_beta = beta, a.ln_y = y, a.ln_ldy = ldy;
    a.ln_mean = mean, a.ln_rstd = rstd, a.ln_d = d, a.ln_rows = rows, a.ln_eps = 1e-5f;
}

// split-K depth of FFN2 in the matrix-core precisions (mfma), dp <= 256: with fewer than 128 output
// tiles of 64x64, aim at ~256 blocks of >= 4 K steps; u2gnn_slab_bias_drop_resid_ln then forms the bias,
// dropout, residual and LayerNorm2.  dp = 64 (C5 and the other
// fused-LayerNorm layers) since round 3; dp <= 256 since round 5: C2's IMDBBINARY batches (Np = 128,
// dp = 192) ran FFN2 as 6 blocks of a 32-step K loop, 16 us, plus a LayerNorm launch
int64_t ffn2_split(int64_t dp, bool mfma, int64_t Np, int64_t ffp) {
    const int64_t tiles = (Np / 64) * (dp / 64);
    if (!mfma || dp > 256 || tiles >= 128) return 1;
    int64_t sp = 256 / tiles;
    if (sp > ffp / 128) sp = ffp / 128;
    return sp > 1 ? sp : 1;
}

// tile of S = Q K^T: 256x128 blocks unless they would leave most CUs idle (C5's Np = 2048 gives 128 of
// them), then 128x128 (the same per-element sums: same bits)
int qk_tile(int64_t Np) { return (Np % 256 == 0 && (Np / 256) * (Np / 128) >= 256) ? 256 : 128; }
// ... and in the three-pass attention forward: 256x128 blocks where the rows allow, else the GEMM's own rule
int qk_tile_3pass(const Dims &D) { return (D.prec_fwd != U2GNN_PREC_F32 && D.Np % 256 == 0) ? 256 : 0; }
// tile of the in-projection: 256x128 blocks from 3 waves of them on (token-sized rows, neighbour mode), the GEMM's
// own rule below that: C4's 19 x 9 blocks of 256x128 leave a third of the CUs idle, its 76 x 18 64-tile blocks run
// the step 0.8 % faster (3/3 reps, profiles/r02/qkv_tile_ab.txt; bit-identical)
int in_proj_tile(const Dims &D) {
    return (D.prec_fwd != U2GNN_PREC_F32 && D.Np % 256 == 0 &&
            (D.Np / 256) * (3 * D.dp / 128) >= U2GNN_BIG_TILE_BLOCKS) ? 256 : 0;
}
// LayerNorm forward inside the bias-dropout-residual GEMM epilogue: one 64-column tile holds whole rows (d <= 64),
// matrix-core precisions
bool fused_ln(const Dims &D) { return D.dp == 64 && D.prec_fwd != U2GNN_PREC_F32; }
// one-stream layers in the matrix-core precisions: LayerNorm1's backward forms the attention backward's delta =
// rowsum(dO * O); the fp32 parity path keeps u2gnn_rowdot, whose error does not grow with |X|
bool ln1_forms_delta(const Dims &D) { return (small_attn(D) || image_attn(D)) && D.prec != U2GNN_PREC_F32; }

// every shape rule of the node-axis (or window) layer in one place: what u2gnn_layer_plan hands out
u2gnn_layer_rules layer_plan(const Dims &D, float p_drop) {
    u2gnn_layer_rules p;
    std::memset(&p, 0, sizeof(p));
    p.rows_pad = D.Np, p.dp = D.dp, p.ffp = D.ffp;
    p.ffn2_split = ffn2_split(D.dp, D.prec_fwd != U2GNN_PREC_F32, D.Np, D.ffp);
    p.small_attn = small_attn(D), p.mid_tail = mid_tail(D), p.fused_attn = fused_attn(D);
    p.qk_tile = qk_tile(D.Np), p.qk_tile_3pass = qk_tile_3pass(D), p.in_proj_tile = in_proj_tile(D);
    p.fused_ln = fused_ln(D), p.ln_delta = ln1_forms_delta(D);
    p.h3_exp = kH3Exp, p.h3_prob_exp = h3_prob_exp(p_drop);
    return p;
}

// the row-local tail of a small-width layer (u2gnn_layer_tail_small_*, small_layer.hip): every precision when the
// attention is the small-width one
u2gnn_small_tail_args tail_args(const Dims &D, const u2gnn_layer_params *w, const u2gnn_layer_seeds *s, const Ctx &c,
                                const float *X, float *X2) {
    u2gnn_small_tail_args t;
    std::memset(&t, 0, sizeof(t));
    t.n_valid = D.N, t.rows_pad = D.Np, t.d = D.d, t.dp = D.dp, t.ff = D.ff, t.ffp = D.ffp;
    t.p = s->p_drop, t.eps = 1e-5f;
    t.seed_drop1 = s->drop1, t.seed_dropff = s->dropff, t.seed_drop2 = s->drop2;
    t.W_o = w->W_o, t.b_o = w->b_o, t.n1_w = w->n1_w, t.n1_b = w->n1_b, t.W1 = w->W1, t.b1 = w->b1;
    t.W2 = w->W2, t.b2 = w->b2, t.n2_w = w->n2_w, t.n2_b = w->n2_b;
    t.O = c.O, t.X = X;
    t.Z1 = c.Z1, t.X1 = c.X1, t.mean1 = c.mean1, t.rstd1 = c.rstd1, t.Hd = c.Hd;
    t.Z2 = c.Z2, t.X2 = X2, t.mean2 = c.mean2, t.rstd2 = c.rstd2;
    return t;
}

int layer_fwd(const Dims &D, const u2gnn_layer_params *w, const u2gnn_layer_seeds *s, const float *X, float *X2,
              Arena &CA, Arena &W, bool need_ctx, hipStream_t st) {
    const int64_t N = D.N, Np = D.Np, d = D.d, dp = D.dp, ffp = D.ffp;
    const int prec = D.prec_fwd;
    const float pd = s->p_drop;
    const bool drop = pd > 0.f;
    const bool plan = W.plan();
    Ctx c = carve_ctx(need_ctx ? CA : W, D);
    const bool fused = fused_attn(D);
    // the in-projection output again in x2 format: the V tiles the fused softmax.P.V kernel reads (bf16x6: it reads
    // the fp32 output itself and splits V in registers, no copy)
    const bool x6 = prec == U2GNN_PREC_BF16X6;
    void *qkv2 = fused && !x6 ? static_cast<void *>(W.take<uint16_t>(Np * 6 * dp)) : nullptr;
    // a3.1 in-projection (+bias, Q scaled by 1/sqrt(d)); the small-width attention does its own
    if (!small_attn(D)) {
        G g(X, w->W_in, c.QKV, Np, 3 * dp, dp, dp, dp, 3 * dp, prec);
        g.tb().epi(U2GNN_EPI_BIAS).tile(in_proj_tile(D));
        g.a.bias = w->b_in;
        g.a.alpha = (float)(1.0 / std::sqrt((double)d));
        g.a.scale_cols = dp;
        // the x2 copy the fused softmax.P.V kernel reads: its V block only (Q and K are never read in x2)
        if (fused && !x6) g.a.Cx2 = qkv2, g.a.ldcx2 = 6 * dp, g.a.cx2_col0 = (int32_t)(2 * dp);
        U2GNN_TRY(g.run(st, plan));
    }
    const float *Q = c.QKV, *Kt = Q ? Q + dp : nullptr, *V = Q ? Q + 2 * dp : nullptr;   // (no image: small path)
    switch (D.attn) {
    case Attn::window:
        if (!plan)
            U2GNN_TRY(u2gnn_window_attn_fwd(c.QKV, 3 * dp, D.window, (int32_t)dp, c.O, dp, c.Psave, pd, s->attn,
                                            N / D.window, Np, st));
        break;
    case Attn::segments:
        if (!plan)
            U2GNN_TRY(u2gnn_segment_attn_fwd_bias(c.QKV, 3 * dp, (int32_t)dp, D.seg, D.n_seg, D.pair_off, D.n_pairs,
                                                  D.seg_bias, c.O, dp, c.stats, pd, s->attn, N, Np, st));
        break;
    case Attn::csr:
        if (!plan)
            U2GNN_TRY(u2gnn_csr_attn_fwd_bias(c.QKV, 3 * dp, (int32_t)dp, D.csr, D.csr_bias, c.O, dp, c.stats, pd,
                                              s->attn, N, Np, st));
        break;
    case Attn::small:
        // d <= 32: the whole layer on the vector ALUs (small_layer.hip): in-projection, softmax -> dropout -> P.V
        // flash-style (the row statistics and a compact Q, K, V saved) and a3.3 + a3.4 -- 2 or 3 launches
        if (!plan) {
            const u2gnn_small_tail_args t = tail_args(D, w, s, c, X, X2);
            probe_mark(U2GNN_ROLE_PV, false, st, plan);
            U2GNN_TRY(u2gnn_layer_small_fwd(&t, w->W_in, w->b_in, s->attn, c.stats, u2gnn_attn_small_ctx_floats(Np, d),
                                            st));
            probe_mark(U2GNN_ROLE_PV, true, st, plan);
        }
        break;
    case Attn::fused: {
        // a3.2 as S = Q K^T with the softmax row partials from the GEMM epilogue, then one fused
        // softmax -> dropout -> P.V pass that overwrites S with the signed image (attn_fused.hip)
        const int64_t ld_rp = Np / 32, groups = Np / 64;   // 64-column groups of the 256 / 128 tiles
        float *rowpart = W.take<float>(Np * 2 * ld_rp);
        float *pv_ws = W.take<float>(u2gnn_attn_softmax_pv_ws_floats(N, Np, dp));
        {
            G g(Q, Kt, c.Pd, Np, Np, dp, 3 * dp, 3 * dp, Np, prec);
            g.tb().epi(U2GNN_EPI_STORE_ROWSTAT).tile(qk_tile(Np)).role(U2GNN_ROLE_QK);
            g.a.rowpart = rowpart, g.a.ld_rowpart = ld_rp, g.a.n_valid = N;
            U2GNN_TRY(g.run(st, plan));
        }
        if (!plan) {
            probe_mark(U2GNN_ROLE_PV, false, st, plan);
            U2GNN_TRY(u2gnn_attn_softmax_pv(c.Pd, Np, rowpart, ld_rp, groups, x6 ? static_cast<const void *>(c.QKV) : qkv2,
                                            x6 ? 3 * dp : 6 * dp, dp, c.Pd, Np, c.O, dp, pv_ws,
                                            u2gnn_attn_softmax_pv_ws_floats(N, Np, dp), N, Np, pd, s->attn, prec, st));
            probe_mark(U2GNN_ROLE_PV, true, st, plan);
        }
        break;
    }
    case Attn::three_pass: {
        // a3.2 scores, softmax + dropout, P.V (fp32 parity path, dp > 384)
        float *S = W.take<float>(Np * Np);
        {
            G g(Q, Kt, S, Np, Np, dp, 3 * dp, 3 * dp, Np, prec);
            g.tb().tile(qk_tile_3pass(D)).role(U2GNN_ROLE_QK);
            U2GNN_TRY(g.run(st, plan));
        }
        if (!plan)
            U2GNN_TRY(u2gnn_attn_softmax_fwd(S, Np, drop ? nullptr : c.Pd, c.Pd, Np, N, Np, N, Np, pd, s->attn,
                                             nullptr, 0, st));
        U2GNN_TRY(gemm_split(W, D, G(c.Pd, V, c.O, Np, dp, Np, Np, 3 * dp, dp, prec).clamp(drop).h3_a(h3_prob_exp(pd))
                                       .role(U2GNN_ROLE_PV), To(st)));
        break;
    }
    }
    if (mid_tail(D)) {
        // a3.3 + a3.4 in two launches: out-projection .. FFN2 partials per row block and hidden chunk, then the
        // slab LayerNorm2 (mid_layer.hip)
        const int64_t wsf = u2gnn_layer_tail_mid_ws_floats(Np, dp, ffp);
        float *mws = W.take<float>(wsf > 0 ? wsf : 1);
        if (!plan) {
            const u2gnn_small_tail_args t = tail_args(D, w, s, c, X, X2);
            U2GNN_TRY(u2gnn_layer_tail_mid_fwd(&t, mws, wsf, st));
        }
    } else if (!small_attn(D)) {   // (the small-width layer: a3.3 + a3.4 ran in u2gnn_layer_small_fwd above)
        // a3.3 out-projection + dropout1 + residual, LayerNorm1
        const bool fuse_ln = fused_ln(D);
        {
            G g(c.O, w->W_o, c.Z1, Np, dp, dp, dp, dp, dp, prec);
            g.tb().epi(fuse_ln ? U2GNN_EPI_BIAS_DROP_RESID_LN : U2GNN_EPI_BIAS_DROP_RESID);
            g.a.bias = w->b_o, g.a.aux0 = X, g.a.ld_aux = dp, g.a.p_drop = pd, g.a.seed = s->drop1;
            if (fuse_ln) set_ln(g.a, w->n1_w, w->n1_b, c.X1, dp, c.mean1, c.rstd1, d, N);
            U2GNN_TRY(g.run(st, plan));
        }
        if (!plan && !fuse_ln)
            U2GNN_TRY(u2gnn_layernorm_fwd(c.Z1, dp, w->n1_w, w->n1_b, c.X1, dp, c.mean1, c.rstd1, N, Np, d, dp, 1e-5f, st));
        // a3.4 FFN + dropout2 + residual, LayerNorm2
        {
            G g(c.X1, w->W1, c.Hd, Np, ffp, dp, dp, dp, ffp, prec);
            g.tb().epi(U2GNN_EPI_BIAS_RELU_DROP);
            g.a.bias = w->b1, g.a.p_drop = pd, g.a.seed = s->dropff;
            U2GNN_TRY(g.run(st, plan));
        }
        const int64_t f2_split = ffn2_split(dp, prec != U2GNN_PREC_F32, Np, ffp);
        if (f2_split > 1) {
            // too few output tiles (C5: 32 of them, each a 32-step K loop): split-K slabs, then the
            // bias / dropout / residual / LayerNorm pass over the slabs
            float *slabs = W.take<float>(f2_split * Np * dp);
            G g(c.Hd, w->W2, slabs, Np, dp, ffp, ffp, ffp, dp, prec);
            g.tb().tile(64);
            g.a.split_k = (int32_t)f2_split, g.a.slab_stride = Np * dp;
            U2GNN_TRY(g.run(st, plan));
            if (!plan)
                U2GNN_TRY(u2gnn_slab_bias_drop_resid_ln(slabs, (int32_t)f2_split, Np * dp, dp, w->b2, c.X1, dp, pd,
                                                        s->drop2, c.Z2, dp, w->n2_w, w->n2_b, X2, dp, c.mean2, c.rstd2, d,
                                                        N, Np, 1e-5f, st));
        } else {
            G g(c.Hd, w->W2, c.Z2, Np, dp, ffp, ffp, ffp, dp, prec);
            g.tb().epi(fuse_ln ? U2GNN_EPI_BIAS_DROP_RESID_LN : U2GNN_EPI_BIAS_DROP_RESID);
            g.a.bias = w->b2, g.a.aux0 = c.X1, g.a.ld_aux = dp, g.a.p_drop = pd, g.a.seed = s->drop2;
            if (fuse_ln) set_ln(g.a, w->n2_w, w->n2_b, X2, dp, c.mean2, c.rstd2, d, N);
            U2GNN_TRY(g.run(st, plan));
        }
        if (!plan && !fuse_ln && f2_split <= 1)
            U2GNN_TRY(u2gnn_layernorm_fwd(c.Z2, dp, w->n2_w, w->n2_b, X2, dp, c.mean2, c.rstd2, N, Np, d, dp, 1e-5f, st));
    }
    if ((W.overflow || CA.overflow) && debug_on())
        std::fprintf(stderr, "u2gnn: layer_fwd arena overflow (ws %lld/%lld, ctx %lld/%lld)\n", (long long)W.used,
                     (long long)W.cap, (long long)CA.used, (long long)CA.cap);
    return (W.overflow || CA.overflow) ? U2GNN_E_ARG : U2GNN_OK;
}

int layer_bwd(const Dims &D, const u2gnn_layer_params *w, const u2gnn_layer_seeds *s, const float *X, Arena &CA,
              const float *dX2, float *dX, const u2gnn_layer_grads *g, Arena &W, hipStream_t st, hipStream_t side_st,
              bool need_dx = true) {
    const int64_t N = D.N, Np = D.Np, d = D.d, dp = D.dp, ff = D.ff, ffp = D.ffp;
    const int prec = D.prec;
    const float pd = s->p_drop;
    const bool plan = W.plan();
    Ctx c = carve_ctx(CA, D);
    Side sd{st, side_st ? side_st : st, plan};
    hipStream_t so = sd.side;
    // The parameter-gradient products and reductions are held back to the end of the layer (df) and go out
    // there as one grouped GEMM launch + one reduction batch: on the side stream, overlapping the next
    // layer's backward (C4: 3.141 / 3.147 / 3.159 vs 3.187 / 3.191 / 3.195 ms per step issued one by one
    // beside this layer, one session, profiles/r03/r3g_side_defer_ab.txt), or on this stream for one-stream
    // layers (C5: -10 launches per layer) and for the last layer of the backward.  The attention products
    // dQ, dK (and dV when it runs on this stream) go out as one grouped launch and their slab reduces as
    // one batch before the in-projection (att; C4 neutral, C5 -2 launches per layer).
    Defer defer_p, defer_a;
    Defer *df = &defer_p, *att = &defer_a;
    const int64_t blk_d[2] = {dp, d}, blk_ff[2] = {ffp, ff};
    const bool tail = small_attn(D);   // the row-local tail kernel (small_layer.hip) forms dX1 ... dO and delta
    const bool ln_delta = ln1_forms_delta(D);
    float *dX1 = W.take<float>(Np * dp), *dF = W.take<float>(Np * dp);
    float *dH = W.take<float>(Np * ffp);
    float *dA = W.take<float>(Np * dp);
    // no input gradient wanted (first layer of the stack): LN1's residual half goes to scratch and
    // the in-projection's dX GEMM below is skipped
    float *dX_scratch = W.take<float>(Np * dp);   // taken in every mode so the plan covers it
    if (!need_dx) dX = dX_scratch;
    float *delta_ln = (ln_delta || tail) ? W.take<float>(Np) : nullptr;
    float *dO = W.take<float>(Np * dp);
    float *small_dqkv = nullptr;   // the small-width layer's dQKV, written by u2gnn_layer_small_bwd
    if (tail) {
        // the tail backward and the attention backward (dQKV; dX += dQKV W_in unless no input gradient is
        // wanted) in 2 or 3 launches (small_layer.hip)
        small_dqkv = W.take<float>(Np * 3 * dp);
        const int64_t wsf = u2gnn_attn_small_ws_floats(N, Np, d);
        float *sa_ws = W.take<float>(wsf);
        if (!plan) {
            u2gnn_small_tail_args t = tail_args(D, w, s, c, X, nullptr);
            t.dX2 = dX2, t.dX1 = dX1, t.dF = dF, t.dH = dH, t.dX = dX, t.dA = dA, t.dO = dO, t.delta = delta_ln;
            probe_mark(U2GNN_ROLE_DS, false, st, plan);
            U2GNN_TRY(u2gnn_layer_small_bwd(&t, w->W_in, s->attn, c.stats, u2gnn_attn_small_ctx_floats(Np, d),
                                            small_dqkv, 3 * dp, need_dx ? 1 : 0, sa_ws, wsf, st));
            probe_mark(U2GNN_ROLE_DS, true, st, plan);
        }
        // the parameter gradients of the tail, held back (df) in the order of the matrix-core branch
        ln_params(df, dX2, c.Z2, c.mean2, c.rstd2, dF, dp, N, d, dp, g->n2_w, g->n2_b, g->l2_b);
        U2GNN_TRY(wgrad(W, D, dF, dp, c.Hd, ffp, dp, ffp, g->l2_w, ff, blk_d, blk_ff, so, df));
        U2GNN_TRY(wgrad(W, D, dH, ffp, c.X1, dp, ffp, dp, g->l1_w, d, blk_ff, blk_d, so, df));
        bias_grad(df, dH, Np, ffp, ffp, ffp, ff, g->l1_b);
        ln_params(df, dX1, c.Z1, c.mean1, c.rstd1, dA, dp, N, d, dp, g->n1_w, g->n1_b, g->out_b);
        U2GNN_TRY(wgrad(W, D, dA, dp, c.O, dp, dp, dp, g->out_w, d, blk_d, blk_d, so, df));
    } else {
        // LN2 backward -> dX1 (residual), dF (dropout2 branch); norm2 + linear2.bias grads (held back: df)
        if (!plan)
            U2GNN_TRY(u2gnn_layernorm_bwd(dX2, dp, c.Z2, dp, c.mean2, c.rstd2, w->n2_w, dX1, dp, dF, dp, pd, s->drop2,
                                          N, Np, d, dp, st));
        ln_params(df, dX2, c.Z2, c.mean2, c.rstd2, dF, dp, N, d, dp, g->n2_w, g->n2_b, g->l2_b);
        // FFN
        {
            G gg(dF, w->W2, dH, Np, ffp, dp, dp, ffp, ffp, prec);
            gg.epi(U2GNN_EPI_RELU_DROP_BWD);
            gg.a.aux0 = c.Hd, gg.a.ld_aux = ffp, gg.a.p_drop = pd;
            U2GNN_TRY(gg.run(st, plan));
        }
        U2GNN_TRY(wgrad(W, D, dF, dp, c.Hd, ffp, dp, ffp, g->l2_w, ff, blk_d, blk_ff, so, df));   // held back (df)
        // one-stream layers in the matrix-core precisions: a split-K dX1 product leaves its slabs to LayerNorm1's
        // backward, which completes dX1 before using it (the separate reduce launch goes; same bits)
        Slabs dx1_slabs;
        U2GNN_TRY(gemm_split(W, D, G(dH, w->W1, dX1, Np, dp, ffp, ffp, dp, dp, prec).accum(),
                             To(st).leave_slabs((ln_delta && so == st) ? &dx1_slabs : nullptr)));
        U2GNN_TRY(wgrad(W, D, dH, ffp, c.X1, dp, ffp, dp, g->l1_w, d, blk_ff, blk_d, so, df));
        bias_grad(df, dH, Np, ffp, ffp, ffp, ff, g->l1_b);
        // LN1 backward -> dX (residual), dA (dropout1 branch); norm1 + out_proj.bias grads (held back: df);
        // node attention: LayerNorm1's backward also forms delta = rowsum(dO * O) for the dS epilogue
        if (!plan && ln_delta && dx1_slabs.p)
            U2GNN_TRY(u2gnn_layernorm_bwd_delta_slabs(dX1, dp, dx1_slabs.p, (int32_t)dx1_slabs.n, Np * dp, c.Z1, dp,
                                                      c.mean1, c.rstd1, w->n1_w, dX, dp, dA, dp, pd, s->drop1, N, Np, d,
                                                      dp, X, dp, w->b_o, delta_ln, st));
        else if (!plan && ln_delta)
            U2GNN_TRY(u2gnn_layernorm_bwd_delta(dX1, dp, c.Z1, dp, c.mean1, c.rstd1, w->n1_w, dX, dp, dA, dp, pd,
                                                s->drop1, N, Np, d, dp, X, dp, w->b_o, delta_ln, st));
        else if (!plan)
            U2GNN_TRY(u2gnn_layernorm_bwd(dX1, dp, c.Z1, dp, c.mean1, c.rstd1, w->n1_w, dX, dp, dA, dp, pd, s->drop1,
                                          N, Np, d, dp, st));
        ln_params(df, dX1, c.Z1, c.mean1, c.rstd1, dA, dp, N, d, dp, g->n1_w, g->n1_b, g->out_b);
        // out-projection
        {
            G gg(dA, w->W_o, dO, Np, dp, dp, dp, dp, dp, prec);
            U2GNN_TRY(gg.run(st, plan));
        }
        U2GNN_TRY(wgrad(W, D, dA, dp, c.O, dp, dp, dp, g->out_w, d, blk_d, blk_d, so, df));   // held back (df)
    }
    const bool have_delta = ln_delta || tail;
    // attention core
    const float *Q = c.QKV, *Kt = Q ? Q + dp : nullptr, *V = Q ? Q + 2 * dp : nullptr;   // (no image: small path)
    const float q_scale = (float)(1.0 / std::sqrt((double)d));
    float *dQKV = tail ? small_dqkv : W.take<float>(Np * 3 * dp);
    hipEvent_t dv_done = nullptr;   // side-stream position after the dV product (in_dx waits for it)
    switch (D.attn) {
    case Attn::window:
        if (!plan)
            U2GNN_TRY(u2gnn_window_attn_bwd(c.QKV, 3 * dp, D.window, (int32_t)dp, dO, dp, c.Psave, pd, s->attn,
                                            q_scale, dQKV, 3 * dp, N / D.window, Np, st));
        break;
    case Attn::segments: {
        // delta, dQ over query tiles, then dK, dV over key tiles (P recomputed from the statistics)
        float *seg_delta = W.take<float>(Np);
        if (!plan)
            U2GNN_TRY(u2gnn_segment_attn_bwd_bias(c.QKV, 3 * dp, (int32_t)dp, D.seg, D.n_seg, D.pair_off, D.n_pairs,
                                                  D.seg_bias, c.O, dO, dp, c.stats, pd, s->attn, q_scale, dQKV, 3 * dp,
                                                  seg_delta, D.seg_dbias, N, Np, st));
        break;
    }
    case Attn::csr: {
        // delta, the entries' Pd and dS and dQ per query row, then dK, dV per key row over the transpose (P
        // recomputed from the statistics)
        float *edge_ws = W.take<float>(2 * D.csr_nnz);
        if (!plan)
            U2GNN_TRY(u2gnn_csr_attn_bwd_bias(c.QKV, 3 * dp, (int32_t)dp, D.csr, D.csr_bias, c.O, dO, dp, c.stats, pd,
                                              s->attn, q_scale, dQKV, 3 * dp, edge_ws, D.csr_dbias, N, Np, st));
        break;
    }
    case Attn::small:   // dQ, dK, dV (P recomputed from the row statistics) and dX += dQKV W_in ran with the tail above
        break;
    case Attn::fused:
    case Attn::three_pass: {
        const bool dv_side = so != st;   // grouped with dQ / dK on this stream instead: 3.136-3.141 vs 3.068-3.098 ms
        // dV needs only Pd and dO: on the side stream it overlaps the dS -> dQ -> dK chain
        U2GNN_TRY(sd.fork());
        U2GNN_TRY(gemm_split(W, D, G(c.Pd, dO, dQKV + 2 * dp, Np, dp, Np, Np, dp, 3 * dp, prec).ta().clamp(pd > 0.f)
                                       .role(U2GNN_ROLE_DV), To(dv_side ? so : st).hold(dv_side ? nullptr : att)));
        if (dv_side) U2GNN_TRY(sd.mark(&dv_done));
        // (the layer's held-back parameter work flushed here, on the side stream behind dV, instead of at the end of
        // the layer: measured neutral-to-worse, C4 3.067 / 3.088 ms per step)
        float *delta = have_delta ? delta_ln : W.take<float>(Np);
        if (!plan && !have_delta) U2GNN_TRY(u2gnn_rowdot(dO, dp, c.O, dp, delta, Np, dp, st));
        float *dS = W.take<float>(Np * Np);
        {
            G gg(dO, V, dS, Np, Np, dp, dp, 3 * dp, Np, D.prec_ab);
            gg.tb().epi(U2GNN_EPI_ATTN_DS_SIGNED).role(U2GNN_ROLE_DS);
            gg.a.aux0 = c.Pd, gg.a.rowvec = delta, gg.a.ld_aux = Np, gg.a.p_drop = pd;
            U2GNN_TRY(gg.run(st, plan));
        }
        U2GNN_TRY(gemm_split(W, D, G(dS, Kt, dQKV, Np, dp, Np, Np, 3 * dp, 3 * dp, D.prec_ab).alpha(q_scale)
                                       .role(U2GNN_ROLE_DQ), To(st).hold(att).pair()));
        U2GNN_TRY(gemm_split(W, D, G(dS, Q, dQKV + dp, Np, dp, Np, Np, 3 * dp, 3 * dp, D.prec_ab).ta()
                                       .role(U2GNN_ROLE_DK), To(st).hold(att).pair()));
        U2GNN_TRY(flush(att, W, st));
        U2GNN_TRY(sd.wait(dv_done));   // dV before dX += dQKV W_in
        break;
    }
    }
    // in-projection
    if (need_dx && !small_attn(D))
        U2GNN_TRY(gemm_split(W, D, G(dQKV, w->W_in, dX, Np, dp, 3 * dp, 3 * dp, dp, dp, prec).accum(), To(st)));
    U2GNN_TRY(wgrad(W, D, dQKV, 3 * dp, X, dp, 3 * dp, dp, g->in_w, d, blk_d, blk_d, st, df));
    // in_proj_bias: the Q and V thirds are column sums of dQKV; the K third is exactly zero -- a softmax row is
    // invariant to a constant added to its scores, so sum_j dK_j = sum_i Q_i sum_j dS_ij = 0.  The reference's
    // value there is summation noise, which Adam's first step (lr g / (|g| + eps)) turns into moves of up to lr;
    // a column sum over zero rows writes the exact zeros
    bias_grad(df, dQKV, Np, dp, 3 * dp, dp, d, g->in_b);
    bias_grad(df, dQKV + dp, 0, dp, 3 * dp, dp, d, g->in_b + d);
    bias_grad(df, dQKV + 2 * dp, Np, dp, 3 * dp, dp, d, g->in_b + 2 * d);
    // the held-back work: on the side stream after everything issued so far, except for the last layer of
    // the backward (need_dx false), where nothing is left to overlap and the hand-off plus the step's final
    // join cost more than the products (C4 round 3: 3.140-3.157 vs 3.171-3.194 ms per step)
    const bool side_flush = so != st && need_dx;
    if (side_flush) U2GNN_TRY(sd.fork());
    U2GNN_TRY(flush(df, W, side_flush ? so : st));
    return (W.overflow || CA.overflow) ? U2GNN_E_ARG : U2GNN_OK;
}

constexpr int32_t FWD_FLAGS = U2GNN_LAYER_FWD_F32 | U2GNN_LAYER_FWD_X6 | U2GNN_LAYER_FWD_H3;
bool dims_ok(const u2gnn_layer_dims *a) {
    return a && a->N >= 1 && a->d >= 1 && a->ff >= 1 && rup(a->d, 64) <= 1024 &&
           (a->precision == U2GNN_PREC_F32 || a->precision == U2GNN_PREC_BF16X3 || a->precision == U2GNN_PREC_BF16) &&
           ((a->flags & FWD_FLAGS) == 0 || a->precision == U2GNN_PREC_BF16X3) &&
           __builtin_popcount((unsigned)(a->flags & FWD_FLAGS)) <= 1 &&   // at most one forward policy
           a->window >= 0 && a->window <= 32 && (a->window == 0 || a->N % a->window == 0);
}

// Plan, then run: the same call in planning mode first (run(ctx arena, workspace arena) is the layer call), so a
// workspace or ctx arena smaller than this call takes is refused before anything is launched (never a launch over
// the end of a caller buffer).  ctx null: the call saves nothing (forward without a backward).
template <typename Run>
int plan_then_run(void *ctx, int64_t ctx_bytes, void *ws, int64_t ws_bytes, Run run) {
    Arena Pc(nullptr, 0), Pw(nullptr, 0);
    run(Pc, Pw);
    if (Pw.used > (ws ? ws_bytes : 0) || (ctx && Pc.used > ctx_bytes)) return U2GNN_E_ARG;
    static char empty_ws alignas(256)[256];   // a null base would mean "plan only"
    Arena C(ctx, ctx_bytes), W(ws ? ws : empty_ws, ws ? ws_bytes : 0);
    return run(C, W);
}

}  // namespace

extern "C" {

int u2gnn_layer_sizes_csr(const u2gnn_layer_dims *dims, float p_drop, int32_t n_seg, int64_t nnz, int64_t *ctx_bytes,
                          int64_t *fwd_ws_bytes, int64_t *bwd_ws_bytes) {
    if (!dims_ok(dims) || !ctx_bytes || !fwd_ws_bytes || !bwd_ws_bytes) return U2GNN_E_ARG;
    const Dims D = make_dims(dims, nullptr, n_seg, nullptr, nnz);
    if (!pattern_ok(D, true)) return U2GNN_E_ARG;
    u2gnn_layer_seeds s{};
    s.p_drop = p_drop;
    const u2gnn_layer_params w{};
    const u2gnn_layer_grads g{};
    Arena C(nullptr, 0), Wf(nullptr, 0), Wb(nullptr, 0), Cb(nullptr, 0);
    layer_fwd(D, &w, &s, nullptr, nullptr, C, Wf, true, nullptr);
    layer_bwd(D, &w, &s, nullptr, Cb, nullptr, nullptr, &g, Wb, nullptr, nullptr);
    *ctx_bytes = C.used;
    *fwd_ws_bytes = Wf.used;
    *bwd_ws_bytes = Wb.used;
    return U2GNN_OK;
}

int u2gnn_layer_sizes_seg(const u2gnn_layer_dims *dims, float p_drop, int32_t n_seg, int64_t *ctx_bytes,
                          int64_t *fwd_ws_bytes, int64_t *bwd_ws_bytes) {
    return u2gnn_layer_sizes_csr(dims, p_drop, n_seg, 0, ctx_bytes, fwd_ws_bytes, bwd_ws_bytes);
}

int u2gnn_layer_sizes(const u2gnn_layer_dims *dims, float p_drop, int64_t *ctx_bytes, int64_t *fwd_ws_bytes,
                      int64_t *bwd_ws_bytes) {
    return u2gnn_layer_sizes_seg(dims, p_drop, 0, ctx_bytes, fwd_ws_bytes, bwd_ws_bytes);
}

// the forward of every pattern: D from make_dims (and, for segments with a bias, seg_pairs), still to be checked
static int layer_fwd_call(const Dims &D, const u2gnn_layer_params *w, const u2gnn_layer_seeds *s, const float *X,
                          float *X2, void *ctx, int64_t ctx_bytes, void *ws, int64_t ws_bytes, void *stream) {
    if (!w || !s || !X || !X2 || (!ws && ws_bytes > 0)) return U2GNN_E_ARG;
    if (!pattern_ok(D, false)) return U2GNN_E_ARG;
    return plan_then_run(ctx, ctx_bytes, ws, ws_bytes, [&](Arena &C, Arena &W) {
        return layer_fwd(D, w, s, X, X2, C, W, ctx != nullptr, reinterpret_cast<hipStream_t>(stream));
    });
}

int u2gnn_layer_fwd_csrb(const u2gnn_layer_dims *dims, const u2gnn_layer_params *w, const u2gnn_layer_seeds *s,
                         const float *X, float *X2, void *ctx, int64_t ctx_bytes, void *ws, int64_t ws_bytes,
                         const int64_t *seg_offsets, int32_t n_seg, const u2gnn_csr_attn *A, const float *bias,
                         void *stream) {
    if (!dims_ok(dims)) return U2GNN_E_ARG;
    return layer_fwd_call(make_dims(dims, seg_offsets, n_seg, A, A ? A->nnz : 0, bias), w, s, X, X2, ctx, ctx_bytes, ws,
                          ws_bytes, stream);
}

int u2gnn_layer_fwd_segb(const u2gnn_layer_dims *dims, const u2gnn_layer_params *w, const u2gnn_layer_seeds *s,
                         const float *X, float *X2, void *ctx, int64_t ctx_bytes, void *ws, int64_t ws_bytes,
                         const int64_t *seg_offsets, int32_t n_seg, const int64_t *pair_off, int64_t n_pairs,
                         const float *bias, void *stream) {
    if (!dims_ok(dims)) return U2GNN_E_ARG;
    Dims D = make_dims(dims, seg_offsets, n_seg, nullptr, 0);
    if (bias) D.pair_off = pair_off, D.n_pairs = n_pairs, D.seg_bias = bias;   // no bias: the _seg call exactly
    return layer_fwd_call(D, w, s, X, X2, ctx, ctx_bytes, ws, ws_bytes, stream);
}

int u2gnn_layer_fwd_csr(const u2gnn_layer_dims *dims, const u2gnn_layer_params *w, const u2gnn_layer_seeds *s,
                        const float *X, float *X2, void *ctx, int64_t ctx_bytes, void *ws, int64_t ws_bytes,
                        const int64_t *seg_offsets, int32_t n_seg, const u2gnn_csr_attn *A, void *stream) {
    return u2gnn_layer_fwd_csrb(dims, w, s, X, X2, ctx, ctx_bytes, ws, ws_bytes, seg_offsets, n_seg, A, nullptr, stream);
}

int u2gnn_layer_fwd_seg(const u2gnn_layer_dims *dims, const u2gnn_layer_params *w, const u2gnn_layer_seeds *s,
                        const float *X, float *X2, void *ctx, int64_t ctx_bytes, void *ws, int64_t ws_bytes,
                        const int64_t *seg_offsets, int32_t n_seg, void *stream) {
    return u2gnn_layer_fwd_csr(dims, w, s, X, X2, ctx, ctx_bytes, ws, ws_bytes, seg_offsets, n_seg, nullptr, stream);
}

int u2gnn_layer_fwd(const u2gnn_layer_dims *dims, const u2gnn_layer_params *w, const u2gnn_layer_seeds *s,
                    const float *X, float *X2, void *ctx, int64_t ctx_bytes, void *ws, int64_t ws_bytes,
                    void *stream) {
    return u2gnn_layer_fwd_seg(dims, w, s, X, X2, ctx, ctx_bytes, ws, ws_bytes, nullptr, 0, stream);
}

// the backward of every pattern, as layer_fwd_call
static int layer_bwd_call(const Dims &D, const u2gnn_layer_params *w, const u2gnn_layer_seeds *s, const float *X,
                          const void *ctx, int64_t ctx_bytes, const float *dX2, float *dX, const u2gnn_layer_grads *g,
                          void *ws, int64_t ws_bytes, void *stream, void *side_stream) {
    if (!w || !s || !X || !ctx || !dX2 || !g || (!ws && ws_bytes > 0)) return U2GNN_E_ARG;
    if (!pattern_ok(D, false)) return U2GNN_E_ARG;
    // (planned with this call's schedule: its streams and whether dX is wanted)
    return plan_then_run(const_cast<void *>(ctx), ctx_bytes, ws, ws_bytes, [&](Arena &C, Arena &W) {
        return layer_bwd(D, w, s, X, C, dX2, dX, g, W, reinterpret_cast<hipStream_t>(stream),
                         reinterpret_cast<hipStream_t>(side_stream), dX != nullptr);
    });
}

int u2gnn_layer_bwd_csrb(const u2gnn_layer_dims *dims, const u2gnn_layer_params *w, const u2gnn_layer_seeds *s,
                         const float *X, const void *ctx, int64_t ctx_bytes, const float *dX2, float *dX,
                         const u2gnn_layer_grads *g, void *ws, int64_t ws_bytes, const int64_t *seg_offsets,
                         int32_t n_seg, const u2gnn_csr_attn *A, const float *bias, float *dbias, void *stream,
                         void *side_stream) {
    if (!dims_ok(dims)) return U2GNN_E_ARG;
    return layer_bwd_call(make_dims(dims, seg_offsets, n_seg, A, A ? A->nnz : 0, bias, dbias), w, s, X, ctx, ctx_bytes,
                          dX2, dX, g, ws, ws_bytes, stream, side_stream);
}

int u2gnn_layer_bwd_segb(const u2gnn_layer_dims *dims, const u2gnn_layer_params *w, const u2gnn_layer_seeds *s,
                         const float *X, const void *ctx, int64_t ctx_bytes, const float *dX2, float *dX,
                         const u2gnn_layer_grads *g, void *ws, int64_t ws_bytes, const int64_t *seg_offsets,
                         int32_t n_seg, const int64_t *pair_off, int64_t n_pairs, const float *bias, float *dbias,
                         void *stream, void *side_stream) {
    if (!dims_ok(dims)) return U2GNN_E_ARG;
    Dims D = make_dims(dims, seg_offsets, n_seg, nullptr, 0);
    if (bias) D.pair_off = pair_off, D.n_pairs = n_pairs, D.seg_bias = bias;   // no bias: the _seg call exactly
    D.seg_dbias = dbias;                                                       // (without a bias: refused)
    return layer_bwd_call(D, w, s, X, ctx, ctx_bytes, dX2, dX, g, ws, ws_bytes, stream, side_stream);
}

int u2gnn_layer_bwd_csr(const u2gnn_layer_dims *dims, const u2gnn_layer_params *w, const u2gnn_layer_seeds *s,
                        const float *X, const void *ctx, int64_t ctx_bytes, const float *dX2, float *dX,
                        const u2gnn_layer_grads *g, void *ws, int64_t ws_bytes, const int64_t *seg_offsets,
                        int32_t n_seg, const u2gnn_csr_attn *A, void *stream, void *side_stream) {
    return u2gnn_layer_bwd_csrb(dims, w, s, X, ctx, ctx_bytes, dX2, dX, g, ws, ws_bytes, seg_offsets, n_seg, A, nullptr,
                                nullptr, stream, side_stream);
}

int u2gnn_layer_bwd_seg(const u2gnn_layer_dims *dims, const u2gnn_layer_params *w, const u2gnn_layer_seeds *s,
                        const float *X, const void *ctx, int64_t ctx_bytes, const float *dX2, float *dX,
                        const u2gnn_layer_grads *g, void *ws, int64_t ws_bytes, const int64_t *seg_offsets,
                        int32_t n_seg, void *stream, void *side_stream) {
    return u2gnn_layer_bwd_csr(dims, w, s, X, ctx, ctx_bytes, dX2, dX, g, ws, ws_bytes, seg_offsets, n_seg, nullptr,
                               stream, side_stream);
}

int u2gnn_layer_bwd(const u2gnn_layer_dims *dims, const u2gnn_layer_params *w, const u2gnn_layer_seeds *s,
                    const float *X, const void *ctx, int64_t ctx_bytes, const float *dX2, float *dX,
                    const u2gnn_layer_grads *g, void *ws, int64_t ws_bytes, void *stream, void *side_stream) {
    return u2gnn_layer_bwd_seg(dims, w, s, X, ctx, ctx_bytes, dX2, dX, g, ws, ws_bytes, nullptr, 0, stream,
                               side_stream);
}

int u2gnn_layer_plan(const u2gnn_layer_dims *dims, float p_drop, u2gnn_layer_rules *plan) {
    if (!dims_ok(dims) || !plan || !(p_drop >= 0.f && p_drop < 1.f)) return U2GNN_E_ARG;
    *plan = layer_plan(make_dims(dims, nullptr, 0, nullptr, 0), p_drop);
    return U2GNN_OK;
}

int u2gnn_gemm_split_plan(const u2gnn_split_query *q, u2gnn_split_plan *plan) {
    if (!q || !plan || q->M < 64 || q->N < 64 || q->K < 16 || q->M % 64 || q->N % 64 || q->K % 16 ||
        q->precision < U2GNN_PREC_F32 || q->precision > U2GNN_PREC_F16X3)
        return U2GNN_E_ARG;
    for (int32_t f : {q->accumulate, q->deep, q->mapped, q->grouped, q->deep_wgrad, q->held})
        if (f != 0 && f != 1) return U2GNN_E_ARG;
    const SplitPlan sp = split_plan(q->M, q->N, q->K, q->precision, q->accumulate, q->deep, q->mapped, q->grouped,
                                    q->deep_wgrad, q->held);
    std::memset(plan, 0, sizeof(*plan));
    plan->direct = sp.direct, plan->tile = sp.tile, plan->launch_tile = sp.launch_tile, plan->split = (int32_t)sp.split;
    return U2GNN_OK;
}

int u2gnn_probe_arm(int32_t role, int32_t capacity) {
    std::lock_guard<std::mutex> lk(g_probe_mu);
    if (g_probe.ev) return U2GNN_E_ARG;   // collect the previous probe first
    if (role < U2GNN_ROLE_QK || role > U2GNN_ROLE_DK || capacity < 1 || capacity > (1 << 16)) return U2GNN_E_ARG;
    hipEvent_t *ev = new hipEvent_t[2 * capacity];
    for (int i = 0; i < 2 * capacity; ++i) {
        // timing events without the system-scope release (the host reads only their timestamps, in
        // u2gnn_probe_collect, after the bench's device synchronize; no data is handed over through them): with
        // it, each mark wrote L2 back and the timed kernel re-fetched its operands -- C4 dS 99.9 -> 89.3 us in
        // rocprof, probe 107.5 -> 93.8 us, step 3.034 -> 3.018 ms (no probe: 3.002; profiles/r05/ab_probe_fence.txt)
        const hipError_t e = hipEventCreateWithFlags(&ev[i], hipEventDisableSystemFence);
        if (e != hipSuccess) {
            for (int j = 0; j < i; ++j) (void)hipEventDestroy(ev[j]);
            delete[] ev;
            return (int)e;
        }
    }
    g_probe.ev = ev, g_probe.cap = capacity, g_probe.n = 0, g_probe.role = role;
    g_probe_role.store(role, std::memory_order_relaxed);
    return U2GNN_OK;
}

int u2gnn_probe_collect(float *total_ms, int32_t *launches) {
    if (!total_ms || !launches) return U2GNN_E_ARG;
    *total_ms = 0.f, *launches = 0;
    std::lock_guard<std::mutex> lk(g_probe_mu);
    if (!g_probe.ev) return U2GNN_OK;
    int rc = U2GNN_OK;
    double tot = 0.0;
    for (int i = 0; i < g_probe.n && rc == U2GNN_OK; ++i) {
        hipError_t e = hipEventSynchronize(g_probe.ev[2 * i + 1]);
        float ms = 0.f;
        if (e == hipSuccess) e = hipEventElapsedTime(&ms, g_probe.ev[2 * i], g_probe.ev[2 * i + 1]);
        if (e != hipSuccess) rc = (int)e;
        tot += ms;
    }
    for (int i = 0; i < 2 * g_probe.cap; ++i) (void)hipEventDestroy(g_probe.ev[i]);
    delete[] g_probe.ev;
    *total_ms = (float)tot, *launches = g_probe.n;
    g_probe = Probe();
    g_probe_role.store(0, std::memory_order_relaxed);
    return rc;
}

}  // extern "C"
