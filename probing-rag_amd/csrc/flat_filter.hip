// Exact filtered top-k search on the flat index: the k best rows of a selected subset S (include/prag.h
// prag_index_search_filtered) - faiss `index.search(x, k, params=SearchParameters(sel=...))`.
//
//   filter_count_kernel    allow bitmap (one uint32 word = one 32-row tile of the direct scan) -> per workgroup: rows
//                          selected, non-empty tiles; its LAST workgroup turns them into exclusive offsets, writes both
//                          totals and the PATH word (1 masked scan, 2 gathered float64) - decided here, on the device
//   filter_compact_kernel  the selected rows (uint32, ascending) and the non-empty tiles ((tile, allow word), ascending)
//   path 1, per query tile (every launch enqueued, gated on the path word):
//     scan_topk_masked_kernel (flat_index.hip): the direct scan over the listed tiles only; an unselected row gets the
//                          key +inf and never enters a per-lane list
//     merge_rerank_kernel  (flat_index.hip): list merge, float64 rerank, certificate - unchanged; a query it cannot
//                          certify goes on the flag list
//   filter_gather_kernel   exact float64 brute force over the selected rows (row_score64, the sum D is defined by):
//                          every query on path 2, the flagged queries on path 1.  Per-workgroup threshold lists in LDS,
//                          folded by the last workgroup of each query.
// The call never waits for its stream with device io.  It reads the stored rows only (no shadow) and touches none of
// the search's state (bounds, grid tuner, plan, tier statistics): every workspace below belongs to the filtered search.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <vector>

#include "flat_index_state.h"

namespace {

constexpr int kFilterMaxB = 1024;
constexpr int kCompactThreads = 256;
constexpr int kCompactRounds = 8;                                       // words per thread
constexpr int kCompactWords = kCompactThreads * kCompactRounds;         // 2048 words = 65 536 rows per workgroup
constexpr int kGatherWaves = kExThreads / 64;
// ctr words
constexpr int kCtrSel = 0, kCtrTiles = 1, kCtrPath = 2, kCtrFlag = 3, kCtrArrive = 4, kCtrWords = 8;

// Path rule (auto): gathered when n_sel B d / kGatherFmaPerUs + kGatherFixedUs is below
// passes (n_tiles 32 row_bytes / kScanBytesPerUs + kMaskedFixedUs).  Measured on MI355X: DESIGN.md section 2.F.
constexpr double kScanBytesPerUs = 6.8e6;     // the direct scan's stream, 6.8 TB/s
constexpr double kMaskedFixedUs = 25.0;       // masked scan + merge / rerank launches of one query tile
constexpr double kGatherFmaPerUs = 1.0e6;     // the gathered path's float64 products per microsecond
constexpr double kGatherFixedUs = 10.0;

struct CompactArgs {
    const uint32_t* allow;    // [n_words] (bits at or past ntotal are ignored)
    int64_t n_words;          // ceil(ntotal / 32)
    int64_t ntotal;
    uint32_t* blk;            // [2][n_blocks]: per workgroup rows / tiles, then their exclusive prefix
    int n_blocks;
    uint32_t* ctr;            // [kCtrWords]
    uint32_t* sel;            // [ntotal] out: selected rows, ascending
    uint2* tiles;             // [n_words] out: (tile, allow word) of the non-empty tiles, ascending
    // path rule
    int pinned;               // PRAG_FILTER_PATH: 0 auto, 1 masked scan, 2 gathered
    int masked_ok;            // k <= 26 and rows present: the masked scan can run
    int B, d, row_bytes, passes;
};

__device__ __forceinline__ uint32_t allow_word(const CompactArgs& a, int64_t w) {
    if (w >= a.n_words) return 0u;
    uint32_t v = a.allow[w];
    const int tail = (int)(a.ntotal & 31);
    if (w == a.n_words - 1 && tail) v &= (1u << tail) - 1u;
    return v;
}

// exclusive prefix of (x, y) over the kCompactThreads threads of the block, and the block totals
__device__ __forceinline__ void block_scan2(uint32_t x, uint32_t y, uint32_t& ex, uint32_t& ey, uint32_t& tx, uint32_t& ty,
                                            uint32_t* s /*[2 * kCompactThreads / 64]*/) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint32_t ix = x, iy = y;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t vx = __shfl_up(ix, o, 64), vy = __shfl_up(iy, o, 64);
        if (lane >= o) {
            ix += vx;
            iy += vy;
        }
    }
    __syncthreads();
    if (lane == 63) {
        s[2 * w] = ix;
        s[2 * w + 1] = iy;
    }
    __syncthreads();
    uint32_t bx = 0, by = 0;
    tx = 0;
    ty = 0;
#pragma unroll
    for (int j = 0; j < kCompactThreads / 64; ++j) {
        if (j < w) {
            bx += s[2 * j];
            by += s[2 * j + 1];
        }
        tx += s[2 * j];
        ty += s[2 * j + 1];
    }
    ex = bx + ix - x;
    ey = by + iy - y;
}

// Round r of a workgroup covers words [blk * kCompactWords + r * 256, + 256): coalesced reads, and the writes of a round
// land in one contiguous stretch of each list.
__global__ __launch_bounds__(kCompactThreads) void filter_count_kernel(CompactArgs a) {
    __shared__ uint32_t s[2 * kCompactThreads / 64];
    __shared__ int s_last;
    const int64_t w0 = (int64_t)blockIdx.x * kCompactWords;
    uint32_t n_sel = 0, n_til = 0;
#pragma unroll
    for (int r = 0; r < kCompactRounds; ++r) {
        const uint32_t v = allow_word(a, w0 + r * kCompactThreads + threadIdx.x);
        n_sel += __builtin_popcount(v);
        n_til += v != 0u;
    }
    uint32_t ex, ey, tx, ty;
    block_scan2(n_sel, n_til, ex, ey, tx, ty, s);
    if (threadIdx.x == 0) {
        a.blk[blockIdx.x] = tx;
        a.blk[a.n_blocks + blockIdx.x] = ty;
    }
    __threadfence();
    __syncthreads();
    if (threadIdx.x == 0) s_last = atomicAdd(a.ctr + kCtrArrive, 1u) == gridDim.x - 1 ? 1 : 0;
    __syncthreads();
    if (!s_last) return;
    __threadfence();
    // the last workgroup: per-workgroup counts -> exclusive offsets (each thread a contiguous run of workgroups)
    const int per = (a.n_blocks + kCompactThreads - 1) / kCompactThreads;
    const int j0 = min(a.n_blocks, (int)threadIdx.x * per), j1 = min(a.n_blocks, j0 + per);
    uint32_t cx = 0, cy = 0;
    for (int j = j0; j < j1; ++j) {
        cx += __hip_atomic_load(a.blk + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        cy += __hip_atomic_load(a.blk + a.n_blocks + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    block_scan2(cx, cy, ex, ey, tx, ty, s);
    for (int j = j0; j < j1; ++j) {
        const uint32_t vx = __hip_atomic_load(a.blk + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const uint32_t vy = __hip_atomic_load(a.blk + a.n_blocks + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        a.blk[j] = ex;
        a.blk[a.n_blocks + j] = ey;
        ex += vx;
        ey += vy;
    }
    if (threadIdx.x == 0) {
        a.ctr[kCtrSel] = tx;
        a.ctr[kCtrTiles] = ty;
        uint32_t path = 2;
        if (a.masked_ok) {
            if (a.pinned == 1 || a.pinned == 2) {
                path = (uint32_t)a.pinned;
            } else {
                const double gather_us = (double)tx * a.B * a.d / kGatherFmaPerUs + kGatherFixedUs;
                const double masked_us = a.passes * ((double)ty * 32.0 * a.row_bytes / kScanBytesPerUs + kMaskedFixedUs);
                path = gather_us < masked_us ? 2u : 1u;
            }
        }
        a.ctr[kCtrPath] = path;
        a.ctr[kCtrArrive] = 0u;
    }
}

__global__ __launch_bounds__(kCompactThreads) void filter_compact_kernel(CompactArgs a) {
    __shared__ uint32_t s[2 * kCompactThreads / 64];
    const int64_t w0 = (int64_t)blockIdx.x * kCompactWords;
    uint32_t bx = a.blk[blockIdx.x], by = a.blk[a.n_blocks + blockIdx.x];
#pragma unroll 1
    for (int r = 0; r < kCompactRounds; ++r) {
        const int64_t w = w0 + r * kCompactThreads + threadIdx.x;
        const uint32_t v = allow_word(a, w);
        uint32_t ex, ey, tx, ty;
        block_scan2(__builtin_popcount(v), v != 0u, ex, ey, tx, ty, s);
        if (v) {
            a.tiles[by + ey] = make_uint2((uint32_t)w, v);
            uint32_t m = v, o = bx + ex;
            while (m) {
                a.sel[o++] = (uint32_t)(w * 32 + __builtin_ctz(m));
                m &= m - 1;
            }
        }
        bx += tx;
        by += ty;
    }
}

struct GatherArgs {
    const void* rows;
    int d, metric_l2;
    const float* q32;         // [B][d] as the rerank uses them (normalised for cosine)
    int B, k;
    const uint32_t* sel;      // selected rows, ascending
    const uint32_t* ctr;      // [kCtrSel] rows selected, [kCtrPath] path
    const uint32_t* n_flag;   // path 1: queries the certificate flagged ...
    const int* flag_list;     // ... and which
    int f0;                   // this launch: query slots [f0, f0 + gridDim.y)
    unsigned long long* part_key;   // [gridDim.y][gridDim.x][k]
    int* part_id;
    uint32_t* done;           // [gridDim.y] arrival counters, zero between searches (the last workgroup re-zeroes)
    int64_t id_offset;
    float* D;                 // [B][k]
    int64_t* I;
};

// One workgroup = one query slot (blockIdx.y) x a 1/gridDim.x share of the selected rows; one wave per row, scored by
// row_score64 itself, so the float64 values ARE the definition's and no re-scoring is needed.  Keys ascend with rank
// (L2: sortable score, IP / COS: its complement), ties by row id in the cuts.
template <bool F32>
__global__ __launch_bounds__(kExThreads) void filter_gather_kernel(GatherArgs a) {
    __shared__ ExTopK tk;
    __shared__ int s_last;
    const uint32_t path = a.ctr[kCtrPath];
    const int n_q = path == 2u ? a.B : path == 1u ? (int)*a.n_flag : 0;
    const int f = a.f0 + (int)blockIdx.y;
    if (f >= n_q) return;
    const int b = path == 2u ? f : a.flag_list[f];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int64_t n_sel = a.ctr[kCtrSel];
    const float* q = a.q32 + (int64_t)b * a.d;
    ex_init(tk);
    __syncthreads();
    const int64_t step = (int64_t)gridDim.x * kGatherWaves;
    for (int64_t base = (int64_t)blockIdx.x * kGatherWaves; base < n_sel; base += step) {
        const int64_t i = base + w;
        if (i < n_sel) {
            const int row = (int)a.sel[i];
            const double s = row_score64<F32>(a.rows, a.d, a.metric_l2, q, row, lane);
            if (lane == 0) ex_push(tk, a.metric_l2 ? sortable_u64(s) : ~sortable_u64(s), row);
        }
        __syncthreads();
        const int c = tk.cnt;
        __syncthreads();
        if (c > kExCap - kGatherWaves) ex_cut(tk, a.k);
    }
    ex_cut(tk, a.k);
    const int slot = (int)blockIdx.y;
    const int64_t o = ((int64_t)slot * gridDim.x + blockIdx.x) * a.k;
    for (int j = tid; j < a.k; j += kExThreads) {
        const bool ok = j < tk.cnt;
        a.part_key[o + j] = ok ? tk.key[j] : ~0ull;
        a.part_id[o + j] = ok ? tk.id[j] : 0x7fffffff;
    }
    __threadfence();
    __syncthreads();
    if (tid == 0) s_last = atomicAdd(a.done + slot, 1u) == gridDim.x - 1 ? 1 : 0;
    __syncthreads();
    if (!s_last) return;
    __threadfence();
    // the last workgroup of this query folds the gridDim.x lists
    ex_init(tk);
    __syncthreads();
    const int64_t total = (int64_t)gridDim.x * a.k;
    const int64_t o0 = (int64_t)slot * total;
    for (int64_t p0 = 0; p0 < total; p0 += kExThreads) {
        const int64_t p = p0 + tid;
        if (p < total) {
            const int id = a.part_id[o0 + p];
            if (id != 0x7fffffff) ex_push(tk, a.part_key[o0 + p], id);
        }
        __syncthreads();
        const int c = tk.cnt;
        __syncthreads();
        if (c > kExCap - kExThreads) ex_cut(tk, a.k);
    }
    ex_cut(tk, a.k);
    for (int j = tid; j < a.k; j += kExThreads) {
        const bool ok = j < tk.cnt;
        const double sc = ok ? unsortable_f64(a.metric_l2 ? tk.key[j] : ~tk.key[j]) : 0.0;
        a.D[(int64_t)b * a.k + j] = ok ? (float)sc : (a.metric_l2 ? FLT_MAX : -FLT_MAX);
        a.I[(int64_t)b * a.k + j] = ok ? (int64_t)tk.id[j] + a.id_offset : -1;
    }
    if (tid == 0) a.done[slot] = 0u;
}

}  // namespace

struct FilterState {
    int d = 0;
    float* q_in = nullptr;            // [kFilterMaxB][d] host queries staged on the device
    float* q32 = nullptr;             // [kFilterMaxB][d]
    _Float16* q16 = nullptr;          // [kFilterMaxB][d]
    _Float16* q16lo = nullptr;
    float* qinfo = nullptr;           // [kFilterMaxB][4]
    double* qn2 = nullptr;
    uint32_t* g_tau = nullptr;        // [kFilterMaxB]
    uint32_t* g_slot = nullptr;       // [kFilterMaxB][kSlotWords]
    int* flag_list = nullptr;         // [kFilterMaxB]
    uint32_t* ctr = nullptr;          // [kCtrWords]
    uint32_t* done = nullptr;         // [kFilterMaxB] arrival counters of the gather's list fold (zero between calls)
    float* part_key = nullptr;        // masked scan: [grid][64][32]
    int* part_idx = nullptr;
    size_t part_cap = 0;
    unsigned long long* g_key = nullptr;   // gathered path: [f_cap][gx][k]
    int* g_id = nullptr;
    size_t g_cap = 0;
    uint32_t* allow_in = nullptr;     // host bitmap staged on the device
    int64_t allow_cap = 0;            // words
    uint32_t* blk = nullptr;          // [2][n_blocks]
    int64_t blk_cap = 0;
    uint32_t* sel = nullptr;          // [rows_cap]
    uint2* tiles = nullptr;           // [tiles_cap]
    int64_t rows_cap = 0;
    float* io_D = nullptr;            // host io: results staged on the device
    int64_t* io_I = nullptr;
    size_t io_cap = 0;                // entries
    int64_t last_B = -1;              // queries of the last filtered search (-1: none)
    int last_k = 0;
    int masked_ran = 0;               // the last call enqueued the masked scan (k <= 26, rows present)
    std::vector<uint32_t> h_ctr = std::vector<uint32_t>(kCtrWords);
};

void filter_state_free(prag_index* ix) {
    FilterState* fs = ix->filter;
    if (!fs) return;
    for (void* p : {(void*)fs->q_in, (void*)fs->q32, (void*)fs->q16, (void*)fs->q16lo, (void*)fs->qinfo, (void*)fs->qn2,
                    (void*)fs->g_tau, (void*)fs->g_slot, (void*)fs->flag_list, (void*)fs->ctr, (void*)fs->done,
                    (void*)fs->part_key, (void*)fs->part_idx, (void*)fs->g_key, (void*)fs->g_id, (void*)fs->allow_in,
                    (void*)fs->blk, (void*)fs->sel, (void*)fs->tiles, (void*)fs->io_D, (void*)fs->io_I})
        if (p) (void)hipFree(p);
    delete fs;
    ix->filter = nullptr;
}

static int filter_state(prag_index* ix, hipStream_t st, FilterState** out) {
    if (!ix->filter) {
        FilterState* fs = new FilterState();
        fs->d = ix->d;
        const size_t qe = (size_t)kFilterMaxB * ix->d;
        const int rc = ws_regrow({{vpp(&fs->q_in), qe * 4}, {vpp(&fs->q32), qe * 4}, {vpp(&fs->q16), qe * 2},
                                  {vpp(&fs->q16lo), qe * 2}, {vpp(&fs->qinfo), (size_t)kFilterMaxB * 16},
                                  {vpp(&fs->qn2), (size_t)kFilterMaxB * 8}, {vpp(&fs->g_tau), (size_t)kFilterMaxB * 4},
                                  {vpp(&fs->g_slot), (size_t)kFilterMaxB * kSlotWords * 4},
                                  {vpp(&fs->flag_list), (size_t)kFilterMaxB * 4}, {vpp(&fs->ctr), (size_t)kCtrWords * 4},
                                  {vpp(&fs->done), (size_t)kFilterMaxB * 4}});
        if (rc != PRAG_OK) {
            delete fs;
            return rc;
        }
        ix->filter = fs;
        PRAG_HIP(hipMemsetAsync(fs->ctr, 0, (size_t)kCtrWords * 4, st));
        PRAG_HIP(hipMemsetAsync(fs->done, 0, (size_t)kFilterMaxB * 4, st));
    }
    *out = ix->filter;
    return PRAG_OK;
}

// grow-only buffer group (the old contents are not kept)
template <typename T>
static int filter_grow(T** p, size_t have, size_t want) {
    if (want <= have) return PRAG_OK;
    return ws_regrow({{vpp(p), want * sizeof(T)}});
}

static int filter_env_path() {
    const char* e = std::getenv("PRAG_FILTER_PATH");
    if (!e || !*e) return 0;
    const int v = std::atoi(e);
    return (v == 1 || v == 2) ? v : 0;
}

extern "C" int prag_index_search_filtered(prag_index_t* ix, const float* q, int B, int k, int64_t id_offset,
                                          const uint32_t* allow, int64_t n_words, int allow_is_device, float* D,
                                          int64_t* I, int io_is_device, void* stream) {
    PRAG_REQUIRE(ix != nullptr, PRAG_EINVAL, "prag_index_search_filtered: NULL handle");
    PRAG_REQUIRE(B >= 0 && B <= kFilterMaxB, PRAG_EINVAL, "prag_index_search_filtered: B=%d (0..%d)", B, kFilterMaxB);
    PRAG_REQUIRE(k >= 1 && k <= 911, PRAG_EINVAL, "prag_index_search_filtered: k=%d (1..911)", k);
    const int64_t need_words = (ix->ntotal + 31) / 32;
    PRAG_REQUIRE(n_words >= need_words, PRAG_EINVAL, "prag_index_search_filtered: n_words=%lld, %lld rows need %lld",
                 (long long)n_words, (long long)ix->ntotal, (long long)need_words);
    if (B == 0) return PRAG_OK;
    PRAG_REQUIRE(q != nullptr && D != nullptr && I != nullptr && (allow != nullptr || need_words == 0), PRAG_EINVAL,
                 "prag_index_search_filtered: NULL pointer");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    FilterState* fs = nullptr;
    {
        const int rc = filter_state(ix, st, &fs);
        if (rc != PRAG_OK) return rc;
    }
    const int d = ix->d;
    const bool f32 = ix->store == PRAG_F32;
    const int metric_l2 = ix->metric == PRAG_METRIC_L2;
    const int64_t N = ix->ntotal;
    // ---- plan (host): masked scan shape; the choice between the paths is the device's ----
    int kc = pick_kc(k);
    if (f32 && kc == 8) kc = 16;      // float32 rows are rounded to fp16 inside the scan (plan_search's rule, any B)
    const int qstride = (d * 2 + 255) / 256 * 256;
    const bool wide_ok = 64 * qstride + 8 * 4096 + 64 * 12 <= 160 * 1024 && kc < 32 && !f32;
    const int QT = (B > 32 && wide_ok) ? 64 : 32;
    // (k > 26, and fp16 rows with 13 <= k <= 26: the gathered path - index_filter_shape_ok)
    const bool masked_ok = N > 0 && kc <= 32 && index_filter_shape_ok(QT, kc, f32);
    const int Bpad = (B + QT - 1) / QT * QT;
    const int n_tiles_max = (int)std::max<int64_t>(1, need_words);
    const int grid = std::max(1, std::min(ix->n_cu, (n_tiles_max + 7) / 8));
    const int passes = Bpad / QT;
    // gathered path: query slots per launch, workgroups per query
    const int f_cap = std::min(B, 64);
    const int gx = std::max(8, std::min(512, (4 * ix->n_cu + f_cap - 1) / f_cap));
    // ---- workspaces ----
    if (masked_ok) {
        const size_t pneed = (size_t)grid * QT * kc;
        if (pneed > fs->part_cap) {
            fs->part_cap = 0;
            const int rc = ws_regrow({{vpp(&fs->part_key), pneed * 4}, {vpp(&fs->part_idx), pneed * 4}});
            if (rc != PRAG_OK) return rc;
            fs->part_cap = pneed;
        }
    }
    {
        const size_t gneed = (size_t)f_cap * gx * k;
        if (gneed > fs->g_cap) {
            fs->g_cap = 0;
            const int rc = ws_regrow({{vpp(&fs->g_key), gneed * 8}, {vpp(&fs->g_id), gneed * 4}});
            if (rc != PRAG_OK) return rc;
            fs->g_cap = gneed;
        }
    }
    const int n_blocks = (int)std::max<int64_t>(1, (need_words + kCompactWords - 1) / kCompactWords);
    if (n_blocks > fs->blk_cap) {
        fs->blk_cap = 0;
        const int rc = filter_grow(&fs->blk, 0, (size_t)2 * n_blocks);
        if (rc != PRAG_OK) return rc;
        fs->blk_cap = n_blocks;
    }
    if (N > fs->rows_cap) {
        fs->rows_cap = 0;
        const int64_t want = (N + 255) / 256 * 256;
        const int rc = ws_regrow({{vpp(&fs->sel), (size_t)want * 4}, {vpp(&fs->tiles), (size_t)(want / 32) * 8}});
        if (rc != PRAG_OK) return rc;
        fs->rows_cap = want;
    }
    if (!io_is_device && (size_t)B * k > fs->io_cap) {
        fs->io_cap = 0;
        const size_t want = std::max<size_t>((size_t)B * k, 4096);
        const int rc = ws_regrow({{vpp(&fs->io_D), want * 4}, {vpp(&fs->io_I), want * 8}});
        if (rc != PRAG_OK) return rc;
        fs->io_cap = want;
    }
    // ---- inputs on the device ----
    const float* q_dev = q;
    float* D_dev = D;
    int64_t* I_dev = I;
    if (!io_is_device) {
        PRAG_HIP(hipMemcpyAsync(fs->q_in, q, (size_t)B * d * sizeof(float), hipMemcpyHostToDevice, st));
        q_dev = fs->q_in;
        D_dev = fs->io_D;
        I_dev = fs->io_I;
    }
    const uint32_t* allow_dev = allow;
    if (!allow_is_device && need_words > 0) {
        if (need_words > fs->allow_cap) {
            fs->allow_cap = 0;
            const int rc = filter_grow(&fs->allow_in, 0, (size_t)need_words);
            if (rc != PRAG_OK) return rc;
            fs->allow_cap = need_words;
        }
        PRAG_HIP(hipMemcpyAsync(fs->allow_in, allow, (size_t)need_words * 4, hipMemcpyHostToDevice, st));
        allow_dev = fs->allow_in;
    }
    {
        int rc = index_refresh_xn_max(ix, st);
        if (rc == PRAG_OK)
            rc = index_prep_queries(ix, q_dev, B, Bpad, fs->q32, fs->q16, fs->q16lo, fs->qinfo, fs->qn2, fs->g_tau,
                                    fs->g_slot, fs->ctr + kCtrFlag, st);
        if (rc != PRAG_OK) return rc;
    }
    // ---- selection -> row list, tile list, path word ----
    CompactArgs ca{};
    ca.allow = allow_dev;
    ca.n_words = need_words;
    ca.ntotal = N;
    ca.blk = fs->blk;
    ca.n_blocks = n_blocks;
    ca.ctr = fs->ctr;
    ca.sel = fs->sel;
    ca.tiles = fs->tiles;
    ca.pinned = filter_env_path();
    ca.masked_ok = masked_ok ? 1 : 0;
    ca.B = B;
    ca.d = d;
    ca.row_bytes = d * (f32 ? 4 : 2);
    ca.passes = passes;
    hipLaunchKernelGGL(filter_count_kernel, dim3(n_blocks), dim3(kCompactThreads), 0, st, ca);
    PRAG_LAUNCH_CHECK();
    hipLaunchKernelGGL(filter_compact_kernel, dim3(n_blocks), dim3(kCompactThreads), 0, st, ca);
    PRAG_LAUNCH_CHECK();
    // ---- path 1: masked scan + merge / rerank / certificate, one query tile at a time ----
    const Gate masked_gate{fs->ctr + kCtrPath, 1u, 1u};
    if (masked_ok) {
        CertArgs c{};     // the error model of a one-term fp16 selection (flat_index.hip search_certificate, not HP)
        c.qinfo = fs->qinfo;
        c.qn2 = fs->qn2;
        c.xn_max = ix->cert_words + 1;
        const double u16 = 1.0 / 2048.0, sub = std::sqrt((double)d) * 2.9802322387695312e-08 /* 2^-25 */;
        c.rq_sel = 1;
        if (!f32) { c.c_row = 0.f; c.c_abs = 0.f; }
        else { c.c_row = (float)(u16 * (1.0 + u16) * 1.001); c.c_abs = (float)(sub * 1.001); }
        c.c_acc = (float)((double)d * 1.1920928955078125e-07 /* 2^-23 */ * 1.001);
        c.n_flag = fs->ctr + kCtrFlag;
        c.flag_list = fs->flag_list;
        c.force = nullptr;
        c.tag_ids = 0;
        c.sq8 = nullptr;
        c.kshift = nullptr;
        c.gate = masked_gate;
        FilterScan fsc{};
        fsc.QT = QT;
        fsc.kc = kc;
        fsc.grid = grid;
        fsc.qstride = qstride;
        fsc.mt.tiles = fs->tiles;
        fsc.mt.count = fs->ctr + kCtrTiles;
        fsc.part_key = fs->part_key;
        fsc.part_idx = fs->part_idx;
        fsc.gate = masked_gate;
        for (int p0 = 0; p0 < Bpad; p0 += QT) {
            fsc.q16 = fs->q16 + (size_t)p0 * d;
            fsc.g_tau = fs->g_tau + p0;
            fsc.g_slot = fs->g_slot + (size_t)p0 * kSlotWords;
            int rc = index_filter_scan(ix, fsc, st);
            if (rc == PRAG_OK)
                rc = index_merge_rerank(ix, kc, fs->part_key, fs->part_idx, grid, QT, std::min(QT, B - p0), p0, fs->q32, k,
                                        id_offset, D_dev, I_dev, c, st);
            if (rc != PRAG_OK) return rc;
        }
    }
    // ---- gathered float64 path: every query (path 2) or the flagged ones (path 1) ----
    GatherArgs ga{};
    ga.rows = ix->rows;
    ga.d = d;
    ga.metric_l2 = metric_l2;
    ga.q32 = fs->q32;
    ga.B = B;
    ga.k = k;
    ga.sel = fs->sel;
    ga.ctr = fs->ctr;
    ga.n_flag = fs->ctr + kCtrFlag;
    ga.flag_list = fs->flag_list;
    ga.part_key = fs->g_key;
    ga.part_id = fs->g_id;
    ga.done = fs->done;
    ga.id_offset = id_offset;
    ga.D = D_dev;
    ga.I = I_dev;
    for (int f0 = 0; f0 < B; f0 += f_cap) {
        ga.f0 = f0;
        if (f32) hipLaunchKernelGGL(filter_gather_kernel<true>, dim3(gx, f_cap), dim3(kExThreads), 0, st, ga);
        else hipLaunchKernelGGL(filter_gather_kernel<false>, dim3(gx, f_cap), dim3(kExThreads), 0, st, ga);
        PRAG_LAUNCH_CHECK();
    }
    fs->last_B = B;
    fs->last_k = k;
    fs->masked_ran = masked_ok ? 1 : 0;
    if (!io_is_device) {
        PRAG_HIP(hipMemcpyAsync(D, D_dev, (size_t)B * k * sizeof(float), hipMemcpyDeviceToHost, st));
        PRAG_HIP(hipMemcpyAsync(I, I_dev, (size_t)B * k * sizeof(int64_t), hipMemcpyDeviceToHost, st));
        PRAG_HIP(hipStreamSynchronize(st));
    }
    return PRAG_OK;
}

extern "C" int prag_index_last_filter(prag_index_t* ix, void* stream, int64_t* n_selected, int64_t* n_tiles, int* path,
                                      int* n_flagged) {
    PRAG_REQUIRE(ix != nullptr, PRAG_EINVAL, "prag_index_last_filter: NULL handle");
    FilterState* fs = ix->filter;
    PRAG_REQUIRE(fs != nullptr && fs->last_B >= 0, PRAG_EINVAL, "prag_index_last_filter: no filtered search yet");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    PRAG_HIP(hipMemcpyAsync(fs->h_ctr.data(), fs->ctr, (size_t)kCtrWords * 4, hipMemcpyDeviceToHost, st));
    PRAG_HIP(hipStreamSynchronize(st));
    const uint32_t p = fs->h_ctr[kCtrPath];
    if (n_selected) *n_selected = (int64_t)fs->h_ctr[kCtrSel];
    if (n_tiles) *n_tiles = (int64_t)fs->h_ctr[kCtrTiles];
    if (path) *path = (int)p;
    if (n_flagged) *n_flagged = p == 1u ? (int)fs->h_ctr[kCtrFlag] : 0;
    return PRAG_OK;
}
