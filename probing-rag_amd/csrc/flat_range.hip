// Exact range search on the flat index: every stored row within `radius` of each query (include/prag.h
// prag_index_range_search, DESIGN.md section 2 "Range search").
//
//   range_scan_kernel    one pass over the rows: selection key on the matrix cores (fp16 query terms, f32
//                        accumulation, the key of the direct scans), a row is a CANDIDATE iff its key is within the
//                        certificate's error bound cert_eps of the radius on the inclusive side - every row outside
//                        that band is provably outside (or provably inside, and then it is a candidate too)
//   range_rerank_kernel  float64 score of every candidate (row_score64: the sum search's D comes from) and the strict
//                        test of the definition; per-query counts of the rows kept
//   (host)               counts -> lims; the call synchronises here anyway to return them
//   range_scatter_kernel kept pairs grouped by query, in the order the atomics landed ...
//   range_sort_tile_kernel / range_merge_pass_kernel  ... then sorted by row id: pieces of <= 4096 in LDS, longer
//                        segments by merge passes in global memory, so the output does not depend on that order
//   range_unpack_kernel  (row, D) pairs -> D float32 / I int64 held by the handle until prag_index_range_result
#include <algorithm>
#include <cmath>
#include <vector>

#include "flat_index_state.h"

namespace {

constexpr int64_t kRangeFirstCap = 1 << 20;   // candidate entries of a handle's first range search
constexpr int kRangeSortTile = 4096;          // segment pieces sorted in LDS (32 KiB of keys)
constexpr int kRangeMaxB = 1024;
constexpr int kCtrWords = 4 + 2 * kRangeMaxB; // [0..1] candidates found (u64), [2] n_flag, [4..) kept per query, fill

struct RangeScanArgs {
    const void* rows;          // [cap][d] as stored (cap a multiple of 256: the last tile's rows past N are readable)
    const float* xnorm;        // [cap]
    const _Float16* q16;       // [Bpad][d]
    int64_t N;
    int d;
    int qstride;               // LDS bytes per query row (multiple of 256)
    int n_tiles;               // ceil(N / 32)
    int B;
    float alpha;               // key = (use_norm ? ||x||^2 : 0) + alpha * dot, as the direct scans
    int use_norm;
    float radius;
    int metric_l2;
    CertArgs cert;             // qinfo / qn2 / xn_max and the rounding constants of this kernel (rq_sel = 1)
    unsigned long long* cand;  // [cap] (query << 32) | row
    int64_t cap;
    unsigned long long* n_cand;   // candidates found; may exceed cap (only the first cap are written)
};

// The rows' A operand of v_mfma_f32_32x32x16_f16 is loaded straight from memory (lane r + 32 hh: row r of the tile,
// elements [16 s + 8 hh, + 8) of k-step s): no LDS staging of rows.  The query tile sits in LDS (swizzled 16-B
// pieces, conflict-free fragment reads), NQ tiles of 32 queries per wave.
template <int NQ, bool F32>
__global__ __launch_bounds__(512) void range_scan_kernel(RangeScanArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int QT = 32 * NQ;
    constexpr int NLD = F32 ? 8 : 4;          // 16-B loads per lane per 64-element chunk
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, hh = lane >> 5;
    const int d = a.d, qstride = a.qstride;
    const int q0 = blockIdx.y * QT;
    float* s_thr = reinterpret_cast<float*>(smem + QT * qstride);
    if (tid < QT) {
        // candidate iff key <= thr: the key's bound on the inclusive side, rounded up to a float (NaN: nothing)
        const int b = q0 + tid;
        float t = -INFINITY;
        if (b < a.B) {
            const double eps = cert_eps(a.cert, b, a.metric_l2);
            const double lim = a.metric_l2 ? ((double)a.radius - a.cert.qn2[b]) + eps : -(double)a.radius + eps;
            t = (float)lim;
            if ((double)t < lim) t = nextafterf(t, INFINITY);
        }
        s_thr[tid] = t;
    }
    {
        const int ppr = d >> 3;
        for (int e = tid; e < QT * ppr; e += 512) {
            const int row = e / ppr, pc = e - row * ppr;
            const u32x4 v = *reinterpret_cast<const u32x4*>(a.q16 + (int64_t)(q0 + row) * d + 8 * pc);
            *reinterpret_cast<u32x4*>(smem + row * qstride + (((pc & ~15) | ((pc ^ row) & 15)) << 4)) = v;
        }
    }
    __syncthreads();
    float thr[NQ];
#pragma unroll
    for (int t = 0; t < NQ; ++t) thr[t] = s_thr[32 * t + r];

    const int nW = gridDim.x * 8;
    const int gw = blockIdx.x * 8 + w;
    const int n_my = gw < a.n_tiles ? (a.n_tiles - gw + nW - 1) / nW : 0;
    const int NCH = d >> 6;
    const int64_t row_bytes = (int64_t)d * (F32 ? 4 : 2);
    constexpr int chunk_bytes = 64 * (F32 ? 4 : 2);
    const int lane_off = r * (int)row_bytes + hh * (F32 ? 32 : 16);
    const char* rows = reinterpret_cast<const char*>(a.rows);
    const int tile_last = a.n_tiles - 1;
    auto issue = [&](u32x4 (&ld)[NLD], int tile, int c) {
        const int tc = tile < tile_last ? tile : tile_last;     // prefetch past the end: re-read the last tile
        const char* base = rows + (int64_t)tc * (32 * row_bytes) + c * chunk_bytes + lane_off;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            if constexpr (F32) {
                ld[2 * s] = *reinterpret_cast<const u32x4*>(base + 64 * s);
                ld[2 * s + 1] = *reinterpret_cast<const u32x4*>(base + 64 * s + 16);
            } else {
                ld[s] = *reinterpret_cast<const u32x4*>(base + 32 * s);
            }
        }
    };
    auto advance = [&](int& t, int& c) {
        const bool wrap = (c + 1 == NCH);
        c = wrap ? 0 : c + 1;
        t = wrap ? t + nW : t;
    };

    f32x16 acc[NQ];
#pragma unroll
    for (int t = 0; t < NQ; ++t)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[t][e] = 0.f;
    f32x4 xn[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) xn[g] = f32x4{0.f, 0.f, 0.f, 0.f};
    int tile_cur = gw, c_cur = 0, tile_nx = gw, c_nx = 0;

    auto body = [&](u32x4 (&ld)[NLD]) {
        if (a.use_norm && c_cur == 0) {   // norms of this tile's rows, waited for in its epilogue
#pragma unroll
            for (int g = 0; g < 4; ++g)
                xn[g] = *reinterpret_cast<const f32x4*>(a.xnorm + (int64_t)tile_cur * 32 + 8 * g + 4 * hh);
        }
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            half8 av;
            if constexpr (F32) {
                const f32x4 f0 = __builtin_bit_cast(f32x4, ld[2 * s]);
                const f32x4 f1 = __builtin_bit_cast(f32x4, ld[2 * s + 1]);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    av[e] = (_Float16)f0[e];
                    av[4 + e] = (_Float16)f1[e];
                }
            } else {
                av = __builtin_bit_cast(half8, ld[s]);
            }
            const int P = c_cur * 8 + 2 * s + hh;
#pragma unroll
            for (int t = 0; t < NQ; ++t) {
                const int qrow = 32 * t + r;
                const half8 bv = *reinterpret_cast<const half8*>(smem + qrow * qstride + (((P & ~15) | ((P ^ qrow) & 15)) << 4));
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(av, bv, acc[t], 0, 0, 0);
            }
        }
        issue(ld, tile_nx, c_nx);
        advance(tile_nx, c_nx);
        if (c_cur == NCH - 1) {
            // ---- epilogue: 16 rows x this lane's queries -> candidate bits, appended with one atomic per wave ----
            const int64_t doc0 = (int64_t)tile_cur * 32;
            uint32_t mask[NQ];
            int n = 0;
#pragma unroll
            for (int t = 0; t < NQ; ++t) {
                mask[t] = 0u;
#pragma unroll
                for (int g = 0; g < 4; ++g)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const bool valid = doc0 + 8 * g + 4 * hh + e < a.N;
                        const float key = fmaf(a.alpha, acc[t][4 * g + e], xn[g][e]);
                        if (valid && key <= thr[t]) mask[t] |= 1u << (4 * g + e);
                        acc[t][4 * g + e] = 0.f;
                    }
                n += __builtin_popcount(mask[t]);
            }
            if (__ballot(n != 0)) {
                int incl = n;
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) {
                    const int v = __shfl_up(incl, o, 64);
                    if (lane >= o) incl += v;
                }
                unsigned long long base = 0;
                if (lane == 63) base = atomicAdd(a.n_cand, (unsigned long long)incl);
                base = __shfl(base, 63, 64);
                unsigned long long off = base + (unsigned long long)(incl - n);
#pragma unroll
                for (int t = 0; t < NQ; ++t) {
                    uint32_t m = mask[t];
                    const unsigned long long qb = (unsigned long long)(q0 + 32 * t + r) << 32;
                    while (m) {
                        const int bit = __builtin_ctz(m);
                        m &= m - 1;
                        if (off < (unsigned long long)a.cap)
                            a.cand[off] = qb | (uint32_t)(doc0 + 8 * (bit >> 2) + 4 * hh + (bit & 3));
                        ++off;
                    }
                }
            }
        }
        advance(tile_cur, c_cur);
    };

    const int n_it = n_my * NCH;
    if (n_it > 0) {
        u32x4 ldA[NLD], ldB[NLD];
        issue(ldA, tile_nx, c_nx);
        advance(tile_nx, c_nx);
        issue(ldB, tile_nx, c_nx);
        advance(tile_nx, c_nx);
        int it = 0;
        for (; it + 1 < n_it; it += 2) {
            body(ldA);
            body(ldB);
        }
        if (it < n_it) body(ldA);
    }
}

// float64 score of every candidate (one wave each) and the strict test of the definition; a candidate that fails is
// overwritten with ~0.  Kept rows are counted per query in LDS first, one global atomic per workgroup and query
// (11.6 M same-address global atomics over 64 queries took 47 ms).
template <bool F32>
__global__ __launch_bounds__(256) void range_rerank_kernel(const void* __restrict__ rows, int d, int metric_l2,
                                                           const float* __restrict__ q32, int B, float radius,
                                                           unsigned long long* __restrict__ cand, float* __restrict__ cand_d,
                                                           const unsigned long long* __restrict__ n_cand, int64_t cap,
                                                           uint32_t* __restrict__ kcnt) {
    __shared__ uint32_t s_cnt[kRangeMaxB];
    for (int i = threadIdx.x; i < B; i += 256) s_cnt[i] = 0u;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int64_t n = (int64_t)min(*n_cand, (unsigned long long)cap);
    const double rad = (double)radius;
    for (int64_t c = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); c < n; c += (int64_t)gridDim.x * 4) {
        const unsigned long long e = cand[c];
        const int b = (int)(e >> 32);
        const int64_t row = (int64_t)(uint32_t)e;
        const double s = row_score64<F32>(rows, d, metric_l2, q32 + (int64_t)b * d, row, lane);
        const bool keep = metric_l2 ? s < rad : s > rad;
        if (lane == 0) {
            if (keep) {
                cand_d[c] = (float)s;
                atomicAdd(&s_cnt[b], 1u);
            } else {
                cand[c] = ~0ull;
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < B; i += 256)
        if (s_cnt[i]) atomicAdd(&kcnt[i], s_cnt[i]);
}

// kept candidates -> segment of their query, as (row << 32) | D bits (ascending key = ascending row: rows are unique
// within a segment).  Chunks of 2048 entries per workgroup: ranks from LDS atomics, then one global atomic per query
// reserves the chunk's slots in the segment.
constexpr int kScatterEpt = 8;
__global__ __launch_bounds__(256) void range_scatter_kernel(const unsigned long long* __restrict__ cand,
                                                            const float* __restrict__ cand_d,
                                                            const unsigned long long* __restrict__ n_cand, int64_t cap,
                                                            const int64_t* __restrict__ lims, int B,
                                                            uint32_t* __restrict__ fill,
                                                            unsigned long long* __restrict__ out) {
    __shared__ uint32_t s_cnt[kRangeMaxB];
    __shared__ uint32_t s_base[kRangeMaxB];
    const int64_t n = (int64_t)min(*n_cand, (unsigned long long)cap);
    constexpr int CH = 256 * kScatterEpt;
    for (int64_t c0 = (int64_t)blockIdx.x * CH; c0 < n; c0 += (int64_t)gridDim.x * CH) {
        for (int i = threadIdx.x; i < B; i += 256) s_cnt[i] = 0u;
        __syncthreads();
        unsigned long long e[kScatterEpt];
        uint32_t rank[kScatterEpt];
#pragma unroll
        for (int j = 0; j < kScatterEpt; ++j) {
            const int64_t i = c0 + j * 256 + threadIdx.x;
            e[j] = i < n ? cand[i] : ~0ull;
            rank[j] = e[j] != ~0ull ? atomicAdd(&s_cnt[(int)(e[j] >> 32)], 1u) : 0u;
        }
        __syncthreads();
        for (int i = threadIdx.x; i < B; i += 256)
            if (s_cnt[i]) s_base[i] = atomicAdd(&fill[i], s_cnt[i]);
        __syncthreads();
#pragma unroll
        for (int j = 0; j < kScatterEpt; ++j) {
            if (e[j] == ~0ull) continue;
            const int64_t i = c0 + j * 256 + threadIdx.x;
            const int b = (int)(e[j] >> 32);
            out[lims[b] + s_base[b] + rank[j]] = ((e[j] & 0xFFFFFFFFull) << 32) | __float_as_uint(cand_d[i]);
        }
        __syncthreads();
    }
}

// one piece (start, len <= 4096) of a segment per workgroup, bitonic sort in LDS
__global__ __launch_bounds__(1024) void range_sort_tile_kernel(unsigned long long* __restrict__ keys,
                                                               const int64_t* __restrict__ tiles) {
    __shared__ unsigned long long s[kRangeSortTile];
    const int64_t start = tiles[2 * blockIdx.x];
    const int len = (int)tiles[2 * blockIdx.x + 1];
    int n_pad = 2;
    while (n_pad < len) n_pad <<= 1;
    for (int i = threadIdx.x; i < n_pad; i += 1024) s[i] = i < len ? keys[start + i] : ~0ull;
    bitonic_sort_u64<1024>(s, n_pad);
    for (int i = threadIdx.x; i < len; i += 1024) keys[start + i] = s[i];
}

// one merge pass over every segment: sorted runs of w -> sorted runs of 2w (src -> dst).  Every key finds its place
// by counting the smaller keys of the partner run (binary search; keys are unique within a segment).
__global__ __launch_bounds__(256) void range_merge_pass_kernel(const unsigned long long* __restrict__ src,
                                                               unsigned long long* __restrict__ dst,
                                                               const int64_t* __restrict__ lims, int B, int64_t n,
                                                               int64_t w) {
    for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < n; p += (int64_t)gridDim.x * 256) {
        int lo = 0, hi = B - 1;     // the last query whose segment starts at or before p (it holds p)
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (lims[mid] <= p) lo = mid;
            else hi = mid - 1;
        }
        const int64_t seg0 = lims[lo], len = lims[lo + 1] - seg0, j = p - seg0;
        const unsigned long long key = src[p];
        const int64_t run = j / w, ps = (run ^ 1) * w;
        if (ps >= len) {
            dst[p] = key;
            continue;
        }
        const int64_t pe = min(ps + w, len);
        const unsigned long long* part = src + seg0 + ps;
        int64_t L = 0, H = pe - ps;
        while (L < H) {
            const int64_t m = (L + H) >> 1;
            if (part[m] < key) L = m + 1;
            else H = m;
        }
        dst[seg0 + (run & ~(int64_t)1) * w + (j - run * w) + L] = key;
    }
}

__global__ __launch_bounds__(256) void range_unpack_kernel(const unsigned long long* __restrict__ keys, int64_t n,
                                                           int64_t id_offset, float* __restrict__ D,
                                                           int64_t* __restrict__ I) {
    for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < n; p += (int64_t)gridDim.x * 256) {
        const unsigned long long k = keys[p];
        D[p] = __uint_as_float((uint32_t)k);
        I[p] = (int64_t)(k >> 32) + id_offset;
    }
}

}  // namespace

struct RangeState {
    int d = 0;
    float* q_in = nullptr;            // [kRangeMaxB][d] host queries staged on the device
    float* q32 = nullptr;             // [kRangeMaxB][d]
    _Float16* q16 = nullptr;          // [kRangeMaxB][d]
    _Float16* q16lo = nullptr;
    float* qinfo = nullptr;           // [kRangeMaxB][4]
    double* qn2 = nullptr;
    uint32_t* g_tau = nullptr;        // (written by the query prep, not read)
    uint32_t* g_slot = nullptr;
    uint32_t* ctr = nullptr;          // [kCtrWords]
    int64_t* lims_dev = nullptr;      // [kRangeMaxB + 1]
    int64_t* tiles_dev = nullptr;     // [tiles_cap][2]
    int64_t tiles_cap = 0;
    unsigned long long* cand = nullptr;   // [cand_cap]; also the second buffer of the merge passes
    float* cand_d = nullptr;
    int64_t cand_cap = 0;
    unsigned long long* kept = nullptr;   // [res_cap]
    float* res_D = nullptr;
    int64_t* res_I = nullptr;
    int64_t res_cap = 0;
    int64_t n_last = -1;              // results held (-1: none)
    int64_t n_cand_last = 0;          // candidates the last scan proposed
    std::vector<uint32_t> h_ctr;
    std::vector<int64_t> h_lims, h_tiles;
};

void range_state_free(prag_index* ix) {
    RangeState* rs = ix->range;
    if (!rs) return;
    for (void* p : {(void*)rs->q_in, (void*)rs->q32, (void*)rs->q16, (void*)rs->q16lo, (void*)rs->qinfo, (void*)rs->qn2,
                    (void*)rs->g_tau, (void*)rs->g_slot, (void*)rs->ctr, (void*)rs->lims_dev, (void*)rs->tiles_dev,
                    (void*)rs->cand, (void*)rs->cand_d, (void*)rs->kept, (void*)rs->res_D, (void*)rs->res_I})
        if (p) (void)hipFree(p);
    delete rs;
    ix->range = nullptr;
}

static int range_state(prag_index* ix, RangeState** out) {
    if (!ix->range) {
        RangeState* rs = new RangeState();
        rs->d = ix->d;
        const size_t qe = (size_t)kRangeMaxB * ix->d;
        const int rc = ws_regrow({{vpp(&rs->q_in), qe * 4}, {vpp(&rs->q32), qe * 4}, {vpp(&rs->q16), qe * 2},
                                  {vpp(&rs->q16lo), qe * 2}, {vpp(&rs->qinfo), (size_t)kRangeMaxB * 16},
                                  {vpp(&rs->qn2), (size_t)kRangeMaxB * 8}, {vpp(&rs->g_tau), (size_t)kRangeMaxB * 4},
                                  {vpp(&rs->g_slot), (size_t)kRangeMaxB * kSlotWordsFwd * 4},
                                  {vpp(&rs->ctr), (size_t)kCtrWords * 4}, {vpp(&rs->lims_dev), (size_t)(kRangeMaxB + 1) * 8},
                                  {vpp(&rs->cand), (size_t)kRangeFirstCap * 8}, {vpp(&rs->cand_d), (size_t)kRangeFirstCap * 4}});
        if (rc != PRAG_OK) {
            delete rs;
            return rc;
        }
        rs->cand_cap = kRangeFirstCap;
        rs->h_ctr.resize(kCtrWords);
        ix->range = rs;
    }
    *out = ix->range;
    return PRAG_OK;
}

// (re)allocate a pair of buffers to exactly `want` entries; on failure the old ones stay
template <typename A, typename Bt>
static int range_grow(A** a, Bt** b, int64_t* cap, int64_t want, const char* what) {
    A* na = nullptr;
    Bt* nb = nullptr;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&na), (size_t)want * sizeof(A));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&nb), (size_t)want * sizeof(Bt));
    if (e != hipSuccess) {
        if (na) (void)hipFree(na);
        (void)hipGetLastError();
        set_error("prag_index_range_search: %s of %lld entries: %s", what, (long long)want, hipGetErrorString(e));
        return e == hipErrorOutOfMemory ? PRAG_ENOMEM : PRAG_EHIP;
    }
    if (*a) (void)hipFree(*a);
    if (*b) (void)hipFree(*b);
    *a = na;
    *b = nb;
    *cap = want;
    return PRAG_OK;
}

template <int NQ, bool F32>
static int launch_range_scan(const RangeScanArgs& a, int grid_x, int grid_y, hipStream_t st) {
    auto kern = range_scan_kernel<NQ, F32>;
    static LdsOptIn lds_opt_in;
    const int rc = lds_opt_in.ensure(reinterpret_cast<const void*>(kern), 160 * 1024);
    if (rc != PRAG_OK) return rc;
    const int lds = 32 * NQ * a.qstride + 32 * NQ * 4;
    hipLaunchKernelGGL(kern, dim3(grid_x, grid_y), dim3(512), lds, st, a);
    PRAG_LAUNCH_CHECK();
    return PRAG_OK;
}

static int grid_for(int64_t n, int n_cu) { return (int)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, (int64_t)n_cu * 16)); }

extern "C" int prag_index_range_search(prag_index_t* ix, const float* q, int B, float radius, int64_t id_offset,
                                       int64_t* lims, int io_is_device, void* stream) {
    PRAG_REQUIRE(ix != nullptr && q != nullptr && lims != nullptr, PRAG_EINVAL, "prag_index_range_search: NULL pointer");
    PRAG_REQUIRE(B >= 1 && B <= kRangeMaxB, PRAG_EINVAL, "prag_index_range_search: B=%d (1..%d)", B, kRangeMaxB);
    RangeState* rs = nullptr;
    {
        const int rc = range_state(ix, &rs);
        if (rc != PRAG_OK) return rc;
    }
    rs->n_last = -1;
    if (ix->ntotal == 0) {
        std::fill(lims, lims + B + 1, (int64_t)0);
        rs->n_cand_last = 0;
        rs->n_last = 0;
        return PRAG_OK;
    }
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int d = ix->d;
    const bool f32 = ix->store == PRAG_F32;
    const int metric_l2 = ix->metric == PRAG_METRIC_L2;
    const float* q_dev = q;
    if (!io_is_device) {
        PRAG_HIP(hipMemcpyAsync(rs->q_in, q, (size_t)B * d * sizeof(float), hipMemcpyHostToDevice, st));
        q_dev = rs->q_in;
    }
    // two 32-query tiles per wave when they fit LDS next to each other (d <= 1024), else one
    const int NQ = (B > 32 && d <= 1024) ? 2 : 1;
    const int QT = 32 * NQ;
    const int Bpad = (B + QT - 1) / QT * QT;
    {
        int rc = index_refresh_xn_max(ix, st);
        if (rc == PRAG_OK)
            rc = index_prep_queries(ix, q_dev, B, Bpad, rs->q32, rs->q16, rs->q16lo, rs->qinfo, rs->qn2, rs->g_tau,
                                    rs->g_slot, rs->ctr + 2, st);
        if (rc != PRAG_OK) return rc;
    }
    RangeScanArgs a{};
    a.rows = ix->rows;
    a.xnorm = ix->xnorm;
    a.q16 = rs->q16;
    a.N = ix->ntotal;
    a.d = d;
    a.qstride = (d * 2 + 255) / 256 * 256;
    a.n_tiles = (int)((ix->ntotal + 31) / 32);
    a.B = B;
    a.alpha = metric_l2 ? -2.f : -1.f;
    a.use_norm = metric_l2;
    a.radius = radius;
    a.metric_l2 = metric_l2;
    {
        // the certificate's error model of a one-term fp16 selection (flat_index.hip search_certificate, not HP)
        CertArgs& c = a.cert;
        c.qinfo = rs->qinfo;
        c.qn2 = rs->qn2;
        c.xn_max = ix->cert_words + 1;
        const double u16 = 1.0 / 2048.0, sub = std::sqrt((double)d) * 2.9802322387695312e-08 /* 2^-25 */;
        c.rq_sel = 1;
        if (!f32) { c.c_row = 0.f; c.c_abs = 0.f; }
        else { c.c_row = (float)(u16 * (1.0 + u16) * 1.001); c.c_abs = (float)(sub * 1.001); }
        c.c_acc = (float)((double)d * 1.1920928955078125e-07 /* 2^-23 */ * 1.001);
    }
    const int grid_x = std::max(1, std::min(ix->n_cu, (a.n_tiles + 7) / 8));
    const int grid_y = Bpad / QT;
    uint32_t* kcnt = rs->ctr + 4;
    uint32_t* fill = rs->ctr + 4 + kRangeMaxB;
    unsigned long long* n_cand = reinterpret_cast<unsigned long long*>(rs->ctr);
    int64_t found = 0;
    for (int attempt = 0;; ++attempt) {
        a.cand = rs->cand;
        a.cap = rs->cand_cap;
        a.n_cand = n_cand;
        PRAG_HIP(hipMemsetAsync(rs->ctr, 0, (size_t)kCtrWords * 4, st));
        int rc;
        if (NQ == 2) rc = f32 ? launch_range_scan<2, true>(a, grid_x, grid_y, st) : launch_range_scan<2, false>(a, grid_x, grid_y, st);
        else rc = f32 ? launch_range_scan<1, true>(a, grid_x, grid_y, st) : launch_range_scan<1, false>(a, grid_x, grid_y, st);
        if (rc != PRAG_OK) return rc;
        const int rgrid = ix->n_cu * 16;
        if (f32)
            hipLaunchKernelGGL(range_rerank_kernel<true>, dim3(rgrid), dim3(256), 0, st, ix->rows, d, metric_l2, rs->q32,
                               B, radius, rs->cand, rs->cand_d, n_cand, rs->cand_cap, kcnt);
        else
            hipLaunchKernelGGL(range_rerank_kernel<false>, dim3(rgrid), dim3(256), 0, st, ix->rows, d, metric_l2, rs->q32,
                               B, radius, rs->cand, rs->cand_d, n_cand, rs->cand_cap, kcnt);
        PRAG_LAUNCH_CHECK();
        PRAG_HIP(hipMemcpyAsync(rs->h_ctr.data(), rs->ctr, (size_t)(4 + B) * 4, hipMemcpyDeviceToHost, st));
        PRAG_HIP(hipStreamSynchronize(st));
        found = (int64_t)(rs->h_ctr[0] | ((uint64_t)rs->h_ctr[1] << 32));
        if (found <= rs->cand_cap) break;
        // the store was full: grow it to the exact count and scan once more (the count does not change)
        PRAG_REQUIRE(attempt == 0, PRAG_EHIP, "prag_index_range_search: %lld candidates after growing to %lld",
                     (long long)found, (long long)rs->cand_cap);
        rc = range_grow(&rs->cand, &rs->cand_d, &rs->cand_cap, found, "candidate store");
        if (rc != PRAG_OK) return rc;
    }
    rs->n_cand_last = found;
    // ---- counts -> lims ----
    rs->h_lims.assign(B + 1, 0);
    int64_t max_len = 0;
    rs->h_tiles.clear();
    for (int b = 0; b < B; ++b) {
        const int64_t len = rs->h_ctr[4 + b];
        rs->h_lims[b + 1] = rs->h_lims[b] + len;
        max_len = std::max(max_len, len);
        for (int64_t t0 = 0; t0 < len; t0 += kRangeSortTile) {
            rs->h_tiles.push_back(rs->h_lims[b] + t0);
            rs->h_tiles.push_back(std::min<int64_t>(kRangeSortTile, len - t0));
        }
    }
    const int64_t n = rs->h_lims[B];
    std::copy(rs->h_lims.begin(), rs->h_lims.end(), lims);
    if (n == 0) {
        rs->n_last = 0;
        return PRAG_OK;
    }
    if (n > rs->res_cap) {
        int rc = range_grow(&rs->res_D, &rs->res_I, &rs->res_cap, n, "results");
        if (rc == PRAG_OK) {
            unsigned long long* nk = nullptr;
            const hipError_t e = hipMalloc(reinterpret_cast<void**>(&nk), (size_t)n * 8);
            if (e != hipSuccess) {
                (void)hipGetLastError();
                set_error("prag_index_range_search: %lld results: %s", (long long)n, hipGetErrorString(e));
                rc = e == hipErrorOutOfMemory ? PRAG_ENOMEM : PRAG_EHIP;
                rs->res_cap = 0;     // (kept no longer matches: the next call reallocates all three)
            } else {
                if (rs->kept) (void)hipFree(rs->kept);
                rs->kept = nk;
            }
        }
        if (rc != PRAG_OK) return rc;
    }
    const int64_t n_tiles = (int64_t)rs->h_tiles.size() / 2;
    if (n_tiles > rs->tiles_cap) {
        if (rs->tiles_dev) (void)hipFree(rs->tiles_dev);
        rs->tiles_dev = nullptr;
        rs->tiles_cap = 0;
        const int64_t want = std::max<int64_t>(n_tiles, 2 * kRangeMaxB);
        const hipError_t e = hipMalloc(reinterpret_cast<void**>(&rs->tiles_dev), (size_t)want * 16);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            rs->tiles_dev = nullptr;
            set_error("prag_index_range_search: sort table: %s", hipGetErrorString(e));
            return e == hipErrorOutOfMemory ? PRAG_ENOMEM : PRAG_EHIP;
        }
        rs->tiles_cap = want;
    }
    PRAG_HIP(hipMemcpyAsync(rs->lims_dev, rs->h_lims.data(), (size_t)(B + 1) * 8, hipMemcpyHostToDevice, st));
    PRAG_HIP(hipMemcpyAsync(rs->tiles_dev, rs->h_tiles.data(), (size_t)n_tiles * 16, hipMemcpyHostToDevice, st));
    // ---- group by query, then order every segment by row id ----
    hipLaunchKernelGGL(range_scatter_kernel, dim3(grid_for((found + kScatterEpt - 1) / kScatterEpt, ix->n_cu)),
                       dim3(256), 0, st, rs->cand, rs->cand_d, n_cand, rs->cand_cap, rs->lims_dev, B, fill, rs->kept);
    PRAG_LAUNCH_CHECK();
    hipLaunchKernelGGL(range_sort_tile_kernel, dim3((unsigned)n_tiles), dim3(1024), 0, st, rs->kept, rs->tiles_dev);
    PRAG_LAUNCH_CHECK();
    unsigned long long* src = rs->kept;
    unsigned long long* dst = rs->cand;      // n <= candidates found <= cand_cap
    for (int64_t w = kRangeSortTile; w < max_len; w *= 2) {
        hipLaunchKernelGGL(range_merge_pass_kernel, dim3(grid_for(n, ix->n_cu)), dim3(256), 0, st, src, dst, rs->lims_dev, B,
                           n, w);
        PRAG_LAUNCH_CHECK();
        std::swap(src, dst);
    }
    hipLaunchKernelGGL(range_unpack_kernel, dim3(grid_for(n, ix->n_cu)), dim3(256), 0, st, src, n, id_offset, rs->res_D,
                       rs->res_I);
    PRAG_LAUNCH_CHECK();
    rs->n_last = n;
    return PRAG_OK;
}

extern "C" int64_t prag_index_range_candidates(const prag_index_t* ix) {
    if (!ix || !ix->range || ix->range->n_last < 0) return -1;
    return ix->range->n_cand_last;
}

extern "C" int prag_index_range_result(prag_index_t* ix, float* D, int64_t* I, int64_t n, int out_is_device, void* stream) {
    PRAG_REQUIRE(ix != nullptr, PRAG_EINVAL, "prag_index_range_result: NULL handle");
    const int64_t have = ix->range ? ix->range->n_last : -1;
    PRAG_REQUIRE(have >= 0 && n == have, PRAG_EINVAL, "prag_index_range_result: n=%lld, the last range search holds %lld",
                 (long long)n, (long long)have);
    if (n == 0) return PRAG_OK;
    PRAG_REQUIRE(D != nullptr && I != nullptr, PRAG_EINVAL, "prag_index_range_result: NULL pointer");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const hipMemcpyKind kind = out_is_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    PRAG_HIP(hipMemcpyAsync(D, ix->range->res_D, (size_t)n * sizeof(float), kind, st));
    PRAG_HIP(hipMemcpyAsync(I, ix->range->res_I, (size_t)n * sizeof(int64_t), kind, st));
    if (!out_is_device) PRAG_HIP(hipStreamSynchronize(st));
    return PRAG_OK;
}
