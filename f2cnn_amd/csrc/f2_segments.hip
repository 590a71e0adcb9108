// Kernels and stage calls of `cnn eval --segments` (include/f2cnn_hip.h): f2_decision_path, f2_decision_runs, f2_interval_tally.
//   k_path_reduce       per tile of F2_PATH_TILE rows: the emissions q and the (max, +) product of the rows' 2 x 2 matrices
//   k_path_scan         per utterance: the vector that enters every tile, the optimum and the state of the last row
//   k_path_apply        per tile: the rows redone from that vector, a back pointer pair per row, their composition per tile
//   k_path_back_scan    per utterance: the state of the last row of every tile
//   k_path_back_apply   per tile: the back pointers of the rows composed from the right, the path written over them
//   k_runs_count / k_runs_scan / k_runs_scatter / k_runs_finish   boundary flags and q, their prefix sums, the runs
//   k_interval_tally    per (utterance, interval): four sums over the rows the interval owns
// gfx950, wave64. Reduce / scan / apply throughout: every kernel reads only what an earlier launch on the stream wrote, none waits for
// another workgroup. Everything is integer arithmetic behind the emissions, written by plain stores: the same bits on every call.
#include <cmath>

#include "f2_internal.h"
#include "f2_tile_owner.h"

namespace {

constexpr int SEG_THREADS = 256;
constexpr int SEG_PER = F2_PATH_TILE / SEG_THREADS;   // consecutive rows of a tile per thread
static_assert(F2_PATH_TILE % SEG_THREADS == 0, "a tile is whole rows of threads");
constexpr int SCAN_CHUNK = F2_PATH_SCAN_CHUNK;        // tiles the per-utterance scans take per step (one per thread)
static_assert(SCAN_CHUNK == SEG_THREADS, "one tile per thread and step");

// ---- the two monoids ----
// A 2 x 2 matrix over (max, +), a[from][to]; row j of an utterance is {{0, q - P}, {-P, q}} and V_j = V_{j-1} (x) M_j with
// V_{-1} = (0, 0) (which gives V_0 = (0, q_0) for any P >= 0). The entries of a product of rows are sums of at most 2^31 emissions
// below 2^24.1 in size and, for the best path with the ends it names, at most one penalty: |entry| < 2^56. MP_NEG stands for
// "no path" in the identity; A (x) I = A exactly while the entries of A differ by less than 2^60, and nothing overflows.
struct mp2 {
    long long a00, a01, a10, a11;
};
constexpr long long MP_NEG = -(1LL << 60);
__device__ inline long long mx(long long a, long long b) { return a > b ? a : b; }
struct mp_op {
    __device__ static mp2 identity() { return {0, MP_NEG, MP_NEG, 0}; }
    __device__ static mp2 apply(const mp2& A, const mp2& B) {   // A first, then B
        return {mx(A.a00 + B.a00, A.a01 + B.a10), mx(A.a00 + B.a01, A.a01 + B.a11), mx(A.a10 + B.a00, A.a11 + B.a10),
                mx(A.a10 + B.a01, A.a11 + B.a11)};
    }
};
__device__ inline mp2 row_matrix(long long q, long long P) { return {0, q - P, -P, q}; }

// A map {0, 1} -> {0, 1} in two bits: bit x is the image of x. 2 is the identity, 0 and 3 are the constants.
__device__ inline unsigned map_at(unsigned m, unsigned x) { return (m >> x) & 1u; }
__device__ inline unsigned map_after(unsigned outer, unsigned inner) {   // x -> outer(inner(x))
    return map_at(outer, map_at(inner, 0)) | map_at(outer, map_at(inner, 1)) << 1;
}
struct map_op {   // earlier rows are the outer maps: f_a o f_{a+1} o ... takes the state of the last row to the row before row a
    __device__ static unsigned identity() { return 2u; }
    __device__ static unsigned apply(unsigned A, unsigned B) { return map_after(A, B); }
};
struct map_rev_op {   // the same product with the operands arriving from the right
    __device__ static unsigned identity() { return 2u; }
    __device__ static unsigned apply(unsigned A, unsigned B) { return map_after(B, A); }
};

struct cnt2 {   // boundary flags and emissions of a span of rows
    long long c, s;
};
struct cnt_op {
    __device__ static cnt2 identity() { return {0, 0}; }
    __device__ static cnt2 apply(const cnt2& A, const cnt2& B) { return {A.c + B.c, A.s + B.s}; }
};

// Inclusive scan of one value per position 0 .. SEG_THREADS - 1 in position order (Hillis-Steele, two LDS buffers, a barrier per
// step; the operands keep their order, so any associative Op will do). Returns the buffer that holds the result: [pos] is the
// inclusive product, [pos - 1] the exclusive one, [SEG_THREADS - 1] the total. The caller puts a barrier before it reuses `buf`.
template <class Op, class T>
__device__ inline const T* block_scan(T (*buf)[SEG_THREADS], int pos, const T& v) {
    int cur = 0;
    buf[0][pos] = v;
    __syncthreads();
#pragma unroll 1
    for (int d = 1; d < SEG_THREADS; d <<= 1) {
        const T mine = buf[cur][pos];
        buf[cur ^ 1][pos] = pos >= d ? Op::apply(buf[cur][pos - d], mine) : mine;
        cur ^= 1;
        __syncthreads();
    }
    return buf[cur];
}
template <class Op, class T>
__device__ inline T scan_exclusive(const T* res, int pos) {
    return pos > 0 ? res[pos - 1] : Op::identity();
}

// the tile of a workgroup: utterance, first row (in the batch), rows, and whether the tile opens its utterance
struct tile_span {
    int u;
    long long base, rows, local0;   // local0: the utterance's row index of the tile's first row
};
__device__ inline tile_span tile_of(const int64_t* __restrict__ wo, const int64_t* __restrict__ first, int U, long long tile) {
    tile_span t;
    t.u = tile_owner(first, U, tile);
    t.local0 = (tile - first[t.u]) * F2_PATH_TILE;
    t.base = wo[t.u] + t.local0;
    const long long left = wo[t.u + 1] - t.base;
    t.rows = left < F2_PATH_TILE ? left : F2_PATH_TILE;
    return t;
}

// q_j of the header: float64 throughout, ties to even, 0 for a NaN
__device__ inline int emission(float p0, float p1, double scale) {
    if (p0 != p0 || p1 != p1) return 0;
    const double l1 = log(fmin(fmax((double)p1, 1e-7), 1.0)), l0 = log(fmin(fmax((double)p0, 1e-7), 1.0));
    return (int)rint(scale * (l1 - l0));
}

__global__ __launch_bounds__(SEG_THREADS) void k_path_reduce(const float* __restrict__ scores, const int64_t* __restrict__ wo,
                                                              const int64_t* __restrict__ first, int U, double scale, long long P,
                                                              int* __restrict__ q, mp2* __restrict__ tprod) {
    __shared__ mp2 buf[2][SEG_THREADS];
    const tile_span T = tile_of(wo, first, U, blockIdx.x);
    mp2 m = mp_op::identity();
#pragma unroll
    for (int i = 0; i < SEG_PER; ++i) {
        const long long r = (long long)threadIdx.x * SEG_PER + i;
        if (r < T.rows) {
            const int qj = emission(scores[2 * (T.base + r)], scores[2 * (T.base + r) + 1], scale);
            q[T.base + r] = qj;
            m = mp_op::apply(m, row_matrix(qj, P));
        }
    }
    const mp2* res = block_scan<mp_op>(buf, threadIdx.x, m);
    if (threadIdx.x == 0) tprod[blockIdx.x] = res[SEG_THREADS - 1];
}

__device__ inline void vec_times(long long& v0, long long& v1, const mp2& M) {
    const long long n0 = mx(v0 + M.a00, v1 + M.a10), n1 = mx(v0 + M.a01, v1 + M.a11);
    v0 = n0, v1 = n1;
}

// One workgroup per utterance, SCAN_CHUNK tiles per step: vin[tile] = (0, 0) (x) the product of the tiles before it.
__global__ __launch_bounds__(SEG_THREADS) void k_path_scan(const mp2* __restrict__ tprod, const int64_t* __restrict__ first,
                                                            long long* __restrict__ vin, long long* __restrict__ value,
                                                            uint8_t* __restrict__ xlast) {
    __shared__ mp2 buf[2][SEG_THREADS];
    const int u = blockIdx.x;
    const long long t0 = first[u], nt = first[u + 1] - t0;
    long long c0 = 0, c1 = 0;
    for (long long s = 0; s < nt; s += SCAN_CHUNK) {
        const long long k = s + threadIdx.x;
        const mp2* res = block_scan<mp_op>(buf, threadIdx.x, k < nt ? tprod[t0 + k] : mp_op::identity());
        if (k < nt) {
            long long v0 = c0, v1 = c1;
            vec_times(v0, v1, scan_exclusive<mp_op>(res, threadIdx.x));
            vin[2 * (t0 + k)] = v0, vin[2 * (t0 + k) + 1] = v1;
        }
        vec_times(c0, c1, res[SEG_THREADS - 1]);
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        value[u] = mx(c0, c1);
        xlast[u] = c1 > c0;   // a tie is falling
    }
}

// The rows of a tile from the vector that enters it. bp[j] holds the pair bp_j(0) | bp_j(1) << 1 as a map (the first row of an
// utterance: the identity, which nothing reads), tmap[tile] the product of the tile's maps.
__global__ __launch_bounds__(SEG_THREADS) void k_path_apply(const int* __restrict__ q, const int64_t* __restrict__ wo,
                                                             const int64_t* __restrict__ first, int U, long long P,
                                                             const long long* __restrict__ vin, uint8_t* __restrict__ bp,
                                                             uint8_t* __restrict__ tmap) {
    __shared__ mp2 buf[2][SEG_THREADS];
    __shared__ unsigned mbuf[2][SEG_THREADS];
    const tile_span T = tile_of(wo, first, U, blockIdx.x);
    int qs[SEG_PER];
    mp2 m = mp_op::identity();
#pragma unroll
    for (int i = 0; i < SEG_PER; ++i) {
        const long long r = (long long)threadIdx.x * SEG_PER + i;
        qs[i] = r < T.rows ? q[T.base + r] : 0;
        if (r < T.rows) m = mp_op::apply(m, row_matrix(qs[i], P));
    }
    const mp2* res = block_scan<mp_op>(buf, threadIdx.x, m);
    long long v0 = vin[2 * (long long)blockIdx.x], v1 = vin[2 * (long long)blockIdx.x + 1];
    vec_times(v0, v1, scan_exclusive<mp_op>(res, threadIdx.x));
    unsigned maps = map_op::identity();
#pragma unroll
    for (int i = 0; i < SEG_PER; ++i) {
        const long long r = (long long)threadIdx.x * SEG_PER + i;
        if (r < T.rows) {
            unsigned code = 2u;
            if (T.local0 + r > 0) code = (v0 >= v1 - P ? 0u : 1u) | (v1 >= v0 - P ? 2u : 0u);   // a tie stays
            bp[T.base + r] = (uint8_t)code;
            maps = map_op::apply(maps, code);
            const long long n0 = mx(v0, v1 - P), n1 = mx(v1, v0 - P) + qs[i];
            v0 = n0, v1 = n1;
        }
    }
    const unsigned* mres = block_scan<map_op>(mbuf, threadIdx.x, maps);
    if (threadIdx.x == 0) tmap[blockIdx.x] = (uint8_t)mres[SEG_THREADS - 1];
}

// One workgroup per utterance, SCAN_CHUNK tiles per step from the last tile down: xin[tile] = the state of the tile's last row,
// which is the product of the maps of all later tiles at the state of the utterance's last row.
__global__ __launch_bounds__(SEG_THREADS) void k_path_back_scan(const uint8_t* __restrict__ tmap, const int64_t* __restrict__ first,
                                                                 const uint8_t* __restrict__ xlast, uint8_t* __restrict__ xin) {
    __shared__ unsigned mbuf[2][SEG_THREADS];
    const int u = blockIdx.x;
    const long long t0 = first[u], nt = first[u + 1] - t0;
    unsigned x = xlast[u];
    for (long long e = nt; e > 0; e -= SCAN_CHUNK) {
        const long long k = e - 1 - threadIdx.x;   // position p of the scan is tile e - 1 - p
        const unsigned* res = block_scan<map_rev_op>(mbuf, threadIdx.x, k >= 0 ? (unsigned)tmap[t0 + k] : 2u);
        if (k >= 0) xin[t0 + k] = (uint8_t)map_at(scan_exclusive<map_rev_op>(res, threadIdx.x), x);
        x = map_at(res[SEG_THREADS - 1], x);
        __syncthreads();
    }
}

// x_{j-1} = bp_j(x_j) inside a tile, from the state of its last row; the path goes where the back pointers were.
__global__ __launch_bounds__(SEG_THREADS) void k_path_back_apply(const int64_t* __restrict__ wo, const int64_t* __restrict__ first, int U,
                                                                  const uint8_t* __restrict__ xin, uint8_t* bp_path) {
    __shared__ unsigned mbuf[2][SEG_THREADS];
    const tile_span T = tile_of(wo, first, U, blockIdx.x);
    unsigned code[SEG_PER], maps = 2u;
#pragma unroll
    for (int i = 0; i < SEG_PER; ++i) {
        const long long r = (long long)threadIdx.x * SEG_PER + i;
        code[i] = r < T.rows ? (unsigned)bp_path[T.base + r] : 2u;   // (rows past the end hand the state through)
        maps = map_op::apply(maps, code[i]);
    }
    // position p of the scan is thread SEG_THREADS - 1 - p: the exclusive product is that of the threads to the right
    const int pos = SEG_THREADS - 1 - (int)threadIdx.x;
    const unsigned* res = block_scan<map_rev_op>(mbuf, pos, maps);
    unsigned x = map_at(scan_exclusive<map_rev_op>(res, pos), (unsigned)xin[blockIdx.x]);   // the state of this thread's last row
#pragma unroll
    for (int i = SEG_PER - 1; i >= 0; --i) {
        const long long r = (long long)threadIdx.x * SEG_PER + i;
        if (r < T.rows) bp_path[T.base + r] = (uint8_t)x;
        x = map_at(code[i], x);
    }
}

// ---- runs ----
// Row j opens a run when it is the first of its utterance or its label differs from the row before.
__device__ inline bool opens_run(const uint8_t* __restrict__ labels, const tile_span& T, long long r) {
    return T.local0 + r == 0 || (labels[T.base + r] != 0) != (labels[T.base + r - 1] != 0);
}

__global__ __launch_bounds__(SEG_THREADS) void k_runs_count(const uint8_t* __restrict__ labels, const int* __restrict__ q,
                                                             const int64_t* __restrict__ wo, const int64_t* __restrict__ first, int U,
                                                             long long* __restrict__ tcount, long long* __restrict__ tqsum) {
    __shared__ cnt2 buf[2][SEG_THREADS];
    const tile_span T = tile_of(wo, first, U, blockIdx.x);
    cnt2 c = {0, 0};
#pragma unroll
    for (int i = 0; i < SEG_PER; ++i) {
        const long long r = (long long)threadIdx.x * SEG_PER + i;
        if (r < T.rows) {
            c.c += opens_run(labels, T, r);
            if (q) c.s += q[T.base + r];
        }
    }
    const cnt2* res = block_scan<cnt_op>(buf, threadIdx.x, c);
    if (threadIdx.x == 0) tcount[blockIdx.x] = res[SEG_THREADS - 1].c, tqsum[blockIdx.x] = res[SEG_THREADS - 1].s;
}

// One workgroup: the tile sums become their exclusive prefix sums in place, entry [tiles] the totals; ro[u] = runs before utterance u.
__global__ __launch_bounds__(SEG_THREADS) void k_runs_scan(long long* __restrict__ tcount, long long* __restrict__ tqsum, long long tiles,
                                                            const int64_t* __restrict__ first, int U, long long* __restrict__ ro) {
    __shared__ cnt2 buf[2][SEG_THREADS];
    cnt2 carry = {0, 0};
    for (long long s = 0; s < tiles; s += SCAN_CHUNK) {
        const long long k = s + threadIdx.x;
        const cnt2 mine = k < tiles ? cnt2{tcount[k], tqsum[k]} : cnt2{0, 0};
        const cnt2* res = block_scan<cnt_op>(buf, threadIdx.x, mine);
        if (k < tiles) {
            const cnt2 ex = cnt_op::apply(carry, scan_exclusive<cnt_op>(res, threadIdx.x));
            tcount[k] = ex.c, tqsum[k] = ex.s;
        }
        carry = cnt_op::apply(carry, res[SEG_THREADS - 1]);
        __syncthreads();
    }
    if (threadIdx.x == 0) tcount[tiles] = carry.c, tqsum[tiles] = carry.s;
    __syncthreads();   // (the workgroup's own global stores, read back below)
    for (int u = threadIdx.x; u <= U; u += SEG_THREADS) ro[u] = tcount[first[u]];
}

// Run r opens at the r-th flagged row of the batch: its first row and label go to runs[r], its first row in the batch and the sum
// of q before it to rstart[r] / rsum[r], from which k_runs_finish takes the two differences.
__global__ __launch_bounds__(SEG_THREADS) void k_runs_scatter(const uint8_t* __restrict__ labels, const int* __restrict__ q,
                                                               const int64_t* __restrict__ wo, const int64_t* __restrict__ first, int U,
                                                               const long long* __restrict__ tcount, const long long* __restrict__ tqsum,
                                                               long long* __restrict__ runs, long long* __restrict__ rstart,
                                                               long long* __restrict__ rsum) {
    __shared__ cnt2 buf[2][SEG_THREADS];
    const tile_span T = tile_of(wo, first, U, blockIdx.x);
    bool open[SEG_PER];
    int qs[SEG_PER];
    cnt2 c = {0, 0};
#pragma unroll
    for (int i = 0; i < SEG_PER; ++i) {
        const long long r = (long long)threadIdx.x * SEG_PER + i;
        open[i] = r < T.rows && opens_run(labels, T, r);
        qs[i] = r < T.rows && q ? q[T.base + r] : 0;
        c.c += open[i], c.s += qs[i];
    }
    const cnt2* res = block_scan<cnt_op>(buf, threadIdx.x, c);
    const cnt2 ex = scan_exclusive<cnt_op>(res, threadIdx.x);
    long long run = tcount[blockIdx.x] + ex.c, sum = tqsum[blockIdx.x] + ex.s;
#pragma unroll
    for (int i = 0; i < SEG_PER; ++i) {
        const long long r = (long long)threadIdx.x * SEG_PER + i;
        if (open[i]) {
            runs[4 * run] = T.local0 + r, runs[4 * run + 2] = labels[T.base + r] != 0;
            rstart[run] = T.base + r, rsum[run] = sum;
            ++run;
        }
        sum += qs[i];
    }
}

__global__ __launch_bounds__(SEG_THREADS) void k_runs_finish(long long* __restrict__ runs, const long long* __restrict__ rstart,
                                                              const long long* __restrict__ rsum, const long long* __restrict__ n_runs,
                                                              const long long* __restrict__ q_total, long long n_rows) {
    const long long r = (long long)blockIdx.x * SEG_THREADS + threadIdx.x, n = *n_runs;
    if (r >= n) return;
    const bool last = r + 1 == n;
    runs[4 * r + 1] = (last ? n_rows : rstart[r + 1]) - rstart[r];
    runs[4 * r + 3] = (last ? *q_total : rsum[r + 1]) - rsum[r];
}

// ---- tally ----
// Workgroup i serves output row i: utterance u = (i / M) R + r, interval k of set r, M = ivo[R] the intervals of all sets. The
// interval [a, b) owns the rows j with a <= origin + j hop < b: ceil((a - origin) / hop) <= j < ceil((b - origin) / hop), cut to
// the utterance's rows (a bound at or before origin: 0).
__device__ inline long long first_row_at(long long bound, long long origin, long long hop, long long rows) {
    if (bound <= origin) return 0;
    const unsigned long long d = (unsigned long long)bound - (unsigned long long)origin;   // (exact for any int64 pair)
    const unsigned long long j = d / (unsigned long long)hop + (d % (unsigned long long)hop != 0);
    return j < (unsigned long long)rows ? (long long)j : rows;
}

__global__ __launch_bounds__(SEG_THREADS) void k_interval_tally(const uint8_t* __restrict__ labels, const uint8_t* __restrict__ path,
                                                                 const int* __restrict__ q, const int64_t* __restrict__ wo,
                                                                 const int64_t* __restrict__ ivo, const int64_t* __restrict__ ivb, int R,
                                                                 long long origin, long long hop, long long* __restrict__ tally) {
    __shared__ cnt2 buf[2][SEG_THREADS];
    const long long M = ivo[R], cycle = (long long)blockIdx.x / M, within = (long long)blockIdx.x % M;
    const int r = tile_owner(ivo, R, within);
    const long long u = cycle * R + r, rows = wo[u + 1] - wo[u];
    const long long j0 = first_row_at(ivb[2 * within], origin, hop, rows), j1 = first_row_at(ivb[2 * within + 1], origin, hop, rows);
    cnt2 a = {0, 0}, b = {0, 0};   // {labels, path}, {q, unused}
    for (long long j = j0 + threadIdx.x; j < j1; j += SEG_THREADS) {
        a.c += labels[wo[u] + j] != 0;
        if (path) a.s += path[wo[u] + j] != 0;
        if (q) b.c += q[wo[u] + j];
    }
    const cnt2* res = block_scan<cnt_op>(buf, threadIdx.x, a);
    const cnt2 ta = res[SEG_THREADS - 1];
    __syncthreads();
    res = block_scan<cnt_op>(buf, threadIdx.x, b);
    if (threadIdx.x == 0) {
        long long* o = tally + 4 * (long long)blockIdx.x;
        o[0] = j1 > j0 ? j1 - j0 : 0, o[1] = ta.c, o[2] = ta.s, o[3] = res[SEG_THREADS - 1].c;
    }
}

constexpr double SCALE_MAX = 1048576.0;          // 2^20
constexpr int64_t PENALTY_MAX = int64_t(1) << 40;

}  // namespace

// ---- what the stage calls and the fused call (f2_pipeline.hip) share ----

int f2_check_decision_path(f2_ctx* ctx, double logit_scale, int64_t penalty) {
    F2_CHECK(ctx, std::isfinite(logit_scale) && logit_scale > 0.0, F2_ERR_INVALID, "logit_scale (%g) must be finite and above 0", logit_scale);
    F2_CHECK(ctx, penalty >= 0, F2_ERR_INVALID, "penalty (%lld) must not be negative", (long long)penalty);
    F2_CHECK(ctx, logit_scale <= SCALE_MAX, F2_ERR_UNSUPPORTED, "logit_scale %g (at most 2^20)", logit_scale);
    F2_CHECK(ctx, penalty <= PENALTY_MAX, F2_ERR_UNSUPPORTED, "penalty %lld (at most 2^40)", (long long)penalty);
    return F2_OK;
}

int f2_check_segment_rows(f2_ctx* ctx, int64_t n_rows) {
    F2_CHECK(ctx, n_rows < (int64_t(1) << 31), F2_ERR_UNSUPPORTED, "%lld rows (fewer than 2^31)", (long long)n_rows);
    return F2_OK;
}

int f2_check_intervals(f2_ctx* ctx, int U, const int64_t* iv_offsets, const int64_t* iv_bounds, int R, int64_t origin, int hop,
                       int64_t max_rows, int64_t* out_rows) {
    F2_CHECK(ctx, U >= 0 && R >= (U > 0 ? 1 : 0) && (U == 0 || U % R == 0), F2_ERR_INVALID,
             "%d utterances cannot be tallied against %d interval sets in turn", U, R);
    F2_CHECK(ctx, hop >= 1 && origin >= 0, F2_ERR_INVALID, "hop (%d) must be at least 1, origin (%lld) at least 0", hop, (long long)origin);
    F2_TRY(f2_check_offsets(ctx, iv_offsets, R, "iv_offsets"));
    const int64_t M = iv_offsets[R];
    F2_CHECK(ctx, iv_bounds || M == 0, F2_ERR_INVALID, "null iv_bounds");
    for (int r = 0; r < R; ++r)
        for (int64_t k = iv_offsets[r]; k < iv_offsets[r + 1]; ++k) {
            const int64_t a = iv_bounds[2 * k], b = iv_bounds[2 * k + 1];
            F2_CHECK(ctx, a >= 0 && a <= b && (k == iv_offsets[r] || iv_bounds[2 * k - 1] <= a), F2_ERR_INVALID,
                     "interval set %d: interval %lld [%lld, %lld) is negative, reversed or starts before the one before it ends", r,
                     (long long)(k - iv_offsets[r]), (long long)a, (long long)b);
        }
    int64_t t_last = 0, out = 0;
    F2_CHECK(ctx, max_rows == 0 || (!__builtin_mul_overflow(max_rows - 1, (int64_t)hop, &t_last) && !__builtin_add_overflow(t_last, origin, &t_last)),
             F2_ERR_UNSUPPORTED, "row %lld at hop %d from origin %lld is beyond int64", (long long)(max_rows - 1), hop, (long long)origin);
    F2_CHECK(ctx, U == 0 || (!__builtin_mul_overflow((int64_t)(U / R), M, &out) && out < (int64_t(1) << 31)), F2_ERR_UNSUPPORTED,
             "%d utterances of %lld intervals per %d (fewer than 2^31 tally rows)", U, (long long)M, R);
    *out_rows = out;
    return F2_OK;
}

void f2_seg_plan::set(const int64_t* window_offsets, int U_) {
    U = U_, wo = window_offsets, n_rows = U > 0 ? window_offsets[U] : 0;
    tiles = f2_tile_table(window_offsets, U, F2_PATH_TILE, &first);
    max_rows = 0;
    for (int u = 0; u < U; ++u) max_rows = std::max(max_rows, window_offsets[u + 1] - window_offsets[u]);
}

// Every array of the call is named once (take), then reserve() sizes ctx->seg_ws and sets the pointers: one block per call, reserved
// before its first launch, since a block that grows is a new block.
template <class T>
static void seg_take(f2_seg_plan* S, T** slot, size_t count) {
    S->slots.push_back({(void*)slot, S->bytes});
    S->bytes += (sizeof(T) * count + 7) & ~size_t(7);
}

void f2_seg_plan::name_arrays(bool want_path, bool want_runs, int64_t intervals, int R) {
    const size_t t = (size_t)tiles, n = (size_t)n_rows, u = (size_t)U;
    seg_take(this, &d_wo, u + 1), seg_take(this, &d_first, u + 1);
    if (want_path) {
        seg_take(this, &d_tprod, 4 * t), seg_take(this, &d_vin, 2 * t), seg_take(this, &d_value, u);
        seg_take(this, &d_tmap, t), seg_take(this, &d_xin, t), seg_take(this, &d_xlast, u);
    }
    if (want_runs) {
        seg_take(this, &d_tcount, t + 1), seg_take(this, &d_tqsum, t + 1), seg_take(this, &d_ro, u + 1);
        seg_take(this, &d_rstart, n), seg_take(this, &d_rsum, n);
    }
    if (R > 0) seg_take(this, &d_ivo, (size_t)R + 1), seg_take(this, &d_ivb, 2 * (size_t)intervals);
}

void f2_seg_plan::name_bytes(char** slot, size_t bytes) { seg_take(this, slot, bytes); }

int f2_seg_plan::reserve(f2_ctx* ctx) {
    F2_TRY(f2_reserve(ctx, ctx->seg_ws, bytes));
    for (const auto& s : slots) {
        char* at = (char*)ctx->seg_ws.ptr + s.at;
        memcpy(s.slot, &at, sizeof(at));   // (the slot is a T*: object pointers share one representation)
    }
    return F2_OK;
}

int f2_seg_plan::upload_tables(f2_ctx* ctx) const {
    F2_TRY(f2_upload_async(ctx, d_wo, wo, sizeof(int64_t) * ((size_t)U + 1)));
    return f2_upload_async(ctx, d_first, first.data(), sizeof(int64_t) * ((size_t)U + 1));
}

int f2_launch_decision_path(f2_ctx* ctx, const f2_seg_plan& S, const float* d_scores, double logit_scale, int64_t penalty, uint8_t* d_path,
                            int32_t* d_q) {
    if (S.U == 0) return F2_OK;
    const dim3 tiles((unsigned)S.tiles), utts((unsigned)S.U), wg(SEG_THREADS);
    if (S.tiles > 0) {
        k_path_reduce<<<tiles, wg, 0, ctx->stream>>>(d_scores, S.d_wo, S.d_first, S.U, logit_scale, (long long)penalty, d_q, (mp2*)S.d_tprod);
        F2_HIP(ctx, hipGetLastError());
    }
    k_path_scan<<<utts, wg, 0, ctx->stream>>>((const mp2*)S.d_tprod, S.d_first, (long long*)S.d_vin, (long long*)S.d_value, S.d_xlast);
    F2_HIP(ctx, hipGetLastError());
    if (S.tiles == 0) return F2_OK;
    k_path_apply<<<tiles, wg, 0, ctx->stream>>>(d_q, S.d_wo, S.d_first, S.U, (long long)penalty, (const long long*)S.d_vin, d_path, S.d_tmap);
    F2_HIP(ctx, hipGetLastError());
    k_path_back_scan<<<utts, wg, 0, ctx->stream>>>(S.d_tmap, S.d_first, S.d_xlast, S.d_xin);
    F2_HIP(ctx, hipGetLastError());
    k_path_back_apply<<<tiles, wg, 0, ctx->stream>>>(S.d_wo, S.d_first, S.U, S.d_xin, d_path);
    F2_HIP(ctx, hipGetLastError());
    return F2_OK;
}

int f2_launch_runs_count(f2_ctx* ctx, const f2_seg_plan& S, const uint8_t* d_labels, const int32_t* d_q) {
    const dim3 wg(SEG_THREADS);
    if (S.tiles > 0) {
        k_runs_count<<<dim3((unsigned)S.tiles), wg, 0, ctx->stream>>>(d_labels, d_q, S.d_wo, S.d_first, S.U, (long long*)S.d_tcount,
                                                                     (long long*)S.d_tqsum);
        F2_HIP(ctx, hipGetLastError());
    }
    k_runs_scan<<<dim3(1), wg, 0, ctx->stream>>>((long long*)S.d_tcount, (long long*)S.d_tqsum, (long long)S.tiles, S.d_first, S.U,
                                                 (long long*)S.d_ro);
    F2_HIP(ctx, hipGetLastError());
    return F2_OK;
}

int f2_launch_runs_scatter(f2_ctx* ctx, const f2_seg_plan& S, const uint8_t* d_labels, const int32_t* d_q, int64_t most_runs, int64_t* d_runs) {
    if (S.tiles == 0 || most_runs == 0) return F2_OK;
    const dim3 wg(SEG_THREADS);
    k_runs_scatter<<<dim3((unsigned)S.tiles), wg, 0, ctx->stream>>>(d_labels, d_q, S.d_wo, S.d_first, S.U, (const long long*)S.d_tcount,
                                                                   (const long long*)S.d_tqsum, (long long*)d_runs, (long long*)S.d_rstart,
                                                                   (long long*)S.d_rsum);
    F2_HIP(ctx, hipGetLastError());
    k_runs_finish<<<dim3((unsigned)((most_runs + SEG_THREADS - 1) / SEG_THREADS)), wg, 0, ctx->stream>>>(
        (long long*)d_runs, (const long long*)S.d_rstart, (const long long*)S.d_rsum, (const long long*)S.d_tcount + S.tiles,
        (const long long*)S.d_tqsum + S.tiles, (long long)S.n_rows);
    F2_HIP(ctx, hipGetLastError());
    return F2_OK;
}

int f2_launch_interval_tally(f2_ctx* ctx, const f2_seg_plan& S, const uint8_t* d_labels, const uint8_t* d_path, const int32_t* d_q,
                             const int64_t* iv_offsets, const int64_t* iv_bounds, int R, int64_t origin, int hop, int64_t out_rows,
                             int64_t* d_tally) {
    if (out_rows == 0) return F2_OK;
    F2_TRY(f2_upload_async(ctx, S.d_ivo, iv_offsets, sizeof(int64_t) * ((size_t)R + 1)));
    F2_TRY(f2_upload_async(ctx, S.d_ivb, iv_bounds, sizeof(int64_t) * 2 * (size_t)iv_offsets[R]));
    k_interval_tally<<<dim3((unsigned)out_rows), dim3(SEG_THREADS), 0, ctx->stream>>>(d_labels, d_path, d_q, S.d_wo, S.d_ivo, S.d_ivb, R,
                                                                                     (long long)origin, (long long)hop, (long long*)d_tally);
    F2_HIP(ctx, hipGetLastError());
    return F2_OK;
}

namespace {

// An input of a stage call on the device: the caller's pointer, or the slot of the plan's block it is copied into
int seg_stage(f2_ctx* ctx, const void* src, char* slot, size_t bytes, int mem_space, const void** d_src) {
    *d_src = src;
    if (mem_space == F2_MEM_DEVICE || !src || bytes == 0) return F2_OK;
    F2_HIP(ctx, hipMemcpyAsync(slot, src, bytes, hipMemcpyHostToDevice, ctx->stream));
    *d_src = slot;
    return F2_OK;
}

// An output likewise (f2_place's rule, with the plan's block as the area)
f2_output seg_output(void* caller_or_null, char* slot, size_t bytes, int mem_space) {
    f2_output o;
    o.bytes = bytes;
    if (mem_space == F2_MEM_DEVICE && caller_or_null) o.dev = (char*)caller_or_null, o.callers = true;
    else o.dev = slot, o.host = mem_space == F2_MEM_DEVICE ? nullptr : (char*)caller_or_null;
    return o;
}
bool seg_needs_slot(const void* caller_or_null, int mem_space) { return mem_space != F2_MEM_DEVICE || !caller_or_null; }

}  // namespace

extern "C" {

int f2_decision_path(f2_ctx* ctx, const float* scores, const int64_t* window_offsets, int U, double logit_scale, int64_t penalty,
                     uint8_t* path, int32_t* emissions_or_null, int64_t* value_or_null, int mem_space) {
    F2_TRY(f2_check_ctx(ctx));
    F2_TRY(f2_check_mem_space(ctx, mem_space, false));
    F2_CHECK(ctx, U >= 0, F2_ERR_INVALID, "negative utterance count (%d)", U);
    F2_TRY(f2_check_offsets(ctx, window_offsets, U, "window_offsets"));
    const int64_t n_rows = window_offsets[U];
    F2_CHECK(ctx, (scores && path) || n_rows == 0, F2_ERR_INVALID, "null scores or path");
    F2_TRY(f2_check_decision_path(ctx, logit_scale, penalty));
    F2_TRY(f2_check_segment_rows(ctx, n_rows));
    if (n_rows == 0) {
        if (value_or_null) std::fill(value_or_null, value_or_null + U, (int64_t)0);
        return F2_OK;
    }
    const size_t n = (size_t)n_rows;
    f2_seg_plan S;
    S.set(window_offsets, U);
    S.name_arrays(true, false, 0, 0);
    char *s_scores = nullptr, *s_path = nullptr, *s_q = nullptr;
    if (mem_space != F2_MEM_DEVICE) S.name_bytes(&s_scores, sizeof(float) * 2 * n);
    if (seg_needs_slot(path, mem_space)) S.name_bytes(&s_path, n);
    if (seg_needs_slot(emissions_or_null, mem_space)) S.name_bytes(&s_q, sizeof(int32_t) * n);
    F2_TRY(S.reserve(ctx));
    const void* d_scores;
    F2_TRY(seg_stage(ctx, scores, s_scores, sizeof(float) * 2 * n, mem_space, &d_scores));
    const f2_output o_path = seg_output(path, s_path, n, mem_space), o_q = seg_output(emissions_or_null, s_q, sizeof(int32_t) * n, mem_space);
    F2_TRY(S.upload_tables(ctx));
    F2_TRY(f2_launch_decision_path(ctx, S, (const float*)d_scores, logit_scale, penalty, o_path.as<uint8_t>(), o_q.as<int32_t>()));
    F2_TRY(f2_copy_back(ctx, o_path));
    F2_TRY(f2_copy_back(ctx, o_q));
    if (!value_or_null) return f2_host_wait(ctx, mem_space);
    F2_HIP(ctx, hipMemcpyAsync(value_or_null, S.d_value, sizeof(int64_t) * (size_t)U, hipMemcpyDeviceToHost, ctx->stream));
    F2_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return F2_OK;
}

int f2_decision_runs(f2_ctx* ctx, const uint8_t* labels, const int32_t* emissions_or_null, const int64_t* window_offsets, int U,
                     int64_t* run_offsets, int64_t* runs_or_null, int64_t capacity, int mem_space) {
    F2_TRY(f2_check_ctx(ctx));
    F2_TRY(f2_check_mem_space(ctx, mem_space, false));
    F2_CHECK(ctx, U >= 0, F2_ERR_INVALID, "negative utterance count (%d)", U);
    F2_TRY(f2_check_offsets(ctx, window_offsets, U, "window_offsets"));
    F2_CHECK(ctx, run_offsets, F2_ERR_INVALID, "run_offsets is NULL");
    const int64_t n_rows = window_offsets[U];
    F2_CHECK(ctx, labels || n_rows == 0, F2_ERR_INVALID, "null labels");
    F2_CHECK(ctx, capacity >= 0 || !runs_or_null, F2_ERR_INVALID, "negative capacity (%lld)", (long long)capacity);
    F2_TRY(f2_check_segment_rows(ctx, n_rows));
    if (n_rows == 0) {
        std::fill(run_offsets, run_offsets + U + 1, (int64_t)0);
        return F2_OK;
    }
    const size_t n = (size_t)n_rows;
    f2_seg_plan S;
    S.set(window_offsets, U);
    S.name_arrays(false, true, 0, 0);
    char *s_labels = nullptr, *s_q = nullptr, *s_runs = nullptr;
    if (mem_space != F2_MEM_DEVICE) S.name_bytes(&s_labels, n), S.name_bytes(&s_q, sizeof(int32_t) * n);
    if (runs_or_null && mem_space != F2_MEM_DEVICE) S.name_bytes(&s_runs, sizeof(int64_t) * 4 * n);
    F2_TRY(S.reserve(ctx));
    const void *d_labels, *d_q;
    F2_TRY(seg_stage(ctx, labels, s_labels, n, mem_space, &d_labels));
    F2_TRY(seg_stage(ctx, emissions_or_null, s_q, sizeof(int32_t) * n, mem_space, &d_q));
    F2_TRY(S.upload_tables(ctx));
    F2_TRY(f2_launch_runs_count(ctx, S, (const uint8_t*)d_labels, (const int32_t*)d_q));
    F2_HIP(ctx, hipMemcpyAsync(run_offsets, S.d_ro, sizeof(int64_t) * ((size_t)U + 1), hipMemcpyDeviceToHost, ctx->stream));
    F2_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (!runs_or_null) return F2_OK;
    const int64_t n_runs = run_offsets[U];
    F2_CHECK(ctx, capacity >= n_runs, F2_ERR_UNSUPPORTED, "%lld runs, room for %lld", (long long)n_runs, (long long)capacity);
    const f2_output o = seg_output(runs_or_null, s_runs, sizeof(int64_t) * 4 * (size_t)n_runs, mem_space);
    F2_TRY(f2_launch_runs_scatter(ctx, S, (const uint8_t*)d_labels, (const int32_t*)d_q, n_runs, o.as<int64_t>()));
    F2_TRY(f2_copy_back(ctx, o));
    return f2_host_wait(ctx, mem_space);
}

int f2_interval_tally(f2_ctx* ctx, const uint8_t* labels, const uint8_t* path_or_null, const int32_t* emissions_or_null,
                      const int64_t* window_offsets, int U, const int64_t* iv_offsets, const int64_t* iv_bounds, int R, int64_t origin,
                      int hop, int64_t* tally, int mem_space) {
    F2_TRY(f2_check_ctx(ctx));
    F2_TRY(f2_check_mem_space(ctx, mem_space, false));
    F2_CHECK(ctx, tally, F2_ERR_INVALID, "tally is NULL");
    F2_CHECK(ctx, U >= 0, F2_ERR_INVALID, "negative utterance count (%d)", U);
    F2_TRY(f2_check_offsets(ctx, window_offsets, U, "window_offsets"));
    const int64_t n_rows = window_offsets[U];
    F2_CHECK(ctx, labels || n_rows == 0, F2_ERR_INVALID, "null labels");
    F2_TRY(f2_check_segment_rows(ctx, n_rows));
    f2_seg_plan S;
    S.set(window_offsets, U);
    int64_t out_rows = 0;
    F2_TRY(f2_check_intervals(ctx, U, iv_offsets, iv_bounds, R, origin, hop, S.max_rows, &out_rows));
    if (out_rows == 0) return F2_OK;
    const size_t n = (size_t)n_rows, out_bytes = sizeof(int64_t) * 4 * (size_t)out_rows;
    S.name_arrays(false, false, iv_offsets[R], R);
    char *s_labels = nullptr, *s_path = nullptr, *s_q = nullptr, *s_tally = nullptr;
    if (mem_space != F2_MEM_DEVICE) {
        S.name_bytes(&s_labels, n), S.name_bytes(&s_path, n), S.name_bytes(&s_q, sizeof(int32_t) * n);
        S.name_bytes(&s_tally, out_bytes);
    }
    F2_TRY(S.reserve(ctx));
    const void *d_labels, *d_path, *d_q;
    F2_TRY(seg_stage(ctx, labels, s_labels, n, mem_space, &d_labels));
    F2_TRY(seg_stage(ctx, path_or_null, s_path, n, mem_space, &d_path));
    F2_TRY(seg_stage(ctx, emissions_or_null, s_q, sizeof(int32_t) * n, mem_space, &d_q));
    const f2_output o = seg_output(tally, s_tally, out_bytes, mem_space);
    F2_TRY(S.upload_tables(ctx));
    F2_TRY(f2_launch_interval_tally(ctx, S, (const uint8_t*)d_labels, (const uint8_t*)d_path, (const int32_t*)d_q, iv_offsets, iv_bounds, R,
                                    origin, hop, out_rows, o.as<int64_t>()));
    F2_TRY(f2_copy_back(ctx, o));
    return f2_host_wait(ctx, mem_space);
}

}  // extern "C"
