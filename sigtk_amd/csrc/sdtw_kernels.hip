// sdtw_kernels.hip -- sgk_sdtw_f32: subsequence dynamic time warping of every query of a float batch against every
// target of another, bit for bit the definition in include/sigtk_gpu.h:
//   c(i,j) = fabsf(q[i] - t[j]);  D(i,j) = c(i,j) + best of D(i-1,j-1), D(i-1,j), D(i,j-1) -- the diagonal wins a tie
//   over "up", both over "left" --;  S(i,j) the column in which the path of cell (i,j) left row 0;
//   score = min_j D(m-1,j), end the smallest such j, start = S(m-1,end).
//   * k_sdtw_flags, one WAVE per read of either batch (float_reads.h): does it hold a NaN or an infinity, is it longer
//     than its batch's max_*_len.  The recurrence below never sees such a read.
//   * k_sdtw<R, START, MULTI>, one WAVE per (query, target) pair, the pairs of the longest queries first, run as a
//     systolic array over the query's rows: lane l owns rows l R .. l R + R - 1 of the band (R = 1, 2, 4, 8, 16 by the
//     query's length, its values in registers) and does, at step s, column j = s - l of them, top to bottom.  t[j] and
//     the cell above its top row (D, S) come from lane l - 1 by a one-lane shift (wave_shr1_i); what came at the step
//     before is the diagonal.  Lane 0 takes t[j] from a 64-value chunk the wave loaded (the next chunk is in flight
//     under the steps of this one) and, as the row above the band, the virtual row D(-1,j) = 0, S(-1,j) = j + 1 for
//     j >= -1: in row 0 the diagonal then wins every time, D(0,j) = c(0,j) + 0 and S(0,j) = j.
//     Everything outside the matrix is +inf: a lane that has not reached column 0 yet, or is past column n - 1, works
//     on t = +inf, so its cells are +inf with S = 0 -- the left and diagonal neighbours column 0 asks for, and nothing
//     a strict < ever picks.  No cell needs a test of its own for an edge.
//     The lane that owns row m - 1 keeps the running best of that row with a strict <: the smallest j, no reduction.
//   * MULTI (queries of more than 1 024 values): the band of 64 x 16 rows runs once per pass; the band's last row (D, S
//     per column) goes to the wave's slot of the workspace and comes back as lane 0's row above in the next pass, in
//     place: column j is read (in a chunk, at step <= j) before it is rewritten (at step j + 63).  The kernel is a
//     fixed number of waves (the slots), each taking every n_slots-th pair.
//   * START = false (SGK_SDTW_NO_START) drops S; the best of three is then a plain minimum (all values are finite or
//     +inf and not negative: the same number whichever wins a tie).
// No LDS, no workgroup barrier; a pair is never split over waves.
#include "float_reads.h"
#include "stat_args.h"

namespace sgk {

constexpr int SDTW_MAX_R = 16;
constexpr uint32_t SDTW_ONE_PASS = 64u * SDTW_MAX_R;  // the longest query that runs in one band
constexpr uint32_t SDTW_SLOTS = 2048;                 // band-row slots = waves of the multi-pass kernel (8 per CU)
constexpr size_t SDTW_BAND_ROOM = (size_t)1 << 30;    // ... fewer where they would pass this many bytes, never less than one

struct SdtwArgs {
    FloatBatch q, t;               // q.order: the queries longest first, or null
    const uint32_t *qflag, *tflag; // SGK_SDTW_NONFINITE / SGK_SDTW_TOO_LONG of every read (k_sdtw_flags)
    sgk_sdtw_rec_t *out;
    float *rows;                   // n_slots slots of 2 row_stride words: D of the band's last row, then S
    uint64_t row_stride;
    uint32_t n_slots;
};

__global__ __launch_bounds__(256) void k_sdtw_flags(FloatBatch q, FloatBatch t, uint32_t max_q, uint32_t max_t, uint32_t *qflag,
                                                    uint32_t *tflag) {
    const uint64_t w = (uint64_t)blockIdx.x * 4 + (uint32_t)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (w >= (uint64_t)q.n_reads + t.n_reads) return;
    const bool isq = w < q.n_reads;
    const FloatBatch b = isq ? q : t;
    const uint32_t r = (uint32_t)(isq ? w : w - q.n_reads);
    uint32_t f = 0u;
    if (b.lengths[r] > (isq ? max_q : max_t)) f = SGK_SDTW_TOO_LONG;  // (not swept: its length is not to be trusted)
    else {
        FloatRead fr;
        fr.init(b, r);
        uint32_t h = 0u;
        fr_sweep(fr, [&](int, const float (&x)[SS_SPL], uint32_t vm) {
#pragma unroll
            for (int e = 0; e < SS_SPL; ++e) h |= (uint32_t)(((vm >> e) & 1u) && !(fabsf(x[e]) < __builtin_inff()));
        });
        if (__ballot(h != 0u) != 0ull) f = SGK_SDTW_NONFINITE;
    }
    if (lane_id() == 0) (isq ? qflag : tflag)[r] = f;
}

__device__ __forceinline__ float sdtw_shr1_f(float v, float first) {
    return __int_as_float(wave_shr1_i(__float_as_int(v), __float_as_int(first)));
}
__device__ __forceinline__ float sdtw_readlane_f(float v, uint32_t lane) {  // lane is wave-uniform
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), (int)lane));
}

template <int R>
struct SdtwState {  // what a lane keeps from one step to the next
    float d[R];     // D of its rows in the column it did last
    uint32_t s[R];  // ... and S
    float t, up;    // that column's t and the cell above the lane's top row (D, S)
    uint32_t ups;
};

template <int R, bool START, bool MULTI>
__global__ __launch_bounds__(256) void k_sdtw(SdtwArgs a) {
    static_assert(!MULTI || R == SDTW_MAX_R, "only the widest band runs in passes");
    const uint32_t wv = blockIdx.x * 4 + (uint32_t)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint64_t n_waves = MULTI ? (uint64_t)a.n_slots : (uint64_t)gridDim.x * 4;
    if (MULTI && wv >= a.n_slots) return;
    const uint64_t n_pairs = (uint64_t)a.q.n_reads * a.t.n_reads;
    const uint32_t lane = (uint32_t)lane_id();
    const float inf = __builtin_inff();
    float *rowD = nullptr;
    uint32_t *rowS = nullptr;
    if constexpr (MULTI) {
        rowD = a.rows + (uint64_t)wv * 2u * a.row_stride;
        rowS = reinterpret_cast<uint32_t *>(rowD + a.row_stride);
    }
#pragma unroll 1
    for (uint64_t idx = wv; idx < n_pairs; idx += n_waves) {
        const uint32_t qs = (uint32_t)(idx / a.t.n_reads), ti = (uint32_t)(idx - (uint64_t)qs * a.t.n_reads);
        const uint32_t qi = a.q.order ? a.q.order[qs] : qs;
        const uint32_t m = a.q.lengths[qi], n = a.t.lengths[ti];
        const uint32_t f = a.qflag[qi] | a.tflag[ti];
        sgk_sdtw_rec_t *rec = a.out + ((uint64_t)qi * a.t.n_reads + ti);
        if (m == 0u || n == 0u || f != 0u) {  // (wave-uniform) no alignment: the first launch writes the record
            if (R == 1 && !MULTI && lane == 0u)
                *rec = sgk_sdtw_rec_t{__builtin_nanf(""), -1, -1, f | ((m == 0u || n == 0u) ? SGK_SDTW_EMPTY : 0u)};
            continue;
        }
        if (MULTI ? m <= SDTW_ONE_PASS : (m > 64u * R || (R > 1 && m <= 32u * R))) continue;  // another launch's pair
        const float *qp = a.q.x + a.q.offsets[qi], *tp = a.t.x + a.t.offsets[ti];
        const uint32_t n_bands = MULTI ? (m + 64u * R - 1u) / (64u * R) : 1u;
        float best = inf;  // of row m - 1, in the lane that owns it: (best, bestj, bests) start as column 0 of an all-inf row
        uint32_t bests = 0u, bestj = 0u, last_lane = 0u;
#pragma unroll 1
        for (uint32_t band = 0; band < n_bands; ++band) {
            const uint32_t row0 = band * 64u * R, rows_in = m - row0 < 64u * R ? m - row0 : 64u * R;
            last_lane = (rows_in - 1u) / R;
            const uint32_t klast = rows_in - 1u - last_lane * R;
            const bool first = band == 0u, last = band + 1u == n_bands;
            if (last) bestj = last_lane;  // (column 0 is this lane's step last_lane)
            float qv[R];
            SdtwState<R> A, B;  // the lane's cells after the last step; two copies, written in turn: no register is moved
#pragma unroll
            for (int k = 0; k < R; ++k) {
                const uint32_t row = row0 + lane * R + k;
                qv[k] = row < m ? qp[row] : 0.0f;  // (rows past the query: finite cells nobody reads)
                A.d[k] = inf;
                A.s[k] = 0u;
            }
            A.t = inf;
            A.up = (first && lane == 0u) ? 0.0f : inf;  // D(-1,-1) = 0 of the virtual row
            A.ups = 0u;
            const uint32_t n_steps = n + last_lane;
            float tn = lane < n ? tp[lane] : inf, wdn = inf;  // the next chunk of t and of the row above the band
            uint32_t wsn = 0u;
            if (MULTI && !first && lane < n) {
                wdn = rowD[lane];
                if constexpr (START) wsn = rowS[lane];
            }
            asm volatile("" ::"v"(tn), "v"(wdn), "v"(wsn));  // the first chunk has arrived: no wait on it inside the step loop
#pragma unroll 1
            for (uint32_t s0 = 0; s0 < n_steps; s0 += 64u) {
                const float tc = tn, wdc = wdn;
                const uint32_t wsc = wsn;
                const uint32_t col = s0 + 64u + lane;
                tn = col < n ? tp[col] : inf;
                if (MULTI && !first) {
                    wdn = col < n ? rowD[col] : inf;
                    if constexpr (START) wsn = col < n ? rowS[col] : 0u;
                }
                const uint32_t cnt = n_steps - s0 < 64u ? n_steps - s0 : 64u;
                // step s0 + i: column s0 + i - lane of the lane's rows, from the cells `o` into the cells `w`
                const auto step = [&](const SdtwState<R> &o, SdtwState<R> &w, uint32_t i) __attribute__((always_inline)) {
                    const uint32_t s = s0 + i;
                    float u0 = 0.0f;
                    uint32_t us0 = s + 1u;
                    if (MULTI && !first) {
                        u0 = sdtw_readlane_f(wdc, i);
                        if constexpr (START) us0 = (uint32_t)__builtin_amdgcn_readlane((int)wsc, (int)i);
                    }
                    const float tj = sdtw_shr1_f(o.t, sdtw_readlane_f(tc, i));
                    float up = sdtw_shr1_f(o.d[R - 1], u0), dg = o.up;  // last step's cell above is this step's diagonal
                    uint32_t ups = 0u, dgs = o.ups;
                    if constexpr (START) ups = (uint32_t)wave_shr1_i((int)o.s[R - 1], (int)us0);
                    w.t = tj;
                    w.up = up;
                    w.ups = ups;
#pragma unroll
                    for (int k = 0; k < R; ++k) {
                        const float c = fabsf(qv[k] - tj), left = o.d[k];
                        float b;
                        if constexpr (START) {
                            const uint32_t lefts = o.s[k];
                            uint32_t bs = dgs;
                            b = dg;
                            if (up < b) { b = up; bs = ups; }
                            if (left < b) { b = left; bs = lefts; }
                            dgs = lefts;
                            ups = bs;
                            w.s[k] = bs;
                        } else {
                            b = __builtin_fminf(__builtin_fminf(dg, up), left);
                            w.s[k] = 0u;
                        }
                        const float nd = c + b;
                        dg = left;
                        up = nd;
                        w.d[k] = nd;
                    }
                    if (last) {  // (wave-uniform) row m - 1 is row klast of lane last_lane
                        // One scalar jump per step, each case a register copy of its own.  (The empty asm keeps the cases
                        // apart: merged, they are an indexed read of d and s, and both arrays would live in scratch.)
                        float dl = w.d[0];
                        uint32_t sl = w.s[0];
                        switch (klast) {
#define SDTW_ROW(K) case K: if constexpr (K < R) { dl = w.d[K < R ? K : 0]; sl = w.s[K < R ? K : 0]; asm volatile("" : "+v"(dl), "+v"(sl)); } break;
                            SDTW_ROW(1) SDTW_ROW(2) SDTW_ROW(3) SDTW_ROW(4) SDTW_ROW(5) SDTW_ROW(6) SDTW_ROW(7) SDTW_ROW(8)
                            SDTW_ROW(9) SDTW_ROW(10) SDTW_ROW(11) SDTW_ROW(12) SDTW_ROW(13) SDTW_ROW(14) SDTW_ROW(15)
#undef SDTW_ROW
                            default: break;
                        }
                        if (dl < best) { best = dl; bestj = s; bests = sl; }
                    } else if constexpr (MULTI) {  // a full band: lane 63 has column s - 63 < n of its last row
                        if (lane == 63u && s >= 63u) {
                            rowD[s - 63u] = w.d[R - 1];
                            if constexpr (START) rowS[s - 63u] = w.s[R - 1];
                        }
                    }
                };
                uint32_t i = 0;
#pragma unroll 1
                for (; i + 1u < cnt; i += 2u) {
                    step(A, B, i);
                    step(B, A, i + 1u);
                }
                if (i < cnt) {  // (an odd count: the last chunk only)
                    step(A, B, i);
                    A = B;
                }
            }
            // the next pass reads, in other lanes, what lane 63 stored
            if constexpr (MULTI) __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        }
        const float score = sdtw_readlane_f(best, last_lane);
        const int32_t end = (int32_t)((uint32_t)__builtin_amdgcn_readlane((int)bestj, (int)last_lane) - last_lane);
        const int32_t start = START ? (int32_t)__builtin_amdgcn_readlane((int)bests, (int)last_lane) : -1;
        if (lane == 0u) *rec = sgk_sdtw_rec_t{score, end, start, 0u};
    }
}

// ---- the workspace: [0, 64) unused, the dispatch order of the queries (order_workspace_bytes), a flag word per query and
// per target, then -- only where a query can be longer than one band -- the band-row slots
struct SdtwLayout {
    size_t qflag, tflag, rows, total;
    uint64_t row_stride;
    uint32_t n_slots;
};
static SdtwLayout sdtw_layout(uint32_t nq, uint32_t max_q, uint32_t nt, uint32_t max_t) {
    SdtwLayout l{};
    size_t off = order_workspace_bytes(nq);
    l.qflag = off;
    off += round_up((uint64_t)nq * 4u, 64);
    l.tflag = off;
    off += round_up((uint64_t)nt * 4u, 64);
    l.rows = off;
    if (max_q > SDTW_ONE_PASS) {
        l.row_stride = round_up(max_t, 64);
        const size_t row_bytes = (size_t)l.row_stride * 8u;
        const uint64_t pairs = (uint64_t)nq * nt;
        const size_t want = (size_t)(pairs < SDTW_SLOTS ? pairs : SDTW_SLOTS) * row_bytes;
        const size_t room = row_bytes > SDTW_BAND_ROOM ? row_bytes : SDTW_BAND_ROOM;  // (both monotone in every argument)
        const size_t bytes = want < room ? want : room;
        l.n_slots = row_bytes ? (uint32_t)(bytes / row_bytes) : 0u;
        off += bytes;
    }
    l.total = off;
    return l;
}

template <bool START>
static int launch_sdtw(const SdtwArgs &a, uint32_t max_q, hipStream_t st) {
    const uint64_t n_pairs = (uint64_t)a.q.n_reads * a.t.n_reads;
    const uint64_t blocks = (n_pairs + 3u) / 4u;
    const uint32_t grid = (uint32_t)(blocks < (1u << 22) ? blocks : (1u << 22));  // (the waves stride over the pairs)
    SGK_LAUNCH(START ? "k_sdtw_r1" : "k_sdtw_r1_nostart", (k_sdtw<1, START, false>), grid, 256, st, a);
    if (max_q > 64u) SGK_LAUNCH(START ? "k_sdtw_r2" : "k_sdtw_r2_nostart", (k_sdtw<2, START, false>), grid, 256, st, a);
    if (max_q > 128u) SGK_LAUNCH(START ? "k_sdtw_r4" : "k_sdtw_r4_nostart", (k_sdtw<4, START, false>), grid, 256, st, a);
    if (max_q > 256u) SGK_LAUNCH(START ? "k_sdtw_r8" : "k_sdtw_r8_nostart", (k_sdtw<8, START, false>), grid, 256, st, a);
    if (max_q > 512u) SGK_LAUNCH(START ? "k_sdtw_r16" : "k_sdtw_r16_nostart", (k_sdtw<16, START, false>), grid, 256, st, a);
    if (max_q > SDTW_ONE_PASS && a.n_slots)
        SGK_LAUNCH(START ? "k_sdtw_passes" : "k_sdtw_passes_nostart", (k_sdtw<16, START, true>), (a.n_slots + 3u) / 4u, 256, st, a);
    return SGK_OK;
}

}  // namespace sgk

using namespace sgk;

extern "C" {

size_t sgk_sdtw_f32_workspace_bytes(uint32_t n_queries, uint32_t max_query_len, uint32_t n_targets, uint32_t max_target_len) {
    return sdtw_layout(n_queries, max_query_len, n_targets, max_target_len).total;
}

int sgk_sdtw_f32(const float *q, const uint64_t *q_offsets, const uint32_t *q_lengths, uint32_t n_queries, uint32_t max_query_len,
                 uint64_t n_q_values, const float *t, const uint64_t *t_offsets, const uint32_t *t_lengths, uint32_t n_targets,
                 uint32_t max_target_len, uint64_t n_t_values, uint32_t options, sgk_sdtw_rec_t *out, void *ws, size_t ws_bytes,
                 void *stream) {
    (void)n_q_values;
    (void)n_t_values;
    if (options & ~SGK_SDTW_NO_START) return SGK_ERR_ARG;
    SGK_TRY(float_batch_check(q, q_offsets, q_lengths, n_queries, max_query_len));
    SGK_TRY(float_batch_check(t, t_offsets, t_lengths, n_targets, max_target_len));
    if (n_queries == 0 || n_targets == 0) return SGK_OK;
    if (!out || !ws || (reinterpret_cast<uintptr_t>(ws) & 15u)) return SGK_ERR_ARG;
    const SdtwLayout l = sdtw_layout(n_queries, max_query_len, n_targets, max_target_len);
    if (ws_bytes < l.total) return SGK_ERR_WORKSPACE;
    if (sgk_device_count() <= 0) return SGK_ERR_NODEVICE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    char *w = static_cast<char *>(ws);
    SdtwArgs a{};
    a.q = FloatBatch{q, q_offsets, q_lengths, n_queries, nullptr};
    a.t = FloatBatch{t, t_offsets, t_lengths, n_targets, nullptr};
    uint32_t *qflag = reinterpret_cast<uint32_t *>(w + l.qflag), *tflag = reinterpret_cast<uint32_t *>(w + l.tflag);
    a.qflag = qflag;
    a.tflag = tflag;
    a.out = out;
    a.rows = reinterpret_cast<float *>(w + l.rows);
    a.row_stride = l.row_stride;
    a.n_slots = l.n_slots;
    SGK_LAUNCH("k_sdtw_flags", k_sdtw_flags, (uint32_t)(((uint64_t)n_queries + n_targets + 3u) / 4u), 256, st, a.q, a.t, max_query_len,
               max_target_len, qflag, tflag);
    SGK_TRY(float_batch_order(a.q, ws, st));
    return (options & SGK_SDTW_NO_START) ? launch_sdtw<false>(a, max_query_len, st) : launch_sdtw<true>(a, max_query_len, st);
}

}  // extern "C"
