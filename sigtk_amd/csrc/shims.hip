// shims.hip -- per-read entry points with the reference's own signatures (SURVEY.md 8b "signatures to keep"):
// jnn_raw / jnn_pa / jnnv2 / find_adaptor / find_polya (src/jnn.h:104-109) and the six stat.h inlines
// (src/stat.h:17-73).  Each is a batch of one over the batched kernels (or, for float input, over the single-array
// compatibility kernels k_jnn_f32 / k_stat_f32 below); results are malloc'd by the callee and freed by the caller, as in the
// reference.  They exist so that a maintainer can diff every function against the original; throughput comes from
// the batch API.  On any failure (no device, out of memory, unsupported parameter) they return NULL / {-1,-1} / NaN
// and sgk_shim_status() tells why.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "host_util.h"
#include "median_literal.h"
#include "seqsum.h"
#include "sgk_common.h"
#include "stat_args.h"
#include "stat_device.h"

namespace sgk {

// jnn_pa (src/jnn.c:295-306) on ONE float array: jnn_core over rm_outlierf(x).  A compatibility entry (the batched
// path never holds pA in memory); every lane of the single wave walks the array, lane 0 stores.
__global__ __launch_bounds__(64) void k_jnn_f32(const float *x, int64_t n, JnnP p, int32_t *seg_x, int32_t *seg_y,
                                                uint32_t cap, uint32_t *n_segs) {
    float top = p.top, bot = p.bot;
    if (p.std_scale > 0.0f) {
        float s = 0.0f;
        for (int64_t j = 0; j < n; ++j) s = s + clampf_pa(x[j]);
        const float mn = s / (float)(int)n;
        float q = 0.0f;
        for (int64_t j = 0; j < n; ++j) {
            const float d = clampf_pa(x[j]) - mn;
            q = q + d * d;
        }
        const float sd = sqrtf(q / (float)(int)n);
        top = mn + sd * p.std_scale;
        bot = mn - sd * p.std_scale;
    }
    JnnAuto A;
    A.init(top, bot, p.corrector, p.seg_dist, p.window, p.stall_len, p.error);
    bool overflow = false;
    const bool writer = lane_id() == 0;
    auto emit = [&](int k, int sx, int sy) {
        if ((uint32_t)k < cap) { if (writer) { seg_x[k] = sx; seg_y[k] = sy; } }
        else overflow = true;
    };
    for (int64_t j = 0; j < n; ++j) A.step((int)j, A.in_mask_f(clampf_pa(x[j])), emit);
    A.finish(emit);
    if (writer) {
        n_segs[0] = (uint32_t)A.nseg;
        n_segs[1] = overflow ? 1u : 0u;
    }
}

// meanf / stdvf / medianf (src/stat.h:17-27, 36-44, 56-63) of ONE float array, for the reference-signature shims:
// the sequential float sums on every lane of the wave (lane 0 stores), the order statistic of rank n/2 by a
// three-level (11 + 11 + 10 bit) radix select on the order-preserving integer image of the floats.
// one seqsum.h chain over a float array: term(x[i]) for i = 0 .. n-1, by one wave (the other waves of the workgroup
// skip it).  Terms can have any sign: the chain is oriented by the sign of its accumulator, tiles holding a term of
// the other sign are added natively.
template <typename F>
__device__ float ss_chain_f32(const float *x, int n, F term) {
    const int lane = lane_id(), q0 = lane * SS_SPL;
    float m = 0.0f, sg = 1.0f;
    const int ntiles = (n + SS_TILE - 1) / SS_TILE;
    const int head = n < SS_HEAD ? n : SS_HEAD;
    for (int t = 0; t < ntiles; ++t) {
        float v[SS_SPL], y[SS_SPL];
#pragma unroll
        for (int e = 0; e < SS_SPL; ++e) {
            const int i = t * SS_TILE + q0 + e;
            v[e] = i < n ? term(x[i]) * sg : 0.0f;  // (* +-1: exact)
        }
        if (t == 0) {  // the head natively; its terms are zeroed for the tile chain
#pragma unroll
            for (int e = 0; e < SS_SPL; ++e) y[e] = (q0 + e < head) ? v[e] : 0.0f;
            if (head > 0) m = ss_serial(m, TermArr{y}, 0, (head - 1) / SS_SPL);
#pragma unroll
            for (int e = 0; e < SS_SPL; ++e) v[e] = (q0 + e < head) ? 0.0f : v[e];
        }
        const SsWalk w = ss_walk<true>(m, TermArr{v});
        int sk;
        if (ss_fast<true>(m, w, TermArr{v}, sk)) m = ss_finish<true>(m, TermArr{v}, w, sk);
        if (m < 0.0f) { m = -m; sg = -sg; }
    }
    return m == 0.0f ? 0.0f : m * sg;
}

// The median: a three-level radix on the floats' bit keys finds the VALUE of rank n / 2.  Where that is a zero (+0 and -0
// compare equal) or the array holds a NaN (which orders with nothing), the reference's median is the element its own
// selection leaves at n / 2: redone literally by one lane on `scratch`, a copy of the array (median_literal.h).  An array
// with a NaN or an infinity in it also gets its mean and deviation redone by that lane, for the sign of their NaN.
__global__ __launch_bounds__(256) void k_stat_f32(const float *x, int n, float *out3, float *scratch) {
    __shared__ uint32_t hist[2048];
    __shared__ uint32_t sel_prefix, sel_rank, has_nan;
    if (threadIdx.x == 0) has_nan = 0u;
    if (threadIdx.x < 64) {  // wave 0: the sequential float sums through seqsum.h
        const float s = ss_chain_f32(x, n, [](float v) { return v; });
        const float mn = s / n;
        const float q = ss_chain_f32(x, n, [&](float v) { return (v - mn) * (v - mn); });
        if (threadIdx.x == 0) { out3[0] = mn; out3[1] = sqrtf(q / n); }
    }
    auto key = [](float f) -> uint32_t {
        const uint32_t u = __float_as_uint(f);
        return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    };
    uint32_t prefix = 0u, rank = (uint32_t)(n / 2);
    const int shifts[3] = {21, 10, 0};
    const int bitsn[3] = {11, 11, 10};
    uint32_t known = 0u;  // mask of the key bits fixed so far
    for (int lvl = 0; lvl < 3; ++lvl) {
        for (int k = threadIdx.x; k < 2048; k += 256) hist[k] = 0u;
        __syncthreads();
        for (int j = threadIdx.x; j < n; j += 256) {
            const float xj = x[j];
            if (lvl == 0 && !(fabsf(xj) < __builtin_inff())) atomicOr(&has_nan, xj != xj ? 3u : 1u);   // (1: not finite, 2: a NaN)
            const uint32_t kk = key(xj);
            if ((kk & known) == prefix) atomicAdd(&hist[(kk >> shifts[lvl]) & ((1u << bitsn[lvl]) - 1u)], 1u);
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t acc = 0u, b = 0u;
            const uint32_t nb = 1u << bitsn[lvl];
            for (; b < nb; ++b) {
                if (acc + hist[b] > rank) break;
                acc += hist[b];
            }
            sel_prefix = prefix | (b << shifts[lvl]);
            sel_rank = rank - acc;
        }
        __syncthreads();
        prefix = sel_prefix;
        rank = sel_rank;
        known |= ((1u << bitsn[lvl]) - 1u) << shifts[lvl];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const uint32_t u = (prefix & 0x80000000u) ? (prefix & 0x7fffffffu) : ~prefix;
        out3[2] = __uint_as_float(u);
        sel_rank = (__uint_as_float(u) == 0.0f || (has_nan & 2u)) ? 1u : 0u;
        if (has_nan) x86_mean_std((int64_t)n, [&](int64_t i) { return x[i]; }, out3[0], out3[1]);
    }
    __syncthreads();
    if (sel_rank) {  // (workgroup-uniform)
        for (int j = threadIdx.x; j < n; j += 256) scratch[j] = x[j];
        __syncthreads();
        if (threadIdx.x == 0) out3[2] = literal_select(scratch, (int64_t)n, (int64_t)(n / 2), [](float p, float q) { return p < q; });
    }
}

static int launch_stat_f32(const float *x, int n, float *out3, float *scratch, hipStream_t st) {
    SGK_LAUNCH("k_stat_f32", k_stat_f32, 1, 256, st, x, n, out3, scratch);
    return SGK_OK;
}

static int launch_jnn_f32(const float *x, int64_t n, const JnnP &p, int32_t *seg_x, int32_t *seg_y, uint32_t cap,
                          uint32_t *n_segs, hipStream_t st) {
    SGK_LAUNCH("k_jnn_f32", k_jnn_f32, 1, 64, st, x, n, p, seg_x, seg_y, cap, n_segs);
    return SGK_OK;
}


}  // namespace sgk

using namespace sgk;

static thread_local int g_shim_rc = SGK_OK;

namespace {

JnnP to_jnnp(const sgk_jnn_param_t &q) {
    JnnP p;
    p.std_scale = q.std_scale; p.corrector = q.corrector; p.seg_dist = q.seg_dist; p.window = q.window;
    p.stall_len = q.stall_len; p.error = q.error; p.top = q.top; p.bot = q.bot;
    return p;
}

// one int16 read on the device, 64-sample aligned with room around it
int upload_one(const int16_t *raw, int64_t n, DeviceBatch &db) {
    if (n < 0 || n > 0x7fffffffLL) return SGK_ERR_ARG;
    const uint64_t offs[2] = {0, (uint64_t)n};
    const double one = 1.0, zero = 0.0;
    sgk_host_batch_t hb = {raw, offs, &one, &zero, &one, 1};
    return db.upload(&hb);
}

sgk_jnn_pair_t *collect_segments(DevBuf &d_x, DevBuf &d_y, uint32_t ns, int *n) {
    sgk_jnn_pair_t *out = (sgk_jnn_pair_t *)malloc(sizeof(sgk_jnn_pair_t) * (ns ? ns : 1));
    if (!out) { g_shim_rc = SGK_ERR_NOMEM; return nullptr; }
    std::vector<int32_t> x(ns ? ns : 1), y(ns ? ns : 1);
    if (ns) {
        if (hipMemcpy(x.data(), d_x.p, (size_t)ns * 4, hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(y.data(), d_y.p, (size_t)ns * 4, hipMemcpyDeviceToHost) != hipSuccess) {
            free(out);
            g_shim_rc = SGK_ERR_HIP;
            return nullptr;
        }
    }
    for (uint32_t k = 0; k < ns; ++k) { out[k].x = x[k]; out[k].y = y[k]; }
    *n = (int)ns;
    return out;
}

int stat_i16(const int16_t *x, int n, sgk_stat_rec_t *rec) {
    if (!x || n <= 0) return SGK_ERR_ARG;
    const uint64_t offs[2] = {0, (uint64_t)n};
    const double one = 1.0, zero = 0.0;
    sgk_host_batch_t hb = {x, offs, &one, &zero, &one, 1};
    return sgk_stat_host(&hb, rec);
}

int stat_f32(const float *x, int n, float *out3) {
    if (!x || n <= 0) return SGK_ERR_ARG;
    if (sgk_device_count() <= 0) return SGK_ERR_NODEVICE;
    DevBuf d_x, d_o, d_s;
    SGK_TRY(d_x.alloc((size_t)n * sizeof(float)));
    SGK_TRY(d_o.alloc(3 * sizeof(float)));
    SGK_TRY(d_s.alloc((size_t)n * sizeof(float)));
    SGK_HIP_TRY(hipMemcpy(d_x.p, x, (size_t)n * sizeof(float), hipMemcpyHostToDevice));
    SGK_TRY(launch_stat_f32(d_x.as<float>(), n, d_o.as<float>(), d_s.as<float>(), nullptr));
    SGK_HIP_TRY(hipDeviceSynchronize());
    SGK_HIP_TRY(hipMemcpy(out3, d_o.p, 3 * sizeof(float), hipMemcpyDeviceToHost));
    return SGK_OK;
}

}  // namespace

// a per-read call on a long read takes the long-read path of the batch API as well (a 3 000 001-sample read: 1 ms instead
// of 10): the workspace it needs, sized for this one read
static int shim_long(StatArgs &a, DevBuf &ws, LongRule auto_div) {
    if (a.b.max_read_len < LC_LONG_MIN / 2) return SGK_OK;   // (the lowest per-batch threshold, stat_args.h: LongRule)
    const size_t bytes = order_workspace_bytes(a.b.n_reads) + long_workspace_bytes(a.b.n_samples, a.b.max_read_len);
    int rc = ws.alloc(bytes);
    if (rc != SGK_OK) return rc;
    return prepare_long(a, ws.p, bytes, 0, auto_div, nullptr);
}

extern "C" {

int sgk_shim_status(void) { return g_shim_rc; }

sgk_jnn_pair_t *sgk_jnn_raw(const int16_t *raw, int64_t nsample, sgk_jnn_param_t param, int *n) {
    g_shim_rc = SGK_OK;
    if (n) *n = 0;
    if (!n || nsample <= 0 || !raw) {  // jnn_raw returns NULL with *n = 0 for an empty read (src/jnn.c:284-291)
        if (!n || (nsample > 0 && !raw)) g_shim_rc = SGK_ERR_ARG;
        return nullptr;
    }
    DeviceBatch db;
    if ((g_shim_rc = upload_one(raw, nsample, db)) != SGK_OK) return nullptr;
    const uint64_t cap = sgk_jnn_slots_for((uint32_t)nsample);
    const uint64_t slots[2] = {0, cap};
    DevBuf d_slots, d_x, d_y, d_n, d_ws;
    if ((g_shim_rc = d_slots.alloc(16)) != SGK_OK || (g_shim_rc = d_x.alloc(cap * 4)) != SGK_OK ||
        (g_shim_rc = d_y.alloc(cap * 4)) != SGK_OK || (g_shim_rc = d_n.alloc(4)) != SGK_OK ||
        (g_shim_rc = d_ws.alloc(64)) != SGK_OK)
        return nullptr;
    if (hipMemcpy(d_slots.p, slots, 16, hipMemcpyHostToDevice) != hipSuccess) { g_shim_rc = SGK_ERR_HIP; return nullptr; }
    StatArgs a;
    memset(&a, 0, sizeof a);
    a.b = db.view;
    a.seg_slots = d_slots.as<uint64_t>();
    a.seg_x = d_x.as<int32_t>();
    a.seg_y = d_y.as<int32_t>();
    a.n_segs = d_n.as<uint32_t>();
    a.err_count = d_ws.as<uint32_t>();
    DevBuf d_long;
    if ((g_shim_rc = shim_long(a, d_long, LC_AUTO_DIV_JNN)) != SGK_OK) return nullptr;
    if ((g_shim_rc = launch_jnn(a, to_jnnp(param), nullptr)) != SGK_OK) return nullptr;
    uint32_t ns = 0, nerr = 0;
    if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(&ns, d_n.p, 4, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(&nerr, d_ws.p, 4, hipMemcpyDeviceToHost) != hipSuccess) {
        g_shim_rc = SGK_ERR_HIP;
        return nullptr;
    }
    if (nerr) { g_shim_rc = SGK_ERR_CAPACITY; return nullptr; }
    return collect_segments(d_x, d_y, ns, n);
}

sgk_jnn_pair_t *sgk_jnn_pa(const float *raw, int64_t nsample, sgk_jnn_param_t param, int *n) {
    g_shim_rc = SGK_OK;
    if (n) *n = 0;
    if (!n || nsample <= 0 || !raw) {
        if (!n || (nsample > 0 && !raw)) g_shim_rc = SGK_ERR_ARG;
        return nullptr;
    }
    if (nsample > 0x7fffffffLL) { g_shim_rc = SGK_ERR_ARG; return nullptr; }
    if (sgk_device_count() <= 0) { g_shim_rc = SGK_ERR_NODEVICE; return nullptr; }
    const uint32_t cap = (uint32_t)sgk_jnn_slots_for((uint32_t)nsample);
    DevBuf d_in, d_x, d_y, d_n;
    if ((g_shim_rc = d_in.alloc((size_t)nsample * 4)) != SGK_OK || (g_shim_rc = d_x.alloc((size_t)cap * 4)) != SGK_OK ||
        (g_shim_rc = d_y.alloc((size_t)cap * 4)) != SGK_OK || (g_shim_rc = d_n.alloc(8)) != SGK_OK)
        return nullptr;
    if (hipMemcpy(d_in.p, raw, (size_t)nsample * 4, hipMemcpyHostToDevice) != hipSuccess) { g_shim_rc = SGK_ERR_HIP; return nullptr; }
    if ((g_shim_rc = launch_jnn_f32(d_in.as<float>(), nsample, to_jnnp(param), d_x.as<int32_t>(), d_y.as<int32_t>(), cap,
                                    d_n.as<uint32_t>(), nullptr)) != SGK_OK)
        return nullptr;
    uint32_t res[2] = {0, 0};
    if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(res, d_n.p, 8, hipMemcpyDeviceToHost) != hipSuccess) {
        g_shim_rc = SGK_ERR_HIP;
        return nullptr;
    }
    if (res[1]) { g_shim_rc = SGK_ERR_CAPACITY; return nullptr; }
    return collect_segments(d_x, d_y, res[0], n);
}

sgk_jnn_pair_t sgk_jnnv2(const int16_t *sig, int64_t nsample, sgk_jnnv2_param_t param) {
    sgk_jnn_pair_t p = {-1, -1};
    g_shim_rc = SGK_OK;
    if (param.window != 2000) { g_shim_rc = SGK_ERR_ARG; return p; }  // both presets of the reference (src/jnn.h:84-98)
    if (nsample <= param.window) return p;  // "Not enough data to trim" (src/jnn.c:172-176)
    if (!sig) { g_shim_rc = SGK_ERR_ARG; return p; }
    DeviceBatch db;
    if ((g_shim_rc = upload_one(sig, nsample, db)) != SGK_OK) return p;
    DevBuf d_out;
    if ((g_shim_rc = d_out.alloc(sizeof(sgk_prefix_rec_t))) != SGK_OK) return p;
    StatArgs a;
    memset(&a, 0, sizeof a);
    a.b = db.view;
    a.prefix = d_out.as<sgk_prefix_rec_t>();
    AdaptP ap;
    ap.std_scale = param.std_scale; ap.seg_dist = param.seg_dist; ap.lo_thresh = param.lo_thresh; ap.hi_thresh = param.hi_thresh;
    DevBuf d_long;
    if ((g_shim_rc = shim_long(a, d_long, LC_AUTO_DIV_PREFIX)) != SGK_OK) return p;
    if ((g_shim_rc = launch_adaptor(a, ap, nullptr)) != SGK_OK) return p;
    sgk_prefix_rec_t rec;
    if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(&rec, d_out.p, sizeof rec, hipMemcpyDeviceToHost) != hipSuccess) {
        g_shim_rc = SGK_ERR_HIP;
        return p;
    }
    p.x = rec.adapt_x;
    p.y = rec.adapt_y;
    return p;
}

// any window of the domain (sgk_prefix_params_check's adaptor part), always on k_adaptor_param
sgk_jnn_pair_t sgk_jnnv2_param(const int16_t *sig, int64_t nsample, sgk_jnnv2_param_t param) {
    sgk_jnn_pair_t p = {-1, -1};
    g_shim_rc = SGK_OK;
    sgk_prefix_params_t chk;
    sgk_prefix_params_preset(0, SGK_PORE_R9, &chk);
    chk.adaptor = param;
    if (sgk_prefix_params_check(&chk) != SGK_OK) { g_shim_rc = SGK_ERR_ARG; return p; }
    if (nsample <= param.window) return p;  // "Not enough data to trim" (src/jnn.c:172-176)
    if (!sig) { g_shim_rc = SGK_ERR_ARG; return p; }
    DeviceBatch db;
    if ((g_shim_rc = upload_one(sig, nsample, db)) != SGK_OK) return p;
    DevBuf d_out;
    if ((g_shim_rc = d_out.alloc(sizeof(sgk_prefix_rec_t))) != SGK_OK) return p;
    StatArgs a;
    memset(&a, 0, sizeof a);
    a.b = db.view;
    a.prefix = d_out.as<sgk_prefix_rec_t>();
    AdaptP ap;
    ap.std_scale = param.std_scale; ap.seg_dist = param.seg_dist; ap.lo_thresh = param.lo_thresh; ap.hi_thresh = param.hi_thresh;
    if ((g_shim_rc = launch_k_adaptor_param(nullptr, a, ap, param.window)) != SGK_OK) return p;
    sgk_prefix_rec_t rec;
    if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(&rec, d_out.p, sizeof rec, hipMemcpyDeviceToHost) != hipSuccess) {
        g_shim_rc = SGK_ERR_HIP;
        return p;
    }
    p.x = rec.adapt_x;
    p.y = rec.adapt_y;
    return p;
}

sgk_jnn_pair_t sgk_find_polya_param(const float *raw, int64_t nsample, float top, float bot, sgk_jnn_param_t param) {
    sgk_jnn_pair_t p = {-1, -1};
    sgk_prefix_params_t chk;
    sgk_prefix_params_preset(1, SGK_PORE_R9, &chk);
    chk.polya = param;
    if (sgk_prefix_params_check(&chk) != SGK_OK) { g_shim_rc = SGK_ERR_ARG; return p; }
    param.std_scale = -1.0f;  // the fixed thresholds
    param.top = top;
    param.bot = bot;
    int ns = 0;
    sgk_jnn_pair_t *segs = sgk_jnn_pa(raw, nsample, param, &ns);
    if (segs) {
        if (ns > 0) p = segs[0];
        free(segs);
    }
    return p;
}

sgk_jnn_pair_t sgk_find_adaptor(const int16_t *raw, int64_t nsample, int8_t pore) {
    const AdaptP ap = adaptor_preset(pore);
    sgk_jnnv2_param_t q;
    q.std_scale = ap.std_scale; q.seg_dist = ap.seg_dist; q.window = 2000; q.stall_len = 0.0f;
    q.hi_thresh = ap.hi_thresh; q.lo_thresh = ap.lo_thresh;
    return sgk_jnnv2(raw, nsample, q);
}

sgk_jnn_pair_t sgk_find_polya(const float *raw, int64_t nsample, float top, float bot, int8_t pore) {
    (void)pore;  // JNNV1_R9_POLYA and JNNV1_RNA004_POLYA hold the same values (src/jnn.h:52-72)
    sgk_jnn_pair_t p = {-1, -1};
    const JnnP pp = jnn_polya_preset();
    sgk_jnn_param_t q;
    q.std_scale = pp.std_scale; q.corrector = pp.corrector; q.seg_dist = pp.seg_dist; q.window = pp.window;
    q.stall_len = pp.stall_len; q.error = pp.error; q.top = top; q.bot = bot;
    int ns = 0;
    sgk_jnn_pair_t *segs = sgk_jnn_pa(raw, nsample, q, &ns);
    if (segs) {
        if (ns > 0) p = segs[0];
        free(segs);
    }
    return p;
}

float sgk_meani16(const int16_t *x, int n) {
    sgk_stat_rec_t r;
    return (g_shim_rc = stat_i16(x, n, &r)) == SGK_OK ? r.raw_mean : NAN;
}
float sgk_stdvi16(const int16_t *x, int n) {
    sgk_stat_rec_t r;
    return (g_shim_rc = stat_i16(x, n, &r)) == SGK_OK ? r.raw_std : NAN;
}
int16_t sgk_mediani16(const int16_t *x, int n) {
    sgk_stat_rec_t r;
    return (g_shim_rc = stat_i16(x, n, &r)) == SGK_OK ? (int16_t)r.raw_median : (int16_t)0;
}
float sgk_meanf(const float *x, int n) {
    float o[3];
    return (g_shim_rc = stat_f32(x, n, o)) == SGK_OK ? o[0] : NAN;
}
float sgk_stdvf(const float *x, int n) {
    float o[3];
    return (g_shim_rc = stat_f32(x, n, o)) == SGK_OK ? o[1] : NAN;
}
float sgk_medianf(const float *x, int n) {
    float o[3];
    return (g_shim_rc = stat_f32(x, n, o)) == SGK_OK ? o[2] : NAN;
}

}  // extern "C"
