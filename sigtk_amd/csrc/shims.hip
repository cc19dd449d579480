// shims.hip -- per-read entry points with the reference's own signatures (SURVEY.md 8b "signatures to keep"):
// jnn_raw / jnn_pa / jnnv2 / find_adaptor / find_polya (src/jnn.h:104-109) and the six stat.h inlines
// (src/stat.h:17-73).  Each is a batch of one over the batched kernels -- meanf / stdvf / medianf included, on the
// kernels of sgk_stat_f32 -- but for jnn_pa, which keeps the single-array kernel k_jnn_f32 below: sets on the literal
// loop of sgk_jnn_f32 take 11 % longer per call on a batch of one than on it (profiles/float_shims.md).  Results are
// malloc'd by the callee and freed by the caller, as in the reference.  They exist so that a maintainer can diff every
// function against the original; throughput comes from the batch API.  On any failure (no device, out of memory,
// unsupported parameter) they return NULL / {-1,-1} / NaN and sgk_shim_status() tells why.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "float_reads.h"
#include "host_util.h"
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

static int launch_jnn_f32(const float *x, int64_t n, const JnnP &p, int32_t *seg_x, int32_t *seg_y, uint32_t cap,
                          uint32_t *n_segs, hipStream_t st) {
    SGK_LAUNCH("k_jnn_f32", k_jnn_f32, 1, 64, st, x, n, p, seg_x, seg_y, cap, n_segs);
    return SGK_OK;
}

}  // namespace sgk

using namespace sgk;

static thread_local int g_shim_rc = SGK_OK;

namespace {

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

// meanf / stdvf / medianf of one float array: a batch of one read on the kernels of sgk_stat_f32.  The read is the
// array at element 0 of an allocation of its own; a second one holds this head -- what the launcher reads of the batch
// (offset, length) and the record it writes -- with the workspace behind it.
struct OneRead {
    uint64_t offset;   // 0
    uint32_t length, pad0;
    sgk_statf_rec_t rec;
    uint32_t pad[8];
};
static_assert(sizeof(OneRead) == 64, "the workspace behind it is 16-byte aligned");

int stat_f32(const float *x, int n, float *out3) {
    if (!x || n <= 0) return SGK_ERR_ARG;
    if (sgk_device_count() <= 0) return SGK_ERR_NODEVICE;
    OneRead h = {};
    h.length = (uint32_t)n;
    DevBuf d_x, d_w;
    SGK_TRY(d_x.alloc((size_t)n * sizeof(float)));
    SGK_TRY(d_w.alloc(sizeof h + sgk_stat_f32_workspace_bytes(1, h.length, h.length)));
    SGK_HIP_TRY(hipMemcpy(d_x.p, x, (size_t)n * sizeof(float), hipMemcpyHostToDevice));
    SGK_HIP_TRY(hipMemcpy(d_w.p, &h, sizeof h, hipMemcpyHostToDevice));
    OneRead *d = d_w.as<OneRead>();
    SGK_TRY(launch_statf(FloatBatch{d_x.as<float>(), &d->offset, &d->length, 1u, nullptr}, h.length, &d->rec, d + 1, nullptr));
    SGK_HIP_TRY(hipDeviceSynchronize());
    SGK_HIP_TRY(hipMemcpy(&h, d, sizeof h, hipMemcpyDeviceToHost));
    out3[0] = h.rec.mean; out3[1] = h.rec.std; out3[2] = h.rec.median;
    return SGK_OK;
}

// a per-read call on a long read takes the long-read path of the batch API as well (a 3 000 001-sample read: 1 ms instead
// of 10): the workspace it needs, sized for this one read
int shim_long(StatArgs &a, DevBuf &ws, LongRule auto_div) {
    if (a.b.max_read_len < LC_LONG_MIN / 2) return SGK_OK;   // (the lowest per-batch threshold, stat_args.h: LongRule)
    const size_t bytes = order_workspace_bytes(a.b.n_reads) + long_workspace_bytes(a.b.n_samples, a.b.max_read_len);
    int rc = ws.alloc(bytes);
    if (rc != SGK_OK) return rc;
    return prepare_long(a, ws.p, bytes, 0, auto_div, nullptr);
}

// jnnv2 of one read, what sgk_jnnv2 and sgk_jnnv2_param share behind their domain checks: upload, the record, the
// launch -- launch(a, ap, ws): the caller's finder, ws for what it needs on the device until the call is over -- and the
// read-back
template <typename Launch>
sgk_jnn_pair_t jnnv2_one(const int16_t *sig, int64_t nsample, const sgk_jnnv2_param_t &param, Launch launch) {
    sgk_jnn_pair_t p = {-1, -1};
    if (nsample <= param.window) return p;  // "Not enough data to trim" (src/jnn.c:172-176)
    if (!sig) { g_shim_rc = SGK_ERR_ARG; return p; }
    DeviceBatch db;
    if ((g_shim_rc = upload_one(sig, nsample, db)) != SGK_OK) return p;
    DevBuf d_out, d_ws;
    if ((g_shim_rc = d_out.alloc(sizeof(sgk_prefix_rec_t))) != SGK_OK) return p;
    StatArgs a;
    memset(&a, 0, sizeof a);
    a.b = db.view;
    a.prefix = d_out.as<sgk_prefix_rec_t>();
    if ((g_shim_rc = launch(a, to_adaptp(param), d_ws)) != SGK_OK) return p;
    sgk_prefix_rec_t rec;
    if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(&rec, d_out.p, sizeof rec, hipMemcpyDeviceToHost) != hipSuccess) {
        g_shim_rc = SGK_ERR_HIP;
        return p;
    }
    p.x = rec.adapt_x;
    p.y = rec.adapt_y;
    return p;
}

// find_polya (src/jnn.c:352-374): the first segment of jnn_pa with `core` on the fixed thresholds top, bot
sgk_jnn_pair_t polya_one(const float *raw, int64_t nsample, float top, float bot, sgk_jnn_param_t core) {
    sgk_jnn_pair_t p = {-1, -1};
    core.std_scale = -1.0f;  // the fixed thresholds
    core.top = top;
    core.bot = bot;
    int ns = 0;
    sgk_jnn_pair_t *segs = sgk_jnn_pa(raw, nsample, core, &ns);
    if (segs) {
        if (ns > 0) p = segs[0];
        free(segs);
    }
    return p;
}

}  // namespace

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
    g_shim_rc = SGK_OK;
    if (param.window != 2000) { g_shim_rc = SGK_ERR_ARG; return {-1, -1}; }  // both presets of the reference (src/jnn.h:84-98)
    return jnnv2_one(sig, nsample, param, [](StatArgs &a, const AdaptP &ap, DevBuf &ws) {
        SGK_TRY(shim_long(a, ws, LC_AUTO_DIV_PREFIX));
        return launch_adaptor(a, ap, nullptr);
    });
}

// any window of the domain (sgk_prefix_params_check's adaptor part), always on k_adaptor_param
sgk_jnn_pair_t sgk_jnnv2_param(const int16_t *sig, int64_t nsample, sgk_jnnv2_param_t param) {
    g_shim_rc = SGK_OK;
    sgk_prefix_params_t chk;
    sgk_prefix_params_preset(0, SGK_PORE_R9, &chk);
    chk.adaptor = param;
    if (sgk_prefix_params_check(&chk) != SGK_OK) { g_shim_rc = SGK_ERR_ARG; return {-1, -1}; }
    return jnnv2_one(sig, nsample, param, [&](StatArgs &a, const AdaptP &ap, DevBuf &) {
        return launch_k_adaptor_param(nullptr, a, ap, param.window);
    });
}

sgk_jnn_pair_t sgk_find_polya_param(const float *raw, int64_t nsample, float top, float bot, sgk_jnn_param_t param) {
    sgk_prefix_params_t chk;
    sgk_prefix_params_preset(1, SGK_PORE_R9, &chk);
    chk.polya = param;
    if (sgk_prefix_params_check(&chk) != SGK_OK) { g_shim_rc = SGK_ERR_ARG; return {-1, -1}; }
    return polya_one(raw, nsample, top, bot, param);
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
    sgk_prefix_params_t preset;
    sgk_prefix_params_preset(1, SGK_PORE_R9, &preset);
    return polya_one(raw, nsample, top, bot, preset.polya);
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
