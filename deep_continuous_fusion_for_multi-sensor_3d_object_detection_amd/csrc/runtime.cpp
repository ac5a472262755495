// runtime.cpp -- error text, version and the optional event-timing layer of libdcf_hip.so.
#include <stdarg.h>
#include <stdlib.h>

#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "dcf_common.h"

static thread_local char g_err[512] = "";

void dcf_set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

extern "C" const char *dcf_last_error(void) { return g_err; }
// 101: dcf_fusion_gather_bwd_inv gained its workspace argument (round 3); the CONV_LC / KNN_TILE_WAVES options (round 4).
// 102 (round 5): the four experimental dcf_conv3x3_*_wf entry points of 101 are GONE from the library (no caller outside
// tools/; they live in tools/variants/ now) -- INTEGRATION.md, "Versions"
// 200 (round 6): no prototype changed since 102, but 102 REMOVED symbols under a minor step; a binding that refuses on a major
// mismatch would have bound them at load and failed with "undefined symbol" instead.  The major moves now, and the policy is
// written down ("Versions"): removing or changing an exported symbol = new major; adding = new minor.
// 201: + dcf_relu_mask_rowscale_bwd
// 202 still: the deterministic-mode entries (dcf_inv_sort_segments, dcf_cam_invert, dcf_point_sample_bwd_det, dcf_fusion_gather_bwd_det,
// dcf_rowscale_bias_bwd_det, dcf_rows_fold, dcf_loss_fwd_bwd_det, dcf_loss_sample_fwd_bwd_det) and the hard-mining entries
// (dcf_loss_hard_workspace_bytes, dcf_loss_hard_fwd_bwd, dcf_loss_hard_fwd_bwd_det) and the focal entries (dcf_loss_focal_workspace_bytes,
// dcf_loss_focal_fwd_bwd, dcf_loss_focal_fwd_bwd_det) and the anchor-assignment entries (dcf_assign_anchors_workspace_bytes,
// dcf_assign_anchors_iou, dcf_loss_anchor_workspace_bytes, dcf_loss_anchor_fwd_bwd) were ADDED without a new minor:
// tests/test_amp_host.py pins 202 exactly.  A binding that needs them asks for the symbols (tests/test_determinism_host.py does).
extern "C" int dcf_version(void) { return 202; }

// ------------------------------------------------------------------ tuning options (dcf_common.h)
std::atomic<int> g_dcf_opt_epoch{0};
namespace {
std::mutex g_opt_mu;
std::map<std::string, const char *> g_opts;      // name -> interned value (nullptr = unset); never freed: call sites cache the pointers
}  // namespace

const char *dcf_opt(const char *name)
{
    std::lock_guard<std::mutex> lk(g_opt_mu);
    auto it = g_opts.find(name);
    if (it != g_opts.end()) return it->second;
    const char *e = getenv((std::string("DCF_") + name).c_str());   // once per option and process
    const char *v = e ? strdup(e) : nullptr;
    g_opts[name] = v;
    return v;
}

extern "C" int dcf_set_option(const char *name, const char *value)
{
    if (!name || !*name) {
        dcf_set_error("dcf_set_option: empty name");
        return DCF_EINVAL;
    }
    std::lock_guard<std::mutex> lk(g_opt_mu);
    g_opts[name] = value ? strdup(value) : nullptr;
    g_dcf_opt_epoch.fetch_add(1, std::memory_order_acq_rel);
    return DCF_OK;
}

// ------------------------------------------------------------------ profiling
// HIP events recorded on the launch stream around every DCF_LAUNCH while enabled.
// Elapsed times are only read in dcf_prof_read (which synchronises the events);
// nothing here runs unless the bench explicitly turns it on.
int g_dcf_prof_on = 0;

namespace {
struct Rec {
    int name_id;
    hipEvent_t a, b;
    double work, bytes;
};
std::mutex g_mu;
std::vector<std::string> g_names;
std::map<std::string, int> g_name_id;
std::vector<Rec> g_recs;
std::vector<hipEvent_t> g_pool;
hipEvent_t g_cur_a;
int g_cur_name = -1;
double g_cur_work = 0.0, g_cur_bytes = 0.0;

hipEvent_t get_event()
{
    if (!g_pool.empty()) {
        hipEvent_t e = g_pool.back();
        g_pool.pop_back();
        return e;
    }
    hipEvent_t e;
    (void)hipEventCreate(&e);
    return e;
}
}  // namespace

void dcf_prof_begin(const char *name, hipStream_t s, double work, double bytes)
{
    std::lock_guard<std::mutex> lk(g_mu);
    auto it = g_name_id.find(name);
    int id;
    if (it == g_name_id.end()) {
        id = (int)g_names.size();
        g_names.push_back(name);
        g_name_id[name] = id;
    } else {
        id = it->second;
    }
    g_cur_name = id;
    g_cur_work = work;
    g_cur_bytes = bytes;
    g_cur_a = get_event();
    (void)hipEventRecord(g_cur_a, s);
}

void dcf_prof_end(hipStream_t s)
{
    std::lock_guard<std::mutex> lk(g_mu);
    hipEvent_t b = get_event();
    (void)hipEventRecord(b, s);
    g_recs.push_back(Rec{g_cur_name, g_cur_a, b, g_cur_work, g_cur_bytes});
}

extern "C" int dcf_prof_enable(int on)
{
    g_dcf_prof_on = on ? 1 : 0;
    return DCF_OK;
}

extern "C" int dcf_prof_reset(void)
{
    std::lock_guard<std::mutex> lk(g_mu);
    for (auto &r : g_recs) {
        (void)hipEventSynchronize(r.b);
        g_pool.push_back(r.a);
        g_pool.push_back(r.b);
    }
    g_recs.clear();
    return DCF_OK;
}

extern "C" int dcf_prof_read(char *names, double *total_ms, int64_t *calls, double *work, int cap)
{
    return dcf_prof_read2(names, total_ms, calls, work, nullptr, cap);
}

extern "C" int dcf_prof_read2(char *names, double *total_ms, int64_t *calls, double *work, double *bytes, int cap)
{
    std::lock_guard<std::mutex> lk(g_mu);
    int n = (int)g_names.size();
    std::vector<double> tot(n, 0.0);
    std::vector<int64_t> cnt(n, 0);
    std::vector<double> wk(n, 0.0), by(n, 0.0);
    for (auto &r : g_recs) {
        (void)hipEventSynchronize(r.b);
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, r.a, r.b);
        tot[r.name_id] += ms;
        cnt[r.name_id] += 1;
        wk[r.name_id] += r.work;
        by[r.name_id] += r.bytes;
    }
    int k = 0;
    for (int i = 0; i < n && k < cap; ++i) {
        if (cnt[i] == 0) continue;
        strncpy(names + (size_t)k * 64, g_names[i].c_str(), 63);
        names[(size_t)k * 64 + 63] = 0;
        total_ms[k] = tot[i];
        calls[k] = cnt[i];
        if (work) work[k] = wk[i];
        if (bytes) bytes[k] = by[i];
        ++k;
    }
    return k;
}

// Empty event brackets on `stream`: their mean elapsed time is the fixed cost that event bracketing adds
// to every measured launch (the bench subtracts it before comparing with rocprofv3's kernel durations).
extern "C" int dcf_prof_calibrate(dcf_stream_t stream, int n)
{
    const int was = g_dcf_prof_on;
    g_dcf_prof_on = 1;
    for (int i = 0; i < n; ++i) {
        dcf_prof_begin("__empty_bracket__", (hipStream_t)stream, 0.0, 0.0);
        dcf_prof_end((hipStream_t)stream);
    }
    g_dcf_prof_on = was;
    return DCF_OK;
}
