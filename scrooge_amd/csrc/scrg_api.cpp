// scrg_api.cpp — host side of the C ABI declared in include/scrooge_amd.h.
//
// Mirrors the staging the reference does around its kernel
// (src/genasm_gpu.cu:890-1065: concatenate + pack sequences, size the CIGAR
// storage, launch, read CIGARs back) with explicit device memory instead of
// managed memory, status codes instead of exit(), and one handle per device
// instead of __managed__ globals.  There is no CPU fallback anywhere in this
// file: without a HIP device every entry point fails with SCRG_ERR_NO_DEVICE.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <numeric>
#include <string>
#include <thread>
#include <vector>

#include "genasm_kernels.h"
#include "edit_stream.h"
#include "host_path.h"
#include "site_rule.h"
#include "text_revcomp.h"
#include "mate_rule.h"
#include "mapq_rule.h"
#include "seed_rule.h"
#include "scrg_internal.h"
#include "../../include/scrooge_amd_io.h"

namespace {

std::atomic<int> g_log{0};
std::atomic<int> g_live_ctx{0};          // handles alive: the result pool is emptied when the last one goes
// the work queue is a 32-bit counter and every wavefront over-asks by up to 64 once it is empty (at most 32 wavefronts
// on each of at most 1024 CUs): leave room for that, or the counter could wrap and hand out low indices a second time
constexpr uint64_t kMaxPairsPerLaunch = 0xffffffffull - 64ull * 32ull * 1024ull;

using scrg_int::DevBuf;
using scrg_int::HostPinned;
using scrg_int::now_ns;
using scrg_int::parallel_for;

}  // namespace

struct scrg_ctx {
    int device = 0;
    int n_cus = 0;
    bool counted = true;          // false: a handle the library made for itself (host path slots)
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    hipEvent_t ev_start = nullptr, ev_stop = nullptr;
    bool have_timing = false;
    std::string last_error;

    DevBuf counter;     // work queue head
    DevBuf spill;       // HBM overflow rows of R
    DevBuf stats;       // profiling counters (params.reserved[1] != 0)
    DevBuf select_ws;   // scrg_select_best: the wavefronts' summaries (select_kernels.hip)
    DevBuf mate_ws;     // scrg_select_mates: the team size the first pass leaves for the second (mate_kernels.hip), a word per call in turn
    uint32_t mate_calls = 0;
    void* host_state = nullptr;   // the pipelined host-pointer path's buffers, streams and resident genome (scrg_host.cpp), made on first use
    bool text_strands = false;    // scrg_ctx_set_text_strands: bit 63 of a pair's text_off is honoured (text_revcomp.h)
    scrg_host::CallOptions opt;   // what the scrg_ctx_set_* entry points ask of the host calls (scrg_internal.h); the edit limit also holds for scrg_align_device*
    scrg_host::SideResults kept;  // the side results of the last host call, each until its scrg_ctx_take_* or the next align call
    uint32_t seed_smer = 0;       // scrg_ctx_set_seed_sampling: what the next scrg_genome_index builds with
    DevBuf pile_ws;               // scrg_pileup_finish: the tiles' sums
    DevBuf site_ws, site_out;     // scrg_ctx_take_pileup_sites: the site passes' scratch with the site count behind it, the records

    scrg_status fail(scrg_status s, const char* what, hipError_t e = hipSuccess)
    {
        last_error = what;
        if (e != hipSuccess) {
            last_error += ": ";
            last_error += hipGetErrorString(e);
            (void)hipGetLastError();
        }
        if (g_log.load()) fprintf(stderr, "[scrooge_amd] error: %s\n", last_error.c_str());
        return s;
    }
};

#define HIP_TRY(ctx, call)                                                     \
    do {                                                                       \
        hipError_t e__ = (call);                                               \
        if (e__ != hipSuccess)                                                 \
            return (ctx)->fail(e__ == hipErrorOutOfMemory ? SCRG_ERR_OOM : SCRG_ERR_HIP, #call, e__); \
    } while (0)

// the error text of this thread's last call without a handle (the _multi calls, scrg_multi_last_error)
static thread_local std::string g_multi_error;

// Host entry points never let a C++ exception cross the C boundary (std::vector growth on huge batches):
// allocation failures become SCRG_ERR_OOM, anything else SCRG_ERR_INVALID_ARG.  (c = nullptr: a call without a handle)
template <typename F> static scrg_status guarded(scrg_ctx* c, F&& f)
{
    auto fail = [&](scrg_status s, const char* what) { return c ? c->fail(s, what) : (g_multi_error = what, s); };
    try {
        return f();
    } catch (const std::bad_alloc&) {
        return fail(SCRG_ERR_OOM, "host allocation failed");
    } catch (...) {
        return fail(SCRG_ERR_INVALID_ARG, "unexpected exception");
    }
}

// a side result of the last host call changes hands, once (`none`: what the caller reads when there is nothing)
template <typename T> static scrg_status take_kept(scrg_ctx* c, T* scrg_host::SideResults::*which, T** out, const char* none)
{
    if (out) *out = nullptr;
    if (!c || !out) return SCRG_ERR_INVALID_ARG;
    if (!(c->kept.*which)) return c->fail(SCRG_ERR_INVALID_ARG, none);
    *out = std::exchange(c->kept.*which, nullptr);
    return SCRG_OK;
}

using scrg_int::g_diff_pool;
using scrg_int::g_pool;

extern "C" {

void scrg_params_default(scrg_params* p)
{
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->W = 64;                // src/genasm_cpu.cpp:7
    p->O = 33;                // src/genasm_cpu.cpp:9
    p->lanes_per_pair = 0;    // 0 = chosen for W: see scrg_params_resolve()
    p->lds_rows = 0;
    p->waves_per_cu = 0;
    p->sort_by_length = 1;
}

const char* scrg_status_string(scrg_status s)
{
    switch (s) {
    case SCRG_OK: return "ok";
    case SCRG_ERR_INVALID_ARG: return "invalid argument";
    case SCRG_ERR_BAD_BASE: return "sequence contains a character other than ACGTacgt";
    case SCRG_ERR_NO_DEVICE: return "no usable HIP device";
    case SCRG_ERR_HIP: return "HIP runtime error";
    case SCRG_ERR_OOM: return "out of memory";
    case SCRG_ERR_CIGAR_OVERFLOW: return "CIGAR arena slice too small";
    case SCRG_PAIR_OVER_EDIT_LIMIT: return "pair over its edit limit";
    case SCRG_PAIR_NOT_BEST: return "pair is not its read's best candidate";
    default: return "unknown status";
    }
}

void scrg_set_log(int enabled) { g_log.store(enabled ? 1 : 0); }
int scrg_get_log(void) { return g_log.load(); }

int scrg_abi_version(void) { return SCRG_ABI_VERSION; }

int scrg_build_flags(void)
{
    int f = 0;
#ifdef SCRG_STATS
    f |= SCRG_BUILD_STATS;
#endif
#ifdef SCRG_ABLATE
    f |= SCRG_BUILD_ABLATE;
#endif
#ifdef SCRG_SELECT
    f |= SCRG_BUILD_SELECT;
#endif
    return f;
}

int scrg_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return n;
}

static scrg_status ctx_create_impl(int device, scrg_ctx** out, bool counted)
{
    if (!out) return SCRG_ERR_INVALID_ARG;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device < 0 || device >= n) {
        (void)hipGetLastError();
        return SCRG_ERR_NO_DEVICE;
    }
    if (hipSetDevice(device) != hipSuccess) return SCRG_ERR_NO_DEVICE;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return SCRG_ERR_NO_DEVICE;
    scrg_ctx* c = new (std::nothrow) scrg_ctx();
    if (!c) return SCRG_ERR_OOM;
    c->device = device;
    c->n_cus = prop.multiProcessorCount;
    c->counted = counted;
    if (hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreate(&c->ev_start) != hipSuccess || hipEventCreate(&c->ev_stop) != hipSuccess) {
        delete c;
        return SCRG_ERR_HIP;
    }
    c->stream = c->own_stream;
    if (counted) g_live_ctx.fetch_add(1);
    if (counted && g_log.load())
        fprintf(stderr, "[scrooge_amd] device %d: %s, %d CUs, arch %s\n", device, prop.name, c->n_cus,
                prop.gcnArchName);
    *out = c;
    return SCRG_OK;
}

scrg_status scrg_ctx_create(int device, scrg_ctx** out) { return ctx_create_impl(device, out, true); }

void scrg_ctx_destroy(scrg_ctx* c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)hipDeviceSynchronize();
    c->counter.release();
    c->spill.release();
    c->stats.release();
    c->select_ws.release();
    c->mate_ws.release();
    c->pile_ws.release();
    c->site_ws.release();
    c->site_out.release();
    c->kept.reset();
    if (c->host_state) scrg_host::state_free(c->host_state);
    c->host_state = nullptr;
    (void)hipSetDevice(c->device);
    if (c->ev_start) (void)hipEventDestroy(c->ev_start);
    if (c->ev_stop) (void)hipEventDestroy(c->ev_stop);
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    const bool counted = c->counted;
    delete c;
    if (counted && g_live_ctx.fetch_sub(1) == 1) { g_pool.trim(); g_diff_pool.trim(); }      // the caller's last handle gone: give the recycled result arrays back
}

scrg_status scrg_ctx_set_stream(scrg_ctx* c, void* hip_stream)
{
    if (!c) return SCRG_ERR_INVALID_ARG;
    c->stream = static_cast<hipStream_t>(hip_stream);
    return SCRG_OK;
}

scrg_status scrg_ctx_use_own_stream(scrg_ctx* c)
{
    if (!c) return SCRG_ERR_INVALID_ARG;
    c->stream = c->own_stream;
    return SCRG_OK;
}

scrg_status scrg_ctx_set_edit_limit(scrg_ctx* c, int64_t max_edits, int32_t per_mille)
{
    if (!c) return SCRG_ERR_INVALID_ARG;
    if (per_mille < 0 || per_mille > 1000) return c->fail(SCRG_ERR_INVALID_ARG, "per_mille must be 0 (none) or 1..1000");
    c->opt.max_edits = max_edits < 0 ? -1 : max_edits;
    c->opt.per_mille = per_mille;
    return SCRG_OK;
}

scrg_status scrg_ctx_get_edit_limit(const scrg_ctx* c, int64_t* max_edits, int32_t* per_mille)
{
    if (!c) return SCRG_ERR_INVALID_ARG;
    if (max_edits) *max_edits = c->opt.max_edits;
    if (per_mille) *per_mille = c->opt.per_mille;
    return SCRG_OK;
}

scrg_status scrg_ctx_set_text_strands(scrg_ctx* c, int enabled)
{
    if (!c) return SCRG_ERR_INVALID_ARG;
    c->text_strands = enabled != 0;
    return SCRG_OK;
}

scrg_status scrg_ctx_get_text_strands(const scrg_ctx* c, int* enabled)
{
    if (!c || !enabled) return SCRG_ERR_INVALID_ARG;
    *enabled = c->text_strands ? 1 : 0;
    return SCRG_OK;
}

scrg_status scrg_ctx_set_diff(scrg_ctx* c, int32_t kind)
{
    if (!c) return SCRG_ERR_INVALID_ARG;
    if (kind != SCRG_DIFF_OFF && kind != SCRG_DIFF_MD && kind != SCRG_DIFF_CS)
        return c->fail(SCRG_ERR_INVALID_ARG, "the difference-string kind is SCRG_DIFF_OFF, SCRG_DIFF_MD or SCRG_DIFF_CS");
    c->opt.diff_kind = kind;
    return SCRG_OK;
}

scrg_status scrg_ctx_get_diff(const scrg_ctx* c, int32_t* kind)
{
    if (!c || !kind) return SCRG_ERR_INVALID_ARG;
    *kind = c->opt.diff_kind;
    return SCRG_OK;
}

static bool cigar_form_ok(int32_t form) { return form == SCRG_CIGAR_WINDOWED || form == SCRG_CIGAR_MERGED || form == SCRG_CIGAR_M; }

scrg_status scrg_ctx_set_cigar_form(scrg_ctx* c, int32_t form)
{
    if (!c) return SCRG_ERR_INVALID_ARG;
    if (!cigar_form_ok(form)) return c->fail(SCRG_ERR_INVALID_ARG, "the CIGAR form is SCRG_CIGAR_WINDOWED, SCRG_CIGAR_MERGED or SCRG_CIGAR_M");
    c->opt.cigar_form = form;
    return SCRG_OK;
}

scrg_status scrg_ctx_get_cigar_form(const scrg_ctx* c, int32_t* form)
{
    if (!c || !form) return SCRG_ERR_INVALID_ARG;
    *form = c->opt.cigar_form;
    return SCRG_OK;
}

scrg_status scrg_ctx_take_diff(scrg_ctx* c, scrg_diff** out)
{
    return take_kept(c, &scrg_host::SideResults::diff, out, "no difference strings to take: none were made by the last align call, or they were taken already");
}

void scrg_diff_free(scrg_diff* d)
{
    if (!d) return;
    g_diff_pool.put(d->offset);
    g_diff_pool.put(d->text);
    free(d);
}

scrg_status scrg_ctx_set_report(scrg_ctx* c, int enabled)
{
    if (!c) return SCRG_ERR_INVALID_ARG;
    c->opt.report = enabled != 0;
    return SCRG_OK;
}

scrg_status scrg_ctx_get_report(const scrg_ctx* c, int* enabled)
{
    if (!c || !enabled) return SCRG_ERR_INVALID_ARG;
    *enabled = c->opt.report ? 1 : 0;
    return SCRG_OK;
}

scrg_status scrg_ctx_take_report(scrg_ctx* c, scrg_report** out)
{
    return take_kept(c, &scrg_host::SideResults::report, out, "no alignment report to take: none was made by the last align call, or it was taken already");
}

void scrg_report_free(scrg_report* r)
{
    if (!r) return;
    free(r->pairs);
    free(r);
}

static const char* const kMapqRuleWanted = "mapq rule: per_edit 0 .. 255, max_q 0 .. 254, zero_per_mille 1 .. 1000, min_keep_q 0 .. 254 and a zero reserved word are wanted";
static const scrg_mapq_rule kMapqDefaults = {10, 60, 250, 0, 0};
static bool mapq_rule_ok(const scrg_mapq_rule& r) { return scrg::mapq_rule_valid(r.per_edit, r.max_q, r.zero_per_mille, r.min_keep_q, r.reserved); }

scrg_status scrg_ctx_set_read_summary(scrg_ctx* c, const scrg_mapq_rule* rule, int enabled)
{
    if (!c) return SCRG_ERR_INVALID_ARG;
    if (!rule) rule = &kMapqDefaults;
    if (!mapq_rule_ok(*rule)) return c->fail(SCRG_ERR_INVALID_ARG, kMapqRuleWanted);
    c->opt.read_summary = enabled != 0;
    c->opt.mapq_rule = *rule;
    return SCRG_OK;
}

scrg_status scrg_ctx_get_read_summary(const scrg_ctx* c, scrg_mapq_rule* rule, int* enabled)
{
    if (!c) return SCRG_ERR_INVALID_ARG;
    if (rule) *rule = c->opt.mapq_rule;
    if (enabled) *enabled = c->opt.read_summary ? 1 : 0;
    return SCRG_OK;
}

scrg_status scrg_ctx_take_read_summary(scrg_ctx* c, scrg_read_summaries** out)
{
    return take_kept(c, &scrg_host::SideResults::summary, out, "no read summary to take: none was made by the last align call, or it was taken already");
}

void scrg_read_summaries_free(scrg_read_summaries* s)
{
    if (!s) return;
    free(s->reads);
    free(s);
}

scrg_status scrg_ctx_set_clip(scrg_ctx* c, int enabled, const int32_t* costs)
{
    if (!c) return SCRG_ERR_INVALID_ARG;
    static const int32_t usual[4] = {2, 4, 4, 2};
    if (!costs) costs = usual;
    if (!scrg_host::clip_costs_ok(costs)) return c->fail(SCRG_ERR_INVALID_ARG, "clip costs: match in 1..255, mismatch, gap_open and gap_extend in 0..255");
    c->opt.clip = enabled != 0;
    memcpy(c->opt.clip_costs, costs, sizeof(c->opt.clip_costs));
    return SCRG_OK;
}

scrg_status scrg_ctx_get_clip(const scrg_ctx* c, int* enabled, int32_t* costs)
{
    if (!c) return SCRG_ERR_INVALID_ARG;
    if (enabled) *enabled = c->opt.clip ? 1 : 0;
    if (costs) memcpy(costs, c->opt.clip_costs, sizeof(c->opt.clip_costs));
    return SCRG_OK;
}

scrg_status scrg_ctx_take_clip(scrg_ctx* c, scrg_clip** out)
{
    return take_kept(c, &scrg_host::SideResults::clip, out, "no clip records to take: none were made by the last align call, or they were taken already");
}

void scrg_clip_free(scrg_clip* r)
{
    if (!r) return;
    free(r->pairs);
    free(r);
}

scrg_status scrg_ctx_set_pileup(scrg_ctx* c, int enabled)
{
    if (!c) return SCRG_ERR_INVALID_ARG;
    c->opt.pileup = enabled != 0;
    if (!c->opt.pileup && c->host_state) scrg_host::pileup_discard(c->host_state, true);       // (off: no device memory is held)
    return SCRG_OK;
}

scrg_status scrg_ctx_get_pileup(const scrg_ctx* c, int* enabled)
{
    if (!c || !enabled) return SCRG_ERR_INVALID_ARG;
    *enabled = c->opt.pileup ? 1 : 0;
    return SCRG_OK;
}

// finish in place, bring planes and counters home, leave the accumulator empty (the next call that adds zeroes it)
scrg_status scrg_ctx_take_pileup(scrg_ctx* c, scrg_pileup** out)
{
    if (out) *out = nullptr;
    if (!c || !out) return SCRG_ERR_INVALID_ARG;
    scrg_host::PileupView v;
    if (!c->host_state || !scrg_host::pileup_view(c->host_state, &v))
        return c->fail(SCRG_ERR_INVALID_ARG, "no pileup to take: nothing was accumulated since the last take (scrg_ctx_set_pileup)");
    const uint64_t words = (uint64_t)SCRG_PILE_PLANES * (v.target_len + 1);
    scrg_pileup* r = static_cast<scrg_pileup*>(calloc(1, sizeof(scrg_pileup)));
    uint32_t* counts = static_cast<uint32_t*>(malloc((words + 2) * sizeof(uint32_t)));
    if (!r || !counts) {
        free(r);
        free(counts);
        return c->fail(SCRG_ERR_OOM, "pileup counts");
    }
    scrg_status s = scrg_pileup_finish(c, v.target_len, v.d_acc, v.d_acc);
    if (s == SCRG_OK) {
        hipError_t e = hipMemcpyAsync(counts, v.d_acc, (words + 2) * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) s = c->fail(SCRG_ERR_HIP, "pileup read-back", e);
    }
    scrg_host::pileup_discard(c->host_state, false);
    if (s != SCRG_OK) {
        free(r);
        free(counts);
        return s;
    }
    r->target_len = v.target_len;
    r->n_out_of_range = counts[words];
    r->n_alignments = counts[words + 1];
    r->counts = counts;
    *out = r;
    return SCRG_OK;
}

void scrg_pileup_free(scrg_pileup* p)
{
    if (!p) return;
    free(p->counts);
    free(p);
}

static const char* site_rule_error(const scrg_site_rule* rule)
{
    if (!rule) return "null site rule";
    if (!scrg::site_rule_valid(rule->min_depth, rule->min_alt_per_mille, rule->reserved))
        return "site rule: min_depth >= 1, min_alt_per_mille <= 1000, reserved = 0 (scrg_site_rule)";
    return nullptr;
}

// finish in place, mark, bring the count home, write, bring the sites and the counters home, leave the accumulator empty
scrg_status scrg_ctx_take_pileup_sites(scrg_ctx* c, const scrg_site_rule* rule, scrg_pileup_sites** out)
{
    if (out) *out = nullptr;
    if (!c || !out) return SCRG_ERR_INVALID_ARG;
    if (const char* why = site_rule_error(rule)) return c->fail(SCRG_ERR_INVALID_ARG, why);
    scrg_host::PileupView v;
    if (!c->host_state || !scrg_host::pileup_view(c->host_state, &v))
        return c->fail(SCRG_ERR_INVALID_ARG, "no pileup to take: nothing was accumulated since the last take (scrg_ctx_set_pileup)");
    // (refusals up to here keep the accumulator)
    const uint64_t* d_seq = nullptr;
    if (!scrg_host::pileup_genome(c->host_state, v.target_len, &d_seq))
        return c->fail(SCRG_ERR_INVALID_ARG, "the pileup sites need the genome the pileup was made on: none is resident, or one of another length (scrg_ctx_take_pileup serves the counts)");
    if (v.target_len >= 0xffffffffull)
        return c->fail(SCRG_ERR_INVALID_ARG, "pileup sites have 32-bit offsets: target_len must be below 2^32 - 1 (scrg_ctx_take_pileup serves the counts)");
    scrg_pileup_sites* r = static_cast<scrg_pileup_sites*>(calloc(1, sizeof(scrg_pileup_sites)));
    if (!r) return c->fail(SCRG_ERR_OOM, "pileup sites");
    const size_t scratch = scrg_pileup_sites_scratch_bytes(v.target_len);
    const uint64_t words = (uint64_t)SCRG_PILE_PLANES * (v.target_len + 1);
    uint64_t n_sites = 0;
    uint32_t counters[2] = {0, 0};
    scrg_site* sites = nullptr;
    auto work = [&]() -> scrg_status {
        HIP_TRY(c, hipSetDevice(c->device));
        HIP_TRY(c, c->site_ws.ensure(scratch + sizeof(uint64_t)));
        uint64_t* const d_n = reinterpret_cast<uint64_t*>(c->site_ws.as<char>() + scratch);
        scrg_status s = scrg_pileup_finish(c, v.target_len, v.d_acc, v.d_acc);
        if (s == SCRG_OK) s = scrg_pileup_sites_mark(c, v.target_len, v.d_acc, d_seq, 0, rule, c->site_ws.p, d_n);
        if (s != SCRG_OK) return s;
        HIP_TRY(c, hipMemcpyAsync(&n_sites, d_n, sizeof(n_sites), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipMemcpyAsync(counters, v.d_acc + words, sizeof(counters), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        if (n_sites == 0) return SCRG_OK;
        sites = static_cast<scrg_site*>(malloc(n_sites * sizeof(scrg_site)));
        if (!sites) return c->fail(SCRG_ERR_OOM, "pileup sites");
        HIP_TRY(c, c->site_out.ensure(n_sites * sizeof(scrg_site)));
        s = scrg_pileup_sites_write(c, v.target_len, v.d_acc, d_seq, 0, c->site_ws.p, n_sites, c->site_out.as<scrg_site>());
        if (s != SCRG_OK) return s;
        HIP_TRY(c, hipMemcpyAsync(sites, c->site_out.p, n_sites * sizeof(scrg_site), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        return SCRG_OK;
    };
    const scrg_status s = work();
    scrg_host::pileup_discard(c->host_state, false);
    if (s != SCRG_OK) {
        free(sites);
        free(r);
        return s;
    }
    r->target_len = v.target_len;
    r->n_out_of_range = counters[0];
    r->n_alignments = counters[1];
    r->n_sites = n_sites;
    r->rule = *rule;
    r->sites = sites;
    *out = r;
    return SCRG_OK;
}

void scrg_pileup_sites_free(scrg_pileup_sites* p)
{
    if (!p) return;
    free(p->sites);
    free(p);
}

// What the kernels compute per pair (lane_common.h: pair_edit_limit), for any read length: floor(per_mille * L / 1000) without
// overflow, the minimum with max_edits; -1 = no limit.
scrg_status scrg_edit_limit_for(int64_t max_edits, int32_t per_mille, uint64_t read_len, int64_t* limit)
{
    if (!limit || per_mille < 0 || per_mille > 1000) return SCRG_ERR_INVALID_ARG;
    int64_t lim = max_edits < 0 ? -1 : max_edits;
    if (per_mille > 0) {
        const uint64_t pm = (uint64_t)per_mille;
        const uint64_t by_len = (read_len / 1000u) * pm + (read_len % 1000u) * pm / 1000u;     // <= read_len
        const int64_t b = by_len > (uint64_t)INT64_MAX ? INT64_MAX : (int64_t)by_len;
        lim = lim < 0 ? b : std::min(lim, b);
    }
    *limit = lim;
    return SCRG_OK;
}

scrg_status scrg_stream_create(int device, int priority, void** stream)
{
    if (!stream || priority < -1 || priority > 1) return SCRG_ERR_INVALID_ARG;
    hipStream_t s = nullptr;
    if (hipSetDevice(device) != hipSuccess) return SCRG_ERR_NO_DEVICE;
    if (hipStreamCreateWithPriority(&s, hipStreamNonBlocking, priority) != hipSuccess) return SCRG_ERR_HIP;
    *stream = s;
    return SCRG_OK;
}

scrg_status scrg_stream_destroy(void* stream)
{
    if (!stream) return SCRG_OK;
    return hipStreamDestroy(static_cast<hipStream_t>(stream)) == hipSuccess ? SCRG_OK : SCRG_ERR_HIP;
}

const char* scrg_last_error(const scrg_ctx* c) { return c ? c->last_error.c_str() : "null context"; }

// ---------------------------------------------------------------------------
// launch geometry
// ---------------------------------------------------------------------------
// why the last resolve_params of this thread refused its parameters (the text behind SCRG_ERR_INVALID_ARG)
static thread_local const char* g_params_error = "bad scrg_params";

// the kernel form these parameters get and what it takes to launch it (genasm_kernels.h)
static scrg::LaunchPlan plan_for(const scrg_params& p, scrg::LaneOutput out)
{
    return scrg::launch_plan(p, out, scrg::align_form(p.W, p.W - p.O, p.lanes_per_pair, SCRG_SEL(p.reserved[0], scrg::SCRG_SWITCH_MW_TABLE)));
}

static bool resolve_params(const scrg_params* in, scrg_params* p)
{
    g_params_error = "bad scrg_params";
    scrg_params_default(p);
    if (in) {
        if (in->W) p->W = in->W;
        if (in->O || in->W) p->O = in->O;
        p->lanes_per_pair = in->lanes_per_pair;
        p->lds_rows = in->lds_rows;
        p->waves_per_cu = in->waves_per_cu;
        p->sort_by_length = in->sort_by_length;
        p->text_stride_words = in->text_stride_words;
        p->read_stride_words = in->read_stride_words;
        p->outputs = in->outputs;
        p->reserved[0] = in->reserved[0];      // ablation switches and profiling counters travel with the parameters
        p->reserved[1] = in->reserved[1];
        p->stranded = in->stranded;
    }
    if (p->stranded != 0 && p->stranded != 1) return false;
    // experiment switches: only those that leave the results intact, unless this is an ablation build (genasm_kernels.h)
    if (p->reserved[0] & ~scrg::SCRG_ALLOWED_SWITCHES) return false;
    if (p->reserved[1] && !scrg::SCRG_HAVE_STATS) return false;       // the kernels' counters exist in -DSCRG_STATS builds only
    // (SCRG_OUT_BEST is a flag on top of the three; runs-and-text-suppressed, 3, stays invalid.  SCRG_OUT_DISTANCE is a flag
    // that excludes the three — there is nothing to render —: 16, and 20 with SCRG_OUT_BEST)
    if (p->outputs < 0 || (p->outputs & ~(3 | SCRG_OUT_BEST | SCRG_OUT_DISTANCE)) || (p->outputs & 3) > SCRG_OUT_RUNS) return false;
    if ((p->outputs & SCRG_OUT_DISTANCE) && (p->outputs & 3)) {
        g_params_error = "SCRG_OUT_DISTANCE excludes SCRG_OUT_TEXT and SCRG_OUT_RUNS: valid with it are 16 and 16 | SCRG_OUT_BEST";
        return false;
    }
    if (p->text_stride_words == 0) p->text_stride_words = 1;
    if (p->read_stride_words == 0) p->read_stride_words = 1;
    if (p->text_stride_words < 1 || p->read_stride_words < 1) return false;
    if (p->W < 2 || p->W > 256) return false;
    const int tbl = p->W - p->O;
    // O = 0 (no overlap: the reference's special case src/genasm_cpu.cpp:104-110, reached by its O sweep for W < 32,
    // scripts/profile.py:92-93): a window's traceback may consume all W characters.  The one-pair-per-lane kernels serve it
    // (a table column holds the steps OUT of it, so column W-1 needs nothing of the boundary column); the GenASM-row
    // mappings, whose traceback reads R[i+1], do not.
    if (tbl < 1 || p->O < 0) return false;
    // a run's count is one byte (scrg_run, the edit streams' replay, the reference's CigarEntry_t): a window that is one run of
    // W-O = 256 operations (W = 256, O = 0 alone) cannot be written.  The reference's own counter wraps to 0 there and it drops
    // the run (src/genasm_cpu.cpp:305, 388-401: its CIGAR no longer consumes the read), so there is nothing to be identical to.
    if (tbl > 255) { g_params_error = "W-O must be <= 255: a run count is one byte (W = 256 needs O >= 1)"; return false; }
    if (p->O == 0 && p->lanes_per_pair > 1) return false;
    const size_t row_bytes = (size_t)scrg::stored_row_dwords(p->W, tbl) * 4;
    // one pair per lane for every W (genasm_kernels.h: align_form); the GenASM-row kernels stay selectable, with multi-word
    // entries for W > 64 (genasm_kernel_multiword.hip): slots of 32 or 64 lanes
    if (p->lanes_per_pair == 0) p->lanes_per_pair = 1;
    if (p->W > 64 && p->lanes_per_pair != 1 && p->lanes_per_pair != 32 && p->lanes_per_pair != 64) return false;
    if (p->lds_rows == 0) {
        if (p->W <= 64 || p->lanes_per_pair == 1) {
            p->lds_rows = 12;                                       // (one pair per lane: not used)
        } else {                                                    // as many rows of R in LDS as fit in about 40 KB per wavefront, the rest of a window's rows go to HBM
            const size_t fit = (40u << 10) / (row_bytes * (64 / p->lanes_per_pair));
            p->lds_rows = (int32_t)std::min<size_t>(32, std::max<size_t>(4, fit));
        }
    }
    if (p->waves_per_cu == 0) p->waves_per_cu = plan_for(*p, scrg::LANE_OUT_RUNS).default_waves_per_cu;
    const int g = p->lanes_per_pair;
    // reverse-strand pairs from one packed copy of the read: the one-pair-per-lane kernels (every W / O)
    if (p->stranded && g != 1) return false;
    if (g == 1) return p->waves_per_cu >= 1 && p->waves_per_cu <= 32;      // no table in LDS: lds_rows is not used
    if (p->text_stride_words != 1 || p->read_stride_words != 1) return false;   // strided sequences: lane kernel only
    if (!(g == 4 || g == 8 || g == 16 || g == 32 || g == 64)) return false;
    if (p->lds_rows < 1) return false;
    if (p->lds_rows > p->W + 1) p->lds_rows = p->W + 1;
    // one wavefront's table has to fit the 160 KB of a CU
    const size_t per_row = row_bytes * (64 / g);
    if ((size_t)p->lds_rows * per_row > (150u << 10)) p->lds_rows = (int32_t)std::max<size_t>(1, (150u << 10) / per_row);
    if (p->waves_per_cu < 1 || p->waves_per_cu > 32) return false;
    return true;
}

// wavefronts of a launch that fills the GPU: waves_per_cu on every CU, fewer where a CU's LDS (160 KB) does not hold that many
static int32_t full_waves(const scrg_ctx* c, const scrg_params& p, const scrg::LaunchPlan& plan)
{
    int wpc = p.waves_per_cu;
    const size_t lds_cap = 160 * 1024;
    if (plan.lds_bytes * wpc > lds_cap) wpc = (int)std::max<size_t>(1, lds_cap / plan.lds_bytes);      // (lds = 0: genasm_lane_mw_kernel in distance-only mode)
    return c->n_cus * wpc;
}

scrg_status scrg_params_resolve(const scrg_params* in, scrg_params* out)
{
    if (!out) return SCRG_ERR_INVALID_ARG;
    return resolve_params(in, out) ? SCRG_OK : SCRG_ERR_INVALID_ARG;
}

scrg_status scrg_query_launch(scrg_ctx* c, const scrg_params* params, int32_t* n_waves, int32_t* pairs_per_wave,
                              int32_t* lds_bytes, int32_t* n_cus)
{
    if (!c) return SCRG_ERR_INVALID_ARG;
    scrg_params p;
    if (!resolve_params(params, &p)) return c->fail(SCRG_ERR_INVALID_ARG, g_params_error);
    // (distance-only mode, one pair per lane: no staging ring and no insertion-run lengths — genasm_kernels.h: LaneOutput)
    const scrg::LaunchPlan plan = plan_for(p, (p.outputs & SCRG_OUT_DISTANCE) ? scrg::LANE_OUT_NONE : scrg::LANE_OUT_RUNS);
    if (n_waves) *n_waves = full_waves(c, p, plan);
    if (pairs_per_wave) *pairs_per_wave = plan.pairs_per_wave;
    if (lds_bytes) *lds_bytes = (int32_t)plan.lds_bytes;
    if (n_cus) *n_cus = c->n_cus;
    return SCRG_OK;
}

// ---------------------------------------------------------------------------
// device-pointer entry points
// ---------------------------------------------------------------------------
scrg_status scrg_pack_planar(scrg_ctx* c, const char* d_ascii, uint64_t n_words, uint64_t* d_planar,
                             uint32_t* d_bad_count)
{
    if (!c || (n_words && (!d_ascii || !d_planar)) || !d_bad_count) return SCRG_ERR_INVALID_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, scrg::launch_pack_planar(d_ascii, n_words, d_planar, d_bad_count, c->n_cus, c->stream));
    return SCRG_OK;
}

scrg_status scrg_pack_planar_groups(scrg_ctx* c, const char* d_ascii, uint64_t n_rows, uint64_t words_per_row,
                                    uint64_t* d_planar, uint32_t* d_bad_count)
{
    if (!c || (n_rows && words_per_row && (!d_ascii || !d_planar)) || !d_bad_count) return SCRG_ERR_INVALID_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, scrg::launch_pack_planar_groups(d_ascii, n_rows, words_per_row, d_planar, d_bad_count, c->n_cus, c->stream));
    return SCRG_OK;
}

static scrg_status align_device_impl(scrg_ctx* c, const scrg_params* params, uint64_t n_pairs, const uint64_t* d_seq,
                                     const scrg_pair_desc* d_pairs, scrg_run* d_runs, int64_t* d_edit_distance,
                                     uint32_t* d_n_runs, uint32_t* d_pair_status, scrg::LaneOutput out, uint32_t* d_run_count = nullptr,
                                     uint32_t* d_text_end = nullptr)
{
    if (!c) return SCRG_ERR_INVALID_ARG;
    scrg_params p;
    if (!resolve_params(params, &p)) return c->fail(SCRG_ERR_INVALID_ARG, g_params_error);
    const bool edits = out == scrg::LANE_OUT_EDITS, distance = out == scrg::LANE_OUT_NONE;
    if (distance && p.lanes_per_pair != 1)
        return c->fail(SCRG_ERR_INVALID_ARG, "distance-only output needs lanes_per_pair = 1, the default (the GenASM-row mappings always write runs)");
    if (edits && p.lanes_per_pair != 1)
        return c->fail(SCRG_ERR_INVALID_ARG, "edit-stream output needs lanes_per_pair = 1, the default "
                                             "(the GenASM-row mappings: scrg_align_device + scrg_encode_edit_stream)");
    if (c->opt.has_edit_limit() && p.lanes_per_pair != 1)
        return c->fail(SCRG_ERR_INVALID_ARG, "an edit limit needs lanes_per_pair = 1, the default (the GenASM-row mappings have none)");
    if (c->text_strands && p.lanes_per_pair != 1)
        return c->fail(SCRG_ERR_INVALID_ARG, "text strands need lanes_per_pair = 1, the default (the GenASM-row mappings read texts forwards only)");
    if (n_pairs > kMaxPairsPerLaunch) return c->fail(SCRG_ERR_INVALID_ARG, "too many pairs for one launch");
    if (n_pairs && (!d_seq || !d_pairs || (!distance && (!d_runs || !d_n_runs)) || !d_edit_distance || !d_pair_status))
        return c->fail(SCRG_ERR_INVALID_ARG, "null device pointer");
    HIP_TRY(c, hipSetDevice(c->device));
    c->have_timing = false;
    if (n_pairs == 0) return SCRG_OK;

    // (scrg_params.outputs belongs to the host entry points; here the ENTRY POINT says what is delivered, and the launch geometry is that mode's)
    const scrg::LaunchPlan plan = plan_for(p, out);
    int32_t n_waves = full_waves(c, p, plan);
    // no point in launching more slots than pairs
    const uint64_t need_waves = (n_pairs + plan.pairs_per_wave - 1) / plan.pairs_per_wave;
    // One pair per lane, runs output, the default table (W <= 64, W-O <= 31): a launch of at most one wavefront per SIMD (65 536
    // pairs on 1024 SIMDs) is bound by the chain of a pair's windows, not by issue slots — it runs with a window's work split
    // over a producer and a consumer wavefront (genasm_lane_split_kernel: 1.93 -> 1.50 ms for 25 k ... 50 k x 10 kb pairs, the
    // chunks of the host entry points included).  From two wavefronts on some SIMDs on the split gains nothing (100 k pairs:
    // 2.51 vs 2.52 ms: those SIMDs are the last to finish either way), and launches that fill the GPU or overlap with others —
    // and edit-stream output — keep the one-wavefront kernel (3 % fewer instructions).  (Test build, -DSCRG_SELECT: reserved[0] = 512 / 1024 force one or the other.)
    bool lane_split = false;
    // A caller that set scrg_params.waves_per_cu itself (co-resident work sized from scrg_query_launch, a work queue shorter than
    // the batch) gets exactly that geometry: the split form, which has its own (two workgroups of eight wavefronts per CU), is
    // then only taken when asked for.
    const bool user_waves = params && params->waves_per_cu > 0;
    if (plan.form == scrg::FORM_LANE && out == scrg::LANE_OUT_RUNS && !SCRG_SEL(p.reserved[0], scrg::SCRG_SWITCH_NO_SPLIT) && !(params && params->reserved[1])) {
        const uint64_t simds = 4ull * (uint64_t)c->n_cus;
        lane_split = SCRG_SEL(p.reserved[0], scrg::SCRG_SWITCH_SPLIT) || (need_waves <= simds && !user_waves);
        if (lane_split) n_waves = c->n_cus * scrg::LANE_SPLIT_PRODUCERS_PER_CU;
    }
    if ((uint64_t)n_waves > need_waves) n_waves = (int32_t)need_waves;

    HIP_TRY(c, c->counter.ensure(sizeof(uint32_t)));
    HIP_TRY(c, c->spill.ensure(plan.spill_for(n_waves)));
    HIP_TRY(c, hipMemsetAsync(c->counter.p, 0, sizeof(uint32_t), c->stream));

    scrg::AlignArgs a;
    a.seq = d_seq;
    a.pairs = d_pairs;
    a.runs = reinterpret_cast<uint16_t*>(d_runs);
    a.ed = d_edit_distance;
    a.n_runs = d_n_runs;
    if (distance) a.text_end = d_text_end;       // (the same kernel argument: genasm_kernels.h)
    a.status = d_pair_status;
    a.run_count = d_run_count;
    a.counter = c->counter.as<uint32_t>();
    a.spill = c->spill.as<uint32_t>();
    a.n_pairs = (uint32_t)n_pairs;
    a.W = p.W;
    a.tb_limit = p.W - p.O;
    a.lds_rows = p.lds_rows;
    a.text_stride = (uint32_t)p.text_stride_words;
    a.read_stride = (uint32_t)p.read_stride_words;
    a.debug = p.reserved[0];
    a.stranded = (uint32_t)p.stranded;
    a.max_edits = c->opt.max_edits < 0 ? 0xffffffffu : (uint32_t)std::min<int64_t>(c->opt.max_edits, 0xffffffffll);     // (no 32-bit sum of edits exceeds 0xffffffff)
    a.per_mille = (uint32_t)c->opt.per_mille;
    a.text_rev = c->text_strands ? 1u : 0u;
    a.stats = nullptr;
    if (params && params->reserved[1]) {
        HIP_TRY(c, c->stats.ensure(12 * sizeof(uint64_t)));
        HIP_TRY(c, hipMemsetAsync(c->stats.p, 0, 12 * sizeof(uint64_t), c->stream));
        a.stats = c->stats.as<uint64_t>();
    }

    HIP_TRY(c, hipEventRecord(c->ev_start, c->stream));
    const size_t lds = plan.lds_bytes;
    hipError_t e = hipSuccess;
    switch (plan.form) {
    case scrg::FORM_ROWS: e = scrg::launch_align(p.lanes_per_pair, a, n_waves, lds, c->stream); break;
    case scrg::FORM_ROWS_MW: e = scrg::launch_align_multiword(p.lanes_per_pair, a, n_waves, lds, c->stream); break;
    case scrg::FORM_LANE: e = lane_split ? scrg::launch_align_lane_split(a, n_waves, c->stream) : scrg::launch_align_lane(a, n_waves, lds, c->stream, out); break;
    case scrg::FORM_LANE_WIDE: e = scrg::launch_align_lane_wide(a, n_waves, lds, c->stream, out); break;
    case scrg::FORM_LANE_PARTS: e = scrg::launch_align_lane_parts(a, n_waves, lds, c->stream, out); break;
    case scrg::FORM_LANE_MW: e = scrg::launch_align_lane_mw(a, n_waves, lds, c->stream, out); break;
    }
    HIP_TRY(c, e);
    HIP_TRY(c, hipEventRecord(c->ev_stop, c->stream));
    c->have_timing = true;
    return SCRG_OK;
}

scrg_status scrg_align_device(scrg_ctx* c, const scrg_params* params, uint64_t n_pairs, const uint64_t* d_seq,
                              const scrg_pair_desc* d_pairs, scrg_run* d_runs, int64_t* d_edit_distance,
                              uint32_t* d_n_runs, uint32_t* d_pair_status)
{
    return align_device_impl(c, params, n_pairs, d_seq, d_pairs, d_runs, d_edit_distance, d_n_runs, d_pair_status, scrg::LANE_OUT_RUNS);
}

scrg_status scrg_align_device_edits(scrg_ctx* c, const scrg_params* params, uint64_t n_pairs, const uint64_t* d_seq,
                                    const scrg_pair_desc* d_pairs, uint8_t* d_streams, int64_t* d_edit_distance,
                                    uint32_t* d_stream_len, uint32_t* d_pair_status, uint32_t* d_n_runs)
{
    if (reinterpret_cast<uintptr_t>(d_streams) & 31u) return c ? c->fail(SCRG_ERR_INVALID_ARG, "d_streams needs 32-byte alignment") : SCRG_ERR_INVALID_ARG;
    return align_device_impl(c, params, n_pairs, d_seq, d_pairs, reinterpret_cast<scrg_run*>(d_streams), d_edit_distance,
                             d_stream_len, d_pair_status, scrg::LANE_OUT_EDITS, d_n_runs);
}

scrg_status scrg_align_device_distance(scrg_ctx* c, const scrg_params* params, uint64_t n_pairs, const uint64_t* d_seq,
                                       const scrg_pair_desc* d_pairs, int64_t* d_edit_distance, uint32_t* d_text_end,
                                       uint32_t* d_pair_status)
{
    return align_device_impl(c, params, n_pairs, d_seq, d_pairs, nullptr, d_edit_distance, nullptr, d_pair_status, scrg::LANE_OUT_NONE,
                             nullptr, d_text_end);
}

scrg_status scrg_last_kernel_ms(scrg_ctx* c, float* ms)
{
    if (!c || !ms) return SCRG_ERR_INVALID_ARG;
    *ms = 0.f;
    if (!c->have_timing) return SCRG_OK;
    HIP_TRY(c, hipEventSynchronize(c->ev_stop));
    HIP_TRY(c, hipEventElapsedTime(ms, c->ev_start, c->ev_stop));
    return SCRG_OK;
}

scrg_status scrg_debug_stats(scrg_ctx* c, uint64_t out[12])
{
    if (!c || !out) return SCRG_ERR_INVALID_ARG;
    memset(out, 0, 12 * sizeof(uint64_t));
    if (!scrg::SCRG_HAVE_STATS)
        return c->fail(SCRG_ERR_INVALID_ARG, "this library was built without -DSCRG_STATS: the kernels have no counters (scripts/ab.sh build stats -DSCRG_STATS)");
    if (!c->stats.p) return SCRG_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipMemcpy(out, c->stats.p, 12 * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return SCRG_OK;
}

scrg_status scrg_compact_runs(scrg_ctx* c, uint64_t n_pairs, const scrg_pair_desc* d_pairs, const scrg_run* d_runs,
                              const uint32_t* d_n_runs, const uint64_t* d_dense_offset, scrg_run* d_dense)
{
    if (!c) return SCRG_ERR_INVALID_ARG;
    if (n_pairs && (!d_pairs || !d_runs || !d_n_runs || !d_dense_offset || !d_dense))
        return c->fail(SCRG_ERR_INVALID_ARG, "null device pointer");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, scrg::launch_compact_runs(n_pairs, d_pairs, reinterpret_cast<const uint16_t*>(d_runs), d_n_runs,
                                         d_dense_offset, reinterpret_cast<uint16_t*>(d_dense), c->n_cus, c->stream));
    return SCRG_OK;
}

scrg_status scrg_select_best(scrg_ctx* c, uint64_t n_pairs, const uint32_t* d_group_key, const int64_t* d_edit_distance,
                             uint32_t* d_pair_status, uint32_t* d_n_runs, uint8_t* d_is_best)
{
    if (!c) return SCRG_ERR_INVALID_ARG;
    if (n_pairs && (!d_group_key || !d_edit_distance || !d_pair_status || !d_n_runs))
        return c->fail(SCRG_ERR_INVALID_ARG, "null device pointer");
    if (n_pairs > 0xffffffffull) return c->fail(SCRG_ERR_INVALID_ARG, "too many pairs");      // (a pair's index is half of its 64-bit value)
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, c->select_ws.ensure(scrg::select_scratch_bytes(n_pairs)));
    HIP_TRY(c, scrg::launch_select_best(n_pairs, d_group_key, 0xffffffffu, d_edit_distance, d_pair_status, d_n_runs, d_is_best,
                                        c->select_ws.p, c->stream));
    return SCRG_OK;
}

scrg_status scrg_select_mates_team(scrg_ctx* c, const scrg_mate_rule* rule, uint32_t team, uint64_t n_mates, const uint64_t* d_first,
                                   const uint64_t* d_start, const uint32_t* d_read_len, const uint8_t* d_reverse, const int64_t* d_edit_distance,
                                   uint32_t* d_pair_status, uint32_t* d_n_runs, uint8_t* d_is_best, scrg_mate_record* d_records)
{
    if (!c) return SCRG_ERR_INVALID_ARG;
    static const scrg_mate_rule any_fr = {0, ~0ull, SCRG_MATES_FR, 0, {0, 0}};
    if (!rule) rule = &any_fr;
    if (!scrg::mate_rule_valid(rule->min_span, rule->max_span, rule->orientation, rule->reserved[0], rule->reserved[1]))
        return c->fail(SCRG_ERR_INVALID_ARG, "mate rule: min_span <= max_span, orientation 0 .. 3 and zero reserved words are wanted");
    if (team != 0 && team != 4 && team != 8 && team != 16 && team != 32 && team != 64) return c->fail(SCRG_ERR_INVALID_ARG, "team: 0, 4, 8, 16, 32 or 64");
    if (n_mates && (!d_first || !d_start || !d_read_len || !d_edit_distance || !d_pair_status || !d_n_runs || !d_records))
        return c->fail(SCRG_ERR_INVALID_ARG, "null device pointer");
    if (n_mates > 0x7fffffffull) return c->fail(SCRG_ERR_INVALID_ARG, "too many mate pairs");
    HIP_TRY(c, hipSetDevice(c->device));
    uint32_t* word = nullptr;
    if (team == 0) {
        // a word per call, 64 of them in turn: calls enqueued on different streams of one handle do not share one
        constexpr uint32_t WORDS = 64;
        HIP_TRY(c, c->mate_ws.ensure(WORDS * sizeof(uint32_t)));
        word = c->mate_ws.as<uint32_t>() + (c->mate_calls++ % WORDS);
    }
    HIP_TRY(c, scrg::launch_select_mates(*rule, team, word, n_mates, d_first, d_start, d_read_len, d_reverse, d_edit_distance, d_pair_status, d_n_runs,
                                         d_is_best, d_records, c->stream));
    return SCRG_OK;
}

scrg_status scrg_select_mates(scrg_ctx* c, const scrg_mate_rule* rule, uint64_t n_mates, const uint64_t* d_first, const uint64_t* d_start,
                              const uint32_t* d_read_len, const uint8_t* d_reverse, const int64_t* d_edit_distance, uint32_t* d_pair_status,
                              uint32_t* d_n_runs, uint8_t* d_is_best, scrg_mate_record* d_records)
{
    return scrg_select_mates_team(c, rule, 0, n_mates, d_first, d_start, d_read_len, d_reverse, d_edit_distance, d_pair_status, d_n_runs, d_is_best, d_records);
}

scrg_status scrg_read_summary(scrg_ctx* c, const scrg_mapq_rule* rule, uint64_t n_reads, uint64_t n_pairs, const uint64_t* d_first,
                              const uint32_t* d_read_len, const int64_t* d_edit_distance, const uint32_t* d_pair_status, scrg_read_record* d_out,
                              uint32_t* d_keep_status)
{
    if (!c) return SCRG_ERR_INVALID_ARG;
    if (!rule) rule = &kMapqDefaults;
    if (!mapq_rule_ok(*rule)) return c->fail(SCRG_ERR_INVALID_ARG, kMapqRuleWanted);
    if (n_reads == 0) return SCRG_OK;
    if (!d_first || !d_out || (n_pairs && (!d_read_len || !d_edit_distance || !d_pair_status))) return c->fail(SCRG_ERR_INVALID_ARG, "null device pointer");
    if (d_keep_status && d_keep_status == d_pair_status) return c->fail(SCRG_ERR_INVALID_ARG, "d_keep_status is a copy: it cannot be d_pair_status itself");
    if (n_pairs > 0xffffffffull || n_reads > 0xffffffffull) return c->fail(SCRG_ERR_INVALID_ARG, "too many pairs");      // (a pair's index is half of its 64-bit value)
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, scrg::launch_read_summary(*rule, n_reads, n_pairs, d_first, d_read_len, d_edit_distance, d_pair_status, d_out, d_keep_status, c->stream));
    return SCRG_OK;
}

// the passes over finished alignments on device buffers (difference strings, report): the stride's check and the kernels'
// view of the arguments (p: the resolved parameters)
static scrg_status pair_runs_args(scrg_ctx* c, const scrg_params& p, uint64_t n_pairs, const uint64_t* d_seq, const scrg_pair_desc* d_pairs,
                                  const scrg_run* d_runs, const uint64_t* d_run_offset, uint64_t run_offset_stride, const uint32_t* d_n_runs,
                                  scrg::PairRuns* pr)
{
    if (run_offset_stride != 1 && run_offset_stride != 6)
        return c->fail(SCRG_ERR_INVALID_ARG, "run_offset_stride is 1 (a plain array) or 6 (&d_pairs[0].cigar_off)");
    *pr = scrg::PairRuns{n_pairs, d_seq, d_pairs, reinterpret_cast<const uint16_t*>(d_runs), d_run_offset, run_offset_stride, d_n_runs,
                         (uint32_t)std::max(1, p.text_stride_words), (uint32_t)std::max(1, p.read_stride_words), p.stranded ? 1u : 0u};
    return SCRG_OK;
}
// (difference strings: the parameters, the kind, then the above)
static scrg_status diff_device_args(scrg_ctx* c, const scrg_params* params, int32_t kind, uint64_t n_pairs, const uint64_t* d_seq,
                                    const scrg_pair_desc* d_pairs, const scrg_run* d_runs, const uint64_t* d_run_offset, uint64_t run_offset_stride,
                                    const uint32_t* d_n_runs, scrg::PairRuns* pr)
{
    scrg_params p;
    if (!resolve_params(params, &p)) return c->fail(SCRG_ERR_INVALID_ARG, g_params_error);
    if (kind != SCRG_DIFF_MD && kind != SCRG_DIFF_CS) return c->fail(SCRG_ERR_INVALID_ARG, "kind must be SCRG_DIFF_MD or SCRG_DIFF_CS");
    return pair_runs_args(c, p, n_pairs, d_seq, d_pairs, d_runs, d_run_offset, run_offset_stride, d_n_runs, pr);
}

scrg_status scrg_diff_lengths(scrg_ctx* c, const scrg_params* params, int32_t kind, uint64_t n_pairs, const uint64_t* d_seq,
                              const scrg_pair_desc* d_pairs, const scrg_run* d_runs, const uint64_t* d_run_offset, uint64_t run_offset_stride,
                              const uint32_t* d_n_runs, uint64_t* d_diff_len)
{
    if (!c) return SCRG_ERR_INVALID_ARG;
    scrg::PairRuns pr;
    const scrg_status s = diff_device_args(c, params, kind, n_pairs, d_seq, d_pairs, d_runs, d_run_offset, run_offset_stride, d_n_runs, &pr);
    if (s != SCRG_OK) return s;
    if (n_pairs && (!d_seq || !d_pairs || !d_runs || !d_run_offset || !d_n_runs || !d_diff_len)) return c->fail(SCRG_ERR_INVALID_ARG, "null device pointer");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, scrg::launch_diff_lengths(pr, kind, d_diff_len, c->n_cus, c->stream));
    return SCRG_OK;
}

scrg_status scrg_diff_render(scrg_ctx* c, const scrg_params* params, int32_t kind, uint64_t n_pairs, const uint64_t* d_seq,
                             const scrg_pair_desc* d_pairs, const scrg_run* d_runs, const uint64_t* d_run_offset, uint64_t run_offset_stride,
                             const uint32_t* d_n_runs, const uint64_t* d_diff_len, const uint64_t* d_diff_offset, char* d_diff_text,
                             uint64_t diff_capacity, uint32_t* d_bad_count)
{
    if (!c) return SCRG_ERR_INVALID_ARG;
    scrg::PairRuns pr;
    const scrg_status s = diff_device_args(c, params, kind, n_pairs, d_seq, d_pairs, d_runs, d_run_offset, run_offset_stride, d_n_runs, &pr);
    if (s != SCRG_OK) return s;
    if (!d_bad_count || (n_pairs && (!d_seq || !d_pairs || !d_runs || !d_run_offset || !d_n_runs || !d_diff_len || !d_diff_offset)) ||
        (diff_capacity && !d_diff_text))
        return c->fail(SCRG_ERR_INVALID_ARG, "null device pointer");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, scrg::launch_diff_render(pr, kind, d_diff_len, d_diff_offset, reinterpret_cast<uint8_t*>(d_diff_text), diff_capacity, d_bad_count, c->n_cus,
                                        c->stream));
    return SCRG_OK;
}

// (the CIGAR text in any form: the form's and the stride's check)
static scrg_status cigar_text_args(scrg_ctx* c, int32_t form, uint64_t run_offset_stride)
{
    if (!cigar_form_ok(form)) return c->fail(SCRG_ERR_INVALID_ARG, "form must be SCRG_CIGAR_WINDOWED, SCRG_CIGAR_MERGED or SCRG_CIGAR_M");
    if (run_offset_stride != 1 && run_offset_stride != 6)
        return c->fail(SCRG_ERR_INVALID_ARG, "run_offset_stride is 1 (a plain array) or 6 (&d_pairs[0].cigar_off)");
    return SCRG_OK;
}

scrg_status scrg_cigar_text_lengths(scrg_ctx* c, int32_t form, uint64_t n_pairs, const scrg_run* d_runs, const uint64_t* d_run_offset,
                                    uint64_t run_offset_stride, const uint32_t* d_n_runs, uint64_t* d_text_len)
{
    if (!c) return SCRG_ERR_INVALID_ARG;
    const scrg_status s = cigar_text_args(c, form, run_offset_stride);
    if (s != SCRG_OK) return s;
    if (n_pairs && (!d_runs || !d_run_offset || !d_n_runs || !d_text_len)) return c->fail(SCRG_ERR_INVALID_ARG, "null device pointer");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, scrg::launch_cigar_text_lengths(n_pairs, reinterpret_cast<const uint16_t*>(d_runs), d_run_offset, run_offset_stride, d_n_runs, form,
                                               d_text_len, c->n_cus, c->stream));
    return SCRG_OK;
}

scrg_status scrg_cigar_text_render(scrg_ctx* c, int32_t form, uint64_t n_pairs, const scrg_run* d_runs, const uint64_t* d_run_offset,
                                   uint64_t run_offset_stride, const uint32_t* d_n_runs, const uint64_t* d_text_len, const uint64_t* d_text_offset,
                                   char* d_text, uint64_t text_capacity, uint32_t* d_bad_count)
{
    if (!c) return SCRG_ERR_INVALID_ARG;
    const scrg_status s = cigar_text_args(c, form, run_offset_stride);
    if (s != SCRG_OK) return s;
    if (!d_bad_count || (n_pairs && (!d_runs || !d_run_offset || !d_n_runs || !d_text_len || !d_text_offset)) || (text_capacity && !d_text))
        return c->fail(SCRG_ERR_INVALID_ARG, "null device pointer");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, scrg::launch_cigar_text_render(n_pairs, reinterpret_cast<const uint16_t*>(d_runs), d_run_offset, run_offset_stride, d_n_runs, form,
                                              d_text_len, d_text_offset, reinterpret_cast<uint8_t*>(d_text), text_capacity, d_bad_count, c->n_cus,
                                              c->stream));
    return SCRG_OK;
}

scrg_status scrg_report_device(scrg_ctx* c, const scrg_params* params, uint64_t n_pairs, const uint64_t* d_seq, const scrg_pair_desc* d_pairs,
                               const scrg_run* d_runs, const uint64_t* d_run_offset, uint64_t run_offset_stride, const uint32_t* d_n_runs,
                               const int64_t* d_edit_distance, const uint32_t* d_pair_status, scrg_pair_report* d_report, uint32_t* d_fail_count)
{
    if (!c) return SCRG_ERR_INVALID_ARG;
    scrg_params p;
    if (!resolve_params(params, &p)) return c->fail(SCRG_ERR_INVALID_ARG, g_params_error);
    scrg::PairRuns pr;
    const scrg_status s = pair_runs_args(c, p, n_pairs, d_seq, d_pairs, d_runs, d_run_offset, run_offset_stride, d_n_runs, &pr);
    if (s != SCRG_OK) return s;
    if (n_pairs && (!d_seq || !d_pairs || !d_runs || !d_run_offset || !d_n_runs || !d_edit_distance || !d_report))
        return c->fail(SCRG_ERR_INVALID_ARG, "null device pointer");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, scrg::launch_report(pr, d_edit_distance, d_pair_status, c->text_strands ? 1u : 0u, d_report, d_fail_count,
                                   SCRG_SEL(p.reserved[0], scrg::SCRG_SWITCH_REPORT_PER_BASE), c->n_cus, c->stream));
    return SCRG_OK;
}

scrg_status scrg_clip_device(scrg_ctx* c, const scrg_params* params, uint64_t n_pairs, const scrg_run* d_runs, uint64_t* d_run_offset,
                             uint64_t run_offset_stride, uint32_t* d_n_runs, const uint32_t* d_pair_status, const int32_t* costs, int apply,
                             scrg_pair_clip* d_clip)
{
    if (!c) return SCRG_ERR_INVALID_ARG;
    scrg_params p;
    if (!resolve_params(params, &p)) return c->fail(SCRG_ERR_INVALID_ARG, g_params_error);
    if (run_offset_stride != 1 && run_offset_stride != 6)
        return c->fail(SCRG_ERR_INVALID_ARG, "run_offset_stride is 1 (a plain array) or 6 (&d_pairs[0].cigar_off)");
    static const int32_t usual[4] = {2, 4, 4, 2};
    if (!costs) costs = usual;
    if (!scrg_host::clip_costs_ok(costs)) return c->fail(SCRG_ERR_INVALID_ARG, "clip costs: match in 1..255, mismatch, gap_open and gap_extend in 0..255");
    if (n_pairs && (!d_runs || !d_run_offset || !d_n_runs || !d_clip)) return c->fail(SCRG_ERR_INVALID_ARG, "null device pointer");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, scrg::launch_clip(n_pairs, reinterpret_cast<const uint16_t*>(d_runs), d_run_offset, run_offset_stride, d_n_runs, d_pair_status, costs,
                                 apply != 0, d_clip, c->n_cus, c->stream));
    return SCRG_OK;
}

scrg_status scrg_pileup_add(scrg_ctx* c, const scrg_params* params, uint64_t n_pairs, const uint64_t* d_seq, const scrg_pair_desc* d_pairs,
                            const scrg_run* d_runs, const uint64_t* d_run_offset, uint64_t run_offset_stride, const uint32_t* d_n_runs,
                            const uint32_t* d_pair_status, const uint64_t* d_target_start, uint64_t target_len, uint32_t* d_acc, uint32_t* d_out_of_range)
{
    if (!c) return SCRG_ERR_INVALID_ARG;
    scrg_params p;
    if (!resolve_params(params, &p)) return c->fail(SCRG_ERR_INVALID_ARG, g_params_error);
    scrg::PairRuns pr;
    const scrg_status s = pair_runs_args(c, p, n_pairs, d_seq, d_pairs, d_runs, d_run_offset, run_offset_stride, d_n_runs, &pr);
    if (s != SCRG_OK) return s;
    if (c->text_strands) return c->fail(SCRG_ERR_INVALID_ARG, "the pileup takes forward texts only: the handle's text strands are on (scrg_ctx_set_text_strands)");
    if (target_len > UINT64_MAX / 64) return c->fail(SCRG_ERR_INVALID_ARG, "target_len too large");
    if (!d_acc || (n_pairs && (!d_seq || !d_pairs || !d_runs || !d_run_offset || !d_n_runs || !d_target_start)))
        return c->fail(SCRG_ERR_INVALID_ARG, "null device pointer");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, scrg::launch_pileup_add(pr, d_pair_status, d_target_start, target_len, d_acc, d_out_of_range, nullptr, c->n_cus, c->stream));
    return SCRG_OK;
}

scrg_status scrg_pileup_finish(scrg_ctx* c, uint64_t target_len, const uint32_t* d_acc, uint32_t* d_counts)
{
    if (!c) return SCRG_ERR_INVALID_ARG;
    if (!d_acc || !d_counts) return c->fail(SCRG_ERR_INVALID_ARG, "null device pointer");
    if (target_len >= 0x7fffffffull * 4096ull) return c->fail(SCRG_ERR_INVALID_ARG, "target_len too large");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, c->pile_ws.ensure(scrg::pileup_finish_scratch_bytes(target_len)));
    HIP_TRY(c, scrg::launch_pileup_finish(target_len, d_acc, d_counts, c->pile_ws.p, c->stream));
    return SCRG_OK;
}

size_t scrg_pileup_sites_scratch_bytes(uint64_t target_len)
{
    return target_len >= 0xffffffffull ? 0 : scrg::site_scratch_bytes(target_len);
}

static scrg_status site_args_check(scrg_ctx* c, uint64_t target_len, const uint32_t* d_counts, const uint64_t* d_seq, const void* d_scratch)
{
    if (target_len >= 0xffffffffull) return c->fail(SCRG_ERR_INVALID_ARG, "pileup sites have 32-bit offsets: target_len must be below 2^32 - 1");
    if (!d_scratch || (target_len && (!d_counts || !d_seq))) return c->fail(SCRG_ERR_INVALID_ARG, "null device pointer");
    if (reinterpret_cast<uintptr_t>(d_scratch) & 7u) return c->fail(SCRG_ERR_INVALID_ARG, "the site scratch must be 8-byte aligned");
    return SCRG_OK;
}

scrg_status scrg_pileup_sites_mark(scrg_ctx* c, uint64_t target_len, const uint32_t* d_counts, const uint64_t* d_seq, uint64_t genome_off,
                                   const scrg_site_rule* rule, void* d_scratch, uint64_t* d_n_sites)
{
    if (!c) return SCRG_ERR_INVALID_ARG;
    if (const char* why = site_rule_error(rule)) return c->fail(SCRG_ERR_INVALID_ARG, why);
    if (!d_n_sites) return c->fail(SCRG_ERR_INVALID_ARG, "null device pointer");
    const scrg_status s = site_args_check(c, target_len, d_counts, d_seq, d_scratch);
    if (s != SCRG_OK) return s;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, scrg::launch_site_mark(target_len, d_counts, d_seq, genome_off, *rule, d_scratch, d_n_sites, c->stream));
    return SCRG_OK;
}

scrg_status scrg_pileup_sites_write(scrg_ctx* c, uint64_t target_len, const uint32_t* d_counts, const uint64_t* d_seq, uint64_t genome_off, void* d_scratch,
                                    uint64_t cap, scrg_site* d_sites)
{
    if (!c) return SCRG_ERR_INVALID_ARG;
    const scrg_status s = site_args_check(c, target_len, d_counts, d_seq, d_scratch);
    if (s != SCRG_OK) return s;
    if (cap && !d_sites) return c->fail(SCRG_ERR_INVALID_ARG, "null device pointer");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, scrg::launch_site_write(target_len, d_counts, d_seq, genome_off, d_scratch, cap, d_sites, c->stream));
    return SCRG_OK;
}

scrg_status scrg_compact_runs_packed(scrg_ctx* c, const scrg_params* params, uint64_t n_pairs, const scrg_pair_desc* d_pairs,
                                     const scrg_run* d_runs, const uint32_t* d_n_runs, const uint64_t* d_dense_offset,
                                     uint8_t* d_packed)
{
    if (!c) return SCRG_ERR_INVALID_ARG;
    scrg_params p;
    if (!resolve_params(params, &p)) return c->fail(SCRG_ERR_INVALID_ARG, g_params_error);
    if (p.W - p.O > 63) return c->fail(SCRG_ERR_INVALID_ARG, "packed runs hold counts up to 63: W-O must be <= 63");
    if (n_pairs && (!d_pairs || !d_runs || !d_n_runs || !d_dense_offset || !d_packed))
        return c->fail(SCRG_ERR_INVALID_ARG, "null device pointer");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, scrg::launch_compact_runs_packed(n_pairs, d_pairs, reinterpret_cast<const uint16_t*>(d_runs), d_n_runs,
                                                d_dense_offset, d_packed, c->n_cus, c->stream));
    return SCRG_OK;
}

scrg_status scrg_unpack_runs(scrg_ctx* c, uint64_t n_runs, const uint8_t* d_packed, scrg_run* d_runs)
{
    if (!c) return SCRG_ERR_INVALID_ARG;
    if (n_runs && (!d_packed || !d_runs)) return c->fail(SCRG_ERR_INVALID_ARG, "null device pointer");
    if ((reinterpret_cast<uintptr_t>(d_packed) & 3u) || (reinterpret_cast<uintptr_t>(d_runs) & 7u))
        return c->fail(SCRG_ERR_INVALID_ARG, "packed runs need 4-byte, runs 8-byte alignment");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, scrg::launch_unpack_runs(n_runs, d_packed, reinterpret_cast<uint16_t*>(d_runs), c->n_cus, c->stream));
    return SCRG_OK;
}

scrg_status scrg_encode_edit_stream(scrg_ctx* c, const scrg_params* params, uint64_t n_pairs, const scrg_pair_desc* d_pairs,
                                    const scrg_run* d_runs, const uint32_t* d_n_runs, uint8_t* d_stream, uint64_t stream_cap,
                                    uint64_t* d_stream_off, uint32_t* d_stream_len, uint64_t* d_total)
{
    if (!c) return SCRG_ERR_INVALID_ARG;
    scrg_params p;
    if (!resolve_params(params, &p)) return c->fail(SCRG_ERR_INVALID_ARG, g_params_error);
    if (!d_total) return c->fail(SCRG_ERR_INVALID_ARG, "d_total is required");
    if (n_pairs && (!d_pairs || !d_runs || !d_n_runs || !d_stream_off || !d_stream_len || (stream_cap && !d_stream)))
        return c->fail(SCRG_ERR_INVALID_ARG, "null device pointer");
    if (reinterpret_cast<uintptr_t>(d_stream) & 3u) return c->fail(SCRG_ERR_INVALID_ARG, "d_stream needs 4-byte alignment");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, scrg::launch_encode_edits(n_pairs, (uint32_t)p.W, (uint32_t)p.O, d_pairs, reinterpret_cast<const uint16_t*>(d_runs), d_n_runs, d_stream,
                                         stream_cap, d_stream_off, d_stream_len, d_total, c->stream));
    return SCRG_OK;
}

scrg_status scrg_decode_edit_stream(scrg_ctx* c, const scrg_params* params, uint64_t n_pairs, const uint8_t* d_stream,
                                    uint64_t stream_bytes, const uint64_t* d_stream_off, const uint32_t* d_stream_len,
                                    const uint64_t* d_read_len, uint64_t read_len_stride, const uint64_t* d_dense_offset,
                                    scrg_run* d_dense, uint64_t dense_capacity, uint32_t* d_n_runs, uint32_t* d_bad_count)
{
    if (!c) return SCRG_ERR_INVALID_ARG;
    scrg_params p;
    if (!resolve_params(params, &p)) return c->fail(SCRG_ERR_INVALID_ARG, g_params_error);
    if (!d_bad_count || (n_pairs && (!d_stream_off || !d_stream_len || !d_read_len || !d_n_runs)) || (stream_bytes && !d_stream))
        return c->fail(SCRG_ERR_INVALID_ARG, "null device pointer");
    if (d_dense && !d_dense_offset) return c->fail(SCRG_ERR_INVALID_ARG, "d_dense needs d_dense_offset");
    // streams are fetched in aligned 16-byte blocks, runs leave in aligned 16-byte stores
    if ((reinterpret_cast<uintptr_t>(d_stream) & 15u) || (reinterpret_cast<uintptr_t>(d_dense) & 15u))
        return c->fail(SCRG_ERR_INVALID_ARG, "d_stream and d_dense need 16-byte alignment");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, scrg::launch_decode_edits(n_pairs, d_stream, stream_bytes, d_stream_off, d_stream_len,
                                         d_read_len, read_len_stride, d_dense_offset, reinterpret_cast<uint16_t*>(d_dense), dense_capacity,
                                         d_n_runs, d_bad_count, c->stream));
    return SCRG_OK;
}

// The device decoder's per-lane state machine (edit_stream.h: decode_lane_step, the code decode_edits_kernel runs in
// every lane) on the host, for ONE pair: same arguments as scrg_edit_stream_to_runs, same runs; like the device it does
// not look at the window geometry.  Exists so that the state machine can be checked without a GPU (tests/test_edit_stream.py).
scrg_status scrg_edit_stream_to_runs_lane(const scrg_params* params, uint64_t read_len, const uint8_t* stream, uint64_t n_bytes,
                                          scrg_run* runs, uint64_t runs_cap, uint64_t* n_runs)
{
    scrg_params p;
    if (!n_runs || (n_bytes && !stream) || (runs_cap && !runs) || !resolve_params(params, &p)) return SCRG_ERR_INVALID_ARG;
    *n_runs = 0;
    if (read_len > 0x7fffffffull || n_bytes > 0x3fffffffull) return SCRG_ERR_INVALID_ARG;
    scrg::DecodeLane s;
    scrg::decode_lane_init(s, 0u);
    for (uint64_t k = 0; k < n_bytes; k++) {
        scrg::decode_lane_step(s, (uint32_t)stream[k], [&](uint32_t at, uint32_t word) {         // at: byte offset of the run's slot
            if ((at >> 1) < runs_cap) { runs[at >> 1].count = (uint8_t)word; runs[at >> 1].op = (char)(word >> 8); }
        });
        if ((k & 15u) == 15u) scrg::decode_lane_guard(s);
    }
    if (read_len > 0x7fffffffull) return SCRG_ERR_INVALID_ARG;
    if (!scrg::decode_lane_clean(s, n_bytes ? (uint32_t)stream[n_bytes - 1] : 0u, (uint32_t)read_len)) return SCRG_ERR_INVALID_ARG;
    *n_runs = scrg::decode_lane_runs(s);
    return *n_runs > runs_cap ? SCRG_ERR_CIGAR_OVERFLOW : SCRG_OK;
}

scrg_status scrg_edit_stream_to_runs(const scrg_params* params, uint64_t read_len, const uint8_t* stream, uint64_t n_bytes,
                                     scrg_run* runs, uint64_t runs_cap, uint64_t* n_runs)
{
    scrg_params p;
    if (!n_runs || (n_bytes && !stream) || (runs_cap && !runs) || !resolve_params(params, &p)) return SCRG_ERR_INVALID_ARG;
    uint64_t k = 0;
    const uint64_t n = scrg::replay_edit_stream(stream, n_bytes, read_len, (uint32_t)(p.W - p.O),
                                                [&](uint32_t op, uint64_t t) {
                                                    if (k < runs_cap) { runs[k].count = (uint8_t)t; runs[k].op = (char)op; }
                                                    k++;
                                                });
    *n_runs = n == ~0ull ? 0 : n;
    if (n == ~0ull) return SCRG_ERR_INVALID_ARG;
    return n > runs_cap ? SCRG_ERR_CIGAR_OVERFLOW : SCRG_OK;
}

scrg_status scrg_runs_to_edit_stream(const scrg_params* params, const scrg_run* runs, uint64_t n_runs, uint8_t* stream,
                                     uint64_t stream_cap, uint64_t* n_bytes)
{
    scrg_params p;
    if (!n_bytes || (n_runs && !runs) || (stream_cap && !stream) || !resolve_params(params, &p)) return SCRG_ERR_INVALID_ARG;
    uint64_t k = 0;
    const uint64_t n = scrg::encode_runs(n_runs, (uint32_t)(p.W - p.O),
                                         [&](uint64_t r) { return (uint32_t)runs[r].count | (uint32_t)(uint8_t)runs[r].op << 8; },
                                         [&](uint8_t b) {
                                             if (k < stream_cap) stream[k] = b;
                                             k++;
                                         });
    *n_bytes = n == ~0ull ? 0 : n;
    if (n == ~0ull) return SCRG_ERR_INVALID_ARG;
    return n > stream_cap ? SCRG_ERR_CIGAR_OVERFLOW : SCRG_OK;
}

scrg_status scrg_ascii_to_twobit(scrg_ctx* c, uint64_t count, const uint64_t* d_lens, const uint64_t* d_ascii_off,
                                 const char* d_ascii, const uint64_t* d_twobit_off, uint8_t* d_twobit,
                                 uint32_t* d_bad_count)
{
    if (!c || !d_bad_count) return SCRG_ERR_INVALID_ARG;
    if (count && (!d_lens || !d_ascii_off || !d_ascii || !d_twobit_off || !d_twobit))
        return c->fail(SCRG_ERR_INVALID_ARG, "null device pointer");
    HIP_TRY(c, hipSetDevice(c->device));
    // the grid's x extent only needs an upper bound on the string length; take it from the
    // device array without a sync by assuming long strings (extra blocks exit immediately)
    HIP_TRY(c, scrg::launch_ascii_to_twobit(count, d_lens, d_ascii_off, d_ascii, d_twobit_off, d_twobit, d_bad_count,
                                            1 << 16, c->stream));
    return SCRG_OK;
}

// ---------------------------------------------------------------------------
// host-pointer entry points
// ---------------------------------------------------------------------------
void scrg_result_pool_trim(void)
{
    g_pool.trim();
    g_diff_pool.trim();
}

void scrg_result_free(scrg_result* r)
{
    if (!r) return;
    g_pool.put(r->edit_distance);
    g_pool.put(r->pair_status);
    g_pool.put(r->run_offset);
    g_pool.put(r->runs);
    g_pool.put(r->cigar_offset);
    g_pool.put(r->cigar_text);
    g_pool.put(r->text_end);
    free(r);
}

}  // extern "C"

// ---------------------------------------------------------------------------
// host-pointer entry points: thin argument checks in front of the pipeline of scrg_host.cpp
// ---------------------------------------------------------------------------
namespace {

std::mutex g_multi_mu;
std::vector<std::pair<int, void*>> g_multi_states;       // (device, state), in the order they were first asked for
std::vector<char> g_multi_busy;

// (every host align call begins with c->kept.reset(): the side results of the call before it that nobody took are dropped)

void* ctx_state(scrg_ctx* c)
{
    if (!c->host_state) c->host_state = scrg_host::state_create(c->device);
    return c->host_state;
}

// checks and the pair -> read table shared by the mapping entry points
scrg_status mapping_batch(uint64_t n_reads, const char* const* reads, const uint64_t* read_lens, const uint64_t* cand_offsets,
                          const uint64_t* cand_start, const uint8_t* cand_reverse, scrg_host::Batch* b, std::vector<uint32_t>* pair_read,
                          std::string* err, bool plan_only = false)
{
    // (plan_only: a batch that is only planned has lengths and counts, no sequences and no starts)
    if ((n_reads && ((!reads && !plan_only) || !read_lens)) || !cand_offsets) { *err = "null input array"; return SCRG_ERR_INVALID_ARG; }
    const uint64_t n_pairs = cand_offsets[n_reads];
    if (n_pairs > kMaxPairsPerLaunch || n_reads > 0xfffffff0ull) { *err = "too many pairs"; return SCRG_ERR_INVALID_ARG; }
    if (n_pairs && !cand_start && !plan_only) { *err = "null candidate array"; return SCRG_ERR_INVALID_ARG; }
    for (uint64_t r = 0; r < n_reads; r++) {
        if (!plan_only && read_lens[r] && !reads[r]) { *err = "null read pointer"; return SCRG_ERR_INVALID_ARG; }
        if (read_lens[r] > 0x7fffffffull) { *err = "read longer than 2^31-1"; return SCRG_ERR_INVALID_ARG; }
        if (cand_offsets[r + 1] < cand_offsets[r]) { *err = "cand_offsets not monotone"; return SCRG_ERR_INVALID_ARG; }
    }
    pair_read->resize(n_pairs);
    parallel_for(n_reads, [&](uint64_t r) {
        for (uint64_t k = cand_offsets[r]; k < cand_offsets[r + 1]; k++) (*pair_read)[k] = (uint32_t)r;
    });
    b->n_pairs = n_pairs;
    b->mapping = true;
    b->reads = reads;
    b->read_lens = read_lens;
    b->cand_start = cand_start;
    b->cand_reverse = cand_reverse;
    b->pair_read = pair_read->data();
    b->cand_offsets = cand_offsets;
    b->n_reads = n_reads;
    return SCRG_OK;
}

scrg_status pairs_batch(const scrg_params* params, uint64_t n_pairs, const char* const* texts, const uint64_t* text_lens, const char* const* queries,
                        const uint64_t* query_lens, scrg_host::Batch* b, std::string* err)
{
    if (params && params->outputs >= 0 && (params->outputs & SCRG_OUT_BEST)) {
        *err = "SCRG_OUT_BEST needs reads with candidates: the mapping calls have them, pairs do not";
        return SCRG_ERR_INVALID_ARG;
    }
    if (n_pairs && (!texts || !text_lens || !queries || !query_lens)) { *err = "null input array"; return SCRG_ERR_INVALID_ARG; }
    if (n_pairs > kMaxPairsPerLaunch) { *err = "too many pairs"; return SCRG_ERR_INVALID_ARG; }
    for (uint64_t i = 0; i < n_pairs; i++) {
        if ((text_lens[i] && !texts[i]) || (query_lens[i] && !queries[i])) { *err = "null sequence pointer"; return SCRG_ERR_INVALID_ARG; }
        if (query_lens[i] > 0x7fffffffull) { *err = "read longer than 2^31-1"; return SCRG_ERR_INVALID_ARG; }
    }
    b->n_pairs = n_pairs;
    b->mapping = false;
    b->texts = texts;
    b->text_lens = text_lens;
    b->reads = queries;
    b->read_lens = query_lens;
    return SCRG_OK;
}

// A call on a handle: its options and its side results travel with it.  (align() fills c->kept only when it delivers a result, and
// every entry point emptied it on the way in: a call that delivers none keeps nothing.  The pileup accumulator outlives calls: one
// that fails with anything other than SCRG_ERR_CIGAR_OVERFLOW — a refusal included — discards it, so that what is taken later is
// never the sum of calls of which one is missing.)
scrg_status ctx_align(scrg_ctx* c, const scrg_params* params, scrg_host::Batch& b, scrg_result** out)
{
    auto checked = [&]() -> scrg_status {
        scrg_params p;
        if (!resolve_params(params, &p)) return c->fail(SCRG_ERR_INVALID_ARG, g_params_error);
        void* st = ctx_state(c);
        if (!st) return c->fail(SCRG_ERR_NO_DEVICE, "no usable HIP device for the host path");
        std::string err;
        const scrg_status s = scrg_host::align(&st, 1, p, b, c->opt, c->text_strands, out, &c->kept, &err);
        if (s != SCRG_OK) c->fail(s, err.c_str());
        return s;
    };
    const scrg_status s = checked();
    if (c->opt.pileup && s != SCRG_OK && s != SCRG_ERR_CIGAR_OVERFLOW && c->host_state) scrg_host::pileup_discard(c->host_state, false);
    return s;
}

// the states of a multi-device call: one per listed device (a device listed twice gets two), kept for later calls
scrg_status multi_states(const int32_t* devices, int32_t n_devices, std::vector<void*>* st, std::vector<size_t>* taken)
{
    std::lock_guard<std::mutex> g(g_multi_mu);
    for (int32_t d = 0; d < n_devices; d++) {
        size_t found = g_multi_states.size();
        for (size_t k = 0; k < g_multi_states.size(); k++)
            if (g_multi_states[k].first == devices[d] && !g_multi_busy[k]) { found = k; break; }
        if (found == g_multi_states.size()) {
            void* s = scrg_host::state_create(devices[d]);
            if (!s) {
                for (size_t k : *taken) g_multi_busy[k] = 0;
                return SCRG_ERR_NO_DEVICE;
            }
            g_multi_states.emplace_back(devices[d], s);
            g_multi_busy.push_back(0);
        }
        g_multi_busy[found] = 1;
        taken->push_back(found);
        st->push_back(g_multi_states[found].second);
    }
    return SCRG_OK;
}

void multi_done(const std::vector<size_t>& taken)
{
    std::lock_guard<std::mutex> g(g_multi_mu);
    for (size_t k : taken) g_multi_busy[k] = 0;
}

scrg_status multi_align(const int32_t* devices, int32_t n_devices, const scrg_params* params, scrg_host::Batch& b, scrg_result** out)
{
    scrg_params p;
    if (!resolve_params(params, &p)) { g_multi_error = g_params_error; return SCRG_ERR_INVALID_ARG; }
    std::vector<void*> st;
    std::vector<size_t> taken;
    scrg_status s = multi_states(devices, n_devices, &st, &taken);
    if (s != SCRG_OK) { g_multi_error = "no usable HIP device"; return s; }
    std::string err;
    s = scrg_host::align(st.data(), (int)st.size(), p, b, scrg_host::CallOptions{}, false, out, nullptr, &err);
    multi_done(taken);
    g_multi_error = s == SCRG_OK ? "" : err;
    return s;
}

}  // namespace

extern "C" {

scrg_status scrg_align_pairs(scrg_ctx* c, const scrg_params* params, uint64_t n_pairs, const char* const* texts,
                             const uint64_t* text_lens, const char* const* queries, const uint64_t* query_lens,
                             scrg_result** out)
{
    if (!c || !out) return SCRG_ERR_INVALID_ARG;
    *out = nullptr;
    c->kept.reset();
    return guarded(c, [&] {
        scrg_host::Batch b;
        std::string err;
        scrg_status s = pairs_batch(params, n_pairs, texts, text_lens, queries, query_lens, &b, &err);
        if (s != SCRG_OK) return c->fail(s, err.c_str());
        return ctx_align(c, params, b, out);
    });
}

scrg_status scrg_align_mapping_stranded(scrg_ctx* c, const scrg_params* params, const char* genome,
                                        uint64_t genome_len, uint64_t n_reads, const char* const* reads,
                                        const uint64_t* read_lens, const uint64_t* cand_offsets,
                                        const uint64_t* cand_start, const uint8_t* cand_reverse, scrg_result** out)
{
    if (!c || !out) return SCRG_ERR_INVALID_ARG;
    *out = nullptr;
    c->kept.reset();
    return guarded(c, [&] {
        if (genome_len && !genome) return c->fail(SCRG_ERR_INVALID_ARG, "null input array");
        scrg_host::Batch b;
        std::vector<uint32_t> pair_read;
        std::string err;
        scrg_status s = mapping_batch(n_reads, reads, read_lens, cand_offsets, cand_start, cand_reverse, &b, &pair_read, &err);
        if (s != SCRG_OK) return c->fail(s, err.c_str());
        static const char empty_genome[1] = {0};
        b.genome = genome ? genome : empty_genome;          // (the genome is staged by this call, as the reference re-converts it, genasm_cpu.cpp:508)
        b.genome_len = genome_len;
        return ctx_align(c, params, b, out);
    });
}

scrg_status scrg_align_mapping(scrg_ctx* c, const scrg_params* params, const char* genome, uint64_t genome_len,
                               uint64_t n_reads, const char* const* reads, const uint64_t* read_lens,
                               const uint64_t* cand_offsets, const uint64_t* cand_start, scrg_result** out)
{
    return scrg_align_mapping_stranded(c, params, genome, genome_len, n_reads, reads, read_lens, cand_offsets,
                                       cand_start, nullptr, out);
}

// scrg_genome_set: pack (host threads) and transfer a genome once; it stays at the front of the handle's sequence
// array until another genome is set or scrg_genome_clear() is called.
scrg_status scrg_genome_set(scrg_ctx* c, const char* genome, uint64_t genome_len)
{
    if (!c || (genome_len && !genome)) return SCRG_ERR_INVALID_ARG;
    return guarded(c, [&] {
        void* st = ctx_state(c);
        if (!st) return c->fail(SCRG_ERR_NO_DEVICE, "no usable HIP device for the host path");
        std::string err;
        static const char empty_genome[1] = {0};
        const scrg_status s = scrg_host::genome_set(st, genome ? genome : empty_genome, genome_len, &err);
        if (s != SCRG_OK) c->fail(s, err.c_str());
        return s;
    });
}

void scrg_genome_clear(scrg_ctx* c)
{
    if (c && c->host_state) scrg_host::genome_clear(c->host_state);
}

// ---- seeding: the index of the resident genome and the reads' candidates (seed_rule.h, seed_kernels.hip, scrg_host.cpp) ----
void scrg_seed_rule_default(scrg_seed_rule* rule)
{
    if (rule) *rule = scrg_seed_rule{13, 4, 64, 32, 2, 4, 3, 0};
}

scrg_status scrg_seed_rule_check(const scrg_seed_rule* r, uint64_t genome_len)
{
    if (!r || !scrg::seed_rule_valid(r->k, r->stride, r->max_occ, r->band, r->min_hits, r->max_candidates, r->strands)) return SCRG_ERR_INVALID_ARG;
    return genome_len <= scrg::SEED_MAX_GENOME && scrg::seed_index_entries(genome_len, r->k, r->stride) <= scrg::SEED_MAX_ENTRIES ? SCRG_OK : SCRG_ERR_INVALID_ARG;
}

scrg_status scrg_ctx_set_seed_sampling(scrg_ctx* c, uint32_t smer)
{
    if (!c) return SCRG_ERR_INVALID_ARG;
    if (!scrg::seed_smer_valid(smer, 16)) return c->fail(SCRG_ERR_INVALID_ARG, "seed sampling: smer is 0 (off) or 3 .. 15");
    c->seed_smer = smer;
    return SCRG_OK;
}

int scrg_seed_key_selected(uint32_t key, uint32_t k, uint32_t smer)
{
    if (k < 8u || k > 16u || !scrg::seed_smer_valid(smer, k)) return 0;
    return scrg::seed_key_selected(k < 16u ? key & ((1u << (2u * k)) - 1u) : key, k, smer) ? 1 : 0;
}

scrg_status scrg_seed_sampling_info(scrg_ctx* c, uint32_t* smer, uint64_t* n_positions, uint64_t* last_n_lookups)
{
    if (!c) return SCRG_ERR_INVALID_ARG;
    if (!c->host_state || !scrg_host::seed_sampling_info(c->host_state, smer, n_positions, last_n_lookups))
        return c->fail(SCRG_ERR_INVALID_ARG, "no genome index: call scrg_genome_index first");
    return SCRG_OK;
}

scrg_status scrg_genome_index(scrg_ctx* c, const scrg_seed_rule* rule)
{
    if (!c) return SCRG_ERR_INVALID_ARG;
    return guarded(c, [&] {
        if (!c->host_state || !scrg_host::genome_resident(c->host_state, nullptr))
            return c->fail(SCRG_ERR_INVALID_ARG, "no resident genome: call scrg_genome_set first");
        scrg_seed_rule k;
        scrg_seed_rule_default(&k);
        if (rule) k = *rule;
        std::string err;
        const scrg_status s = scrg_host::genome_index(c->host_state, k, c->seed_smer, &err);
        if (s != SCRG_OK) c->fail(s, err.c_str());
        return s;
    });
}

void scrg_genome_index_clear(scrg_ctx* c)
{
    if (c && c->host_state) scrg_host::genome_index_clear(c->host_state);
}

scrg_status scrg_genome_index_info(scrg_ctx* c, scrg_seed_rule* rule, uint64_t* n_entries, uint64_t* device_bytes)
{
    if (!c) return SCRG_ERR_INVALID_ARG;
    if (!c->host_state || !scrg_host::genome_index_info(c->host_state, rule, n_entries, device_bytes))
        return c->fail(SCRG_ERR_INVALID_ARG, "no genome index: call scrg_genome_index first");
    return SCRG_OK;
}

void scrg_candidates_free(scrg_candidates* x)
{
    if (!x) return;
    free(x->cand_offsets);
    free(x->cand_start);
    free(x->cand_reverse);
    free(x->cand_votes);
    free(x);
}

scrg_status scrg_find_candidates(scrg_ctx* c, uint64_t n_reads, const char* const* reads, const uint64_t* read_lens, scrg_candidates** out)
{
    if (!c || !out) return SCRG_ERR_INVALID_ARG;
    *out = nullptr;
    return guarded(c, [&] {
        if (!c->host_state) return c->fail(SCRG_ERR_INVALID_ARG, "no genome index: call scrg_genome_set and scrg_genome_index first");
        std::string err;
        const scrg_status s = scrg_host::find_candidates(c->host_state, n_reads, reads, read_lens, out, &err);
        if (s != SCRG_OK) c->fail(s, err.c_str());
        return s;
    });
}

scrg_status scrg_align_mapping_resident(scrg_ctx* c, const scrg_params* params, uint64_t n_reads, const char* const* reads,
                                        const uint64_t* read_lens, const uint64_t* cand_offsets, const uint64_t* cand_start,
                                        const uint8_t* cand_reverse, scrg_result** out)
{
    if (!c || !out) return SCRG_ERR_INVALID_ARG;
    *out = nullptr;
    c->kept.reset();
    return guarded(c, [&] {
        if (!c->host_state || !scrg_host::genome_resident(c->host_state, nullptr))
            return c->fail(SCRG_ERR_INVALID_ARG, "no resident genome: call scrg_genome_set first");
        scrg_host::Batch b;
        std::vector<uint32_t> pair_read;
        std::string err;
        scrg_status s = mapping_batch(n_reads, reads, read_lens, cand_offsets, cand_start, cand_reverse, &b, &pair_read, &err);
        if (s != SCRG_OK) return c->fail(s, err.c_str());
        b.genome = nullptr;                                  // the resident one
        return ctx_align(c, params, b, out);
    });
}

void scrg_mates_free(scrg_mates* m)
{
    if (!m) return;
    free(m->records);
    free(m);
}

scrg_status scrg_align_mapping_paired(scrg_ctx* c, const scrg_params* params, uint64_t n_reads, const char* const* reads, const uint64_t* read_lens,
                                      const uint64_t* cand_offsets, const uint64_t* cand_start, const uint8_t* cand_reverse, const scrg_mate_rule* rule,
                                      scrg_mates** mates, scrg_result** out)
{
    if (mates) *mates = nullptr;
    if (out) *out = nullptr;
    if (!c || !out || !mates) return SCRG_ERR_INVALID_ARG;
    c->kept.reset();
    return guarded(c, [&] {
        if (!c->host_state || !scrg_host::genome_resident(c->host_state, nullptr))
            return c->fail(SCRG_ERR_INVALID_ARG, "no resident genome: call scrg_genome_set first");
        scrg_host::Batch b;
        std::vector<uint32_t> pair_read;
        std::string err;
        scrg_status s = mapping_batch(n_reads, reads, read_lens, cand_offsets, cand_start, cand_reverse, &b, &pair_read, &err);
        if (s != SCRG_OK) return c->fail(s, err.c_str());
        static const scrg_mate_rule any_fr = {0, ~0ull, SCRG_MATES_FR, 0, {0, 0}};
        b.mate_rule = rule ? rule : &any_fr;
        b.genome = nullptr;                                  // the resident one
        s = ctx_align(c, params, b, out);
        *mates = std::exchange(c->kept.mates, nullptr);      // (set only when *out is)
        return s;
    });
}

scrg_status scrg_align_mapping_directed(scrg_ctx* c, const scrg_params* params, uint64_t n_reads, const char* const* reads,
                                        const uint64_t* read_lens, const uint64_t* cand_offsets, const uint64_t* cand_start,
                                        const uint8_t* cand_reverse, const uint8_t* cand_leftward, scrg_result** out)
{
    if (!c || !out) return SCRG_ERR_INVALID_ARG;
    *out = nullptr;
    c->kept.reset();
    return guarded(c, [&] {
        if (!c->host_state || !scrg_host::genome_resident(c->host_state, nullptr))
            return c->fail(SCRG_ERR_INVALID_ARG, "no resident genome: call scrg_genome_set first");
        scrg_host::Batch b;
        std::vector<uint32_t> pair_read;
        std::string err;
        scrg_status s = mapping_batch(n_reads, reads, read_lens, cand_offsets, cand_start, cand_reverse, &b, &pair_read, &err);
        if (s != SCRG_OK) return c->fail(s, err.c_str());
        // (no candidate leftward: exactly the resident call, whatever lanes_per_pair is)
        bool any_left = false;
        for (uint64_t p = 0; cand_leftward && p < b.n_pairs && !any_left; p++) any_left = cand_leftward[p] != 0;
        b.cand_leftward = any_left ? cand_leftward : nullptr;
        b.genome = nullptr;                                  // the resident one
        return ctx_align(c, params, b, out);
    });
}

scrg_status scrg_join_anchored_runs(const scrg_run* left, uint64_t n_left, const scrg_run* right, uint64_t n_right, scrg_run* runs,
                                    uint64_t runs_cap, uint64_t* n_runs, uint64_t* left_text)
{
    if ((n_left && !left) || (n_right && !right) || !n_runs || (runs_cap && !runs) || n_left > UINT64_MAX - n_right) return SCRG_ERR_INVALID_ARG;
    uint64_t consumed = 0;
    for (uint64_t k = 0; k < n_left; k++) {
        const char op = left[k].op;
        if (op != '=' && op != 'X' && op != 'I' && op != 'D') return SCRG_ERR_INVALID_ARG;
        if (op != 'I') consumed += left[k].count;
    }
    for (uint64_t k = 0; k < n_right; k++) {
        const char op = right[k].op;
        if (op != '=' && op != 'X' && op != 'I' && op != 'D') return SCRG_ERR_INVALID_ARG;
    }
    *n_runs = n_left + n_right;
    if (left_text) *left_text = consumed;
    if (*n_runs > runs_cap) return SCRG_ERR_CIGAR_OVERFLOW;
    for (uint64_t k = 0; k < n_left; k++) runs[k] = left[n_left - 1 - k];
    for (uint64_t k = 0; k < n_right; k++) runs[n_left + k] = right[k];
    return SCRG_OK;
}

scrg_status scrg_align_mapping_anchored(scrg_ctx* c, const scrg_params* params, uint64_t n_reads, const char* const* reads,
                                        const uint64_t* read_lens, const uint64_t* cand_offsets, const uint64_t* anchor_genome,
                                        const uint64_t* anchor_read, const uint8_t* cand_reverse, uint64_t* text_start, scrg_result** out)
{
    if (!c || !out) return SCRG_ERR_INVALID_ARG;
    *out = nullptr;
    c->kept.reset();
    return guarded(c, [&] {
        const int64_t t_begin = now_ns();
        scrg_params p;
        if (!resolve_params(params, &p)) return c->fail(SCRG_ERR_INVALID_ARG, g_params_error);
        if (p.outputs & SCRG_OUT_BEST)
            return c->fail(SCRG_ERR_INVALID_ARG, "anchored alignment has no best-candidate mode: the halves of a pair are aligned apart");
        if (c->opt.has_edit_limit())
            return c->fail(SCRG_ERR_INVALID_ARG, "anchored alignment takes no edit limit: a limit per half is not a limit per read");
        if (c->opt.diff_kind != SCRG_DIFF_OFF)
            return c->fail(SCRG_ERR_INVALID_ARG, "difference strings of joined pairs are not made on the device (scrg_ctx_set_diff; scrg_diff_from_runs)");
        if (c->opt.report)
            return c->fail(SCRG_ERR_INVALID_ARG, "the alignment report of joined pairs is not made on the device (scrg_ctx_set_report; scrg_report_from_runs)");
        if (c->opt.clip)
            return c->fail(SCRG_ERR_INVALID_ARG, "joined pairs are not clipped on the device yet (scrg_ctx_set_clip; scrg_clip_from_runs)");
        if (c->opt.pileup) {
            if (c->host_state) scrg_host::pileup_discard(c->host_state, false);
            return c->fail(SCRG_ERR_INVALID_ARG, "joined pairs do not pile up on the device yet (scrg_ctx_set_pileup; scrg_pileup_from_runs)");
        }
        if (p.lanes_per_pair != 1)
            return c->fail(SCRG_ERR_INVALID_ARG, "anchored alignment needs lanes_per_pair = 1, the default (the GenASM-row mappings read texts forwards only)");
        if (c->opt.read_summary)
            return c->fail(SCRG_ERR_INVALID_ARG, "anchored alignment has no best-candidate mode, so no read summary is made (scrg_ctx_set_read_summary)");
        uint64_t glen = 0;
        if (!c->host_state || !scrg_host::genome_resident(c->host_state, &glen))
            return c->fail(SCRG_ERR_INVALID_ARG, "no resident genome: call scrg_genome_set first");
        if ((n_reads && (!reads || !read_lens)) || !cand_offsets) return c->fail(SCRG_ERR_INVALID_ARG, "null input array");
        const uint64_t n = cand_offsets[n_reads];
        if (2 * n > kMaxPairsPerLaunch) return c->fail(SCRG_ERR_INVALID_ARG, "too many pairs");
        if (n && (!anchor_genome || !anchor_read)) return c->fail(SCRG_ERR_INVALID_ARG, "null anchor array");
        for (uint64_t r = 0; r < n_reads; r++) {
            if (read_lens[r] && !reads[r]) return c->fail(SCRG_ERR_INVALID_ARG, "null read pointer");
            if (read_lens[r] > 0x7fffffffull) return c->fail(SCRG_ERR_INVALID_ARG, "read longer than 2^31-1");
            if (cand_offsets[r + 1] < cand_offsets[r]) return c->fail(SCRG_ERR_INVALID_ARG, "cand_offsets not monotone");
        }
        // the halves: sub-read 2p = R'[0, ra) leftwards ending at ga, sub-read 2p + 1 = R'[ra, L) rightwards from ga — as
        // stretches of the caller's (forward) read, which for a reverse-strand candidate lie the other way round
        static const char nothing[1] = {0};
        std::vector<const char*> h_reads(2 * n);
        std::vector<uint64_t> h_lens(2 * n), h_off(2 * n + 1), h_start(2 * n);
        std::vector<uint8_t> h_rev(2 * n), h_left(2 * n);
        for (uint64_t r = 0; r < n_reads; r++) {
            const uint64_t L = read_lens[r];
            const char* const rd = reads[r] ? reads[r] : nothing;
            for (uint64_t q = cand_offsets[r]; q < cand_offsets[r + 1]; q++) {
                const uint64_t ra = anchor_read[q], ga = anchor_genome[q];
                if (ra > L || ga > glen) return c->fail(SCRG_ERR_INVALID_ARG, "anchor out of range: anchor_read 0 .. read length, anchor_genome 0 .. genome length");
                const bool rev = cand_reverse && cand_reverse[q];
                h_reads[2 * q] = rev ? rd + (L - ra) : rd;
                h_lens[2 * q] = ra;
                h_reads[2 * q + 1] = rev ? rd : rd + ra;
                h_lens[2 * q + 1] = L - ra;
                h_start[2 * q] = h_start[2 * q + 1] = ga;
                h_rev[2 * q] = h_rev[2 * q + 1] = rev ? 1 : 0;
                h_left[2 * q] = 1;
                h_left[2 * q + 1] = 0;
            }
        }
        for (uint64_t k = 0; k <= 2 * n; k++) h_off[k] = k;
        const bool distance = (p.outputs & SCRG_OUT_DISTANCE) != 0;
        const bool want_runs = !distance && p.outputs != SCRG_OUT_TEXT, want_text = !distance && p.outputs != SCRG_OUT_RUNS;
        scrg_params q = p;
        q.outputs = distance ? SCRG_OUT_DISTANCE : SCRG_OUT_RUNS;          // (the text is rendered from the joined runs)
        scrg_result* h = nullptr;
        scrg_status s = scrg_align_mapping_directed(c, &q, 2 * n, h_reads.data(), h_lens.data(), h_off.data(), h_start.data(), h_rev.data(),
                                                    h_left.data(), &h);
        if (s != SCRG_OK && !(s == SCRG_ERR_CIGAR_OVERFLOW && h)) return s;

        scrg_result* r = static_cast<scrg_result*>(calloc(1, sizeof(scrg_result)));
        auto bail = [&](scrg_status st, const char* what) {
            scrg_result_free(h);
            scrg_result_free(r);
            return c->fail(st, what);
        };
        if (!r) return bail(SCRG_ERR_OOM, "result");
        r->n_pairs = n;
        r->edit_distance = static_cast<int64_t*>(g_pool.get((n + 1) * 8, true));
        r->pair_status = static_cast<uint32_t*>(g_pool.get((n + 1) * 4, true));
        r->run_offset = static_cast<uint64_t*>(g_pool.get((n + 1) * 8, true));
        r->cigar_offset = static_cast<uint64_t*>(g_pool.get((n + 1) * 8, true));
        if (distance) r->text_end = static_cast<uint64_t*>(g_pool.get((n + 1) * 8, true));
        if (!r->edit_distance || !r->pair_status || !r->run_offset || !r->cigar_offset || (distance && !r->text_end)) return bail(SCRG_ERR_OOM, "result arrays");
        bool overflow = false;
        uint64_t total_text = 0;
        auto chars_of = [](const scrg_run& x) -> uint64_t { return 2u + (x.count >= 10 ? 1u : 0u) + (x.count >= 100 ? 1u : 0u); };
        std::vector<scrg_run> joined;
        // pair k's runs, joined (the runs of its two halves lie side by side in h)
        auto join = [&](uint64_t k, uint64_t* nj) {
            const uint64_t a0 = h->run_offset[2 * k], a1 = h->run_offset[2 * k + 1], a2 = h->run_offset[2 * k + 2];
            joined.resize(a2 - a0 + 1);
            return scrg_join_anchored_runs(h->runs + a0, a1 - a0, h->runs + a1, a2 - a1, joined.data(), joined.size(), nj, nullptr);
        };
        for (uint64_t k = 0; k < n; k++) {
            r->edit_distance[k] = h->edit_distance[2 * k] + h->edit_distance[2 * k + 1];
            const bool ov = h->pair_status[2 * k] != SCRG_OK || h->pair_status[2 * k + 1] != SCRG_OK;
            r->pair_status[k] = ov ? (uint32_t)SCRG_ERR_CIGAR_OVERFLOW : (uint32_t)SCRG_OK;
            overflow = overflow || ov;
            uint64_t consumed = 0;
            if (distance) {
                consumed = h->text_end[2 * k];
                r->text_end[k] = h->text_end[2 * k] + h->text_end[2 * k + 1];
            } else {
                // (the runs of pair k are the runs of its two halves, which lie side by side: the offsets carry over)
                uint64_t chars = 1;
                for (uint64_t x = h->run_offset[2 * k]; x < h->run_offset[2 * k + 2]; x++) {
                    if (x < h->run_offset[2 * k + 1] && h->runs[x].op != 'I') consumed += h->runs[x].count;
                    chars += chars_of(h->runs[x]);
                }
                if (want_text && c->opt.cigar_form != SCRG_CIGAR_WINDOWED) {       // (a stretch may cross the seam: measured on the joined runs)
                    uint64_t nj = 0;
                    if (join(k, &nj) != SCRG_OK || scrg_cigar_from_runs(c->opt.cigar_form, joined.data(), nj, nullptr, 0, &chars) != SCRG_OK)
                        return bail(SCRG_ERR_INVALID_ARG, "internal: a half's runs hold a zero count or an operation other than = X I D");
                }
                if (want_runs) r->run_offset[k + 1] = h->run_offset[2 * k + 2];
                if (want_text) {
                    total_text += chars;
                    r->cigar_offset[k + 1] = total_text;
                }
            }
            if (text_start) text_start[k] = anchor_genome[k] - consumed;
        }
        const uint64_t total_runs = want_runs ? h->run_offset[2 * n] : 0;
        r->runs = static_cast<scrg_run*>(g_pool.get(2 * total_runs + 16, false));
        r->cigar_text = static_cast<char*>(g_pool.get(total_text + 16, false));
        if (!r->runs || !r->cigar_text) return bail(SCRG_ERR_OOM, "result arrays");
        if (!distance) {
            for (uint64_t k = 0; k < n; k++) {
                const uint64_t a0 = h->run_offset[2 * k];
                uint64_t nj = 0;
                const scrg_status js = join(k, &nj);
                if (js != SCRG_OK) return bail(SCRG_ERR_INVALID_ARG, "internal: a half's runs hold an operation other than = X I D");
                if (want_runs && nj) memcpy(r->runs + a0, joined.data(), nj * sizeof(scrg_run));
                if (want_text) {
                    char* t = r->cigar_text + r->cigar_offset[k];
                    if (c->opt.cigar_form != SCRG_CIGAR_WINDOWED) {
                        uint64_t len = 0;
                        if (scrg_cigar_from_runs(c->opt.cigar_form, joined.data(), nj, t, r->cigar_offset[k + 1] - r->cigar_offset[k], &len) != SCRG_OK)
                            return bail(SCRG_ERR_INVALID_ARG, "internal: the joined text does not have its measured length");
                        continue;
                    }
                    for (uint64_t x = 0; x < nj; x++) t += sprintf(t, "%d%c", (int)joined[x].count, joined[x].op);
                    *t = 0;
                }
            }
        }
        r->kernel_ns = h->kernel_ns;
        r->pack_ns = h->pack_ns;
        scrg_result_free(h);
        r->total_ns = now_ns() - t_begin;
        *out = r;
        if (overflow) return c->fail(SCRG_ERR_CIGAR_OVERFLOW, "at least one pair overflowed its CIGAR slice (see pair_status)");
        return (scrg_status)SCRG_OK;
    });
}

static uint64_t host_brev64(uint64_t v)
{
    v = ((v >> 1) & 0x5555555555555555ull) | ((v & 0x5555555555555555ull) << 1);
    v = ((v >> 2) & 0x3333333333333333ull) | ((v & 0x3333333333333333ull) << 2);
    v = ((v >> 4) & 0x0f0f0f0f0f0f0f0full) | ((v & 0x0f0f0f0f0f0f0f0full) << 4);
    return __builtin_bswap64(v);
}

scrg_status scrg_text_window_planes(const uint64_t* planar, uint64_t n_words, uint64_t text_off, uint64_t text_len, uint64_t ref_idx,
                                    int32_t W, uint64_t stride_words, uint64_t* lo, uint64_t* hi, uint64_t* first_word, uint64_t* last_word)
{
    if (!planar || !lo || !hi || W < 1 || W > 256 || stride_words > 0xffffffffull) return SCRG_ERR_INVALID_ARG;
    const uint32_t stride = stride_words ? (uint32_t)stride_words : 1u;
    const scrg::TextStretch ts = scrg::text_stretch(text_off, text_len, true, stride);
    if (ref_idx > ts.len) return SCRG_ERR_INVALID_ARG;
    const uint32_t at0 = (uint32_t)ref_idx, n = std::min<uint32_t>((uint32_t)W, ts.len - at0), nw = ((uint32_t)W + 63u) / 64u;
    // (as the kernels: a word of 64 characters is three words of the array from the word its first base is in; words of the
    // window that hold no character of the text are not loaded)
    uint64_t w0[4], first = ~0ull, last = 0;
    uint32_t bit[4], sh[4];
    for (uint32_t w = 0; w < nw && 64u * w < n; w++) {
        uint32_t k = at0 + 64u * w;              // (< text_len: this word holds a character of the text)
        sh[w] = 0;
        if (ts.rev) {
            const scrg::TextRevAt r = scrg::text_rev_at(ts.len, at0, w);
            k = r.at;
            sh[w] = r.sh;
        }
        w0[w] = scrg::window_first_word(ts.off, k, stride, bit[w]);
        if (w0[w] >= n_words || 2ull * stride >= n_words - w0[w]) return SCRG_ERR_INVALID_ARG;
        first = std::min<uint64_t>(first, w0[w]);
        last = std::max<uint64_t>(last, w0[w] + 2ull * stride);
    }
    for (uint32_t w = 0; w < nw; w++) {
        lo[w] = hi[w] = 0;
        if (64u * w >= n) continue;
        const uint64_t a = planar[w0[w]], b = planar[w0[w] + stride], c3 = planar[w0[w] + 2ull * stride];
        auto funnel = [&](uint32_t x0, uint32_t x1, uint32_t x2) -> uint64_t {
            const uint32_t s5 = bit[w];
            const uint32_t l = (uint32_t)((((uint64_t)x1 << 32) | x0) >> s5), h2 = (uint32_t)((((uint64_t)x2 << 32) | x1) >> s5);
            return ((uint64_t)h2 << 32) | l;
        };
        uint64_t flo = funnel((uint32_t)a, (uint32_t)b, (uint32_t)c3), fhi = funnel((uint32_t)(a >> 32), (uint32_t)(b >> 32), (uint32_t)(c3 >> 32));
        if (ts.rev) {
            flo = ~host_brev64(flo << sh[w]);
            fhi = ~host_brev64(fhi << sh[w]);
        }
        lo[w] = flo;
        hi[w] = fhi;
    }
    if (first_word) *first_word = first;
    if (last_word) *last_word = last;
    return SCRG_OK;
}

scrg_status scrg_align_pairs_multi(const int32_t* devices, int32_t n_devices, const scrg_params* params, uint64_t n_pairs,
                                   const char* const* texts, const uint64_t* text_lens, const char* const* queries,
                                   const uint64_t* query_lens, scrg_result** out)
{
    if (!out || !devices || n_devices < 1 || n_devices > 64) return SCRG_ERR_INVALID_ARG;
    *out = nullptr;
    return guarded(nullptr, [&] {
        scrg_host::Batch b;
        std::string err;
        scrg_status s = pairs_batch(params, n_pairs, texts, text_lens, queries, query_lens, &b, &err);
        if (s != SCRG_OK) { g_multi_error = err; return s; }
        return multi_align(devices, n_devices, params, b, out);
    });
}

scrg_status scrg_align_mapping_multi(const int32_t* devices, int32_t n_devices, const scrg_params* params, const char* genome,
                                     uint64_t genome_len, uint64_t n_reads, const char* const* reads, const uint64_t* read_lens,
                                     const uint64_t* cand_offsets, const uint64_t* cand_start, const uint8_t* cand_reverse,
                                     scrg_result** out)
{
    if (!out || !devices || n_devices < 1 || n_devices > 64 || (genome_len && !genome)) return SCRG_ERR_INVALID_ARG;
    *out = nullptr;
    return guarded(nullptr, [&] {
        scrg_host::Batch b;
        std::vector<uint32_t> pair_read;
        std::string err;
        scrg_status s = mapping_batch(n_reads, reads, read_lens, cand_offsets, cand_start, cand_reverse, &b, &pair_read, &err);
        if (s != SCRG_OK) { g_multi_error = err; return s; }
        static const char empty_genome[1] = {0};
        b.genome = genome ? genome : empty_genome;
        b.genome_len = genome_len;
        return multi_align(devices, n_devices, params, b, out);
    });
}

scrg_status scrg_host_plan(const scrg_params* params, int32_t n_devices, uint64_t n_pairs, const uint64_t* text_lens,
                           const uint64_t* read_lens, uint32_t* issue_order, uint64_t* chunk_first, uint64_t chunk_cap, uint64_t* n_chunks)
{
    if (n_devices < 1 || !n_chunks || (n_pairs && !read_lens)) return SCRG_ERR_INVALID_ARG;
    return guarded(nullptr, [&] {
        scrg_params p;
        if (!resolve_params(params, &p) || (p.outputs & SCRG_OUT_BEST)) return (scrg_status)SCRG_ERR_INVALID_ARG;      // (pairs have no groups)
        scrg_host::Batch b;
        std::vector<uint64_t> zeros;
        b.n_pairs = n_pairs;
        b.mapping = false;
        b.read_lens = read_lens;
        if (!text_lens) {
            zeros.assign(n_pairs, 0);
            text_lens = zeros.data();
        }
        b.text_lens = text_lens;
        return scrg_host::plan(p, n_devices, b, issue_order, chunk_first, chunk_cap, n_chunks);
    });
}

scrg_status scrg_host_plan_mapping(const scrg_params* params, int32_t n_devices, uint64_t n_reads, const uint64_t* read_lens,
                                   const uint64_t* cand_offsets, uint32_t* issue_order, uint64_t* chunk_first, uint64_t chunk_cap,
                                   uint64_t* n_chunks)
{
    if (n_devices < 1 || !n_chunks || !cand_offsets || (n_reads && !read_lens)) return SCRG_ERR_INVALID_ARG;
    return guarded(nullptr, [&] {
        scrg_params p;
        if (!resolve_params(params, &p)) return (scrg_status)SCRG_ERR_INVALID_ARG;
        scrg_host::Batch b;
        std::vector<uint32_t> pair_read;
        std::vector<const char*> no_reads(n_reads, "");      // (the plan looks at lengths only)
        std::string err;
        std::vector<uint64_t> no_starts(cand_offsets[n_reads], 0);
        const scrg_status s = mapping_batch(n_reads, no_reads.data(), read_lens, cand_offsets, no_starts.data(), nullptr, &b, &pair_read, &err);
        if (s != SCRG_OK) { g_multi_error = err; return s; }
        return scrg_host::plan(p, n_devices, b, issue_order, chunk_first, chunk_cap, n_chunks);
    });
}

scrg_status scrg_host_plan_mates(const scrg_params* params, int32_t n_devices, uint64_t n_reads, const uint64_t* read_lens,
                                 const uint64_t* cand_offsets, uint32_t* issue_order, uint64_t* chunk_first, uint64_t chunk_cap, uint64_t* n_chunks)
{
    if (n_devices < 1 || !n_chunks || !cand_offsets || (n_reads && !read_lens) || n_reads % 2) return SCRG_ERR_INVALID_ARG;
    return guarded(nullptr, [&] {
        scrg_params p;
        if (!resolve_params(params, &p)) return (scrg_status)SCRG_ERR_INVALID_ARG;
        scrg_host::Batch b;
        std::vector<uint32_t> pair_read;
        std::string err;
        // (the plan looks at lengths and counts only: no reads, no starts; the offsets are checked before anything is sized by them)
        const scrg_status s = mapping_batch(n_reads, nullptr, read_lens, cand_offsets, nullptr, nullptr, &b, &pair_read, &err, true);
        if (s != SCRG_OK) { g_multi_error = err; return s; }
        static const scrg_mate_rule any_fr = {0, ~0ull, SCRG_MATES_FR, 0, {0, 0}};
        b.mate_rule = &any_fr;
        return scrg_host::plan(p, n_devices, b, issue_order, chunk_first, chunk_cap, n_chunks);
    });
}

scrg_status scrg_pack_planar_host(const char* ascii, uint64_t n_bases, uint64_t* planar, uint64_t stride_words, uint64_t n_words)
{
    if ((n_bases && !ascii) || (n_words && !planar) || 32 * n_words < n_bases) return SCRG_ERR_INVALID_ARG;
    return scrg_host::pack_planar_host(ascii, n_bases, planar, stride_words, n_words) ? SCRG_ERR_BAD_BASE : SCRG_OK;
}

void scrg_multi_release(void)
{
    std::lock_guard<std::mutex> g(g_multi_mu);
    for (auto& ds : g_multi_states) scrg_host::state_free(ds.second);
    g_multi_states.clear();
    g_multi_busy.clear();
    if (g_live_ctx.load() == 0) { g_pool.trim(); g_diff_pool.trim(); }     // no handle of the caller's is alive either: give the recycled result arrays back
}

const char* scrg_multi_last_error(void) { return g_multi_error.c_str(); }

}  // extern "C"

namespace scrg_int {
scrg_status ctx_create_internal(int device, scrg_ctx** out) { return ctx_create_impl(device, out, false); }
}  // namespace scrg_int
