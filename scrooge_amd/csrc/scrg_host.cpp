// scrg_host.cpp — the host-pointer entry points as a PIPELINE over chunks, streams and GPUs.
//
// What the reference does around its kernel (src/genasm_gpu.cu:890-1065: convert and concatenate the sequences, size the
// CIGAR storage, launch, walk the lists into strings) happens here per CHUNK of a few thousand pairs, four chunks in
// flight per GPU, so that the PCIe transfers, the kernels and the host's own work overlap:
//
//   host   pack the chunk's sequences to 2 bits per base (AVX2: 32 bases per load, two movemasks) straight into pinned
//          memory, in the lane-interleaved layout the align kernel reads best — a quarter of the bytes of ASCII cross PCIe
//   H2D    packed sequences + 8..16 bytes per pair; the 48-byte problem descriptors are built on the device
//   GPU    genasm_lane_kernel, per-pair text lengths, offsets by prefix sum, run compaction, "%d%c" rendering of the text
//   D2H    dense runs, text, offsets, scores of the chunk into pinned staging; two sizes come back first
//   host   the chunk's results are copied to their place in the result arrays (threads), offsets get their base
//
// A batch is cut in issue order (longest read first, src/tests.cu:375-377); chunk k goes to device k mod N, so several
// GPUs share one call (scrg_align_pairs_multi: two host threads, four streams and four buffer sets per device).
// Results are assembled in issue order as chunks finish and put into caller order at the end (nothing to do when the
// batch already was in issue order).  No CPU fallback anywhere: without a device every entry point fails.
#include <hip/hip_runtime.h>
#include <immintrin.h>

#include <condition_variable>
#include <cstdio>
#include <memory>
#include <numeric>
#include <shared_mutex>

#include "genasm_kernels.h"
#include "host_path.h"
#include "mate_rule.h"
#include "mapq_rule.h"
#include "pileup_rule.h"
#include "seed_rule.h"
#include "scrg_internal.h"

namespace {

using scrg_int::DevBuf;
using scrg_int::g_diff_pool;
using scrg_int::g_pool;
using scrg_int::HostPinned;
using scrg_int::now_ns;
using scrg_int::parallel_for;

constexpr int NSLOT = 4;                                 // chunks in flight per device (HIP has 4 hardware queues per process and device) ...
constexpr int MAXSLOT = 8;                               // ... and twice as many for short reads: their kernels take ~0.2 ms per chunk, what limits such a call is
                                                         // how soon a slot comes back (pack, H2D, kernels, look at the sizes, compaction, text, D2H, collection)
constexpr uint64_t SHORT_READS = 1000;                   // longest read of a call that uses MAXSLOT slots
constexpr size_t NCOLLECT = 2;                            // collect threads per device
constexpr size_t LAG2_DEFAULT = 2;                        // a chunk's sizes are looked at this many chunks after it was launched
constexpr uint64_t GROUP = 64;
constexpr uint64_t SEQ_PAD = 2 * GROUP + 2;              // SCRG_SEQ_PAD_WORDS_STRIDED(64)

// ---------------------------------------------------------------------------------------------------------------
// ASCII -> planar 2-bit on the host.  One uint64 per 32 bases: bit k of the low dword = bit 0 of base k's code, bit k of
// the high dword = bit 1 (A0 C1 G2 T3, src/genasm_cpu.cpp:87-90; lower case too, :462-493).  (c >> 1) & 3 gives
// A0 C1 T2 G3; code = x ^ (x >> 1).  Returns the word; *bad gets a bit for every byte that is not one of ACGTacgt.
// ---------------------------------------------------------------------------------------------------------------
__attribute__((target("avx2"))) inline uint64_t pack32_avx2(const char* p, uint32_t* bad)
{
    const __m256i x = _mm256_loadu_si256(reinterpret_cast<const __m256i*>(p));
    const uint32_t b1 = (uint32_t)_mm256_movemask_epi8(_mm256_slli_epi16(x, 6));      // bit 1 of every byte
    const uint32_t b2 = (uint32_t)_mm256_movemask_epi8(_mm256_slli_epi16(x, 5));      // bit 2
    const __m256i u = _mm256_and_si256(x, _mm256_set1_epi8((char)0xDF));
    const __m256i ok = _mm256_or_si256(_mm256_or_si256(_mm256_cmpeq_epi8(u, _mm256_set1_epi8('A')), _mm256_cmpeq_epi8(u, _mm256_set1_epi8('C'))),
                                       _mm256_or_si256(_mm256_cmpeq_epi8(u, _mm256_set1_epi8('G')), _mm256_cmpeq_epi8(u, _mm256_set1_epi8('T'))));
    *bad = ~(uint32_t)_mm256_movemask_epi8(ok);
    return ((uint64_t)b2 << 32) | (uint64_t)(b1 ^ b2);
}

inline uint64_t pack32_scalar(const char* p, uint32_t* bad)
{
    uint32_t lo = 0, hi = 0, bd = 0;
    for (unsigned k = 0; k < 32; k++) {
        const unsigned c = (unsigned char)p[k], u = c & 0xDFu;
        const unsigned x0 = (c >> 1) & 1u, x1 = (c >> 2) & 1u;
        lo |= (x0 ^ x1) << k;
        hi |= x1 << k;
        bd |= (u == 'A' || u == 'C' || u == 'G' || u == 'T' ? 0u : 1u) << k;
    }
    *bad = bd;
    return ((uint64_t)hi << 32) | lo;
}

const bool g_have_avx2 = __builtin_cpu_supports("avx2");

inline char complement_base(char c)
{
    switch (c) {
    case 'A': return 'T'; case 'C': return 'G'; case 'G': return 'C'; case 'T': return 'A';
    case 'a': return 't'; case 'c': return 'g'; case 'g': return 'c'; case 't': return 'a';
    default: return c;   // left as is: counted as a bad base
    }
}

// words [w_from, words) of one sequence at dst[w * stride] (zero beyond the sequence); returns true if a bad base was seen
bool pack_sequence(const char* src, uint64_t len, bool revcomp, uint64_t* dst, uint64_t stride, uint64_t words, uint64_t w_from = 0)
{
    bool bad_any = false;
    const uint64_t full = len / 32;
    uint32_t bad = 0;
    if (!revcomp) {
        // (a 64-bases-per-step AVX-512BW version of this loop packs at the same rate on the EPYC 9575F of the GPU boxes: with
        // 16 threads the packing is bound by memory bandwidth, ~150 GB/s of ASCII, not by instructions)
        if (g_have_avx2)
            for (uint64_t w = w_from; w < full; w++) { dst[w * stride] = pack32_avx2(src + 32 * w, &bad); bad_any |= bad != 0; }
        else
            for (uint64_t w = w_from; w < full; w++) { dst[w * stride] = pack32_scalar(src + 32 * w, &bad); bad_any |= bad != 0; }
    }
    char tmp[32];
    for (uint64_t w = revcomp ? w_from : std::max(full, w_from); 32 * w < len; w++) {
        const uint64_t n = std::min<uint64_t>(32, len - 32 * w);
        if (revcomp) for (uint64_t k = 0; k < n; k++) tmp[k] = complement_base(src[len - 1 - (32 * w + k)]);
        else memcpy(tmp, src + 32 * w, n);
        if (n < 32) memset(tmp + n, 'A', 32 - n);
        uint64_t v = g_have_avx2 ? pack32_avx2(tmp, &bad) : pack32_scalar(tmp, &bad);
        if (n < 32) {                        // padding encodes as A = 0 anyway; keep only the real bases' error bits
            bad &= (1u << n) - 1u;
        }
        dst[w * stride] = v;
        bad_any |= bad != 0;
    }
    for (uint64_t w = std::max((len + 31) / 32, w_from); w < words; w++) dst[w * stride] = 0;
    return bad_any;
}

// Eight forward rows of one group of the lane-interleaved layout at once (dst[w * 64 + l], l = 0..7 consecutive lanes):
// the whole words all eight have are packed word by word across the rows, so that every store completes a 64-byte line
// (row by row, consecutive stores of a row are 512 bytes apart); the rest of each row follows row by row.
__attribute__((target("avx2"))) bool pack_rows8_avx2(const char* const* src, const uint64_t* len, uint64_t* dst, uint64_t words)
{
    uint64_t common = ~0ull;
    for (int l = 0; l < 8; l++) common = std::min(common, len[l] / 32);
    uint32_t bad_acc = 0, bad = 0;
    for (uint64_t w = 0; w < common; w++) {
        uint64_t* const line = dst + w * GROUP;
        for (int l = 0; l < 8; l++) {
            line[l] = pack32_avx2(src[l] + 32 * w, &bad);
            bad_acc |= bad;
        }
    }
    bool bad_any = bad_acc != 0;
    for (int l = 0; l < 8; l++) bad_any |= pack_sequence(src[l], len[l], false, dst + l, GROUP, words, common);
    return bad_any;
}

// ---------------------------------------------------------------------------------------------------------------
// per-device state
// ---------------------------------------------------------------------------------------------------------------
// The kinds of fixed-size per-pair records a call can make beside its result (CallOptions: report, clip).  A kind is one line here
// and one in Call::rec_on(); its slot buffers, read-back, place in the call's issue-order array and way into caller order are shared.
enum { REC_REPORT, REC_CLIP, N_REC };
constexpr size_t REC_SIZE[N_REC] = {sizeof(scrg_pair_report), sizeof(scrg_pair_clip)};
struct RecordBuf {
    DevBuf d;                                // [n] records, written by the kind's kernel in stage 1
    HostPinned h;                            // their staging area: read back in stage 2, placed in stage 3
};

struct Slot {
    hipStream_t stream = nullptr;
    scrg_ctx* ctx = nullptr;                 // a handle of the device-pointer layer bound to `stream`
    hipEvent_t ev_tot = nullptr, ev_done = nullptr;
    HostPinned h_seq, h_meta, h_out, h_tot;
    DevBuf d_meta, d_desc, d_slices, d_ed, d_nruns, d_cnt64, d_len64, d_tot, d_dense, d_temp;     // d_ed: the per-pair results (PerPairLayout), d_dense: runs, then text
    // difference strings (a handle with a kind set): lengths [n + 1], offsets [n + 1] and the render pass's bad count behind them, the text
    DevBuf d_dlen, d_doff, d_dtext;
    HostPinned h_diff;                       // [offsets 8 (n + 2) | text]
    RecordBuf rec[N_REC];                    // the alignment report and the clip records: one record per pair
    // a paired call (MatesLayout): the chunk's mate pairs' offsets and the pairs' strands go up, one record per mate pair comes back
    HostPinned h_mates, h_mrec;
    DevBuf d_mates;
    uint64_t mate0 = 0, n_mates = 0;         // the chunk's mate pairs: first (in issue order) and number
    // the read summary (SummaryLayout): the chunk's reads' offsets go up, one record per read comes back
    HostPinned h_sum, h_srec;
    DevBuf d_sum;
    uint64_t sum0 = 0, n_sum = 0;            // the chunk's reads: first (in issue order) and number
    scrg_params pp;                          // the chunk's launch parameters (strides, strands): the render pass of stage 2 reads the sequences again
    // the chunk in flight
    uint64_t n = 0, first = 0;               // pairs, first issue index
    uint64_t tot_runs = 0, tot_text = 0, tot_diff = 0;
    int64_t t_pack_ns = 0;
};

// scrg_find_candidates' device buffers: the call's reads (packed, first words, lengths, lane offsets), every read's totals, a chunk's buffers
enum SeedWs { W_SEQ, W_WORD, W_LEN, W_LANE, W_HITS, W_OVER, W_LOOK, W_CNT, W_OFF, W_WORDS, W_U32, W_ANCHOR, W_OUT, W_TEMP, N_SEED_WS };

struct DeviceState {
    int device = 0, n_cus = 0;
    DevBuf d_seq;                            // [ genome | slot 0 | slot 1 | slot 2 ]
    uint64_t genome_words = 0, genome_len = 0;
    bool genome_ok = false;                  // d_seq starts with a packed genome
    uint64_t slot_words = 0;
    Slot slot[MAXSLOT];
    // the pileup accumulator (a handle with scrg_ctx_set_pileup; scrg_internal.h: PileupView): the one buffer that outlives a call
    DevBuf d_pile;
    uint64_t pile_len = 0;
    bool pile_dirty = false;                 // a call has added to it since the last take
    // the k-mer index of the resident genome (scrg_genome_index): entries sorted by key and the bucket table.  Positions, no pointers:
    // ensure_seq may move the genome.  It goes when the genome goes (drop_index).
    struct SeedIndex {
        bool ok = false;
        scrg::SeedRule rule{};
        uint64_t n_entries = 0;
        uint32_t bucket_bits = 0;
        uint32_t smer = 0;                   // the sampling it was built with (scrg_ctx_set_seed_sampling at that time)
        uint64_t n_positions = 0;            // the positions it considered: n_entries of them were selected
        uint64_t last_n_lookups = 0;         // the selected (read, strand, r) of the last successful scrg_find_candidates
        DevBuf keys, pos, buckets;
    } seed;
    DevBuf seed_ws[N_SEED_WS];               // scrg_find_candidates' buffers (SeedWs): kept between calls, given back with the index
    void drop_index()
    {
        seed.ok = false;
        seed.keys.release();
        seed.pos.release();
        seed.buckets.release();
        for (DevBuf& b : seed_ws) b.release();
    }
    std::mutex mu;                           // one call at a time per device state
    // the last error text: written by the launch thread and both collect threads of a call
    std::mutex err_mu;
    std::string err;
    void set_err(const std::string& e)
    {
        std::lock_guard<std::mutex> g(err_mu);
        err = e;
    }
    std::string get_err()
    {
        std::lock_guard<std::mutex> g(err_mu);
        return err;
    }
};

#define HTRY(ds, call)                                                                                   \
    do {                                                                                                 \
        hipError_t e__ = (call);                                                                         \
        if (e__ != hipSuccess) {                                                                         \
            (ds)->set_err(std::string(#call) + ": " + hipGetErrorString(e__));                           \
            (void)hipGetLastError();                                                                     \
            return e__ == hipErrorOutOfMemory ? SCRG_ERR_OOM : SCRG_ERR_HIP;                             \
        }                                                                                                \
    } while (0)

// a call on the slot's own handle of the device-pointer layer: its error text travels with the status
#define CTRY(ds, sl, call)                                                                               \
    do {                                                                                                 \
        const scrg_status s__ = (call);                                                                  \
        if (s__ != SCRG_OK) {                                                                            \
            (ds)->set_err(scrg_last_error((sl).ctx));                                                    \
            return s__;                                                                                  \
        }                                                                                                \
    } while (0)

// the slot's runs as the device-pointer layer takes them — runs, run_offset, run_offset_stride, n_runs: the slices as the align
// kernel left them, every pair's offset in its descriptor (6 words apart), the run counts
#define SLOT_RUNS(sl) (sl).d_slices.as<scrg_run>(), &(sl).d_desc.as<scrg_pair_desc>()->cigar_off, 6, (sl).d_nruns.as<uint32_t>()

// the sequence array: genome first (so that a candidate's text offset is its start_in_reference), then one region per slot
scrg_status ensure_seq(DeviceState* ds, uint64_t genome_words, uint64_t slot_words)
{
    const uint64_t gpad = genome_words ? genome_words + SCRG_SEQ_PAD_WORDS : 0;
    const uint64_t need_slot = std::max(slot_words, ds->slot_words);
    const uint64_t have_g = ds->genome_words ? ds->genome_words + SCRG_SEQ_PAD_WORDS : 0;
    if (gpad == have_g && need_slot == ds->slot_words && ds->d_seq.p) return SCRG_OK;
    HTRY(ds, hipSetDevice(ds->device));
    HTRY(ds, hipDeviceSynchronize());
    DevBuf bigger;
    const uint64_t grow_slot = need_slot > ds->slot_words ? need_slot + need_slot / 4 : need_slot;
    HTRY(ds, bigger.ensure((gpad + MAXSLOT * grow_slot + 8) * sizeof(uint64_t)));
    if (ds->genome_ok && gpad == have_g && gpad) {       // keep a resident genome
        HTRY(ds, hipMemcpy(bigger.p, ds->d_seq.p, gpad * sizeof(uint64_t), hipMemcpyDeviceToDevice));
    } else {
        ds->genome_ok = false;
        ds->drop_index();
    }
    ds->d_seq.release();
    ds->d_seq = bigger;
    ds->genome_words = genome_words;
    ds->slot_words = grow_slot;
    return SCRG_OK;
}

// A genome is packed ONCE per call, whatever the number of device states: into one pinned, portable staging buffer
// (host threads), from which every device gets its copy — the H2D copies of all devices run side by side.  The staging
// buffer is kept for the next call while it is small (a 100 Mbp chromosome is 25 MB) and released when it is not (a
// 3 Gbp genome would otherwise pin 0.8 GB of host memory for good).
constexpr size_t GENOME_STAGING_KEEP = 256u << 20;
struct GenomeStaging {
    std::mutex mu;
    HostPinned buf;                    // (registered memory is portable: every device copies from it)
    void* p = nullptr;
    size_t cap = 0;
    hipError_t ensure(size_t bytes)
    {
        if (bytes <= cap) return hipSuccess;
        release();
        hipError_t e = bytes >= HostPinned::kRegisterMin ? buf.ensure(bytes) : hipErrorInvalidValue;
        if (e == hipSuccess && buf.registered) {
            p = buf.p;
            cap = buf.cap;
            return hipSuccess;
        }
        buf.release();                 // small, or not registered: portable memory from HIP itself
        e = hipHostMalloc(&p, bytes, hipHostMallocPortable);
        if (e == hipSuccess) cap = bytes;
        else p = nullptr;
        return e;
    }
    void release()
    {
        if (buf.p) buf.release();
        else if (p) (void)hipHostFree(p);
        p = nullptr;
        cap = 0;
    }
};
GenomeStaging g_genome_staging;

scrg_status stage_genome(DeviceState* const* dss, int n_states, const char* genome, uint64_t genome_len)
{
    const uint64_t words = (genome_len + 31) / 32;
    for (int d = 0; d < n_states; d++) {
        dss[d]->genome_ok = false;
        dss[d]->drop_index();
        scrg_status s = ensure_seq(dss[d], words, dss[d]->slot_words);
        if (s != SCRG_OK) {
            if (d) dss[0]->set_err(dss[d]->get_err());
            return s;
        }
    }
    DeviceState* const ds = dss[0];
    std::lock_guard<std::mutex> g(g_genome_staging.mu);
    // a staging area larger than GENOME_STAGING_KEEP is given back on EVERY way out of this function (a rejected 3 Gbp genome
    // must not leave 0.8 GB pinned until the next call)
    struct ReleaseOversize {
        ~ReleaseOversize() { if (g_genome_staging.cap > GENOME_STAGING_KEEP) g_genome_staging.release(); }
    } release_oversize;
    HTRY(ds, hipSetDevice(ds->device));
    HTRY(ds, g_genome_staging.ensure((words + SCRG_SEQ_PAD_WORDS) * sizeof(uint64_t)));
    uint64_t* const h = static_cast<uint64_t*>(g_genome_staging.p);
    const uint64_t PIECE = 1u << 15;                    // words per work item: 1 Mbase
    std::atomic<int> bad{0};
    parallel_for((words + PIECE - 1) / PIECE, [&](uint64_t i) {
        const uint64_t w0 = i * PIECE, w1 = std::min(words, w0 + PIECE);
        const uint64_t b0 = 32 * w0, b1 = std::min(genome_len, 32 * w1);
        if (pack_sequence(genome + b0, b1 - b0, false, h + w0, 1, w1 - w0)) bad.store(1, std::memory_order_relaxed);
    }, true);
    for (uint64_t w = words; w < words + SCRG_SEQ_PAD_WORDS; w++) h[w] = 0;
    if (bad.load()) {
        ds->set_err("genome contains characters other than ACGTacgt");
        return SCRG_ERR_BAD_BASE;
    }
    scrg_status st = SCRG_OK;
    int issued = 0;
    for (int d = 0; d < n_states && st == SCRG_OK; d++) {
        hipError_t e = hipSetDevice(dss[d]->device);
        if (e == hipSuccess)
            e = hipMemcpyAsync(dss[d]->d_seq.p, h, (words + SCRG_SEQ_PAD_WORDS) * sizeof(uint64_t), hipMemcpyHostToDevice, dss[d]->slot[0].stream);
        if (e != hipSuccess) {
            ds->set_err(std::string("genome upload: ") + hipGetErrorString(e));
            (void)hipGetLastError();
            st = SCRG_ERR_HIP;
        } else {
            issued = d + 1;
        }
    }
    for (int d = 0; d < issued; d++) {
        (void)hipSetDevice(dss[d]->device);
        const hipError_t e = hipStreamSynchronize(dss[d]->slot[0].stream);
        if (e != hipSuccess && st == SCRG_OK) {
            ds->set_err(std::string("genome upload: ") + hipGetErrorString(e));
            (void)hipGetLastError();
            st = SCRG_ERR_HIP;
        }
        if (st == SCRG_OK) {
            dss[d]->genome_len = genome_len;
            dss[d]->genome_ok = true;
        }
    }
    return st;
}

scrg_status pack_genome(DeviceState* ds, const char* genome, uint64_t genome_len)
{
    DeviceState* one[1] = {ds};
    return stage_genome(one, 1, genome, genome_len);
}

// ---------------------------------------------------------------------------------------------------------------
// a call
// ---------------------------------------------------------------------------------------------------------------
struct Grow {                          // a result array that the chunks' collectors fill, each chunk at its own offset
    char* p = nullptr;
    size_t cap = 0;
    std::atomic<size_t> hi{0};         // end of the highest region that has been written (chunks may be collected out of order)
};

struct Call {
    const scrg_host::Batch* b = nullptr;
    scrg_params p;
    uint64_t n = 0;
    std::vector<uint32_t> order;       // issue index -> caller index
    bool identity = true;
    std::vector<uint64_t> chunk_first; // issue index of every chunk's first pair, + n at the end
    int want_runs = 1, want_text = 1;
    bool best = false;                 // SCRG_OUT_BEST: only a read's best candidate keeps its runs and text (mapping calls)
    bool distance = false;             // SCRG_OUT_DISTANCE: edit distance, status and text end only — no slices, no compaction, no text
    // a paired call (Batch::mate_rule; best is set too): reads 2m and 2m+1 are chosen together.  The mate pairs that have pairs, in
    // issue order: mate_id[k], the issue index of its first pair mate_start[k] (+ n at the end) and of its side B's first pair mate_b[k]
    bool mates = false;
    std::vector<uint32_t> mate_id;
    std::vector<uint64_t> mate_start, mate_b;
    scrg_mate_record* mate_rec = nullptr;      // [n_reads / 2] records in caller order (malloc), winner[] as caller pair indices
    // the read summary (opt.read_summary; best is set: the refusal list sees to it).  The reads that have pairs, in issue order:
    // sum_id[k] and the issue index of its first pair sum_start[k] (+ n at the end)
    bool summary = false;
    std::vector<uint32_t> sum_id;
    std::vector<uint64_t> sum_start;
    scrg_read_record* sum_rec = nullptr;       // [n_reads] records in caller order (malloc), winner as the caller's pair index
    bool keep_filter() const { return summary && opt.pileup && opt.mapq_rule.min_keep_q > 0; }
    scrg_host::CallOptions opt;        // the caller's handle's settings (scrg_internal.h)
    bool rec_on(int kind) const { return kind == REC_REPORT ? opt.report : opt.clip; }
    char* iss_rec[N_REC] = {};         // [n] records of every kind that is on, issue order (malloc)

    // results in issue order
    std::shared_mutex grow_mu;
    Grow runs, text, diff;
    uint64_t* iss_diff_off = nullptr;  // [n + 1], with a difference-string kind
    uint64_t* iss_run_off = nullptr;   // [n + 1]
    uint64_t* iss_text_off = nullptr;  // [n + 1]
    int64_t* iss_ed = nullptr;
    uint32_t* iss_status = nullptr;
    uint64_t* iss_tend = nullptr;      // [n + 1], distance-only mode
    // chunk totals, published in any order; bases are prefix sums over them
    std::mutex tot_mu;
    std::condition_variable tot_cv;
    std::vector<uint64_t> c_runs, c_text, c_diff;
    std::vector<char> c_known;
    // status
    std::atomic<int> status{SCRG_OK};
    std::atomic<int> any_overflow{0};
    std::mutex err_mu;
    std::string err;
    std::atomic<int64_t> kernel_ns{0}, pack_ns{0};
    unsigned threads_per_worker = 16;
    int n_slots = NSLOT;               // slots a device uses for this call (make_plan)

    void fail(scrg_status s, const std::string& what)
    {
        int expect = SCRG_OK;
        if (status.compare_exchange_strong(expect, s)) {
            std::lock_guard<std::mutex> g(err_mu);
            err = what;
        }
        // a collector that has just evaluated its wait predicate (under tot_mu) and not blocked yet must not miss this:
        // pass through the mutex before notifying
        { std::lock_guard<std::mutex> g(tot_mu); }
        tot_cv.notify_all();
    }
    bool failed() const { return status.load() != SCRG_OK; }
    // whatever was not handed to the result (std::exchange) goes back where it came from
    ~Call()
    {
        for (void* q : {(void*)runs.p, (void*)text.p, (void*)iss_run_off, (void*)iss_text_off, (void*)iss_ed, (void*)iss_status, (void*)iss_tend}) g_pool.put(q);
        g_diff_pool.put(diff.p);
        g_diff_pool.put(iss_diff_off);
        for (char* q : iss_rec) free(q);
        free(mate_rec);
        free(sum_rec);
    }
};

inline uint64_t read_of(const Call& c, uint64_t p) { return c.b->mapping ? c.b->pair_read[p] : p; }
// the length a pair is issued by: its read's, or — a paired call — the longer mate's, so that a mate pair's pairs sort as one
inline uint64_t issue_len(const Call& c, uint64_t p)
{
    if (!c.mates) return c.b->read_lens[read_of(c, p)];
    const uint64_t r = (uint64_t)c.b->pair_read[p] & ~1ull;
    return std::max(c.b->read_lens[r], c.b->read_lens[r + 1]);
}

// a paired call's per-chunk buffers: [first 8 (2 nm + 1) | reverse n (pad) | records 32 nm] on the device, the first two uploaded
struct MatesLayout {
    size_t o_rev, o_rec, bytes;
    MatesLayout(uint64_t n, uint64_t nm) : o_rev((8 * (2 * nm + 1) + 15) & ~(size_t)15), o_rec((o_rev + n + 255) & ~(size_t)255), bytes(o_rec + 32 * nm + 256) {}
};

// `hint`: what the whole call is expected to need (from the first chunk that arrives: bytes per pair x pairs + 8 %).
// Writers hold grow_mu shared while they copy and raise g.hi first; a regrow (exclusive) moves everything below g.hi.
bool grow_to(Call& c, Grow& g, size_t need, size_t hint, scrg_int::ResultPool& pool = g_pool)
{
    {
        std::shared_lock<std::shared_mutex> lk(c.grow_mu);
        if (need <= g.cap) return true;
    }
    std::unique_lock<std::shared_mutex> lk(c.grow_mu);
    if (need <= g.cap) return true;
    // sizes in classes (steps of 2^(1/4)): which chunk arrives first, and with it the hint, differs from call to call, and
    // the pool hands a block back only to a request it fits (a fresh block of 100 MB costs ~10 ms of page faults)
    size_t cap = std::max(std::max(need + need / 8, g.cap + g.cap / 2), hint);
    if (cap > (1u << 20)) {
        size_t cls = (size_t)1 << 20;
        while (cls < cap) cls <<= 1;                       // 2^k >= cap
        const size_t q = cls / 8;                          // candidates: 5/8, 6/8, 7/8, 8/8 of 2^k
        for (size_t m8 = 5; m8 <= 8; m8++)
            if (q * m8 >= cap) { cap = q * m8; break; }
    }
    char* np = static_cast<char*>(pool.get(cap, false));
    if (!np) return false;
    const size_t used = std::min(g.hi.load(), g.cap);
    if (g.p && used) {
        const size_t CH = 1u << 22;
        parallel_for((used + CH - 1) / CH, [&](uint64_t i) { memcpy(np + i * CH, g.p + i * CH, std::min(CH, used - i * CH)); }, true);
    }
    pool.put(g.p);
    g.p = np;
    g.cap = cap;
    return true;
}

// What stage 1 learns about the chunk it stages, step by step
struct Chunk {
    uint64_t first = 0, n = 0;
    // Reverse-strand candidates (cand_reverse): the one-pair-per-lane kernels take the read's reverse complement on the DEVICE
    // from the one packed copy (scrg_params.stranded: the pair's descriptor carries the strand), so both strands of a read share
    // a row; the GenASM-row mappings get a row of their own, packed reverse-complemented here.
    bool dev_strand = false;
    bool linear = false;                   // contiguous rows (the GenASM-row kernels, lanes_per_pair >= 4) instead of lane-interleaved groups of 64
    // (best-candidate mode groups pairs by read.  The read row does that — a new row starts exactly where the read changes —
    // unless the rows are split by strand as well (GenASM-row mappings with cand_reverse): then the read index travels too)
    bool own_key = false;
    std::vector<uint32_t> row;             // mapping: the read row of every pair (one row per run of pairs with the same read)
    std::vector<uint64_t> row_pair;        // a pair that owns each row (its read is the row's content)
    uint64_t n_rows = 0, rw = 0, tw = 0, r_groups = 0, t_groups = 0, read_words = 0, text_words = 0, seq_words = 0;
    uint64_t cap = 0;                      // runs per slice (src/genasm_gpu.cu:906-911: 2 * read_len)
    // the device side
    uint64_t* d_seq = nullptr;
    char* d_pp = nullptr;                  // the per-pair results (PerPairLayout)
    size_t temp_bytes = 0;
    uint64_t rstride() const { return linear ? 1 : GROUP; }
};

struct RowCount {                          // what number_rows adds up over a chunk's pairs: rows started, the longest read and text
    uint64_t rows = 0, max_read = 0, max_text = 0;
    RowCount& operator+=(const RowCount& o)
    {
        rows += o.rows;
        max_read = std::max(max_read, o.max_read);
        max_text = std::max(max_text, o.max_text);
        return *this;
    }
};

// layout of the chunk's sequences: read rows (mapping: one row per run of pairs with the same read), text rows
void number_rows(const Call& c, Chunk& k)
{
    const scrg_host::Batch& b = *c.b;
    const uint64_t first = k.first, n = k.n;
    k.dev_strand = b.mapping && (b.cand_reverse || b.cand_leftward) && c.p.lanes_per_pair == 1;
    k.linear = c.p.lanes_per_pair != 1;
    k.own_key = c.best && b.cand_reverse && !k.dev_strand;
    k.row.resize(b.mapping ? n : 0);
    auto starts_row = [&](uint64_t i) -> bool {
        if (i == 0) return true;
        const uint64_t p = c.order[first + i], q = c.order[first + i - 1];
        return !(b.pair_read[q] == b.pair_read[p] &&
                 (k.dev_strand || (b.cand_reverse && b.cand_reverse[q]) == (b.cand_reverse && b.cand_reverse[p])));
    };
    const scrg_int::BlockScan<RowCount> scan(n, 1u << 14, c.threads_per_worker, [&](uint64_t i) {
        const uint64_t p = c.order[first + i];
        if (b.mapping) return RowCount{starts_row(i) ? 1u : 0u, b.read_lens[b.pair_read[p]], 0};
        return RowCount{0, b.read_lens[p], b.text_lens[p]};
    });
    if (b.mapping) {
        k.row_pair.resize(scan.total().rows);
        scan.place([&](uint64_t i, const RowCount& x) {
            const uint64_t st = starts_row(i) ? 1 : 0;
            if (st) k.row_pair[x.rows] = c.order[first + i];
            k.row[i] = (uint32_t)(x.rows + st - 1);
            return RowCount{st, 0, 0};
        });
    }
    const uint64_t max_read = scan.total().max_read, max_text = scan.total().max_text;
    k.n_rows = b.mapping ? k.row_pair.size() : n;
    k.rw = std::max<uint64_t>(1, (max_read + 31) / 32);
    k.tw = b.mapping ? 0 : std::max<uint64_t>(1, (max_text + 31) / 32);
    k.r_groups = (k.n_rows + GROUP - 1) / GROUP;
    k.t_groups = b.mapping ? 0 : (n + GROUP - 1) / GROUP;
    k.read_words = k.r_groups * GROUP * k.rw;
    k.text_words = k.t_groups * GROUP * k.tw;
    k.seq_words = k.read_words + k.text_words + SEQ_PAD;
    k.cap = (2 * max_read + 8 + 15) & ~(uint64_t)15;
}

// pack: one work item per group of 64 rows (the group's block of the interleaved layout is written by one thread; the GenASM-row
// kernels read contiguous rows instead)
scrg_status pack_chunk(DeviceState* ds, Slot& sl, const Call& c, const Chunk& k)
{
    const scrg_host::Batch& b = *c.b;
    const uint64_t first = k.first, n = k.n, r_groups = k.r_groups;
    if (k.seq_words > ds->slot_words) {
        ds->set_err("internal: chunk larger than its slot");
        return SCRG_ERR_INVALID_ARG;
    }
    HTRY(ds, sl.h_seq.ensure(k.seq_words * sizeof(uint64_t)));
    uint64_t* const h = static_cast<uint64_t*>(sl.h_seq.p);
    const bool linear = k.linear;
    std::atomic<int> bad{0};
    parallel_for(r_groups + k.t_groups, [&](uint64_t g) {
        const bool is_text = g >= r_groups;
        const uint64_t gi = is_text ? g - r_groups : g, W = is_text ? k.tw : k.rw;
        uint64_t* const blockp = h + (is_text ? k.read_words : 0) + gi * GROUP * W;
        const uint64_t rows_here = std::min<uint64_t>(GROUP, (is_text ? n : k.n_rows) - gi * GROUP);
        bool bd = false;
        // the rows of this group: source, length, strand
        const char* rsrc[GROUP];
        uint64_t rlen[GROUP];
        bool rrev[GROUP];
        for (uint64_t l = 0; l < GROUP; l++) {
            rsrc[l] = nullptr;
            rlen[l] = 0;
            rrev[l] = false;
            if (l >= rows_here) continue;
            const uint64_t r = gi * GROUP + l;
            if (is_text) {
                const uint64_t p = c.order[first + r];
                rsrc[l] = b.texts[p];
                rlen[l] = b.text_lens[p];
            } else if (b.mapping) {
                const uint64_t p = k.row_pair[r], rd = b.pair_read[p];
                rsrc[l] = b.reads[rd];
                rlen[l] = b.read_lens[rd];
                rrev[l] = !k.dev_strand && b.cand_reverse && b.cand_reverse[p];
            } else {
                const uint64_t p = c.order[first + r];
                rsrc[l] = b.reads[p];
                rlen[l] = b.read_lens[p];
            }
        }
        // short rows (reads of a mapper: a million separate strings) are cache misses, not bandwidth: ask for all of the
        // group's lines before the first one is needed
        if (W <= 16)
            for (uint64_t l = 0; l < rows_here; l++)
                for (uint64_t o = 0; o < rlen[l]; o += 64) __builtin_prefetch(rsrc[l] + o, 0, 0);
        for (uint64_t l0 = 0; l0 < GROUP; l0 += 8) {
            bool plain = !linear && g_have_avx2;
            for (uint64_t l = l0; l < l0 + 8; l++) plain = plain && !rrev[l] && (rlen[l] == 0 || rsrc[l] != nullptr);
            if (plain) {
                static const char none[1] = {0};
                const char* s8[8];
                for (int j = 0; j < 8; j++) s8[j] = rsrc[l0 + j] ? rsrc[l0 + j] : none;
                bd |= pack_rows8_avx2(s8, rlen + l0, blockp + l0, W);
            } else {
                for (uint64_t l = l0; l < l0 + 8; l++)
                    bd |= pack_sequence(rsrc[l] ? rsrc[l] : "", rlen[l], rrev[l], linear ? blockp + l * W : blockp + l, k.rstride(), W);
            }
        }
        if (bd) bad.store(1, std::memory_order_relaxed);
    }, true, c.threads_per_worker);
    for (uint64_t w = k.read_words + k.text_words; w < k.seq_words; w++) h[w] = 0;
    if (bad.load()) {
        ds->set_err("input contains characters other than ACGTacgt");
        return SCRG_ERR_BAD_BASE;
    }
    return SCRG_OK;
}

// per-pair scalars (MetaLayout): read length + text length | start in the genome and row word (+ the read index, own_key)
scrg_status fill_meta(DeviceState* ds, Slot& sl, const Call& c, const Chunk& k, const scrg::MetaLayout& meta)
{
    const scrg_host::Batch& b = *c.b;
    HTRY(ds, sl.h_meta.ensure(meta.bytes));
    char* const m = static_cast<char*>(sl.h_meta.p);
    uint32_t* const m_rl = reinterpret_cast<uint32_t*>(m + meta.o_read_len);
    uint32_t* const m_tl = reinterpret_cast<uint32_t*>(m + meta.o_text_len);
    uint64_t* const m_st = reinterpret_cast<uint64_t*>(m + meta.o_start);
    uint32_t* const m_key = reinterpret_cast<uint32_t*>(m + meta.o_key);
    parallel_for(k.n, [&](uint64_t i) {
        const uint64_t p = c.order[k.first + i];
        if (b.mapping) {
            m_rl[i] = (uint32_t)b.read_lens[b.pair_read[p]];
            // (a leftward candidate aligns the reverse complement of the read as its strand names it, against the reversed genome prefix)
            const bool rev = b.cand_reverse && b.cand_reverse[p], left = b.cand_leftward && b.cand_leftward[p];
            m_tl[i] = k.row[i] | ((k.dev_strand && rev != left) ? scrg::ROW_REVERSE : 0u) | (left ? scrg::ROW_LEFTWARD : 0u);
            m_st[i] = b.cand_start[p];
            if (k.own_key) m_key[i] = b.pair_read[p];
        } else {
            m_rl[i] = (uint32_t)b.read_lens[p];
            m_tl[i] = (uint32_t)std::min<uint64_t>(b.text_lens[p], 0xffffffffull);
        }
    }, false, c.threads_per_worker);
    return SCRG_OK;
}

// size the slot's device buffers, send sequences and scalars, build the descriptors
scrg_status size_and_upload(DeviceState* ds, Slot& sl, const Call& c, Chunk& k, const scrg::MetaLayout& meta)
{
    const scrg_host::Batch& b = *c.b;
    const uint64_t n = k.n;
    if (c.best && k.cap > scrg::WIRE_COUNT_MASK) {
        ds->set_err("SCRG_OUT_BEST: reads of 2^28 bases or more are not supported");
        return SCRG_ERR_INVALID_ARG;
    }
    const uint64_t slot_index = (uint64_t)(&sl - ds->slot);
    const uint64_t gpad = ds->genome_words ? ds->genome_words + SCRG_SEQ_PAD_WORDS : 0;
    const uint64_t base_word = gpad + slot_index * ds->slot_words;
    k.d_seq = ds->d_seq.as<uint64_t>();
    HTRY(ds, sl.d_meta.ensure(meta.bytes));
    HTRY(ds, sl.d_desc.ensure(n * sizeof(scrg_pair_desc)));
    if (!c.distance) HTRY(ds, sl.d_slices.ensure(n * k.cap * sizeof(scrg_run)));
    // the four per-pair result arrays sit back to back in one buffer, in the layout of the host staging area: ONE read-back
    // (a read-back of 1-2 MB runs at ~12 GB/s; six of them per chunk were 0.85 ms of 1.3 ms per 250 k mapping pairs)
    HTRY(ds, sl.d_ed.ensure(scrg::PerPairLayout(n).bytes + 256));
    k.d_pp = sl.d_ed.as<char>();
    HTRY(ds, sl.d_nruns.ensure(n * 4));
    HTRY(ds, sl.d_cnt64.ensure(n * 8));
    HTRY(ds, sl.d_len64.ensure(std::max<size_t>(n * 8, c.best ? scrg::select_scratch_bytes(n) : 0)));
    HTRY(ds, sl.d_tot.ensure(16));
    k.temp_bytes = scrg::host_scan_temp_bytes(n + 1);      // (n + 1: the difference strings' offsets end with their total)
    HTRY(ds, sl.d_temp.ensure(k.temp_bytes + 256));
    HTRY(ds, sl.h_tot.ensure(32));
    if (c.opt.diff_kind) {
        HTRY(ds, sl.d_dlen.ensure((n + 2) * 8));
        HTRY(ds, sl.d_doff.ensure((n + 2) * 8));
    }
    for (int kind = 0; kind < N_REC; kind++)
        if (c.rec_on(kind)) HTRY(ds, sl.rec[kind].d.ensure(n * REC_SIZE[kind] + 256));
    HTRY(ds, hipMemcpyAsync(k.d_seq + base_word, sl.h_seq.p, k.seq_words * sizeof(uint64_t), hipMemcpyHostToDevice, sl.stream));
    HTRY(ds, hipMemcpyAsync(sl.d_meta.p, sl.h_meta.p, meta.bytes, hipMemcpyHostToDevice, sl.stream));
    const char* const d_meta = sl.d_meta.as<char>();
    scrg::HostDescArgs da{};
    da.n = n;
    da.desc = sl.d_desc.as<scrg_pair_desc>();
    da.read_len = reinterpret_cast<const uint32_t*>(d_meta + meta.o_read_len);
    da.text_len = b.mapping ? nullptr : reinterpret_cast<const uint32_t*>(d_meta + meta.o_text_len);
    da.row = b.mapping ? reinterpret_cast<const uint32_t*>(d_meta + meta.o_text_len) : nullptr;
    da.start = b.mapping ? reinterpret_cast<const uint64_t*>(d_meta + meta.o_start) : nullptr;
    da.genome_len = ds->genome_len;
    da.read_base = base_word;
    da.read_words = k.rw;
    da.text_base = base_word + k.read_words;
    da.text_words = k.tw;
    da.cap = k.cap;
    da.linear = k.linear ? 1u : 0u;
    HTRY(ds, scrg::launch_build_desc(da, sl.stream));
    return SCRG_OK;
}

// best-candidate mode: the losers of every read lose their runs before the counts are summed (d_len64 is free until
// text_len_kernel: scratch).  Pairs are grouped by the row word's row, or by the read index where that travels (own_key).
hipError_t select_best(Slot& sl, const Chunk& k, const scrg::MetaLayout& meta)
{
    const char* const d_meta = sl.d_meta.as<char>();
    return scrg::launch_select_best(k.n, reinterpret_cast<const uint32_t*>(d_meta + (k.own_key ? meta.o_key : meta.o_text_len)),
                                    k.own_key ? 0xffffffffu : scrg::ROW_INDEX_MASK, reinterpret_cast<int64_t*>(k.d_pp),
                                    reinterpret_cast<uint32_t*>(k.d_pp + scrg::PerPairLayout(k.n).o_st), sl.d_nruns.as<uint32_t>(), nullptr, sl.d_len64.p,
                                    sl.stream);
}

// a paired call: the chunk's mate pairs' offsets and the pairs' strands go up, the selection kernel runs with the team size the
// offsets ask for, and its records are left on the device for the read-back (d_nruns as for select_best)
scrg_status select_mates(DeviceState* ds, Slot& sl, const Call& c, const Chunk& k, const scrg::MetaLayout& meta)
{
    const scrg_host::Batch& b = *c.b;
    const uint64_t k0 = (uint64_t)(std::lower_bound(c.mate_start.begin(), c.mate_start.end(), k.first) - c.mate_start.begin());
    const uint64_t k1 = (uint64_t)(std::lower_bound(c.mate_start.begin(), c.mate_start.end(), k.first + k.n) - c.mate_start.begin());
    if (k0 >= c.mate_start.size() || c.mate_start[k0] != k.first || k1 >= c.mate_start.size() || c.mate_start[k1] != k.first + k.n) {
        ds->set_err("internal: a chunk of a paired call does not hold whole mate pairs");
        return SCRG_ERR_INVALID_ARG;
    }
    const uint64_t nm = sl.n_mates = k1 - k0;
    sl.mate0 = k0;
    const MatesLayout ml(k.n, nm);
    HTRY(ds, sl.h_mates.ensure(ml.o_rec));
    HTRY(ds, sl.d_mates.ensure(ml.bytes));
    char* const h = static_cast<char*>(sl.h_mates.p);
    uint64_t* const first = reinterpret_cast<uint64_t*>(h);
    uint64_t most = 1;
    for (uint64_t i = 0; i < nm; i++) {
        const uint64_t a0 = c.mate_start[k0 + i], b0 = c.mate_b[k0 + i], e = c.mate_start[k0 + i + 1];
        first[2 * i] = a0 - k.first;
        first[2 * i + 1] = b0 - k.first;
        most = std::max(most, std::min<uint64_t>(64, (b0 - a0) * std::min<uint64_t>(64, e - b0)));
    }
    first[2 * nm] = k.n;
    if (b.cand_reverse) {
        uint8_t* const rev = reinterpret_cast<uint8_t*>(h + ml.o_rev);
        parallel_for(k.n, [&](uint64_t i) { rev[i] = b.cand_reverse[c.order[k.first + i]] ? 1 : 0; }, false, c.threads_per_worker);
    }
    char* const d = sl.d_mates.as<char>();
    HTRY(ds, hipMemcpyAsync(d, h, b.cand_reverse ? ml.o_rev + k.n : 8 * (2 * nm + 1), hipMemcpyHostToDevice, sl.stream));
    const char* const d_meta = sl.d_meta.as<char>();
    HTRY(ds, scrg::launch_select_mates(*b.mate_rule, scrg::mate_team_size(most), nullptr, nm, reinterpret_cast<const uint64_t*>(d),
                                       reinterpret_cast<const uint64_t*>(d_meta + meta.o_start), reinterpret_cast<const uint32_t*>(d_meta + meta.o_read_len),
                                       b.cand_reverse ? reinterpret_cast<const uint8_t*>(d + ml.o_rev) : nullptr, reinterpret_cast<const int64_t*>(k.d_pp),
                                       reinterpret_cast<uint32_t*>(k.d_pp + scrg::PerPairLayout(k.n).o_st), sl.d_nruns.as<uint32_t>(), nullptr,
                                       reinterpret_cast<scrg_mate_record*>(d + ml.o_rec), sl.stream));
    return SCRG_OK;
}

// the chunk's records on their way back (before ev_done is recorded)
scrg_status read_back_mates(DeviceState* ds, Slot& sl)
{
    const MatesLayout ml(sl.n, sl.n_mates);
    const size_t bytes = (32 * sl.n_mates + 255) & ~(size_t)255;
    HTRY(ds, sl.h_mrec.ensure(bytes));
    HTRY(ds, hipMemcpyAsync(sl.h_mrec.p, sl.d_mates.as<char>() + ml.o_rec, bytes, hipMemcpyDeviceToHost, sl.stream));
    return SCRG_OK;
}

// ... and into the call's array: by mate pair, the winners as the caller's pair indices
void collect_mates(const Slot& sl, Call& c)
{
    const scrg_mate_record* const got = static_cast<const scrg_mate_record*>(sl.h_mrec.p);
    parallel_for(sl.n_mates, [&](uint64_t i) {
        scrg_mate_record r = got[i];
        for (uint64_t& w : r.winner)
            if (w != scrg::MATE_NONE) w = c.order[sl.first + w];
        c.mate_rec[c.mate_id[sl.mate0 + i]] = r;
    }, false, c.threads_per_worker);
}

// the read summary's per-chunk buffers: [first 8 (nr + 1) | records 32 nr | keep status 4 n] on the device, the first uploaded
struct SummaryLayout {
    size_t o_rec, o_keep, bytes;
    SummaryLayout(uint64_t n, uint64_t nr) : o_rec((8 * (nr + 1) + 255) & ~(size_t)255), o_keep((o_rec + 32 * nr + 255) & ~(size_t)255), bytes(o_keep + 4 * n + 256) {}
};

// the read summary: the chunk's reads' offsets go up (8 bytes per read, as select_mates sends its), the kernel runs behind the
// selection, and its records are left on the device for the read-back.  With the keep filter on, the statuses' copy is made too.
scrg_status read_summary(DeviceState* ds, Slot& sl, const Call& c, const Chunk& k, const scrg::MetaLayout& meta)
{
    const uint64_t k0 = (uint64_t)(std::lower_bound(c.sum_start.begin(), c.sum_start.end(), k.first) - c.sum_start.begin());
    const uint64_t k1 = (uint64_t)(std::lower_bound(c.sum_start.begin(), c.sum_start.end(), k.first + k.n) - c.sum_start.begin());
    if (k0 >= c.sum_start.size() || c.sum_start[k0] != k.first || k1 >= c.sum_start.size() || c.sum_start[k1] != k.first + k.n) {
        ds->set_err("internal: a chunk of a call with the read summary does not hold whole reads");
        return SCRG_ERR_INVALID_ARG;
    }
    const uint64_t nr = sl.n_sum = k1 - k0;
    sl.sum0 = k0;
    const SummaryLayout ml(k.n, nr);
    HTRY(ds, sl.h_sum.ensure(ml.o_rec));
    HTRY(ds, sl.d_sum.ensure(ml.bytes));
    uint64_t* const first = static_cast<uint64_t*>(sl.h_sum.p);
    for (uint64_t i = 0; i <= nr; i++) first[i] = c.sum_start[k0 + i] - k.first;
    char* const d = sl.d_sum.as<char>();
    HTRY(ds, hipMemcpyAsync(d, first, 8 * (nr + 1), hipMemcpyHostToDevice, sl.stream));
    HTRY(ds, scrg::launch_read_summary(c.opt.mapq_rule, nr, k.n, reinterpret_cast<const uint64_t*>(d),
                                       reinterpret_cast<const uint32_t*>(sl.d_meta.as<char>() + meta.o_read_len), reinterpret_cast<const int64_t*>(k.d_pp),
                                       reinterpret_cast<const uint32_t*>(k.d_pp + scrg::PerPairLayout(k.n).o_st), reinterpret_cast<scrg_read_record*>(d + ml.o_rec),
                                       c.keep_filter() ? reinterpret_cast<uint32_t*>(d + ml.o_keep) : nullptr, sl.stream));
    return SCRG_OK;
}

// the chunk's records on their way back (before ev_done is recorded)
scrg_status read_back_summary(DeviceState* ds, Slot& sl)
{
    const SummaryLayout ml(sl.n, sl.n_sum);
    const size_t bytes = (32 * sl.n_sum + 255) & ~(size_t)255;
    HTRY(ds, sl.h_srec.ensure(bytes));
    HTRY(ds, hipMemcpyAsync(sl.h_srec.p, sl.d_sum.as<char>() + ml.o_rec, bytes, hipMemcpyDeviceToHost, sl.stream));
    return SCRG_OK;
}

// ... and into the call's array: by read, the winner as the caller's pair index (as collect_mates)
void collect_summary(const Slot& sl, Call& c)
{
    const scrg_read_record* const got = static_cast<const scrg_read_record*>(sl.h_srec.p);
    parallel_for(sl.n_sum, [&](uint64_t i) {
        scrg_read_record r = got[i];
        if (r.winner != scrg::MAPQ_NONE) r.winner = c.order[sl.first + r.winner];
        c.sum_rec[c.sum_id[sl.sum0 + i]] = r;
    }, false, c.threads_per_worker);
}

// runs and / or text: align, select, lay the results out (sizes come back through ev_tot; stage 2 goes on from there)
scrg_status enqueue_runs(DeviceState* ds, Slot& sl, const Call& c, const Chunk& k, const scrg::MetaLayout& meta, const scrg_params& pp)
{
    const uint64_t n = k.n;
    const scrg::PerPairLayout lay(n);
    int64_t* const d_ed = reinterpret_cast<int64_t*>(k.d_pp);
    uint32_t* const d_status = reinterpret_cast<uint32_t*>(k.d_pp + lay.o_st);
    const scrg_pair_desc* const d_desc = sl.d_desc.as<scrg_pair_desc>();
    CTRY(ds, sl, scrg_align_device(sl.ctx, &pp, n, k.d_seq, d_desc, sl.d_slices.as<scrg_run>(), d_ed, sl.d_nruns.as<uint32_t>(), d_status));
    // (the compaction, the rendering and both read-backs then carry the winners only)
    if (c.mates) {
        const scrg_status s = select_mates(ds, sl, c, k, meta);
        if (s != SCRG_OK) return s;
    } else if (c.best) {
        HTRY(ds, select_best(sl, k, meta));
    }
    if (c.summary) {
        const scrg_status s = read_summary(ds, sl, c, k, meta);
        if (s != SCRG_OK) return s;
    }
    // soft clipping, in apply mode on the slices and descriptors: everything from here on — the layout, the compaction, the wire,
    // the text in every form — works on the kept runs (a loser of the selection, a pair over its limit and an overflowed slice
    // are not looked at)
    if (c.opt.clip)
        CTRY(ds, sl, scrg_clip_device(sl.ctx, &pp, n, SLOT_RUNS(sl), d_status, c.opt.clip_costs, 1, sl.rec[REC_CLIP].d.as<scrg_pair_clip>()));
    HTRY(ds, scrg::launch_result_layout(n, sl.d_desc.as<scrg_pair_desc>(), sl.d_slices.as<uint16_t>(), sl.d_nruns.as<uint32_t>(), d_ed, d_status,
                                        sl.d_cnt64.as<uint64_t>(), sl.d_len64.as<uint64_t>(), reinterpret_cast<uint64_t*>(k.d_pp + lay.o_ro),
                                        reinterpret_cast<uint64_t*>(k.d_pp + lay.o_to), sl.d_tot.as<uint64_t>(),
                                        reinterpret_cast<uint32_t*>(k.d_pp + lay.o_wire), sl.d_temp.p, k.temp_bytes, c.want_text, c.opt.cigar_form, ds->n_cus, sl.stream));
    HTRY(ds, hipMemcpyAsync(sl.h_tot.p, sl.d_tot.p, 16, hipMemcpyDeviceToHost, sl.stream));
    // the alignment report, from the slices: after the selection, so that a loser has no alignment (leftward candidates are served)
    if (c.opt.report)
        CTRY(ds, sl, scrg_report_device(sl.ctx, &pp, n, k.d_seq, d_desc, SLOT_RUNS(sl), d_ed, d_status, sl.rec[REC_REPORT].d.as<scrg_pair_report>(), nullptr));
    if (c.opt.pileup) {
        // the pileup: every OK pair of the chunk at its candidate's start, summed into the state's accumulator (chunks on other slots
        // add at the same time: atomics); after the selection, so that only the winners pile up — with min_keep_q > 0 the winners of
        // KEPT reads only: the statuses' copy the summary kernel made (everything else goes on reading d_status)
        const uint32_t* const d_pile_status =
            c.keep_filter() ? reinterpret_cast<const uint32_t*>(sl.d_sum.as<char>() + SummaryLayout(n, sl.n_sum).o_keep) : d_status;
        const scrg::PairRuns pr{n, k.d_seq, d_desc, sl.d_slices.as<uint16_t>(), &d_desc->cigar_off, 6, sl.d_nruns.as<uint32_t>(),
                                (uint32_t)std::max(1, pp.text_stride_words), (uint32_t)std::max(1, pp.read_stride_words), pp.stranded ? 1u : 0u};
        uint32_t* const counters = ds->d_pile.as<uint32_t>() + scrg::PILE_PLANES * (ds->pile_len + 1);
        HTRY(ds, scrg::launch_pileup_add(pr, d_pile_status, reinterpret_cast<const uint64_t*>(sl.d_meta.as<char>() + meta.o_start), ds->pile_len,
                                         ds->d_pile.as<uint32_t>(), counters, counters + 1, ds->n_cus, sl.stream));
    }
    if (c.opt.diff_kind) {
        // difference strings: the lengths from the slices (the losers of best-candidate mode have no runs any more), the offsets,
        // and the total as a third size for stage 2
        CTRY(ds, sl, scrg_diff_lengths(sl.ctx, &pp, c.opt.diff_kind, n, k.d_seq, d_desc, SLOT_RUNS(sl), sl.d_dlen.as<uint64_t>()));
        HTRY(ds, scrg::launch_diff_offsets(n, sl.d_dlen.as<uint64_t>(), sl.d_doff.as<uint64_t>(), sl.d_temp.p, k.temp_bytes, sl.stream));
        HTRY(ds, hipMemsetAsync(sl.d_doff.as<uint64_t>() + n + 1, 0, 8, sl.stream));       // (the render pass's bad count)
        HTRY(ds, hipMemcpyAsync(static_cast<char*>(sl.h_tot.p) + 16, sl.d_doff.as<uint64_t>() + n, 8, hipMemcpyDeviceToHost, sl.stream));
    }
    HTRY(ds, hipEventRecord(sl.ev_tot, sl.stream));
    return SCRG_OK;
}

// Distance-only mode: [ed 8n | status 4n | text end 4n] (PerPairLayout) is all a chunk produces, and it comes back as it is — one
// read-back of 16 bytes per pair, enqueued here: there are no sizes to wait for (stage 2 only publishes zero totals).
scrg_status enqueue_distance(DeviceState* ds, Slot& sl, const Call& c, const Chunk& k, const scrg::MetaLayout& meta, const scrg_params& pp)
{
    const uint64_t n = k.n;
    const scrg::PerPairLayout lay(n);
    CTRY(ds, sl, scrg_align_device_distance(sl.ctx, &pp, n, k.d_seq, sl.d_desc.as<scrg_pair_desc>(), reinterpret_cast<int64_t*>(k.d_pp),
                                            reinterpret_cast<uint32_t*>(k.d_pp + lay.o_tend), reinterpret_cast<uint32_t*>(k.d_pp + lay.o_st)));
    if (c.best) {                    // (the selection wants run counts to clear: there are none)
        HTRY(ds, hipMemsetAsync(sl.d_nruns.p, 0, n * 4, sl.stream));
        if (c.mates) {
            scrg_status s = select_mates(ds, sl, c, k, meta);
            if (s == SCRG_OK) s = read_back_mates(ds, sl);
            if (s != SCRG_OK) return s;
        } else {
            HTRY(ds, select_best(sl, k, meta));
        }
    }
    if (c.summary) {
        scrg_status s = read_summary(ds, sl, c, k, meta);
        if (s == SCRG_OK) s = read_back_summary(ds, sl);
        if (s != SCRG_OK) return s;
    }
    HTRY(ds, sl.h_out.ensure(lay.distance_bytes + 512));
    HTRY(ds, hipMemcpyAsync(sl.h_out.p, k.d_pp, (lay.distance_bytes + 255) & ~(size_t)255, hipMemcpyDeviceToHost, sl.stream));
    HTRY(ds, hipEventRecord(sl.ev_tot, sl.stream));
    HTRY(ds, hipEventRecord(sl.ev_done, sl.stream));
    return SCRG_OK;
}

// stage 1: pack the chunk, send it, align it, lay its results out
scrg_status stage1(DeviceState* ds, Slot& sl, Call& c, uint64_t chunk)
{
    Chunk k;
    k.first = sl.first = c.chunk_first[chunk];
    k.n = sl.n = c.chunk_first[chunk + 1] - k.first;
    const int64_t t0 = now_ns();
    HTRY(ds, hipSetDevice(ds->device));
    number_rows(c, k);
    scrg_status s = pack_chunk(ds, sl, c, k);
    if (s != SCRG_OK) return s;
    const scrg::MetaLayout meta(k.n, c.b->mapping, k.own_key);
    s = fill_meta(ds, sl, c, k, meta);
    if (s != SCRG_OK) return s;
    sl.t_pack_ns = now_ns() - t0;
    s = size_and_upload(ds, sl, c, k, meta);
    if (s != SCRG_OK) return s;
    scrg_params pp = c.p;
    pp.read_stride_words = (int32_t)k.rstride();
    pp.text_stride_words = c.b->mapping ? 1 : (int32_t)k.rstride();
    pp.stranded = k.dev_strand ? 1 : 0;
    sl.pp = pp;
    // (the slot's own handle: both set for every chunk, so nothing to restore)
    CTRY(ds, sl, scrg_ctx_set_edit_limit(sl.ctx, c.opt.max_edits, c.opt.per_mille));
    CTRY(ds, sl, scrg_ctx_set_text_strands(sl.ctx, c.b->cand_leftward ? 1 : 0));
    return c.distance ? enqueue_distance(ds, sl, c, k, meta, pp) : enqueue_runs(ds, sl, c, k, meta, pp);
}

// stage 2: the sizes are known — compact the runs, render the text, bring everything back
scrg_status stage2(DeviceState* ds, Slot& sl, Call& c, uint64_t chunk)
{
    HTRY(ds, hipSetDevice(ds->device));
    HTRY(ds, hipEventSynchronize(sl.ev_tot));
    const uint64_t* const tot = static_cast<const uint64_t*>(sl.h_tot.p);
    sl.tot_runs = c.distance ? 0 : tot[0];       // (distance-only mode: no runs, no text, and nobody wrote h_tot)
    sl.tot_text = c.distance ? 0 : tot[1];
    sl.tot_diff = c.opt.diff_kind ? tot[2] : 0;
    {
        std::lock_guard<std::mutex> g(c.tot_mu);
        c.c_runs[chunk] = sl.tot_runs;
        c.c_text[chunk] = sl.tot_text;
        c.c_diff[chunk] = sl.tot_diff;
        c.c_known[chunk] = 1;
    }
    c.tot_cv.notify_all();
    float ms = 0.f;
    if (scrg_last_kernel_ms(sl.ctx, &ms) == SCRG_OK) c.kernel_ns.fetch_add((int64_t)((double)ms * 1e6));
    c.pack_ns.fetch_add(sl.t_pack_ns);
    if (c.distance) return SCRG_OK;          // (the chunk's read-back was enqueued with its kernel)
    const uint64_t n = sl.n;
    // host staging of a chunk: [wire: ed 4n | run count + flags 4n | text length 4n (absent without text)] [runs 2R (+pad)]
    // [text T] (PerPairLayout: host_runs() follows from wire_bytes); on the device the per-pair arrays are one buffer
    // and runs + text another: two read-backs per chunk, the first of the wire only
    const scrg::PerPairLayout lay(n);
    const size_t o_runs = lay.host_runs(), text_rel = (2 * sl.tot_runs + 15) & ~(size_t)15;
    const size_t o_text = o_runs + text_rel, total = o_text + sl.tot_text + 512;
    HTRY(ds, sl.h_out.ensure(total));
    char* const h = static_cast<char*>(sl.h_out.p);
    HTRY(ds, sl.d_dense.ensure(text_rel + (c.want_text ? sl.tot_text : 0) + 512));
    char* const d_pp = sl.d_ed.as<char>();
    uint64_t* const d_runoff = reinterpret_cast<uint64_t*>(d_pp + lay.o_ro);
    uint64_t* const d_textoff = reinterpret_cast<uint64_t*>(d_pp + lay.o_to);
    uint8_t* const d_text = sl.d_dense.as<uint8_t>() + text_rel;
    CTRY(ds, sl, scrg_compact_runs(sl.ctx, n, sl.d_desc.as<scrg_pair_desc>(), sl.d_slices.as<scrg_run>(), sl.d_nruns.as<uint32_t>(), d_runoff,
                                   sl.d_dense.as<scrg_run>()));
    if (c.want_text)
        HTRY(ds, scrg::launch_render_text(n, sl.d_dense.as<uint16_t>(), d_runoff, sl.d_cnt64.as<uint64_t>(), d_textoff, d_text, c.opt.cigar_form, ds->n_cus, sl.stream));
    // (whole multiples of 256 bytes to page-aligned host addresses: the buffers have the slack)
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    HTRY(ds, hipMemcpyAsync(h, d_pp + lay.o_wire, up(c.want_text ? 12 * n : 8 * n), hipMemcpyDeviceToHost, sl.stream));
    if (c.want_runs && c.want_text && sl.tot_runs + sl.tot_text)
        HTRY(ds, hipMemcpyAsync(h + o_runs, sl.d_dense.p, up(text_rel + sl.tot_text), hipMemcpyDeviceToHost, sl.stream));
    else if (c.want_runs && sl.tot_runs)
        HTRY(ds, hipMemcpyAsync(h + o_runs, sl.d_dense.p, up(2 * sl.tot_runs), hipMemcpyDeviceToHost, sl.stream));
    else if (c.want_text && sl.tot_text)
        HTRY(ds, hipMemcpyAsync(h + o_text, d_text, up(sl.tot_text), hipMemcpyDeviceToHost, sl.stream));
    if (c.opt.diff_kind) {
        // the difference strings, from the slices and the chunk's sequences (both stay until the slot's next chunk): [offsets and
        // the bad count | text] come back in a staging area of their own
        const size_t off_bytes = up(8 * (n + 2));
        HTRY(ds, sl.d_dtext.ensure(sl.tot_diff + 512));
        HTRY(ds, sl.h_diff.ensure(off_bytes + sl.tot_diff + 512));
        CTRY(ds, sl, scrg_diff_render(sl.ctx, &sl.pp, c.opt.diff_kind, n, ds->d_seq.as<uint64_t>(), sl.d_desc.as<scrg_pair_desc>(), SLOT_RUNS(sl),
                                      sl.d_dlen.as<uint64_t>(), sl.d_doff.as<uint64_t>(), sl.d_dtext.as<char>(), sl.tot_diff,
                                      reinterpret_cast<uint32_t*>(sl.d_doff.as<uint64_t>() + n + 1)));
        HTRY(ds, hipMemcpyAsync(sl.h_diff.p, sl.d_doff.p, 8 * (n + 2), hipMemcpyDeviceToHost, sl.stream));
        if (sl.tot_diff) HTRY(ds, hipMemcpyAsync(static_cast<char*>(sl.h_diff.p) + off_bytes, sl.d_dtext.p, up(sl.tot_diff), hipMemcpyDeviceToHost, sl.stream));
    }
    for (int kind = 0; kind < N_REC; kind++) {       // the records of every kind that is on, each in a staging area of its own
        if (!c.rec_on(kind)) continue;
        RecordBuf& rb = sl.rec[kind];
        HTRY(ds, rb.h.ensure(up(n * REC_SIZE[kind]) + 256));
        HTRY(ds, hipMemcpyAsync(rb.h.p, rb.d.p, up(n * REC_SIZE[kind]), hipMemcpyDeviceToHost, sl.stream));
    }
    if (c.mates) {
        const scrg_status s = read_back_mates(ds, sl);
        if (s != SCRG_OK) return s;
    }
    if (c.summary) {
        const scrg_status s = read_back_summary(ds, sl);
        if (s != SCRG_OK) return s;
    }
    HTRY(ds, hipEventRecord(sl.ev_done, sl.stream));
    return SCRG_OK;
}

// A chunk's piece of a byte stream (the runs as 2-byte items, the CIGAR text, the difference text) on its way from the slot's
// staging area to its place in the call's array
struct Piece {
    Grow* g;
    size_t base, bytes;                    // where the chunk's bytes go: everything the chunks before it produced
    const char* src;
    size_t slack;                          // room kept behind the piece (a terminator)
    scrg_int::ResultPool* pool;
};

// Grows each array to hold its piece at its base, raises `hi`, and copies all pieces in chunks of 512 KB in one dispatch, under the
// shared lock.  false: out of memory.
bool place_pieces(Call& c, const Piece* pc, int n_pieces, double per_pair_scale)
{
    constexpr size_t CH = 1u << 19;
    uint64_t first[4] = {0};               // the first work item of every piece, and their number
    for (int k = 0; k < n_pieces; k++) {
        if (!grow_to(c, *pc[k].g, pc[k].base + pc[k].bytes + pc[k].slack, (size_t)((double)pc[k].bytes * per_pair_scale) + 4096, *pc[k].pool)) return false;
        first[k + 1] = first[k] + (pc[k].bytes + CH - 1) / CH;
    }
    std::shared_lock<std::shared_mutex> lk(c.grow_mu);
    for (int k = 0; k < n_pieces; k++) {
        std::atomic<size_t>& hi = pc[k].g->hi;
        size_t cur = hi.load();
        while (cur < pc[k].base + pc[k].bytes && !hi.compare_exchange_weak(cur, pc[k].base + pc[k].bytes)) {}
    }
    parallel_for(first[n_pieces], [&](uint64_t i) {
        int k = 0;
        while (i >= first[k + 1]) k++;
        const size_t at = (i - first[k]) * CH;
        memcpy(pc[k].g->p + pc[k].base + at, pc[k].src + at, std::min(CH, pc[k].bytes - at));
    }, true, c.threads_per_worker);
    return true;
}

// distance-only mode's stage 3: [ed 8n | status 4n | text end 4n] as the kernels left them (status: done, over the edit limit, not the read's best)
void collect_distance(const Slot& sl, Call& c)
{
    const uint64_t n = sl.n, first = sl.first;
    const scrg::PerPairLayout lay(n);
    const char* const hd = static_cast<const char*>(sl.h_out.p);
    const int64_t* const h_ed = reinterpret_cast<const int64_t*>(hd);
    const uint32_t* const h_st = reinterpret_cast<const uint32_t*>(hd + lay.o_st);
    const uint32_t* const h_te = reinterpret_cast<const uint32_t*>(hd + lay.o_tend);
    parallel_for(n, [&](uint64_t i) {
        c.iss_ed[first + i] = h_ed[i];
        c.iss_status[first + i] = scrg::public_status(h_st[i]);
        c.iss_tend[first + i] = h_st[i] == scrg::LANE_STATUS_DONE ? (uint64_t)h_te[i] : 0ull;
        c.iss_run_off[first + i] = 0;
        c.iss_text_off[first + i] = 0;
    }, false, c.threads_per_worker);
}

struct RunsText {                          // a pair's or a chunk's runs and text bytes
    uint64_t runs = 0, text = 0;
    RunsText& operator+=(const RunsText& o)
    {
        runs += o.runs;
        text += o.text;
        return *this;
    }
};

// stage 3: the chunk's results go to their place in the (issue order) result arrays
scrg_status stage3(DeviceState* ds, Slot& sl, Call& c, uint64_t chunk)
{
    HTRY(ds, hipSetDevice(ds->device));
    HTRY(ds, hipEventSynchronize(sl.ev_done));
    // bases: everything the chunks before this one produced
    uint64_t base_runs = 0, base_text = 0, base_diff = 0;
    {
        std::unique_lock<std::mutex> lk(c.tot_mu);
        c.tot_cv.wait(lk, [&] {
            if (c.failed()) return true;
            for (uint64_t k = 0; k < chunk; k++)
                if (!c.c_known[k]) return false;
            return true;
        });
        if (c.failed()) return (scrg_status)c.status.load();
        for (uint64_t k = 0; k < chunk; k++) {
            base_runs += c.c_runs[k];
            base_text += c.c_text[k];
            base_diff += c.c_diff[k];
        }
    }
    const uint64_t n = sl.n, first = sl.first;
    if (c.mates) collect_mates(sl, c);
    if (c.summary) collect_summary(sl, c);
    if (c.distance) {
        collect_distance(sl, c);
        return SCRG_OK;
    }
    const scrg::PerPairLayout lay(n);
    const size_t o_runs = lay.host_runs();
    const size_t o_text = o_runs + ((2 * sl.tot_runs + 15) & ~(size_t)15);
    const char* const h = static_cast<const char*>(sl.h_out.p);
    const double per_pair_scale = 1.08 * (double)c.n / (double)std::max<uint64_t>(1, n);
    // (the runs are a byte stream of 2-byte items; both streams go in one dispatch)
    Piece pieces[2];
    int n_pieces = 0;
    if (c.want_runs) pieces[n_pieces++] = Piece{&c.runs, 2 * base_runs, 2 * sl.tot_runs, h + o_runs, 2, &g_pool};
    if (c.want_text) pieces[n_pieces++] = Piece{&c.text, base_text, sl.tot_text, h + o_text, 1, &g_pool};
    if (!place_pieces(c, pieces, n_pieces, per_pair_scale)) return SCRG_ERR_OOM;
    // the wire (PerPairLayout): edit distances, run counts with their flags, text lengths; the offsets are their prefix sums
    const uint32_t* const w_ed = reinterpret_cast<const uint32_t*>(h);
    const uint32_t* const w_cnt = w_ed + n;
    const uint32_t* const w_len = w_cnt + n;
    auto sizes = [&](uint64_t i) { return RunsText{w_cnt[i] & scrg::WIRE_COUNT_MASK, c.want_text ? w_len[i] : 0u}; };
    const scrg_int::BlockScan<RunsText> scan(n, 1u << 14, c.threads_per_worker, sizes);
    std::atomic<int> ovf{0};
    scan.place([&](uint64_t i, const RunsText& x) {
        const uint32_t cw = w_cnt[i];
        c.iss_ed[first + i] = (int64_t)w_ed[i];
        c.iss_status[first + i] = scrg::wire_pair_status(cw);
        if (scrg::wire_overflowed(cw)) ovf.store(1, std::memory_order_relaxed);
        c.iss_run_off[first + i] = base_runs + x.runs;
        c.iss_text_off[first + i] = c.want_text ? base_text + x.text : 0;
        return sizes(i);
    });
    if (scan.total().runs != sl.tot_runs || (c.want_text && scan.total().text != sl.tot_text)) {
        ds->set_err("internal: a chunk's per-pair sizes do not add up to its totals");
        return SCRG_ERR_HIP;
    }
    if (ovf.load()) c.any_overflow.store(1);
    if (c.opt.diff_kind) {
        // difference strings: [offsets 8 (n + 1), the render pass's bad count | text]; the offsets get the chunks' base
        const char* const hd = static_cast<const char*>(sl.h_diff.p);
        const uint64_t* const d_off = reinterpret_cast<const uint64_t*>(hd);
        const size_t off_bytes = (8 * (n + 2) + 255) & ~(size_t)255;
        if (d_off[n] != sl.tot_diff || (uint32_t)d_off[n + 1] != 0) {
            ds->set_err("internal: a chunk's difference strings do not add up to their total, or a pair's runs do not fit its sequences");
            return SCRG_ERR_HIP;
        }
        const Piece text{&c.diff, base_diff, sl.tot_diff, hd + off_bytes, 1, &g_diff_pool};
        if (!place_pieces(c, &text, 1, per_pair_scale)) return SCRG_ERR_OOM;
        parallel_for(n, [&](uint64_t i) { c.iss_diff_off[first + i] = base_diff + d_off[i]; }, false, c.threads_per_worker);
    }
    for (int kind = 0; kind < N_REC; kind++)
        if (c.rec_on(kind)) memcpy(c.iss_rec[kind] + first * REC_SIZE[kind], sl.rec[kind].h.p, n * REC_SIZE[kind]);
    return SCRG_OK;
}

// One device: a LAUNCH thread packs chunk i, sends it and starts its kernels; the sizes of an earlier chunk are looked at
// as soon as they have arrived (without waiting, unless the chunk is LAG2 launches behind) and its compaction, rendering
// and read-back are started; two COLLECT threads put finished chunks into the result arrays.  A slot is reused n_slots
// chunks later, once its previous chunk has been collected.  n_slots is 4 for long reads — the align kernel of a chunk of
// 10 kb reads takes ~2 ms however small the chunk is (~330 dependent window rounds), and HIP has four hardware queues —
// and 8 for short ones, where a chunk's kernels take ~0.5 ms and what limits the call is how soon a slot comes back
// (1 M x 4 mapping pairs: 21 ms with four slots, 16 ms with eight; the read-back alone is 11.5 ms at PCIe rate).
void worker(DeviceState* ds, Call* c, int dev_index, int n_dev)
{
    std::vector<uint64_t> mine;
    const uint64_t n_chunks = c->chunk_first.size() - 1;
    for (uint64_t k = dev_index; k < n_chunks; k += n_dev) mine.push_back(k);
    const size_t m = mine.size();
    const bool timing = getenv("SCRG_HOST_TIMING") != nullptr;
    // a call whose chunks all have a slot launches every one of them before it waits for the first (a chunk's kernel takes
    // ~2 ms for 10 kb reads however small the chunk); a longer call keeps one slot of slack between launch and collection
    const size_t NS = (size_t)c->n_slots;
    const size_t LAG2 = m <= NS ? NS - 1 : (NS > (size_t)NSLOT ? NS - 2 : LAG2_DEFAULT);      // launches a chunk's stage 2 may be behind
    const int64_t tw0 = now_ns();

    std::mutex mu;
    std::condition_variable cv;
    size_t ready = 0;            // chunks (local index) whose read-back has been enqueued: the collector may wait for them
    bool stop = false;
    auto fail_with = [&](scrg_status s) {
        const std::string e = ds->get_err();
        c->fail(s, e.empty() ? std::string(scrg_status_string(s)) : e);
        { std::lock_guard<std::mutex> g(mu); }      // (the launch thread may be between its predicate and its wait on cv)
        cv.notify_all();
    };

    // COLLECT threads: chunk i (local index) is taken by collector i mod NCOLLECT — a chunk's place in the result arrays
    // depends only on the totals of the chunks before it, which are known before it is read back
    std::vector<char> done(m, 0);
    auto collect = [&](size_t which) {
        // (no exception leaves a thread: a std::bad_alloc in here would otherwise be std::terminate)
        try {
        for (size_t i = which; i < m; i += NCOLLECT) {
            {
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&] { return ready > i || stop; });
                if (ready <= i) return;
            }
            const int64_t ta = now_ns();
            scrg_status s = c->failed() ? (scrg_status)c->status.load() : stage3(ds, ds->slot[i % NS], *c, mine[i]);
            if (s != SCRG_OK) fail_with(s);
            if (timing)
                fprintf(stderr, "[scrooge_amd host] dev %d chunk %zu collected at %.3f ms: stage3 %.3f ms\n", dev_index, i, (now_ns() - tw0) / 1e6,
                        (now_ns() - ta) / 1e6);
            {
                std::lock_guard<std::mutex> g(mu);
                done[i] = 1;
            }
            cv.notify_all();
        }
        } catch (const std::bad_alloc&) {
            ds->set_err("host allocation failed while collecting results");
            fail_with(SCRG_ERR_OOM);
        } catch (...) {
            ds->set_err("unexpected exception while collecting results");
            fail_with(SCRG_ERR_INVALID_ARG);
        }
    };
    std::thread collectors[NCOLLECT];
    for (size_t k = 0; k < NCOLLECT; k++) collectors[k] = std::thread(collect, k);

    // LAUNCH thread.  A chunk's sizes are looked at (stage 2) as soon as they have arrived — asked for without waiting after
    // every launch — and waited for only when the chunk is LAG chunks behind the launches or nothing is left to launch.
    size_t next2 = 0;
    bool ok = true;
    auto do_stage2 = [&](size_t k) -> bool {
        const int64_t tb = now_ns();
        scrg_status s = stage2(ds, ds->slot[k % NS], *c, mine[k]);
        if (s != SCRG_OK) {
            fail_with(s);
            return false;
        }
        {
            std::lock_guard<std::mutex> g(mu);
            ready = k + 1;
        }
        cv.notify_all();
        if (timing) fprintf(stderr, "[scrooge_amd host] dev %d chunk %zu stage2 at %.3f ms: %.3f ms\n", dev_index, k, (tb - tw0) / 1e6, (now_ns() - tb) / 1e6);
        return true;
    };
    try {
    for (size_t i = 0; i < m && ok; i++) {
        if (c->failed()) break;
        const int64_t ta = now_ns();
        if (i >= NS) {               // the slot's previous chunk must have been collected (its stage 2 is behind us: LAG < NS)
            std::unique_lock<std::mutex> lk(mu);
            cv.wait(lk, [&] { return done[i - NS] || c->failed(); });
            if (c->failed()) break;
        }
        scrg_status s = stage1(ds, ds->slot[i % NS], *c, mine[i]);
        if (timing)
            fprintf(stderr, "[scrooge_amd host] dev %d chunk %zu stage1 at %.3f ms: %.3f ms (pack %.3f)\n", dev_index, i, (ta - tw0) / 1e6,
                    (now_ns() - ta) / 1e6, ds->slot[i % NS].t_pack_ns / 1e6);
        if (s != SCRG_OK) {
            fail_with(s);
            break;
        }
        while (ok && next2 <= i) {
            const bool must = i + 1 - next2 > LAG2;
            if (!must && hipEventQuery(ds->slot[next2 % NS].ev_tot) != hipSuccess) {
                (void)hipGetLastError();
                break;
            }
            ok = do_stage2(next2++);
        }
    }
    while (ok && !c->failed() && next2 < m) ok = do_stage2(next2++);
    } catch (const std::bad_alloc&) {
        ds->set_err("host allocation failed while staging a chunk");
        fail_with(SCRG_ERR_OOM);
    } catch (...) {
        ds->set_err("unexpected exception while staging a chunk");
        fail_with(SCRG_ERR_INVALID_ARG);
    }
    {
        std::lock_guard<std::mutex> g(mu);
        stop = true;
    }
    cv.notify_all();
    for (auto& t : collectors) t.join();
    (void)hipSetDevice(ds->device);
    for (Slot& sl : ds->slot) (void)hipStreamSynchronize(sl.stream);        // nothing of this call is in flight when it returns
}

// The plan of a call: the issue order (longest read first, src/tests.cu:375-377; stable, so a batch that is sorted already
// keeps its order) and the chunks it is cut into.  Chunk k is processed by device state k mod n_states.
void make_plan(Call& c, const scrg_params& resolved, int n_states, bool* sorted_issue_out)
{
    const scrg_host::Batch& b = *c.b;
    const uint64_t n = c.n;
    c.order.resize(n);
    std::atomic<int> unsorted{0}, long_reads{0};
    {
        const uint64_t BLK = 1u << 16, nb = (n + BLK - 1) / BLK;
        parallel_for(nb, [&](uint64_t blk) {
            bool ok = true, lng = false;
            for (uint64_t k = blk * BLK; k < std::min(n, (blk + 1) * BLK); k++) {
                c.order[k] = (uint32_t)k;
                const uint64_t len = issue_len(c, k);
                if (k && issue_len(c, k - 1) < len) ok = false;
                if (len > SHORT_READS) lng = true;
            }
            if (!ok) unsorted.store(1, std::memory_order_relaxed);
            if (lng) long_reads.store(1, std::memory_order_relaxed);
        }, true);
    }
    c.n_slots = long_reads.load() ? NSLOT : MAXSLOT;
    c.identity = true;
    if (resolved.sort_by_length && unsorted.load()) {
        std::stable_sort(c.order.begin(), c.order.end(),
                         [&](uint32_t x, uint32_t y) { return issue_len(c, x) > issue_len(c, y); });
        c.identity = false;
    }
    // chunks in issue order: whole groups of 64 pairs.  A chunk's align kernel takes ~2 ms for 10 kb reads however few
    // pairs it has, and only NSLOT of them run side by side: a small batch is cut into NSLOT chunks per device, a large one
    // into chunks of at most 32 MB of packed sequence or 256 k pairs.  In sorted issue order the first pair of a chunk has
    // its longest read.
    const bool sorted_issue = resolved.sort_by_length || !unsorted.load();
    // A device's LAST chunk is smaller (0.6 of the others): after the last launch nothing overlaps that chunk's kernel,
    // read-back and collection any more, so it should be the cheapest one (20 k x 10 kb pairs: 6.9 -> 6.6 ms).
    const uint64_t max_words = 4u << 20, want_chunks = (uint64_t)n_states * c.n_slots;
    const uint64_t full_chunks = want_chunks - (uint64_t)n_states;                       // chunks of the full size
    const uint64_t per_full = (uint64_t)((double)n / ((double)full_chunks + 0.6 * (double)n_states));
    const uint64_t target_full = std::min<uint64_t>(1u << 18, std::max<uint64_t>(512, (per_full + GROUP - 1) / GROUP * GROUP));
    const uint64_t rest = n > full_chunks * target_full ? n - full_chunks * target_full : 0;
    const uint64_t target_last = std::min<uint64_t>(1u << 18, std::max<uint64_t>(512, (rest / (uint64_t)n_states + GROUP - 1) / GROUP * GROUP));
    c.chunk_first.clear();
    c.chunk_first.push_back(0);
    uint64_t k = 0;
    while (k < n) {
        const uint64_t target = c.chunk_first.size() - 1 < full_chunks ? target_full : target_last;
        uint64_t e;
        if (sorted_issue && b.mapping) {
            const uint64_t w = std::max<uint64_t>(1, (issue_len(c, c.order[k]) + 31) / 32);
            e = k + std::max<uint64_t>(GROUP, std::min(target, max_words / w / GROUP * GROUP));
        } else {
            uint64_t words = 0;
            e = k;
            while (e < n) {
                const uint64_t p = c.order[e];
                const uint64_t w = (b.read_lens[read_of(c, p)] + 31) / 32 + (b.mapping ? 0 : (b.text_lens[p] + 31) / 32);
                if (e > k && (e - k) % GROUP == 0 && (e - k >= target || words + w > max_words)) break;
                words += w;
                e++;
            }
        }
        e = std::min(e, n);
        // best-candidate mode: a read's candidates (adjacent in issue order: the sort is stable) stay in one chunk, so that the
        // selection sees whole groups — the cut moves forward to the next pair of another read, and the chunk's last group
        // of 64 is then a partial one, as the call's last chunk's may be anyway
        // (a paired call: a mate pair's two reads stay in one chunk)
        const uint32_t same = c.mates ? ~1u : ~0u;
        if (c.best)
            while (e < n && (b.pair_read[c.order[e]] & same) == (b.pair_read[c.order[e - 1]] & same)) e++;
        c.chunk_first.push_back(e);
        k = e;
    }
    if (sorted_issue_out) *sorted_issue_out = sorted_issue;
    if (c.mates) {
        // the mate pairs in issue order: the sort is stable and by mate pair, so each one's pairs are adjacent, side A's first
        c.mate_id.clear();
        c.mate_start.clear();
        c.mate_b.clear();
        c.mate_id.reserve(b.n_reads / 2);
        c.mate_start.reserve(b.n_reads / 2 + 1);
        c.mate_b.reserve(b.n_reads / 2);
        for (uint64_t i = 0; i < n;) {
            const uint64_t m = b.pair_read[c.order[i]] >> 1;
            const uint64_t n_a = b.cand_offsets[2 * m + 1] - b.cand_offsets[2 * m], n_b = b.cand_offsets[2 * m + 2] - b.cand_offsets[2 * m + 1];
            c.mate_id.push_back((uint32_t)m);
            c.mate_start.push_back(i);
            c.mate_b.push_back(i + n_a);
            i += n_a + n_b;
        }
        c.mate_start.push_back(n);
    }
    if (c.summary) {
        // the reads in issue order: the sort is stable and a read's pairs share its length, so they are adjacent and in caller order
        // (found by the threads: issue position i starts a read where the pair before it is another read's — count per block, sum, fill)
        constexpr uint64_t BLK = 1u << 16;
        const uint64_t n_blk = (n + BLK - 1) / BLK;
        std::vector<uint64_t> blk_first(n_blk + 1, 0);
        auto starts_read = [&](uint64_t i) { return i == 0 || b.pair_read[c.order[i]] != b.pair_read[c.order[i - 1]]; };
        parallel_for(n_blk, [&](uint64_t blk) {
            uint64_t cnt = 0;
            for (uint64_t i = blk * BLK; i < std::min(n, (blk + 1) * BLK); i++) cnt += starts_read(i) ? 1 : 0;
            blk_first[blk + 1] = cnt;
        }, true);
        for (uint64_t blk = 0; blk < n_blk; blk++) blk_first[blk + 1] += blk_first[blk];
        const uint64_t n_with = blk_first[n_blk];
        c.sum_id.assign(n_with, 0);
        c.sum_start.assign(n_with + 1, n);
        parallel_for(n_blk, [&](uint64_t blk) {
            uint64_t at = blk_first[blk];
            for (uint64_t i = blk * BLK; i < std::min(n, (blk + 1) * BLK); i++)
                if (starts_read(i)) {
                    c.sum_id[at] = b.pair_read[c.order[i]];
                    c.sum_start[at++] = i;
                }
        }, true);
    }
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------------
// interface (scrg_internal.h)
// ---------------------------------------------------------------------------------------------------------------
namespace scrg_host {

// The issue order and the chunk boundaries a call with these lengths would use (no GPU involved): what the CPU tests check.
scrg_status plan(const scrg_params& resolved, int n_states, const Batch& b, uint32_t* order_out, uint64_t* chunk_first_out,
                 uint64_t chunk_cap, uint64_t* n_chunks_out)
{
    if (n_states < 1 || !n_chunks_out) return SCRG_ERR_INVALID_ARG;
    Call c;
    c.b = &b;
    c.p = resolved;
    c.n = b.n_pairs;
    c.mates = b.mapping && b.mate_rule;
    c.best = b.mapping && ((resolved.outputs & SCRG_OUT_BEST) || c.mates);
    make_plan(c, resolved, n_states, nullptr);
    const uint64_t nc = c.chunk_first.size() - 1;
    *n_chunks_out = nc;
    if (order_out) memcpy(order_out, c.order.data(), c.n * sizeof(uint32_t));
    if (chunk_first_out) {
        if (chunk_cap < nc + 1) return SCRG_ERR_CIGAR_OVERFLOW;
        memcpy(chunk_first_out, c.chunk_first.data(), (nc + 1) * sizeof(uint64_t));
    }
    return SCRG_OK;
}

// One sequence, ASCII -> planar 2-bit, with the packer the host entry points use (AVX2 or scalar by what the CPU has)
bool pack_planar_host(const char* ascii, uint64_t n_bases, uint64_t* planar, uint64_t stride_words, uint64_t n_words)
{
    return pack_sequence(ascii ? ascii : "", n_bases, false, planar, stride_words ? stride_words : 1, n_words);
}

void* state_create(int device)
{
    int nd = 0;
    if (hipGetDeviceCount(&nd) != hipSuccess || device < 0 || device >= nd) {
        (void)hipGetLastError();
        return nullptr;
    }
    if (hipSetDevice(device) != hipSuccess) return nullptr;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return nullptr;
    DeviceState* ds = new (std::nothrow) DeviceState();
    if (!ds) return nullptr;
    ds->device = device;
    ds->n_cus = prop.multiProcessorCount;
    // three streams of different priorities: HIP maps them to different hardware queues, so the kernels of consecutive
    // chunks share the GPU instead of queueing behind each other
    const int prio[MAXSLOT] = {0, -1, 1, 0, 0, -1, 1, 0};
    for (int k = 0; k < MAXSLOT; k++) {
        Slot& sl = ds->slot[k];
        if (hipStreamCreateWithPriority(&sl.stream, hipStreamNonBlocking, prio[k]) != hipSuccess || hipEventCreateWithFlags(&sl.ev_tot, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&sl.ev_done, hipEventDisableTiming) != hipSuccess || scrg_int::ctx_create_internal(device, &sl.ctx) != SCRG_OK ||
            scrg_ctx_set_stream(sl.ctx, sl.stream) != SCRG_OK) {
            state_free(ds);
            return nullptr;
        }
    }
    return ds;
}

void state_free(void* state)
{
    DeviceState* ds = static_cast<DeviceState*>(state);
    if (!ds) return;
    (void)hipSetDevice(ds->device);
    (void)hipDeviceSynchronize();
    for (Slot& sl : ds->slot) {
        if (sl.ctx) scrg_ctx_destroy(sl.ctx);
        if (sl.ev_tot) (void)hipEventDestroy(sl.ev_tot);
        if (sl.ev_done) (void)hipEventDestroy(sl.ev_done);
        if (sl.stream) (void)hipStreamDestroy(sl.stream);
        for (HostPinned* hp : {&sl.h_seq, &sl.h_meta, &sl.h_out, &sl.h_tot, &sl.h_mates, &sl.h_mrec, &sl.h_sum, &sl.h_srec}) hp->release();
        sl.d_mates.release();
        sl.d_sum.release();
        for (DevBuf* db : {&sl.d_meta, &sl.d_desc, &sl.d_slices, &sl.d_ed, &sl.d_nruns, &sl.d_cnt64, &sl.d_len64, &sl.d_tot, &sl.d_dense, &sl.d_temp,
                           &sl.d_dlen, &sl.d_doff, &sl.d_dtext})
            db->release();
        sl.h_diff.release();
        for (RecordBuf& rb : sl.rec) {
            rb.d.release();
            rb.h.release();
        }
    }
    ds->d_seq.release();
    ds->d_pile.release();
    ds->drop_index();
    delete ds;
    {   // the genome staging buffer is not worth keeping pinned for a process that is letting go of its device states
        std::lock_guard<std::mutex> g(g_genome_staging.mu);
        g_genome_staging.release();
    }
}

scrg_status genome_set(void* state, const char* genome, uint64_t genome_len, std::string* err)
{
    DeviceState* ds = static_cast<DeviceState*>(state);
    if (!ds) return SCRG_ERR_NO_DEVICE;
    std::lock_guard<std::mutex> g(ds->mu);
    ds->set_err("");
    scrg_status s = pack_genome(ds, genome, genome_len);
    if (s != SCRG_OK && err) *err = ds->get_err();
    return s;
}

void genome_clear(void* state)
{
    DeviceState* ds = static_cast<DeviceState*>(state);
    if (!ds) return;
    std::lock_guard<std::mutex> g(ds->mu);
    ds->genome_ok = false;
    ds->drop_index();
}

bool pileup_view(void* state, PileupView* v)
{
    DeviceState* ds = static_cast<DeviceState*>(state);
    if (!ds) return false;
    std::lock_guard<std::mutex> g(ds->mu);
    if (!ds->pile_dirty || !ds->d_pile.p) return false;
    v->target_len = ds->pile_len;
    v->d_acc = ds->d_pile.as<uint32_t>();
    return true;
}

void pileup_discard(void* state, bool release)
{
    DeviceState* ds = static_cast<DeviceState*>(state);
    if (!ds) return;
    std::lock_guard<std::mutex> g(ds->mu);
    ds->pile_dirty = false;
    if (release && ds->d_pile.p) {
        (void)hipSetDevice(ds->device);
        (void)hipDeviceSynchronize();
        ds->d_pile.release();
    }
}

bool pileup_genome(void* state, uint64_t target_len, const uint64_t** d_seq)
{
    DeviceState* ds = static_cast<DeviceState*>(state);
    if (!ds) return false;
    // (read under the state's lock, as the calls that replace the genome write it; the pointer stays good only while no other call
    // runs on the handle, which is what a handle asks of its caller anyway: one call at a time)
    std::lock_guard<std::mutex> g(ds->mu);
    if (!ds->genome_ok || !ds->d_seq.p || ds->genome_len != target_len) return false;
    *d_seq = ds->d_seq.as<uint64_t>();
    return true;
}

// the accumulator of a call with the pileup on: the one the calls before it left, or a zeroed one for this genome
static scrg_status pileup_prepare(DeviceState* ds)
{
    if (ds->pile_dirty && ds->pile_len != ds->genome_len) {
        ds->set_err("the pileup accumulator holds a genome of another length: take the pileup first (scrg_ctx_set_pileup, scrg_ctx_take_pileup)");
        return SCRG_ERR_INVALID_ARG;
    }
    if (ds->pile_dirty) return SCRG_OK;
    const uint64_t words = scrg::PILE_PLANES * (ds->genome_len + 1) + 2;
    HTRY(ds, hipSetDevice(ds->device));
    HTRY(ds, ds->d_pile.ensure(words * sizeof(uint32_t)));
    HTRY(ds, hipMemsetAsync(ds->d_pile.p, 0, words * sizeof(uint32_t), ds->slot[0].stream));
    HTRY(ds, hipStreamSynchronize(ds->slot[0].stream));
    ds->pile_len = ds->genome_len;
    ds->pile_dirty = true;
    return SCRG_OK;
}

bool genome_resident(void* state, uint64_t* genome_len)
{
    DeviceState* ds = static_cast<DeviceState*>(state);
    if (!ds || !ds->genome_ok) return false;
    if (genome_len) *genome_len = ds->genome_len;
    return true;
}

// ---- seeding (include/scrooge_amd.h: SEEDING; seed_kernels.hip) ----
scrg_status genome_index(void* state, const scrg_seed_rule& rule, uint32_t smer, std::string* err)
{
    DeviceState* ds = static_cast<DeviceState*>(state);
    if (!ds) return SCRG_ERR_NO_DEVICE;
    std::lock_guard<std::mutex> g(ds->mu);
    ds->set_err("");
    const scrg_status s = [&]() -> scrg_status {
        if (!ds->genome_ok) {
            ds->set_err("no resident genome: call scrg_genome_set first");
            return SCRG_ERR_INVALID_ARG;
        }
        if (scrg_seed_rule_check(&rule, ds->genome_len) != SCRG_OK) {
            ds->set_err("seed rule: k 8 .. 16, stride 1 .. 64, max_occ 1 .. 65535, band 0 .. 65535, min_hits >= 1, max_candidates 1 .. 64, strands 1 or 3, "
                        "a genome shorter than 2^32 bases and at most 2^31 - 1 index entries ((genome_len - k) / stride + 1)");
            return SCRG_ERR_INVALID_ARG;
        }
        ds->drop_index();
        if (!scrg::seed_smer_valid(smer, rule.k)) {
            ds->set_err("seed sampling: smer is 0 or 3 .. k - 1 (scrg_ctx_set_seed_sampling)");
            return SCRG_ERR_INVALID_ARG;
        }
        HTRY(ds, hipSetDevice(ds->device));
        DeviceState::SeedIndex& ix = ds->seed;
        hipStream_t st = ds->slot[0].stream;
        const uint64_t n_positions = scrg::seed_index_entries(ds->genome_len, rule.k, rule.stride);
        uint64_t n = n_positions;
        DevBuf keys_tmp, pos_tmp, temp, block_cnt, block_base;
        struct Release {
            DevBuf *a, *b, *c, *d, *e;
            ~Release() { a->release(); b->release(); c->release(); d->release(); e->release(); }
        } release{&keys_tmp, &pos_tmp, &temp, &block_cnt, &block_base};
        if (smer) {                          // the entries depend on the data: a count per workgroup, their sum home in one synchronisation
            const uint64_t nb = scrg::seed_select_blocks(n_positions);
            const size_t scan_bytes = scrg::seed_select_temp_bytes(n_positions);
            HTRY(ds, block_cnt.ensure((nb + 1) * sizeof(uint32_t)));
            HTRY(ds, block_base.ensure((nb + 1) * sizeof(uint32_t)));
            HTRY(ds, temp.ensure(scan_bytes));
            HTRY(ds, scrg::launch_seed_select_count(ds->d_seq.as<uint64_t>(), n_positions, rule.k, rule.stride, smer, block_cnt.as<uint32_t>(),
                                                    block_base.as<uint32_t>(), temp.p, scan_bytes, st));
            uint32_t total = 0;
            HTRY(ds, hipMemcpyAsync(&total, block_base.as<uint32_t>() + nb, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
            HTRY(ds, hipStreamSynchronize(st));
            n = total;
            if (n > n_positions) {
                ds->set_err("internal error: more index entries than positions");
                return SCRG_ERR_HIP;
            }
        }
        const uint32_t bits = scrg::seed_bucket_bits(n, rule.k);
        const size_t temp_bytes = scrg::seed_index_sort_temp_bytes(n, rule.k);
        HTRY(ds, ix.keys.ensure((n + 1) * sizeof(uint32_t)));
        HTRY(ds, ix.pos.ensure((n + 1) * sizeof(uint32_t)));
        HTRY(ds, ix.buckets.ensure(((1ull << bits) + 1) * sizeof(uint32_t)));
        HTRY(ds, keys_tmp.ensure((n + 1) * sizeof(uint32_t)));
        HTRY(ds, pos_tmp.ensure((n + 1) * sizeof(uint32_t)));
        HTRY(ds, temp.ensure(temp_bytes));
        HTRY(ds, scrg::launch_seed_index(ds->d_seq.as<uint64_t>(), n, rule.k, rule.stride, keys_tmp.as<uint32_t>(), pos_tmp.as<uint32_t>(), ix.keys.as<uint32_t>(),
                                         ix.pos.as<uint32_t>(), bits, ix.buckets.as<uint32_t>(), temp.p, temp_bytes, st, smer, n_positions,
                                         block_base.as<uint32_t>()));
        HTRY(ds, hipStreamSynchronize(st));
        ix.smer = smer;
        ix.n_positions = n_positions;
        ix.last_n_lookups = 0;
        ix.rule = scrg::SeedRule{rule.k, rule.stride, rule.max_occ, rule.band, rule.min_hits, rule.max_candidates, rule.strands,
                                 rule.hit_budget_mb ? rule.hit_budget_mb : scrg::SEED_DEFAULT_BUDGET_MB};
        ix.n_entries = n;
        ix.bucket_bits = bits;
        ix.ok = true;
        return SCRG_OK;
    }();
    if (s != SCRG_OK) {
        ds->drop_index();
        if (err) *err = ds->get_err();
    }
    return s;
}

void genome_index_clear(void* state)
{
    DeviceState* ds = static_cast<DeviceState*>(state);
    if (!ds) return;
    std::lock_guard<std::mutex> g(ds->mu);
    ds->drop_index();
}

bool genome_index_info(void* state, scrg_seed_rule* rule, uint64_t* n_entries, uint64_t* device_bytes)
{
    DeviceState* ds = static_cast<DeviceState*>(state);
    if (!ds) return false;
    std::lock_guard<std::mutex> g(ds->mu);
    if (!ds->seed.ok || !ds->genome_ok) return false;
    const scrg::SeedRule& k = ds->seed.rule;
    if (rule) *rule = scrg_seed_rule{k.k, k.stride, k.max_occ, k.band, k.min_hits, k.max_candidates, k.strands, k.hit_budget_mb};
    if (n_entries) *n_entries = ds->seed.n_entries;
    if (device_bytes) *device_bytes = ds->seed.keys.cap + ds->seed.pos.cap + ds->seed.buckets.cap;
    return true;
}

bool seed_sampling_info(void* state, uint32_t* smer, uint64_t* n_positions, uint64_t* last_n_lookups)
{
    DeviceState* ds = static_cast<DeviceState*>(state);
    if (!ds) return false;
    std::lock_guard<std::mutex> g(ds->mu);
    if (!ds->seed.ok || !ds->genome_ok) return false;
    if (smer) *smer = ds->seed.smer;
    if (n_positions) *n_positions = ds->seed.n_positions;
    if (last_n_lookups) *last_n_lookups = ds->seed.last_n_lookups;
    return true;
}

scrg_status find_candidates(void* state, uint64_t n_reads, const char* const* reads, const uint64_t* read_lens, scrg_candidates** out, std::string* err)
{
    DeviceState* ds = static_cast<DeviceState*>(state);
    if (!ds) return SCRG_ERR_NO_DEVICE;
    std::lock_guard<std::mutex> g(ds->mu);
    ds->set_err("");
    struct Free {
        void operator()(scrg_candidates* c) const { scrg_candidates_free(c); }
    };
    std::unique_ptr<scrg_candidates, Free> res;
    const scrg_status s = [&]() -> scrg_status {
        auto fail = [&](scrg_status code, const char* what) {
            ds->set_err(what);
            return code;
        };
        if (!ds->seed.ok || !ds->genome_ok) return fail(SCRG_ERR_INVALID_ARG, "no genome index: call scrg_genome_index first (scrg_genome_set and scrg_genome_clear drop it)");
        if (n_reads && (!reads || !read_lens)) return fail(SCRG_ERR_INVALID_ARG, "null input array");
        const scrg::SeedRule k = ds->seed.rule;
        const uint32_t n_strands = k.strands == 3u ? 2u : 1u, M = k.max_candidates;
        res.reset(static_cast<scrg_candidates*>(calloc(1, sizeof(scrg_candidates))));
        if (!res) return fail(SCRG_ERR_OOM, "host allocation failed");
        res->n_reads = n_reads;
        res->rule = scrg_seed_rule{k.k, k.stride, k.max_occ, k.band, k.min_hits, k.max_candidates, k.strands, k.hit_budget_mb};
        res->cand_offsets = static_cast<uint64_t*>(calloc(n_reads + 1, sizeof(uint64_t)));
        if (!res->cand_offsets) return fail(SCRG_ERR_OOM, "host allocation failed");
        std::vector<uint64_t> starts;
        std::vector<uint8_t> strands;
        std::vector<uint32_t> votes;
        uint64_t n_lookups = 0;
        auto deliver = [&]() -> scrg_status {
            const size_t n = starts.size();
            res->cand_start = static_cast<uint64_t*>(malloc((n + 1) * sizeof(uint64_t)));
            res->cand_reverse = static_cast<uint8_t*>(malloc(n + 1));
            res->cand_votes = static_cast<uint32_t*>(malloc((n + 1) * sizeof(uint32_t)));
            if (!res->cand_start || !res->cand_reverse || !res->cand_votes) return fail(SCRG_ERR_OOM, "host allocation failed");
            if (n) {
                memcpy(res->cand_start, starts.data(), n * sizeof(uint64_t));
                memcpy(res->cand_reverse, strands.data(), n);
                memcpy(res->cand_votes, votes.data(), n * sizeof(uint32_t));
            }
            ds->seed.last_n_lookups = n_lookups;
            return SCRG_OK;
        };
        if (n_reads == 0) return deliver();

        // the reads: packed once (host threads), a word of padding behind each
        std::vector<uint64_t> word(n_reads + 1, 0), lane_off(n_reads + 1, 0);
        std::vector<uint32_t> len(n_reads);
        for (uint64_t r = 0; r < n_reads; r++) {
            const uint64_t L = read_lens[r];
            if (L > scrg::SEED_MAX_READ) return fail(SCRG_ERR_INVALID_ARG, "a read of 2^30 bases or more cannot be seeded");
            if (L && !reads[r]) return fail(SCRG_ERR_INVALID_ARG, "null read");
            len[r] = (uint32_t)L;
            word[r + 1] = word[r] + (L + 31) / 32 + 1;
            lane_off[r + 1] = lane_off[r] + n_strands * scrg::seed_read_positions(L, k.k);
        }
        std::vector<uint64_t> packed(word[n_reads]);
        std::atomic<int> bad{0};
        parallel_for(n_reads, [&](uint64_t r) {
            if (pack_sequence(reads[r], len[r], false, packed.data() + word[r], 1, word[r + 1] - word[r])) bad.store(1, std::memory_order_relaxed);
        });
        if (bad.load()) return fail(SCRG_ERR_BAD_BASE, "a read contains characters other than ACGTacgt");

        HTRY(ds, hipSetDevice(ds->device));
        hipStream_t st = ds->slot[0].stream;
        DevBuf* const ws = ds->seed_ws;
        HTRY(ds, ws[W_SEQ].ensure(packed.size() * sizeof(uint64_t)));
        HTRY(ds, ws[W_WORD].ensure(word.size() * sizeof(uint64_t)));
        HTRY(ds, ws[W_LEN].ensure(len.size() * sizeof(uint32_t)));
        HTRY(ds, ws[W_LANE].ensure(lane_off.size() * sizeof(uint64_t)));
        HTRY(ds, ws[W_HITS].ensure(n_reads * sizeof(uint64_t)));
        HTRY(ds, ws[W_OVER].ensure(n_reads * sizeof(uint32_t)));
        HTRY(ds, ws[W_LOOK].ensure(n_reads * sizeof(uint32_t)));
        HTRY(ds, hipMemcpyAsync(ws[W_SEQ].p, packed.data(), packed.size() * sizeof(uint64_t), hipMemcpyHostToDevice, st));
        HTRY(ds, hipMemcpyAsync(ws[W_WORD].p, word.data(), word.size() * sizeof(uint64_t), hipMemcpyHostToDevice, st));
        HTRY(ds, hipMemcpyAsync(ws[W_LEN].p, len.data(), len.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        HTRY(ds, hipMemcpyAsync(ws[W_LANE].p, lane_off.data(), lane_off.size() * sizeof(uint64_t), hipMemcpyHostToDevice, st));
        const scrg::SeedIndexView ix{ds->seed.keys.as<uint32_t>(), ds->seed.pos.as<uint32_t>(), ds->seed.buckets.as<uint32_t>(), 2u * k.k - ds->seed.bucket_bits,
                                     k.k, k.max_occ, k.band, k.min_hits, M, ds->seed.smer};
        const scrg::SeedReadsView rd{ws[W_SEQ].as<uint64_t>(), ws[W_WORD].as<uint64_t>(), ws[W_LEN].as<uint32_t>(), ws[W_LANE].as<uint64_t>(), n_strands};

        // every read's hits: what the chunks are cut by
        constexpr uint64_t MAX_CHUNK_READS = 1ull << 22, MAX_COUNT = 0x7ffffff0ull;
        for (uint64_t r0 = 0; r0 < n_reads; r0 += MAX_CHUNK_READS)
            HTRY(ds, scrg::launch_seed_totals(ix, rd, r0, std::min(MAX_CHUNK_READS, n_reads - r0), ws[W_HITS].as<uint64_t>(), ws[W_OVER].as<uint32_t>(),
                                              ws[W_LOOK].as<uint32_t>(), st));
        std::vector<uint64_t> hits(n_reads);
        std::vector<uint32_t> over(n_reads), looked(n_reads);
        HTRY(ds, hipMemcpyAsync(looked.data(), ws[W_LOOK].p, n_reads * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        HTRY(ds, hipMemcpyAsync(hits.data(), ws[W_HITS].p, n_reads * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
        HTRY(ds, hipMemcpyAsync(over.data(), ws[W_OVER].p, n_reads * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        HTRY(ds, hipStreamSynchronize(st));
        for (uint64_t r = 0; r < n_reads; r++) {
            res->n_hits += hits[r];
            res->n_keys_over_max_occ += over[r];
            n_lookups += looked[r];
        }

        // chunks of whole reads whose hits fit the budget (48 bytes per hit: its word and r twice over for the sort, head, cluster,
        // position and anchor), and whose lanes fit four times as many; a read that exceeds either alone gets a chunk of its own
        const uint64_t budget_hits = std::min<uint64_t>(MAX_COUNT, std::max<uint64_t>(1, ((uint64_t)k.hit_budget_mb << 20) / 48));
        const uint64_t budget_lanes = std::min<uint64_t>(MAX_COUNT, 4 * budget_hits);
        std::vector<uint32_t> o_n, o_start, o_votes;
        std::vector<uint8_t> o_strand;
        for (uint64_t r0 = 0; r0 < n_reads;) {
            uint64_t r1 = r0 + 1, h = hits[r0];
            if (h > MAX_COUNT) return fail(SCRG_ERR_INVALID_ARG, "a read with 2^31 hits or more: lower max_occ");
            while (r1 < n_reads && r1 - r0 < MAX_CHUNK_READS && h + hits[r1] <= budget_hits && lane_off[r1 + 1] - lane_off[r0] <= budget_lanes) h += hits[r1++];
            scrg::SeedChunk ch{};
            ch.read0 = r0;
            ch.n_reads = r1 - r0;
            ch.lane_base = lane_off[r0];
            ch.n_lanes = lane_off[r1] - lane_off[r0];
            ch.n_hits = h;
            ch.temp_bytes = scrg::seed_chunk_temp_bytes(ch.n_lanes, h, ch.n_reads);
            const uint64_t nm = ch.n_reads * M;
            HTRY(ds, ws[W_CNT].ensure((ch.n_lanes + 1) * sizeof(uint64_t)));
            HTRY(ds, ws[W_OFF].ensure((ch.n_lanes + 1) * sizeof(uint64_t)));
            HTRY(ds, ws[W_WORDS].ensure((2 * h + 1) * sizeof(uint64_t)));
            HTRY(ds, ws[W_U32].ensure((5 * h + 2) * sizeof(uint32_t)));
            HTRY(ds, ws[W_ANCHOR].ensure((h + 1) * sizeof(uint64_t)));
            HTRY(ds, ws[W_OUT].ensure((ch.n_reads + 2 * nm) * sizeof(uint32_t) + nm));
            HTRY(ds, ws[W_TEMP].ensure(ch.temp_bytes));
            ch.cnt = ws[W_CNT].as<uint64_t>();
            ch.off = ws[W_OFF].as<uint64_t>();
            ch.word_tmp = ws[W_WORDS].as<uint64_t>();
            ch.word = ch.word_tmp + h;
            ch.r_tmp = ws[W_U32].as<uint32_t>();
            ch.r = ch.r_tmp + h;
            ch.head = ch.r + h;
            ch.cluster = ch.head + h;
            ch.first = ch.cluster + h;
            ch.anchor = ws[W_ANCHOR].as<uint64_t>();
            ch.out_n = ws[W_OUT].as<uint32_t>();
            ch.out_start = ch.out_n + ch.n_reads;
            ch.out_votes = ch.out_start + nm;
            ch.out_strand = reinterpret_cast<uint8_t*>(ch.out_votes + nm);
            ch.temp = ws[W_TEMP].p;
            HTRY(ds, scrg::launch_seed_chunk(ix, rd, ch, st));
            o_n.resize(ch.n_reads);
            o_start.resize(nm);
            o_votes.resize(nm);
            o_strand.resize(nm);
            uint32_t n_clusters = 0;
            HTRY(ds, hipMemcpyAsync(o_n.data(), ch.out_n, ch.n_reads * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
            HTRY(ds, hipMemcpyAsync(o_start.data(), ch.out_start, nm * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
            HTRY(ds, hipMemcpyAsync(o_votes.data(), ch.out_votes, nm * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
            HTRY(ds, hipMemcpyAsync(o_strand.data(), ch.out_strand, nm, hipMemcpyDeviceToHost, st));
            if (h) HTRY(ds, hipMemcpyAsync(&n_clusters, ch.cluster + (h - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, st));
            HTRY(ds, hipStreamSynchronize(st));
            res->n_clusters += n_clusters;
            for (uint64_t q = 0; q < ch.n_reads; q++) {
                if (o_n[q] > M) return fail(SCRG_ERR_HIP, "internal error: a read with more candidates than the rule allows");
                for (uint32_t j = 0; j < o_n[q]; j++) {
                    starts.push_back(o_start[q * M + j]);
                    votes.push_back(o_votes[q * M + j]);
                    strands.push_back(o_strand[q * M + j]);
                }
                res->cand_offsets[r0 + q + 1] = starts.size();
            }
            r0 = r1;
        }
        return deliver();
    }();
    if (s != SCRG_OK) {
        if (err) *err = ds->get_err();
        return s;
    }
    *out = res.release();
    return SCRG_OK;
}

// ---- results from issue order into caller order
// A byte stream with offsets: iss_off [n + 1] counts items of `item` bytes
struct OffsetStream {
    const uint64_t* iss_off;
    const char* iss;
    uint64_t* off;                         // out, [n + 1]
    char* out;
    uint64_t item;
};

// Every stream's sizes into caller order (per_pair(k, p) rides along: issue index k is the caller's pair p), their prefix sums in
// place, then the gather
template <typename F> static void streams_to_caller(const Call& c, const OffsetStream* st, int n_streams, F per_pair)
{
    const uint64_t n = c.n;
    parallel_for(n, [&](uint64_t k) {
        const uint64_t p = c.order[k];
        for (int j = 0; j < n_streams; j++) st[j].off[p] = st[j].iss_off[k + 1] - st[j].iss_off[k];
        per_pair(k, p);
    });
    for (int j = 0; j < n_streams; j++) {
        uint64_t* const off = st[j].off;
        const scrg_int::BlockScan<uint64_t> scan(n, 1u << 16, 16, [&](uint64_t i) { return off[i]; });
        scan.place([&](uint64_t i, uint64_t x) {
            const uint64_t size = off[i];
            off[i] = x;
            return size;
        });
        off[n] = scan.total();
    }
    parallel_for(n, [&](uint64_t k) {
        const uint64_t p = c.order[k];
        for (int j = 0; j < n_streams; j++)
            memcpy(st[j].out + st[j].item * st[j].off[p], st[j].iss + st[j].item * st[j].iss_off[k], st[j].item * (st[j].iss_off[k + 1] - st[j].iss_off[k]));
    });
}

// Fixed-size per-pair records: identity hands the array over, otherwise a new one (malloc) is filled by c.order.  nullptr: out of memory.
template <typename T> static T* records_to_caller(Call& c, int kind)
{
    T* const iss = reinterpret_cast<T*>(c.iss_rec[kind]);
    if (c.identity) {
        c.iss_rec[kind] = nullptr;
        return iss;
    }
    T* const out = static_cast<T*>(malloc((c.n + 1) * sizeof(T)));
    if (out) parallel_for(c.n, [&](uint64_t k) { out[c.order[k]] = iss[k]; });
    return out;
}

const char* refusal(const CallOptions& o, bool text_strands, const scrg_params& p, const Batch& b, int n_states)
{
    const bool lanes = p.lanes_per_pair != 1, distance = (p.outputs & SCRG_OUT_DISTANCE) != 0;
    if (o.has_edit_limit() && lanes) return "an edit limit needs lanes_per_pair = 1, the default (the GenASM-row mappings have none)";
    // (as scrg_align_device; the host calls write their own descriptors, which carry the bit only for leftward candidates)
    if (text_strands && lanes) return "text strands need lanes_per_pair = 1, the default (the GenASM-row mappings read texts forwards only)";
    if (o.diff_kind != SCRG_DIFF_OFF) {
        if (lanes) return "difference strings need lanes_per_pair = 1, the default (scrg_ctx_set_diff)";
        if (distance) return "difference strings are made from runs: SCRG_OUT_DISTANCE has none (scrg_ctx_set_diff)";
        if (b.cand_leftward) return "difference strings of leftward candidates are not made on the device (scrg_ctx_set_diff; scrg_diff_from_runs)";
    }
    if (o.report) {
        if (lanes) return "the alignment report needs lanes_per_pair = 1, the default (scrg_ctx_set_report)";
        if (distance) return "the alignment report is made from runs: SCRG_OUT_DISTANCE has none (scrg_ctx_set_report)";
    }
    if (o.clip) {
        if (distance) return "clipping keeps a stretch of the runs: SCRG_OUT_DISTANCE has none (scrg_ctx_set_clip)";
        if (lanes) return "clipping needs lanes_per_pair = 1, the default (scrg_ctx_set_clip)";
        if (o.diff_kind != SCRG_DIFF_OFF)
            return "difference strings of clipped alignments are not made yet: their positions would start at 0, not at the kept stretch (scrg_ctx_set_clip)";
        if (o.report)
            return "the alignment report of clipped alignments is not made yet: its counts would describe another alignment than the one returned (scrg_ctx_set_clip)";
    }
    if (o.pileup) {
        if (!b.mapping) return "the pileup needs a target: pairs have none, the mapping calls have the genome (scrg_ctx_set_pileup)";
        if (distance) return "the pileup is summed from runs: SCRG_OUT_DISTANCE has none (scrg_ctx_set_pileup)";
        if (lanes) return "the pileup needs lanes_per_pair = 1, the default (scrg_ctx_set_pileup)";
        if (b.cand_leftward) return "the pileup takes forward texts only: leftward candidates are not served (scrg_ctx_set_pileup)";
        if (o.clip) return "the pileup of clipped alignments is not made yet: the kept stretch's positions are a later change (scrg_ctx_set_pileup)";
        if (n_states != 1) return "internal: the pileup is summed on one device state";      // (a handle has one; the calls without a handle have no options)
    }
    if (b.mate_rule) {
        const scrg_mate_rule& r = *b.mate_rule;
        if (!b.mapping || !b.cand_offsets) return "mate pairs need reads with candidates: scrg_align_mapping_paired";
        if (b.n_reads % 2) return "mate pairs: reads 2m and 2m+1 are mates, so the number of reads must be even (scrg_align_mapping_paired)";
        if (!scrg::mate_rule_valid(r.min_span, r.max_span, r.orientation, r.reserved[0], r.reserved[1]))
            return "mate rule: min_span <= max_span, orientation 0 .. 3 and zero reserved words are wanted (scrg_align_mapping_paired)";
        if (b.cand_leftward) return "mate pairs of leftward candidates are not served (scrg_align_mapping_paired)";
        if (n_states != 1) return "internal: a paired call runs on one device state";
        // (2^32 combinations need a side of 2^16 candidates at least: most batches are settled by their largest read)
        std::atomic<int> wide{0};
        parallel_for((b.n_reads + 65535) / 65536, [&](uint64_t blk) {
            for (uint64_t r = blk * 65536; r < std::min(b.n_reads, (blk + 1) * 65536); r++)
                if (b.cand_offsets[r + 1] - b.cand_offsets[r] >= 65536) wide.store(1, std::memory_order_relaxed);
        }, true);
        for (uint64_t m = 0; wide.load() && m < b.n_reads / 2; m++) {
            const uint64_t n_a = b.cand_offsets[2 * m + 1] - b.cand_offsets[2 * m], n_b = b.cand_offsets[2 * m + 2] - b.cand_offsets[2 * m + 1];
            if (n_a && n_b && n_a > 0xffffffffull / n_b) return "mate pairs: a mate pair's n_a x n_b must stay below 2^32 (scrg_align_mapping_paired)";
        }
    }
    if (distance && lanes) return "SCRG_OUT_DISTANCE needs lanes_per_pair = 1, the default (the GenASM-row mappings always write runs)";
    if (b.cand_leftward && lanes) return "leftward candidates need lanes_per_pair = 1, the default (the GenASM-row mappings read texts forwards only)";
    if ((p.outputs & SCRG_OUT_BEST) && !b.mapping) return "SCRG_OUT_BEST needs reads with candidates: a mapping call";
    if (o.clip) {
        // scores are summed in 32 bits: the longest read and the longest text together.  (A mapping pair's text is the rest of
        // the genome; what counts is what an alignment of its read can consume of it, taken as twice the read and a window.)
        uint64_t longest_read = 0, longest_text = 0;
        for (uint64_t i = 0; i < (b.mapping ? b.n_reads : b.n_pairs); i++) longest_read = std::max(longest_read, b.read_lens[i]);
        if (b.mapping) longest_text = 2 * longest_read + (uint64_t)p.W;
        else
            for (uint64_t i = 0; i < b.n_pairs; i++) longest_text = std::max(longest_text, b.text_lens[i]);
        if (!clip_scores_fit(o.clip_costs, longest_read + longest_text))
            return "clip scores are summed in 32 bits: (longest read + longest text) * max(match, mismatch, gap_open + gap_extend) must stay below 2^31";
    }
    if (o.read_summary) {
        const scrg_mapq_rule& r = o.mapq_rule;
        if (!b.mapping || !b.cand_offsets) return "the read summary needs reads with candidates: a mapping call in best-candidate mode (scrg_ctx_set_read_summary)";
        if (b.mate_rule) return "the read summary judges every read alone: a paired call's mate records carry cost and second_cost (scrg_ctx_set_read_summary)";
        if (!(p.outputs & SCRG_OUT_BEST)) return "the read summary needs SCRG_OUT_BEST: only then is every read whole inside one chunk (scrg_ctx_set_read_summary)";
        if (!scrg::mapq_rule_valid(r.per_edit, r.max_q, r.zero_per_mille, r.min_keep_q, r.reserved))
            return "mapq rule: per_edit 0 .. 255, max_q 0 .. 254, zero_per_mille 1 .. 1000, min_keep_q 0 .. 254 and a zero reserved word are wanted (scrg_ctx_set_read_summary)";
        if (r.min_keep_q > 0 && !o.pileup) return "min_keep_q > 0 filters the pileup, which is off (scrg_ctx_set_read_summary, scrg_ctx_set_pileup)";
        if (n_states != 1) return "internal: the read summary is made on one device state";
    }
    return nullptr;
}

scrg_status align(void* const* states, int n_states, const scrg_params& resolved, const Batch& b, const CallOptions& opt, bool text_strands,
                  scrg_result** out, SideResults* side, std::string* err)
{
    const int64_t t_begin = now_ns();
    if (!out || n_states < 1 || !states) return SCRG_ERR_INVALID_ARG;
    *out = nullptr;
    for (int d = 0; d < n_states; d++)
        if (!states[d]) return SCRG_ERR_NO_DEVICE;
    if ((opt.diff_kind != SCRG_DIFF_OFF || opt.report || opt.clip || b.mate_rule || opt.read_summary) && !side) return SCRG_ERR_INVALID_ARG;
    const uint64_t n = b.n_pairs;
    // every way out below releases what the call still owns: the result and the side results through their holders, the
    // issue-order arrays through Call's destructor
    struct ResultHolder {
        scrg_result* r = nullptr;
        ~ResultHolder() { scrg_result_free(r); }
    } res;
    SideResults made;
    auto bail = [&](scrg_status s, const std::string& e) {
        if (err) *err = e;
        return s;
    };
    if (const char* why = refusal(opt, text_strands, resolved, b, n_states)) return bail(SCRG_ERR_INVALID_ARG, why);

    res.r = static_cast<scrg_result*>(calloc(1, sizeof(scrg_result)));
    if (!res.r) return SCRG_ERR_OOM;
    scrg_result* const r = res.r;
    r->n_pairs = n;
    Call c;
    c.b = &b;
    c.p = resolved;
    c.opt = opt;
    c.n = n;
    c.distance = (resolved.outputs & SCRG_OUT_DISTANCE) != 0;
    c.want_runs = !c.distance && (resolved.outputs & ~SCRG_OUT_BEST) != SCRG_OUT_TEXT;
    c.want_text = !c.distance && (resolved.outputs & ~SCRG_OUT_BEST) != SCRG_OUT_RUNS;
    c.mates = b.mate_rule != nullptr;                    // (the refusal list has seen to it that this is a mapping call with an even number of reads)
    c.best = (resolved.outputs & SCRG_OUT_BEST) != 0 || c.mates;
    c.summary = opt.read_summary;                        // (the refusal list has seen to it that this is a mapping call in best-candidate mode)
    {
        const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
        c.threads_per_worker = std::max(1u, std::min(16u, hw / (unsigned)n_states));
    }

    bool sorted_issue = false;
    make_plan(c, resolved, n_states, &sorted_issue);
    const uint64_t n_chunks = c.chunk_first.size() - 1;
    c.c_runs.assign(n_chunks, 0);
    c.c_text.assign(n_chunks, 0);
    c.c_diff.assign(n_chunks, 0);
    c.c_known.assign(n_chunks, 0);

    // ---- result arrays in issue order
    c.iss_ed = static_cast<int64_t*>(g_pool.get((n + 1) * 8, n < 4096));
    c.iss_status = static_cast<uint32_t*>(g_pool.get((n + 1) * 4, n < 4096));
    c.iss_run_off = static_cast<uint64_t*>(g_pool.get((n + 1) * 8, n < 4096));
    c.iss_text_off = static_cast<uint64_t*>(g_pool.get((n + 1) * 8, n < 4096));
    if (c.distance) c.iss_tend = static_cast<uint64_t*>(g_pool.get((n + 1) * 8, n < 4096));
    if (opt.diff_kind) c.iss_diff_off = static_cast<uint64_t*>(g_diff_pool.get((n + 1) * 8, n < 4096));
    bool have_rec = true;
    for (int kind = 0; kind < N_REC; kind++)
        if (c.rec_on(kind)) have_rec = (c.iss_rec[kind] = static_cast<char*>(malloc((n + 1) * REC_SIZE[kind]))) != nullptr && have_rec;
    if (c.mates) {
        // a mate pair without pairs is in no chunk: its record is written here
        const uint64_t nm = b.n_reads / 2;
        c.mate_rec = static_cast<scrg_mate_record*>(malloc((nm + 1) * sizeof(scrg_mate_record)));
        if (!c.mate_rec) return bail(SCRG_ERR_OOM, "mate records");
        const scrg_mate_record none = {{scrg::MATE_NONE, scrg::MATE_NONE}, 0u, 0xffffffffu, 0u, 0, 0, 0};
        // (filled by the threads: 32 bytes per mate pair of fresh pages)
        parallel_for(nm / 4096 + 1, [&](uint64_t blk) {
            for (uint64_t m = blk * 4096; m <= std::min(nm, blk * 4096 + 4095); m++) c.mate_rec[m] = none;
        }, true);
    }
    if (c.summary) {
        // a read without pairs is in no chunk: its record is written here
        c.sum_rec = static_cast<scrg_read_record*>(malloc((b.n_reads + 1) * sizeof(scrg_read_record)));
        if (!c.sum_rec) return bail(SCRG_ERR_OOM, "read summary");
        const scrg_read_record none = {scrg::MAPQ_NONE, scrg::MAPQ_NO_ED, scrg::MAPQ_NO_ED, 0u, 0u, 0u, 0, 0, 0};
        parallel_for(b.n_reads / 4096 + 1, [&](uint64_t blk) {
            for (uint64_t r = blk * 4096; r <= std::min(b.n_reads, blk * 4096 + 4095); r++) c.sum_rec[r] = none;
        }, true);
    }
    if (!c.iss_ed || !c.iss_status || !c.iss_run_off || !c.iss_text_off || (c.distance && !c.iss_tend) || (opt.diff_kind && !c.iss_diff_off) || !have_rec)
        return bail(SCRG_ERR_OOM, "result arrays");

    // ---- device side: lock the states, size their sequence arrays (the largest chunk decides), genome
    std::vector<DeviceState*> ds(n_states);
    for (int d = 0; d < n_states; d++) ds[d] = static_cast<DeviceState*>(states[d]);
    std::vector<std::unique_lock<std::mutex>> locks;
    {
        std::vector<DeviceState*> uniq(ds.begin(), ds.end());
        std::sort(uniq.begin(), uniq.end());
        uniq.erase(std::unique(uniq.begin(), uniq.end()), uniq.end());
        if (uniq.size() != ds.size()) return bail(SCRG_ERR_INVALID_ARG, "a device state may be used once per call");
        for (DeviceState* u : uniq) locks.emplace_back(u->mu);
    }
    uint64_t slot_words = 0;
    {
        std::vector<uint64_t> cw(n_chunks, 0);
        parallel_for(n_chunks, [&](uint64_t k) {
            // upper bound of the chunk's padded layout: rows x the chunk's longest read / text
            uint64_t mr = 0, mt = 0;
            const uint64_t a = c.chunk_first[k], e = c.chunk_first[k + 1];
            if (sorted_issue && b.mapping) mr = issue_len(c, c.order[a]);
            else
                for (uint64_t i = a; i < e; i++) {
                    const uint64_t p = c.order[i];
                    mr = std::max<uint64_t>(mr, b.read_lens[read_of(c, p)]);
                    if (!b.mapping) mt = std::max<uint64_t>(mt, b.text_lens[p]);
                }
            const uint64_t rows = (e - a + GROUP - 1) / GROUP * GROUP;
            cw[k] = rows * std::max<uint64_t>(1, (mr + 31) / 32) + (b.mapping ? 0 : rows * std::max<uint64_t>(1, (mt + 31) / 32)) + SEQ_PAD;
        }, true);
        for (uint64_t w : cw) slot_words = std::max(slot_words, w);
    }
    for (int d = 0; d < n_states; d++) ds[d]->set_err("");
    if (b.mapping && b.genome) {             // packed once, copied to every device side by side
        const scrg_status s = stage_genome(ds.data(), n_states, b.genome, b.genome_len);
        if (s != SCRG_OK) return bail(s, ds[0]->get_err());
    }
    for (int d = 0; d < n_states; d++) {
        scrg_status s = SCRG_OK;
        if (b.mapping && !ds[d]->genome_ok) {
            ds[d]->set_err("no resident genome: call scrg_genome_set first");
            s = SCRG_ERR_INVALID_ARG;
        }
        if (s == SCRG_OK) s = ensure_seq(ds[d], ds[d]->genome_words, slot_words);
        if (s != SCRG_OK) return bail(s, ds[d]->get_err());
    }
    if (opt.pileup) {
        const scrg_status s = pileup_prepare(ds[0]);
        if (s != SCRG_OK) return bail(s, ds[0]->get_err());
    }
    if (b.mapping) {
        const uint64_t glen = ds[0]->genome_len;
        std::atomic<int> past{0};
        parallel_for(n, [&](uint64_t p) { if (b.cand_start[p] > glen) past.store(1, std::memory_order_relaxed); });
        if (past.load()) return bail(SCRG_ERR_INVALID_ARG, "candidate past end of genome");
    }

    const int64_t t_setup = now_ns();
    // ---- run: one worker per device
    if (n) {
        if (n_states == 1) worker(ds[0], &c, 0, 1);
        else {
            std::vector<std::thread> th;
            for (int d = 0; d < n_states; d++) th.emplace_back(worker, ds[d], &c, d, n_states);
            for (auto& t : th) t.join();
        }
    }
    if (c.failed()) return bail((scrg_status)c.status.load(), c.err);
    if (getenv("SCRG_HOST_TIMING"))
        fprintf(stderr, "[scrooge_amd host] %llu pairs, %llu chunks, %d device state(s): set-up %.3f ms, pipeline %.3f ms\n", (unsigned long long)n,
                (unsigned long long)n_chunks, n_states, (t_setup - t_begin) / 1e6, (now_ns() - t_setup) / 1e6);

    uint64_t total_runs = 0, total_text = 0, total_diff = 0;
    for (uint64_t k = 0; k < n_chunks; k++) {
        total_runs += c.c_runs[k];
        total_text += c.c_text[k];
        total_diff += c.c_diff[k];
    }
    c.iss_run_off[n] = total_runs;
    c.iss_text_off[n] = total_text;
    if (!c.runs.p) c.runs.p = static_cast<char*>(g_pool.get(16, true));
    if (!c.text.p) c.text.p = static_cast<char*>(g_pool.get(16, true));

    // ---- caller order
    if (c.identity) {
        r->edit_distance = std::exchange(c.iss_ed, nullptr);
        r->pair_status = std::exchange(c.iss_status, nullptr);
        r->run_offset = std::exchange(c.iss_run_off, nullptr);
        r->cigar_offset = std::exchange(c.iss_text_off, nullptr);
        r->runs = reinterpret_cast<scrg_run*>(std::exchange(c.runs.p, nullptr));
        r->cigar_text = std::exchange(c.text.p, nullptr);
        r->text_end = std::exchange(c.iss_tend, nullptr);
    } else {
        r->edit_distance = static_cast<int64_t*>(g_pool.get((n + 1) * 8, false));
        r->pair_status = static_cast<uint32_t*>(g_pool.get((n + 1) * 4, false));
        r->run_offset = static_cast<uint64_t*>(g_pool.get((n + 1) * 8, false));
        r->cigar_offset = static_cast<uint64_t*>(g_pool.get((n + 1) * 8, false));
        r->runs = static_cast<scrg_run*>(g_pool.get(2 * total_runs + 16, false));
        r->cigar_text = static_cast<char*>(g_pool.get(total_text + 16, false));
        if (c.distance) r->text_end = static_cast<uint64_t*>(g_pool.get((n + 1) * 8, false));
        if (!r->edit_distance || !r->pair_status || !r->run_offset || !r->cigar_offset || !r->runs || !r->cigar_text || (c.distance && !r->text_end))
            return bail(SCRG_ERR_OOM, "result arrays");
        OffsetStream st[2];
        int n_streams = 0;
        if (c.want_runs) st[n_streams++] = OffsetStream{c.iss_run_off, c.runs.p, r->run_offset, reinterpret_cast<char*>(r->runs), 2};
        if (c.want_text) st[n_streams++] = OffsetStream{c.iss_text_off, c.text.p, r->cigar_offset, r->cigar_text, 1};
        streams_to_caller(c, st, n_streams, [&](uint64_t k, uint64_t p) {
            r->edit_distance[p] = c.iss_ed[k];
            r->pair_status[p] = c.iss_status[k];
            if (c.distance) r->text_end[p] = c.iss_tend[k];
        });
    }
    r->edit_distance[n] = 0;
    r->pair_status[n] = 0;
    if (r->text_end) r->text_end[n] = 0;
    if (!c.want_runs) memset(r->run_offset, 0, (n + 1) * sizeof(uint64_t));
    if (!c.want_text) memset(r->cigar_offset, 0, (n + 1) * sizeof(uint64_t));
    // ---- the side results, in caller order
    if (opt.diff_kind) {
        c.iss_diff_off[n] = total_diff;
        if (!c.diff.p) c.diff.p = static_cast<char*>(g_diff_pool.get(16, true));
        scrg_diff* const d = made.diff = static_cast<scrg_diff*>(calloc(1, sizeof(scrg_diff)));
        if (!c.diff.p || !d) return bail(SCRG_ERR_OOM, "difference strings");
        d->n_pairs = n;
        d->kind = opt.diff_kind;
        if (c.identity) {
            d->offset = std::exchange(c.iss_diff_off, nullptr);
            d->text = std::exchange(c.diff.p, nullptr);
        } else {
            d->offset = static_cast<uint64_t*>(g_diff_pool.get((n + 1) * 8, false));
            d->text = static_cast<char*>(g_diff_pool.get(total_diff + 16, false));
            if (!d->offset || !d->text) return bail(SCRG_ERR_OOM, "difference strings");
            const OffsetStream ds_text{c.iss_diff_off, c.diff.p, d->offset, d->text, 1};
            streams_to_caller(c, &ds_text, 1, [](uint64_t, uint64_t) {});
        }
    }
    if (opt.report) {
        scrg_report* const rp = made.report = static_cast<scrg_report*>(calloc(1, sizeof(scrg_report)));
        if (rp) rp->pairs = records_to_caller<scrg_pair_report>(c, REC_REPORT);
        if (!rp || !rp->pairs) return bail(SCRG_ERR_OOM, "alignment report");
        rp->n_pairs = n;
        for (uint64_t k = 0; k < n; k++) rp->n_failed += rp->pairs[k].verdict != 0 && rp->pairs[k].verdict != SCRG_REPORT_NO_ALIGNMENT;
    }
    if (opt.clip) {
        scrg_clip* const cl = made.clip = static_cast<scrg_clip*>(calloc(1, sizeof(scrg_clip)));
        if (cl) cl->pairs = records_to_caller<scrg_pair_clip>(c, REC_CLIP);
        if (!cl || !cl->pairs) return bail(SCRG_ERR_OOM, "clip records");
        cl->n_pairs = n;
        memcpy(cl->costs, opt.clip_costs, sizeof(cl->costs));
    }
    if (c.mates) {
        scrg_mates* const mt = made.mates = static_cast<scrg_mates*>(calloc(1, sizeof(scrg_mates)));
        if (!mt) return bail(SCRG_ERR_OOM, "mate records");
        mt->n_mates = b.n_reads / 2;
        mt->records = std::exchange(c.mate_rec, nullptr);
    }
    if (c.summary) {
        scrg_read_summaries* const sm = made.summary = static_cast<scrg_read_summaries*>(calloc(1, sizeof(scrg_read_summaries)));
        if (!sm) return bail(SCRG_ERR_OOM, "read summary");
        sm->n_reads = b.n_reads;
        sm->reads = std::exchange(c.sum_rec, nullptr);
        sm->rule = opt.mapq_rule;
    }
    r->kernel_ns = c.kernel_ns.load();
    if (scrg_get_log() && r->kernel_ns > 0)   // the reference's log line, src/genasm_gpu.cu:949-951 (kernel time: the sum over the chunks' launches)
        fprintf(stderr, "core algorithm ran at %lld aligns/second\n", (long long)((double)n * 1e9 / (double)r->kernel_ns));
    r->pack_ns = c.pack_ns.load();
    r->total_ns = now_ns() - t_begin;
    if (getenv("SCRG_HOST_TIMING"))
        fprintf(stderr, "[scrooge_amd host] total %.3f ms (results in %s order)\n", r->total_ns / 1e6, c.identity ? "issue = caller" : "caller (permuted)");
    *out = std::exchange(res.r, nullptr);
    if (side) side->take_from(made);
    if (c.any_overflow.load()) {
        if (err) *err = "at least one pair overflowed its CIGAR slice (see pair_status)";
        return SCRG_ERR_CIGAR_OVERFLOW;
    }
    return SCRG_OK;
}

}  // namespace scrg_host
