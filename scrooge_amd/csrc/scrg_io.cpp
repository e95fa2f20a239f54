// scrg_io.cpp — file formats and result checks either side of the hot path
// (include/scrooge_amd_io.h).  Restates the behaviour of the reference's
// src/util.cpp readers and src/tests.cu / src/cpu_baseline.cpp checks; written
// against the formats, not translated from the reference sources.

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <sstream>
#include <memory>
#include <new>
#include <atomic>
#include <string>
#include <thread>
#include <vector>

#include "../../include/scrooge_amd_io.h"
#include "clip_rule.h"
#include "pileup_rule.h"
#include "site_rule.h"
#include "mate_rule.h"
#include "mapq_rule.h"
#include "seed_rule.h"

namespace {

bool slurp(const std::string& path, std::string& out, std::string& err)
{
    std::ifstream f(path, std::ios::binary);
    if (!f) {
        err = "could not read file \"" + path + "\"";
        return false;
    }
    f.seekg(0, std::ios::end);
    const std::streamoff n = f.tellg();
    if (!f || n < 0) {                     // a directory or an unseekable path
        err = "could not read file \"" + path + "\"";
        return false;
    }
    f.seekg(0, std::ios::beg);
    out.resize((size_t)n);
    if (n) f.read(&out[0], n);
    if (!f) {
        err = "could not read file \"" + path + "\"";
        return false;
    }
    return true;
}

struct Chromosome {
    std::string name;
    uint64_t start, len;
};

struct Candidate {
    std::string read_name, chromosome;
    long long start_in_chromosome = 0;
    long long start_of_aligned_region = 0;
    long long size_of_aligned_region = 0;
    bool forward = true;
};

// FASTA (src/util.cpp:45-92): the description is the whole header line; content skips
// newlines, carriage returns and blanks up to the next '>'.
void parse_fasta(const std::string& raw, std::string& content, std::vector<Chromosome>& chroms)
{
    size_t i = 0;
    const size_t n = raw.size();
    while (i < n) {
        while (i < n && raw[i] != '>') i++;
        if (i >= n) break;
        i++;
        Chromosome c;
        while (i < n && raw[i] != '\n' && raw[i] != '\r') c.name.push_back(raw[i++]);
        c.start = content.size();
        while (i < n && raw[i] != '>') {
            const char ch = raw[i++];
            if (ch != '\n' && ch != '\r' && ch != ' ') content.push_back(ch);
        }
        c.len = content.size() - c.start;
        chroms.push_back(c);
    }
}

struct FastqRead {
    std::string name, seq;
};

// FASTQ: '@' header (blanks and CRs removed from the name, src/util.cpp:134-141), one sequence
// line, '+' line, quality line.  Unlike the reference's scan for the next '@' character
// (src/util.cpp:123-130), records are consumed as four lines, so an '@' inside a quality
// string cannot start a bogus record; on files without such characters both agree.
void parse_fastq(const std::string& raw, std::vector<FastqRead>& reads)
{
    size_t i = 0;
    const size_t n = raw.size();
    auto next_line = [&](size_t& b, size_t& e) {
        b = i;
        while (i < n && raw[i] != '\n') i++;
        e = i;
        if (i < n) i++;
        while (e > b && raw[e - 1] == '\r') e--;
    };
    while (i < n) {
        size_t b, e;
        next_line(b, e);
        if (e == b || raw[b] != '@') continue;
        FastqRead r;
        for (size_t k = b + 1; k < e; k++)
            if (raw[k] != ' ' && raw[k] != '\r') r.name.push_back(raw[k]);
        next_line(b, e);
        r.seq.assign(raw, b, e - b);
        const size_t save = i;
        next_line(b, e);
        if (e > b && raw[b] == '+') next_line(b, e);   // quality line
        else i = save;                                    // sequence-only record
        reads.push_back(std::move(r));
    }
}

// MAF as written by PBSIM (src/util.cpp:175-236): an 'a' line opens a block, 's' lines carry
// "src start size strand srcSize text"; the line whose src is "ref" gives the reference start.
void parse_maf(const std::string& raw, std::vector<Candidate>& out)
{
    std::istringstream in(raw);
    std::string line;
    while (std::getline(in, line)) {
        while (!line.empty() && (line.back() == '\r' || line.back() == '\n')) line.pop_back();
        if (line.empty() || line[0] != 'a') continue;
        Candidate c;
        while (std::getline(in, line)) {
            while (!line.empty() && (line.back() == '\r' || line.back() == '\n')) line.pop_back();
            if (line.empty()) break;
            if (line[0] != 's') continue;
            std::istringstream ls(line.substr(1));
            std::string src, strand, text;
            long long start = 0, size = 0, src_size = 0;
            ls >> src >> start >> size >> strand >> src_size >> text;
            if (src == "ref") {
                c.start_in_chromosome = start;
                c.chromosome = "ref";
            } else {
                c.read_name = src;
                c.forward = (strand == "+");
                c.start_of_aligned_region = start;
                c.size_of_aligned_region = size;
            }
        }
        out.push_back(c);
    }
}

// PAF (src/util.cpp:238-276): qname qlen qstart qend strand tname tlen tstart tend matches alnlen ...
bool parse_paf(const std::string& raw, std::vector<Candidate>& out, std::string& err)
{
    std::istringstream in(raw);
    std::string line;
    size_t lineno = 0;
    while (std::getline(in, line)) {
        lineno++;
        while (!line.empty() && (line.back() == '\r' || line.back() == '\n')) line.pop_back();
        if (line.empty()) continue;
        std::vector<std::string> f;
        size_t b = 0;
        while (b <= line.size() && f.size() < 12) {
            size_t e = line.find('\t', b);
            if (e == std::string::npos) e = line.size();
            f.push_back(line.substr(b, e - b));
            b = e + 1;
        }
        if (f.size() < 9) {
            err = "PAF line " + std::to_string(lineno) + " has fewer than 9 columns";
            return false;
        }
        Candidate c;
        c.read_name = f[0];
        const long long qstart = atoll(f[2].c_str()), qend = atoll(f[3].c_str());
        c.forward = (f[4] == "+");
        c.chromosome = f[5];
        c.start_in_chromosome = atoll(f[7].c_str());
        c.start_of_aligned_region = qstart;
        c.size_of_aligned_region = qend - qstart;
        out.push_back(c);
    }
    return true;
}

bool ends_with(const std::string& s, const char* suf)
{
    const size_t n = strlen(suf);
    return s.size() >= n && s.compare(s.size() - n, n, suf) == 0;
}

void set_err(char* err, size_t n, const std::string& msg)
{
    if (err && n) {
        snprintf(err, n, "%s", msg.c_str());
    }
}

}  // namespace

struct scrg_job {
    std::string genome;
    std::vector<Chromosome> chroms;
    std::vector<std::string> read_names, read_seqs;
    std::vector<const char*> read_ptrs;
    std::vector<uint64_t> read_lens, cand_offsets, cand_start, cand_chrom, cand_start_in_chrom;
    std::vector<uint8_t> cand_reverse;
    std::vector<uint64_t> pair_read;   // read index of every pair
};

// The entry points below never let a C++ exception cross the C boundary: allocation failures become
// SCRG_ERR_OOM, anything else SCRG_ERR_INVALID_ARG.
template <typename F> static scrg_status guarded(F&& f)
{
    try {
        return f();
    } catch (const std::bad_alloc&) {
        return SCRG_ERR_OOM;
    } catch (...) {
        return SCRG_ERR_INVALID_ARG;
    }
}

extern "C" {

void scrg_job_options_default(scrg_job_options* o)
{
    if (!o) return;
    o->reverse_strand = 0;
    o->sort_by_length = 1;
    o->inflation = 1;
    o->left_extend = 1;
    o->read_length_cap = -1;
}

static scrg_status job_load_impl(const char* genome_fasta, const char* reads_fastq, const char* seeds_path,
                          const scrg_job_options* opt_in, scrg_job** out, char* err, size_t err_len, bool seeded = true)
{
    if (!genome_fasta || !reads_fastq || (seeded && !seeds_path) || !out) return SCRG_ERR_INVALID_ARG;
    *out = nullptr;
    scrg_job_options opt;
    scrg_job_options_default(&opt);
    if (opt_in) opt = *opt_in;
    std::string raw, msg;
    std::unique_ptr<scrg_job> job_owner(new scrg_job());       // released to the caller on success only
    scrg_job* job = job_owner.get();
    auto fail = [&](scrg_status s, const std::string& m) {
        set_err(err, err_len, m);
        return s;
    };

    if (!slurp(genome_fasta, raw, msg)) return fail(SCRG_ERR_IO, msg);
    parse_fasta(raw, job->genome, job->chroms);
    std::map<std::string, size_t> chrom_idx;
    // seeds name chromosomes by the full header line (as the reference's map does) or, as PAF
    // writers do, by its first word
    for (size_t k = 0; k < job->chroms.size(); k++) {
        const std::string& nm = job->chroms[k].name;
        chrom_idx.emplace(nm.substr(0, nm.find_first_of(" \t")), k);
    }
    for (size_t k = 0; k < job->chroms.size(); k++) chrom_idx[job->chroms[k].name] = k;

    std::vector<FastqRead> reads;
    if (!slurp(reads_fastq, raw, msg)) return fail(SCRG_ERR_IO, msg);
    parse_fastq(raw, reads);

    std::vector<Candidate> cands;
    if (seeded) {
        if (!slurp(seeds_path, raw, msg)) return fail(SCRG_ERR_IO, msg);
        const std::string sp(seeds_path);
        if (ends_with(sp, ".paf")) {
            if (!parse_paf(raw, cands, msg)) return fail(SCRG_ERR_FORMAT, msg);
        } else if (ends_with(sp, ".maf")) {
            parse_maf(raw, cands);
        } else {
            return fail(SCRG_ERR_FORMAT, "unknown seed file ending (want .maf or .paf)");   // src/util.cpp:312-314
        }
    } else if (job->chroms.empty()) {                    // scrg_job_load_unseeded: no pairs until scrg_job_seed installs them
        return fail(SCRG_ERR_FORMAT, "genome FASTA holds no sequence");
    }

    std::map<std::string, size_t> read_idx;
    for (size_t k = 0; k < reads.size(); k++) read_idx[reads[k].name] = k;
    std::vector<std::vector<size_t>> per_read(reads.size());
    for (size_t k = 0; k < cands.size(); k++) {
        auto it = read_idx.find(cands[k].read_name);
        if (it == read_idx.end())   // src/util.cpp:326-329 exits here
            return fail(SCRG_ERR_FORMAT, "candidate location specified unknown read \"" + cands[k].read_name + "\"");
        per_read[it->second].push_back(k);
    }

    // read order: optional inflation, then longest first (stable), as src/tests.cu:366-377
    std::vector<size_t> order;
    const int infl = opt.inflation > 1 ? opt.inflation : 1;
    for (int rep = 0; rep < infl; rep++)
        for (size_t k = 0; k < reads.size(); k++) order.push_back(k);
    auto capped_len = [&](size_t k) {
        const size_t L = reads[k].seq.size();
        return (opt.read_length_cap >= 0 && (size_t)opt.read_length_cap < L) ? (size_t)opt.read_length_cap : L;
    };
    if (opt.sort_by_length)
        std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return capped_len(a) > capped_len(b); });

    job->cand_offsets.push_back(0);
    for (size_t k : order) {
        const size_t L = capped_len(k);
        const size_t full_len = reads[k].seq.size();
        job->read_names.push_back(reads[k].name);
        job->read_seqs.push_back(reads[k].seq.substr(0, L));
        job->read_lens.push_back(L);
        for (size_t ci : per_read[k]) {
            const Candidate& c = cands[ci];
            if (!c.forward && !opt.reverse_strand) continue;   // src/tests.cu:346-355
            size_t chrom = 0;
            if (job->chroms.size() > 1) {   // get_global_seeds, src/util.cpp:292-301
                auto it = chrom_idx.find(c.chromosome);
                if (it == chrom_idx.end())
                    return fail(SCRG_ERR_FORMAT, "candidate location names unknown chromosome \"" + c.chromosome + "\"");
                chrom = it->second;
            } else if (job->chroms.empty()) {
                return fail(SCRG_ERR_FORMAT, "genome FASTA holds no sequence");
            }
            long long start = c.start_in_chromosome;
            if (opt.left_extend) {
                // left_extend_locations (src/util.cpp:284-290): move the start back by the unaligned
                // read prefix.  On the reverse strand the prefix of the reverse-complemented read is
                // the unaligned SUFFIX of the original read.
                long long lead = c.forward ? c.start_of_aligned_region
                                           : (long long)full_len - (c.start_of_aligned_region + c.size_of_aligned_region);
                if (lead < 0) lead = 0;
                start = std::max(0ll, start - lead);
            }
            uint64_t s = (uint64_t)std::max(0ll, start);
            if (s > job->chroms[chrom].len) s = job->chroms[chrom].len;
            job->cand_chrom.push_back(chrom);
            job->cand_start_in_chrom.push_back(s);
            job->cand_start.push_back(job->chroms[chrom].start + s);
            job->cand_reverse.push_back(c.forward ? 0 : 1);
            job->pair_read.push_back(job->read_names.size() - 1);
        }
        job->cand_offsets.push_back(job->cand_start.size());
    }
    for (const std::string& s : job->read_seqs) job->read_ptrs.push_back(s.data());
    *out = job_owner.release();
    return SCRG_OK;
}

scrg_status scrg_job_load(const char* genome_fasta, const char* reads_fastq, const char* seeds_path,
                          const scrg_job_options* opt_in, scrg_job** out, char* err, size_t err_len)
{
    const scrg_status st = guarded([&] { return job_load_impl(genome_fasta, reads_fastq, seeds_path, opt_in, out, err, err_len); });
    if (st == SCRG_ERR_OOM) set_err(err, err_len, "out of memory while loading the job");
    return st;
}

void scrg_job_free(scrg_job* job) { delete job; }

void scrg_job_counts(const scrg_job* job, uint64_t* n_reads, uint64_t* n_pairs, uint64_t* genome_len,
                     uint64_t* n_chromosomes)
{
    if (!job) return;
    if (n_reads) *n_reads = job->read_lens.size();
    if (n_pairs) *n_pairs = job->cand_start.size();
    if (genome_len) *genome_len = job->genome.size();
    if (n_chromosomes) *n_chromosomes = job->chroms.size();
}

void scrg_job_arrays(const scrg_job* job, const char** genome, const char* const** reads, const uint64_t** read_lens,
                     const uint64_t** cand_offsets, const uint64_t** cand_start, const uint8_t** cand_reverse)
{
    if (!job) return;
    if (genome) *genome = job->genome.data();
    if (reads) *reads = job->read_ptrs.data();
    if (read_lens) *read_lens = job->read_lens.data();
    if (cand_offsets) *cand_offsets = job->cand_offsets.data();
    if (cand_start) *cand_start = job->cand_start.data();
    if (cand_reverse) *cand_reverse = job->cand_reverse.data();
}

const char* scrg_job_read_name(const scrg_job* job, uint64_t read)
{
    return (job && read < job->read_names.size()) ? job->read_names[read].c_str() : "";
}

const char* scrg_job_pair_chromosome(const scrg_job* job, uint64_t pair, uint64_t* start_in_chromosome,
                                     uint64_t* chromosome_len)
{
    if (!job || pair >= job->cand_start.size()) return "";
    const Chromosome& c = job->chroms[job->cand_chrom[pair]];
    if (start_in_chromosome) *start_in_chromosome = job->cand_start_in_chrom[pair];
    if (chromosome_len) *chromosome_len = c.len;
    return c.name.c_str();
}

scrg_status scrg_job_align(scrg_ctx* ctx, const scrg_params* params, const scrg_job* job, scrg_result** out)
{
    if (!job) return SCRG_ERR_INVALID_ARG;
    return scrg_align_mapping_stranded(ctx, params, job->genome.data(), job->genome.size(), job->read_lens.size(),
                                       job->read_ptrs.data(), job->read_lens.data(), job->cand_offsets.data(),
                                       job->cand_start.data(), job->cand_reverse.data(), out);
}

// Paired-end mapping of a job: its reads 2m and 2m+1 are mates (interleaved FASTQ).  The call runs against the resident genome,
// so the job's is made resident first.
scrg_status scrg_job_align_paired(scrg_ctx* ctx, const scrg_params* params, const scrg_job* job, const scrg_mate_rule* rule, scrg_mates** mates,
                                  scrg_result** out)
{
    if (mates) *mates = nullptr;
    if (out) *out = nullptr;
    if (!job || !mates || !out) return SCRG_ERR_INVALID_ARG;
    if (job->read_lens.size() % 2) return SCRG_ERR_FORMAT;
    const scrg_status s = scrg_genome_set(ctx, job->genome.data(), job->genome.size());
    if (s != SCRG_OK) return s;
    return scrg_align_mapping_paired(ctx, params, job->read_lens.size(), job->read_ptrs.data(), job->read_lens.data(), job->cand_offsets.data(),
                                     job->cand_start.data(), job->cand_reverse.data(), rule, mates, out);
}

scrg_status scrg_job_load_unseeded(const char* genome_fasta, const char* reads_fastq, const scrg_job_options* opt_in, scrg_job** out, char* err,
                                   size_t err_len)
{
    const scrg_status st = guarded([&] { return job_load_impl(genome_fasta, reads_fastq, nullptr, opt_in, out, err, err_len, false); });
    if (st == SCRG_ERR_OOM) set_err(err, err_len, "out of memory while loading the job");
    return st;
}

// ---- seeding on the host: seed_rule.h, the text the kernels compile, on ASCII and with an index of its own ----
static int seed_base_code(char c)
{
    switch (c) {
    case 'A': case 'a': return 0;
    case 'C': case 'c': return 1;
    case 'G': case 'g': return 2;
    case 'T': case 't': return 3;
    default: return -1;
    }
}

// the keys of every window of k bases of `codes` (n of them, 0 .. 3): key[i] = sum of codes[i + j] 4^(k-1-j)
static void seed_keys_of(const uint8_t* codes, uint64_t n, uint32_t k, std::vector<uint32_t>& keys)
{
    keys.clear();
    if (n < k) return;
    const uint64_t mask = k == 16 ? 0xffffffffull : (1ull << (2 * k)) - 1u;
    uint64_t key = 0;
    for (uint64_t i = 0; i < n; i++) {
        key = ((key << 2) | codes[i]) & mask;
        if (i + 1 >= k) keys.push_back((uint32_t)key);
    }
}

scrg_status scrg_candidates_from_genome(const scrg_seed_rule* rule, const char* genome, uint64_t genome_len, uint64_t n_reads, const char* const* reads,
                                        const uint64_t* read_lens, scrg_candidates** out)
{
    return scrg_candidates_from_genome_sampled(rule, 0, genome, genome_len, n_reads, reads, read_lens, out, nullptr, nullptr);
}

scrg_status scrg_candidates_from_genome_sampled(const scrg_seed_rule* rule, uint32_t smer, const char* genome, uint64_t genome_len, uint64_t n_reads,
                                                const char* const* reads, const uint64_t* read_lens, scrg_candidates** out, uint64_t* n_entries,
                                                uint64_t* n_lookups)
{
    if (out) *out = nullptr;
    if (n_entries) *n_entries = 0;
    if (n_lookups) *n_lookups = 0;
    if (!out || (genome_len && !genome) || (n_reads && (!reads || !read_lens))) return SCRG_ERR_INVALID_ARG;
    scrg_seed_rule k;
    scrg_seed_rule_default(&k);
    if (rule) k = *rule;
    if (scrg_seed_rule_check(&k, genome_len) != SCRG_OK || !scrg::seed_smer_valid(smer, k.k)) return SCRG_ERR_INVALID_ARG;
    return guarded([&]() -> scrg_status {
        // the index: (key << 32 | p), sorted
        std::vector<uint8_t> gcodes(genome_len);
        for (uint64_t i = 0; i < genome_len; i++) {
            const int c = seed_base_code(genome[i]);
            if (c < 0) return SCRG_ERR_BAD_BASE;
            gcodes[i] = (uint8_t)c;
        }
        std::vector<uint64_t> index;
        {
            std::vector<uint32_t> gkeys;
            seed_keys_of(gcodes.data(), genome_len, k.k, gkeys);
            for (uint64_t p = 0; p < gkeys.size(); p += k.stride)
                if (scrg::seed_key_selected(gkeys[p], k.k, smer)) index.push_back(((uint64_t)gkeys[p] << 32) | p);
            std::sort(index.begin(), index.end());
        }
        for (uint64_t r = 0; r < n_reads; r++) {
            if (read_lens[r] > scrg::SEED_MAX_READ || (read_lens[r] && !reads[r])) return SCRG_ERR_INVALID_ARG;
            for (uint64_t i = 0; i < read_lens[r]; i++)
                if (seed_base_code(reads[r][i]) < 0) return SCRG_ERR_BAD_BASE;
        }
        struct Cand {
            uint32_t start, votes;
            uint8_t strand;
        };
        std::vector<std::vector<Cand>> per_read(n_reads);
        std::atomic<uint64_t> next{0}, n_hits{0}, n_clusters{0}, n_over{0}, n_looked{0};
        const uint32_t n_strands = k.strands == 3u ? 2u : 1u;
        std::atomic<int> failed{0};                      // 1: out of memory, 2: anything else — a worker thread lets no exception out
        auto work_body = [&] {
            std::vector<uint8_t> codes;
            std::vector<uint32_t> keys;
            std::vector<std::pair<uint64_t, uint32_t>> hits;      // (word, r)
            std::vector<scrg::SeedRank> ranks;
            for (;;) {
                const uint64_t r = next.fetch_add(1);
                if (r >= n_reads || failed.load(std::memory_order_relaxed)) break;
                const uint64_t L = read_lens[r];
                hits.clear();
                uint64_t over = 0, looked = 0;
                for (uint32_t strand = 0; strand < n_strands; strand++) {
                    codes.resize(L);
                    for (uint64_t i = 0; i < L; i++)
                        codes[i] = (uint8_t)(strand ? 3 - seed_base_code(reads[r][L - 1 - i]) : seed_base_code(reads[r][i]));
                    seed_keys_of(codes.data(), L, k.k, keys);
                    for (uint64_t q = 0; q < keys.size(); q++) {
                        if (!scrg::seed_key_selected(keys[q], k.k, smer)) continue;
                        looked++;
                        const auto a = std::lower_bound(index.begin(), index.end(), (uint64_t)keys[q] << 32);
                        const auto e = std::upper_bound(a, index.end(), ((uint64_t)keys[q] << 32) | 0xffffffffull);
                        if ((uint64_t)(e - a) > k.max_occ) {
                            over++;
                            continue;
                        }
                        for (auto it = a; it != e; ++it) hits.emplace_back(scrg::seed_hit_word(0, strand, (uint32_t)*it, (uint32_t)q), (uint32_t)q);
                    }
                }
                std::sort(hits.begin(), hits.end());
                ranks.clear();
                uint64_t clusters = 0;
                for (size_t i = 0; i < hits.size();) {
                    size_t j = i + 1;
                    uint64_t anchor = scrg::seed_anchor_word(hits[i].second, scrg::seed_hit_dbias(hits[i].first));
                    while (j < hits.size() && !scrg::seed_is_head(hits[j - 1].first, hits[j].first, k.band)) {
                        anchor = std::min(anchor, scrg::seed_anchor_word(hits[j].second, scrg::seed_hit_dbias(hits[j].first)));
                        j++;
                    }
                    if (j - i >= k.min_hits)
                        ranks.push_back(scrg::seed_rank((uint32_t)(j - i), scrg::seed_anchor_start(anchor), scrg::seed_hit_strand(hits[i].first), (uint32_t)clusters));
                    clusters++;
                    i = j;
                }
                std::sort(ranks.begin(), ranks.end(), [](const scrg::SeedRank& x, const scrg::SeedRank& y) { return scrg::seed_rank_less(x, y); });
                for (size_t c = 0; c < ranks.size() && c < k.max_candidates; c++)
                    per_read[r].push_back(Cand{scrg::seed_rank_start(ranks[c]), scrg::seed_rank_votes(ranks[c]), (uint8_t)scrg::seed_rank_strand(ranks[c])});
                n_hits += hits.size();
                n_clusters += clusters;
                n_over += over;
                n_looked += looked;
            }
        };
        auto work = [&] {
            try {
                work_body();
            } catch (const std::bad_alloc&) {
                failed.store(1);
            } catch (...) {
                failed.store(2);
            }
        };
        {
            const unsigned hw = std::thread::hardware_concurrency();
            const unsigned nt = (unsigned)std::min<uint64_t>(std::min(hw ? hw : 4u, 16u), std::max<uint64_t>(1, n_reads / 64));
            std::vector<std::thread> threads;
            for (unsigned t = 1; t < nt; t++) threads.emplace_back(work);
            work();
            for (std::thread& t : threads) t.join();
        }
        if (failed.load()) return failed.load() == 1 ? SCRG_ERR_OOM : SCRG_ERR_INVALID_ARG;
        std::unique_ptr<scrg_candidates, void (*)(scrg_candidates*)> res(static_cast<scrg_candidates*>(calloc(1, sizeof(scrg_candidates))), scrg_candidates_free);
        if (!res) return SCRG_ERR_OOM;
        uint64_t total = 0;
        for (const auto& v : per_read) total += v.size();
        res->n_reads = n_reads;
        res->rule = k;
        if (!res->rule.hit_budget_mb) res->rule.hit_budget_mb = scrg::SEED_DEFAULT_BUDGET_MB;
        res->n_hits = n_hits.load();
        res->n_clusters = n_clusters.load();
        res->n_keys_over_max_occ = n_over.load();
        res->cand_offsets = static_cast<uint64_t*>(calloc(n_reads + 1, sizeof(uint64_t)));
        res->cand_start = static_cast<uint64_t*>(malloc((total + 1) * sizeof(uint64_t)));
        res->cand_reverse = static_cast<uint8_t*>(malloc(total + 1));
        res->cand_votes = static_cast<uint32_t*>(malloc((total + 1) * sizeof(uint32_t)));
        if (!res->cand_offsets || !res->cand_start || !res->cand_reverse || !res->cand_votes) return SCRG_ERR_OOM;
        uint64_t at = 0;
        for (uint64_t r = 0; r < n_reads; r++) {
            for (const Cand& c : per_read[r]) {
                res->cand_start[at] = c.start;
                res->cand_reverse[at] = c.strand;
                res->cand_votes[at] = c.votes;
                at++;
            }
            res->cand_offsets[r + 1] = at;
        }
        if (n_entries) *n_entries = index.size();
        if (n_lookups) *n_lookups = n_looked.load();
        *out = res.release();
        return SCRG_OK;
    });
}

// The job's genome made resident and indexed, its reads' candidates found on the GPU and installed as its pairs.
scrg_status scrg_job_seed(scrg_ctx* ctx, const scrg_seed_rule* rule, scrg_job* job)
{
    if (!ctx || !job) return SCRG_ERR_INVALID_ARG;
    scrg_status s = scrg_genome_set(ctx, job->genome.data(), job->genome.size());
    if (s == SCRG_OK) s = scrg_genome_index(ctx, rule);
    if (s != SCRG_OK) return s;
    scrg_candidates* c = nullptr;
    s = scrg_find_candidates(ctx, job->read_lens.size(), job->read_ptrs.data(), job->read_lens.data(), &c);
    if (s != SCRG_OK) return s;
    std::unique_ptr<scrg_candidates, void (*)(scrg_candidates*)> owner(c, scrg_candidates_free);
    return guarded([&]() -> scrg_status {
        if (job->chroms.empty()) return SCRG_ERR_FORMAT;
        const uint64_t n = c->cand_offsets[c->n_reads];
        std::vector<uint64_t> start(c->cand_start, c->cand_start + n), chrom(n), in_chrom(n), pair_read(n);
        for (uint64_t r = 0; r < c->n_reads; r++)
            for (uint64_t p = c->cand_offsets[r]; p < c->cand_offsets[r + 1]; p++) pair_read[p] = r;
        for (uint64_t p = 0; p < n; p++) {
            // the chromosome that holds the start (a candidate across a seam belongs to the one it starts in)
            const auto it = std::upper_bound(job->chroms.begin(), job->chroms.end(), start[p], [](uint64_t x, const Chromosome& ch) { return x < ch.start; });
            chrom[p] = it == job->chroms.begin() ? 0 : (uint64_t)(it - job->chroms.begin()) - 1;
            in_chrom[p] = start[p] - job->chroms[chrom[p]].start;
        }
        job->cand_offsets.assign(c->cand_offsets, c->cand_offsets + c->n_reads + 1);
        job->cand_start.swap(start);
        job->cand_reverse.assign(c->cand_reverse, c->cand_reverse + n);
        job->cand_chrom.swap(chrom);
        job->cand_start_in_chrom.swap(in_chrom);
        job->pair_read.swap(pair_read);
        return SCRG_OK;
    });
}

// The text bases pair k's alignment consumed: from its runs, or — a result without runs (SCRG_OUT_TEXT) — from its CIGAR text
static void consumed_of(const scrg_result* res, uint64_t k, uint64_t* tcons, uint64_t* matches, uint64_t* cols)
{
    *tcons = *matches = *cols = 0;
    if (res->run_offset[k + 1] > res->run_offset[k]) {
        for (uint64_t q = res->run_offset[k]; q < res->run_offset[k + 1]; q++) {
            const unsigned n = res->runs[q].count;
            const char op = res->runs[q].op;
            if (op != 'I') *tcons += n;
            if (op == '=') *matches += n;
            *cols += n;
        }
        return;
    }
    uint64_t n = 0;
    for (const char* c = res->cigar_text + res->cigar_offset[k]; *c; c++) {
        if (*c >= '0' && *c <= '9') {
            n = 10 * n + (uint64_t)(*c - '0');
            continue;
        }
        if (*c != 'I') *tcons += n;
        if (*c == '=') *matches += n;
        *cols += n;
        n = 0;
    }
}

static scrg_status job_write_paired_impl(const scrg_job* job, const scrg_result* res, const scrg_mates* mates, const char* path, int format)
{
    if (!job || !res || !mates || !path || (format != 0 && format != 1)) return SCRG_ERR_INVALID_ARG;
    const uint64_t n_reads = job->read_lens.size(), n = res->n_pairs;
    if (n != job->cand_start.size() || n_reads % 2 || mates->n_mates != n_reads / 2 || (mates->n_mates && !mates->records)) return SCRG_ERR_INVALID_ARG;
    if (res->text_end) return SCRG_ERR_INVALID_ARG;          // (a distance-only result has no CIGARs: no SAM column 6, no TLEN)
    // every winner is a pair of its own read
    for (uint64_t r = 0; r < n_reads; r++) {
        const uint64_t w = mates->records[r / 2].winner[r % 2];
        if (w != ~0ull && (w >= n || job->pair_read[w] != r)) return SCRG_ERR_INVALID_ARG;
    }
    FILE* f = fopen(path, "w");
    if (!f) return SCRG_ERR_IO;
    if (format == 1) {
        fprintf(f, "@HD\tVN:1.6\tSO:unknown\n");
        for (const Chromosome& c : job->chroms) {
            std::string nm = c.name.substr(0, c.name.find_first_of(" \t"));
            fprintf(f, "@SQ\tSN:%s\tLN:%llu\n", nm.c_str(), (unsigned long long)c.len);
        }
        fprintf(f, "@PG\tID:scrooge_amd\tPN:scrooge_amd\n");
    }
    auto chrom_name = [&](uint64_t k) {
        const Chromosome& c = job->chroms[job->cand_chrom[k]];
        return c.name.substr(0, c.name.find_first_of(" \t"));
    };
    for (uint64_t r = 0; r < n_reads; r++) {
        const scrg_mate_record& rec = mates->records[r / 2];
        const uint64_t side = r % 2, w = rec.winner[side], mw = rec.winner[1 - side];
        const bool has = w != ~0ull, mate_has = mw != ~0ull;
        uint64_t tcons = 0, matches = 0, cols = 0, m_tcons = 0, m_matches = 0, m_cols = 0;
        if (has) consumed_of(res, w, &tcons, &matches, &cols);
        if (mate_has) consumed_of(res, mw, &m_tcons, &m_matches, &m_cols);
        if (format == 0) {
            // PAF: the winners only, as best-candidate mode's
            if (!has) continue;
            const Chromosome& c = job->chroms[job->cand_chrom[w]];
            const uint64_t ts = job->cand_start_in_chrom[w];
            fprintf(f, "%s\t%llu\t0\t%llu\t%c\t%s\t%llu\t%llu\t%llu\t%llu\t%llu\t255\tNM:i:%lld\tcg:Z:%s\ttp:A:P\n", job->read_names[r].c_str(),
                    (unsigned long long)job->read_lens[r], (unsigned long long)job->read_lens[r], job->cand_reverse[w] ? '-' : '+', chrom_name(w).c_str(),
                    (unsigned long long)c.len, (unsigned long long)ts, (unsigned long long)(ts + tcons), (unsigned long long)matches, (unsigned long long)cols,
                    (long long)res->edit_distance[w], res->cigar_text + res->cigar_offset[w]);
            continue;
        }
        // SAM: one record per read.  0x1 paired, 0x40 / 0x80 first / last, 0x2 from PROPER — cleared where the mates lie on different
        // chromosomes (the rule saw one concatenated coordinate) —, 0x4 / 0x8 this one / the mate without a winner, 0x10 / 0x20 strands
        const bool same_chrom = has && mate_has && job->cand_chrom[w] == job->cand_chrom[mw];
        const bool rev = has && job->cand_reverse[w] != 0, mate_rev = mate_has && job->cand_reverse[mw] != 0;
        const int flag = 0x1 | (side ? 0x80 : 0x40) | ((rec.flags & SCRG_MATES_PROPER) && same_chrom ? 0x2 : 0) | (has ? 0 : 0x4) | (mate_has ? 0 : 0x8) |
                         (rev ? 0x10 : 0) | (mate_rev ? 0x20 : 0);
        const std::string rnext = !mate_has ? "*" : same_chrom ? "=" : chrom_name(mw);
        const unsigned long long pnext = mate_has ? job->cand_start_in_chrom[mw] + 1 : 0;
        // TLEN: leftmost start to rightmost end of the two winners' alignments, plus for the leftmost mate (equal starts: mate 1), minus
        // for the other; 0 when a mate is absent or on another chromosome
        long long tlen = 0;
        if (same_chrom) {
            const uint64_t s0 = job->cand_start_in_chrom[w], s1 = job->cand_start_in_chrom[mw];
            const uint64_t span = std::max(s0 + tcons, s1 + m_tcons) - std::min(s0, s1);
            const bool leftmost = s0 < s1 || (s0 == s1 && side == 0);
            tlen = leftmost ? (long long)span : -(long long)span;
        }
        std::string seq = job->read_seqs[r];
        if (rev) {
            std::reverse(seq.begin(), seq.end());
            for (char& ch : seq) {
                switch (ch) {
                case 'A': ch = 'T'; break; case 'C': ch = 'G'; break; case 'G': ch = 'C'; break; case 'T': ch = 'A'; break;
                case 'a': ch = 't'; break; case 'c': ch = 'g'; break; case 'g': ch = 'c'; break; case 't': ch = 'a'; break;
                default: break;
                }
            }
        }
        if (!has) {
            fprintf(f, "%s\t%d\t*\t0\t0\t*\t%s\t%llu\t0\t%s\t*\n", job->read_names[r].c_str(), flag, mate_has ? chrom_name(mw).c_str() : "*", pnext,
                    seq.empty() ? "*" : seq.c_str());
            continue;
        }
        const char* const cigar = res->cigar_text + res->cigar_offset[w];
        fprintf(f, "%s\t%d\t%s\t%llu\t%d\t%s\t%s\t%llu\t%lld\t%s\t*\tNM:i:%lld\n", job->read_names[r].c_str(), flag, chrom_name(w).c_str(),
                (unsigned long long)(job->cand_start_in_chrom[w] + 1), (rec.flags & SCRG_MATES_TIED) ? 0 : 255, *cigar ? cigar : "*", rnext.c_str(), pnext, tlen,
                seq.empty() ? "*" : seq.c_str(), (long long)res->edit_distance[w]);
    }
    return fclose(f) == 0 ? (scrg_status)SCRG_OK : (scrg_status)SCRG_ERR_IO;
}

scrg_status scrg_job_write_paired(const scrg_job* job, const scrg_result* res, const scrg_mates* mates, const char* path, int format)
{
    return guarded([&] { return job_write_paired_impl(job, res, mates, path, format); });
}

static scrg_status job_write_impl(const scrg_job* job, const scrg_result* res, const scrg_diff* diff, const scrg_report* report, const int64_t* costs,
                                  const char* path, int format, const scrg_clip* clip = nullptr, const scrg_read_summaries* summary = nullptr);
scrg_status scrg_job_write(const scrg_job* job, const scrg_result* res, const char* path, int format)
{
    return guarded([&] { return job_write_impl(job, res, nullptr, nullptr, nullptr, path, format); });
}
scrg_status scrg_job_write_diff(const scrg_job* job, const scrg_result* res, const scrg_diff* diff, const char* path, int format)
{
    return guarded([&] { return job_write_impl(job, res, diff, nullptr, nullptr, path, format); });
}
scrg_status scrg_job_write_report(const scrg_job* job, const scrg_result* res, const scrg_diff* diff, const scrg_report* report, const int64_t* costs,
                                  const char* path, int format)
{
    return guarded([&] { return job_write_impl(job, res, diff, report, costs, path, format); });
}
scrg_status scrg_job_write_mapq(const scrg_job* job, const scrg_result* res, const scrg_diff* diff, const scrg_report* report, const int64_t* costs,
                                const scrg_read_summaries* summary, const char* path, int format)
{
    return guarded([&] { return job_write_impl(job, res, diff, report, costs, path, format, nullptr, summary); });
}
scrg_status scrg_job_write_clipped(const scrg_job* job, const scrg_result* res, const scrg_clip* clip, const char* path, int format)
{
    return guarded([&] { return job_write_impl(job, res, nullptr, nullptr, nullptr, path, format, clip); });
}
static scrg_status job_write_impl(const scrg_job* job, const scrg_result* res, const scrg_diff* diff, const scrg_report* report, const int64_t* costs,
                                  const char* path, int format, const scrg_clip* clip, const scrg_read_summaries* summary)
{
    if (!job || !res || !path) return SCRG_ERR_INVALID_ARG;
    if (res->n_pairs != job->cand_start.size()) return SCRG_ERR_INVALID_ARG;
    // clip records (scrg_ctx_take_clip; `res` holds the kept stretches): the records say where a stretch lies in the read and in
    // the text — soft clips and a moved POS in SAM, query and target intervals in PAF, AS:i and the stretch's own NM:i in both;
    // TSV has no place for them
    if (clip && (format == 2 || clip->n_pairs != res->n_pairs || (clip->n_pairs && !clip->pairs))) return SCRG_ERR_INVALID_ARG;
    // the alignment report (scrg_ctx_take_report): AS:i and de:f on the PAF and SAM records of pairs that have an alignment, and PAF's
    // columns 10 and 11 without walking the runs; TSV has no tags
    if (report && (format == 2 || report->n_pairs != res->n_pairs || (report->n_pairs && !report->pairs))) return SCRG_ERR_INVALID_ARG;
    static const int64_t default_costs[4] = {2, 4, 4, 2};      // match, mismatch, gap open, gap extend: the reference baseline's default (src/cpu_baseline.cpp:883)
    if (!costs) costs = default_costs;
    // difference strings (scrg_ctx_take_diff): one more tag on the PAF and SAM records of pairs that have an alignment; TSV has no tags
    if (diff && (format == 2 || diff->n_pairs != res->n_pairs || !diff->offset || !diff->text || (diff->kind != SCRG_DIFF_MD && diff->kind != SCRG_DIFF_CS)))
        return SCRG_ERR_INVALID_ARG;
    // the read summaries (scrg_ctx_take_read_summary): a winner's MAPQ instead of 0 / 255; they belong to a result of best-candidate mode
    // (checked below, before anything is written); TSV has no such column
    if (summary && (format == 2 || !res->pair_status || summary->n_reads != job->read_lens.size() || (summary->n_reads && !summary->reads))) return SCRG_ERR_INVALID_ARG;
    for (uint64_t r = 0; summary && r < summary->n_reads; r++) {
        uint64_t w = ~0ull, n_w = 0;
        for (uint64_t k = job->cand_offsets[r]; k < job->cand_offsets[r + 1]; k++)
            if (res->pair_status[k] != (uint32_t)SCRG_PAIR_NOT_BEST && res->pair_status[k] != (uint32_t)SCRG_PAIR_OVER_EDIT_LIMIT) {
                if (!n_w++) w = k;
            }
        if (n_w > 1 || summary->reads[r].winner != w) return SCRG_ERR_INVALID_ARG;
    }
    const char* const diff_tag = !diff ? "" : diff->kind == SCRG_DIFF_MD ? "\tMD:Z:" : "\tcs:Z:";
    // a distance-only result (SCRG_OUT_DISTANCE: text_end is set) has no runs and no text: PAF's columns 10 and 11 and a SAM CIGAR
    // cannot be made from a distance — format 2 (TSV) is what it can be written as
    if (res->text_end && format != 2) return SCRG_ERR_INVALID_ARG;
    FILE* f = fopen(path, "w");
    if (!f) return SCRG_ERR_IO;
    if (format == 1) {
        fprintf(f, "@HD\tVN:1.6\tSO:unknown\n");
        for (const Chromosome& c : job->chroms) {
            std::string nm = c.name.substr(0, c.name.find_first_of(" \t"));
            fprintf(f, "@SQ\tSN:%s\tLN:%llu\n", nm.c_str(), (unsigned long long)c.len);
        }
        fprintf(f, "@PG\tID:scrooge_amd\tPN:scrooge_amd\n");
    }
    // A result of best-candidate mode (SCRG_OUT_BEST) is known by its SCRG_PAIR_NOT_BEST statuses.  Then a read has one
    // record: PAF writes the winners only, as primary (tp:A:P); SAM writes the winner — MAPQ 0 if another eligible candidate
    // has the same edit distance, 255 otherwise — or one unmapped record for a read without a winner; the other pairs are
    // not written.  Without such a status every pair is written, as ever.
    bool best_mode = summary != nullptr;      // (a result in which no read has a loser is best-candidate mode's all the same)
    if (res->pair_status)
        for (uint64_t k = 0; k < res->n_pairs && !best_mode; k++) best_mode = res->pair_status[k] == (uint32_t)SCRG_PAIR_NOT_BEST;
    std::vector<uint8_t> skip, tied, has_winner;          // best mode only: per pair, per pair, per read
    const uint64_t n_reads = job->read_lens.size();
    auto mapq_of = [&](uint64_t k) { return summary ? (int)summary->reads[job->pair_read[k]].mapq : best_mode && tied[k] ? 0 : 255; };
    uint64_t next_read = 0;                   // best mode: reads before this one have their record
    auto unmapped_upto = [&](uint64_t upto) {
        for (; next_read < upto; next_read++) {
            if (format != 1 || has_winner[next_read]) continue;
            const std::string& seq = job->read_seqs[next_read];
            fprintf(f, "%s\t4\t*\t0\t0\t*\t*\t0\t0\t%s\t*\n", job->read_names[next_read].c_str(), seq.empty() ? "*" : seq.c_str());
        }
    };
    if (best_mode) {
        skip.assign(res->n_pairs, 1);
        tied.assign(res->n_pairs, 0);
        has_winner.assign(n_reads, 0);
        for (uint64_t r = 0; r < n_reads; r++) {
            const uint64_t a = job->cand_offsets[r], e = job->cand_offsets[r + 1];
            uint64_t w = e;
            for (uint64_t k = a; k < e && w == e; k++)
                if (res->pair_status[k] != (uint32_t)SCRG_PAIR_NOT_BEST && res->pair_status[k] != (uint32_t)SCRG_PAIR_OVER_EDIT_LIMIT) w = k;
            if (w == e) continue;
            has_winner[r] = 1;
            skip[w] = 0;
            for (uint64_t k = a; k < e; k++)
                if (res->pair_status[k] == (uint32_t)SCRG_PAIR_NOT_BEST && res->edit_distance[k] == res->edit_distance[w]) tied[w] = 1;
        }
    }
    for (uint64_t k = 0; k <= res->n_pairs; k++) {
        if (k == res->n_pairs) {
            if (best_mode) unmapped_upto(n_reads);
            break;
        }
        if (best_mode && skip[k]) continue;
        if (best_mode) unmapped_upto(job->pair_read[k] + 1);      // (the reads before this winner's that have none)
        const uint64_t r = job->pair_read[k];
        const Chromosome& c = job->chroms[job->cand_chrom[k]];
        const std::string chrom = c.name.substr(0, c.name.find_first_of(" \t"));
        const char* cigar = format == 2 ? "" : res->cigar_text + res->cigar_offset[k];
        const char* const diff_str = diff ? diff->text + diff->offset[k] : "";
        // text bases consumed, matches and alignment columns from the runs
        uint64_t tcons = 0, matches = 0, cols = 0;
        // (a record whose counts cover the pair's runs — scrg_report_score says which — has them already)
        char report_tags[64] = "";
        int64_t score = 0;
        const scrg_pair_report* const rp = report ? report->pairs + k : nullptr;
        const bool counted = rp && scrg_report_score(rp, costs[0], costs[1], costs[2], costs[3], &score) == SCRG_OK;
        if (counted) {
            tcons = (uint64_t)rp->n_match + rp->n_mismatch + rp->n_del;
            matches = rp->n_match;
            cols = tcons + rp->n_ins;
            const uint64_t diverged = (uint64_t)rp->n_mismatch + rp->n_indel, blocks = matches + diverged;
            snprintf(report_tags, sizeof(report_tags), "\tAS:i:%lld\tde:f:%.4f", (long long)score, blocks ? (double)diverged / (double)blocks : 0.0);
        }
        for (uint64_t q = res->run_offset[k]; !counted && !res->text_end && q < res->run_offset[k + 1]; q++) {
            const unsigned n = res->runs[q].count;
            const char op = res->runs[q].op;
            if (op != 'I') tcons += n;
            if (op == '=') matches += n;
            cols += n;
        }
        const uint64_t ts = job->cand_start_in_chrom[k];
        const bool rev = job->cand_reverse[k] != 0;
        // a pair over the handle's edit limit (scrg_ctx_set_edit_limit) has no alignment: PAF leaves it out, SAM has it as
        // placed but unmapped at its candidate (FLAG 4, CIGAR *, no NM)
        // (nor has a pair whose clip record keeps nothing)
        const scrg_pair_clip* const cp = clip ? clip->pairs + k : nullptr;
        const bool over = (res->pair_status && res->pair_status[k] == (uint32_t)SCRG_PAIR_OVER_EDIT_LIMIT) || (cp && cp->n_runs == 0);
        if (over && format != 1) continue;
        if (format == 2) {
            // TSV: read name, read length, strand, chromosome, target start, target end, edit distance
            fprintf(f, "%s\t%llu\t%c\t%s\t%llu\t%llu\t%lld\n", job->read_names[r].c_str(), (unsigned long long)job->read_lens[r],
                    rev ? '-' : '+', chrom.c_str(), (unsigned long long)ts, (unsigned long long)(ts + (res->text_end ? res->text_end[k] : tcons)),
                    (long long)res->edit_distance[k]);
        } else if (format == 1) {
            // SAM uses M/I/D/=/X; '=' and 'X' are valid SAM operators, so the CIGAR is kept verbatim
            const std::string& seq = job->read_seqs[r];
            std::string s = seq;
            if (rev) {
                std::reverse(s.begin(), s.end());
                for (char& ch : s) {
                    switch (ch) {
                    case 'A': ch = 'T'; break; case 'C': ch = 'G'; break; case 'G': ch = 'C'; break; case 'T': ch = 'A'; break;
                    case 'a': ch = 't'; break; case 'c': ch = 'g'; break; case 'g': ch = 'c'; break; case 't': ch = 'a'; break;
                    default: break;
                    }
                }
            }
            if (over)
                fprintf(f, "%s\t%d\t%s\t%llu\t0\t*\t*\t0\t0\t%s\t*\n", job->read_names[r].c_str(), rev ? 4 | 16 : 4,
                        chrom.c_str(), (unsigned long long)(ts + 1), s.empty() ? "*" : s.c_str());
            else if (cp) {
                // <read_start>S, the kept stretch's text, <read_len - read_end>S (none of length 0); POS moved by text_start
                std::string clipped;
                const uint64_t tail = job->read_lens[r] - std::min<uint64_t>(job->read_lens[r], cp->read_end);
                if (cp->read_start) clipped += std::to_string(cp->read_start) + "S";
                clipped += cigar;
                if (tail) clipped += std::to_string(tail) + "S";
                fprintf(f, "%s\t%d\t%s\t%llu\t%d\t%s\t*\t0\t0\t%s\t*\tNM:i:%u\tAS:i:%d\n", job->read_names[r].c_str(), rev ? 16 : 0, chrom.c_str(),
                        (unsigned long long)(ts + cp->text_start + 1), best_mode && tied[k] ? 0 : 255, clipped.c_str(), s.empty() ? "*" : s.c_str(),
                        cp->n_edits, cp->score);
            } else
                fprintf(f, "%s\t%d\t%s\t%llu\t%d\t%s\t*\t0\t0\t%s\t*\tNM:i:%lld%s%s%s\n", job->read_names[r].c_str(), rev ? 16 : 0,
                        chrom.c_str(), (unsigned long long)(ts + 1), mapq_of(k), *cigar ? cigar : "*", s.empty() ? "*" : s.c_str(),
                        (long long)res->edit_distance[k], diff_tag, diff_str, report_tags);
        } else if (cp) {
            // the query interval on the read's forward strand, as PAF wants it: a minus-strand candidate aligned the reverse complement
            const uint64_t len = job->read_lens[r];
            const uint64_t qs = rev ? len - std::min<uint64_t>(len, cp->read_end) : cp->read_start, qe = rev ? len - std::min<uint64_t>(len, cp->read_start) : cp->read_end;
            fprintf(f, "%s\t%llu\t%llu\t%llu\t%c\t%s\t%llu\t%llu\t%llu\t%llu\t%llu\t255\tNM:i:%u\tcg:Z:%s%s\tAS:i:%d\n", job->read_names[r].c_str(),
                    (unsigned long long)len, (unsigned long long)qs, (unsigned long long)qe, rev ? '-' : '+', chrom.c_str(), (unsigned long long)c.len,
                    (unsigned long long)(ts + cp->text_start), (unsigned long long)(ts + cp->text_end), (unsigned long long)matches, (unsigned long long)cols,
                    cp->n_edits, cigar, best_mode ? "\ttp:A:P" : "", cp->score);
        } else {
            fprintf(f, "%s\t%llu\t0\t%llu\t%c\t%s\t%llu\t%llu\t%llu\t%llu\t%llu\t%d\tNM:i:%lld\tcg:Z:%s%s%s%s%s\n",
                    job->read_names[r].c_str(), (unsigned long long)job->read_lens[r],
                    (unsigned long long)job->read_lens[r], rev ? '-' : '+', chrom.c_str(), (unsigned long long)c.len,
                    (unsigned long long)ts, (unsigned long long)(ts + tcons), (unsigned long long)matches,
                    (unsigned long long)cols, summary ? mapq_of(k) : 255, (long long)res->edit_distance[k], cigar, best_mode ? "\ttp:A:P" : "", diff_tag, diff_str,
                    report_tags);
        }
    }
    fclose(f);
    return SCRG_OK;
}

// The difference string of ONE pair on the host, from the rules of include/scrooge_amd.h (DIFFERENCE STRINGS) — written apart
// from the device kernels (diff_kernels.hip), which the tests hold to it.
static scrg_status diff_from_runs_impl(int32_t kind, const char* text, uint64_t text_len, const char* read, uint64_t read_len, const scrg_run* runs,
                                       uint64_t n_runs, char* buf, uint64_t cap, uint64_t* len)
{
    if ((kind != SCRG_DIFF_MD && kind != SCRG_DIFF_CS) || !len || (n_runs && !runs) || (text_len && !text) || (read_len && !read)) return SCRG_ERR_INVALID_ARG;
    const bool md = kind == SCRG_DIFF_MD;
    auto base = [&](char c) { return (char)(md ? (c & ~0x20) : (c | 0x20)); };
    std::string out;
    uint64_t t = 0, q = 0, pend = 0;
    char prev = 0;
    auto number = [&] {
        if (md || pend) {
            if (!md) out += ':';
            out += std::to_string(pend);
        }
        pend = 0;
    };
    for (uint64_t k = 0; k < n_runs; k++) {
        const uint64_t c = runs[k].count;
        const char op = runs[k].op;
        if (c == 0 || (op != '=' && op != 'X' && op != 'I' && op != 'D')) return SCRG_ERR_INVALID_ARG;
        if ((op != 'I' && c > text_len - t) || (op != 'D' && c > read_len - q)) return SCRG_ERR_INVALID_ARG;      // more than the sequences hold
        if (op == '=') {
            pend += c;
        } else if (op == 'X') {
            for (uint64_t j = 0; j < c; j++) {
                number();
                if (md) out += base(text[t + j]);
                else { out += '*'; out += base(text[t + j]); out += base(read[q + j]); }
            }
        } else if (op == 'D') {
            if (prev != 'D') { number(); out += md ? '^' : '-'; }
            for (uint64_t j = 0; j < c; j++) out += base(text[t + j]);
        } else if (!md) {
            if (prev != 'I') { number(); out += '+'; }
            for (uint64_t j = 0; j < c; j++) out += base(read[q + j]);
        }
        if (op != 'I') t += c;
        if (op != 'D') q += c;
        prev = op;
    }
    if (n_runs) number();                    // (a pair without runs: "" in both kinds)
    *len = out.size() + 1;
    if (!buf) return SCRG_OK;
    if (cap < *len) return SCRG_ERR_CIGAR_OVERFLOW;
    memcpy(buf, out.c_str(), out.size() + 1);
    return SCRG_OK;
}

scrg_status scrg_diff_from_runs(int32_t kind, const char* text, uint64_t text_len, const char* read, uint64_t read_len, const scrg_run* runs,
                                uint64_t n_runs, char* buf, uint64_t cap, uint64_t* len)
{
    return guarded([&] { return diff_from_runs_impl(kind, text, text_len, read, read_len, runs, n_runs, buf, cap, len); });
}

// The CIGAR text of ONE pair's runs in a form of include/scrooge_amd.h (CIGAR FORMS) — written apart from the device kernels
// (host_path_kernels.hip), which the tests hold to it: a plain walk with the open stretch.
scrg_status scrg_cigar_from_runs(int32_t form, const scrg_run* runs, uint64_t n_runs, char* buf, uint64_t cap, uint64_t* len)
{
    return guarded([&]() -> scrg_status {
        if (!len || (n_runs && !runs) || (form != SCRG_CIGAR_WINDOWED && form != SCRG_CIGAR_MERGED && form != SCRG_CIGAR_M)) return SCRG_ERR_INVALID_ARG;
        std::string out;
        char cls = 0;
        uint64_t sum = 0;
        auto close = [&] {
            if (cls) out += std::to_string(sum) + cls;
            sum = 0;
        };
        for (uint64_t k = 0; k < n_runs; k++) {
            const char op = runs[k].op;
            if (runs[k].count == 0 || (op != '=' && op != 'X' && op != 'I' && op != 'D')) return SCRG_ERR_INVALID_ARG;
            const char c = (form == SCRG_CIGAR_M && (op == '=' || op == 'X')) ? 'M' : op;
            if (form == SCRG_CIGAR_WINDOWED || c != cls) close();
            cls = c;
            sum += runs[k].count;
        }
        close();
        *len = out.size() + 1;
        if (!buf) return SCRG_OK;
        if (cap < *len) return SCRG_ERR_CIGAR_OVERFLOW;
        memcpy(buf, out.c_str(), out.size() + 1);
        return SCRG_OK;
    });
}

// The clip record of ONE pair on the host, from the rule of include/scrooge_amd.h (SOFT CLIPPING) — written apart from the device
// kernel (clip_kernels.hip), which the tests hold to it: for every end the earliest least start, then the latest best end.
scrg_status scrg_clip_from_runs(const scrg_run* runs, uint64_t n_runs, const int32_t* costs, scrg_pair_clip* out)
{
    static const int32_t usual[4] = {2, 4, 4, 2};
    if (!costs) costs = usual;
    if (!out || (n_runs && !runs) || n_runs > 0xffffffffull || !scrg_host::clip_costs_ok(costs)) return SCRG_ERR_INVALID_ARG;
    memset(out, 0, sizeof(*out));
    uint64_t bases = 0;
    for (uint64_t k = 0; k < n_runs; k++) {
        const char op = runs[k].op;
        if (runs[k].count == 0 || (op != '=' && op != 'X' && op != 'I' && op != 'D')) return SCRG_OK;      // (no run: the pair is not looked at)
        bases += (op == '=' || op == 'X' ? 2u : 1u) * (uint64_t)runs[k].count;
    }
    if (!scrg_host::clip_scores_fit(costs, bases)) return SCRG_ERR_INVALID_ARG;
    struct At { uint32_t t, q, e; };
    At at{0, 0, 0}, low_at{0, 0, 0};
    int64_t P = 0, low = INT64_MAX, best = 0;
    uint32_t low_run = 0;
    for (uint64_t k = 0; k < n_runs; k++) {
        const char op = runs[k].op;
        const int64_t c = runs[k].count;
        if (op == '=' && P < low) {
            low = P;
            low_run = (uint32_t)k;
            low_at = at;
        }
        if (op == '=') P += costs[0] * c;
        else if (op == 'X') P -= costs[1] * c;
        else P -= costs[3] * c + (k > 0 && (runs[k - 1].op == 'I' || runs[k - 1].op == 'D') ? 0 : costs[2]);
        if (op != 'I') at.t += (uint32_t)c;
        if (op != 'D') at.q += (uint32_t)c;
        if (op != '=') at.e += (uint32_t)c;
        if (op == '=' && P - low >= best) {
            best = P - low;
            out->read_start = low_at.q;
            out->read_end = at.q;
            out->text_start = low_at.t;
            out->text_end = at.t;
            out->first_run = low_run;
            out->n_runs = (uint32_t)k - low_run + 1u;
            out->score = (int32_t)best;
            out->n_edits = at.e - low_at.e;
        }
    }
    return SCRG_OK;
}

// ONE alignment added to a pileup on the host, from the rule of include/scrooge_amd.h (PILEUP) — written apart from the device
// kernel (pileup_kernels.hip), which the tests hold to it: counts form, one column at a time; what is a stretch, an insertion event
// and outside the target comes from pileup_rule.h, which the kernel shares.
scrg_status scrg_pileup_from_runs(const scrg_run* runs, uint64_t n_runs, const char* read_aligned, uint64_t read_len, uint64_t target_start,
                                  uint64_t target_len, uint32_t* counts, uint64_t* out_of_range)
{
    if (!counts || (n_runs && !runs) || (read_len && !read_aligned) || target_len == UINT64_MAX) return SCRG_ERR_INVALID_ARG;
    auto code = [](char c) { return c == 'A' || c == 'a' ? 0 : c == 'C' || c == 'c' ? 1 : c == 'G' || c == 'g' ? 2 : c == 'T' || c == 't' ? 3 : -1; };
    // validate first: nothing is added of a list that is refused
    uint64_t q = 0;
    for (uint64_t k = 0; k < n_runs; k++) {
        const uint64_t c = runs[k].count;
        const char op = runs[k].op;
        if (c == 0 || (op != '=' && op != 'X' && op != 'I' && op != 'D')) return SCRG_ERR_INVALID_ARG;
        if (op == 'D') continue;
        if (c > read_len - q) return SCRG_ERR_INVALID_ARG;
        for (uint64_t j = 0; op == 'X' && j < c; j++)
            if (code(read_aligned[q + j]) < 0) return SCRG_ERR_INVALID_ARG;
        q += c;
    }
    const uint64_t stride = target_len + 1;
    uint64_t t = 0;
    uint32_t prev = 0;
    bool outside = false;
    q = 0;
    for (uint64_t k = 0; k < n_runs; k++) {
        const uint32_t c = runs[k].count, op = (uint8_t)runs[k].op;
        const uint64_t g = scrg::pile_pos(target_start, t);
        if (op == 'I') {
            if (scrg::pile_ins_event(op, prev)) {
                if (scrg::pile_ins_outside(g, target_len)) outside = true;
                else counts[scrg::PILE_INS * stride + g]++;
            }
        } else {
            outside |= scrg::pile_columns_outside(g, c, target_len);
            for (uint64_t j = 0; j < c && g < target_len && j < target_len - g; j++) {
                const uint32_t plane = scrg::pile_stretch_op(op) ? scrg::pile_stretch_plane(op) : scrg::PILE_BASE + (uint32_t)code(read_aligned[q + j]);
                counts[plane * stride + g + j]++;
            }
        }
        if (op != 'I') t += c;
        if (op != 'D') q += c;
        prev = op;
    }
    if (out_of_range && outside) ++*out_of_range;
    return SCRG_OK;
}

// The pileup as a table: one row per position that at least max(min_depth, 1) alignments cover.
scrg_status scrg_job_write_pileup(const scrg_job* job, const scrg_pileup* pileup, const char* path, uint64_t min_depth)
{
    return guarded([&] {
        if (!job || !pileup || !path || !pileup->counts || pileup->target_len != job->genome.size()) return (scrg_status)SCRG_ERR_INVALID_ARG;
        FILE* f = fopen(path, "w");
        if (!f) return (scrg_status)SCRG_ERR_IO;
        fprintf(f, "chrom\tpos\tref\tdepth\tmatch\tA\tC\tG\tT\tdel\tins\n");
        const uint64_t stride = pileup->target_len + 1, need = std::max<uint64_t>(min_depth, 1);
        const uint32_t* const n = pileup->counts;
        auto rows = [&](const char* chrom, uint64_t first, uint64_t len) {
            for (uint64_t i = first; i < first + len && i < pileup->target_len; i++) {
                uint64_t depth = 0;
                for (uint32_t pl = scrg::PILE_MATCH; pl <= scrg::PILE_DEL; pl++) depth += n[pl * stride + i];
                if (depth < need) continue;
                const char ref = job->genome[i];
                fprintf(f, "%s\t%llu\t%c\t%llu\t%u\t%u\t%u\t%u\t%u\t%u\t%u\n", chrom, (unsigned long long)(i - first + 1),
                        (char)(ref >= 'a' && ref <= 'z' ? ref - 32 : ref), (unsigned long long)depth, n[i], n[stride + i], n[2 * stride + i], n[3 * stride + i],
                        n[4 * stride + i], n[scrg::PILE_DEL * stride + i], n[scrg::PILE_INS * stride + i]);
            }
        };
        // (chromosome and position as scrg_job_write has them for a candidate's start: the name up to the first blank, 1-based)
        if (job->chroms.empty()) rows("*", 0, pileup->target_len);
        for (const Chromosome& c : job->chroms) rows(c.name.substr(0, c.name.find_first_of(" \t")).c_str(), c.start, c.len);
        return fclose(f) == 0 ? (scrg_status)SCRG_OK : (scrg_status)SCRG_ERR_IO;
    });
}

// The sites of a pileup on the host: site_rule.h, the text the device passes compile, applied position by position in order.
scrg_status scrg_pileup_sites_from_counts(const uint32_t* counts, uint64_t target_len, const char* genome_ascii, const scrg_site_rule* rule, scrg_site* out,
                                          uint64_t cap, uint64_t* n_sites)
{
    if (!rule || !scrg::site_rule_valid(rule->min_depth, rule->min_alt_per_mille, rule->reserved) || target_len >= 0xffffffffull) return SCRG_ERR_INVALID_ARG;
    if (target_len && (!counts || !genome_ascii)) return SCRG_ERR_INVALID_ARG;
    auto code = [](char c) { return c == 'A' || c == 'a' ? 0 : c == 'C' || c == 'c' ? 1 : c == 'G' || c == 'g' ? 2 : c == 'T' || c == 't' ? 3 : -1; };
    const scrg::SiteRule k{rule->min_depth, rule->min_alt, rule->min_alt_per_mille};
    const uint64_t stride = target_len + 1;
    // two passes: the first validates and counts, so that nothing is written of a call that is refused
    for (int pass = 0; pass < 2; pass++) {
        uint64_t n = 0;
        for (uint64_t g = 0; g < target_len; g++) {
            const int r = code(genome_ascii[g]);
            if (r < 0) return SCRG_ERR_BAD_BASE;
            uint32_t c[scrg::PILE_PLANES];
            for (uint32_t pl = 0; pl < scrg::PILE_PLANES; pl++) c[pl] = counts[pl * stride + g];
            const scrg::SiteVerdict v = scrg::site_verdict(k, c, (uint32_t)r);
            if (!v.site) continue;
            if (pass == 1) {
                scrg_site& s = out[n];
                s.pos = g;
                memcpy(s.counts, c, sizeof(c));
                s.ref = (uint8_t)r;
                s.alt = v.alt;
                s.call = v.call;
                s.flags = v.flags;
            }
            n++;
        }
        if (n_sites) *n_sites = n;
        if (!out) return SCRG_OK;
        if (cap < n) return SCRG_ERR_CIGAR_OVERFLOW;
    }
    return SCRG_OK;
}

// One mate pair's choice on the host: mate_rule.h, the text the device pass compiles, applied combination by combination in order.
scrg_status scrg_mates_from_distances(const scrg_mate_rule* rule, uint64_t n_a, const uint64_t* start_a, const uint8_t* rev_a, const int64_t* ed_a,
                                      const uint32_t* status_a, uint64_t len_a, uint64_t n_b, const uint64_t* start_b, const uint8_t* rev_b,
                                      const int64_t* ed_b, const uint32_t* status_b, uint64_t len_b, scrg_mate_record* record, uint8_t* is_best_a,
                                      uint8_t* is_best_b)
{
    static const scrg_mate_rule any_fr = {0, ~0ull, SCRG_MATES_FR, 0, {0, 0}};
    if (!rule) rule = &any_fr;
    if (!scrg::mate_rule_valid(rule->min_span, rule->max_span, rule->orientation, rule->reserved[0], rule->reserved[1])) return SCRG_ERR_INVALID_ARG;
    if (!record || (n_a && (!start_a || !ed_a)) || (n_b && (!start_b || !ed_b))) return SCRG_ERR_INVALID_ARG;
    if (n_a && n_b && n_a > 0xffffffffull / n_b) return SCRG_ERR_INVALID_ARG;
    const scrg::MateRule k{rule->min_span, rule->max_span, rule->orientation, rule->unpaired_penalty};
    auto eligible = [](const uint32_t* status, uint64_t p) { return !status || status[p] != (uint32_t)SCRG_PAIR_OVER_EDIT_LIMIT; };
    scrg::MateMin2 x = scrg::mate_min2_none(), a = scrg::mate_min2_none(), b = scrg::mate_min2_none();
    for (uint64_t i = 0; i < n_a; i++) {
        if (!eligible(status_a, i)) continue;
        scrg::mate_min2_push(a, scrg::mate_value(scrg::mate_ed(ed_a[i]), (uint32_t)i));
        for (uint64_t j = 0; j < n_b; j++)
            if (eligible(status_b, j) && scrg::mate_proper(k, start_a[i], rev_a && rev_a[i] ? 1u : 0u, len_a, start_b[j], rev_b && rev_b[j] ? 1u : 0u, len_b))
                scrg::mate_min2_push(x, scrg::mate_value((uint64_t)scrg::mate_ed(ed_a[i]) + scrg::mate_ed(ed_b[j]), (uint32_t)(i * n_b + j)));
    }
    for (uint64_t j = 0; j < n_b; j++)
        if (eligible(status_b, j)) scrg::mate_min2_push(b, scrg::mate_value(scrg::mate_ed(ed_b[j]), (uint32_t)j));
    const scrg::MateVerdict v = scrg::mate_decide(k, x, a, b, (uint32_t)n_b);
    record->winner[0] = v.i;
    record->winner[1] = v.j;
    record->cost = v.cost;
    record->second_cost = v.second_cost;
    record->span = v.i != scrg::MATE_NONE && v.j != scrg::MATE_NONE ? scrg::mate_span32(scrg::mate_span(start_a[v.i], len_a, start_b[v.j], len_b)) : 0u;
    record->n_proper = v.n_proper;
    record->flags = v.flags;
    record->reserved = 0;
    for (uint64_t i = 0; is_best_a && i < n_a; i++) is_best_a[i] = i == v.i ? 1 : 0;
    for (uint64_t j = 0; is_best_b && j < n_b; j++) is_best_b[j] = j == v.j ? 1 : 0;
    return SCRG_OK;
}

// The read summaries on the host: mapq_rule.h, the text the device pass compiles, applied read by read and candidate by candidate in order.
scrg_status scrg_read_summary_from_distances(const scrg_mapq_rule* rule, uint64_t n_reads, const uint64_t* first, const uint32_t* read_len,
                                             const int64_t* edit_distance, const uint32_t* pair_status, scrg_read_record* out, uint32_t* keep_status)
{
    static const scrg_mapq_rule defaults = {10, 60, 250, 0, 0};
    if (!rule) rule = &defaults;
    if (!scrg::mapq_rule_valid(rule->per_edit, rule->max_q, rule->zero_per_mille, rule->min_keep_q, rule->reserved)) return SCRG_ERR_INVALID_ARG;
    if (n_reads == 0) return SCRG_OK;
    if (!first || !out || (keep_status && !pair_status)) return SCRG_ERR_INVALID_ARG;
    for (uint64_t r = 0; r < n_reads; r++)
        if (first[r] > first[r + 1]) return SCRG_ERR_INVALID_ARG;
    if (first[n_reads] > 0xffffffffull || (first[n_reads] > first[0] && (!read_len || !edit_distance))) return SCRG_ERR_INVALID_ARG;
    const scrg::MapqRule k{rule->per_edit, rule->max_q, rule->zero_per_mille, rule->min_keep_q};
    static_assert(sizeof(scrg_read_record) == sizeof(scrg::MapqWords), "a record is eight dwords");
    for (uint64_t r = 0; r < n_reads; r++) {
        const uint64_t a = first[r], e = first[r + 1];
        scrg::MapqPart part = scrg::mapq_part_none();
        for (uint64_t p = a; p < e; p++)
            if (!pair_status || pair_status[p] != (uint32_t)SCRG_PAIR_OVER_EDIT_LIMIT)
                part = scrg::mapq_merge(part, scrg::mapq_part_one(scrg::mapq_ed(edit_distance[p]), (uint32_t)p));
        const scrg::MapqWords rec = scrg::mapq_record(k, part, e > a ? read_len[a] : 0u, (uint32_t)(e - a));
        memcpy(&out[r], rec.w, sizeof(rec.w));
        for (uint64_t p = a; keep_status && p < e; p++)
            keep_status[p] = scrg::mapq_keep_status(pair_status[p], scrg::mapq_words_kept(rec) && (uint32_t)p == rec.w[0], (uint32_t)SCRG_PAIR_NOT_BEST);
    }
    return SCRG_OK;
}

scrg_status scrg_read_summary_merge(const uint64_t* a, const uint64_t* b, uint64_t* out)
{
    if (!a || !b || !out) return SCRG_ERR_INVALID_ARG;
    const scrg::MapqPart r = scrg::mapq_merge(scrg::MapqPart{a[0], (uint32_t)a[1], (uint32_t)a[2], (uint32_t)a[3]},
                                              scrg::MapqPart{b[0], (uint32_t)b[1], (uint32_t)b[2], (uint32_t)b[3]});
    out[0] = r.best;
    out[1] = r.n_tied;
    out[2] = r.second_ed;
    out[3] = r.n_eligible;
    return SCRG_OK;
}

// The sites as a table: the columns of scrg_job_write_pileup, then alt, call and flags.
scrg_status scrg_job_write_sites(const scrg_job* job, const scrg_pileup_sites* sites, const char* path)
{
    return guarded([&] {
        if (!job || !sites || !path || (sites->n_sites && !sites->sites) || sites->target_len != job->genome.size()) return (scrg_status)SCRG_ERR_INVALID_ARG;
        const scrg_site* const first = sites->sites;
        const scrg_site* const last = first + sites->n_sites;
        for (const scrg_site* s = first; s != last; s++)
            if (s->pos >= sites->target_len) return (scrg_status)SCRG_ERR_INVALID_ARG;
        FILE* f = fopen(path, "w");
        if (!f) return (scrg_status)SCRG_ERR_IO;
        fprintf(f, "chrom\tpos\tref\tdepth\tmatch\tA\tC\tG\tT\tdel\tins\talt\tcall\tflags\n");
        auto allele = [](uint8_t a) { return a < 4 ? "ACGT"[a] : a == SCRG_SITE_DEL ? '*' : '.'; };
        auto rows = [&](const char* chrom, uint64_t start, uint64_t len) {
            const scrg_site* s = std::lower_bound(first, last, start, [](const scrg_site& x, uint64_t p) { return x.pos < p; });
            for (; s != last && s->pos - start < len; s++) {
                const uint32_t* const n = s->counts;
                const uint64_t depth = (uint64_t)n[0] + n[1] + n[2] + n[3] + n[4] + n[5];
                const char ref = job->genome[s->pos];
                fprintf(f, "%s\t%llu\t%c\t%llu\t%u\t%u\t%u\t%u\t%u\t%u\t%u\t%c\t%c\t%u\n", chrom, (unsigned long long)(s->pos - start + 1),
                        (char)(ref >= 'a' && ref <= 'z' ? ref - 32 : ref), (unsigned long long)depth, n[0], n[1], n[2], n[3], n[4], n[5], n[6], allele(s->alt),
                        allele(s->call), (unsigned)s->flags);
            }
        };
        // (chromosome and position as scrg_job_write_pileup has them)
        if (job->chroms.empty()) rows("*", 0, sites->target_len);
        for (const Chromosome& c : job->chroms) rows(c.name.substr(0, c.name.find_first_of(" \t")).c_str(), c.start, c.len);
        return fclose(f) == 0 ? (scrg_status)SCRG_OK : (scrg_status)SCRG_ERR_IO;
    });
}

// The alignment report of ONE pair on the host, from the rules of include/scrooge_amd.h (ALIGNMENT REPORT) — written apart from the
// device kernel (report_kernels.hip), which the tests hold to it: a plain walk, one base at a time.
scrg_status scrg_report_from_runs(const char* text, uint64_t text_len, const char* read, uint64_t read_len, const scrg_run* runs, uint64_t n_runs,
                                  int64_t edit_distance, scrg_pair_report* out)
{
    if (!out || (n_runs && !runs) || (text_len && !text) || (read_len && !read) || n_runs > 0xffffffffull) return SCRG_ERR_INVALID_ARG;
    auto up = [](char c) { return (char)((c >= 'a' && c <= 'z') ? c - 32 : c); };
    auto failed = [&](uint32_t verdict, uint64_t run) {
        memset(out, 0, sizeof(*out));
        out->verdict = verdict;
        out->bad_run = (uint32_t)run;
        return (scrg_status)SCRG_OK;
    };
    scrg_pair_report r;
    memset(&r, 0, sizeof(r));
    uint64_t t = 0, q = 0;
    char prev = 0;
    for (uint64_t k = 0; k < n_runs; k++) {
        const uint64_t c = runs[k].count;
        const char op = runs[k].op;
        if (c == 0) return failed(2, k);
        if (op == '=' || op == 'X') {
            if (q + c > read_len) return failed(3, k);
            if (t + c > text_len) return failed(4, k);
            for (uint64_t j = 0; j < c; j++)
                if ((up(text[t + j]) == up(read[q + j])) != (op == '=')) return failed(5, k);
            (op == '=' ? r.n_match : r.n_mismatch) += (uint32_t)c;
            t += c;
            q += c;
        } else if (op == 'I') {
            if (q + c > read_len) return failed(3, k);
            r.n_ins += (uint32_t)c;
            q += c;
        } else if (op == 'D') {
            if (t + c > text_len) return failed(4, k);
            r.n_del += (uint32_t)c;
            t += c;
        } else {
            return failed(1, k);
        }
        if (op == 'I' || op == 'D') {
            if (prev != 'I' && prev != 'D') r.n_gap_open++;
            if (prev != op) r.n_indel++;
        }
        prev = op;
    }
    if (q != read_len) r.verdict = 3;
    else if ((int64_t)((uint64_t)r.n_mismatch + r.n_ins + r.n_del) != edit_distance) r.verdict = 6;
    if (r.verdict) r.bad_run = (uint32_t)n_runs;
    *out = r;
    return SCRG_OK;
}

scrg_status scrg_report_score(const scrg_pair_report* rep, int64_t match_bonus, int64_t mismatch_cost, int64_t gap_open_cost, int64_t gap_extend_cost,
                              int64_t* score)
{
    if (!rep || !score) return SCRG_ERR_INVALID_ARG;
    // the counts cover the pair's runs for verdict 0, 6 and the 3 met AFTER the last run: that one has bases counted for each of its
    // bad_run runs, where a 3 met AT a run has none (bad_run 0 with no counts: no runs at all, which scores 0 either way)
    if (rep->verdict != 0 && rep->verdict != 6 && rep->verdict != 3) return SCRG_ERR_INVALID_ARG;
    if (rep->verdict == 3 && rep->bad_run != 0 && !(rep->n_match | rep->n_mismatch | rep->n_ins | rep->n_del)) return SCRG_ERR_INVALID_ARG;
    *score = match_bonus * (int64_t)rep->n_match - mismatch_cost * (int64_t)rep->n_mismatch - gap_open_cost * (int64_t)rep->n_gap_open -
             gap_extend_cost * ((int64_t)rep->n_ins + (int64_t)rep->n_del);
    return SCRG_OK;
}

scrg_status scrg_affine_score(const char* cigar, int64_t match_bonus, int64_t mismatch_cost, int64_t gap_open_cost,
                              int64_t gap_extend_cost, int64_t* score)
{
    if (!cigar || !score) return SCRG_ERR_INVALID_ARG;
    int64_t s = 0;
    bool in_gap = false;
    const char* p = cigar;
    while (*p) {
        if (*p < '0' || *p > '9') return SCRG_ERR_FORMAT;
        int64_t n = 0;
        while (*p >= '0' && *p <= '9') n = n * 10 + (*p++ - '0');
        const char op = *p++;
        if (op == '=') {
            s += n * match_bonus;
            in_gap = false;
        } else if (op == 'X') {
            s -= n * mismatch_cost;
            in_gap = false;
        } else if (op == 'I' || op == 'D') {
            if (!in_gap) s -= gap_open_cost;
            s -= n * gap_extend_cost;
            in_gap = true;
        } else {
            return SCRG_ERR_FORMAT;
        }
    }
    *score = s;
    return SCRG_OK;
}

scrg_status scrg_validate_alignment(const char* text, uint64_t text_len, const char* read, uint64_t read_len,
                                    const char* cigar, int64_t edit_distance, int32_t* why)
{
    if (!cigar || (text_len && !text) || (read_len && !read)) return SCRG_ERR_INVALID_ARG;
    auto bad = [&](int32_t code) {
        if (why) *why = code;
        return (scrg_status)SCRG_ERR_FORMAT;
    };
    auto up = [](char c) { return (char)((c >= 'a' && c <= 'z') ? c - 32 : c); };
    uint64_t i = 0, j = 0;
    int64_t edits = 0;
    const char* p = cigar;
    while (*p) {
        if (*p < '0' || *p > '9') return bad(1);
        uint64_t n = 0;
        while (*p >= '0' && *p <= '9') n = n * 10 + (uint64_t)(*p++ - '0');
        const char op = *p++;
        if (n == 0) return bad(2);
        if (op == '=' || op == 'X') {
            if (j + n > read_len) return bad(3);
            if (i + n > text_len) return bad(4);
            for (uint64_t k = 0; k < n; k++)
                if ((up(text[i + k]) == up(read[j + k])) != (op == '=')) return bad(5);
            i += n;
            j += n;
        } else if (op == 'I') {
            if (j + n > read_len) return bad(3);
            j += n;
        } else if (op == 'D') {
            if (i + n > text_len) return bad(4);
            i += n;
        } else {
            return bad(1);
        }
        if (op != '=') edits += (int64_t)n;
    }
    if (j != read_len) return bad(3);
    if (edits != edit_distance) return bad(6);
    if (why) *why = 0;
    return SCRG_OK;
}

}  // extern "C"
