// The C++ shim's directed and anchored calls (include/scrooge_amd.hpp: Handle::align_directed, Handle::align_anchored) on a case
// that tests/test_cpp_shim.py writes and whose expected lines it derives from the CPU oracle.
//
// Case file (whitespace separated): the genome; the number of reads; per read: its bases ("-" = an empty read), the number
// of its locations, and per location: start_in_reference, strand (0/1), leftward (0/1), anchor_read.
// Output, one line per location in nested order:
//   directed cigar=<CIGAR> edit_distance=<d>                       (start, strand, leftward)
//   anchored cigar=<CIGAR> edit_distance=<d> text_start=<t>        (start = the anchor's genome position, strand, anchor_read)
// and one line per wrong-size check.  Exit status 2 with the reason on stderr if anything throws.
#include <fstream>
#include <iostream>
#include <stdexcept>

#include "scrooge_amd.hpp"

int main(int argc, char** argv)
{
    scrooge_amd::enabled_algorithm_log = false;
    if (argc != 2) {
        std::cerr << "usage: shim_anchored CASE_FILE\n";
        return 1;
    }
    try {
        std::ifstream in(argv[1]);
        Genome_t genome;
        size_t n_reads = 0;
        if (!(in >> genome.content >> n_reads)) throw std::runtime_error("case file: no genome / read count");
        std::vector<Read_t> reads(n_reads);
        std::vector<uint8_t> leftward;
        std::vector<uint64_t> anchor_read;
        for (Read_t& r : reads) {
            size_t n_loc = 0;
            if (!(in >> r.content >> n_loc)) throw std::runtime_error("case file: read");
            if (r.content == "-") r.content.clear();
            for (size_t k = 0; k < n_loc; k++) {
                CandidateLocation_t loc{};
                int strand = 0, left = 0;
                uint64_t ra = 0;
                if (!(in >> loc.start_in_reference >> strand >> left >> ra)) throw std::runtime_error("case file: location");
                loc.strand = strand != 0;
                r.locations.push_back(loc);
                leftward.push_back(left ? 1 : 0);
                anchor_read.push_back(ra);
            }
        }

        // the genome is staged and packed once, every call below aligns against the resident copy
        scrooge_amd::Handle& h = scrooge_amd::default_handle();
        h.set_genome(genome);
        for (const Alignment_t& a : h.align_directed(reads, leftward))
            std::cout << "directed cigar=" << a.cigar << " edit_distance=" << a.edit_distance << "\n";
        std::vector<uint64_t> text_start;
        const std::vector<Alignment_t> joined = h.align_anchored(reads, anchor_read, &text_start);
        if (text_start.size() != joined.size()) throw std::runtime_error("text_start: not one entry per location");
        for (size_t k = 0; k < joined.size(); k++)
            std::cout << "anchored cigar=" << joined[k].cigar << " edit_distance=" << joined[k].edit_distance << " text_start=" << text_start[k] << "\n";

        // a per-location vector of the wrong size is refused before anything is aligned
        std::vector<uint8_t> wrong_left(leftward.size() + 1, 0);
        bool refused = false;
        try {
            h.align_directed(reads, wrong_left);
        } catch (const std::invalid_argument&) {
            refused = true;
        }
        std::cout << "directed_wrong_size invalid_argument=" << refused << "\n";
        std::vector<uint64_t> wrong_anchor(anchor_read.begin(), anchor_read.end() - (anchor_read.empty() ? 0 : 1));
        if (anchor_read.empty()) wrong_anchor.push_back(0);
        refused = false;
        try {
            h.align_anchored(reads, wrong_anchor);
        } catch (const std::invalid_argument&) {
            refused = true;
        }
        std::cout << "anchored_wrong_size invalid_argument=" << refused << "\n";
        h.clear_genome();
    } catch (const std::exception& e) {
        std::cerr << "error: " << e.what() << "\n";
        return 2;
    }
    return 0;
}
