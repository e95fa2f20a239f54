"""ctypes binding of include/scrooge_amd_io.h: the reference's read-mapping front door
(FASTA + FASTQ + MAF/PAF, src/util.cpp:45-336), affine re-scoring
(src/cpu_baseline.cpp:694-725) and the CIGAR validator (src/tests.cu:27-169)."""
import ctypes as C

from . import api

SCRG_ERR_IO = 16
SCRG_ERR_FORMAT = 17


class JobOptions(C.Structure):
    _fields_ = [("reverse_strand", C.c_int32), ("sort_by_length", C.c_int32), ("inflation", C.c_int32),
                ("left_extend", C.c_int32), ("read_length_cap", C.c_int64)]


_bound = False


def _lib():
    global _bound
    lib = api.load_library()
    if _bound:
        return lib
    vp, u64p = C.c_void_p, C.POINTER(C.c_uint64)
    sig = {
        "scrg_job_options_default": (None, [C.POINTER(JobOptions)]),
        "scrg_job_load": (C.c_int32, [C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(JobOptions), C.POINTER(vp),
                                      C.c_char_p, C.c_size_t]),
        "scrg_job_free": (None, [vp]),
        "scrg_job_counts": (None, [vp, u64p, u64p, u64p, u64p]),
        "scrg_job_arrays": (None, [vp, C.POINTER(C.c_char_p), C.POINTER(C.POINTER(C.c_char_p)), C.POINTER(u64p),
                                   C.POINTER(u64p), C.POINTER(u64p), C.POINTER(C.POINTER(C.c_uint8))]),
        "scrg_job_read_name": (C.c_char_p, [vp, C.c_uint64]),
        "scrg_job_pair_chromosome": (C.c_char_p, [vp, C.c_uint64, u64p, u64p]),
        "scrg_align_mapping_stranded": (C.c_int32, [vp, C.POINTER(api.Params), C.c_char_p, C.c_uint64, C.c_uint64,
                                                    C.POINTER(C.c_char_p), u64p, u64p, u64p,
                                                    C.POINTER(C.c_uint8), C.POINTER(C.POINTER(api.Result))]),
        "scrg_job_align": (C.c_int32, [vp, C.POINTER(api.Params), vp, C.POINTER(C.POINTER(api.Result))]),
        "scrg_job_write": (C.c_int32, [vp, C.POINTER(api.Result), C.c_char_p, C.c_int]),
        "scrg_job_write_diff": (C.c_int32, [vp, C.POINTER(api.Result), C.POINTER(api.Diff), C.c_char_p, C.c_int]),
        "scrg_diff_from_runs": api._LAZY_SIGS["scrg_diff_from_runs"],
        "scrg_cigar_from_runs": api._LAZY_SIGS["scrg_cigar_from_runs"],
        "scrg_job_write_report": (C.c_int32, [vp, C.POINTER(api.Result), C.POINTER(api.Diff), C.POINTER(api.Report), C.POINTER(C.c_int64), C.c_char_p,
                                              C.c_int]),
        "scrg_report_from_runs": api._LAZY_SIGS["scrg_report_from_runs"],
        "scrg_report_score": api._LAZY_SIGS["scrg_report_score"],
        "scrg_job_write_clipped": (C.c_int32, [vp, C.POINTER(api.Result), C.POINTER(api.Clip), C.c_char_p, C.c_int]),
        "scrg_clip_from_runs": api._LAZY_SIGS["scrg_clip_from_runs"],
        "scrg_pileup_from_runs": api._LAZY_SIGS["scrg_pileup_from_runs"],
        "scrg_job_write_pileup": (C.c_int32, [vp, C.POINTER(api.Pileup), C.c_char_p, C.c_uint64]),
        "scrg_pileup_sites_from_counts": api._LAZY_SIGS["scrg_pileup_sites_from_counts"],
        "scrg_job_write_sites": (C.c_int32, [vp, C.POINTER(api.PileupSites), C.c_char_p]),
        "scrg_mates_from_distances": api._LAZY_SIGS["scrg_mates_from_distances"],
        "scrg_job_align_paired": (C.c_int32, [vp, C.POINTER(api.Params), vp, vp, C.POINTER(C.POINTER(api.Mates)), C.POINTER(C.POINTER(api.Result))]),
        "scrg_job_write_paired": (C.c_int32, [vp, C.POINTER(api.Result), C.POINTER(api.Mates), C.c_char_p, C.c_int]),
        "scrg_read_summary_from_distances": api._LAZY_SIGS["scrg_read_summary_from_distances"],
        "scrg_read_summary_merge": api._LAZY_SIGS["scrg_read_summary_merge"],
        "scrg_job_write_mapq": (C.c_int32, [vp, C.POINTER(api.Result), C.POINTER(api.Diff), C.POINTER(api.Report), C.POINTER(C.c_int64),
                                            C.POINTER(api.ReadSummaries), C.c_char_p, C.c_int]),
        "scrg_candidates_from_genome": api._LAZY_SIGS["scrg_candidates_from_genome"],
        "scrg_job_load_unseeded": (C.c_int32, [C.c_char_p, C.c_char_p, C.POINTER(JobOptions), C.POINTER(vp), C.c_char_p, C.c_size_t]),
        "scrg_job_seed": (C.c_int32, [vp, vp, vp]),
        "scrg_affine_score": (C.c_int32, [C.c_char_p, C.c_int64, C.c_int64, C.c_int64, C.c_int64,
                                          C.POINTER(C.c_int64)]),
        "scrg_validate_alignment": (C.c_int32, [C.c_char_p, C.c_uint64, C.c_char_p, C.c_uint64, C.c_char_p,
                                                C.c_int64, C.POINTER(C.c_int32)]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _bound = True
    return lib


IO_SYMBOLS = ["scrg_job_options_default", "scrg_job_load", "scrg_job_free", "scrg_job_counts", "scrg_job_arrays",
              "scrg_job_read_name", "scrg_job_pair_chromosome", "scrg_align_mapping_stranded", "scrg_job_align",
              "scrg_job_write", "scrg_affine_score", "scrg_validate_alignment", "scrg_job_write_diff", "scrg_diff_from_runs",
              "scrg_job_write_report", "scrg_report_from_runs", "scrg_report_score", "scrg_cigar_from_runs",
              "scrg_job_write_clipped", "scrg_clip_from_runs", "scrg_pileup_from_runs", "scrg_job_write_pileup",
              "scrg_pileup_sites_from_counts", "scrg_job_write_sites", "scrg_mates_from_distances",
              "scrg_job_align_paired", "scrg_job_write_paired", "scrg_read_summary_from_distances", "scrg_read_summary_merge",
              "scrg_job_write_mapq", "scrg_candidates_from_genome", "scrg_job_load_unseeded", "scrg_job_seed",
              "scrg_candidates_from_genome_sampled"]

cigar_from_runs = api.cigar_from_runs            # scrg_cigar_from_runs: the CIGAR text of one pair's runs in a form, on the host

report_from_runs = api.report_from_runs          # scrg_report_from_runs: the alignment report of one pair on the host
report_score = api.report_score                  # scrg_report_score
clip_from_runs = api.clip_from_runs              # scrg_clip_from_runs: the best-scoring stretch of one pair's runs on the host
pileup_from_runs = api.pileup_from_runs          # scrg_pileup_from_runs: one alignment added to a pileup on the host
pileup_sites_from_counts = api.pileup_sites_from_counts      # scrg_pileup_sites_from_counts: the sites of a pileup on the host
mates_from_distances = api.mates_from_distances  # scrg_mates_from_distances: one mate pair's choice on the host
read_summary_from_distances = api.read_summary_from_distances    # scrg_read_summary_from_distances: the reads' summaries and MAPQs on the host
candidates_from_genome = api.candidates_from_genome  # scrg_candidates_from_genome: the reads' candidates on the host (seeding)


def affine_score(cigar, match=2, mismatch=4, gap_open=4, gap_extend=2):
    """Defaults are the costs of the reference's accuracy study (scripts/profile.py, 2,4,4,2)."""
    out = C.c_int64(0)
    st = _lib().scrg_affine_score(cigar.encode(), match, mismatch, gap_open, gap_extend, C.byref(out))
    if st != 0:
        raise api.ScroogeError(st, "malformed CIGAR")
    return int(out.value)


def validate_alignment(text, read, cigar, edit_distance):
    """0 if consistent, else the reason code of scrg_validate_alignment."""
    text = text.encode() if isinstance(text, str) else bytes(text)
    read = read.encode() if isinstance(read, str) else bytes(read)
    why = C.c_int32(0)
    st = _lib().scrg_validate_alignment(text, len(text), read, len(read), cigar.encode(), int(edit_distance),
                                        C.byref(why))
    return 0 if st == 0 else int(why.value)


class Job:
    """A read-mapping job loaded from genome FASTA + reads FASTQ + seeds (.maf/.paf); seeds=None: a job with no pairs
    (scrg_job_load_unseeded) until seed() finds them on the GPU."""

    def __init__(self, genome_fasta, reads_fastq, seeds=None, **options):
        self.lib = _lib()
        o = JobOptions()
        self.lib.scrg_job_options_default(C.byref(o))
        for k, v in options.items():
            if not hasattr(o, k):
                raise TypeError("unknown option %r" % k)
            setattr(o, k, int(v))
        h = C.c_void_p()
        err = C.create_string_buffer(512)
        if seeds is None:
            st = self.lib.scrg_job_load_unseeded(str(genome_fasta).encode(), str(reads_fastq).encode(), C.byref(o), C.byref(h), err, len(err))
        else:
            st = self.lib.scrg_job_load(str(genome_fasta).encode(), str(reads_fastq).encode(), str(seeds).encode(),
                                        C.byref(o), C.byref(h), err, len(err))
        if st != 0:
            raise api.ScroogeError(st, err.value.decode())
        self.h = h
        self._counts()

    def _counts(self):
        a, b, c, d = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint64()
        self.lib.scrg_job_counts(self.h, C.byref(a), C.byref(b), C.byref(c), C.byref(d))
        self.n_reads, self.n_pairs, self.genome_len, self.n_chromosomes = a.value, b.value, c.value, d.value

    def seed(self, aligner, rule=None):
        """scrg_job_seed: the job's genome made resident on `aligner`'s GPU and indexed, the reads' candidates found there by `rule`
        (an api.SeedRule; None: the defaults) and installed as the job's pairs — align(), align_paired() and the writers then work
        as for a job loaded with a seeds file.  -> the number of pairs."""
        aligner._check(self.lib.scrg_job_seed(aligner.h, api._seed_rule(rule), self.h))
        self._counts()
        return self.n_pairs

    def close(self):
        if getattr(self, "h", None):
            self.lib.scrg_job_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def genome(self):
        """-> the genome's bases (bytes, all chromosomes end to end: what a pileup's positions index)"""
        return C.string_at(self._arrays()[0], self.genome_len)

    def _arrays(self):
        g = C.c_char_p()
        reads = C.POINTER(C.c_char_p)()
        lens, offs, starts = (C.POINTER(C.c_uint64)() for _ in range(3))
        rev = C.POINTER(C.c_uint8)()
        self.lib.scrg_job_arrays(self.h, C.byref(g), C.byref(reads), C.byref(lens), C.byref(offs), C.byref(starts),
                                 C.byref(rev))
        return g, reads, lens, offs, starts, rev

    def views(self):
        """-> (genome bytes, [read bytes], [[(start_in_reference, reverse)]...], [names])"""
        g, reads, lens, offs, starts, rev = self._arrays()
        genome = C.string_at(g, self.genome_len)
        rs, cands, names = [], [], []
        for r in range(self.n_reads):
            rs.append(C.string_at(reads[r], lens[r]))
            cands.append([(int(starts[k]), bool(rev[k])) for k in range(offs[r], offs[r + 1])])
            names.append(self.lib.scrg_job_read_name(self.h, r).decode())
        return genome, rs, cands, names

    def pair_chromosome(self, k):
        s, ln = C.c_uint64(), C.c_uint64()
        nm = self.lib.scrg_job_pair_chromosome(self.h, k, C.byref(s), C.byref(ln))
        return nm.decode(), int(s.value), int(ln.value)

    def align(self, aligner, out_path=None, fmt="paf", max_edits=None, max_edit_per_mille=None, diff=None, report=None, costs=None, report_tags=True,
              cigar_form=None, clip=None, mapq=None, **params):
        """Aligns every pair on `aligner`'s GPU; optionally writes PAF/SAM.  -> [Alignment]; the pairs' statuses are left in
        aligner.last_status.  max_edits / max_edit_per_mille: an edit limit for this call (Aligner.set_edit_limit) — pairs over
        it have status SCRG_PAIR_OVER_EDIT_LIMIT and an empty CIGAR, PAF leaves them out and SAM writes them unmapped.
        best=True: best-candidate mode (SCRG_OUT_BEST) — only every read's best candidate keeps its CIGAR, the others have status
        SCRG_PAIR_NOT_BEST; PAF then holds the winners only (tp:A:P) and SAM one record per read.
        distance_only=True: distance-only mode (SCRG_OUT_DISTANCE) — every CIGAR is "", aligner.last_text_end has the text every
        alignment consumed, and the only format such a result can be written in is fmt="tsv" (read name, read length, strand,
        chromosome, target start, target end, edit distance).
        diff="md" / "cs": every pair's difference string for this call (Aligner.set_diff) — written as MD:Z: / cs:Z: tags on the
        PAF and SAM records (not with fmt="tsv") and left in aligner.last_diff.
        report=True: every pair's alignment report for this call (Aligner.set_report) — written as AS:i: / de:f: tags on the PAF and
        SAM records (scrg_job_write_report; costs = (match, mismatch, gap open, gap extend), default 2, 4, 4, 2), left in
        aligner.last_report (a structured array) and aligner.last_report_failed; report_tags=False keeps the tags out of the file.
        cigar_form="windowed" / "merged" / "m": the form of the CIGAR text for this call (Aligner.set_cigar_form) — what the
        Alignments hold and what SAM column 6 and PAF's cg:Z: get.
        clip=True or (match, mismatch, gap open, gap extend): every pair comes back as its best-scoring stretch for this call
        (Aligner.set_clip) — the file is written by scrg_job_write_clipped (soft clips and a moved POS in SAM, query and target
        intervals in PAF, AS:i: and the stretch's NM:i: in both; not with fmt="tsv", diff= or report=) and the records are left in
        aligner.last_clip.
        mapq=True or an api.MapqRule (with best=True; it implies nothing): every read's summary and MAPQ for this call
        (Aligner.set_mapq) — the file is written by scrg_job_write_mapq (SAM column 5 of a winner's record and PAF column 12 are the
        read's MAPQ; not with fmt="tsv" or clip=) and the records are left in aligner.last_read_summary."""
        with_mapq = mapq not in (None, False)
        if with_mapq and (clip not in (None, False) or (fmt == "tsv" and out_path is not None)):
            raise api.ScroogeError(api.SCRG_ERR_INVALID_ARG, "the MAPQ goes into paf and sam records of whole alignments: not with tsv or clip= yet")
        if clip not in (None, False):
            if fmt == "tsv" and out_path is not None:
                raise api.ScroogeError(api.SCRG_ERR_INVALID_ARG, "tsv has no place for clip records: clipped alignments go with paf and sam")
            with aligner._call_limit(max_edits, max_edit_per_mille), aligner._call_form(cigar_form), aligner._call_diff(diff), aligner._call_report(report), \
                    aligner._call_clip(clip):
                return self._align_clipped(aligner, out_path, fmt, **params)
        if (diff is not None or report) and fmt == "tsv":
            raise api.ScroogeError(api.SCRG_ERR_INVALID_ARG, "tsv has no tags: difference strings and the report's tags go with paf and sam")
        with aligner._call_limit(max_edits, max_edit_per_mille), aligner._call_form(cigar_form), aligner._call_diff(diff), aligner._call_report(report), \
                aligner._call_mapq(mapq):
            return self._align(aligner, out_path, fmt, diff is not None, bool(report), costs, report_tags, with_mapq, **params)

    def align_paired(self, aligner, out_path=None, fmt="sam", rule=None, max_edits=None, max_edit_per_mille=None, cigar_form=None, **params):
        """scrg_job_align_paired: the job's reads 2m and 2m+1 are mates (an interleaved FASTQ; an odd number of reads is
        SCRG_ERR_FORMAT), and every mate pair's winners are chosen together on `aligner`'s GPU by `rule` (an api.MateRule; None:
        FR, any span, penalty 0).  -> ([Alignment], mates): the alignments as align(best=True) returns them, the statuses in
        aligner.last_status, and one record per mate pair (api.mate_dtype(); winner[] are pair indices).  out_path: the file
        scrg_job_write_paired writes — fmt="sam": one record per read with the pair's FLAG bits, RNEXT, PNEXT and TLEN; "paf":
        the winners only."""
        import numpy as np
        if fmt not in ("paf", "sam"):
            raise api.ScroogeError(api.SCRG_ERR_INVALID_ARG, "a paired result is written as sam or paf")
        res, mt = C.POINTER(api.Result)(), C.POINTER(api.Mates)()
        with aligner._call_limit(max_edits, max_edit_per_mille), aligner._call_form(cigar_form):
            st = self.lib.scrg_job_align_paired(aligner.h, C.byref(aligner._params(params)), self.h, api._mate_rule(rule), C.byref(mt), C.byref(res))
        if st == SCRG_ERR_FORMAT:
            raise api.ScroogeError(st, "mate pairs: the job has an odd number of reads (an interleaved FASTQ has read 2m and 2m+1 as mates)")
        aligner._check(st, allow=(api.SCRG_ERR_CIGAR_OVERFLOW,))
        try:
            m = mt.contents
            mates = np.zeros(int(m.n_mates), dtype=api.mate_dtype())
            if m.n_mates:
                C.memmove(mates.ctypes.data, m.records, 32 * int(m.n_mates))
            if out_path is not None:
                w = self.lib.scrg_job_write_paired(self.h, res, mt, str(out_path).encode(), {"paf": 0, "sam": 1}[fmt])
                if w != 0:
                    raise api.ScroogeError(w, "could not write %s" % out_path)
            r = res.contents
            n = int(r.n_pairs)
            text = C.string_at(r.cigar_text, int(r.cigar_offset[n])) if n else b""
            out = [api.Alignment(text[int(r.cigar_offset[i]):int(r.cigar_offset[i + 1]) - 1].decode(), int(r.edit_distance[i])) for i in range(n)]
            aligner.last_timing = {"kernel_ns": int(r.kernel_ns), "pack_ns": int(r.pack_ns), "total_ns": int(r.total_ns)}
            aligner.last_status = [int(r.pair_status[i]) for i in range(n)]
            aligner.last_text_end = None
        finally:
            self.lib.scrg_result_free(res)
            api._lazy(self.lib, "scrg_mates_free")(mt)
        return out, mates

    def write_pileup(self, pileup, path, min_depth=1):
        """scrg_job_write_pileup: a pileup of this job's genome (the dict Aligner.take_pileup returns: "counts", a
        (7, genome_len + 1) uint32 array, and "target_len") as a TSV — chrom, pos (1-based), ref, depth, match, A, C, G, T, del, ins —
        one row per position whose depth is at least max(min_depth, 1)."""
        import numpy as np
        counts = np.ascontiguousarray(pileup["counts"], dtype=np.uint32)
        if counts.size != api.SCRG_PILE_PLANES * (int(pileup["target_len"]) + 1):
            raise api.ScroogeError(api.SCRG_ERR_INVALID_ARG, "counts is not (7, target_len + 1)")
        rec = api.Pileup(int(pileup["target_len"]), int(pileup.get("n_alignments", 0)), int(pileup.get("n_out_of_range", 0)),
                         counts.ctypes.data_as(C.POINTER(C.c_uint32)))
        w = self.lib.scrg_job_write_pileup(self.h, C.byref(rec), str(path).encode(), int(min_depth))
        if w != 0:
            raise api.ScroogeError(w, "could not write %s" % path)

    def write_sites(self, sites, path):
        """scrg_job_write_sites: sites of this job's genome (the dict Aligner.take_pileup_sites returns, or {"sites":
        api.pileup_sites_from_counts(...), "target_len": ...}) as a TSV — the eleven columns of write_pileup, then alt, call (A C G
        T, * deleted, . none) and flags — one row per site."""
        import numpy as np
        recs = np.ascontiguousarray(sites["sites"], dtype=api.site_dtype())
        rule = api.SiteRule(*[int(x) for x in sites.get("rule", (1, 1, 0))], 0)
        rec = api.PileupSites(int(sites["target_len"]), int(sites.get("n_alignments", 0)), int(sites.get("n_out_of_range", 0)), len(recs), rule,
                              recs.ctypes.data if len(recs) else None)
        w = self.lib.scrg_job_write_sites(self.h, C.byref(rec), str(path).encode())
        if w != 0:
            raise api.ScroogeError(w, "could not write %s" % path)

    def _align_clipped(self, aligner, out_path, fmt, **params):
        res = C.POINTER(api.Result)()
        st = self.lib.scrg_job_align(aligner.h, C.byref(aligner._params(params)), self.h, C.byref(res))
        aligner._check(st, allow=(api.SCRG_ERR_CIGAR_OVERFLOW,))
        cp = C.POINTER(api.Clip)()
        try:
            import numpy as np
            aligner._check(api._lazy(self.lib, "scrg_ctx_take_clip")(aligner.h, C.byref(cp)))
            n_c = int(cp.contents.n_pairs)
            aligner.last_clip = np.ctypeslib.as_array(C.cast(cp.contents.pairs, C.POINTER(C.c_uint32)), shape=(n_c * len(api.CLIP_FIELDS),)) \
                .copy().view(api.clip_dtype()) if n_c else np.zeros(0, dtype=api.clip_dtype())
            if out_path is not None:
                w = self.lib.scrg_job_write_clipped(self.h, res, cp, str(out_path).encode(), {"paf": 0, "sam": 1, "tsv": 2}[fmt])
                if w != 0:
                    raise api.ScroogeError(w, "could not write %s" % out_path)
            r = res.contents
            n = int(r.n_pairs)
            text = C.string_at(r.cigar_text, int(r.cigar_offset[n])) if n else b""
            out = [api.Alignment(text[int(r.cigar_offset[i]):int(r.cigar_offset[i + 1]) - 1].decode(), int(r.edit_distance[i])) for i in range(n)]
            aligner.last_timing = {"kernel_ns": int(r.kernel_ns), "pack_ns": int(r.pack_ns), "total_ns": int(r.total_ns)}
            aligner.last_status = [int(r.pair_status[i]) for i in range(n)]
            aligner.last_text_end = None
        finally:
            self.lib.scrg_result_free(res)
            if cp:
                api._lazy(self.lib, "scrg_clip_free")(cp)
        return out

    def _align(self, aligner, out_path, fmt, with_diff, with_report=False, costs=None, report_tags=True, with_mapq=False, **params):
        res = C.POINTER(api.Result)()
        st = self.lib.scrg_job_align(aligner.h, C.byref(aligner._params(params)), self.h, C.byref(res))
        aligner._check(st, allow=(api.SCRG_ERR_CIGAR_OVERFLOW,))
        d = C.POINTER(api.Diff)()
        rp = C.POINTER(api.Report)()
        sm = C.POINTER(api.ReadSummaries)()
        try:
            if with_mapq:
                import numpy as np
                aligner._check(api._lazy(self.lib, "scrg_ctx_take_read_summary")(aligner.h, C.byref(sm)))
                aligner.last_read_summary = np.zeros(int(sm.contents.n_reads), dtype=api.read_summary_dtype())
                if sm.contents.n_reads:
                    C.memmove(aligner.last_read_summary.ctypes.data, sm.contents.reads, 32 * int(sm.contents.n_reads))
            if with_report:
                import numpy as np
                aligner._check(api._lazy(self.lib, "scrg_ctx_take_report")(aligner.h, C.byref(rp)))
                n_r = int(rp.contents.n_pairs)
                aligner.last_report_failed = int(rp.contents.n_failed)
                aligner.last_report = np.ctypeslib.as_array(C.cast(rp.contents.pairs, C.POINTER(C.c_uint32)), shape=(n_r * len(api.REPORT_FIELDS),)) \
                    .copy().view(api.report_dtype()) if n_r else np.zeros(0, dtype=api.report_dtype())
            if with_diff:
                aligner._check(api._lazy(self.lib, "scrg_ctx_take_diff")(aligner.h, C.byref(d)))
                n_d = int(d.contents.n_pairs)
                blob = C.string_at(d.contents.text, int(d.contents.offset[n_d])) if n_d else b""
                aligner.last_diff = [blob[int(d.contents.offset[i]):int(d.contents.offset[i + 1]) - 1].decode() for i in range(n_d)]
            if out_path is not None:
                cost_arr = (C.c_int64 * 4)(*[int(x) for x in costs]) if costs is not None else None
                if with_mapq:
                    w = self.lib.scrg_job_write_mapq(self.h, res, d, rp if report_tags else None, cost_arr, sm, str(out_path).encode(), {"paf": 0, "sam": 1, "tsv": 2}[fmt])
                else:
                    w = self.lib.scrg_job_write_report(self.h, res, d, rp if report_tags else None, cost_arr, str(out_path).encode(), {"paf": 0, "sam": 1, "tsv": 2}[fmt])
                if w != 0:
                    raise api.ScroogeError(w, "could not write %s" % out_path)
            r = res.contents
            n = int(r.n_pairs)
            text = C.string_at(r.cigar_text, int(r.cigar_offset[n])) if n else b""
            out = [api.Alignment(text[int(r.cigar_offset[i]):int(r.cigar_offset[i + 1]) - 1].decode(),
                                 int(r.edit_distance[i])) for i in range(n)]
            aligner.last_timing = {"kernel_ns": int(r.kernel_ns), "pack_ns": int(r.pack_ns),
                                   "total_ns": int(r.total_ns)}
            aligner.last_status = [int(r.pair_status[i]) for i in range(n)]
            aligner.last_text_end = [int(r.text_end[i]) for i in range(n)] if r.text_end else None
        finally:
            self.lib.scrg_result_free(res)
            if d:
                api._lazy(self.lib, "scrg_diff_free")(d)
            if rp:
                api._lazy(self.lib, "scrg_report_free")(rp)
            if sm:
                api._lazy(self.lib, "scrg_read_summaries_free")(sm)
        return out
