"""Command-line front door: align the candidate locations of a read set on a GPU.

    python -m scrooge_amd.cli --reference=genome.fa --reads=reads.fastq \\
        [--seeds=seeds.paf | --seed_rule=K,STRIDE,MAX_OCC,BAND,MIN_HITS,MAX_CAND --seed_sample=S] \\
        [--out=aln.paf] [--format=paf|sam|tsv] [--reverse_strand] [--read_length_cap=N] \\
        [--dataset_inflation=K] [--W=64 --O=33] [--device=0] [--validate] \\
        [--paired [--mate_rule=MIN,MAX,FR|RF|FF|ANY,PENALTY]] \\
        [--max_edits=K] [--max_edit_per_mille=P] [--best] [--distance_only] [--md | --cs] \\
        [--report] [--score=M,X,O,E] [--verify] [--cigar=windowed|merged|m] [--clip] [--clip_costs=M,X,O,E] \\
        [--pileup=FILE] [--pileup_min_depth=N] [--sites=FILE] [--sites_rule=DEPTH,ALT,PERMILLE] \\
        [--mapq [--mapq_rule=PER_EDIT,MAX,ZERO_PER_MILLE] [--pileup_min_mapq=Q]]

Without --seeds the candidate locations are found on the GPU from a k-mer index of the reference (both strands).  With it: the same
inputs and preparation as the reference's performance harness
(`tests --reference= --reads= --seeds=`, src/tests.cu:335-410, 782-813: forward-strand candidates,
optional length cap and inflation, reads sorted longest first) and the same report lines, which the
reference's sweep driver scrapes (scripts/profile.py:170-175)."""
import argparse
import sys
import time


def main(argv=None):
    ap = argparse.ArgumentParser(prog="scrooge_amd.cli", description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reference", required=True, help="genome FASTA")
    ap.add_argument("--reads", required=True, help="reads FASTQ")
    ap.add_argument("--seeds", default=None, help="candidate locations, .paf or .maf; without it they are found on the GPU from a k-mer index "
                                                  "of the reference, on both strands (--seed_rule); the reference is then packed and uploaded twice, once to be "
                                                  "indexed and once by the alignment")
    ap.add_argument("--seed_rule", default=None, metavar="K,STRIDE,MAX_OCC,BAND,MIN_HITS,MAX_CAND",
                    help="the rule the candidates are found by without --seeds: bases per k-mer (8..16), the stride of the indexed reference "
                         "positions (1..64), the most index entries of a k-mer that still counts (1..65535), the largest gap between "
                         "neighbouring diagonals of a cluster (0..65535), the fewest hits of a candidate (>= 1) and the most candidates per "
                         "read (1..64); default 13,4,64,32,2,4")
    ap.add_argument("--seed_sample", type=int, default=None, metavar="S",
                    help="without --seeds: sample the k-mers of reference and reads alike as closed syncmers of S-mers (3 .. K - 1): fewer "
                         "index entries and lookups, about 2 / (K - S + 1) of them; default 0, every k-mer")
    ap.add_argument("--out", help="write one alignment per candidate (PAF with cg:Z:, SAM, or TSV: read name, read length, strand, "
                                  "chromosome, target start, target end, edit distance)")
    ap.add_argument("--format", choices=["paf", "sam", "tsv"], default=None, help="default: paf (tsv with --distance_only)")
    ap.add_argument("--reverse_strand", action="store_true",
                    help="align '-' candidates with the reverse-complemented read (the reference drops them)")
    ap.add_argument("--read_length_cap", type=int, default=-1)
    ap.add_argument("--dataset_inflation", type=int, default=1)
    ap.add_argument("--W", type=int, default=64)
    ap.add_argument("--O", type=int, default=33)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--validate", action="store_true", help="check every CIGAR against the sequences (validateCigarString)")
    ap.add_argument("--max_edits", type=int, default=None,
                    help="edit limit: drop a candidate as soon as its alignment has more than K edits")
    ap.add_argument("--max_edit_per_mille", type=int, default=None,
                    help="edit limit per read base: more than floor(P * read length / 1000) edits (P in 1..1000)")
    ap.add_argument("--best", action="store_true",
                    help="keep only every read's best candidate (fewest edits, ties: the first), chosen on the GPU: PAF gets the "
                         "winners (tp:A:P), SAM one record per read (MAPQ 0 for a tied winner, unmapped without one)")
    ap.add_argument("--distance_only", action="store_true",
                    help="edit distance and target end of every candidate, no CIGARs (nothing is traced into runs, stored or "
                         "transferred for them); implies --format tsv; works with --best, --max_edits and --reverse_strand")
    ap.add_argument("--md", action="store_true", help="add an MD:Z: tag to every PAF / SAM record that has an alignment (made on the GPU)")
    ap.add_argument("--cs", action="store_true", help="add a short cs:Z: tag instead (what paftools call reads)")
    ap.add_argument("--report", action="store_true",
                    help="add AS:i: (affine score) and de:f: (gap-compressed divergence) tags to every PAF / SAM record that has an "
                         "alignment, from the alignment report made on the GPU")
    ap.add_argument("--score", default=None, metavar="M,X,O,E",
                    help="the costs of AS:i: — match bonus, mismatch, gap open and gap extend costs (default 2,4,4,2)")
    ap.add_argument("--verify", action="store_true",
                    help="check every alignment against its sequences and its edit distance on the GPU (the report's verdict); "
                         "exit status 1 if one fails")
    ap.add_argument("--cigar", choices=["windowed", "merged", "m"], default="windowed",
                    help="the form of every CIGAR (made on the GPU): windowed = one run per window stretch, as the reference writes "
                         "them (29=21=); merged = adjacent equal operations merged (50=); m = merged, with = and X written M")
    ap.add_argument("--clip", action="store_true",
                    help="soft-clip every alignment to its best-scoring stretch (chosen on the GPU): SAM gets S items and a moved POS, "
                         "PAF the query and target intervals, both AS:i: and the stretch's NM:i:")
    ap.add_argument("--clip_costs", default=None, metavar="M,X,O,E",
                    help="the costs --clip scores with: match bonus (1..255), mismatch, gap open and gap extend costs (0..255; default 2,4,4,2)")
    ap.add_argument("--pileup", default=None, metavar="FILE",
                    help="also write what the alignments say at every genome position (summed on the GPU) as a TSV: chrom, pos, ref, "
                         "depth, match, A, C, G, T, del, ins; with --best only the winners pile up")
    ap.add_argument("--pileup_min_depth", type=int, default=None, metavar="N", help="rows of --pileup: positions that at least N alignments cover (default 1)")
    ap.add_argument("--sites", default=None, metavar="FILE",
                    help="also write the genome positions where the alignments disagree with the reference or insertions pile up (picked "
                         "and compacted on the GPU) as a TSV: the columns of --pileup, then alt, call (A C G T, * deleted, . none) and flags")
    ap.add_argument("--sites_rule", default=None, metavar="DEPTH,ALT,PERMILLE",
                    help="the rule of --sites: positions of at least DEPTH alignments where at least ALT observations, and PERMILLE per "
                         "mille of the depth, disagree (default 1,1,0; ALT 0 and PERMILLE 0: every covered position)")
    ap.add_argument("--paired", action="store_true",
                    help="the reads are an interleaved FASTQ: reads 2m and 2m+1 are mates, and each mate pair's candidates are chosen together "
                         "on the GPU (orientation, distance apart, least joint cost; the single bests where no combination is good enough); "
                         "SAM gets the pair's FLAG bits, RNEXT, PNEXT and TLEN, PAF the winners; implies --best")
    ap.add_argument("--mate_rule", default=None, metavar="MIN,MAX,FR|RF|FF|ANY,PENALTY",
                    help="the rule of --paired: span bounds (outermost start to outermost end, from starts and read lengths), orientation, and "
                         "the edits a proper combination may cost more than the two single bests (default 0,18446744073709551615,FR,0)")
    ap.add_argument("--mapq", action="store_true",
                    help="grade every read's winner on the GPU: SAM column 5 and PAF column 12 get a MAPQ from the distance to the read's "
                         "second-best candidate and the winner's own edit rate (0 for a tie; a heuristic, validated against no truth set); "
                         "implies --best")
    ap.add_argument("--mapq_rule", default=None, metavar="PER_EDIT,MAX,ZERO_PER_MILLE",
                    help="the rule of --mapq: MAPQ per edit between best and second (0..255), the largest MAPQ (0..254), and the edits per "
                         "1000 read bases at which the winner's MAPQ reaches 0 (1..1000); default 10,60,250")
    ap.add_argument("--pileup_min_mapq", type=int, default=None, metavar="Q",
                    help="with --mapq and --pileup / --sites: only reads placed with MAPQ >= Q pile up (filtered on the GPU)")
    args = ap.parse_args(argv)
    seed_rule = None
    if args.seed_rule is not None:
        if args.seeds is not None:
            ap.error("--seed_rule is the rule candidates are FOUND by: with --seeds they come from the file")
        try:
            seed_rule = tuple(int(x) for x in args.seed_rule.split(","))
        except ValueError:
            seed_rule = ()
        lo_hi = ((8, 16), (1, 64), (1, 65535), (0, 65535), (1, 2**32 - 1), (1, 64))
        if len(seed_rule) != 6 or any(not lo <= v <= hi for v, (lo, hi) in zip(seed_rule, lo_hi)):
            ap.error("--seed_rule takes K,STRIDE,MAX_OCC,BAND,MIN_HITS,MAX_CAND with 8 <= K <= 16, 1 <= STRIDE <= 64, 1 <= MAX_OCC <= 65535, "
                     "0 <= BAND <= 65535, MIN_HITS >= 1 and 1 <= MAX_CAND <= 64")
    if args.seed_sample is not None:
        if args.seeds is not None:
            ap.error("--seed_sample samples the k-mers candidates are FOUND by: with --seeds they come from the file")
        k = 13 if seed_rule is None else seed_rule[0]
        if args.seed_sample != 0 and not 3 <= args.seed_sample < k:
            ap.error("--seed_sample takes 0 or 3 .. K - 1 (K = %d)" % k)
    mapq_rule = None
    if args.mapq_rule is not None:
        if not args.mapq:
            ap.error("--mapq_rule sets the rule of --mapq")
        try:
            mapq_rule = tuple(int(x) for x in args.mapq_rule.split(","))
        except ValueError:
            mapq_rule = ()
        if len(mapq_rule) != 3 or not 0 <= mapq_rule[0] <= 255 or not 0 <= mapq_rule[1] <= 254 or not 1 <= mapq_rule[2] <= 1000:
            ap.error("--mapq_rule takes PER_EDIT,MAX,ZERO_PER_MILLE with 0 <= PER_EDIT <= 255, 0 <= MAX <= 254 and 1 <= ZERO_PER_MILLE <= 1000")
    if args.pileup_min_mapq is not None:
        if not args.mapq or (args.pileup is None and args.sites is None):
            ap.error("--pileup_min_mapq filters what piles up by the MAPQ: it goes with --mapq and --pileup or --sites")
        if not 0 <= args.pileup_min_mapq <= 254:
            ap.error("--pileup_min_mapq takes a MAPQ of 0 .. 254")
    if args.mapq and (args.paired or args.clip or args.distance_only or args.format == "tsv"):
        ap.error("--mapq grades single reads' winners in sam and paf records of whole alignments: it does not go with --paired, --clip, "
                 "--distance_only or tsv yet")
    if args.mapq:
        args.best = True
    mate_rule = None
    if args.mate_rule is not None:
        if not args.paired:
            ap.error("--mate_rule sets the rule of --paired")
        parts = args.mate_rule.split(",")
        try:
            mate_rule = (int(parts[0]), int(parts[1]), {"FR": 0, "RF": 1, "FF": 2, "ANY": 3}[parts[2].upper()], int(parts[3])) if len(parts) == 4 else None
        except (ValueError, KeyError):
            mate_rule = None
        if mate_rule is None or not 0 <= mate_rule[0] <= mate_rule[1] < 2**64 or not 0 <= mate_rule[3] < 2**32:
            ap.error("--mate_rule takes MIN,MAX,FR|RF|FF|ANY,PENALTY with 0 <= MIN <= MAX < 2^64 and 0 <= PENALTY < 2^32")
    if args.paired and (args.md or args.cs or args.report or args.verify or args.clip or args.distance_only or args.format == "tsv"):
        ap.error("--paired writes sam or paf from whole alignments: it does not go with --md / --cs, --report / --verify, --clip, "
                 "--distance_only or tsv yet")
    if args.pileup_min_depth is not None and args.pileup is None:
        ap.error("--pileup_min_depth chooses the rows of --pileup")
    site_rule = (1, 1, 0)
    if args.sites_rule is not None:
        if args.sites is None:
            ap.error("--sites_rule sets the rule of --sites")
        try:
            site_rule = tuple(int(x) for x in args.sites_rule.split(","))
        except ValueError:
            site_rule = ()
        if len(site_rule) != 3 or not 1 <= site_rule[0] < 2**32 or not 0 <= site_rule[1] < 2**32 or not 0 <= site_rule[2] <= 1000:
            ap.error("--sites_rule takes three integers: depth (1 .. 2^32 - 1), alt (0 .. 2^32 - 1), per mille (0 .. 1000)")
    if args.sites is not None and (args.distance_only or args.clip):
        ap.error("--sites come from the pileup, which is summed from the runs of whole alignments: they do not go with --distance_only or --clip")
    if args.pileup is not None and (args.distance_only or args.clip):
        ap.error("--pileup is summed from the runs of whole alignments: it does not go with --distance_only or --clip")
    clip = None
    if args.clip_costs is not None:
        if not args.clip:
            ap.error("--clip_costs sets the costs of --clip")
        try:
            clip = tuple(int(x) for x in args.clip_costs.split(","))
        except ValueError:
            clip = ()
        if len(clip) != 4:
            ap.error("--clip_costs takes four integers: match,mismatch,gap_open,gap_extend")
    elif args.clip:
        clip = True
    if args.clip and (args.md or args.cs or args.report or args.verify or args.distance_only or args.validate or args.format == "tsv"):
        ap.error("--clip returns a stretch of every alignment: it does not go with --md / --cs, --report / --verify, --validate, "
                 "--distance_only or tsv yet")
    if args.cigar == "m" and args.validate:
        ap.error("--validate checks every = and X against the sequences: --cigar m writes neither (--verify checks the runs instead)")
    costs = None
    if args.score is not None:
        try:
            costs = tuple(int(x) for x in args.score.split(","))
        except ValueError:
            costs = ()
        if len(costs) != 4:
            ap.error("--score takes four integers: match,mismatch,gap_open,gap_extend")
        if not args.report:
            ap.error("--score sets the costs of the AS:i: tag: it goes with --report")
    if (args.report or args.verify) and args.distance_only:
        ap.error("--report / --verify are made from CIGAR runs: --distance_only produces none")
    if args.report and args.format == "tsv":
        ap.error("--report adds tags to PAF and SAM records: tsv has none")
    if args.md and args.cs:
        ap.error("--md and --cs exclude each other: a call makes one kind of difference string")
    if (args.md or args.cs) and args.distance_only:
        ap.error("--md / --cs are made from CIGAR runs: --distance_only produces none")
    if (args.md or args.cs) and args.format == "tsv":
        ap.error("--md / --cs are tags of PAF and SAM records: tsv has none")
    if args.distance_only:
        if args.validate:
            ap.error("--validate checks CIGARs: --distance_only produces none")
        if args.format not in (None, "tsv"):
            ap.error("--distance_only writes tsv: a distance has no PAF match columns and no SAM CIGAR")
        args.format = "tsv"
    elif args.format is None:
        args.format = "paf"

    import scrooge_amd
    from scrooge_amd import io as sio

    t0 = time.time()
    job = sio.Job(args.reference, args.reads, args.seeds, reverse_strand=int(args.reverse_strand),
                  read_length_cap=args.read_length_cap, inflation=args.dataset_inflation)
    print("loaded %d reads, %d candidate locations, %d bp reference (%d sequences) in %.1fs"
          % (job.n_reads, job.n_pairs, job.genome_len, job.n_chromosomes, time.time() - t0), file=sys.stderr)
    al = scrooge_amd.Aligner(args.device)
    if args.seeds is None:
        ts = time.time()
        if args.seed_sample:
            al.set_seed_sampling(args.seed_sample)
        job.seed(al, None if seed_rule is None else scrooge_amd.api.SeedRule(*seed_rule))
        print("found %d candidate locations on the GPU in %.1fs" % (job.n_pairs, time.time() - ts), file=sys.stderr)
    if args.pileup is not None or args.sites is not None:
        al.set_pileup(True)
    t1 = time.time()
    mates = None
    if args.paired:
        from scrooge_amd.api import MateRule
        alns, mates = job.align_paired(al, out_path=args.out, fmt=args.format, rule=None if mate_rule is None else MateRule(*mate_rule), W=args.W, O=args.O,
                                       max_edits=args.max_edits, max_edit_per_mille=args.max_edit_per_mille,
                                       **({"cigar_form": args.cigar} if args.cigar != "windowed" else {}))
    else:
        alns = job.align(al, out_path=args.out, fmt=args.format, W=args.W, O=args.O, max_edits=args.max_edits,
                         max_edit_per_mille=args.max_edit_per_mille, **({"best": True} if args.best else {}),
                         **({"distance_only": True} if args.distance_only else {}),
                         **({"diff": "md" if args.md else "cs"} if args.md or args.cs else {}),
                         **({"cigar_form": args.cigar} if args.cigar != "windowed" else {}),
                         **({"clip": clip} if clip is not None else {}),
                         **({"mapq": scrooge_amd.api.MapqRule(*(mapq_rule or (10, 60, 250)), args.pileup_min_mapq or 0)} if args.mapq else {}),
                         **({"report": True, "costs": costs, "report_tags": args.report} if args.report or args.verify else {}))
    wall_ms = (time.time() - t1) * 1e3
    if args.pileup is not None:
        pile = al.take_pileup()
        job.write_pileup(pile, args.pileup, 1 if args.pileup_min_depth is None else args.pileup_min_depth)
        print("piled up %d alignments (%d reach outside the reference)" % (pile["n_alignments"], pile["n_out_of_range"]), file=sys.stderr)
        if args.sites is not None:      # (one take: the counts are on the host already, the rule is applied to them there)
            found = dict(pile, sites=scrooge_amd.api.pileup_sites_from_counts(pile["counts"], job.genome(), *site_rule), rule=site_rule)
            job.write_sites(found, args.sites)
            print("%d sites" % len(found["sites"]), file=sys.stderr)
    elif args.sites is not None:
        found = al.take_pileup_sites(*site_rule)
        job.write_sites(found, args.sites)
        print("piled up %d alignments (%d reach outside the reference), %d sites" % (found["n_alignments"], found["n_out_of_range"], found["n_sites"]),
              file=sys.stderr)
    over = [s == scrooge_amd.api.SCRG_PAIR_OVER_EDIT_LIMIT for s in al.last_status]
    if args.max_edits is not None or args.max_edit_per_mille is not None:
        print("%d of %d candidate locations over the edit limit (no alignment)" % (sum(over), len(over)), file=sys.stderr)
    not_best = [s == scrooge_amd.api.SCRG_PAIR_NOT_BEST for s in al.last_status]
    if args.mapq:
        q = args.pileup_min_mapq or 0
        summary = al.last_read_summary
        print("%d of %d reads placed with MAPQ >= %d" % (int(((summary["flags"] & scrooge_amd.api.SCRG_MAPQ_KEPT) != 0).sum()), len(summary), q), file=sys.stderr)
    if mates is not None:
        print("%d of %d mate pairs proper" % (int((mates["flags"] & 1).sum()), len(mates)), file=sys.stderr)
    if args.best or args.paired:
        print("%d of %d candidate locations kept as their read's best" % (len(over) - sum(over) - sum(not_best), len(over)), file=sys.stderr)
    kernel_ms = al.last_timing["kernel_ns"] / 1e6
    # report lines as src/tests.cu:402-406
    print("align_all() took %dms (data transfers, conversion, gpu kernel and post-processing)" % wall_ms)
    print("GPU kernel took %dms" % kernel_ms)
    print("GPU kernel ran at %d aligns/second" % (len(alns) / max(kernel_ms, 1e-6) * 1e3))
    rc = 0
    if args.verify:
        verdict = al.last_report["verdict"]
        n_verified = int((verdict != scrooge_amd.api.REPORT_NO_ALIGNMENT).sum())
        for k in ((verdict != 0) & (verdict != scrooge_amd.api.REPORT_NO_ALIGNMENT)).nonzero()[0][:20]:
            print("FAILED verification of alignment %d: verdict %d at run %d" % (k, verdict[k], al.last_report["bad_run"][k]))
        print("verified %d alignments, %d failed" % (n_verified, al.last_report_failed))
        rc = 1 if al.last_report_failed else 0
    if args.validate:
        genome, reads, cands, _ = job.views()
        comp = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")
        k = bad = 0
        for r, cs in zip(reads, cands):
            for start, rev in cs:
                q = r.translate(comp)[::-1] if rev else r
                if over[k]:
                    # dropped at the limit: what it reports must lie above the limit
                    lim = scrooge_amd.api.edit_limit_for(len(q), args.max_edits, args.max_edit_per_mille)
                    if alns[k].cigar or lim is None or alns[k].edit_distance <= lim:
                        print("FAILED over-limit check for alignment %d" % k)
                        bad += 1
                    k += 1
                    continue
                if not_best[k]:
                    # not its read's best: no CIGAR to check
                    if alns[k].cigar:
                        print("FAILED not-best check for alignment %d" % k)
                        bad += 1
                    k += 1
                    continue
                # the alignment consumes a prefix of the suffix: at most len(read) + edits <= 2 * len(read) characters of it
                if sio.validate_alignment(genome[start:start + 2 * len(q) + args.W], q, alns[k].cigar, alns[k].edit_distance) != 0:
                    print("FAILED sanity check for alignment %d" % k)
                    bad += 1
                k += 1
        print("validated %d alignments, %d failed" % (k, bad))
        rc = 1 if bad or rc else 0
    return rc


if __name__ == "__main__":
    sys.exit(main())
