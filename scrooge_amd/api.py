"""ctypes binding of include/scrooge_amd.h."""
import contextlib
import ctypes as C
import dataclasses
import os
import subprocess
import sys
from collections import namedtuple

HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

# same two fields as the reference's Alignment_t (src/util.hpp:38-41)
Alignment = namedtuple("Alignment", ["cigar", "edit_distance"])

SCRG_OK = 0
SCRG_ERR_INVALID_ARG = 1
SCRG_ERR_BAD_BASE = 2
SCRG_ERR_NO_DEVICE = 3
SCRG_ERR_HIP = 4
SCRG_ERR_OOM = 5
SCRG_ERR_CIGAR_OVERFLOW = 6
SCRG_PAIR_OVER_EDIT_LIMIT = 7  # a pair status only: over the handle's edit limit (set_edit_limit), no alignment
SCRG_PAIR_NOT_BEST = 8         # a pair status only: best-candidate mode (best=True) — aligned, but another candidate of the read won
SCRG_OUT_ALL, SCRG_OUT_TEXT, SCRG_OUT_RUNS = 0, 1, 2      # scrg_params.outputs
SCRG_OUT_BEST = 4              # ... | SCRG_OUT_BEST: only every read's best candidate keeps its runs and text (mapping calls)
SCRG_OUT_DISTANCE = 16         # distance-only mode (distance_only=True): edit distance, status and text end of every pair, no runs, no text
DEVICE_STATUS_OVER_EDIT_LIMIT = 2   # the same in d_pair_status of the device-pointer calls
SCRG_ABI_VERSION = 8          # include/scrooge_amd.h (tests/test_abi.py holds the two equal)
SEQ_PAD_WORDS = 4
GROUP = 64                     # rows per group of the lane-interleaved layout
SEQ_PAD_WORDS_GROUPS = 2 * GROUP + 2


class ScroogeError(RuntimeError):
    def __init__(self, status, message):
        super().__init__("scrooge_amd status %d: %s" % (status, message))
        self.status = status


class Params(C.Structure):
    _fields_ = [("W", C.c_int32), ("O", C.c_int32), ("lanes_per_pair", C.c_int32),
                ("lds_rows", C.c_int32), ("waves_per_cu", C.c_int32),
                ("sort_by_length", C.c_int32), ("text_stride_words", C.c_int32), ("read_stride_words", C.c_int32),
                ("outputs", C.c_int32), ("reserved", C.c_int32 * 2), ("stranded", C.c_int32)]


READ_REVCOMP = 1 << 63            # include/scrooge_amd.h: SCRG_READ_REVCOMP
TEXT_REVCOMP = 1 << 63            # include/scrooge_amd.h: SCRG_TEXT_REVCOMP (bit 63 of text_off, on a handle with set_text_strands(True))


class PairDesc(C.Structure):
    _fields_ = [("text_off", C.c_uint64), ("text_len", C.c_uint64), ("read_off", C.c_uint64),
                ("read_len", C.c_uint64), ("cigar_off", C.c_uint64), ("cigar_cap", C.c_uint64)]


class Run(C.Structure):
    _fields_ = [("count", C.c_uint8), ("op", C.c_char)]


class Result(C.Structure):
    _fields_ = [("n_pairs", C.c_uint64),
                ("edit_distance", C.POINTER(C.c_int64)),
                ("pair_status", C.POINTER(C.c_uint32)),
                ("run_offset", C.POINTER(C.c_uint64)),
                ("runs", C.POINTER(Run)),
                ("cigar_offset", C.POINTER(C.c_uint64)),
                ("cigar_text", C.POINTER(C.c_char)),
                ("kernel_ns", C.c_int64), ("pack_ns", C.c_int64), ("total_ns", C.c_int64),
                ("text_end", C.POINTER(C.c_uint64))]      # distance-only mode; NULL otherwise


DIFF_OFF, DIFF_MD, DIFF_CS = 0, 1, 2      # include/scrooge_amd.h: SCRG_DIFF_* (difference strings: SAM's MD:Z:, PAF's short cs:Z:)
_DIFF_KINDS = {None: DIFF_OFF, "md": DIFF_MD, "cs": DIFF_CS}


class Diff(C.Structure):
    """scrg_diff: the difference strings of a host call, as Aligner.take_diff gets them."""
    _fields_ = [("n_pairs", C.c_uint64), ("kind", C.c_int32), ("offset", C.POINTER(C.c_uint64)), ("text", C.POINTER(C.c_char))]


def _diff_kind(kind):
    if kind in _DIFF_KINDS:
        return _DIFF_KINDS[kind]
    if kind in (DIFF_OFF, DIFF_MD, DIFF_CS) and not isinstance(kind, bool):
        return int(kind)
    raise ValueError('the difference-string kind is "md", "cs" or None, not %r' % (kind,))


CIGAR_WINDOWED, CIGAR_MERGED, CIGAR_M = 0, 1, 2      # include/scrooge_amd.h: SCRG_CIGAR_* (CIGAR FORMS: the form of the CIGAR text)
_CIGAR_FORMS = {"windowed": CIGAR_WINDOWED, "merged": CIGAR_MERGED, "m": CIGAR_M}


def _cigar_form(form):
    if isinstance(form, str) and form in _CIGAR_FORMS:
        return _CIGAR_FORMS[form]
    if form in (CIGAR_WINDOWED, CIGAR_MERGED, CIGAR_M) and not isinstance(form, (bool, str)):
        return int(form)
    raise ValueError('the CIGAR form is "windowed", "merged" or "m", not %r' % (form,))


def library_path(variant=None):
    """The shipped library, or — variant="select" — the TEST build of the same sources (-DSCRG_SELECT: ab_libs/lib_select.so),
    in which scrg_params.reserved[0] selects between formulations that give identical results; the parity tests that compare
    formulations load it next to the shipped one.  SCRG_LIB names another build of the shipped library (kernel A/B)."""
    if variant == "select":
        return os.path.join(HERE, "..", "ab_libs", "lib_select.so")
    if variant is not None:
        raise ValueError("unknown library variant %r" % (variant,))
    return os.environ.get("SCRG_LIB") or os.path.join(HERE, "libscrooge_amd.so")


def _source_digest(srcs):
    import hashlib
    h = hashlib.sha256()
    for f in sorted(srcs):
        h.update(os.path.basename(f).encode())
        with open(f, "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()


def build_library(force=False, variant=None):
    """Compile the HIP kernels + host code for gfx950 (hipcc cross-compiles without a GPU); variant="select": the test build
    (library_path).

    Whether the built library is current is decided by the CONTENT of the sources (a digest kept next to the
    library), not by modification times: a copy of the tree (the snapshot a GPU box gets) keeps the contents but
    not necessarily the order of the time stamps, and a needless rebuild costs a minute and needs a compiler."""
    so = library_path(variant)
    if variant is None and os.environ.get("SCRG_LIB"):
        return so
    src_dir = os.path.join(HERE, "csrc")
    srcs = [os.path.join(src_dir, f) for f in os.listdir(src_dir) if not f.startswith(".")] + \
        [os.path.join(HERE, "..", "include", f) for f in ("scrooge_amd.h", "scrooge_amd_io.h", "scrooge_amd_device.hpp")]
    stamp = so + ".sources.sha256"
    digest = _source_digest(srcs)

    def is_stale():
        if not os.path.exists(so):
            return True
        try:
            return open(stamp).read().strip() != digest
        except OSError:
            return True

    if force or is_stale():
        # several ranks of one job may get here at once: serialise, and re-check under the lock
        import fcntl
        with open(os.path.join(HERE, ".build.lock"), "w") as lk:
            fcntl.flock(lk, fcntl.LOCK_EX)
            if force or is_stale():
                # (make echoes the compiler command: keep it off stdout, which callers such as bench.py reserve for their
                # own output; -B because make's own idea of freshness is the time stamps)
                cmd = ["make", "-C", src_dir, "--no-print-directory", "-B"] + (["VARIANT=%s" % variant] if variant else [])
                subprocess.check_call(cmd, stdout=sys.stderr)
                with open(stamp, "w") as fh:
                    fh.write(digest + "\n")
    return so


_VARIANT_LIBS = {}


def load_library(variant=None):
    """Load libscrooge_amd.so (variant="select": the test build, a second handle next to it); raises (never falls back) when
    it is missing."""
    global _LIB
    if variant is None and _LIB is not None:
        return _LIB
    if variant is not None and variant in _VARIANT_LIBS:
        return _VARIANT_LIBS[variant]
    so = library_path(variant)
    # PyTorch-ROCm ships its own libamdhip64.so; whichever HIP runtime is loaded first serves the whole
    # process.  If this library pulled in /opt/rocm's copy first, a later `import torch` finds no GPU.
    # So when torch is installed, let it load its runtime before us (SCRG_NO_TORCH_PRELOAD=1 skips this).
    if "torch" not in sys.modules and not os.environ.get("SCRG_NO_TORCH_PRELOAD"):
        try:
            import torch  # noqa: F401
        except Exception:
            pass
    if not os.path.exists(so):
        raise ScroogeError(SCRG_ERR_NO_DEVICE,
                           "%s not built; run scrooge_amd.build_library() (needs hipcc)" % so)
    lib = C.CDLL(so)
    vp, u64, i32p = C.c_void_p, C.c_uint64, C.POINTER(C.c_int32)
    sigs = {
        "scrg_params_default": (None, [C.POINTER(Params)]),
        "scrg_params_resolve": (C.c_int32, [C.POINTER(Params), C.POINTER(Params)]),
        "scrg_ctx_create": (C.c_int32, [C.c_int, C.POINTER(vp)]),
        "scrg_ctx_destroy": (None, [vp]),
        "scrg_ctx_set_stream": (C.c_int32, [vp, vp]),
        "scrg_ctx_use_own_stream": (C.c_int32, [vp]),
        "scrg_stream_create": (C.c_int32, [C.c_int, C.c_int, C.POINTER(vp)]),
        "scrg_stream_destroy": (C.c_int32, [vp]),
        "scrg_last_error": (C.c_char_p, [vp]),
        "scrg_status_string": (C.c_char_p, [C.c_int32]),
        "scrg_set_log": (None, [C.c_int]),
        "scrg_get_log": (C.c_int, []),
        "scrg_device_count": (C.c_int, []),
        "scrg_build_flags": (C.c_int, []),
        "scrg_abi_version": (C.c_int, []),
        "scrg_result_free": (None, [C.POINTER(Result)]),
        "scrg_result_pool_trim": (None, []),
        "scrg_align_pairs": (C.c_int32, [vp, C.POINTER(Params), u64, C.POINTER(C.c_char_p),
                                         C.POINTER(u64), C.POINTER(C.c_char_p), C.POINTER(u64),
                                         C.POINTER(C.POINTER(Result))]),
        "scrg_align_mapping": (C.c_int32, [vp, C.POINTER(Params), C.c_char_p, u64, u64,
                                           C.POINTER(C.c_char_p), C.POINTER(u64), C.POINTER(u64),
                                           C.POINTER(u64), C.POINTER(C.POINTER(Result))]),
        "scrg_align_pairs_multi": (C.c_int32, [i32p, C.c_int32, C.POINTER(Params), u64, C.POINTER(C.c_char_p), C.POINTER(u64),
                                               C.POINTER(C.c_char_p), C.POINTER(u64), C.POINTER(C.POINTER(Result))]),
        "scrg_align_mapping_multi": (C.c_int32, [i32p, C.c_int32, C.POINTER(Params), C.c_char_p, u64, u64, C.POINTER(C.c_char_p),
                                                 C.POINTER(u64), C.POINTER(u64), C.POINTER(u64), vp, C.POINTER(C.POINTER(Result))]),
        "scrg_host_plan": (C.c_int32, [C.POINTER(Params), C.c_int32, u64, vp, vp, vp, vp, u64, C.POINTER(u64)]),
        "scrg_multi_release": (None, []),
        "scrg_multi_last_error": (C.c_char_p, []),
        "scrg_genome_set": (C.c_int32, [vp, C.c_char_p, u64]),
        "scrg_genome_clear": (None, [vp]),
        "scrg_align_mapping_resident": (C.c_int32, [vp, vp, u64, vp, vp, vp, vp, vp, vp]),
        "scrg_pack_planar": (C.c_int32, [vp, vp, u64, vp, vp]),
        "scrg_pack_planar_host": (C.c_int32, [vp, u64, vp, u64, u64]),
        "scrg_pack_planar_groups": (C.c_int32, [vp, vp, u64, u64, vp, vp]),
        "scrg_compact_runs_packed": (C.c_int32, [vp, vp, u64, vp, vp, vp, vp, vp]),
        "scrg_unpack_runs": (C.c_int32, [vp, u64, vp, vp]),
        "scrg_encode_edit_stream": (C.c_int32, [vp, C.POINTER(Params), u64, vp, vp, vp, vp, u64, vp, vp, vp]),
        "scrg_decode_edit_stream": (C.c_int32, [vp, vp, u64, vp, u64, vp, vp, vp, u64, vp, vp, u64, vp, vp]),
        "scrg_edit_stream_to_runs": (C.c_int32, [C.POINTER(Params), u64, vp, u64, vp, u64, C.POINTER(u64)]),
        "scrg_edit_stream_to_runs_lane": (C.c_int32, [C.POINTER(Params), u64, vp, u64, vp, u64, C.POINTER(u64)]),
        "scrg_runs_to_edit_stream": (C.c_int32, [C.POINTER(Params), vp, u64, vp, u64, C.POINTER(u64)]),
        "scrg_align_device": (C.c_int32, [vp, C.POINTER(Params), u64, vp, vp, vp, vp, vp, vp]),
        "scrg_compact_runs": (C.c_int32, [vp, u64, vp, vp, vp, vp, vp]),
        "scrg_align_device_edits": (C.c_int32, [vp, C.POINTER(Params), u64, vp, vp, vp, vp, vp, vp, vp]),
        "scrg_ascii_to_twobit": (C.c_int32, [vp, u64, vp, vp, vp, vp, vp, vp]),
        "scrg_query_launch": (C.c_int32, [vp, C.POINTER(Params), i32p, i32p, i32p, i32p]),
        "scrg_last_kernel_ms": (C.c_int32, [vp, C.POINTER(C.c_float)]),
        "scrg_debug_stats": (C.c_int32, [vp, C.POINTER(C.c_uint64)]),
    }
    for name, (res, args) in sigs.items():
        fn = getattr(lib, name)   # AttributeError if the library lacks a declared symbol
        fn.restype = res
        fn.argtypes = args
    # the signatures above are those of interface version SCRG_ABI_VERSION (include/scrooge_amd.h): a library built from other
    # sources (SCRG_LIB, a stale copy) must say so instead of taking shifted arguments
    if lib.scrg_abi_version() != SCRG_ABI_VERSION:
        raise ScroogeError(SCRG_ERR_INVALID_ARG, "%s has interface version %d, this binding speaks version %d"
                           % (so, lib.scrg_abi_version(), SCRG_ABI_VERSION))
    if variant is None:
        _LIB = lib
    else:
        _VARIANT_LIBS[variant] = lib
    return lib


EXPORTED_SYMBOLS = [
    "scrg_params_default", "scrg_params_resolve", "scrg_ctx_create", "scrg_ctx_destroy", "scrg_ctx_set_stream",
    "scrg_ctx_use_own_stream", "scrg_stream_create", "scrg_stream_destroy",
    "scrg_last_error", "scrg_status_string", "scrg_set_log", "scrg_get_log", "scrg_device_count", "scrg_build_flags", "scrg_abi_version",
    "scrg_result_free", "scrg_result_pool_trim", "scrg_align_pairs", "scrg_align_mapping", "scrg_align_pairs_multi", "scrg_align_mapping_multi",
    "scrg_host_plan", "scrg_multi_release", "scrg_multi_last_error", "scrg_genome_set", "scrg_genome_clear",
    "scrg_align_mapping_resident", "scrg_pack_planar", "scrg_pack_planar_host", "scrg_pack_planar_groups",
    "scrg_align_device", "scrg_align_device_edits", "scrg_compact_runs", "scrg_compact_runs_packed", "scrg_unpack_runs",
    "scrg_encode_edit_stream", "scrg_decode_edit_stream", "scrg_edit_stream_to_runs", "scrg_edit_stream_to_runs_lane", "scrg_runs_to_edit_stream", "scrg_ascii_to_twobit", "scrg_query_launch",
    "scrg_last_kernel_ms", "scrg_debug_stats", "scrg_ctx_set_edit_limit", "scrg_ctx_get_edit_limit", "scrg_edit_limit_for",
    "scrg_select_best", "scrg_host_plan_mapping", "scrg_align_device_distance",
    "scrg_ctx_set_text_strands", "scrg_ctx_get_text_strands", "scrg_text_window_planes", "scrg_align_mapping_directed",
    "scrg_align_mapping_anchored", "scrg_join_anchored_runs",
    "scrg_ctx_set_diff", "scrg_ctx_get_diff", "scrg_ctx_take_diff", "scrg_diff_free", "scrg_diff_lengths", "scrg_diff_render",
    "scrg_ctx_set_report", "scrg_ctx_get_report", "scrg_ctx_take_report", "scrg_report_free", "scrg_report_device",
    "scrg_ctx_set_cigar_form", "scrg_ctx_get_cigar_form", "scrg_cigar_text_lengths", "scrg_cigar_text_render",
    "scrg_ctx_set_clip", "scrg_ctx_get_clip", "scrg_ctx_take_clip", "scrg_clip_free", "scrg_clip_device",
    "scrg_ctx_set_pileup", "scrg_ctx_get_pileup", "scrg_ctx_take_pileup", "scrg_pileup_free", "scrg_pileup_add", "scrg_pileup_finish",
    "scrg_ctx_take_pileup_sites", "scrg_pileup_sites_free", "scrg_pileup_sites_scratch_bytes", "scrg_pileup_sites_mark", "scrg_pileup_sites_write",
    "scrg_select_mates", "scrg_select_mates_team", "scrg_align_mapping_paired", "scrg_mates_free", "scrg_host_plan_mates",
    "scrg_read_summary", "scrg_ctx_set_read_summary", "scrg_ctx_get_read_summary", "scrg_ctx_take_read_summary", "scrg_read_summaries_free",
    "scrg_seed_rule_default", "scrg_seed_rule_check", "scrg_genome_index", "scrg_genome_index_clear", "scrg_genome_index_info",
    "scrg_find_candidates", "scrg_candidates_free",
    "scrg_ctx_set_seed_sampling", "scrg_seed_sampling_info", "scrg_seed_key_selected"]

# Entry points bound on first use, outside the table load_library() insists on: a library from before they existed (the
# parent commit's, for a kernel A/B) still loads, and only a call that needs one of them fails.
_LAZY_SIGS = {
    "scrg_ctx_set_edit_limit": (C.c_int32, [C.c_void_p, C.c_int64, C.c_int32]),
    "scrg_ctx_get_edit_limit": (C.c_int32, [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int32)]),
    "scrg_edit_limit_for": (C.c_int32, [C.c_int64, C.c_int32, C.c_uint64, C.POINTER(C.c_int64)]),
    "scrg_select_best": (C.c_int32, [C.c_void_p, C.c_uint64] + [C.c_void_p] * 5),
    "scrg_host_plan_mapping": (C.c_int32, [C.POINTER(Params), C.c_int32, C.c_uint64] + [C.c_void_p] * 4 + [C.c_uint64, C.POINTER(C.c_uint64)]),
    "scrg_align_device_distance": (C.c_int32, [C.c_void_p, C.POINTER(Params), C.c_uint64] + [C.c_void_p] * 5),
    "scrg_ctx_set_text_strands": (C.c_int32, [C.c_void_p, C.c_int]),
    "scrg_ctx_get_text_strands": (C.c_int32, [C.c_void_p, C.POINTER(C.c_int)]),
    "scrg_text_window_planes": (C.c_int32, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int32, C.c_uint64] + [C.c_void_p] * 4),
    "scrg_align_mapping_directed": (C.c_int32, [C.c_void_p, C.POINTER(Params), C.c_uint64] + [C.c_void_p] * 6 + [C.POINTER(C.POINTER(Result))]),
    "scrg_align_mapping_anchored": (C.c_int32, [C.c_void_p, C.POINTER(Params), C.c_uint64] + [C.c_void_p] * 7 + [C.POINTER(C.POINTER(Result))]),
    "scrg_join_anchored_runs": (C.c_int32, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "scrg_ctx_set_diff": (C.c_int32, [C.c_void_p, C.c_int32]),
    "scrg_ctx_get_diff": (C.c_int32, [C.c_void_p, C.POINTER(C.c_int32)]),
    "scrg_ctx_take_diff": (C.c_int32, [C.c_void_p, C.POINTER(C.POINTER(Diff))]),
    "scrg_diff_free": (None, [C.POINTER(Diff)]),
    "scrg_diff_lengths": (C.c_int32, [C.c_void_p, C.POINTER(Params), C.c_int32, C.c_uint64] + [C.c_void_p] * 4 + [C.c_uint64] + [C.c_void_p] * 2),
    "scrg_diff_render": (C.c_int32, [C.c_void_p, C.POINTER(Params), C.c_int32, C.c_uint64] + [C.c_void_p] * 4 + [C.c_uint64] + [C.c_void_p] * 4 +
                         [C.c_uint64, C.c_void_p]),
    "scrg_diff_from_runs": (C.c_int32, [C.c_int32, C.c_char_p, C.c_uint64, C.c_char_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64,
                                        C.POINTER(C.c_uint64)]),
    "scrg_report_device": (C.c_int32, [C.c_void_p, C.POINTER(Params), C.c_uint64] + [C.c_void_p] * 4 + [C.c_uint64] + [C.c_void_p] * 5),
    "scrg_report_from_runs": (C.c_int32, [C.c_char_p, C.c_uint64, C.c_char_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_int64, C.c_void_p]),
    "scrg_report_score": (C.c_int32, [C.c_void_p] + [C.c_int64] * 4 + [C.POINTER(C.c_int64)]),
    "scrg_ctx_set_report": (C.c_int32, [C.c_void_p, C.c_int]),
    "scrg_ctx_get_report": (C.c_int32, [C.c_void_p, C.POINTER(C.c_int)]),
    "scrg_ctx_take_report": (C.c_int32, [C.c_void_p, C.c_void_p]),
    "scrg_report_free": (None, [C.c_void_p]),
    "scrg_ctx_set_cigar_form": (C.c_int32, [C.c_void_p, C.c_int32]),
    "scrg_ctx_get_cigar_form": (C.c_int32, [C.c_void_p, C.POINTER(C.c_int32)]),
    "scrg_cigar_text_lengths": (C.c_int32, [C.c_void_p, C.c_int32, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]),
    "scrg_cigar_text_render": (C.c_int32, [C.c_void_p, C.c_int32, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64] + [C.c_void_p] * 4 +
                               [C.c_uint64, C.c_void_p]),
    "scrg_cigar_from_runs": (C.c_int32, [C.c_int32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]),
    "scrg_ctx_set_clip": (C.c_int32, [C.c_void_p, C.c_int, C.POINTER(C.c_int32)]),
    "scrg_ctx_get_clip": (C.c_int32, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int32)]),
    "scrg_ctx_take_clip": (C.c_int32, [C.c_void_p, C.c_void_p]),
    "scrg_clip_free": (None, [C.c_void_p]),
    "scrg_clip_device": (C.c_int32, [C.c_void_p, C.POINTER(Params), C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p,
                                     C.POINTER(C.c_int32), C.c_int, C.c_void_p]),
    "scrg_clip_from_runs": (C.c_int32, [C.c_void_p, C.c_uint64, C.POINTER(C.c_int32), C.c_void_p]),
    "scrg_ctx_set_pileup": (C.c_int32, [C.c_void_p, C.c_int]),
    "scrg_ctx_get_pileup": (C.c_int32, [C.c_void_p, C.POINTER(C.c_int)]),
    "scrg_ctx_take_pileup": (C.c_int32, [C.c_void_p, C.c_void_p]),
    "scrg_pileup_free": (None, [C.c_void_p]),
    "scrg_pileup_add": (C.c_int32, [C.c_void_p, C.POINTER(Params), C.c_uint64] + [C.c_void_p] * 4 + [C.c_uint64] + [C.c_void_p] * 3 +
                        [C.c_uint64, C.c_void_p, C.c_void_p]),
    "scrg_pileup_finish": (C.c_int32, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]),
    "scrg_pileup_from_runs": (C.c_int32, [C.c_void_p, C.c_uint64, C.c_char_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p, C.POINTER(C.c_uint64)]),
    "scrg_ctx_take_pileup_sites": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "scrg_pileup_sites_free": (None, [C.c_void_p]),
    "scrg_pileup_sites_scratch_bytes": (C.c_size_t, [C.c_uint64]),
    "scrg_pileup_sites_mark": (C.c_int32, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "scrg_pileup_sites_write": (C.c_int32, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p]),
    "scrg_pileup_sites_from_counts": (C.c_int32, [C.c_void_p, C.c_uint64, C.c_char_p, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]),
    "scrg_select_mates": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_uint64] + [C.c_void_p] * 9),
    "scrg_select_mates_team": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64] + [C.c_void_p] * 9),
    "scrg_align_mapping_paired": (C.c_int32, [C.c_void_p, C.POINTER(Params), C.c_uint64] + [C.c_void_p] * 6 + [C.c_void_p, C.POINTER(C.POINTER(Result))]),
    "scrg_mates_free": (None, [C.c_void_p]),
    "scrg_host_plan_mates": (C.c_int32, [C.POINTER(Params), C.c_int32, C.c_uint64] + [C.c_void_p] * 4 + [C.c_uint64, C.POINTER(C.c_uint64)]),
    "scrg_mates_from_distances": (C.c_int32, [C.c_void_p] + ([C.c_uint64] + [C.c_void_p] * 4 + [C.c_uint64]) * 2 + [C.c_void_p] * 3),
    "scrg_read_summary": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64] + [C.c_void_p] * 6),
    "scrg_ctx_set_read_summary": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_int]),
    "scrg_ctx_get_read_summary": (C.c_int32, [C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]),
    "scrg_ctx_take_read_summary": (C.c_int32, [C.c_void_p, C.c_void_p]),
    "scrg_read_summaries_free": (None, [C.c_void_p]),
    "scrg_read_summary_from_distances": (C.c_int32, [C.c_void_p, C.c_uint64] + [C.c_void_p] * 6),
    "scrg_read_summary_merge": (C.c_int32, [C.c_void_p] * 3),
    "scrg_seed_rule_default": (None, [C.c_void_p]),
    "scrg_seed_rule_check": (C.c_int32, [C.c_void_p, C.c_uint64]),
    "scrg_genome_index": (C.c_int32, [C.c_void_p, C.c_void_p]),
    "scrg_genome_index_clear": (None, [C.c_void_p]),
    "scrg_genome_index_info": (C.c_int32, [C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "scrg_find_candidates": (C.c_int32, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "scrg_candidates_free": (None, [C.c_void_p]),
    "scrg_candidates_from_genome": (C.c_int32, [C.c_void_p, C.c_char_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "scrg_ctx_set_seed_sampling": (C.c_int32, [C.c_void_p, C.c_uint32]),
    "scrg_seed_sampling_info": (C.c_int32, [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "scrg_seed_key_selected": (C.c_int, [C.c_uint32, C.c_uint32, C.c_uint32]),
    "scrg_candidates_from_genome_sampled": (C.c_int32, [C.c_void_p, C.c_uint32, C.c_char_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p,
                                                        C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
}


def _lazy(lib, name):
    fn = getattr(lib, name, None)
    if fn is None:
        raise ScroogeError(SCRG_ERR_INVALID_ARG, "this library has no %s (built before that entry point existed)" % name)
    if fn.argtypes is None:
        fn.restype, fn.argtypes = _LAZY_SIGS[name]
    return fn


def best_per_read(edit_distance, pair_status, cand_offsets):
    """Per read of a mapping result (best-candidate mode or not), in numpy on the host: the rule of SCRG_OUT_BEST.
    Eligible pairs are those whose status is not SCRG_PAIR_OVER_EDIT_LIMIT.  -> dict of int64 arrays, one entry per read:
    best_pair (global pair index of the eligible pair with the smallest edit distance, ties to the lowest index; -1: none),
    best_ed (its edit distance, -1), n_tied (eligible pairs at that distance, 0), second_ed (the smallest eligible distance
    above it, -1: none)."""
    import numpy as np
    ed = np.asarray(edit_distance, dtype=np.int64)
    st = np.asarray(pair_status)
    co = np.asarray(cand_offsets, dtype=np.int64)
    nr = len(co) - 1
    out = {k: np.full(nr, -1, dtype=np.int64) for k in ("best_pair", "best_ed", "second_ed")}
    out["n_tied"] = np.zeros(nr, dtype=np.int64)
    n = len(ed)
    if n == 0 or nr == 0:
        return out
    read = np.repeat(np.arange(nr, dtype=np.int64), np.diff(co))
    big = np.iinfo(np.int64).max
    key = np.where(st != SCRG_PAIR_OVER_EDIT_LIMIT, ed, big)
    has = np.diff(co) > 0
    starts = co[:-1][has]                                    # (reduceat wants the non-empty groups only)
    best = np.full(nr, big, dtype=np.int64)
    best[has] = np.minimum.reduceat(key, starts)
    at_best = (key == best[read]) & (key != big)
    idx = np.where(at_best, np.arange(n, dtype=np.int64), big)
    first = np.full(nr, big, dtype=np.int64)
    first[has] = np.minimum.reduceat(idx, starts)
    tied = np.zeros(nr, dtype=np.int64)
    tied[has] = np.add.reduceat(at_best.astype(np.int64), starts)
    above = np.where((key > best[read]) & (key != big), key, big)
    second = np.full(nr, big, dtype=np.int64)
    second[has] = np.minimum.reduceat(above, starts)
    won = best != big
    out["best_pair"][won] = first[won]
    out["best_ed"][won] = best[won]
    out["n_tied"] = tied
    out["second_ed"][second != big] = second[second != big]
    return out


def host_plan_mapping(read_lens, cand_offsets, n_devices=1, **params):
    """scrg_host_plan_mapping (no GPU): the issue order and the chunk cuts of a mapping call with these read lengths and
    candidate counts; best=True: the cuts of best-candidate mode, which fall between reads.  -> (order, chunk_first)."""
    import numpy as np
    lib = load_library()
    p = Params()
    lib.scrg_params_default(C.byref(p))
    best = params.pop("best", False)
    distance_only = params.pop("distance_only", False)
    for k, v in params.items():
        setattr(p, k, int(v))
    if best:
        p.outputs |= SCRG_OUT_BEST
    if distance_only:                   # (the cuts are those of the call without the flag)
        p.outputs = (p.outputs & SCRG_OUT_BEST) | SCRG_OUT_DISTANCE
    rl = np.ascontiguousarray(read_lens, dtype=np.uint64)
    co = np.ascontiguousarray(cand_offsets, dtype=np.uint64)
    nr = len(rl)
    assert co.shape == (nr + 1,)
    n = int(co[nr])
    order = np.zeros(max(n, 1), dtype=np.uint32)
    cap = n // 64 + 1024
    first = np.zeros(cap, dtype=np.uint64)
    nc = C.c_uint64(0)
    st = _lazy(lib, "scrg_host_plan_mapping")(C.byref(p), int(n_devices), nr, rl.ctypes.data, co.ctypes.data, order.ctypes.data,
                                              first.ctypes.data, cap, C.byref(nc))
    if st != SCRG_OK:
        raise ScroogeError(st, "scrg_host_plan_mapping: %s" % lib.scrg_status_string(st).decode())
    return order[:n], first[:nc.value + 1]


def host_plan_mates(read_lens, cand_offsets, n_devices=1, **params):
    """scrg_host_plan_mates (no GPU): the issue order and the chunk cuts of a paired call (Aligner.align_mapping_paired) with these
    read lengths and candidate counts — mate pairs sorted as one, no cut inside one.  -> (order, chunk_first)."""
    import numpy as np
    lib = load_library()
    p = Params()
    lib.scrg_params_default(C.byref(p))
    for k, v in params.items():
        setattr(p, k, int(v))
    rl = np.ascontiguousarray(read_lens, dtype=np.uint64)
    co = np.ascontiguousarray(cand_offsets, dtype=np.uint64)
    nr = len(rl)
    assert co.shape == (nr + 1,)
    n = int(co[nr])
    order = np.zeros(max(n, 1), dtype=np.uint32)
    cap = n // 64 + 1024
    first = np.zeros(cap, dtype=np.uint64)
    nc = C.c_uint64(0)
    st = _lazy(lib, "scrg_host_plan_mates")(C.byref(p), int(n_devices), nr, rl.ctypes.data, co.ctypes.data, order.ctypes.data,
                                            first.ctypes.data, cap, C.byref(nc))
    if st != SCRG_OK:
        raise ScroogeError(st, "scrg_host_plan_mates: %s" % lib.scrg_status_string(st).decode())
    return order[:n], first[:nc.value + 1]


def _limit_args(max_edits, per_mille):
    """Python's None (off) -> the C encoding: max_edits -1, per_mille 0."""
    return (-1 if max_edits is None else int(max_edits)), (0 if per_mille is None else int(per_mille))


def edit_limit_for(read_len, max_edits=None, per_mille=None):
    """The edit limit the kernels apply to a pair with this read length (scrg_edit_limit_for, no GPU):
    min(max_edits, floor(per_mille * read_len / 1000)), a part that is None dropping out; None = no limit."""
    lib = load_library()
    me, pm = _limit_args(max_edits, per_mille)
    out = C.c_int64(0)
    st = _lazy(lib, "scrg_edit_limit_for")(me, pm, int(read_len), C.byref(out))
    if st != SCRG_OK:
        raise ScroogeError(st, "invalid edit limit (max_edits=%r, per_mille=%r)" % (max_edits, per_mille))
    return None if out.value < 0 else int(out.value)


def _parse_cigar(cigar):
    """"12=1X3I" -> [(12, "="), (1, "X"), (3, "I")] (run counts are at most 255)."""
    cigar = cigar.decode() if isinstance(cigar, bytes) else cigar
    runs, k = [], 0
    while k < len(cigar):
        e = k
        while e < len(cigar) and cigar[e].isdigit():
            e += 1
        if e == k or e == len(cigar) or not 0 < int(cigar[k:e]) < 256 or cigar[e] not in "=XID":
            raise ScroogeError(SCRG_ERR_INVALID_ARG, "not a CIGAR of runs of at most 255 of = X I D: %r" % cigar)
        runs.append((int(cigar[k:e]), cigar[e]))
        k = e + 1
    return runs


def join_anchored(left, right, capacity=None):
    """scrg_join_anchored_runs on the host (no GPU, no handle): the CIGAR of an anchored pair from its halves — `left` as the
    leftward alignment produced it (from the anchor outwards), `right` as the rightward one did; CIGAR strings or lists of
    (count, op).  Returns (cigar, runs, left_text): the left half's runs in reversed order, then the right half's, nothing merged
    at the seam; left_text = the text characters the left half consumed (text_start = anchor - left_text).  capacity: the
    output array's size in runs (default: what is needed); too small raises ScroogeError(SCRG_ERR_CIGAR_OVERFLOW), whose
    `needed` attribute is the number of runs."""
    lib = load_library()
    lr = _parse_cigar(left) if isinstance(left, (str, bytes)) else [(int(c), o) for c, o in left]
    rr = _parse_cigar(right) if isinstance(right, (str, bytes)) else [(int(c), o) for c, o in right]

    def arr(runs):
        a = (Run * max(len(runs), 1))()
        for k, (c, o) in enumerate(runs):
            a[k].count, a[k].op = c, (o.encode() if isinstance(o, str) else o)
        return a
    la, ra = arr(lr), arr(rr)
    cap = len(lr) + len(rr) if capacity is None else int(capacity)
    out = (Run * max(cap, 1))()
    n, lt = C.c_uint64(0), C.c_uint64(0)
    st = _lazy(lib, "scrg_join_anchored_runs")(C.cast(la, C.c_void_p), len(lr), C.cast(ra, C.c_void_p), len(rr),
                                               C.cast(out, C.c_void_p) if cap else None, cap, C.byref(n), C.byref(lt))
    if st != SCRG_OK:
        e = ScroogeError(st, lib.scrg_status_string(st).decode())
        e.needed = int(n.value)
        raise e
    runs = [(int(out[k].count), out[k].op.decode()) for k in range(int(n.value))]
    return "".join("%d%s" % r for r in runs), runs, int(lt.value)


def diff_from_runs(kind, text, read, runs):
    """scrg_diff_from_runs: the difference string ("md" or "cs") of one pair on the host, no GPU — text and read (the read as
    aligned) as bytes or str, runs as a CIGAR string ("4=1X2=") or a list of (count, op).  ScroogeError for runs that consume more
    than the sequences hold."""
    text = text.encode() if isinstance(text, str) else bytes(text)
    read = read.encode() if isinstance(read, str) else bytes(read)
    runs = _parse_cigar(runs) if isinstance(runs, str) else list(runs)
    arr = (Run * max(len(runs), 1))()
    for k, (count, op) in enumerate(runs):
        arr[k].count = int(count)
        arr[k].op = op.encode() if isinstance(op, str) else bytes(op)
    fn = _lazy(load_library(), "scrg_diff_from_runs")
    need = C.c_uint64(0)
    st = fn(_diff_kind(kind), text, len(text), read, len(read), C.cast(arr, C.c_void_p), len(runs), None, 0, C.byref(need))
    if st != SCRG_OK:
        raise ScroogeError(st, "runs that are no alignment of these sequences")
    buf = C.create_string_buffer(int(need.value))
    st = fn(_diff_kind(kind), text, len(text), read, len(read), C.cast(arr, C.c_void_p), len(runs), buf, len(buf), C.byref(need))
    if st != SCRG_OK:
        raise ScroogeError(st, "scrg_diff_from_runs")
    return buf.value.decode()


def cigar_from_runs(form, runs):
    """scrg_cigar_from_runs: the CIGAR text of one pair's runs in a form ("windowed", "merged" or "m") on the host, no GPU —
    runs as a CIGAR string ("29=21=") or a list of (count, op).  ScroogeError for a zero count or an operation other than = X I D."""
    runs = _parse_cigar(runs) if isinstance(runs, str) else list(runs)
    arr = (Run * max(len(runs), 1))()
    for k, (count, op) in enumerate(runs):
        arr[k].count = int(count)
        arr[k].op = op.encode() if isinstance(op, str) else bytes(op)
    fn = _lazy(load_library(), "scrg_cigar_from_runs")
    need = C.c_uint64(0)
    st = fn(_cigar_form(form), C.cast(arr, C.c_void_p), len(runs), None, 0, C.byref(need))
    if st != SCRG_OK:
        raise ScroogeError(st, "runs with a zero count or an operation other than = X I D")
    buf = C.create_string_buffer(int(need.value))
    st = fn(_cigar_form(form), C.cast(arr, C.c_void_p), len(runs), buf, len(buf), C.byref(need))
    if st != SCRG_OK:
        raise ScroogeError(st, "scrg_cigar_from_runs")
    return buf.value.decode()


REPORT_FIELDS = ("n_match", "n_mismatch", "n_ins", "n_del", "n_gap_open", "n_indel", "verdict", "bad_run")     # scrg_pair_report
REPORT_PER_BASE = 16384           # scrg_params.reserved[0] of the test build (genasm_kernels.h: SCRG_SWITCH_REPORT_PER_BASE)
REPORT_NO_ALIGNMENT = 7           # include/scrooge_amd.h: SCRG_REPORT_NO_ALIGNMENT
REPORT_DEFAULT_COSTS = (2, 4, 4, 2)      # match, mismatch, gap open, gap extend: the reference baseline's default


class PairReport(C.Structure):
    """scrg_pair_report (include/scrooge_amd.h, ALIGNMENT REPORT): 32 bytes."""
    _fields_ = [(f, C.c_uint32) for f in REPORT_FIELDS]


class Report(C.Structure):
    """scrg_report: the alignment report of a host call, as Aligner.take_report gets it."""
    _fields_ = [("n_pairs", C.c_uint64), ("pairs", C.POINTER(PairReport)), ("n_failed", C.c_uint64)]


def report_dtype():
    """The numpy structured dtype of scrg_pair_report."""
    import numpy as np
    return np.dtype([(f, np.uint32) for f in REPORT_FIELDS])


def report_from_runs(text, read, runs, edit_distance):
    """scrg_report_from_runs: the alignment report of one pair on the host, no GPU — text and read (both as aligned) as bytes or
    str, runs as a CIGAR string or a list of (count, op) (any count 0..255, any op byte: a finding, not an error).  -> a dict
    with REPORT_FIELDS."""
    text = text.encode() if isinstance(text, str) else bytes(text)
    read = read.encode() if isinstance(read, str) else bytes(read)
    runs = _parse_cigar(runs) if isinstance(runs, str) else list(runs)
    arr = (Run * max(len(runs), 1))()
    for k, (count, op) in enumerate(runs):
        arr[k].count = int(count)
        arr[k].op = op.encode("latin-1") if isinstance(op, str) else bytes(op)
    out = PairReport()
    st = _lazy(load_library(), "scrg_report_from_runs")(text, len(text), read, len(read), C.cast(arr, C.c_void_p), len(runs), int(edit_distance),
                                                        C.byref(out))
    if st != SCRG_OK:
        raise ScroogeError(st, "scrg_report_from_runs")
    return {f: int(getattr(out, f)) for f in REPORT_FIELDS}


CLIP_FIELDS = ("read_start", "read_end", "text_start", "text_end", "first_run", "n_runs", "score", "n_edits")     # scrg_pair_clip
CLIP_DEFAULT_COSTS = (2, 4, 4, 2)        # match, mismatch, gap open, gap extend


class PairClip(C.Structure):
    """scrg_pair_clip (include/scrooge_amd.h, SOFT CLIPPING): 32 bytes."""
    _fields_ = [(f, C.c_int32 if f == "score" else C.c_uint32) for f in CLIP_FIELDS]


class Clip(C.Structure):
    """scrg_clip: the clip records of a host call, as Aligner.take_clip gets them."""
    _fields_ = [("n_pairs", C.c_uint64), ("pairs", C.POINTER(PairClip)), ("costs", C.c_int32 * 4)]


def clip_dtype():
    """The numpy structured dtype of scrg_pair_clip."""
    import numpy as np
    return np.dtype([(f, np.int32 if f == "score" else np.uint32) for f in CLIP_FIELDS])


def _clip_costs(costs):
    return None if costs is None else (C.c_int32 * 4)(*[int(x) for x in costs])


def clip_from_runs(runs, costs=None):
    """scrg_clip_from_runs: the best-scoring stretch of one pair's runs on the host, no GPU — runs as a CIGAR string or a list of
    (count, op) (any count 0..255, any op byte: such a list is not looked at, all zeros).  costs = (match, mismatch, gap open,
    gap extend), default 2, 4, 4, 2.  -> a dict with CLIP_FIELDS."""
    runs = _parse_cigar(runs) if isinstance(runs, str) else list(runs)
    arr = (Run * max(len(runs), 1))()
    for k, (count, op) in enumerate(runs):
        arr[k].count = int(count)
        arr[k].op = op.encode("latin-1") if isinstance(op, str) else bytes(op)
    out = PairClip()
    st = _lazy(load_library(), "scrg_clip_from_runs")(C.cast(arr, C.c_void_p), len(runs), _clip_costs(costs), C.byref(out))
    if st != SCRG_OK:
        raise ScroogeError(st, "scrg_clip_from_runs")
    return {f: int(getattr(out, f)) for f in CLIP_FIELDS}


# the planes of a pileup (include/scrooge_amd.h, PILEUP): counts[plane][position], target_len + 1 positions per plane
SCRG_PILE_MATCH, SCRG_PILE_A, SCRG_PILE_C, SCRG_PILE_G, SCRG_PILE_T, SCRG_PILE_DEL, SCRG_PILE_INS = range(7)
SCRG_PILE_PLANES = 7


class Pileup(C.Structure):
    """scrg_pileup: the counts of a handle's accumulator, as Aligner.take_pileup gets them."""
    _fields_ = [("target_len", C.c_uint64), ("n_alignments", C.c_uint64), ("n_out_of_range", C.c_uint64), ("counts", C.POINTER(C.c_uint32))]


def pileup_from_runs(runs, read_aligned, target_start, target_len, counts=None):
    """scrg_pileup_from_runs: one alignment added to a pileup on the host, no GPU — runs as a CIGAR string or a list of
    (count, op); read_aligned: the read as it was aligned (bytes or str: of a reverse-strand candidate the reverse complement);
    counts: a C-contiguous (7, target_len + 1) uint32 array to add to (None: a new one of zeros).  -> (counts, out_of_range: did a
    column or an insertion lie outside the target).  ScroogeError, nothing added: a run that is no run, a read shorter than the
    runs consume, a base under X other than ACGTacgt."""
    import numpy as np
    runs = _parse_cigar(runs) if isinstance(runs, str) else list(runs)
    arr = (Run * max(len(runs), 1))()
    for k, (count, op) in enumerate(runs):
        arr[k].count = int(count)
        arr[k].op = op.encode("latin-1") if isinstance(op, str) else bytes(op)
    read = read_aligned.encode("latin-1") if isinstance(read_aligned, str) else bytes(read_aligned)
    if counts is None:
        counts = np.zeros((SCRG_PILE_PLANES, int(target_len) + 1), dtype=np.uint32)
    if counts.dtype != np.uint32 or counts.shape != (SCRG_PILE_PLANES, int(target_len) + 1) or not counts.flags["C_CONTIGUOUS"]:
        raise ScroogeError(SCRG_ERR_INVALID_ARG, "counts: a C-contiguous (7, target_len + 1) uint32 array")
    outside = C.c_uint64(0)
    st = _lazy(load_library(), "scrg_pileup_from_runs")(C.cast(arr, C.c_void_p), len(runs), read, len(read), int(target_start), int(target_len),
                                                        C.c_void_p(counts.ctypes.data), C.byref(outside))
    if st != SCRG_OK:
        raise ScroogeError(st, "scrg_pileup_from_runs")
    return counts, bool(outside.value)


# the sites of a pileup (include/scrooge_amd.h, PILEUP SITES): allele codes 0..3 = A C G T, and the flag bits
SCRG_SITE_DEL, SCRG_SITE_NONE = 4, 255
SCRG_SITE_F_NONREF, SCRG_SITE_F_INS, SCRG_SITE_F_CALL = 1, 2, 4


class SiteRule(C.Structure):
    """scrg_site_rule"""
    _fields_ = [("min_depth", C.c_uint32), ("min_alt", C.c_uint32), ("min_alt_per_mille", C.c_uint32), ("reserved", C.c_uint32)]


class PileupSites(C.Structure):
    """scrg_pileup_sites: the sites of a handle's accumulator, as Aligner.take_pileup_sites gets them (also what
    io.Job.write_sites hands to the writer)."""
    _fields_ = [("target_len", C.c_uint64), ("n_alignments", C.c_uint64), ("n_out_of_range", C.c_uint64), ("n_sites", C.c_uint64),
                ("rule", SiteRule), ("sites", C.c_void_p)]


def site_dtype():
    """scrg_site as a numpy structured dtype: 40 bytes — pos, counts[7] (SCRG_PILE_*), ref, alt, call, flags."""
    import numpy as np
    return np.dtype([("pos", np.uint64), ("counts", np.uint32, (7,)), ("ref", np.uint8), ("alt", np.uint8), ("call", np.uint8), ("flags", np.uint8)])


def _site_rule(min_depth, min_alt, min_alt_per_mille, reserved=0):
    vals = [int(min_depth), int(min_alt), int(min_alt_per_mille), int(reserved)]
    if any(v < 0 or v > 0xffffffff for v in vals):
        raise ScroogeError(SCRG_ERR_INVALID_ARG, "site rule: min_depth, min_alt and min_alt_per_mille are 32-bit counts")
    return SiteRule(*vals)


def pileup_sites_from_counts(counts, genome, min_depth=1, min_alt=1, min_alt_per_mille=0, cap=None):
    """scrg_pileup_sites_from_counts: the sites of a pileup on the host, no GPU, by the rule of include/scrooge_amd.h (PILEUP
    SITES).  counts: a (7, target_len + 1) uint32 array in counts form (Aligner.take_pileup's "counts"); genome: the target's
    target_len bases (bytes or str, either case).  -> a structured array (site_dtype()) in ascending pos.  cap=None: count first
    (the call with out = NULL), then fill; a number: room for that many records.  ScroogeError: a rule that is refused, a base
    outside ACGTacgt (SCRG_ERR_BAD_BASE), cap below the number of sites (SCRG_ERR_CIGAR_OVERFLOW)."""
    import numpy as np
    counts = np.ascontiguousarray(counts, dtype=np.uint32)
    genome = genome.encode("latin-1") if isinstance(genome, str) else bytes(genome)
    if counts.ndim != 2 or counts.shape != (SCRG_PILE_PLANES, len(genome) + 1):
        raise ScroogeError(SCRG_ERR_INVALID_ARG, "counts: a (7, len(genome) + 1) uint32 array")
    rule = _site_rule(min_depth, min_alt, min_alt_per_mille)
    fn = _lazy(load_library(), "scrg_pileup_sites_from_counts")
    n = C.c_uint64(0)

    def call(out, room):
        st = fn(C.c_void_p(counts.ctypes.data), len(genome), genome, C.byref(rule), out, room, C.byref(n))
        if st != SCRG_OK:
            raise ScroogeError(st, "scrg_pileup_sites_from_counts")
        return int(n.value)

    if cap is None:
        cap = call(None, 0)
    out = np.zeros(int(cap), dtype=site_dtype())
    # (an empty array has no address worth passing: one spare record keeps `out` non-NULL, so that cap is honoured and not "count only")
    buf = out if len(out) else np.zeros(1, dtype=site_dtype())
    return out[:call(C.c_void_p(buf.ctypes.data), int(cap))]


# mate pairs (include/scrooge_amd.h, MATE PAIRS): the orientations a rule may ask for and the flag bits of a record
SCRG_MATES_FR, SCRG_MATES_RF, SCRG_MATES_FF, SCRG_MATES_ANY = 0, 1, 2, 3
SCRG_MATES_PROPER, SCRG_MATES_HAS_A, SCRG_MATES_HAS_B, SCRG_MATES_TIED = 1, 2, 4, 8
MATES_NONE = 0xffffffffffffffff         # a record's winner[] where a side has none
_MATE_ORIENTATIONS = {"fr": SCRG_MATES_FR, "rf": SCRG_MATES_RF, "ff": SCRG_MATES_FF, "any": SCRG_MATES_ANY}


class Mates(C.Structure):
    """scrg_mates"""
    _fields_ = [("n_mates", C.c_uint64), ("records", C.c_void_p)]


class _MateRuleC(C.Structure):
    """scrg_mate_rule"""
    _fields_ = [("min_span", C.c_uint64), ("max_span", C.c_uint64), ("orientation", C.c_uint32), ("unpaired_penalty", C.c_uint32),
                ("reserved", C.c_uint32 * 2)]


@dataclasses.dataclass
class MateRule:
    """scrg_mate_rule: inclusive bounds on a combination's span, the orientation ("fr", "rf", "ff", "any" or SCRG_MATES_*) and the
    edits a proper combination may cost more than the two single bests.  The default is the library's for rule = NULL."""
    min_span: int = 0
    max_span: int = 0xffffffffffffffff
    orientation: object = SCRG_MATES_FR
    unpaired_penalty: int = 0
    reserved: tuple = (0, 0)

    def as_c(self):
        o = self.orientation
        o = _MATE_ORIENTATIONS[o.lower()] if isinstance(o, str) else int(o)
        vals = [int(self.min_span), int(self.max_span), o, int(self.unpaired_penalty), int(self.reserved[0]), int(self.reserved[1])]
        if any(v < 0 for v in vals) or max(vals[:2]) > 0xffffffffffffffff or max(vals[2:]) > 0xffffffff:
            raise ScroogeError(SCRG_ERR_INVALID_ARG, "mate rule: spans are 64-bit, the other fields 32-bit counts")
        return _MateRuleC(vals[0], vals[1], vals[2], vals[3], (C.c_uint32 * 2)(vals[4], vals[5]))


def _mate_rule(rule):
    return None if rule is None else C.byref((rule if isinstance(rule, MateRule) else MateRule(*rule)).as_c())


def mate_dtype():
    """scrg_mate_record as a numpy structured dtype: 32 bytes — winner[2], cost, second_cost, span, n_proper, flags, reserved."""
    import numpy as np
    return np.dtype([("winner", np.uint64, (2,)), ("cost", np.uint32), ("second_cost", np.uint32), ("span", np.uint32),
                     ("n_proper", np.uint16), ("flags", np.uint8), ("reserved", np.uint8)])


def mates_from_distances(rule, side_a, side_b):
    """scrg_mates_from_distances: one mate pair's choice on the host, no GPU, by the rule of include/scrooge_amd.h (MATE PAIRS).
    side_a / side_b: (start, reverse or None, edit_distance, status or None, read_len) with one entry per candidate; statuses are a
    result's (SCRG_PAIR_OVER_EDIT_LIMIT: not eligible).  -> (record: a mate_dtype() scalar whose winner[] are indices within the
    sides, is_best_a, is_best_b: uint8 arrays)."""
    import numpy as np
    args, keep, marks = [], [], []
    for start, rev, ed, status, length in (side_a, side_b):
        st = np.ascontiguousarray(start, dtype=np.uint64)
        arrs = [st, None if rev is None else np.ascontiguousarray(rev, dtype=np.uint8), np.ascontiguousarray(ed, dtype=np.int64),
                None if status is None else np.ascontiguousarray(status, dtype=np.uint32)]
        if any(a is not None and a.shape != st.shape for a in arrs) or st.ndim != 1:
            raise ValueError("one entry per candidate expected")
        keep.append(arrs)
        marks.append(np.full(len(st) + 1, 9, dtype=np.uint8))
        # (an empty array has no address worth passing; the library looks at none of them then)
        args += [len(st)] + [None if a is None or not len(a) else C.c_void_p(a.ctypes.data) for a in arrs] + [int(length)]
    rec = np.zeros(1, dtype=mate_dtype())
    st = _lazy(load_library(), "scrg_mates_from_distances")(_mate_rule(rule), *args, C.c_void_p(rec.ctypes.data), C.c_void_p(marks[0].ctypes.data),
                                                            C.c_void_p(marks[1].ctypes.data))
    if st != SCRG_OK:
        raise ScroogeError(st, "scrg_mates_from_distances")
    return rec[0], marks[0][:-1], marks[1][:-1]


SCRG_MAPQ_HAS_WINNER, SCRG_MAPQ_TIED, SCRG_MAPQ_HAS_SECOND, SCRG_MAPQ_KEPT = 1, 2, 4, 8      # scrg_read_summary.flags
MAPQ_NONE = 0xffffffffffffffff          # scrg_read_summary.winner: no winner
MAPQ_NO_ED = 0xffffffff                 # best_ed / second_ed: none


class _MapqRuleC(C.Structure):
    """scrg_mapq_rule"""
    _fields_ = [("per_edit", C.c_uint32), ("max_q", C.c_uint32), ("zero_per_mille", C.c_uint16), ("min_keep_q", C.c_uint16), ("reserved", C.c_uint32)]


class ReadSummaries(C.Structure):
    """scrg_read_summaries"""
    _fields_ = [("n_reads", C.c_uint64), ("reads", C.c_void_p), ("rule", _MapqRuleC)]


@dataclasses.dataclass
class MapqRule:
    """scrg_mapq_rule (include/scrooge_amd.h, READ SUMMARY AND MAPPING QUALITY): MAPQ per edit between the best and the second
    distance, the largest MAPQ, the edit rate (per 1000 read bases) at which the cap reaches 0, and the MAPQ from which a read is
    KEPT (what the pileup then sums).  The defaults are the library's for rule = NULL: a heuristic, validated against no truth set."""
    per_edit: int = 10
    max_q: int = 60
    zero_per_mille: int = 250
    min_keep_q: int = 0
    reserved: int = 0

    def as_c(self):
        vals = [int(self.per_edit), int(self.max_q), int(self.zero_per_mille), int(self.min_keep_q), int(self.reserved)]
        if any(v < 0 for v in vals) or max(vals[0], vals[1], vals[4]) > 0xffffffff or max(vals[2:4]) > 0xffff:
            raise ScroogeError(SCRG_ERR_INVALID_ARG, "mapq rule: per_edit, max_q and reserved are 32-bit, zero_per_mille and min_keep_q 16-bit counts")
        return _MapqRuleC(*vals)


def _mapq_rule(rule):
    return None if rule is None else C.byref((rule if isinstance(rule, MapqRule) else MapqRule(*rule)).as_c())


def read_summary_dtype():
    """scrg_read_summary as a numpy structured dtype: 32 bytes — winner, best_ed, second_ed, n_tied, n_eligible, n_candidates, mapq,
    flags, reserved."""
    import numpy as np
    return np.dtype([("winner", np.uint64), ("best_ed", np.uint32), ("second_ed", np.uint32), ("n_tied", np.uint32), ("n_eligible", np.uint32),
                     ("n_candidates", np.uint32), ("mapq", np.uint8), ("flags", np.uint8), ("reserved", np.uint16)])


def read_summary_from_distances(rule, first, read_len, edit_distance, pair_status=None, keep=False):
    """scrg_read_summary_from_distances: every read's summary and MAPQ on the host, no GPU, by the rule of include/scrooge_amd.h
    (READ SUMMARY AND MAPPING QUALITY).  first: n_reads + 1 offsets of the reads' first pairs; read_len (the pair's read's length),
    edit_distance and pair_status (a result's: SCRG_PAIR_OVER_EDIT_LIMIT is not eligible; None: all eligible) per pair.
    -> records (read_summary_dtype(), winner as a pair index), or (records, keep_status) with keep=True."""
    import numpy as np
    fi = np.ascontiguousarray(first, dtype=np.uint64)
    rl = np.ascontiguousarray(read_len, dtype=np.uint32)
    ed = np.ascontiguousarray(edit_distance, dtype=np.int64)
    st = None if pair_status is None else np.ascontiguousarray(pair_status, dtype=np.uint32)
    if fi.ndim != 1 or len(fi) < 1 or rl.shape != ed.shape or ed.ndim != 1 or (st is not None and st.shape != ed.shape) or \
            (len(fi) > 1 and int(fi.max()) > len(ed)):
        raise ValueError("first: n_reads + 1 offsets into the per-pair arrays expected")
    nr = len(fi) - 1
    out = np.zeros(nr, dtype=read_summary_dtype())
    kept = np.zeros(len(ed) + 1, dtype=np.uint32) if keep else None
    ptr = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
    code = _lazy(load_library(), "scrg_read_summary_from_distances")(_mapq_rule(rule), nr, ptr(fi), ptr(rl), ptr(ed), ptr(st), ptr(out), ptr(kept))
    if code != SCRG_OK:
        raise ScroogeError(code, "scrg_read_summary_from_distances")
    return (out, kept[:-1]) if keep else out


def read_summary_merge(a, b):
    """scrg_read_summary_merge: the merge of two partial summaries (best = ed << 32 | index, n_tied, second_ed, n_eligible) of one
    read — the function the kernel's lanes call.  -> a tuple of four ints."""
    import numpy as np
    x, y, out = (np.array([int(v) for v in t], dtype=np.uint64) for t in (a, b, (0, 0, 0, 0)))
    code = _lazy(load_library(), "scrg_read_summary_merge")(C.c_void_p(x.ctypes.data), C.c_void_p(y.ctypes.data), C.c_void_p(out.ctypes.data))
    if code != SCRG_OK:
        raise ScroogeError(code, "scrg_read_summary_merge")
    return tuple(int(v) for v in out)


class _SeedRuleC(C.Structure):
    """scrg_seed_rule"""
    _fields_ = [(n, C.c_uint32) for n in ("k", "stride", "max_occ", "band", "min_hits", "max_candidates", "strands", "hit_budget_mb")]


class Candidates(C.Structure):
    """scrg_candidates"""
    _fields_ = [("n_reads", C.c_uint64), ("cand_offsets", C.POINTER(C.c_uint64)), ("cand_start", C.POINTER(C.c_uint64)),
                ("cand_reverse", C.POINTER(C.c_uint8)), ("cand_votes", C.POINTER(C.c_uint32)), ("n_hits", C.c_uint64), ("n_clusters", C.c_uint64),
                ("n_keys_over_max_occ", C.c_uint64), ("rule", _SeedRuleC)]


@dataclasses.dataclass
class SeedRule:
    """scrg_seed_rule (include/scrooge_amd.h, SEEDING): bases per k-mer, the stride of the indexed genome positions, the most
    index entries a key may have and still count, the largest gap between neighbouring diagonals of one cluster, the fewest hits
    of a candidate, the most candidates per read, the strands (1: forward, 3: both) and the device memory, in MB, for the hits
    of one chunk of reads (0: 256).  The defaults are the library's for rule = NULL."""
    k: int = 13
    stride: int = 4
    max_occ: int = 64
    band: int = 32
    min_hits: int = 2
    max_candidates: int = 4
    strands: int = 3
    hit_budget_mb: int = 0

    def as_c(self):
        vals = [int(v) for v in dataclasses.astuple(self)]
        if any(v < 0 or v > 0xffffffff for v in vals):
            raise ScroogeError(SCRG_ERR_INVALID_ARG, "seed rule: every field is a 32-bit count")
        return _SeedRuleC(*vals)


def _seed_rule(rule):
    return None if rule is None else C.byref((rule if isinstance(rule, SeedRule) else SeedRule(*rule)).as_c())


def seed_rule_check(rule, genome_len):
    """scrg_seed_rule_check: the status (SCRG_OK or SCRG_ERR_INVALID_ARG) of a rule and a genome length.  No GPU."""
    return int(_lazy(load_library(), "scrg_seed_rule_check")(_seed_rule(rule), int(genome_len)))


def _take_candidates(lib, cp):
    """A scrg_candidates as per-read lists and its counters; the record is freed."""
    try:
        c = cp.contents
        nr = int(c.n_reads)
        offs = [int(c.cand_offsets[i]) for i in range(nr + 1)]
        n = offs[-1]
        starts, rev, votes = ([int(a[i]) for i in range(n)] for a in (c.cand_start, c.cand_reverse, c.cand_votes))
        info = {"n_hits": int(c.n_hits), "n_clusters": int(c.n_clusters), "n_keys_over_max_occ": int(c.n_keys_over_max_occ),
                "rule": SeedRule(*[int(getattr(c.rule, f)) for f, _ in _SeedRuleC._fields_])}
    finally:
        _lazy(lib, "scrg_candidates_free")(cp)
    cut = lambda a: [a[offs[r]:offs[r + 1]] for r in range(nr)]
    return cut(starts), cut(rev), cut(votes), info


def seed_key_selected(key, k, smer):
    """scrg_seed_key_selected: does the sampling `smer` (0, or 3 .. k - 1) take the key of k bases?  No GPU."""
    return bool(_lazy(load_library(), "scrg_seed_key_selected")(int(key) & 0xffffffff, int(k), int(smer)))


def candidates_from_genome(rule, genome, reads, info=False, smer=0):
    """scrg_candidates_from_genome(_sampled): every read's candidates on the host, no GPU, by the rule of include/scrooge_amd.h
    (SEEDING) — the twin Aligner.find_candidates is held to.  smer: the sampling (Aligner.set_seed_sampling).  -> (candidates,
    reverse, votes), per-read lists; info=True: and a dict of the counters (n_hits, n_clusters, n_keys_over_max_occ, n_entries,
    n_lookups) and the rule."""
    genome = genome.encode() if isinstance(genome, str) else bytes(genome)
    reads = _bytes_list(reads)
    nr = len(reads)
    lib = load_library()
    rp = (C.c_char_p * max(nr, 1))(*reads)
    rl = (C.c_uint64 * max(nr, 1))(*[len(r) for r in reads])
    cp = C.POINTER(Candidates)()
    smer = int(smer)
    if smer < 0 or smer > 0xffffffff:
        raise ScroogeError(SCRG_ERR_INVALID_ARG, "seed sampling: smer is 0 or 3 .. k - 1")
    n_entries, n_lookups = C.c_uint64(), C.c_uint64()
    code = _lazy(lib, "scrg_candidates_from_genome_sampled")(_seed_rule(rule), smer, genome, len(genome), nr, C.cast(rp, C.c_void_p), C.cast(rl, C.c_void_p),
                                                             C.byref(cp), C.byref(n_entries), C.byref(n_lookups))
    if code != SCRG_OK:
        raise ScroogeError(code, "scrg_candidates_from_genome_sampled")
    out = _take_candidates(lib, cp)
    out[3].update(n_entries=int(n_entries.value), n_lookups=int(n_lookups.value))
    return out if info else out[:3]


def report_score(rep, costs=REPORT_DEFAULT_COSTS):
    """scrg_report_score, vectorised: match * n_match - mismatch * n_mismatch - open * n_gap_open - extend * (n_ins + n_del) of a
    report record (a dict), or of a structured array of them -> int / int64 array.  costs = (match, mismatch, open, extend).
    ScroogeError for a record whose counts do not cover its runs (a verdict other than 0, 6 and the 3 met after the last run)."""
    import numpy as np
    m, x, o, e = (int(c) for c in costs)
    if isinstance(rep, dict):
        r = PairReport(*[int(rep[f]) for f in REPORT_FIELDS])
        score = C.c_int64(0)
        st = _lazy(load_library(), "scrg_report_score")(C.byref(r), m, x, o, e, C.byref(score))
        if st != SCRG_OK:
            raise ScroogeError(st, "the record's counts do not cover its runs (verdict %d)" % r.verdict)
        return int(score.value)
    rep = np.asarray(rep)
    v = rep["verdict"]
    counted = (rep["n_match"] | rep["n_mismatch"] | rep["n_ins"] | rep["n_del"]) != 0
    bad = ~((v == 0) | (v == 6) | ((v == 3) & (counted | (rep["bad_run"] == 0))))
    if bad.any():
        raise ScroogeError(SCRG_ERR_INVALID_ARG, "%d records' counts do not cover their runs (the first: %d)" % (int(bad.sum()), int(np.argmax(bad))))
    i64 = np.int64
    return m * rep["n_match"].astype(i64) - x * rep["n_mismatch"].astype(i64) - o * rep["n_gap_open"].astype(i64) - \
        e * (rep["n_ins"].astype(i64) + rep["n_del"].astype(i64))


def text_window_planes(planar, text_off, text_len, ref_idx, W=64, stride=1):
    """scrg_text_window_planes (no GPU, no handle): the planes of the window of W characters at character ref_idx of the text
    (text_off — TEXT_REVCOMP honoured —, text_len) of a planar numpy uint64 array, through the address arithmetic the kernels
    use.  Returns (lo, hi, first_word, last_word): lists of (W + 63) // 64 words, and the lowest / highest word index read
    (None, None if no word was)."""
    import numpy as np
    lib = load_library()
    planar = np.ascontiguousarray(planar, dtype=np.uint64)
    nw = (int(W) + 63) // 64 if 1 <= int(W) <= 256 else 1
    lo, hi = (C.c_uint64 * nw)(), (C.c_uint64 * nw)()
    first, last = C.c_uint64(0), C.c_uint64(0)
    st = _lazy(lib, "scrg_text_window_planes")(planar.ctypes.data, planar.size, int(text_off), int(text_len), int(ref_idx), int(W), int(stride),
                                               C.cast(lo, C.c_void_p), C.cast(hi, C.c_void_p), C.cast(C.pointer(first), C.c_void_p),
                                               C.cast(C.pointer(last), C.c_void_p))
    if st != SCRG_OK:
        raise ScroogeError(st, lib.scrg_status_string(st).decode())
    none = first.value == 2 ** 64 - 1
    return list(lo), list(hi), (None if none else int(first.value)), (None if none else int(last.value))


def edit_stream_to_cigar(stream, read_len, W=64, O=33, lane_form=False):
    """Host-side decoder of ONE pair's edit stream (bytes, format version 2: window ends on the wire) -> the CIGAR text the
    aligner returns (scrg_edit_stream_to_runs: no GPU involved; it also holds the window ends to the window loop of W/O.
    lane_form=True: through the state machine the device decoder runs in every lane, scrg_edit_stream_to_runs_lane, which
    like the device does not look at the window geometry).  Raises ScroogeError for a malformed stream."""
    lib = load_library()
    fn = lib.scrg_edit_stream_to_runs_lane if lane_form else lib.scrg_edit_stream_to_runs
    p = Params()
    lib.scrg_params_default(C.byref(p))
    p.W, p.O = int(W), int(O)
    buf = (C.c_uint8 * max(1, len(stream))).from_buffer_copy(bytes(stream) or b"\0")
    n = C.c_uint64(0)
    st = fn(C.byref(p), int(read_len), buf, len(stream), None, 0, C.byref(n))
    if st not in (SCRG_OK, SCRG_ERR_CIGAR_OVERFLOW):
        raise ScroogeError(st, "malformed edit stream")
    runs = (C.c_uint8 * (2 * max(1, n.value)))()
    st = fn(C.byref(p), int(read_len), buf, len(stream), runs, n.value, C.byref(n))
    if st != SCRG_OK:
        raise ScroogeError(st, "malformed edit stream")
    return "".join("%d%s" % (runs[2 * k], chr(runs[2 * k + 1])) for k in range(n.value))


def cigar_to_edit_stream(cigar, W=64, O=33):
    """Host-side encoder: CIGAR text (=, X, I, D runs) -> canonical edit stream bytes (scrg_runs_to_edit_stream; the window
    loop of W/O places the window-end bytes)."""
    import re
    lib = load_library()
    p = Params()
    lib.scrg_params_default(C.byref(p))
    p.W, p.O = int(W), int(O)
    items = re.findall(r"(\d+)([=XID])", cigar)
    if "".join(a + b for a, b in items) != cigar:
        raise ValueError("not a CIGAR of =, X, I, D runs: %r" % cigar[:40])
    raw = bytearray()
    for cnt, op in items:
        c = int(cnt)
        while c > 0:                       # scrg_run counts are one byte
            raw += bytes((min(c, 255), ord(op)))
            c -= 255
    runs = (C.c_uint8 * max(1, len(raw))).from_buffer_copy(bytes(raw) or b"\0")
    n = C.c_uint64(0)
    lib.scrg_runs_to_edit_stream(C.byref(p), runs, len(raw) // 2, None, 0, C.byref(n))
    out = (C.c_uint8 * max(1, n.value))()
    st = lib.scrg_runs_to_edit_stream(C.byref(p), runs, len(raw) // 2, out, n.value, C.byref(n))
    if st != SCRG_OK:
        raise ScroogeError(st, "bad runs")
    return bytes(out[: n.value])


def create_stream(device=0, priority=0):
    """A raw HIP stream handle of the given priority (-1 high, 0 normal, 1 low); wrap it with
    torch.cuda.ExternalStream(handle) to use it from torch."""
    lib = load_library()
    h = C.c_void_p()
    st = lib.scrg_stream_create(int(device), int(priority), C.byref(h))
    if st != SCRG_OK:
        raise ScroogeError(st, lib.scrg_status_string(st).decode())
    return h.value


def _bytes_list(seqs):
    return [s.encode() if isinstance(s, str) else bytes(s) for s in seqs]


def _ptr(t):
    """device pointer of a torch tensor (or None)"""
    return None if t is None else C.c_void_p(t.data_ptr())


class Aligner:
    """One handle per GPU (scrg_ctx).

    ``align_pairs`` / ``align_mapping`` mirror the two overloads of
    genasm_gpu::align_all (src/genasm_gpu.hpp:7-8) and return a list of
    ``Alignment(cigar, edit_distance)`` in the reference's result order.
    """

    def __init__(self, device=0, variant=None, **params):
        self.lib = load_library(variant)
        h = C.c_void_p()
        st = self.lib.scrg_ctx_create(int(device), C.byref(h))
        if st != SCRG_OK:
            raise ScroogeError(st, self.lib.scrg_status_string(st).decode())
        self.h = h
        self.device = int(device)
        self.params = self.make_params(**params)
        self.last_timing = {}

    def make_params(self, **kw):
        p = Params()
        self.lib.scrg_params_default(C.byref(p))
        for k, v in kw.items():
            if not hasattr(p, k):
                raise TypeError("unknown parameter %r" % k)
            setattr(p, k, int(v))
        return p

    def close(self):
        if getattr(self, "h", None):
            self.lib.scrg_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, st, allow=()):
        if st != SCRG_OK and st not in allow:
            raise ScroogeError(st, (self.lib.scrg_last_error(self.h) or b"").decode() or
                               self.lib.scrg_status_string(st).decode())

    def _params(self, kw):
        """The handle's parameters with the call's keywords on top.  best=True (the mapping calls: align_mapping,
        align_mapping_rows, align_mapping_multi, io.Job.align) sets SCRG_OUT_BEST in `outputs`: of every read's candidates
        only the one with the fewest edits (ties: the first) keeps its CIGAR; the others come back with their edit distance,
        status SCRG_PAIR_NOT_BEST and "" (best_per_read() sums a result up per read).
        distance_only=True (every align call of the host layer) sets SCRG_OUT_DISTANCE: edit distance, status and text end
        of every pair and nothing else — the list form returns CIGAR "", the arrays form gains "text_end"."""
        if not kw:
            return self.params
        kw = dict(kw)
        best = kw.pop("best", None)
        distance_only = kw.pop("distance_only", None)
        p = Params()
        C.memmove(C.byref(p), C.byref(self.params), C.sizeof(Params))
        for k, v in kw.items():
            if not hasattr(p, k):
                raise TypeError("unknown parameter %r" % k)
            setattr(p, k, int(v))
        if best is not None:
            p.outputs = (p.outputs | SCRG_OUT_BEST) if best else (p.outputs & ~SCRG_OUT_BEST)
        if distance_only is not None:
            p.outputs = ((p.outputs & SCRG_OUT_BEST) | SCRG_OUT_DISTANCE) if distance_only else (p.outputs & ~SCRG_OUT_DISTANCE)
        return p

    def set_edit_limit(self, max_edits=None, per_mille=None):
        """The handle's edit limit (scrg_ctx_set_edit_limit) for every later align call on it: a pair whose running sum of
        edits exceeds min(max_edits, floor(per_mille * read_len / 1000)) at a window end is dropped there — status
        SCRG_PAIR_OVER_EDIT_LIMIT (device layer: 2), edit distance = that sum, no runs, CIGAR "".  None = that part off;
        set_edit_limit() with no arguments removes the limit.  per_mille: 1..1000."""
        me, pm = _limit_args(max_edits, per_mille)
        self._check(_lazy(self.lib, "scrg_ctx_set_edit_limit")(self.h, me, pm))

    def edit_limit(self):
        """(max_edits, per_mille) of the handle, None for a part that is off."""
        me, pm = C.c_int64(-1), C.c_int32(0)
        self._check(_lazy(self.lib, "scrg_ctx_get_edit_limit")(self.h, C.byref(me), C.byref(pm)))
        return (None if me.value < 0 else int(me.value)), (None if pm.value == 0 else int(pm.value))

    def set_text_strands(self, enabled=True):
        """The handle's text-strand setting (scrg_ctx_set_text_strands) for every later align call on it: enabled, bit 63 of a
        pair's text_off (TEXT_REVCOMP) means "align against the reverse complement of this stretch", taken from the text's one
        packed copy; the one-pair-per-lane kernels only (lanes_per_pair = 1, the default).  Off by default."""
        self._check(_lazy(self.lib, "scrg_ctx_set_text_strands")(self.h, 1 if enabled else 0))

    def text_strands(self):
        on = C.c_int(0)
        self._check(_lazy(self.lib, "scrg_ctx_get_text_strands")(self.h, C.byref(on)))
        return bool(on.value)

    def set_diff(self, kind=None):
        """The handle's difference-string kind (scrg_ctx_set_diff) for every later host align call on it: "md" (SAM's MD:Z:),
        "cs" (PAF's short cs:Z:) or None (off, the default).  With a kind set the call also renders every pair's string on the
        GPU and keeps them on the handle for take_diff()."""
        self._check(_lazy(self.lib, "scrg_ctx_set_diff")(self.h, _diff_kind(kind)))

    def diff(self):
        """The handle's difference-string kind: "md", "cs" or None."""
        k = C.c_int32(0)
        self._check(_lazy(self.lib, "scrg_ctx_get_diff")(self.h, C.byref(k)))
        return {DIFF_OFF: None, DIFF_MD: "md", DIFF_CS: "cs"}[k.value]

    def take_diff(self, arrays=False):
        """The difference strings of the last host align call (scrg_ctx_take_diff), in the pairs' order, ONCE: a list of str, or
        — arrays=True — (offset: uint64 [n + 1], text: bytes, every string NUL-terminated).  ScroogeError if there are none
        (no kind was set, the call failed, or they were taken already)."""
        d = C.POINTER(Diff)()
        self._check(_lazy(self.lib, "scrg_ctx_take_diff")(self.h, C.byref(d)))
        try:
            import numpy as np
            n = int(d.contents.n_pairs)
            off = np.ctypeslib.as_array(d.contents.offset, shape=(n + 1,)).copy()
            total = int(off[n])
            text = np.ctypeslib.as_array(C.cast(d.contents.text, C.POINTER(C.c_uint8)), shape=(total,)).tobytes() if total else b""
        finally:
            _lazy(self.lib, "scrg_diff_free")(d)
        if arrays:
            return off, text
        return [text[int(off[i]):int(off[i + 1]) - 1].decode() for i in range(n)]

    def set_cigar_form(self, form="windowed"):
        """The handle's form of the CIGAR text (scrg_ctx_set_cigar_form) for every later host align call on it: "windowed" (the
        default: the runs printed one by one, as the reference writes them), "merged" (adjacent equal operations merged: 29=21= ->
        50=) or "m" (merged, with = and X written M).  The runs of a result are the same in every form."""
        self._check(_lazy(self.lib, "scrg_ctx_set_cigar_form")(self.h, _cigar_form(form)))

    def cigar_form(self):
        """The handle's form of the CIGAR text: "windowed", "merged" or "m"."""
        f = C.c_int32(0)
        self._check(_lazy(self.lib, "scrg_ctx_get_cigar_form")(self.h, C.byref(f)))
        return {v: k for k, v in _CIGAR_FORMS.items()}[f.value]

    @contextlib.contextmanager
    def _call_form(self, form):
        """The per-call keyword cigar_form= of the host align methods, handled as diff= is: the form for this call only, the
        handle's own setting restored afterwards."""
        if form is None:
            yield
            return
        old = self.cigar_form()
        self.set_cigar_form(form)
        try:
            yield
        finally:
            self.set_cigar_form(old)

    def set_report(self, enabled=True):
        """The handle's report setting (scrg_ctx_set_report) for every later host align call on it: enabled, the call also makes
        every pair's alignment report on the GPU — counts per operation, gap openings, indel stretches and a verdict (is this an
        alignment of these sequences with this edit distance) — and keeps it on the handle for take_report().  Off by default."""
        self._check(_lazy(self.lib, "scrg_ctx_set_report")(self.h, 1 if enabled else 0))

    def report(self):
        on = C.c_int(0)
        self._check(_lazy(self.lib, "scrg_ctx_get_report")(self.h, C.byref(on)))
        return bool(on.value)

    def take_report(self):
        """The alignment report of the last host align call (scrg_ctx_take_report), in the pairs' order, ONCE: a numpy structured
        array with REPORT_FIELDS (a copy); `last_report_failed` = the pairs whose verdict is neither 0 nor REPORT_NO_ALIGNMENT.
        ScroogeError if there is none (the setting was off, the call failed, or it was taken already)."""
        import numpy as np
        r = C.POINTER(Report)()
        self._check(_lazy(self.lib, "scrg_ctx_take_report")(self.h, C.byref(r)))
        try:
            n = int(r.contents.n_pairs)
            self.last_report_failed = int(r.contents.n_failed)
            if n == 0:
                return np.zeros(0, dtype=report_dtype())
            raw = np.ctypeslib.as_array(C.cast(r.contents.pairs, C.POINTER(C.c_uint32)), shape=(n * len(REPORT_FIELDS),))
            return raw.copy().view(report_dtype())
        finally:
            _lazy(self.lib, "scrg_report_free")(r)

    @contextlib.contextmanager
    def _call_report(self, on):
        """The per-call keyword report= of the host align methods, handled as diff= is: the setting for this call only.  Yields a
        function that puts the call's records where they belong: "report" into the arrays form, `last_report` beside the list form."""
        if on is None:
            yield lambda out: out
            return
        old = self.report()
        self.set_report(bool(on))

        def deliver(out):
            if on:
                rep = self.take_report()
                if isinstance(out, dict):
                    out["report"] = rep
                else:
                    self.last_report = rep
            return out
        try:
            yield deliver
        finally:
            self.set_report(old)

    def set_clip(self, costs=None, enabled=True):
        """The handle's clip setting (scrg_ctx_set_clip) for every later host align call on it: enabled, every pair comes back
        as the stretch of its runs with the best affine score — runs, offsets and CIGAR text are those of the kept stretch, the
        edit distance stays the full alignment's — and the records (where the stretch lies, its score, its edits) are kept on the
        handle for take_clip().  costs = (match, mismatch, gap open, gap extend), default 2, 4, 4, 2.  Off by default."""
        self._check(_lazy(self.lib, "scrg_ctx_set_clip")(self.h, 1 if enabled else 0, _clip_costs(costs)))

    def clip(self):
        """-> (enabled, costs) of the handle's clip setting."""
        on, costs = C.c_int(0), (C.c_int32 * 4)()
        self._check(_lazy(self.lib, "scrg_ctx_get_clip")(self.h, C.byref(on), costs))
        return bool(on.value), tuple(costs)

    def take_clip(self):
        """The clip records of the last host align call (scrg_ctx_take_clip), in the pairs' order, ONCE: a numpy structured array
        with CLIP_FIELDS (a copy).  ScroogeError if there are none (the setting was off, the call failed, or they were taken)."""
        import numpy as np
        r = C.POINTER(Clip)()
        self._check(_lazy(self.lib, "scrg_ctx_take_clip")(self.h, C.byref(r)))
        try:
            n = int(r.contents.n_pairs)
            if n == 0:
                return np.zeros(0, dtype=clip_dtype())
            raw = np.ctypeslib.as_array(C.cast(r.contents.pairs, C.POINTER(C.c_uint32)), shape=(n * len(CLIP_FIELDS),))
            return raw.copy().view(clip_dtype())
        finally:
            _lazy(self.lib, "scrg_clip_free")(r)

    def set_mapq(self, rule=None, enabled=True):
        """The handle's read-summary setting (scrg_ctx_set_read_summary) for every later mapping call on it: enabled, a call in
        best-candidate mode (best=True) also makes every read's summary and MAPQ on the GPU, by `rule` (a MapqRule; None: the
        defaults), and keeps them for take_read_summary(); any other call is then refused.  With the pileup on and
        rule.min_keep_q > 0, only the winners of reads with that MAPQ pile up.  Off by default."""
        self._check(_lazy(self.lib, "scrg_ctx_set_read_summary")(self.h, _mapq_rule(rule), 1 if enabled else 0))

    def mapq(self):
        """-> (enabled, rule) of the handle's read-summary setting."""
        on, r = C.c_int(0), _MapqRuleC()
        self._check(_lazy(self.lib, "scrg_ctx_get_read_summary")(self.h, C.byref(r), C.byref(on)))
        return bool(on.value), MapqRule(r.per_edit, r.max_q, r.zero_per_mille, r.min_keep_q, r.reserved)

    def take_read_summary(self):
        """The read summaries of the last host align call (scrg_ctx_take_read_summary), in the reads' order, ONCE: a numpy
        structured array (read_summary_dtype(); a copy), winner as a pair index of the result (MAPQ_NONE: none).  ScroogeError if
        there are none (the setting was off, the call failed, or they were taken already)."""
        import numpy as np
        r = C.c_void_p()
        self._check(_lazy(self.lib, "scrg_ctx_take_read_summary")(self.h, C.byref(r)))
        try:
            m = C.cast(r, C.POINTER(ReadSummaries)).contents
            out = np.zeros(int(m.n_reads), dtype=read_summary_dtype())
            if m.n_reads:
                C.memmove(out.ctypes.data, m.reads, 32 * int(m.n_reads))
            return out
        finally:
            _lazy(self.lib, "scrg_read_summaries_free")(r)

    @contextlib.contextmanager
    def _call_mapq(self, mapq):
        """The per-call keyword mapq= of the mapping methods (True, or a MapqRule), handled as report= is: the setting for this call
        only.  It implies nothing: without best=True the library refuses the call.  Yields a function that puts the call's records
        where they belong: "read_summary" into the arrays form, `last_read_summary` beside the list form."""
        if mapq is None:
            yield lambda out: out
            return
        old_on, old_rule = self.mapq()
        on = mapq is not False
        self.set_mapq(None if mapq in (True, False) else mapq, on)

        def deliver(out):
            if on:
                rec = self.take_read_summary()
                if isinstance(out, dict):
                    out["read_summary"] = rec
                else:
                    self.last_read_summary = rec
            return out
        try:
            yield deliver
        finally:
            self.set_mapq(old_rule, old_on)

    def set_pileup(self, enabled=True):
        """The handle's pileup setting (scrg_ctx_set_pileup) for every later mapping call on it: enabled, every OK pair of every
        call is added, on the GPU, to per-position counts the handle keeps on the device (28 bytes per genome base) until
        take_pileup().  The calls' own results do not change.  Off (the default) also discards and releases the accumulator."""
        self._check(_lazy(self.lib, "scrg_ctx_set_pileup")(self.h, 1 if enabled else 0))

    def pileup(self):
        """-> is the handle's pileup setting on."""
        on = C.c_int(0)
        self._check(_lazy(self.lib, "scrg_ctx_get_pileup")(self.h, C.byref(on)))
        return bool(on.value)

    def take_pileup(self):
        """What the mapping calls since the last take piled up (scrg_ctx_take_pileup), ONCE: a dict with "counts", a
        (7, target_len + 1) uint32 array indexed by SCRG_PILE_* and position, "target_len", "n_alignments" and "n_out_of_range".
        The accumulator is empty afterwards.  ScroogeError when nothing was accumulated since the last take."""
        import numpy as np
        r = C.POINTER(Pileup)()
        self._check(_lazy(self.lib, "scrg_ctx_take_pileup")(self.h, C.byref(r)))
        try:
            n = int(r.contents.target_len) + 1
            counts = np.ctypeslib.as_array(r.contents.counts, shape=(SCRG_PILE_PLANES * n,)).copy().reshape(SCRG_PILE_PLANES, n)
            return {"counts": counts, "target_len": int(r.contents.target_len), "n_alignments": int(r.contents.n_alignments),
                    "n_out_of_range": int(r.contents.n_out_of_range)}
        finally:
            _lazy(self.lib, "scrg_pileup_free")(r)

    def take_pileup_sites(self, min_depth=1, min_alt=1, min_alt_per_mille=0):
        """The SITES of what the mapping calls since the last take piled up (scrg_ctx_take_pileup_sites), ONCE: the positions of
        depth >= min_depth where at least min_alt observations, and min_alt_per_mille of the depth, disagree with the resident
        genome — or as many insertions pile up — picked and compacted on the GPU.  -> a dict with "sites", a structured array
        (site_dtype(): pos, counts[7], ref, alt, call, flags) in ascending pos, "n_sites", "target_len", "n_alignments",
        "n_out_of_range" and "rule".  The accumulator is empty afterwards, as after take_pileup().  ScroogeError when nothing was
        accumulated, or (the accumulator is kept) when the genome is no longer resident or has another length."""
        import numpy as np
        rule = _site_rule(min_depth, min_alt, min_alt_per_mille)
        r = C.POINTER(PileupSites)()
        self._check(_lazy(self.lib, "scrg_ctx_take_pileup_sites")(self.h, C.byref(rule), C.byref(r)))
        try:
            n = int(r.contents.n_sites)
            sites = np.zeros(n, dtype=site_dtype())
            if n:
                C.memmove(sites.ctypes.data, r.contents.sites, n * sites.dtype.itemsize)
            return {"sites": sites, "n_sites": n, "target_len": int(r.contents.target_len), "n_alignments": int(r.contents.n_alignments),
                    "n_out_of_range": int(r.contents.n_out_of_range), "rule": (int(min_depth), int(min_alt), int(min_alt_per_mille))}
        finally:
            _lazy(self.lib, "scrg_pileup_sites_free")(r)

    @contextlib.contextmanager
    def _call_clip(self, clip):
        """The per-call keyword clip= of the host align methods (True, or the costs), handled as report= is: the setting for this
        call only.  Yields a function that puts the call's records where they belong: "clip" into the arrays form, `last_clip`
        beside the list form."""
        if clip is None:
            yield lambda out: out
            return
        old_on, old_costs = self.clip()
        on = clip is not False
        self.set_clip(None if clip in (True, False) else clip, on)

        def deliver(out):
            if on:
                rec = self.take_clip()
                if isinstance(out, dict):
                    out["clip"] = rec
                else:
                    self.last_clip = rec
            return out
        try:
            yield deliver
        finally:
            self.set_clip(old_costs, old_on)

    @contextlib.contextmanager
    def _call_diff(self, kind, arrays=False):
        """The per-call keyword diff= of the host align methods: the kind for this call only, the handle's own setting restored
        afterwards.  Yields a function that puts the call's strings where they belong: "diff_offset" / "diff_text" into the
        arrays form, `last_diff` (a list of str) beside the list form."""
        if kind is None:
            yield lambda out: out
            return
        old = self.diff()
        self.set_diff(kind)

        def deliver(out):
            if isinstance(out, dict):
                out["diff_offset"], out["diff_text"] = self.take_diff(arrays=True)
            else:
                self.last_diff = self.take_diff()
            return out
        try:
            yield deliver
        finally:
            self.set_diff(old)

    @contextlib.contextmanager
    def _call_limit(self, max_edits, per_mille):
        """The per-call keywords max_edits= / max_edit_per_mille= of the align methods: the limit for this call only — the
        handle's own setting is restored afterwards, whatever happens."""
        if max_edits is None and per_mille is None:
            yield
            return
        old = self.edit_limit()
        self.set_edit_limit(max_edits, per_mille)
        try:
            yield
        finally:
            self.set_edit_limit(*old)

    @staticmethod
    def _no_limit(max_edits, per_mille):
        if max_edits is not None or per_mille is not None:
            raise ScroogeError(SCRG_ERR_INVALID_ARG, "the _multi calls have no handle and no edit limit")

    def _collect(self, res_p, st):
        try:
            r = res_p.contents
            n = int(r.n_pairs)
            text = C.string_at(r.cigar_text, int(r.cigar_offset[n])) if n else b""
            out = []
            for i in range(n):
                a, b = int(r.cigar_offset[i]), int(r.cigar_offset[i + 1])
                out.append(Alignment(text[a:b - 1].decode(), int(r.edit_distance[i])))
            self.last_timing = {"kernel_ns": int(r.kernel_ns), "pack_ns": int(r.pack_ns),
                                "total_ns": int(r.total_ns)}
            self.last_status = [int(r.pair_status[i]) for i in range(n)]
            self.last_text_end = [int(r.text_end[i]) for i in range(n)] if r.text_end else None      # distance-only mode
        finally:
            self.lib.scrg_result_free(res_p)
        return out

    def _collect_arrays(self, res_p, st):
        """The result as numpy arrays (copies): no per-pair Python objects — for batches of millions of pairs."""
        import numpy as np
        try:
            r = res_p.contents
            n = int(r.n_pairs)

            def arr(ptr, count, dtype):
                if count == 0:
                    return np.zeros(0, dtype=dtype)
                return np.ctypeslib.as_array(ptr, shape=(count,)).view(dtype).copy()

            run_offset = arr(r.run_offset, n + 1, np.uint64)
            cigar_offset = arr(r.cigar_offset, n + 1, np.uint64)
            total_runs = int(run_offset[n]) if n else 0
            out = {"edit_distance": arr(r.edit_distance, n, np.int64),
                   "status": arr(r.pair_status, n, np.uint32),
                   "run_offset": run_offset,
                   # (views of the library's arrays copied with numpy: ctypes.string_at takes no more than 2 GB, a batch of a
                   # million 10 kb pairs has 4.3 GB of runs)
                   "runs": arr(C.cast(r.runs, C.POINTER(C.c_uint8)), 2 * total_runs, np.uint8).reshape(-1, 2)
                           if total_runs else np.zeros((0, 2), np.uint8),      # columns: count, op
                   "cigar_offset": cigar_offset,
                   "cigar_text": arr(C.cast(r.cigar_text, C.POINTER(C.c_uint8)), int(cigar_offset[n]), np.uint8).tobytes() if n else b""}
            if r.text_end:               # distance-only mode
                out["text_end"] = arr(r.text_end, n, np.uint64)
            self.last_timing = {"kernel_ns": int(r.kernel_ns), "pack_ns": int(r.pack_ns),
                                "total_ns": int(r.total_ns)}
        finally:
            self.lib.scrg_result_free(res_p)
        return out

    # -- genasm_gpu::align_all(texts, queries)  (src/genasm_gpu.cu:982-1065) --------
    def _finish(self, res, st, arrays, strict):
        """Collect (and free) the library's result; a pair that overflowed its CIGAR slice is an error unless
        strict=False, in which case the truncated result is returned and `last_status` / `status` says which pairs
        (the C++ shim throws in the same case, scrooge_amd.hpp).  Pairs over the edit limit (status SCRG_PAIR_OVER_EDIT_LIMIT:
        CIGAR "", edit distance > the limit) are results, not errors: strict does not raise for them."""
        out = self._collect_arrays(res, st) if arrays else self._collect(res, st)
        if st == SCRG_ERR_CIGAR_OVERFLOW and strict:
            raise ScroogeError(st, (self.lib.scrg_last_error(self.h) or b"").decode() or
                               "at least one pair overflowed its CIGAR slice")
        return out

    def align_pairs(self, texts, queries, arrays=False, strict=True, max_edits=None, max_edit_per_mille=None, diff=None, report=None,
                    cigar_form=None, clip=None, **kw):
        """diff="md" / "cs": also every pair's difference string, for this call (set_diff): the arrays form gains "diff_offset"
        and "diff_text", the list form leaves the strings in `last_diff`.  report=True: also every pair's alignment report, for
        this call (set_report): the arrays form gains "report", the list form leaves the records in `last_report`.
        cigar_form="windowed" / "merged" / "m": the form of the CIGAR text, for this call (set_cigar_form).
        clip=True or (match, mismatch, gap open, gap extend): every pair comes back as its best-scoring stretch, for this call
        (set_clip): the arrays form gains "clip", the list form leaves the records in `last_clip`."""
        with self._call_limit(max_edits, max_edit_per_mille), self._call_form(cigar_form), self._call_diff(diff) as deliver, \
                self._call_report(report) as deliver_report, self._call_clip(clip) as deliver_clip:
            return deliver_clip(deliver_report(deliver(self._align_pairs(texts, queries, arrays, strict, **kw))))

    def _align_pairs(self, texts, queries, arrays, strict, **kw):
        texts, queries = _bytes_list(texts), _bytes_list(queries)
        if len(texts) != len(queries):
            raise ValueError("texts and queries differ in length")   # reference: assert, genasm_cpu.cpp:559
        n = len(texts)
        tp = (C.c_char_p * max(n, 1))(*texts)
        qp = (C.c_char_p * max(n, 1))(*queries)
        tl = (C.c_uint64 * max(n, 1))(*[len(t) for t in texts])
        ql = (C.c_uint64 * max(n, 1))(*[len(q) for q in queries])
        res = C.POINTER(Result)()
        st = self.lib.scrg_align_pairs(self.h, C.byref(self._params(kw)), n, tp, tl, qp, ql,
                                       C.byref(res))
        self._check(st, allow=(SCRG_ERR_CIGAR_OVERFLOW,))
        return self._finish(res, st, arrays, strict)

    def align_pairs_rows(self, rows, text_off, text_lens, read_off, read_lens, strict=True, devices=None, max_edits=None,
                         max_edit_per_mille=None, diff=None, report=None, cigar_form=None, **kw):
        if devices is not None:
            self._no_limit(max_edits, max_edit_per_mille)
            if diff is not None or report:
                raise ScroogeError(SCRG_ERR_INVALID_ARG, "the _multi calls have no handle and make no difference strings and no report")
            if cigar_form is not None:
                raise ScroogeError(SCRG_ERR_INVALID_ARG, "the _multi calls have no handle: their CIGAR text is the windowed one")
            report = None
        with self._call_limit(max_edits, max_edit_per_mille), self._call_form(cigar_form), self._call_diff(diff) as deliver, \
                self._call_report(report) as deliver_report:
            return deliver_report(deliver(self._align_pairs_rows(rows, text_off, text_lens, read_off, read_lens, strict, devices, **kw)))

    def _align_pairs_rows(self, rows, text_off, text_lens, read_off, read_lens, strict=True, devices=None, **kw):
        """scrg_align_pairs on sequences that sit in ONE 2-D uint8 numpy array (row p: the text of pair p at byte
        text_off, its read at byte read_off — bench.py's staging layout), lengths as integers or per-row arrays: the
        pointer arrays are built with numpy, so a batch of 100 k x 10 kb pairs costs no per-pair Python objects.
        devices: a device list -> scrg_align_pairs_multi (a device may be listed more than once).
        -> the result as numpy arrays (see _collect_arrays); `last_timing` has the library's own clock."""
        import numpy as np
        rows = np.ascontiguousarray(rows, dtype=np.uint8)
        n, stride = rows.shape
        base = rows.ctypes.data + np.arange(n, dtype=np.uint64) * np.uint64(stride)
        tp = (base + np.uint64(text_off)).astype(np.uint64)
        qp = (base + np.uint64(read_off)).astype(np.uint64)
        tl = np.ascontiguousarray(np.broadcast_to(np.asarray(text_lens, dtype=np.uint64), (n,)))
        ql = np.ascontiguousarray(np.broadcast_to(np.asarray(read_lens, dtype=np.uint64), (n,)))
        pp, up = C.POINTER(C.c_char_p), C.POINTER(C.c_uint64)
        res = C.POINTER(Result)()
        if devices is not None:
            dv = (C.c_int32 * len(devices))(*devices)
            st = self.lib.scrg_align_pairs_multi(dv, len(devices), C.byref(self._params(kw)), n, C.cast(tp.ctypes.data, pp),
                                                 C.cast(tl.ctypes.data, up), C.cast(qp.ctypes.data, pp), C.cast(ql.ctypes.data, up), C.byref(res))
            if st not in (SCRG_OK, SCRG_ERR_CIGAR_OVERFLOW):
                raise ScroogeError(st, (self.lib.scrg_multi_last_error() or b"").decode())
            return self._finish(res, st, True, strict)
        st = self.lib.scrg_align_pairs(self.h, C.byref(self._params(kw)), n, C.cast(tp.ctypes.data, pp), C.cast(tl.ctypes.data, up),
                                       C.cast(qp.ctypes.data, pp), C.cast(ql.ctypes.data, up), C.byref(res))
        self._check(st, allow=(SCRG_ERR_CIGAR_OVERFLOW,))
        return self._finish(res, st, True, strict)

    def align_mapping_rows(self, genome, read_rows, read_lens, cand_offsets, cand_start, strict=True, max_edits=None,
                           max_edit_per_mille=None, diff=None, report=None, cigar_form=None, mapq=None, **kw):
        with self._call_limit(max_edits, max_edit_per_mille), self._call_form(cigar_form), self._call_diff(diff) as deliver, \
                self._call_report(report) as deliver_report, self._call_mapq(mapq) as deliver_mapq:
            return deliver_mapq(deliver_report(deliver(self._align_mapping_rows(genome, read_rows, read_lens, cand_offsets, cand_start, strict, **kw))))

    def _align_mapping_rows(self, genome, read_rows, read_lens, cand_offsets, cand_start, strict=True, **kw):
        """scrg_align_mapping (genome: bytes / uint8 array) or scrg_align_mapping_resident (genome=None) with the reads in
        one 2-D uint8 numpy array (one read per row) and the candidates as numpy arrays (cand_offsets: n_reads + 1)."""
        import numpy as np
        read_rows = np.ascontiguousarray(read_rows, dtype=np.uint8)
        nr, stride = read_rows.shape
        rp = (read_rows.ctypes.data + np.arange(nr, dtype=np.uint64) * np.uint64(stride)).astype(np.uint64)
        rl = np.ascontiguousarray(np.broadcast_to(np.asarray(read_lens, dtype=np.uint64), (nr,)))
        co = np.ascontiguousarray(cand_offsets, dtype=np.uint64)
        cs = np.ascontiguousarray(cand_start, dtype=np.uint64)
        assert co.shape == (nr + 1,) and cs.shape == (int(co[nr]),)
        pp, up = C.POINTER(C.c_char_p), C.POINTER(C.c_uint64)
        res = C.POINTER(Result)()
        if genome is None:
            st = self.lib.scrg_align_mapping_resident(self.h, C.byref(self._params(kw)), nr, C.c_void_p(rp.ctypes.data), C.c_void_p(rl.ctypes.data),
                                                      C.c_void_p(co.ctypes.data), C.c_void_p(cs.ctypes.data), None, C.byref(res))
        else:
            g = np.ascontiguousarray(np.frombuffer(genome, dtype=np.uint8) if isinstance(genome, (bytes, bytearray)) else genome, dtype=np.uint8)
            st = self.lib.scrg_align_mapping(self.h, C.byref(self._params(kw)), C.cast(g.ctypes.data, C.c_char_p), g.size, nr,
                                             C.cast(rp.ctypes.data, pp), C.cast(rl.ctypes.data, up), C.cast(co.ctypes.data, up),
                                             C.cast(cs.ctypes.data, up), C.byref(res))
        self._check(st, allow=(SCRG_ERR_CIGAR_OVERFLOW,))
        return self._finish(res, st, True, strict)

    def set_genome_array(self, genome_u8):
        """set_genome for a uint8 numpy array (no copy into a bytes object)."""
        import numpy as np
        g = np.ascontiguousarray(genome_u8, dtype=np.uint8)
        self._check(self.lib.scrg_genome_set(self.h, C.cast(g.ctypes.data, C.c_char_p), g.size))

    def align_pairs_multi(self, devices, texts, queries, arrays=False, strict=True, max_edits=None, max_edit_per_mille=None, **kw):
        """scrg_align_pairs_multi: the same call spread over several GPUs (a device may be listed more than once).  No edit
        limit (no handle): max_edits / max_edit_per_mille raise."""
        self._no_limit(max_edits, max_edit_per_mille)
        texts, queries = _bytes_list(texts), _bytes_list(queries)
        n = len(texts)
        tp = (C.c_char_p * max(n, 1))(*texts)
        qp = (C.c_char_p * max(n, 1))(*queries)
        tl = (C.c_uint64 * max(n, 1))(*[len(t) for t in texts])
        ql = (C.c_uint64 * max(n, 1))(*[len(q) for q in queries])
        dv = (C.c_int32 * len(devices))(*devices)
        res = C.POINTER(Result)()
        st = self.lib.scrg_align_pairs_multi(dv, len(devices), C.byref(self._params(kw)), n, tp, tl, qp, ql, C.byref(res))
        if st not in (SCRG_OK, SCRG_ERR_CIGAR_OVERFLOW):
            raise ScroogeError(st, (self.lib.scrg_multi_last_error() or b"").decode())
        return self._finish(res, st, arrays, strict)

    def align_mapping_multi(self, devices, genome, reads, candidates, reverse=None, arrays=False, strict=True, max_edits=None,
                            max_edit_per_mille=None, **kw):
        """scrg_align_mapping_multi: read mapping spread over several GPUs; reverse: optional list (per read) of 0/1 lists.  No
        edit limit (no handle): max_edits / max_edit_per_mille raise."""
        self._no_limit(max_edits, max_edit_per_mille)
        genome = genome.encode() if isinstance(genome, str) else bytes(genome)
        reads = _bytes_list(reads)
        nr = len(reads)
        offs, starts, rev = [0], [], []
        for k, c in enumerate(candidates):
            starts.extend(int(x) for x in c)
            rev.extend(int(x) for x in (reverse[k] if reverse is not None else [0] * len(c)))
            offs.append(len(starts))
        rp = (C.c_char_p * max(nr, 1))(*reads)
        rl = (C.c_uint64 * max(nr, 1))(*[len(r) for r in reads])
        co = (C.c_uint64 * (nr + 1))(*offs)
        cs = (C.c_uint64 * max(len(starts), 1))(*starts)
        cr = (C.c_uint8 * max(len(rev), 1))(*rev)
        dv = (C.c_int32 * len(devices))(*devices)
        res = C.POINTER(Result)()
        st = self.lib.scrg_align_mapping_multi(dv, len(devices), C.byref(self._params(kw)), genome, len(genome), nr, rp, rl, co, cs,
                                               C.cast(cr, C.c_void_p) if reverse is not None else None, C.byref(res))
        if st not in (SCRG_OK, SCRG_ERR_CIGAR_OVERFLOW):
            raise ScroogeError(st, (self.lib.scrg_multi_last_error() or b"").decode())
        return self._finish(res, st, arrays, strict)

    # -- genasm_gpu::align_all(genome, reads)  (src/genasm_gpu.cu:890-980) ----------
    def set_genome(self, genome):
        """Stage, transfer and pack a genome once; align_mapping(None, reads, candidates) then aligns batches
        against it without touching it again (scrg_genome_set / scrg_align_mapping_resident)."""
        genome = genome.encode() if isinstance(genome, str) else bytes(genome)
        self._check(self.lib.scrg_genome_set(self.h, genome, len(genome)))

    def clear_genome(self):
        self.lib.scrg_genome_clear(self.h)

    # -- seeding (include/scrooge_amd.h, SEEDING) ----------
    def index_genome(self, rule=None):
        """scrg_genome_index: the k-mer index of the genome left resident by set_genome(), built on the GPU by `rule` (a SeedRule;
        None: the defaults) and kept on the handle until clear_index(), clear_genome() or another genome.  -> a dict: the rule,
        n_entries and device_bytes (scrg_genome_index_info), smer and n_positions (scrg_seed_sampling_info)."""
        self._check(_lazy(self.lib, "scrg_genome_index")(self.h, _seed_rule(rule)))
        return self.index_info()

    def set_seed_sampling(self, smer):
        """scrg_ctx_set_seed_sampling: the next index_genome() (and io.Job.seed) samples its k-mers as closed syncmers of `smer`-mers
        (3 .. 15 and below the rule's k); 0, the default: every k-mer.  An index that exists keeps the value it was built with."""
        smer = int(smer)
        if smer < 0 or smer > 0xffffffff:
            raise ScroogeError(SCRG_ERR_INVALID_ARG, "seed sampling: smer is 0 (off) or 3 .. 15")
        self._check(_lazy(self.lib, "scrg_ctx_set_seed_sampling")(self.h, smer))

    def seed_sampling_info(self):
        """scrg_seed_sampling_info -> a dict: smer of the current index, n_positions it considered, n_lookups of the last
        find_candidates.  ScroogeError without an index."""
        s, n, l = C.c_uint32(), C.c_uint64(), C.c_uint64()
        self._check(_lazy(self.lib, "scrg_seed_sampling_info")(self.h, C.byref(s), C.byref(n), C.byref(l)))
        return {"smer": int(s.value), "n_positions": int(n.value), "n_lookups": int(l.value)}

    def index_info(self):
        k, n, b = _SeedRuleC(), C.c_uint64(), C.c_uint64()
        self._check(_lazy(self.lib, "scrg_genome_index_info")(self.h, C.byref(k), C.byref(n), C.byref(b)))
        info = {"rule": SeedRule(*[int(getattr(k, f)) for f, _ in _SeedRuleC._fields_]), "n_entries": int(n.value), "device_bytes": int(b.value)}
        if hasattr(self.lib, "scrg_seed_sampling_info"):          # (a library from before sampling, loaded for a kernel A/B, has neither field)
            sampling = self.seed_sampling_info()
            info.update(smer=sampling["smer"], n_positions=sampling["n_positions"])
        return info

    def clear_index(self):
        _lazy(self.lib, "scrg_genome_index_clear")(self.h)

    def find_candidates(self, reads, info=False):
        """scrg_find_candidates: every read's candidates against the handle's index, found on the GPU.  -> (candidates, reverse,
        votes), per-read lists in the form align_mapping_directed / align_mapping_paired(reads, candidates, reverse=...) take, the
        best-voted candidate first; info=True: and a dict of the counters (n_hits, n_clusters, n_keys_over_max_occ, n_lookups) and
        the rule."""
        reads = _bytes_list(reads)
        nr = len(reads)
        rp = (C.c_char_p * max(nr, 1))(*reads)
        rl = (C.c_uint64 * max(nr, 1))(*[len(r) for r in reads])
        cp = C.POINTER(Candidates)()
        self._check(_lazy(self.lib, "scrg_find_candidates")(self.h, nr, C.cast(rp, C.c_void_p), C.cast(rl, C.c_void_p), C.byref(cp)))
        out = _take_candidates(self.lib, cp)
        if info:
            out[3]["n_lookups"] = self.seed_sampling_info()["n_lookups"]
        return out if info else out[:3]

    def align_mapping(self, genome, reads, candidates, arrays=False, strict=True, max_edits=None, max_edit_per_mille=None, diff=None, report=None,
                      cigar_form=None, clip=None, mapq=None, **kw):
        """candidates[r] = list of start_in_reference for read r (forward strand).  genome=None: the genome
        left resident by set_genome().  diff="md" / "cs", report=True, cigar_form=, clip=: as align_pairs.  mapq=True or a MapqRule
        (with best=True): also every read's summary and MAPQ — "read_summary" in the arrays form, `last_read_summary` otherwise."""
        with self._call_limit(max_edits, max_edit_per_mille), self._call_form(cigar_form), self._call_diff(diff) as deliver, \
                self._call_report(report) as deliver_report, self._call_clip(clip) as deliver_clip, self._call_mapq(mapq) as deliver_mapq:
            return deliver_mapq(deliver_clip(deliver_report(deliver(self._align_mapping(genome, reads, candidates, arrays, strict, **kw)))))

    def _align_mapping(self, genome, reads, candidates, arrays, strict, **kw):
        if genome is not None:
            genome = genome.encode() if isinstance(genome, str) else bytes(genome)
        reads = _bytes_list(reads)
        nr = len(reads)
        if len(candidates) != nr:
            raise ValueError("one candidate list per read expected")
        offs, starts = [0], []
        for c in candidates:
            starts.extend(int(x) for x in c)
            offs.append(len(starts))
        rp = (C.c_char_p * max(nr, 1))(*reads)
        rl = (C.c_uint64 * max(nr, 1))(*[len(r) for r in reads])
        co = (C.c_uint64 * (nr + 1))(*offs)
        cs = (C.c_uint64 * max(len(starts), 1))(*starts)
        res = C.POINTER(Result)()
        if genome is None:
            st = self.lib.scrg_align_mapping_resident(self.h, C.byref(self._params(kw)), nr, rp, rl, co, cs, None,
                                                      C.byref(res))
        else:
            st = self.lib.scrg_align_mapping(self.h, C.byref(self._params(kw)), genome, len(genome),
                                             nr, rp, rl, co, cs, C.byref(res))
        self._check(st, allow=(SCRG_ERR_CIGAR_OVERFLOW,))
        return self._finish(res, st, arrays, strict)

    @staticmethod
    def _flat_candidates(reads, candidates, per_candidate):
        """The mapping calls' arguments: reads as bytes, cand_offsets, and every per-candidate list (one list per read, or None)
        flattened — ValueError where a list's shape is not that of `candidates`."""
        reads = _bytes_list(reads)
        if len(candidates) != len(reads):
            raise ValueError("one candidate list per read expected")
        offs = [0]
        for c in candidates:
            offs.append(offs[-1] + len(c))
        flat = []
        for name, lists in per_candidate:
            if lists is None:
                flat.append(None)
                continue
            if len(lists) != len(candidates) or any(len(a) != len(c) for a, c in zip(lists, candidates)):
                raise ValueError("%s: one entry per candidate expected" % name)
            flat.append([int(x) for a in lists for x in a])
        return reads, offs, flat

    def align_mapping_directed(self, reads, candidates, reverse=None, leftward=None, arrays=False, strict=True, max_edits=None,
                               max_edit_per_mille=None, report=None, cigar_form=None, clip=None, mapq=None, **kw):
        """scrg_align_mapping_directed, against the genome left resident by set_genome(): candidates[r] = list of positions of
        read r; reverse / leftward: optional lists (per read) of 0/1 lists.  A leftward candidate aligns the read (its reverse
        complement if reverse) so that it ENDS at its position and grows to the left: the result is the reference's for the
        reverse complements of that read and of genome[0:position], its CIGAR from the anchor outwards.  leftward=None: exactly
        align_mapping(None, ...) with strands."""
        reads, offs, (starts, rev, left) = self._flat_candidates(reads, candidates, (("candidates", candidates), ("reverse", reverse),
                                                                                      ("leftward", leftward)))
        nr, n = len(reads), offs[-1]
        rp = (C.c_char_p * max(nr, 1))(*reads)
        rl = (C.c_uint64 * max(nr, 1))(*[len(r) for r in reads])
        co = (C.c_uint64 * (nr + 1))(*offs)
        cs = (C.c_uint64 * max(n, 1))(*starts)
        cr = (C.c_uint8 * max(n, 1))(*(rev or []))
        cl = (C.c_uint8 * max(n, 1))(*(left or []))
        res = C.POINTER(Result)()
        with self._call_limit(max_edits, max_edit_per_mille), self._call_form(cigar_form), self._call_report(report) as deliver_report, \
                self._call_clip(clip) as deliver_clip, self._call_mapq(mapq) as deliver_mapq:
            st = _lazy(self.lib, "scrg_align_mapping_directed")(self.h, C.byref(self._params(kw)), nr, C.cast(rp, C.c_void_p), C.cast(rl, C.c_void_p),
                                                                C.cast(co, C.c_void_p), C.cast(cs, C.c_void_p),
                                                                C.cast(cr, C.c_void_p) if rev is not None else None,
                                                                C.cast(cl, C.c_void_p) if left is not None else None, C.byref(res))
            self._check(st, allow=(SCRG_ERR_CIGAR_OVERFLOW,))
            return deliver_mapq(deliver_clip(deliver_report(self._finish(res, st, arrays, strict))))

    def align_mapping_paired(self, reads, candidates, reverse=None, rule=None, arrays=False, strict=True, max_edits=None, max_edit_per_mille=None,
                             report=None, cigar_form=None, clip=None, **kw):
        """scrg_align_mapping_paired, against the genome left resident by set_genome(): reads 2m and 2m+1 are mate pair m, and their
        winners are chosen together on the GPU by `rule` (a MateRule; None: FR, any span, penalty 0) — otherwise best-candidate mode:
        winners as without it, losers SCRG_PAIR_NOT_BEST with their distance.  candidates / reverse as align_mapping_directed.
        -> (results, mates): results as align_mapping's, mates a structured array (mate_dtype()) with one record per mate pair,
        winner[] as pair indices of the result (MATES_NONE: none)."""
        import numpy as np
        reads, offs, (starts, rev) = self._flat_candidates(reads, candidates, (("candidates", candidates), ("reverse", reverse)))
        nr, n = len(reads), offs[-1]
        rp = (C.c_char_p * max(nr, 1))(*reads)
        rl = (C.c_uint64 * max(nr, 1))(*[len(r) for r in reads])
        co = (C.c_uint64 * (nr + 1))(*offs)
        cs = (C.c_uint64 * max(n, 1))(*starts)
        cr = (C.c_uint8 * max(n, 1))(*(rev or []))
        res, mt = C.POINTER(Result)(), C.c_void_p()
        with self._call_limit(max_edits, max_edit_per_mille), self._call_form(cigar_form), self._call_report(report) as deliver_report, \
                self._call_clip(clip) as deliver_clip:
            st = _lazy(self.lib, "scrg_align_mapping_paired")(self.h, C.byref(self._params(kw)), nr, C.cast(rp, C.c_void_p), C.cast(rl, C.c_void_p),
                                                              C.cast(co, C.c_void_p), C.cast(cs, C.c_void_p),
                                                              C.cast(cr, C.c_void_p) if rev is not None else None, _mate_rule(rule), C.byref(mt),
                                                              C.byref(res))
            try:
                self._check(st, allow=(SCRG_ERR_CIGAR_OVERFLOW,))
                m = C.cast(mt, C.POINTER(Mates)).contents
                mates = np.zeros(int(m.n_mates), dtype=mate_dtype())
                if m.n_mates:
                    C.memmove(mates.ctypes.data, m.records, 32 * int(m.n_mates))
            finally:
                _lazy(self.lib, "scrg_mates_free")(mt)
            return deliver_clip(deliver_report(self._finish(res, st, arrays, strict))), mates

    def align_anchored(self, reads, anchors, reverse=None, arrays=False, strict=True, cigar_form=None, **kw):
        """scrg_align_mapping_anchored, against the genome left resident by set_genome(): anchors[r] = list of (genome position,
        read position) for read r — the read position counted in the read as aligned (its reverse complement where reverse says
        so); reverse: optional list (per read) of 0/1 lists.  What lies left of the anchor is aligned leftwards ending at it, the
        rest rightwards from it, and the halves are joined (join_anchored).  Returns the usual result — a list of Alignment, or
        the arrays — and text_start: `(alignments, text_start)`, or the arrays with "text_start" among them.  No best-candidate
        mode and no edit limit (ScroogeError).  cigar_form=: as align_pairs — the joined text in that form, across the seam."""
        with self._call_form(cigar_form):
            return self._align_anchored(reads, anchors, reverse, arrays, strict, **kw)

    def _align_anchored(self, reads, anchors, reverse, arrays, strict, **kw):
        for a in anchors:
            for x in a:
                if len(x) != 2 or int(x[0]) < 0 or int(x[1]) < 0:
                    raise ValueError("an anchor is (genome position, read position), both >= 0")
        ga = [[int(x[0]) for x in a] for a in anchors]
        ra = [[int(x[1]) for x in a] for a in anchors]
        reads, offs, (ga_f, ra_f, rev) = self._flat_candidates(reads, anchors, (("anchors", ga), ("anchors", ra), ("reverse", reverse)))
        for r, a in zip(reads, ra):
            if any(x > len(r) for x in a):
                raise ValueError("anchor out of range: a read position is 0 .. the read's length")
        import numpy as np
        nr, n = len(reads), offs[-1]
        rp = (C.c_char_p * max(nr, 1))(*reads)
        rl = (C.c_uint64 * max(nr, 1))(*[len(r) for r in reads])
        co = (C.c_uint64 * (nr + 1))(*offs)
        cg = (C.c_uint64 * max(n, 1))(*ga_f)
        ca = (C.c_uint64 * max(n, 1))(*ra_f)
        cr = (C.c_uint8 * max(n, 1))(*(rev or []))
        ts = (C.c_uint64 * max(n, 1))()
        res = C.POINTER(Result)()
        st = _lazy(self.lib, "scrg_align_mapping_anchored")(self.h, C.byref(self._params(kw)), nr, C.cast(rp, C.c_void_p), C.cast(rl, C.c_void_p),
                                                            C.cast(co, C.c_void_p), C.cast(cg, C.c_void_p), C.cast(ca, C.c_void_p),
                                                            C.cast(cr, C.c_void_p) if rev is not None else None, C.cast(ts, C.c_void_p), C.byref(res))
        self._check(st, allow=(SCRG_ERR_CIGAR_OVERFLOW,))
        out = self._finish(res, st, arrays, strict)
        text_start = np.array(ts[:n], dtype=np.uint64)
        if arrays:
            out["text_start"] = text_start
            return out
        return out, [int(x) for x in text_start]

    # -- device-pointer layer (torch tensors as plain device memory) -----------
    def set_stream(self, stream_handle):
        """stream_handle: a hipStream_t as an integer (0 = the device's null stream)."""
        self._check(self.lib.scrg_ctx_set_stream(self.h, C.c_void_p(stream_handle)))
        self._stream = int(stream_handle)

    def use_own_stream(self):
        self._check(self.lib.scrg_ctx_use_own_stream(self.h))
        self._stream = None

    def restore_stream(self, saved):
        """saved: what `stream_setting` returned — the handle enqueues where it did then."""
        if saved is None:
            self.use_own_stream()
        else:
            self.set_stream(saved)

    @property
    def stream_setting(self):
        """None: the handle's own stream; else the hipStream_t (integer) given to set_stream."""
        return getattr(self, "_stream", None)

    def pack_planar(self, ascii_u8, planar_u64, bad_u32):
        n_words = ascii_u8.numel() // 32
        self._check(self.lib.scrg_pack_planar(self.h, _ptr(ascii_u8), n_words, _ptr(planar_u64),
                                              _ptr(bad_u32)))

    def pack_planar_groups(self, ascii_u8, n_rows, words_per_row, planar_u64, bad_u32):
        """ASCII rows -> planar 2-bit in the lane-interleaved layout (scrg_pack_planar_groups): word w of row r at
        ((r // 64) * words_per_row + w) * 64 + r % 64; align with text_stride_words = read_stride_words = 64."""
        self._check(self.lib.scrg_pack_planar_groups(self.h, _ptr(ascii_u8), int(n_rows), int(words_per_row),
                                                     _ptr(planar_u64), _ptr(bad_u32)))

    def align_device(self, n_pairs, seq, pairs, runs, ed, n_runs, status, max_edits=None, max_edit_per_mille=None, **kw):
        with self._call_limit(max_edits, max_edit_per_mille):
            self._check(self.lib.scrg_align_device(self.h, C.byref(self._params(kw)), int(n_pairs),
                                                   _ptr(seq), _ptr(pairs), _ptr(runs), _ptr(ed),
                                                   _ptr(n_runs), _ptr(status)))

    def align_device_edits(self, n_pairs, seq, pairs, streams_u8, ed, stream_len, status, n_runs=None, max_edits=None,
                           max_edit_per_mille=None, **kw):
        """Like align_device, but the pairs' slices receive EDIT STREAMS (one byte per edit and per window end) and stream_len their
        lengths in bytes: the one-pair-per-lane kernels only (lanes_per_pair = 1, the default for every W/O).
        n_runs (optional int32 tensor): the run count of every alignment, for a receiver that decodes in one pass."""
        with self._call_limit(max_edits, max_edit_per_mille):
            self._check(self.lib.scrg_align_device_edits(self.h, C.byref(self._params(kw)), int(n_pairs),
                                                         _ptr(seq), _ptr(pairs), _ptr(streams_u8), _ptr(ed),
                                                         _ptr(stream_len), _ptr(status), _ptr(n_runs)))

    def align_device_distance(self, n_pairs, seq, pairs, ed, text_end, status, max_edits=None, max_edit_per_mille=None, **kw):
        """scrg_align_device_distance: edit distance (int64), status (int32: 0, or 2 over the edit limit) and — text_end may
        be None — the text characters every alignment consumed (int32), on device tensors.  No run buffer exists and the
        descriptors' cigar_off / cigar_cap are not looked at; the one-pair-per-lane kernels only."""
        with self._call_limit(max_edits, max_edit_per_mille):
            self._check(_lazy(self.lib, "scrg_align_device_distance")(self.h, C.byref(self._params(kw)), int(n_pairs), _ptr(seq), _ptr(pairs),
                                                                      _ptr(ed), _ptr(text_end), _ptr(status)))

    def diff_lengths(self, kind, n_pairs, seq, pairs, runs, run_offset, run_offset_stride, n_runs, diff_len, **kw):
        """scrg_diff_lengths on device tensors: diff_len[p] (int64) = the length of pair p's "md" / "cs" string incl. its NUL.
        run_offset / run_offset_stride: a plain int64 tensor and 1 (dense runs), or None and 6 (the pairs' slices: the
        descriptors' cigar_off, n_runs capped at cigar_cap).  kw: text_stride_words, read_stride_words, stranded."""
        ro = C.c_void_p(pairs.data_ptr() + 32) if run_offset is None else _ptr(run_offset)
        self._check(_lazy(self.lib, "scrg_diff_lengths")(self.h, C.byref(self._params(kw)), _diff_kind(kind), int(n_pairs), _ptr(seq), _ptr(pairs),
                                                         _ptr(runs), ro, int(run_offset_stride), _ptr(n_runs), _ptr(diff_len)))

    def diff_render(self, kind, n_pairs, seq, pairs, runs, run_offset, run_offset_stride, n_runs, diff_len, diff_offset, diff_text_u8, bad_i32,
                    capacity=None, **kw):
        """scrg_diff_render on device tensors: pair p's string goes to diff_text_u8[diff_offset[p]:]; bad_i32[0] counts the pairs
        whose segment is not inside the capacity (default: the tensor's size) or whose runs do not fit their sequences."""
        ro = C.c_void_p(pairs.data_ptr() + 32) if run_offset is None else _ptr(run_offset)
        cap = int(diff_text_u8.numel()) if capacity is None else int(capacity)
        self._check(_lazy(self.lib, "scrg_diff_render")(self.h, C.byref(self._params(kw)), _diff_kind(kind), int(n_pairs), _ptr(seq), _ptr(pairs),
                                                        _ptr(runs), ro, int(run_offset_stride), _ptr(n_runs), _ptr(diff_len), _ptr(diff_offset),
                                                        _ptr(diff_text_u8), cap, _ptr(bad_i32)))

    def cigar_text_lengths(self, form, n_pairs, runs, run_offset, run_offset_stride, n_runs, text_len, pairs=None):
        """scrg_cigar_text_lengths on device tensors: text_len[p] (int64) = the length of pair p's CIGAR text in `form`
        ("windowed", "merged", "m") incl. its NUL.  run_offset / run_offset_stride: a plain int64 tensor and 1 (dense runs), or
        None and 6 with pairs= the descriptors (their cigar_off, n_runs capped at cigar_cap)."""
        ro = C.c_void_p(pairs.data_ptr() + 32) if run_offset is None else _ptr(run_offset)
        self._check(_lazy(self.lib, "scrg_cigar_text_lengths")(self.h, _cigar_form(form), int(n_pairs), _ptr(runs), ro, int(run_offset_stride),
                                                               _ptr(n_runs), _ptr(text_len)))

    def cigar_text_render(self, form, n_pairs, runs, run_offset, run_offset_stride, n_runs, text_len, text_offset, text_u8, bad_i32, capacity=None,
                          pairs=None):
        """scrg_cigar_text_render on device tensors: pair p's text goes to text_u8[text_offset[p]:]; bad_i32[0] counts the pairs
        whose segment is not inside the capacity (default: the tensor's size), whose text_len is not their string's length, or
        (merged forms) whose runs hold a zero count or an operation other than = X I D."""
        ro = C.c_void_p(pairs.data_ptr() + 32) if run_offset is None else _ptr(run_offset)
        cap = int(text_u8.numel()) if capacity is None else int(capacity)
        self._check(_lazy(self.lib, "scrg_cigar_text_render")(self.h, _cigar_form(form), int(n_pairs), _ptr(runs), ro, int(run_offset_stride),
                                                              _ptr(n_runs), _ptr(text_len), _ptr(text_offset), _ptr(text_u8), cap, _ptr(bad_i32)))

    def report_device(self, n_pairs, seq, pairs, runs, run_offset, run_offset_stride, n_runs, ed, status, report, fail_i32=None, per_base=False,
                      **kw):
        """scrg_report_device on device tensors: report (n_pairs x 8 int32: REPORT_FIELDS per row, or any tensor of 32 bytes per
        pair) gets every pair's record; fail_i32[0] (optional) += the pairs whose verdict is neither 0 nor REPORT_NO_ALIGNMENT.
        run_offset / run_offset_stride as diff_lengths; ed: int64; status: int32 as an align call or select_best left it, or None
        (every pair has an alignment).  kw: text_stride_words, read_stride_words, stranded; TEXT_REVCOMP is honoured when
        set_text_strands(True).  per_base=True (the test build only, variant="select": scrg_params.reserved[0] = 16384): the same
        kernel with the base check one base at a time — identical records; the shipped library refuses it."""
        ro = C.c_void_p(pairs.data_ptr() + 32) if run_offset is None else _ptr(run_offset)
        p = self._params(kw)
        if per_base:
            q = Params()
            C.memmove(C.byref(q), C.byref(p), C.sizeof(Params))
            q.reserved[0] |= REPORT_PER_BASE
            p = q
        self._check(_lazy(self.lib, "scrg_report_device")(self.h, C.byref(p), int(n_pairs), _ptr(seq), _ptr(pairs), _ptr(runs), ro,
                                                          int(run_offset_stride), _ptr(n_runs), _ptr(ed), _ptr(status), _ptr(report), _ptr(fail_i32)))

    def clip_device(self, n_pairs, runs, run_offset, run_offset_stride, n_runs, status, clip, costs=None, apply=False, pairs=None):
        """scrg_clip_device on device tensors: clip (n_pairs x 8 int32: CLIP_FIELDS per row, or any tensor of 32 bytes per pair)
        gets every pair's record.  run_offset / run_offset_stride as report_device (run_offset=None with stride 6: the
        descriptors' cigar_off, `pairs`); status: int32 as an align call or select_best left it, or None (every pair is OK).
        apply=True: the kept stretch also becomes the pair's alignment — n_runs, run_offset and (stride 6) the capacity behind
        it are WRITTEN."""
        ro = C.c_void_p(pairs.data_ptr() + 32) if run_offset is None and pairs is not None else _ptr(run_offset)
        self._check(_lazy(self.lib, "scrg_clip_device")(self.h, None, int(n_pairs), _ptr(runs), ro, int(run_offset_stride), _ptr(n_runs), _ptr(status),
                                                        _clip_costs(costs), 1 if apply else 0, _ptr(clip)))

    def pileup_add(self, n_pairs, seq, pairs, runs, run_offset, run_offset_stride, n_runs, status, target_start, target_len, acc_u32,
                   out_of_range_i32=None, **kw):
        """scrg_pileup_add on device tensors: every pair with status 0 (status None: every pair) and runs is added to acc_u32
        (7 * (target_len + 1) words of 32 bits, zeroed by the caller before the first add) at target_start[p] (int64);
        out_of_range_i32[0] (optional) += the pairs with a column or an insertion outside the target.  run_offset /
        run_offset_stride as report_device.  kw: text_stride_words, read_stride_words, stranded.  Planes 0 and 5 are in edge form
        until pileup_finish."""
        ro = C.c_void_p(pairs.data_ptr() + 32) if run_offset is None else _ptr(run_offset)
        self._check(_lazy(self.lib, "scrg_pileup_add")(self.h, C.byref(self._params(kw)), int(n_pairs), _ptr(seq), _ptr(pairs), _ptr(runs), ro,
                                                       int(run_offset_stride), _ptr(n_runs), _ptr(status), _ptr(target_start), int(target_len),
                                                       _ptr(acc_u32), _ptr(out_of_range_i32)))

    def pileup_finish(self, target_len, acc_u32, counts_u32=None):
        """scrg_pileup_finish on device tensors: counts_u32 (None: acc_u32 itself, in place) = the counts of acc_u32."""
        self._check(_lazy(self.lib, "scrg_pileup_finish")(self.h, int(target_len), _ptr(acc_u32), _ptr(acc_u32 if counts_u32 is None else counts_u32)))

    def pileup_sites_scratch_bytes(self, target_len):
        """scrg_pileup_sites_scratch_bytes: the caller's scratch for pileup_sites_mark / _write on a target of target_len positions."""
        return int(_lazy(self.lib, "scrg_pileup_sites_scratch_bytes")(int(target_len)))

    def pileup_sites_mark(self, target_len, counts_u32, seq, genome_off, rule, scratch_u8, n_sites_i64):
        """scrg_pileup_sites_mark on device tensors: the rule — (min_depth, min_alt, min_alt_per_mille[, reserved]) — at every
        position of counts_u32 (7 * (target_len + 1) words, counts form) against the bases packed in seq from base genome_off;
        n_sites_i64[0] = the number of sites; scratch_u8 (pileup_sites_scratch_bytes, 8-byte aligned) then holds what
        pileup_sites_write needs."""
        r = _site_rule(*rule)
        self._check(_lazy(self.lib, "scrg_pileup_sites_mark")(self.h, int(target_len), _ptr(counts_u32), _ptr(seq), int(genome_off), C.byref(r),
                                                              _ptr(scratch_u8), _ptr(n_sites_i64)))

    def pileup_sites_write(self, target_len, counts_u32, seq, genome_off, scratch_u8, cap, sites_u8):
        """scrg_pileup_sites_write on device tensors: sites_u8 (40 bytes per record, site_dtype()) = the sites the mark found, in
        ascending pos, those of index < cap only."""
        self._check(_lazy(self.lib, "scrg_pileup_sites_write")(self.h, int(target_len), _ptr(counts_u32), _ptr(seq), int(genome_off), _ptr(scratch_u8),
                                                               int(cap), _ptr(sites_u8)))

    def compact_runs(self, n_pairs, pairs, runs, n_runs, dense_off, dense):
        self._check(self.lib.scrg_compact_runs(self.h, int(n_pairs), _ptr(pairs), _ptr(runs),
                                               _ptr(n_runs), _ptr(dense_off), _ptr(dense)))

    def select_best(self, n_pairs, group_key_u32, ed, status, n_runs, is_best_u8=None):
        """scrg_select_best on device tensors: in every run of consecutive pairs with the same group key the eligible pair
        (status != 2) with the smallest edit distance stays, ties to the first; the others get n_runs 0 and status 3.  After
        it, compact_runs with offsets made from the new n_runs gathers the winners only."""
        self._check(_lazy(self.lib, "scrg_select_best")(self.h, int(n_pairs), _ptr(group_key_u32), _ptr(ed), _ptr(status), _ptr(n_runs),
                                                        _ptr(is_best_u8)))

    def select_mates(self, n_mates, first_i64, start_i64, read_len_i32, reverse_u8, ed, status, n_runs, is_best_u8=None, records_u8=None, rule=None,
                     team=None):
        """scrg_select_mates on device tensors: reads 2m and 2m+1 are mate pair m, first_i64[r] (2 n_mates + 1 entries) the index of
        read r's first pair; per pair its start, its read's length, its strand (reverse_u8 may be None: all forward), ed (int64) and
        status.  By the rule (a MateRule, None: the default) every mate pair's winners stay as they are, every other eligible pair
        gets n_runs 0 and status 3; records_u8: 32 bytes per mate pair (mate_dtype()).  Enqueued, not synchronised.  team: the lanes
        per mate pair (4 .. 64) for a caller that knows its largest n_a x n_b (scrg_select_mates_team); None: found on the device."""
        self._check(_lazy(self.lib, "scrg_select_mates_team")(self.h, _mate_rule(rule), int(team or 0), int(n_mates), _ptr(first_i64), _ptr(start_i64),
                                                              _ptr(read_len_i32), _ptr(reverse_u8) if reverse_u8 is not None else None, _ptr(ed),
                                                              _ptr(status), _ptr(n_runs), _ptr(is_best_u8) if is_best_u8 is not None else None,
                                                              _ptr(records_u8)))

    def read_summary(self, n_reads, n_pairs, first_i64, read_len_i32, ed, status, out_u8, keep_status=None, rule=None):
        """scrg_read_summary on device tensors: first_i64[r] (n_reads + 1 entries) the index of read r's first pair; per pair its
        read's length, ed (int64) and status (2: over the edit limit, not eligible; none is written).  out_u8: 32 bytes per read
        (read_summary_dtype()), winner as an index into these arrays; keep_status (may be None; n_pairs int32, not `status`): the
        statuses with every status-0 pair that is not the winner of a KEPT read as 3.  rule: a MapqRule, None: the defaults.
        Enqueued, not synchronised; before or after select_best with the same records."""
        self._check(_lazy(self.lib, "scrg_read_summary")(self.h, _mapq_rule(rule), int(n_reads), int(n_pairs), _ptr(first_i64), _ptr(read_len_i32),
                                                         _ptr(ed), _ptr(status), _ptr(out_u8), _ptr(keep_status) if keep_status is not None else None))

    def compact_runs_packed(self, n_pairs, pairs, runs, n_runs, dense_off, packed_u8, **kw):
        """Like compact_runs, one byte per run (op << 6 | count; W-O <= 63): the transfer format of the RCCL gather."""
        self._check(self.lib.scrg_compact_runs_packed(self.h, C.byref(self._params(kw)), int(n_pairs), _ptr(pairs),
                                                      _ptr(runs), _ptr(n_runs), _ptr(dense_off), _ptr(packed_u8)))

    def unpack_runs(self, n_runs, packed_u8, runs_u8):
        """Restores scrg_run pairs (2 bytes each) from packed runs."""
        self._check(self.lib.scrg_unpack_runs(self.h, int(n_runs), _ptr(packed_u8), _ptr(runs_u8)))

    def encode_edit_stream(self, n_pairs, pairs, runs, n_runs, stream_u8, stream_off_i64, stream_len_i32, total_i64, **kw):
        """Runs -> edit stream (one byte per edit and per window, scrooge_amd.h): the transfer format of the RCCL gather.
        total_i64[0] = bytes of stream_u8 used, total_i64[1] = pairs that did not fit.  W / O (kw) place the window ends."""
        self._check(self.lib.scrg_encode_edit_stream(self.h, C.byref(self._params(kw)), int(n_pairs), _ptr(pairs), _ptr(runs), _ptr(n_runs),
                                                     _ptr(stream_u8), int(stream_u8.numel()), _ptr(stream_off_i64),
                                                     _ptr(stream_len_i32), _ptr(total_i64)))

    def decode_edit_stream(self, n_pairs, stream_u8, stream_off_i64, stream_len_i32, read_len_i64, read_len_stride,
                           dense_off_i64, dense_u8, n_runs_i32, bad_i32, **kw):
        """Edit stream -> scrg_run pairs, window by window as the stream says; dense_u8 None: count only."""
        self._check(self.lib.scrg_decode_edit_stream(self.h, C.byref(self._params(kw)), int(n_pairs), _ptr(stream_u8),
                                                     int(stream_u8.numel()), _ptr(stream_off_i64), _ptr(stream_len_i32), _ptr(read_len_i64),
                                                     int(read_len_stride),
                                                     _ptr(dense_off_i64) if dense_off_i64 is not None else None,
                                                     _ptr(dense_u8) if dense_u8 is not None else None,
                                                     int(dense_u8.numel() * dense_u8.element_size() // 2) if dense_u8 is not None else 0,      # capacity in runs (2 bytes each), whatever the tensor's element type
                                                     _ptr(n_runs_i32), _ptr(bad_i32)))

    def ascii_to_twobit(self, count, lens, ascii_off, ascii, twobit_off, twobit, bad):
        self._check(self.lib.scrg_ascii_to_twobit(self.h, int(count), _ptr(lens), _ptr(ascii_off),
                                                  _ptr(ascii), _ptr(twobit_off), _ptr(twobit),
                                                  _ptr(bad)))

    def last_kernel_ms(self):
        ms = C.c_float(0)
        self._check(self.lib.scrg_last_kernel_ms(self.h, C.byref(ms)))
        return float(ms.value)

    def debug_stats(self):
        out = (C.c_uint64 * 12)()
        self._check(self.lib.scrg_debug_stats(self.h, out))
        return {"rounds": int(out[0]), "dc_steps": int(out[1]), "tb_macro_steps": int(out[2]),
                "cycles_fetch": int(out[3]), "cycles_setup": int(out[4]), "cycles_dc": int(out[5]),
                "cycles_tb": int(out[6]), "cycles_tb_loop": int(out[7]), "diag_rounds": int(out[8]),
                "diag_fallbacks": int(out[9]), "cycles_diag_dc": int(out[10]), "cycles_diag_tb": int(out[11])}

    def debug_stats_lane(self):
        """The same counters as read by the one-pair-per-lane kernel (scrooge_amd.h: scrg_debug_stats): window rounds,
        rounds with a short text window, rounds that swept the band table / redid it on the full table / were eligible for it
        but left to the full table by the back-off, shader cycles per phase summed over wavefronts, wavefront life times on the
        100 MHz wall clock."""
        out = (C.c_uint64 * 12)()
        self._check(self.lib.scrg_debug_stats(self.h, out))
        o = [int(x) for x in out]
        big = 1 << 62
        m21 = (1 << 21) - 1
        # (genasm_lane_kernel packs its band counters into the first two words in fields of 21 bits, which do not saturate: the
        # figures hold for launches of up to 2 M window rounds — 100 k x 10 kb pairs are 0.52 M, 40 k x 50 kb 1.04 M — and above
        # that the fields run into each other.  The other lane kernels have no band counters, and their second word is read
        # through the same 21-bit mask: the same limit holds for their short-text rounds.)
        return {"rounds": o[0] & 0xffffffff, "band_backed_off_rounds": o[0] >> 32, "short_text_rounds": o[1] & m21,
                "band_rounds": (o[1] >> 21) & m21, "band_redone_rounds": o[1] >> 42, "cycles_pass1": o[2], "cycles_fetch": o[3], "cycles_setup": o[4],
                "cycles_table": o[5], "cycles_traceback": o[6], "life_ticks_sum": o[7], "last_start": o[8],
                "first_start": big - o[9], "last_end": o[10], "first_end": big - o[11]}

    def resolved_params(self, **kw):
        """The parameters a launch with these overrides will really use (defaults filled in)."""
        out = Params()
        st = self.lib.scrg_params_resolve(C.byref(self._params(kw)), C.byref(out))
        if st != SCRG_OK:
            raise ScroogeError(st, "invalid parameters")
        return out

    def query_launch(self, **kw):
        a, b, c, d = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        self._check(self.lib.scrg_query_launch(self.h, C.byref(self._params(kw)), C.byref(a),
                                               C.byref(b), C.byref(c), C.byref(d)))
        return {"n_waves": a.value, "pairs_per_wave": b.value, "lds_bytes": c.value,
                "n_cus": d.value}
