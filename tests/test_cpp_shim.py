"""The header-only C++ shim (include/scrooge_amd.hpp) keeps the reference's
align_all signatures (src/genasm_gpu.hpp:7-8): it must compile with plain g++
against the C ABI, and on a GPU produce the reference's answers."""
import os
import subprocess

import pytest

import scrooge_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPECTED = [
    "pairwise cigar=7= edit_distance=0",
    "pairwise cigar=4=4D4=4I4= edit_distance=8",
    "pairwise_timed cigar=7= edit_distance=0",
    "pairwise_timed cigar=4=4D4=4I4= edit_distance=8",
    "pairwise_timed kernel_ns>0=1",
    "mapping cigar=7= edit_distance=0",
    "mapping cigar=3X4= edit_distance=3",
    "mapping cigar=12= edit_distance=0",
    "mapping_timed cigar=7= edit_distance=0",
    "mapping_timed cigar=3X4= edit_distance=3",
    "mapping_timed cigar=12= edit_distance=0",
    "mapping_timed kernel_ns>0=1",
    "resident cigar=7= edit_distance=0",
    "resident cigar=3X4= edit_distance=3",
    "resident cigar=12= edit_distance=0",
    "resident cigar=12= edit_distance=0",
]


def build_example(exe):
    scrooge_amd.build_library()
    libdir = os.path.join(ROOT, "scrooge_amd")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "library_example.cpp"),
                           "-L" + libdir, "-lscrooge_amd", "-Wl,-rpath," + libdir, "-o", exe])


def test_shim_compiles_with_gxx_and_fails_loudly_without_gpu(tmp_path):
    exe = str(tmp_path / "library_example")
    build_example(exe)
    lib = scrooge_amd.load_library()
    if lib.scrg_device_count() > 0:
        pytest.skip("GPU present; covered by the gpu test")
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 2
    assert "no usable HIP device" in p.stderr


@pytest.mark.gpu
def test_shim_matches_reference_answers(tmp_path):
    exe = str(tmp_path / "library_example")
    build_example(exe)
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    assert p.stdout.strip().splitlines() == EXPECTED


@pytest.mark.gpu
def test_shim_converts_large_results_in_parallel(tmp_path):
    """More than 8 MB of CIGAR text: the strings of the reference's result type are filled by several threads
    (include/scrooge_amd.hpp, detail::to_alignments); every pair against the C ABI's own arrays (tests/proto/shim_large.cpp)."""
    scrooge_amd.build_library()
    libdir = os.path.join(ROOT, "scrooge_amd")
    exe = str(tmp_path / "shim_large")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "proto", "shim_large.cpp"), "-L" + libdir, "-lscrooge_amd", "-Wl,-rpath," + libdir,
                           "-pthread", "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    out = p.stdout.strip()
    assert out.endswith("mismatches=0") and int(out.split("text_mb=")[1].split()[0]) >= 8, out


def build_pipeline_example(exe):
    scrooge_amd.build_library()
    libdir = os.path.join(ROOT, "scrooge_amd")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-std=c++17", "-Wall",
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "pipeline_example.cpp"),
                           "-L" + libdir, "-lscrooge_amd", "-Wl,-rpath," + libdir, "-o", exe])


def test_pipeline_example_builds(tmp_path):
    """examples/pipeline_example.cpp: the device-pointer layer driven from C++ over two handles and two
    streams."""
    build_pipeline_example(str(tmp_path / "pipeline_example"))


@pytest.mark.gpu
def test_pipeline_example_runs(tmp_path):
    exe = str(tmp_path / "pipeline_example")
    build_pipeline_example(exe)
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stdout.strip().endswith("mismatches=0")


# ------------------------------------------------------------------------------------------------ directed and anchored calls
def build_shim_anchored(exe):
    scrooge_amd.build_library()
    libdir = os.path.join(ROOT, "scrooge_amd")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "proto", "shim_anchored.cpp"), "-L" + libdir, "-lscrooge_amd", "-Wl,-rpath," + libdir,
                           "-pthread", "-o", exe])


def write_shim_case(path, genome, reads, locations):
    """locations[r]: list of (start, strand, leftward, anchor_read) — the case file of tests/proto/shim_anchored.cpp."""
    with open(path, "w") as f:
        f.write("%s\n%d\n" % (genome.decode(), len(reads)))
        for r, locs in zip(reads, locations):
            f.write("%s %d\n" % (r.decode() or "-", len(locs)))
            for loc in locs:
                f.write("%d %d %d %d\n" % tuple(loc))


def test_anchored_shim_compiles_with_gxx_and_fails_loudly_without_gpu(tmp_path):
    exe = str(tmp_path / "shim_anchored")
    build_shim_anchored(exe)
    if scrooge_amd.load_library().scrg_device_count() > 0:
        return                                         # (a GPU is present: test_shim_directed_and_anchored_calls runs the program)
    case = str(tmp_path / "case.txt")
    write_shim_case(case, b"TTTTACGTACGTTTTTAAAACCCCGGGGTTTT", [b"ACGTACG", b""], [[(4, 0, 0, 3), (11, 1, 1, 0)], [(0, 0, 1, 0)]])
    p = subprocess.run([exe, case], capture_output=True, text=True)
    assert p.returncode == 2
    assert "no usable HIP device" in p.stderr


@pytest.mark.gpu
def test_shim_directed_and_anchored_calls(tmp_path, oracle):
    """Handle::align_directed and Handle::align_anchored (with a text_start vector) against the resident genome, line by line
    against the oracle on explicitly reverse-complemented strings: 30 reads of the directed set and 30 of the anchored set of
    tests/anchored_inputs.py, a long one of each among them.  Every location serves both calls: the directed set's locations
    get a read position (7 x start mod (L + 1)), the anchored set's a direction (leftward every second one)."""
    from tests import anchored_inputs as ai
    d, a = ai.directed_inputs(oracle), ai.anchored_inputs(oracle)
    reads, locations = [], []
    for r in list(range(29)) + [ai.DIRECTED_READS]:
        L = len(d["reads"][r])
        reads.append(d["reads"][r])
        locations.append([(p, rv, lw, 7 * p % (L + 1)) for p, rv, lw in zip(d["cands"][r], d["rev"][r], d["left"][r])])
    for r in list(range(29)) + [ai.ANCHORED_READS]:
        reads.append(a["reads"][r])
        locations.append([(ga, rv, (k + r) & 1, ra) for k, ((ga, ra), rv) in enumerate(zip(a["anchors"][r], a["rev"][r]))])
    assert b"" in reads and sum(len(x) for x in locations) >= 100
    assert all(any(loc[1] == s and loc[2] == w for locs in locations for loc in locs) for s in (0, 1) for w in (0, 1))
    start = [[loc[0] for loc in locs] for locs in locations]
    rev = [[loc[1] for loc in locs] for locs in locations]
    left = [[loc[2] for loc in locs] for locs in locations]
    anchors = [[(loc[0], loc[3]) for loc in locs] for locs in locations]
    want_d = ai.directed_expectation(oracle, d["genome"], reads, start, rev, left)
    want_a = ai.anchored_expectation(oracle, d["genome"], reads, anchors, rev)
    expected = ["directed cigar=%s edit_distance=%d" % x for x in zip(want_d["cigars"], want_d["eds"])]
    expected += ["anchored cigar=%s edit_distance=%d text_start=%d" % x for x in zip(want_a["cigars"], want_a["ed"], want_a["text_start"])]
    expected += ["directed_wrong_size invalid_argument=1", "anchored_wrong_size invalid_argument=1"]
    exe, case = str(tmp_path / "shim_anchored"), str(tmp_path / "case.txt")
    build_shim_anchored(exe)
    write_shim_case(case, d["genome"], reads, locations)
    p = subprocess.run([exe, case], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    got = p.stdout.strip().splitlines()
    assert len(got) == len(expected)
    bad = [k for k in range(len(got)) if got[k] != expected[k]]
    assert not bad, [(k, got[k][:120], expected[k][:120]) for k in bad[:4]]
