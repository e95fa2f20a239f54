"""Seeding at the front door (CPU): a job loaded without a seeds file, and the command line's argument errors."""
import ctypes as C

import pytest

import scrooge_amd
from scrooge_amd import api, cli
from scrooge_amd import io as sio
from tests.test_io import make_dataset


def test_unseeded_job_has_the_reads_and_no_pairs(tmp_path):
    scrooge_amd.build_library()
    fa, fq, seeds, chroms, truth = make_dataset(str(tmp_path))
    seeded = sio.Job(fa, fq, seeds, reverse_strand=1)
    job = sio.Job(fa, fq)
    assert (job.n_reads, job.n_pairs, job.genome_len, job.n_chromosomes) == (len(truth), 0, sum(len(s) for _, s in chroms), len(chroms))
    g0, r0, c0, n0 = seeded.views()
    g1, r1, c1, n1 = job.views()
    assert (g1, r1, n1) == (g0, r0, n0) and c1 == [[] for _ in truth]          # the same genome and reads in the same (longest first) order
    assert job.genome().upper() == b"".join(s for _, s in chroms)
    capped = sio.Job(fa, fq, None, read_length_cap=100, inflation=2)
    assert capped.n_reads == 2 * len(truth) and capped.n_pairs == 0 and max(len(r) for r in capped.views()[1]) == 100


def test_unseeded_load_errors_and_the_seeded_one_stays(tmp_path):
    lib = sio._lib()
    fa, fq, seeds, _, _ = make_dataset(str(tmp_path))
    with pytest.raises(api.ScroogeError) as e:
        sio.Job(str(tmp_path / "none.fa"), fq)
    assert e.value.status == sio.SCRG_ERR_IO and "none.fa" in str(e.value)
    with pytest.raises(api.ScroogeError) as e:
        sio.Job(fa, str(tmp_path / "none.fq"))
    assert e.value.status == sio.SCRG_ERR_IO
    empty = tmp_path / "empty.fa"
    empty.write_text("")
    with pytest.raises(api.ScroogeError) as e:
        sio.Job(str(empty), fq)
    assert e.value.status == sio.SCRG_ERR_FORMAT
    # scrg_job_load with a NULL seeds path is the error it was
    h, err = C.c_void_p(), C.create_string_buffer(256)
    assert lib.scrg_job_load(fa.encode(), fq.encode(), None, None, C.byref(h), err, len(err)) == api.SCRG_ERR_INVALID_ARG and not h.value
    assert lib.scrg_job_load_unseeded(fa.encode(), None, None, C.byref(h), err, len(err)) == api.SCRG_ERR_INVALID_ARG
    assert lib.scrg_job_seed(None, None, None) == api.SCRG_ERR_INVALID_ARG


def test_cli_argument_errors(capsys):
    files = ["--reference=none.fa", "--reads=none.fq"]
    for bad, word in ((["--seeds=none.paf", "--seed_rule=13,4,64,32,2,4"], "--seeds"),
                      (["--seed_rule=13,4,64,32,2"], "K,STRIDE"), (["--seed_rule=13,4,64,32,2,4,3"], "K,STRIDE"), (["--seed_rule=a,4,64,32,2,4"], "K,STRIDE"),
                      (["--seed_rule=7,4,64,32,2,4"], "K,STRIDE"), (["--seed_rule=17,4,64,32,2,4"], "K,STRIDE"), (["--seed_rule=13,0,64,32,2,4"], "K,STRIDE"),
                      (["--seed_rule=13,65,64,32,2,4"], "K,STRIDE"), (["--seed_rule=13,4,0,32,2,4"], "K,STRIDE"), (["--seed_rule=13,4,65536,32,2,4"], "K,STRIDE"),
                      (["--seed_rule=13,4,64,65536,2,4"], "K,STRIDE"), (["--seed_rule=13,4,64,32,0,4"], "K,STRIDE"), (["--seed_rule=13,4,64,32,2,0"], "K,STRIDE"),
                      (["--seed_rule=13,4,64,32,2,65"], "K,STRIDE")):
        with pytest.raises(SystemExit) as e:
            cli.main(files + bad)
        assert e.value.code == 2
        assert word in capsys.readouterr().err
    # a good rule and no seeds file pass the arguments: what fails is the missing FASTA
    with pytest.raises(api.ScroogeError) as e:
        cli.main(files + ["--seed_rule=13,4,64,32,2,4"])
    assert e.value.status == sio.SCRG_ERR_IO
    with pytest.raises(api.ScroogeError) as e:
        cli.main(files)
    assert e.value.status == sio.SCRG_ERR_IO
