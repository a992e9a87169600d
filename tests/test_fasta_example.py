"""examples/fasta_genome.cpp: it compiles as C++14 against include/sbgpu_host.hpp, and prints a file's .fai -- the golden genome's
line, which tools/make_e2e_golden.py wrote for the reference to read, and a three-contig file's.  No GPU (the host form)."""
import os
import subprocess

import pytest

import fasta_util as FU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "strawberry_amd", "lib")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    from strawberry_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    out = str(tmp_path_factory.mktemp("fasta_example") / "fasta_genome")
    r = subprocess.run(["g++", "-std=c++14", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "examples", "fasta_genome.cpp"), "-L" + LIBDIR, "-lsbgpu", "-Wl,-rpath," + LIBDIR, "-o", out],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return out


def test_the_golden_genome(program):
    path = os.path.join(ROOT, "tests", "golden", "e2e_toy_bias", "genome.fa")
    r = subprocess.run([program, path], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    length = len(FU.restate(open(path, "rb").read())["seqs"][0])
    assert r.stdout == "chr1\t%d\t6\t60\t61\n" % length and "1 contigs" in r.stderr


def test_three_contigs(program, tmp_path):
    s = FU.bases(300, 4)
    data = b">one first\n" + FU.wrap(s[:130], 60) + b">two\r\n" + FU.wrap(s[130:200], 25, b"\r\n") + b">hollow\n>three\n" + s[200:] + b"\n\n"
    path = tmp_path / "three.fa"
    path.write_bytes(data)
    r = subprocess.run([program, str(path)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    assert r.stdout == "one\t130\t11\t60\t61\ntwo\t70\t150\t25\t27\nthree\t100\t241\t100\t101\n" == FU.fai_of(FU.restate(data))
    assert "4 contigs" in r.stderr and "1 empty" in r.stderr


def test_failures_by_their_text(program, tmp_path):
    r = subprocess.run([program, "/nonexistent.fa"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "cannot open" in r.stderr
    path = tmp_path / "ragged.fa"
    path.write_bytes(b">r\nACGT\nACGTA\n")
    r = subprocess.run([program, str(path)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "'r'" in r.stderr and r.stdout == ""
    path.write_bytes(b"ACGT\n>r\nAC\n")
    r = subprocess.run([program, str(path)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "offset 0" in r.stderr
