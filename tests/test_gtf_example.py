"""examples/gtf_annotation.cpp: it compiles as C++14 against include/sbgpu_host.hpp, and its output for the two-chromosome
golden is the `loci` section that the restatement of tests/gtf_util.py writes.  No GPU (the host form)."""
import os
import subprocess

import pytest

import e2e_util
import gtf_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "strawberry_amd", "lib")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    from strawberry_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    out = str(tmp_path_factory.mktemp("gtf_example") / "gtf_annotation")
    r = subprocess.run(["g++", "-std=c++14", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "examples", "gtf_annotation.cpp"), "-L" + LIBDIR, "-lsbgpu", "-Wl,-rpath," + LIBDIR, "-o", out],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return out


def loci_lines(want):
    out = ["loci %d" % len(want["loci"])]
    for locus in want["loci"]:
        out.append("locus %s %d %s %s" % (locus["gene_id"].decode(), len(locus["isoforms"]), ".+-"[locus["strand"]], want["chrom"][locus["chrom"]].decode()))
        for t, _, _, exons in locus["isoforms"]:
            out.append("iso %s %d %s" % (t.decode(), len(exons), " ".join("%d %d" % e for e in exons)))
    return out


@pytest.mark.parametrize("refs", [[], ["chr2", "CHR1"]], ids=["first_appearance", "table"])
def test_output_is_the_loci_section(program, refs):
    path = os.path.join(e2e_util.E2E_CHROMS, "toy.gtf")
    r = subprocess.run([program, path] + refs, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    want = U.restate(open(path, "rb").read(), refs or None)
    assert r.stdout.splitlines() == loci_lines(want)
    assert len(want["chrom"]) == 2 and "6 loci" in r.stderr


def test_a_missing_file_fails_by_its_text(program):
    r = subprocess.run([program, "/nonexistent.gtf"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "cannot open" in r.stderr
