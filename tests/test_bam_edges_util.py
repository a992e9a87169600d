"""The samples of tests/bam_edges_util.py, on the CPU: stage_limits against csrc/front_schedule.h itself (a stand-alone C++
program under AddressSanitizer and UBSan that includes that header alone), every sample's reason for being there, seen
through the oracle alone, and the library's host decode -- the device's decoder body, through ByteLoads -- against the
oracle on every sample.  tests/test_bamdecode_edges_gpu.py decodes the same streams on the device."""
import os
import subprocess

import numpy as np
import pytest

import bam_edges_util as E
from test_bamdecode import check_library_against_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""#include "front_schedule.h"
#include <cstdio>
#include <cstdlib>
// arguments: n n_bytes lds_max one_pass_limit scan_limit, five at a time
int main(int argc, char **argv)
{
   if (argc < 6 || (argc - 1) % 5) return 2;
   for (int k = 1; k + 4 < argc; k += 5) {
      const long long n = std::atoll(argv[k]), n_bytes = std::atoll(argv[k + 1]), lds = std::atoll(argv[k + 2]);
      const sb::BamOnepassLaunch p = sb::bam_onepass_launch(n, n_bytes, (int)lds, 256);
      const sb::BamScanLaunch q = sb::bam_scan_launch(n, n_bytes, (int)lds, 256);
      if (p.stage_bytes - 16 != std::atoll(argv[k + 3]) || q.stage_bytes - 16 != std::atoll(argv[k + 4]) || p.block_cap != 2 * n + 1024) {
         std::printf("n %lld, %lld bytes, %lld of LDS: the header stages up to %d and %d bytes\n", n, n_bytes, lds, p.stage_bytes - 16, q.stage_bytes - 16);
         return 1;
      }
   }
   std::printf("ok\n");
   return 0;
}
"""


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    d = tmp_path_factory.mktemp("bam_stage_limits_cpp")
    src, exe = d / "stage_limits.cpp", d / "stage_limits"
    src.write_text(PROGRAM)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "strawberry_amd", "csrc"), str(src), "-o", str(exe)])
    return exe


def test_stage_limits_equal_the_header(program):
    s = E.staging_sweep()
    # by hand from front_schedule.h: the floors (36-byte records), the caps at 64 KB and at 160 KB (1 KB records), in between
    # (200-byte records), the sweep's average (120: 64 * 121 * 26 / 25 + 767 = 8820 -> 8704; 70 * 121 = 8470 -> 8 KB + 2 KB)
    by_hand = {(1000000, 36000000, 65536): (4096 - 16, 8192 - 16), (1000000, 1024000000, 65536): (16128 - 16, 65280 - 16),
               (1000000, 1024000000, 160 * 1024): (32768 - 16, 65536 - 16), (1 << 20, 200 << 20, 65536): (14080 - 16, 14336 - 16),
               (1000, 100000, 512): (-16, 256 - 16), (1000, 100000, 100): (-16, -16), (1, 120, 65536): (8688, 10224)}
    for k, want in by_hand.items():
        assert E.stage_limits(*k) == want, k
    points = list(by_hand) + [(s.n, s.raw.size, lds) for lds in E.LDS_SIZES]
    points += [(1, 36, 65536), (1000, 100000, 1000), (1000, 100000, 256), (7, 7 * 515, 65536), (64, 64 * 468, 40000), (64, 64 * 469, 40000),
               (1 << 20, 117 << 20, 65536), (1 << 20, 146 << 20, 160 * 1024), ((1 << 31) - 3, 36 * ((1 << 31) - 3), 65536)]
    args = [str(v) for p in points for v in p + E.stage_limits(*p)]
    out = subprocess.run([str(program)] + args, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "ok", (out.stdout[-2000:], out.stderr[-2000:])


def test_sweep_brackets_both_limits_at_every_alignment(oracle):
    s = E.staging_sweep()
    limits, groups = s.info["limits"], s.info["groups"]
    for lds in E.LDS_SIZES:                      # whatever the device grants a workgroup
        assert E.stage_limits(s.n, s.raw.size, lds) == limits
    assert limits == (8688, 10224)               # (by hand in the test above; the builder computed them)
    assert s.n == E.GROUP * len(groups) and [g[0] for g in groups] == list(range(0, s.n, E.GROUP))
    start = s.off[::E.GROUP]
    np.testing.assert_array_equal(np.diff(start), [g[1] for g in groups])          # every group as long as intended
    o = E.oracle_of(oracle, s)
    for T in limits:
        assert {g[1] for g in groups if g[2] is None and g[3] is not None and abs(g[1] - T) <= 17} == set(range(T - 17, T + 18))
        for d in (0, 1):
            assert sorted(int(start[i]) & 15 for i, g in enumerate(groups) if g[2] is not None and g[1] == T + d) == list(range(16))
    n_tagged = [0, 0, 0]
    for i, (first, length, align, nh) in enumerate(groups):
        if align is not None:
            assert int(start[i]) & 15 == align
        if nh is None:
            continue
        last = first + E.GROUP - 1
        # the tags are the last bytes of the range and of the record in front
        tail = bytes(s.raw[s.off[last + 1] - 7:s.off[last + 1]])
        assert tail[-4:] == b"NHC" + bytes([nh]) or tail == b"NHi" + bytes([nh, 0, 0, 0])
        assert bytes(s.raw[s.off[last] - 4:s.off[last]]) == b"XSA-"
        assert o["status"][last] == (0 if nh == 1 else 9) and o["nh"][last] == nh
        assert o["status"][last - 1] == 0 and o["strand"][last - 1] == 2
        n_tagged[nh] += 1
    assert n_tagged[1] == n_tagged[2] == (len(groups) - sum(g[3] is None for g in groups)) // 2
    both = E.oracle_of(oracle, s, unique_only=False, library=1)
    assert int((both["status"] == 9).sum()) == 0 and int((o["status"] == 9).sum()) == n_tagged[2]
    assert E.blocks_per_record(o).sum() <= E.block_cap(s.n) and E.blocks_per_record(o).max() == 4


def test_samples_have_the_property_they_were_built_for(oracle):
    for s in E.capacity_edges():
        o = E.oracle_of(oracle, s)
        nb = E.blocks_per_record(o)
        assert s.n == E.CAP_N and int(nb.sum()) == s.info["blocks"]
    a, b, c, d = E.capacity_edges()
    cap = E.block_cap(E.CAP_N)
    assert [x.info["blocks"] - cap for x in (a, b, c, d)] == [0, 1, 1, 0]
    nb = [E.blocks_per_record(E.oracle_of(oracle, x)) for x in (a, b, c, d)]
    assert nb[1][:E.TILE].sum() == nb[0][:E.TILE].sum() + 1 and nb[2][-1] == nb[0][-1] + 1 and (nb[2][:-1] == nb[0][:-1]).all()
    assert (E.oracle_of(oracle, d)["status"][-64:] == 1).all() and (E.oracle_of(oracle, d)["status"][:-64] == 0).all()
    for s in E.sparse_tiles():
        o = E.oracle_of(oracle, s)
        assert s.n == 6 * E.TILE
        assert ((o["status"] == 0).reshape(6, E.TILE).sum(1) == s.info["per_tile"]).all() and set(np.unique(o["status"])) <= {0, 1}
        assert E.blocks_per_record(o).sum() <= E.block_cap(s.n)
    per_tile = {s.name: s.info["per_tile"] for s in E.sparse_tiles()}
    assert per_tile["tiles_0_and_5"] == [1024, 0, 0, 0, 0, 1024] and per_tile["none"] == [0] * 6
    assert per_tile["first_only"] == [1, 0, 0, 0, 0, 0] and per_tile["last_only"] == [0, 0, 0, 0, 0, 1]
    assert per_tile["only_1023"] == [1, 0, 0, 0, 0, 0] and per_tile["only_1024"] == per_tile["only_1025"] == [0, 1, 0, 0, 0, 0]
    s = E.slow_head()
    o = E.oracle_of(oracle, s)
    assert (o["status"] == 0).all() and (E.blocks_per_record(o) == 1).all()        # the first tile and all behind it
    assert (np.diff(o["cig_off"])[:E.TILE] == 1).all() and (s.sizes[:E.TILE] > 4 * E.SLOW_OPS).all()   # (pads are not kept)
    assert s.n >= 131 * E.TILE and s.n // E.TILE - 1 > 2 * 64 and s.raw.size < 15 << 20
    assert (s.sizes[:E.TILE].reshape(-1, 64).sum(1) > 65536).all()                 # no buffer holds a pass of them
    s = E.block_counts()
    o = E.oracle_of(oracle, s)
    nb = E.blocks_per_record(o)
    big = s.info["big"]
    assert nb[big] == 32768 and s.sizes[big] > 4 * E.BIG_OPS and int(o["left"][big]) + 32768 + 32767 * 25 - 1 == int(o["right"][big]) < 2 ** 32
    assert nb[big - 1] == 500 and (o["status"][:s.info["n_special"]] == 0).all()
    first = nb[:4 * E.GROUP].reshape(4, E.GROUP)
    assert all(sorted(p.tolist()) == sorted(list(range(1, 9)) * 8) for p in first)
    assert len(set(zip(first[0][:-1].tolist(), first[0][1:].tolist()))) == 63          # every ordered pair of counts but one
    assert int(nb.sum()) <= E.block_cap(s.n)                                           # the one pass has room for it


@pytest.mark.parametrize("kw", [dict(), dict(unique_only=False, library=1)], ids=["default", "multi_fr"])
def test_host_decode_equals_oracle_on_the_sweep(oracle, kw):
    from strawberry_amd import bam
    s = E.staging_sweep()
    d = bam.decode(s.raw, s.off, bam.BamOptions(n_ref=E.N_REF, **kw))
    check_library_against_oracle(d, E.oracle_of(oracle, s, **kw))
    d.close()


def test_host_decode_equals_oracle_on_every_sample(oracle):
    from strawberry_amd import bam
    for s in E.all_samples()[1:]:
        d = bam.decode(s.raw, s.off, bam.BamOptions(n_ref=E.N_REF))
        check_library_against_oracle(d, E.oracle_of(oracle, s))
        d.close()
    none = bam.decode(E.sparse_tiles()[3].raw, None, bam.BamOptions(n_ref=E.N_REF))
    assert none.n_reads == 0 and none.block_off.tolist() == [0]


def test_host_decode_equals_oracle_on_the_count_prefixes(oracle):
    from strawberry_amd import bam
    s = E.count_edges()
    o = E.oracle_of(oracle, s)
    assert s.info["counts"][-1] == s.n == 66 * 1024 + 63
    for n in s.info["counts"]:
        d = bam.decode(s.raw[:s.off[n]], s.off[:n + 1], bam.BamOptions(n_ref=E.N_REF))
        check_library_against_oracle(d, E.oracle_prefix(o, n))
        d.close()
        assert E.blocks_per_record(o)[:n].sum() <= E.block_cap(n)          # the one pass has room for every prefix
    assert set(np.unique(o["status"])) >= {0, 1, 3, 4, 5, 6, 7, 8, 9}
