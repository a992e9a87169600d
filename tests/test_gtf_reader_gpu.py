"""The GTF reader's device form (sbgpu_gtf_read_device, csrc/gtf_device.h) against its host form: every array, status, name and
info word exact -- on the goldens, on the hand-written file of every rule and the seeded random files of tests/gtf_util.py
(which tests/test_gtf_reader.py holds to the restatement on the CPU), and at every threshold sbgpu_gtf_limits reports: line
counts around a wave's tile, the scan's round and the grid's passes, a tile at the staging limit, a line at the device's longest,
the sixteen alignments of the buffer, a file that ends on its last line's last byte, transcripts of 1 to 1 000 exons, a forced
hash collision, and the upload form."""
import glob
import os

import numpy as np
import pytest

import e2e_util
import gtf_util as U
from strawberry_amd import _lib, gtf

pytestmark = pytest.mark.gpu

HAND = U.hand_files()


@pytest.fixture(scope="module")
def LIM():
    """sbgpu_gtf_limits: the tests read their edges from the library (when they run, not when the module is collected)"""
    return gtf.limits()


@pytest.fixture(scope="module")
def ctx():
    from strawberry_amd import em
    return em.default_context(0)


def on_device(ctx, data, refs=None, shift=0, **kw):
    """The device form on `data` placed `shift` bytes into a device buffer."""
    import torch
    n = len(data)
    buf = torch.zeros(n + 64, dtype=torch.uint8, device="cuda:%d" % ctx.device)
    assert buf.data_ptr() % 16 == 0
    if n:
        buf[shift:shift + n] = torch.from_numpy(np.frombuffer(bytes(data), np.uint8).copy()).to(buf.device)
    view = buf[shift:shift + n]
    assert n == 0 or view.data_ptr() % 16 == shift % 16
    return gtf.read_gtf(view, ref_names=refs, ctx=ctx, **kw)


def both(ctx, data, refs=None, shift=0):
    host = gtf.read_gtf(data, ref_names=refs)
    dev = on_device(ctx, data, refs, shift)
    U.assert_same(dev, host)
    return host


def lines_file(n, seed, tail_newline=True):
    """n lines: about one in eight an exon line of one of 40 transcripts, the others comments, short lines and CDS lines."""
    rng = np.random.default_rng(seed)
    kind = rng.integers(0, 16, n)
    pos = rng.integers(1, 100000, n)
    tx = rng.integers(0, 40, n)
    junk = [b"#", b"# c", b"x", b"", b"short\tline"]
    out = []
    for k in range(n):
        if kind[k] < 2:
            out.append(U.exon_line("chr%d" % (tx[k] % 3), int(pos[k]), int(pos[k]) + 50, "+-"[tx[k] % 2], "g%d" % (tx[k] // 4), "t%d" % tx[k]))
        elif kind[k] == 2:
            out.append(U.exon_line("chr1", int(pos[k]), int(pos[k]) + 50, "+", "g", "t", kind="CDS"))
        else:
            out.append(junk[kind[k] % 5])
    return b"\n".join(out) + (b"\n" if tail_newline else b"")


# ---------------------------------------------------------------- content
@pytest.mark.parametrize("directory", sorted(glob.glob(os.path.join(e2e_util.HERE, "golden", "e2e_toy*"))), ids=os.path.basename)
def test_goldens(ctx, directory):
    assert both(ctx, open(os.path.join(directory, "toy.gtf"), "rb").read()).n_loci > 0


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_written_files(ctx, name):
    data, refs = HAND[name]
    host = both(ctx, data, refs)
    U.assert_matches(host, U.restate(data, refs))


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_seeded_random_files(ctx, seed):
    data = U.random_gtf(seed, long_attrs=seed == 3)
    assert both(ctx, data).n_loci == 300
    both(ctx, data, refs=["chr2", "CHR1", "chrUn"])


# ---------------------------------------------------------------- line counts
# T: a wave's tile of lines; R: the lines of one round of the scan over the tiles' totals; G: the lines of one pass of the grid
LINE_COUNTS = {"1": lambda T, R, G: 1, "T-1": lambda T, R, G: T - 1, "T": lambda T, R, G: T, "T+1": lambda T, R, G: T + 1,
               "R-T": lambda T, R, G: R - T, "R": lambda T, R, G: R, "R+1": lambda T, R, G: R + 1, "2R": lambda T, R, G: 2 * R,
               "2R+1": lambda T, R, G: 2 * R + 1, "2G+1": lambda T, R, G: 2 * G + 1}


@pytest.mark.parametrize("which", list(LINE_COUNTS))
def test_line_counts(ctx, LIM, which):
    n = LINE_COUNTS[which](LIM["tile_lines"], LIM["tile_lines"] * LIM["scan_tile"], LIM["tile_lines"] * LIM["grid_cap"])
    host = both(ctx, lines_file(n, seed=n % 97))
    assert host.info["lines"] == n and (n < 64 or host.info["lines_ok"] > 0)


def test_index_tiles_beyond_one_scan_round(ctx, LIM):
    """More tiles of the line index than one round of the scan takes, from few lines: comments near the device's longest line."""
    n_tiles = LIM["scan_tile"] + 2
    filler = b"#" + b"c" * (LIM["max_line"] - 1000)
    lines = [filler] * (n_tiles * LIM["index_tile"] // len(filler) + 4)
    lines[3] = U.exon_line("chr1", 10, 20, "+", "g", "t")
    lines[-1] = U.exon_line("chr1", 30, 40, "+", "g", "t")
    data = b"\n".join(lines) + b"\n"
    assert len(data) > n_tiles * LIM["index_tile"]
    host = both(ctx, data)
    assert host.info["lines_ok"] == 2 and host.info["exons"] == 2


# ---------------------------------------------------------------- line and tile sizes
def padded_tile(total):
    """64 exon lines whose bytes, newlines included, are `total`."""
    lines = [U.exon_line("chr1", 100 * k + 1, 100 * k + 50, "+", "g", "t%d" % (k % 5)) for k in range(64)]
    short = total - sum(len(l) + 1 for l in lines)
    assert short > 20
    lines[63] = lines[63] + b' note "' + b"p" * (short - 9) + b'";'
    data = b"\n".join(lines) + b"\n"
    assert len(data) == total
    return data


@pytest.mark.parametrize("over", [0, 1])
def test_a_tile_at_the_staging_limit_and_one_byte_above(ctx, LIM, over):
    first = padded_tile(LIM["stage_limit"] + over)
    host = both(ctx, first + lines_file(100, seed=5))
    assert host.line_status[:64].tolist() == [U.OK] * 64
    both(ctx, first + lines_file(100, seed=5), shift=15)


def long_line(n):
    line = U.exon_line("chr1", 100, 200, "+", "g", "t")
    return line + b' note "' + b"q" * (n - len(line) - 9) + b'";'


def test_a_line_at_the_longest_and_one_byte_above(ctx, LIM):
    at = long_line(LIM["max_line"])
    assert len(at) == LIM["max_line"]
    # (the one '\r' in front of the '\n' is not the line's: a CRLF line of the longest length is taken too)
    data = lines_file(70, seed=6) + at + b"\n" + U.exon_line("chr1", 300, 400, "+", "g", "t") + b"\n" + at + b"\r\n"
    host = both(ctx, data)
    assert host.line_status[70] == U.OK and host.line_status[72] == U.OK and host.info["exons"] >= 2
    with pytest.raises(_lib.SbgpuError, match="a line of more than %d bytes" % LIM["max_line"]):
        on_device(ctx, long_line(LIM["max_line"] + 1) + b"\r\n")
    over = lines_file(70, seed=6) + long_line(LIM["max_line"] + 1) + b"\n"
    assert gtf.read_gtf(over).line_status[70] == U.OK        # the host form takes any line
    with pytest.raises(_lib.SbgpuError, match="a line of more than %d bytes" % LIM["max_line"]):
        on_device(ctx, over)


# ---------------------------------------------------------------- alignment and file end
@pytest.mark.parametrize("shift", range(16))
def test_every_alignment_of_the_buffer(ctx, shift):
    both(ctx, lines_file(300, seed=7, tail_newline=shift % 2 == 0), shift=shift)


def test_last_line_without_newline_ends_on_the_last_byte(ctx):
    import torch
    data = lines_file(200, seed=8) + U.exon_line("chrL", 7, 9, "-", "glast", "tlast")
    d = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).to("cuda:%d" % ctx.device)
    assert d.numel() == len(data)
    dev, host = gtf.read_gtf(d, ctx=ctx), gtf.read_gtf(data)
    U.assert_same(dev, host)
    assert host.line_status[-1] == U.OK and b"tlast" in host.transcript_id and host.info["lines"] == 201


# ---------------------------------------------------------------- transcript sizes
@pytest.mark.parametrize("n_exons", [1, 2, 65, 1000])
def test_transcript_sizes(ctx, n_exons):
    rng = np.random.default_rng(n_exons)
    lines = [U.exon_line("chr1", 1000 * k + 1, 1000 * k + int(rng.integers(10, 1200)), "+", "big", "tbig") for k in range(n_exons)]
    lines += [U.exon_line("chr1", 50, 60, "+", "small", "tsmall")]
    order = rng.permutation(len(lines))
    host = both(ctx, b"\n".join(lines[k] for k in order) + b"\n")
    assert host.info["transcripts"] == 2 and host.info["exons"] + host.info["merged_exons"] == n_exons + 1


def test_5000_single_exon_transcripts(ctx):
    lines = [U.exon_line("chr%d" % (k % 7), 10 * k + 1, 10 * k + 5, "+-"[k % 2], "g%d" % (k // 3), "t%d" % k) for k in range(5000)]
    host = both(ctx, b"\n".join(lines) + b"\n")
    assert host.info["transcripts"] == 5000 and host.info["exons"] == 5000


# ---------------------------------------------------------------- refusals and upload
def test_a_hash_collision_is_refused_by_its_text(ctx):
    lines = [U.exon_line("chr1", 10 * k + 1, 10 * k + 5, "+", "g%d" % k, "t%d" % k) for k in range(300)]
    data = b"\n".join(lines) + b"\n"
    with pytest.raises(_lib.SbgpuError, match="collision"):
        on_device(ctx, data, hash_bits=8)
    U.assert_same(on_device(ctx, data, hash_bits=48), gtf.read_gtf(data))
    assert gtf.read_gtf(data, hash_bits=8).info["transcripts"] == 300   # the host form compares bytes: no hash to collide


def test_upload_equals_the_device_form(ctx):
    data = U.random_gtf(9, n_genes=60)
    up = gtf.read_gtf(data, ctx=ctx)
    U.assert_same(up, on_device(ctx, data))
    U.assert_same(up, gtf.read_gtf(data))
    U.assert_same(gtf.read_gtf(b"", ctx=ctx), gtf.read_gtf(b""))
    U.assert_same(gtf.read_gtf(b"# only\n", ctx=ctx), gtf.read_gtf(b"# only\n"))
