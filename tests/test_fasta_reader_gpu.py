"""The FASTA reader's device form (sbgpu_fasta_read_device, csrc/fasta_device.h) against its host form: every array, flag, name,
info word and packed byte exact -- on the cases tests/test_fasta_reader.py holds to the restatement on the CPU, and at every
threshold sbgpu_fasta_limits reports (tests/test_fasta_util.py asserts that each generated file has the property it is named
for): buffer sizes around a tile, tile counts around a scan round and beyond two passes of the grid, headers at tile edges and
at the longest the device form takes, "\\r\\n" split across tiles, unwrapped contigs, many small contigs, the sixteen alignments
of the buffer, the upload form, and a file of more than 2^32 bytes built on the device."""
import numpy as np
import pytest

import fasta_util as FU
from strawberry_amd import _lib, fasta

pytestmark = pytest.mark.gpu

CASES = FU.cpu_cases()


@pytest.fixture(scope="module")
def LIM():
    return fasta.limits()


@pytest.fixture(scope="module")
def ctx():
    from strawberry_amd import em
    return em.default_context(0)


def on_device(ctx, data, shift=0):
    """The device form on `data` placed `shift` bytes into a device buffer."""
    import torch
    n = len(data)
    buf = torch.zeros(n + 64, dtype=torch.uint8, device="cuda:%d" % ctx.device)
    assert buf.data_ptr() % 16 == 0
    if n:
        buf[shift:shift + n] = torch.from_numpy(np.frombuffer(bytes(data), np.uint8).copy()).to(buf.device)
    view = buf[shift:shift + n]
    assert n == 0 or view.data_ptr() % 16 == shift % 16
    return fasta.read_fasta(view, ctx=ctx)


def assert_same(dev, host):
    assert dev.names == host.names
    for name in ("seq_off", "offset", "line_bases", "line_width", "flags"):
        np.testing.assert_array_equal(getattr(dev, name), getattr(host, name), err_msg=name)
    for k in fasta.INFO_KEYS[:10]:
        assert dev.info[k] == host.info[k], k
    assert dev.on_device == (host.info["bytes"] > 0) and not host.on_device
    np.testing.assert_array_equal(dev.packed(), host.packed())


def both(ctx, data, shift=0):
    host = fasta.read_fasta(data)
    dev = on_device(ctx, data, shift)
    assert_same(dev, host)
    return host


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_cpu_case(ctx, name):
    both(ctx, CASES[name])


@pytest.mark.parametrize("name", sorted(FU.refused_cases()))
def test_text_in_front_is_refused_with_its_offset(ctx, name):
    data, at = FU.refused_cases()[name]
    with pytest.raises(_lib.SbgpuError) as e:
        on_device(ctx, data)
    assert "(-1)" in str(e.value) and "offset %d" % at in str(e.value)
    # far into the file too: only empty lines in front, over several tiles
    far = b"\n" * 40000 + data
    with pytest.raises(_lib.SbgpuError) as e:
        on_device(ctx, far)
    assert "offset %d" % (at + 40000) in str(e.value)


@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_buffer_sizes_around_a_tile(ctx, LIM, delta):
    for tiles in (1, 2):
        both(ctx, FU.wrapped_file(tiles * LIM["tile"] + delta))
        both(ctx, FU.wrapped_file(tiles * LIM["tile"] + delta, width=59))


@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_tile_counts_around_a_scan_round(ctx, LIM, delta):
    n = (LIM["scan_tile"] + delta) * LIM["tile"]
    h = both(ctx, FU.blocks_file(n)[:n - 8] + b"\n>last\nA")
    assert -(-h.info["bytes"] // LIM["tile"]) == LIM["scan_tile"] + delta


def test_more_tiles_than_two_passes_of_the_grid(ctx, LIM):
    n = 2 * LIM["grid_cap"] * LIM["tile"] + 5 * LIM["tile"] + 11
    h = both(ctx, FU.blocks_file(n))
    assert h.info["bytes"] > 2 * LIM["grid_cap"] * LIM["tile"] + LIM["tile"] and h.info["contigs"] > 100 and h.info["ragged"] == 0


def test_headers_at_tile_edges(ctx, LIM):
    T = LIM["tile"]
    for pos in (T - 1, T, T + 1, 2 * T - 1):          # '>' is a tile's last byte, its first, its second
        h = both(ctx, FU.header_at(pos, b">edge of tile\n"))
        assert h.names[1] == b"edge" and h.offset[1] == pos + 14
    h = both(ctx, FU.header_at(T - 5, b">edge\n"))    # the header's '\n' is a tile's first byte
    assert h.offset[1] == T + 1
    h = both(ctx, FU.header_at(T - 5, b">straddling_name x\n"))
    assert h.names[1] == b"straddling_name"
    h = both(ctx, FU.header_at(T - 4, b">cr\r\n"))    # the header's "\r\n" split across tiles
    assert h.offset[1] == T + 1 and h.names[1] == b"cr"


def test_long_header_lines(ctx, LIM):
    T, M = LIM["tile"], LIM["max_header"]
    for ln in (T + 100, 2 * T + 100):
        h = both(ctx, FU.header_at(100, b">n " + b"d" * ln + b"\n"))
        assert h.names[1] == b"n"
        h = both(ctx, FU.header_at(100, b">" + b"N" * ln + b"\r\n", tail=b"AC\r\nG\r\n"))
        assert len(h.names[1]) == ln
    for term in (b"\n", b"\r\n", b""):
        at_limit = b">" + b"x" * (M - 1) + term
        both(ctx, b">a\nAC\n" + at_limit + (b"ACGT\n" if term else b""))
        above = b">a\nAC\n>" + b"x" * M + term + (b"ACGT\n" if term else b"")
        with pytest.raises(_lib.SbgpuError) as e:
            on_device(ctx, above)
        assert "(-6)" in str(e.value) and "header line" in str(e.value) and "host form" in str(e.value)
        assert fasta.read_fasta(above).info["contigs"] == 2       # the host form takes it


def test_terminators(ctx, LIM):
    T = LIM["tile"]
    for pos in (T, 2 * T):
        h = both(ctx, FU.crlf_split_at(pos))
        assert h.info["ragged"] == 0 and h.line_width[0] == 62
    both(ctx, b">a\nAC\rGT\nAC\rGT\n>b\n\rACG\nT\rAC\r\n")
    both(ctx, FU.header_at(T - 2, b">x\n", tail=b"ACG\rT\nACG\rT\n"))      # a lone '\r' next to the tile's edge
    both(ctx, b">a\n" + b"ACGT\r" * (T // 5) + b"\r\n")                       # lone '\r' at every phase of the chunks, one line


@pytest.mark.parametrize("final_newline", [True, False])
def test_unwrapped_contig_over_tiles(ctx, LIM, final_newline):
    for n in (3 * LIM["tile"] + 17, 5 * LIM["tile"]):
        h = both(ctx, FU.unwrapped(n, final_newline))
        assert h.length[1] == n and h.line_bases[1] == n and h.line_width[1] == n + (1 if final_newline else 0) and h.flags[1] == 0


def test_many_small_contigs(ctx, LIM):
    h = both(ctx, FU.many_contigs(5000, seed=11))
    assert h.info["contigs"] == 5000 and h.info["bytes"] / 5000 * 64 < LIM["tile"]     # a tile holds more than 64 headers
    assert h.info["ragged"] > 100


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_contig_counts_around_a_wave(ctx, n):
    assert both(ctx, FU.small_contigs(n)).info["contigs"] == n


@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_contig_counts_around_a_scan_round(ctx, LIM, delta):
    n = LIM["scan_tile"] + delta
    assert both(ctx, FU.small_contigs(n)).info["contigs"] == n
    assert both(ctx, FU.small_contigs(2 * LIM["scan_tile"] + delta)).info["contigs"] == 2 * LIM["scan_tile"] + delta


def test_sixteen_alignments(ctx, LIM):
    data = FU.many_contigs(300, seed=5) + FU.crlf_split_at(LIM["tile"]) + b">tail\nACGT"
    host = fasta.read_fasta(data)
    for shift in range(16):
        assert_same(on_device(ctx, data, shift), host)
        assert_same(on_device(ctx, data[:37], shift), fasta.read_fasta(data[:37]))


def test_upload_form(ctx):
    data = CASES["lf"] + FU.many_contigs(100, seed=2)
    up = fasta.read_fasta(data, ctx=ctx)
    assert up.on_device and up.info["device"] == ctx.device
    assert_same(up, fasta.read_fasta(data))
    assert fasta.read_fasta(CASES["lf"], ctx=ctx).fai_text() == fasta.read_fasta(CASES["lf"]).fai_text()     # (from a device handle too)
    assert up.fetch("chr2", 2, 5) == fasta.read_fasta(data).fetch("chr2", 2, 5)
    with pytest.raises(_lib.SbgpuError):
        up.fetch("chr2", 120, 2)
    empty = fasta.read_fasta(b"", ctx=ctx)
    assert empty.info["contigs"] == 0 and not empty.on_device


def test_past_two_to_the_32_bytes(ctx):
    """The file is built on the device by repeating a block of whole contigs whose length is prime to the tile; what is expected
    is arithmetic on the block."""
    import torch
    dev = torch.device("cuda", ctx.device)
    free, _ = torch.cuda.mem_get_info(dev)
    if free < 10 * 2 ** 30:
        pytest.skip("the device has less than 10 GB free")
    block = b">p\n" + FU.wrap((b"ACGTTGCAAC" * 30001)[:300007], 60) + b">q r\n" + FU.wrap((b"GGATCCTTAA" * 20001)[:200003], 70)
    assert len(block) % 2 == 1
    hb = fasta.read_fasta(block)
    reps = 2 ** 32 // len(block) + 2
    d_block = torch.from_numpy(np.frombuffer(block, np.uint8).copy()).to(dev)
    big = d_block.repeat(reps)
    assert big.numel() > 2 ** 32
    g = fasta.read_fasta(big, ctx=ctx)
    del big
    nb = int(hb.seq_off[-1])
    assert g.n_contigs == 2 * reps and g.info["bytes"] == reps * len(block) and g.info["bases"] == reps * nb and g.info["ragged"] == 0
    k = np.arange(reps, dtype=np.int64)
    for c in (0, 1):
        np.testing.assert_array_equal(g.seq_off[c:-1:2], k * nb + hb.seq_off[c])
        np.testing.assert_array_equal(g.offset[c::2], k * len(block) + hb.offset[c])
        assert (g.line_bases[c::2] == hb.line_bases[c]).all() and (g.line_width[c::2] == hb.line_width[c]).all() 
        assert g.flags[c] == 0 and (g.flags[c + 2::2] == FU.DUPLICATE).all()       # (the block's names come again)
    assert g.names[:2] == [b"p", b"q"] and g.names[-2:] == [b"p", b"q"]
    spots = {0, 1, g.n_contigs - 2, g.n_contigs - 1}
    for edge in (2 ** 31, 2 ** 32):
        c = int(np.searchsorted(g.offset, edge))
        spots |= {c - 2, c - 1, c, c + 1}
    for c in sorted(spots):
        want = hb.sequence(c % 2)
        assert g.fetch(c, 1, 500) == want[:500] and g.fetch(c, len(want) - 499, 500) == want[-500:] and g.fetch(c, 150001, 77) == want[150000:150077]
    # one device-side sum over the packed bytes
    ptr, is_dev = g.sequence_pointer()
    assert is_dev

    class Packed:
        __cuda_array_interface__ = {"shape": (reps * nb,), "typestr": "|u1", "data": (ptr, False), "version": 2}
    total = int(torch.as_tensor(Packed(), device=dev).sum(dtype=torch.int64).item())
    assert total == reps * int(hb.packed().sum(dtype=np.int64))
