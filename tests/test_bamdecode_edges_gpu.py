"""sbgpu_bam_decode_device at its tile, staging and capacity edges (csrc/bamdecode_device.h): the streams of
tests/bam_edges_util.py -- what each is for is checked on the CPU in tests/test_bam_edges_util.py -- decoded twice on the
device, by default (bam_onepass_kernel first) and with SBGPU_BAM_TWO_PASS=1 (bam_scan_kernel + bam_fill_kernel), both held
to the oracle and to each other, every array of every record.  Which form served a default call cannot be observed from
outside: a stream whose blocks exceed 2 n + 1 024 (capacity_edges B and C) is served by the two kernels either way, and
slow_head may be, if its look-back runs out of polls; only the result is asserted."""
import ctypes as C

import numpy as np
import pytest

import bam_edges_util as E
from test_bamdecode import check_library_against_oracle

pytestmark = pytest.mark.gpu

ARRAYS = ("status", "record", "read_id", "ref", "left", "right", "partner_pos", "flags", "nh", "nm", "read_len", "sam_flag",
          "block_off", "block_left", "block_right")


@pytest.fixture(scope="module")
def ctx():
    from strawberry_amd import em
    return em.default_context(0)


def same_arrays(x, y):
    for k in ARRAYS:
        np.testing.assert_array_equal(getattr(x, k), getattr(y, k), err_msg=k)
    assert x.by_status == y.by_status and x.any_paired == y.any_paired
    assert (x.n_records, x.n_reads, x.n_blocks) == (y.n_records, y.n_reads, y.n_blocks) and x.block_off[-1] == y.block_off[-1] == x.n_blocks


def both_forms(ctx, monkeypatch, raw, off, o, **kw):
    """default and forced two-pass decodes of one stream, each against the oracle's answer `o`, and against each other"""
    from strawberry_amd import bam
    one = bam.decode(raw, off, bam.BamOptions(n_ref=E.N_REF, **kw), device=ctx)
    monkeypatch.setenv("SBGPU_BAM_TWO_PASS", "1")
    two = bam.decode(raw, off, bam.BamOptions(n_ref=E.N_REF, **kw), device=ctx)
    monkeypatch.delenv("SBGPU_BAM_TWO_PASS")
    assert one.on_device and two.on_device
    check_library_against_oracle(one, o)
    check_library_against_oracle(two, o)
    same_arrays(one, two)
    one.close(), two.close()


@pytest.mark.parametrize("kw", [dict(), dict(unique_only=False, library=1)], ids=["default", "multi_fr"])
def test_staging_limits_at_every_alignment(ctx, oracle, monkeypatch, kw):
    s = E.staging_sweep()
    both_forms(ctx, monkeypatch, s.raw, s.off, E.oracle_of(oracle, s, **kw), **kw)


def test_stream_that_starts_off_the_allocators_alignment(ctx, oracle, monkeypatch):
    """sbgpu_bam_decode_device itself, on a stream that begins 0, 1, 8 and 15 bytes into its allocation (offsets on the
    device): every range's `address & 15` moves with it, the result does not; at 0 it is bam.decode's, bit for bit."""
    import torch
    from strawberry_amd import _lib, bam
    s = E.staging_sweep()
    o = E.oracle_of(oracle, s)
    L = _lib.load()
    dev = torch.device("cuda", ctx.device)
    d_off = torch.from_numpy(s.off).to(dev)
    h_raw = torch.from_numpy(s.raw.copy())
    opts = bam.BamOptions(n_ref=E.N_REF).c()
    via_decode = bam.decode(s.raw, s.off, bam.BamOptions(n_ref=E.N_REF), device=ctx)
    for two_pass in (False, True):
        if two_pass:
            monkeypatch.setenv("SBGPU_BAM_TWO_PASS", "1")
        for lead in (0, 1, 8, 15):
            buf = torch.zeros(s.raw.size + 32, dtype=torch.uint8, device=dev)
            assert buf.data_ptr() % 16 == 0
            buf[lead:lead + s.raw.size] = h_raw.to(dev)
            torch.cuda.synchronize(dev)
            h = C.c_void_p()
            _lib.check(L.sbgpu_bam_decode_device(ctx.h, buf.data_ptr() + lead, s.raw.size, d_off.data_ptr(), s.n, C.byref(opts), None, C.byref(h)),
                       "sbgpu_bam_decode_device")
            d = bam.DecodedReads(h, keep=(buf, d_off))
            check_library_against_oracle(d, o)
            same_arrays(d, via_decode)
            d.close()
        if two_pass:
            monkeypatch.delenv("SBGPU_BAM_TWO_PASS")
    via_decode.close()


@pytest.mark.parametrize("n", E.COUNTS)
def test_record_counts_at_pass_wave_and_tile_edges(ctx, oracle, monkeypatch, n):
    s = E.count_edges()
    both_forms(ctx, monkeypatch, s.raw[:s.off[n]], s.off[:n + 1], E.oracle_prefix(E.oracle_of(oracle, s), n))


@pytest.mark.parametrize("k", range(7), ids=E.SPARSE_NAMES)
def test_tiles_without_an_accepted_record(ctx, oracle, monkeypatch, k):
    s = E.sparse_tiles()[k]
    assert s.name == E.SPARSE_NAMES[k]
    both_forms(ctx, monkeypatch, s.raw, s.off, E.oracle_of(oracle, s))
    if s.name == "none":
        from strawberry_amd import bam
        d = bam.decode(s.raw, s.off, bam.BamOptions(n_ref=E.N_REF), device=ctx)
        assert d.n_reads == 0 and d.n_blocks == 0 and d.block_off.tolist() == [0]
        d.close()


def test_first_tile_slow_and_three_look_back_windows(ctx, oracle, monkeypatch):
    s = E.slow_head()
    both_forms(ctx, monkeypatch, s.raw, s.off, E.oracle_of(oracle, s))


@pytest.mark.parametrize("k", range(4), ids=E.CAPACITY_NAMES)
def test_blocks_at_the_one_pass_capacity(ctx, oracle, monkeypatch, k):
    s = E.capacity_edges()[k]
    assert s.name == E.CAPACITY_NAMES[k]
    both_forms(ctx, monkeypatch, s.raw, s.off, E.oracle_of(oracle, s))


def test_every_way_a_record_writes_its_blocks(ctx, oracle, monkeypatch):
    s = E.block_counts()
    both_forms(ctx, monkeypatch, s.raw, s.off, E.oracle_of(oracle, s))
