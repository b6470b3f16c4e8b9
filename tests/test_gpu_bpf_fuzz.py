"""The BPF filter on the device (bpf_filter_device, pv_host.cpp: pv_bpf_keep's machine, the scans,
pv_bpf_gather, pv_bpf_secs / pv_bpf_secs_compact and the pv_index_info the host rebuilds), seen
through pv_bpf_filter_device, which runs it exactly as pv_process_device does and copies back what
it kept. The programs, their seed and the corpus are those of tests/test_bpf_fuzz.py; every program
set on a context has passed valid() and pv_bpf_validate and has run on the CPU restatement first."""
import os
import random
import struct

import numpy as np
import pytest

import pktvisor_amd as pa
from pktvisor_amd import synth
from tests import bpf_fuzz as bf
from tests import bpf_progs
from tests import parse_corpus as pc
from tests.test_bpf_fuzz import SEED
from tests.test_gpu_parity import GOLD, diff

pytestmark = pytest.mark.gpu

N_DEVICE_PROGRAMS = 96
INFO_FIELDS = ("n_records", "bytes_used", "first_sec", "first_nsec", "last_sec", "last_nsec", "monotone", "n_sec_changes")


def checked(prog):
    """only a program both checkers accept goes to a context"""
    assert bf.valid(prog) and pa.load_library().pv_bpf_validate(pa.bpf_program(prog), len(prog)) == 0, prog
    return prog


class Batch:
    """records in HBM with their index, as pv_process_device takes them"""

    def __init__(self, recs, ts_nano=0):
        import torch
        self.recs = recs
        self.index = pa.RecordIndex(recs, ts_nano)
        self.d_recs = torch.from_numpy(np.frombuffer(recs + bytes(pa.PV_RECS_PAD), dtype=np.uint8).copy()).cuda()
        self.d_offs = torch.from_numpy(np.ascontiguousarray(self.index.offsets[: max(1, self.index.n)])).cuda()

    def process(self, h):
        h.process_device(self.d_recs.data_ptr(), self.d_offs.data_ptr(), self.index)
        h.synchronize()

    def filter(self, h, **kw):
        return h.bpf_filter_device(self.d_recs.data_ptr(), self.d_offs.data_ptr(), self.index, **kw)


def assert_kept(got, want, ts_nano, what):
    """the kept blob byte for byte; offsets, the eight pv_index_info fields and the change points
    as pv_index_records gives them for the kept records"""
    kept, offs, info, sci, scs = got[:5]
    assert kept == want, (what, len(kept), len(want))
    if not want:
        assert info.n_records == 0 and len(offs) == 0 and len(sci) == 0, what
        return
    ref = pa.RecordIndex(want, ts_nano)
    assert np.array_equal(offs, ref.offsets), what
    a, b = {f: getattr(info, f) for f in INFO_FIELDS}, {f: getattr(ref.info, f) for f in INFO_FIELDS}
    assert a == b, (what, a, b)
    assert np.array_equal(sci, ref.sc_idx[: ref.info.n_sec_changes]) and np.array_equal(scs, ref.sc_sec[: ref.info.n_sec_changes]), what


# ---------------------------------------------------------------- the machine
@pytest.fixture(scope="module")
def fuzz_cases():
    """(name, program, the records the restatement keeps) of 96 random programs and the long ones"""
    recs, index = bf.corpus()
    frames = [(recs[o + 16:o + 16 + c], w) for o, c, w in index]
    longs = bf.long_programs()
    too_long = longs.pop("n4097")
    assert not bf.valid(too_long) and pa.load_library().pv_bpf_validate(pa.bpf_program(too_long), len(too_long)) != 0
    progs = [(f"random {i}", p) for i, p in enumerate(bf.random_programs(SEED, N_DEVICE_PROGRAMS))] + list(longs.items())
    cases = []
    for name, p in progs:
        keep = [bpf_progs.run(p, f, w) != 0 for f, w in frames]
        cases.append((name, checked(p), b"".join(recs[o:o + 16 + c] for (o, c, w), k in zip(index, keep) if k)))
    return recs, cases


@pytest.mark.parametrize("ts_nano", [0, 1])
def test_device_machine_fuzz(fuzz_cases, ts_nano):
    """pv_set_bpf, then the filter, per program on one context (the program buffer grows and
    shrinks between them) over the corpus as one device-resident batch"""
    recs, cases = fuzz_cases
    batch = Batch(recs, ts_nano)
    h = pa.PvHandlers(num_periods=1, max_records=batch.index.n, ts_nano=ts_nano)
    try:
        with pytest.raises(pa.PvError):  # no program set
            batch.filter(h)
        n_all = n_none = n_mixed = 0
        for name, prog, want in cases:
            h.set_bpf(prog)
            assert_kept(batch.filter(h), want, ts_nano, (name, prog if len(prog) < 300 else len(prog)))
            n_none += not want
            n_all += want == recs
            n_mixed += 0 < len(want) < len(recs)
        print(f"{len(cases)} programs: {n_all} keep all, {n_none} drop all, {n_mixed} keep and drop")
        assert n_none and n_all and n_mixed >= 0.2 * N_DEVICE_PROGRAMS
        h.set_bpf([])
        with pytest.raises(pa.PvError):
            batch.filter(h)
    finally:
        h.close()


# ---------------------------------------------------------------- the compaction
BYTE0 = [(0x30, 0, 0, 0), (0x16, 0, 0, 0)]                  # ldb [0]; ret a
LEN_BIT = [(0x80, 0, 0, 0), (0x54, 0, 0, 1), (0x16, 0, 0, 0)]  # ld len; and #1; ret a
PATTERNS = {
    "all": lambda i, n: True,
    "none": lambda i, n: False,
    "first": lambda i, n: i == 0,
    "last": lambda i, n: i == n - 1,
    "alternating": lambda i, n: i % 2 == 1,
    "all_but_one_tile": lambda i, n: i // 64 != (1 if n > 128 else 0),
    "only_63_64": lambda i, n: i in (63, 64),
}


def shaped_batch(kind, n, pattern, secs=None):
    """n records whose sizes walk the caplen list (from a start that depends on n), kept by BYTE0
    (kind "byte": the frame's first byte; no empty capture) or LEN_BIT ("len": the low bit of the
    wire length, so a record without a single captured byte can be kept too)"""
    caps = [c for c in bf.CAPLENS if c or kind == "len"]
    rng = random.Random(n)
    out = bytearray()
    for i in range(n):
        cap = caps[(i + n) % len(caps)]
        keep = PATTERNS[pattern](i, n)
        f = bytearray(rng.randbytes(cap))
        if kind == "byte":
            f[0] = rng.randrange(1, 256) if keep else 0
        wirelen = (cap + 2 * rng.randrange(0, 3)) | 1 if keep else (cap + 1) & ~1
        sec = bf.BASE_SEC + i // 5 if secs is None else secs[i]
        out += struct.pack("<IIII", sec, (i * 3571) % 1_000_000, cap, wirelen if kind == "len" else max(cap, wirelen)) + f
    return bytes(out)


@pytest.mark.parametrize("kind", ["byte", "len"])
def test_compaction_shapes(kind):
    """record counts around the wave and the workgroup, keep patterns at their edges, record sizes
    on both sides of the gather's 64-byte step, and timestamps that go back"""
    prog = checked(BYTE0 if kind == "byte" else LEN_BIT)
    h = pa.PvHandlers(num_periods=1, max_records=257, bpf=prog)
    try:
        for n in (1, 63, 64, 65, 256, 257):
            for pattern in PATTERNS:
                recs = shaped_batch(kind, n, pattern)
                want = bpf_progs.filter_records(recs, prog)
                n_want = sum(1 for i in range(n) if PATTERNS[pattern](i, n))
                assert pa.RecordIndex(want).n == n_want if want else n_want == 0
                assert_kept(Batch(recs).filter(h), want, 0, (kind, n, pattern))
        # a kept run that goes back in time; then one whose only steps back lie in dropped records
        n = 257
        secs = [bf.BASE_SEC + i // 5 for i in range(n)]
        for i in (101, 103, 191):  # odd: kept by "alternating"
            secs[i] -= 40
        recs = shaped_batch(kind, n, "alternating", secs)
        want = bpf_progs.filter_records(recs, prog)
        got = Batch(recs).filter(h)
        assert_kept(got, want, 0, (kind, "kept run goes back"))
        assert got[2].monotone == 0
        secs = [bf.BASE_SEC + i // 5 for i in range(n)]
        for i in (100, 102, 190, 256):  # even: dropped
            secs[i] -= 40
        recs = shaped_batch(kind, n, "alternating", secs)
        batch = Batch(recs)
        assert batch.index.info.monotone == 0
        got = batch.filter(h)
        assert_kept(got, bpf_progs.filter_records(recs, prog), 0, (kind, "only dropped records go back"))
        assert got[2].monotone == 1
    finally:
        h.close()


# ---------------------------------------------------------------- what lies behind the kept records
def restamp(recs, sec, usec=0, step_us=1000):
    """the records with rising stamps from (sec, usec) on; returns (records, the last stamp)"""
    out = bytearray(recs)
    pos = 0
    last = (sec, usec)
    while pos + 16 <= len(out):
        last = (sec + usec // 1_000_000, usec % 1_000_000)
        struct.pack_into("<II", out, pos, *last)
        usec += step_us
        pos += 16 + struct.unpack_from("<I", out, pos + 8)[0]
    return bytes(out), last


def cut_query_batch(sec):
    """a few whole UDP/53 queries, then one cut by its caplen inside the question name"""
    rng = random.Random(7)
    frames = [pc.eth(rng, pc.v4hdr(rng, pc.dns_l4(rng, 17, "stale"), 17, src="10.1.2.3", dst="8.8.8.8"), 0x0800) for _ in range(5)]
    recs = [pc.record(f, sec=sec, usec=k) for k, f in enumerate(frames[:-1])]
    recs.append(pc.record(frames[-1], caplen=14 + 20 + 8 + 12 + 3, sec=sec, usec=len(frames)))
    return b"".join(recs)


def test_small_batch_after_large_window():
    """a large batch, then a small one whose last kept record is a DNS query cut inside its name, both
    through the filter: the window of a context without a program fed the host-filtered records"""
    big = synth.pcap_bytes(4, 6000)[24:]
    last = pa.last_record_ts(big, pa.RecordIndex(big))
    small = cut_query_batch(last[0] + 1)
    assert bpf_progs.filter_records(small, bpf_progs.UDP53) == small
    end = pa.last_record_ts(small, pa.RecordIndex(small))
    wins = []
    for bpf in (checked(bpf_progs.UDP53), None):
        h = pa.PvHandlers(host_spec=synth.HOST_SPEC, num_periods=1, max_records=1 << 14, bpf=bpf)
        try:
            for recs in (big, small):
                Batch(recs if bpf else bpf_progs.filter_records(recs, bpf_progs.UDP53)).process(h)
            h.set_end_tstamp(*end)
            wins.append(h.window_json(0))
        finally:
            h.close()
    assert wins[1]["dns"]["wire_packets"]["total"] > 1000
    assert diff(wins[0], wins[1]) is None, diff(wins[0], wins[1])


def test_padding_behind_kept_run_is_zero():
    """the PV_RECS_PAD bytes behind the kept records, which the kernels after the filter may read,
    are zero after a larger batch has been through the same buffer, as behind every staged batch"""
    big = synth.pcap_bytes(4, 6000)[24:]
    small = cut_query_batch(bf.BASE_SEC)
    h = pa.PvHandlers(num_periods=1, max_records=1 << 14, bpf=checked(bpf_progs.UDP53))
    try:
        kept = Batch(big).filter(h, with_pad=True)
        assert len(kept[0]) > len(small) + pa.PV_RECS_PAD
        assert kept[5] == bytes(pa.PV_RECS_PAD)
        got = Batch(small).filter(h, with_pad=True)
        assert_kept(got, small, 0, "small batch")
        assert got[5] == bytes(pa.PV_RECS_PAD), got[5].hex()
        # a shorter kept run of a longer batch: the first record alone
        first = checked([(0x30, 0, 0, 0), (0x15, 0, 1, small[16]), (0x06, 0, 0, 1), (0x06, 0, 0, 0)])
        h.set_bpf(first)
        recs = small + big[: int(pa.RecordIndex(big).offsets[40])]
        want = bpf_progs.filter_records(recs, first)
        assert 0 < len(want) < len(small)
        got = Batch(recs).filter(h, with_pad=True)
        assert_kept(got, want, 0, "first record")
        assert got[5] == bytes(pa.PV_RECS_PAD), got[5].hex()
    finally:
        h.close()


# ---------------------------------------------------------------- program changes, dropped batches
def test_program_changes_and_dropped_batches():
    """program A, a longer program B (past the LDS part), none, A again on one context, a batch per
    step; then a batch A drops wholly, a period ahead, as the capture's final one: no shift, no
    event, and the end-of-capture flush all the same. Equal to a context without a program fed the
    host-filtered records of each batch in order."""
    _, _, recs = pa.read_pcap(os.path.join(GOLD, "dns_udp_tcp_random.pcap"))
    idx = pa.RecordIndex(recs)
    cuts = [0, int(idx.offsets[5000]), int(idx.offsets[10000]), len(recs)]
    parts = [recs[cuts[k]:cuts[k + 1]] for k in range(3)]
    # a connection whose response only the capture's end delivers, at the second part's last stamp
    held, _ = restamp(synth.tcp_hole18_pcap()[24:], *pa.last_record_ts(parts[1], pa.RecordIndex(parts[1]))[:1], step_us=0)
    prog_a = checked(bpf_progs.UDP53)
    prog_b = checked([(0x05, 0, 0, 1200)] + [bf.FILL] * 1200 + bpf_progs.UDP)
    last = pa.last_record_ts(recs, idx)
    tcp_only = bpf_progs.filter_records(parts[0], [(0x30, 0, 0, 23), (0x15, 0, 1, 6), (0x06, 0, 0, 1), (0x06, 0, 0, 0)])
    ahead, _ = restamp(tcp_only, last[0] + 120)
    assert len(ahead) > 1000 and bpf_progs.filter_records(ahead, prog_a) == b""
    steps = [(prog_a, parts[0]), (prog_b, parts[1]), ([], held), (prog_a, parts[2])]
    for p, r in steps[:2]:
        assert 0 < len(bpf_progs.filter_records(r, p)) < len(r)

    def window(h):
        return [h.window_json(0), h.window_json(3, merged=True), h.window_periods(pa.PART_NET), h.window_periods(pa.PART_DNS)]

    kw = dict(host_spec="192.168.0.0/24", num_periods=3, max_records=1 << 14)
    h = pa.PvHandlers(**kw)
    try:
        for p, r in steps:
            h.set_bpf(p)
            Batch(r).process(h)
        before = window(h)
        h.set_end_of_capture()
        Batch(ahead).process(h)
        after = window(h)
        assert after[2:] == before[2:]  # no period shift
        assert after[0]["packets"] == before[0]["packets"]  # no event
        h.set_end_tstamp(*last)
        got = window(h)
    finally:
        h.close()
    ref = pa.PvHandlers(**kw)
    try:
        for p, r in steps:
            Batch(bpf_progs.filter_records(r, p) if p else r).process(ref)
        open_before = window(ref)
        ref.set_end_of_capture()
        Batch(b"").process(ref)
        flushed = window(ref) != open_before
        ref.set_end_tstamp(*last)
        want = window(ref)
    finally:
        ref.close()
    assert flushed, "the capture's end closed no connection: the flush is not exercised"
    assert (after != before) == flushed
    for a, b in zip(got, want):
        assert diff(a, b) is None, diff(a, b)
