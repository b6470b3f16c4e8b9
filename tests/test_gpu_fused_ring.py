"""pv_net_combine_ring: the fused launch of a plain short-chain batch without the compact IP log.
The Net waves hand each tile's IPv4 words and direction mask to the inserting waves through a ring
in LDS: two sections of K = 3 tiles of each of the four Net waves, 12 tiles or 768 records a
section, one barrier a section. The host takes it only after two plain batches in a row, so batches
1 to 3 of a context run unfused, fused with the log, and without it; a batch that is not plain
after all has pv_net_iplog write the log before the regular chain runs.

A choice of speed only. Every case runs its batches in three contexts (default; PV_FUSE_RING=0: the
logged fused launch; PV_FUSE_PLAIN=0: the two launches) and requires equal windows after every batch,
equal to the oracle's over the same records (the cardinalities replay first occurrences, so a wrong
record index shows), and the expected pv_ring_stats and pv_fuse_stats. Where the case is about
batch 3 alone, batches 1 and 2 are 200 records: plain, too small to fuse."""
import struct

import numpy as np
import pytest

import pktvisor_amd as pa
from tests.test_gpu_fused_plain import (ETH, GROUPS, HOST, ME, _cus, _fusable, _hdr, _plain_rows, _rec_dns, _rec_v6, _rec_vlan, _ref,
                                        _remote, _rows, _t, _with)
from tests.test_gpu_parity import diff

pytestmark = pytest.mark.gpu

K = 3            # tiles of each Net wave a section (PV_RING_K)
SEC = 4 * K * 64  # records a section


def _run(batches, env=(), timing=0, **kw):
    """one context over the batches (no reset in between): the window, pv_fuse_stats and
    pv_ring_stats after each batch"""
    mp = pytest.MonkeyPatch()
    try:
        for k in ("PV_CB_FAN", "PV_CB_COMPACT", "PV_NET_WGCU", "PV_PLAIN_CHAIN", "PV_FUSE_PLAIN", "PV_FUSE_RING"):
            mp.delenv(k, raising=False)
        for k, v in dict(env).items():
            mp.setenv(k, v)
        h = pa.PvHandlers(host_spec=HOST, num_periods=1, max_records=max(len(b) for b in batches) // 80 + 64, **kw)
        wins, fstats, rstats = [], [], []
        try:
            if timing:
                h.set_kernel_timing(timing)
            for b in batches:
                h.process_host(b)
                h.set_end_tstamp(*pa.last_record_ts(b, pa.RecordIndex(b, max_records=len(b) // 80 + 64)))
                wins.append(h.window_json(0))
                fstats.append(h.fuse_stats())
                rstats.append(h.ring_stats())
        finally:
            h.close()
        return wins, fstats, rstats
    finally:
        mp.undo()


def _check(oracle, batches, want_fuse, want_ring, okw=None, **kw):
    wins, fs, rs = _run(batches, **kw)
    winsl, fsl, rsl = _run(batches, env={"PV_FUSE_RING": "0"}, **kw)
    wins0, fs0, rs0 = _run(batches, env={"PV_FUSE_PLAIN": "0"}, **kw)
    for k in range(len(batches)):
        ref = _ref(oracle, batches, k + 1, **(okw or {}))
        assert diff(wins0[k], ref) is None, (k, "PV_FUSE_PLAIN=0", diff(wins0[k], ref))
        assert diff(winsl[k], ref) is None, (k, "PV_FUSE_RING=0", diff(winsl[k], ref))
        assert diff(wins[k], ref) is None, (k, diff(wins[k], ref))
        assert wins[k] == winsl[k] == wins0[k], (k, diff(wins[k], winsl[k]), diff(wins[k], wins0[k]))
    zero = [(0, 0)] * len(batches)
    assert (fs, rs) == (want_fuse, want_ring), (fs, rs)
    assert (fsl, rsl) == (want_fuse, zero), (fsl, rsl)
    assert (fs0, rs0) == (zero, zero), (fs0, rs0)
    return wins


SMALL = [_plain_rows(b, 200).tobytes() for b in range(2)]  # batches 1 and 2 of a case about batch 3
THIRD = ([(0, 0), (0, 0), (1, 0)], [(0, 0), (0, 0), (1, 0)])


def _n(wt, ragged=True):
    n = 3 * _cus() * 64 * wt - (37 if ragged else 0)
    assert _fusable(n, _cus())
    return n


@pytest.mark.parametrize("groups", list(GROUPS), ids=list(GROUPS))
@pytest.mark.parametrize("shape", ["one_tile", "ragged", "short_last_group"])
def test_smallest_shapes(oracle, groups, shape):
    """3 C ranges of one tile (three Net waves of every workgroup have no tile); of two tiles with a
    ragged last tile; 3 C - 2 ranges of two tiles with a ragged last tile, so that the last group is
    a single range (as C2's 766 ranges leave one; without the ring it takes the generic table).
    Three batches of that size: unfused, logged, no-log."""
    n = {"one_tile": _n(1, False), "ragged": _n(2), "short_last_group": 64 * 2 * (3 * _cus() - 2) - 37}[shape]
    assert _fusable(n, _cus())
    batches = [_plain_rows(b, n).tobytes() for b in range(3)]
    kw = GROUPS[groups]
    _check(oracle, batches, [(0, 0), (1, 0), (2, 0)], [(0, 0), (0, 0), (1, 0)], okw=kw, **kw)


@pytest.mark.parametrize("wt", [4 * K, 4 * K + 1, 8 * K - 1])
def test_section_edges(oracle, wt):
    """a range of exactly one full section; of a section of one tile behind it; of a last section
    one tile short; the batch's last tile ragged"""
    batches = SMALL + [_plain_rows(2, _n(wt)).tobytes()]
    _check(oracle, batches, *THIRD)


def test_first_occurrence_across_section_range_and_group_edges(oracle):
    """ranges of 2 K 4 + 1 tiles (two sections and one tile), groups of three. p: first seen at the
    last record of a range's first section and again at the first of its second; x: both directions
    inside one tile; q: a group's last record and the next group's first; r: a range's last record
    and the next range's first, inside a group; all of them again in other groups. The rest from
    a pool of 20,000 other addresses (a batch of distinct ones costs the oracle seconds), every
    third outbound."""
    wt = 2 * K * 4 + 1
    n, rr = _n(wt, False), 64 * wt
    p, x, q, r = (int(v) for v in _remote(np.arange(30001, 30005)))
    addr, out = _remote(np.random.default_rng(5).integers(0, 20000, n)), np.arange(n) % 3 == 0
    g = 5 * 3 * rr  # group 5's first record
    for k, v, o in ((g + rr + SEC - 1, p, 0), (g + rr + SEC, p, 0), (g + 70, x, 0), (g + 100, x, 1), (g + 3 * rr - 1, q, 0),
                    (g + 3 * rr, q, 0), (g + 2 * rr - 1, r, 1), (g + 2 * rr, r, 1), (7, p, 1), (n - 1, q, 1), (n - 2, x, 0),
                    (20 * rr + 5, r, 0), (20 * rr + SEC + 5, p, 0)):
        addr[k], out[k] = v, bool(o)
    batches = SMALL + [_rows(addr, out, _t(2), step_us=1).tobytes()]
    _check(oracle, batches, *THIRD)


def test_one_hot_key(oracle):
    """every record of the batch the same address, inbound: every lane of every inserting wave hits
    one slot of its group's table"""
    n = _n(8, False)
    batches = SMALL + [_rows(np.full(n, int(_remote(4242))), np.zeros(n, bool), _t(2), step_us=1).tobytes()]
    wins = _check(oracle, batches, *THIRD)
    v = int(_remote(4242))
    assert {"name": "20.%d.%d.%d" % (v >> 16 & 255, v >> 8 & 255, v & 255), "estimate": n} in wins[2]["packets"]["top_ipv4"]


def test_entries_that_must_not_be_inserted(oracle):
    """records with neither address in the host subnets (direction unknown) and records from
    0.0.0.0, mixed into a plain batch: they log a zero word, which no one inserts"""
    n = _n(5)
    rows = _plain_rows(2, n)
    k = np.arange(n)
    other = np.asarray(_remote(k + 9000), dtype=np.int64).astype(">u4").view(np.uint8).reshape(n, 4)
    unk, zero = k % 5 == 1, k % 7 == 3
    rows[unk, 16 + 26:16 + 30] = other[unk]            # source and destination both remote
    rows[unk, 16 + 30:16 + 34] = other[::-1][unk]
    rows[zero, 16 + 26:16 + 30] = 0                    # 0.0.0.0 -> ME
    rows[zero, 16 + 30:16 + 34] = np.frombuffer(struct.pack(">I", ME), dtype=np.uint8)
    _check(oracle, SMALL + [rows.tobytes()], *THIRD)


def test_spill_in_the_no_log_batch(oracle):
    """test_gpu_fused_plain's k = 89 construction (17,088 keys a group, past the compact table's
    16,384 slots) as the no-log batch"""
    c = _cus()
    k = -(-17000 // 192)
    n = 3 * c * 64 * k
    i = np.arange(n, dtype=np.int64)
    big = _rows((20 << 24) + 1 + i % (n // 3), i % 3 == 0, _t(2), step_us=1).tobytes()
    assert 192 * k >= 17000 and 192 * k < 65536 and n // 3 > 192 * k
    _check(oracle, SMALL + [big], *THIRD)


@pytest.mark.parametrize("where", ["first_group", "last_group", "middle_group"])
@pytest.mark.parametrize("what", ["dns", "vlan", "ipv6"])
def test_wrong_guess_in_a_no_log_batch(oracle, what, where):
    """seven batches of 3 C tiles in one window; batch 4, launched without the log, holds one
    record the short chain cannot take: pv_net_iplog writes the log and the regular chain combines
    the batch. Batch 5 runs the regular chain, batch 6 fused with the log, batch 7 without it. No
    top_ipv4 estimate may count twice."""
    c = _cus()
    n = 3 * c * 64
    k = {"first_group": 5, "last_group": n - 3, "middle_group": 192 * (c // 2) + 100}[where]
    x = int(_remote(7001))
    sub = {"dns": _rec_dns(int(_remote(7002)), ME, _t(3, k), 77), "vlan": _rec_vlan(x, ME, _t(3, k)), "ipv6": _rec_v6(9, _t(3, k))}[what]
    rows = [_plain_rows(b, n) for b in range(7)]
    batches = [r.tobytes() for r in rows]
    batches[3] = _with(rows[3], {k: sub})
    wins = _check(oracle, batches, [(0, 0), (1, 0), (2, 0), (3, 1), (3, 1), (4, 1), (5, 1)],
                  [(0, 0), (0, 0), (1, 0), (2, 1), (2, 1), (2, 1), (3, 1)])
    assert wins[6]["packets"]["events"] == 7 * n
    if what == "ipv6":
        assert wins[6]["packets"]["top_ipv6"] == [{"name": "2001:db8::9", "estimate": 1}]


def _rec_tcp(src, dst, ts_us, flags, sport=40000, dport=8443, payload=b"0123456789"):
    """Ethernet + IPv4 + TCP, 64 bytes as the UDP rows"""
    tcp = struct.pack(">HHIIBBHHH", sport, dport, 1000, 0, 5 << 4, flags, 1024, 0, 0) + payload
    return _hdr(ts_us, ETH + b"\x08\x00" + struct.pack(">BBHHHBBHII", 0x45, 0, 20 + len(tcp), 0, 0, 64, 6, 0, src, dst) + tcp)


def test_tcp_segments_in_a_no_log_batch(oracle):
    """TCP records on a non-DNS port (SYNs and data, both directions) in a plain batch: a one-span
    batch's Net pass emits their tile masks and segments (tcp_emit), which stay global stores"""
    n = _n(2)
    rows = _plain_rows(2, n)
    subs = {}
    for j, k in enumerate(range(11, n, 97)):
        a = int(_remote(k))
        s, d = (ME, a) if j % 2 else (a, ME)
        subs[k] = _rec_tcp(s, d, _t(2, k), 0x02 if j % 3 == 0 else 0x18, sport=40000 + j % 1000)
    assert all(len(v) == 80 for v in subs.values())
    _check(oracle, SMALL + [_with(rows, subs)], *THIRD)


def test_stamped_batches_stay_unfused(oracle):
    """pv_set_kernel_timing(2) over eight batches: batches 1, 3, 5 and 7 are dispatch-stamped and
    keep the two launches (they count as plain batches); batch 2 follows one plain batch and is
    fused with the log, batches 4, 6 and 8 run without it"""
    n = _n(2)
    batches = [_plain_rows(b, n).tobytes() for b in range(8)]
    wins, fs, rs = _run(batches, timing=2)
    wins0, fs0, rs0 = _run(batches, env={"PV_FUSE_PLAIN": "0"}, timing=2)
    assert fs == [(0, 0), (1, 0), (1, 0), (2, 0), (2, 0), (3, 0), (3, 0), (4, 0)], fs
    assert rs == [(0, 0), (0, 0), (0, 0), (1, 0), (1, 0), (2, 0), (2, 0), (3, 0)], rs
    assert fs0 == rs0 == [(0, 0)] * 8
    assert wins == wins0
    assert diff(wins[7], _ref(oracle, batches, 8)) is None
