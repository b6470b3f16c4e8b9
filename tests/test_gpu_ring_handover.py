"""pv_net_combine_ring's hand-over: the combine tail starts without waiting for the Net phase's
global stores. What it needs of the Net phase comes through LDS: the `bad` word (a DNS message or a
deferred record in any range of the workgroup's group, ORed over the ranges) and the Net waves'
counters, summed there and added to the window once a workgroup; the tail's barriers are LDS-only
and the inserting waves wait for their own spill stores, which the out pass reads back.

As in test_gpu_fused_ring: every case runs its batches in three contexts (default, PV_FUSE_RING=0,
PV_FUSE_PLAIN=0) and requires equal windows after every batch, equal to the oracle's over the same
records, and the expected pv_ring_stats and pv_fuse_stats. Batches 1 and 2 are 200 records where
the case is about batch 3."""
import struct

import numpy as np
import pytest

from tests.test_gpu_fused_plain import ETH, ME, _cus, _fusable, _hdr, _plain_rows, _rec_dns, _rec_vlan, _remote, _rows, _t, _udp4, _with
from tests.test_gpu_fused_ring import SMALL, THIRD, _check, _rec_tcp

pytestmark = pytest.mark.gpu

WT = 4  # tiles a range in the `bad` cases: tile t of a range is Net wave t's


@pytest.mark.parametrize("wave", [0, 3])
@pytest.mark.parametrize("what", ["dns", "vlan"])
@pytest.mark.parametrize("where", ["first_range", "middle_range", "last_range", "single_range_group"])
def test_bad_word_accumulates_over_the_ranges(oracle, where, what, wave):
    """batch 3, launched without the log, holds one UDP/53 record or one VLAN (deferred) record in
    one range of one group, on a tile of Net wave 0 or 3: the first, middle or last range of a
    middle group of a 3 C range batch, or the single range of the last group of a 3 C - 2 range
    batch. Its workgroup must leave its lists alone whichever range set the word, pv_net_iplog
    writes the log and the regular chain combines the batch. Batches 4 to 6 (3 C tiles, plain) run
    the regular chain, the logged fused launch and the ring again."""
    c = _cus()
    ranges = 3 * c - 2 if where == "single_range_group" else 3 * c
    n = 64 * WT * ranges - 37
    assert _fusable(n, c) and _fusable(3 * c * 64, c)
    r = {"first_range": 3 * (c // 2), "middle_range": 3 * (c // 2) + 1, "last_range": 3 * (c // 2) + 2,
         "single_range_group": ranges - 1}[where]
    k = (r * WT + wave) * 64 + 5
    assert k < n
    sub = {"dns": _rec_dns(int(_remote(7002)), ME, _t(2, k), 77), "vlan": _rec_vlan(int(_remote(7001)), ME, _t(2, k))}[what]
    batches = SMALL + [_with(_plain_rows(2, n), {k: sub})] + [_plain_rows(b, 3 * c * 64).tobytes() for b in range(3, 6)]
    wins = _check(oracle, batches, [(0, 0), (0, 0), (1, 1), (1, 1), (2, 1), (3, 1)], [(0, 0), (0, 0), (1, 1), (1, 1), (1, 1), (2, 1)])
    assert wins[5]["packets"]["events"] == 400 + n + 3 * 3 * c * 64


def _rec_icmp(src, dst, ts_us):
    """Ethernet + IPv4 + ICMP echo: another L4 on the lean pass's fast path"""
    icmp = struct.pack(">BBHHH", 8, 0, 0, 1, 1) + bytes(22)
    return _hdr(ts_us, ETH + b"\x08\x00" + struct.pack(">BBHHHBBHII", 0x45, 0, 20 + len(icmp), 0, 0, 64, 1, 0, src, dst) + icmp)


def _mixed(b, n):
    """batch b's plain rows with every fifth record replaced: TCP with and without SYN, ICMP, UDP of
    other sizes (payload bins 164, 664, 1464 and, past the LDS histogram, 2100), directions in, out
    and unknown"""
    rows, subs = _plain_rows(b, n), {}
    for j, k in enumerate(range(3, n, 5)):
        a, o, t = int(_remote(k % 4000)), int(_remote(9000 + k % 4000)), _t(b, k)
        subs[k] = (lambda: _rec_tcp(a, ME, t, 0x02), lambda: _rec_tcp(ME, a, t, 0x18, payload=bytes(300)), lambda: _rec_icmp(a, ME, t),
                   lambda: _hdr(t, ETH + b"\x08\x00" + _udp4(a, o, payload=bytes(122))), lambda: _hdr(t, ETH + b"\x08\x00" + _udp4(ME, a, payload=bytes(1422))),
                   lambda: _rec_tcp(a, o, t, 0x10), lambda: _hdr(t, ETH + b"\x08\x00" + _udp4(a, ME, payload=bytes(622))),
                   lambda: _rec_icmp(o, a, t), lambda: _rec_tcp(ME, a, t, 0x12),
                   lambda: _hdr(t, ETH + b"\x08\x00" + _udp4(a, ME, payload=bytes(2058 if j % 90 == 9 else 22))))[j % 10]()
    return _with(rows, subs)


@pytest.mark.parametrize("shape", ["one_tile", "ragged"])
def test_workgroup_counter_flush(oracle, shape):
    """a no-log batch that mixes UDP, TCP with and without SYN and ICMP, inbound, outbound and of
    unknown direction, in several payload bins: 3 C ranges of one tile (three Net waves of every
    workgroup have no tile) and of two tiles with a ragged last one. Every `packets` counter and the
    payload quantiles equal the oracle's (the whole window does), and no counter of the mix is zero."""
    c = _cus()
    n = 3 * c * 64 if shape == "one_tile" else 3 * c * 64 * 2 - 37
    assert _fusable(n, c)
    wins = _check(oracle, SMALL + [_mixed(2, n)], *THIRD)
    p = wins[2]["packets"]
    assert p["events"] == p["total"] == p["ipv4"] == n + 400 and p["in"] + p["out"] + p["unknown_dir"] == n + 400
    assert p["udp"] + p["tcp"] + p["other_l4"] == n + 400
    assert min(p["udp"], p["tcp"], p["other_l4"], p["protocol"]["tcp"]["syn"], p["in"], p["out"], p["unknown_dir"]) > 0
    assert p["protocol"]["tcp"]["syn"] < p["tcp"] and p["payload_size"]["p50"] < p["payload_size"]["p99"]


def test_first_probe_and_bucket_slots_both_directions(oracle):
    """one group of 3 x 32 tiles holds 3,000 addresses in both directions (6,000 of its table's
    16,384 slots: claims at the first probe and in the buckets after it), every address first seen
    inbound and outbound at known records; the other groups draw from a small pool"""
    c = _cus()
    wt = 32
    n = 3 * c * 64 * wt
    assert _fusable(n, c)
    g0, gn = (c // 2) * 192 * wt, 192 * wt
    rng = np.random.default_rng(12)
    addr, out = _remote(rng.integers(0, 3000, n)), np.arange(n) % 3 == 0
    j = np.arange(gn)
    addr[g0:g0 + gn] = _remote(20000 + j % 3000)
    out[g0:g0 + gn] = (j // 3000) % 2 == 1
    _check(oracle, SMALL + [_rows(addr, out, _t(2), step_us=1).tobytes()], *THIRD)


def test_spill_read_back_behind_the_moved_wait(oracle):
    """one group with 17,088 distinct (address, direction) pairs in its 17,088 records, past the
    compact table's 16,384 slots, so the inserting waves spill and the out pass reads the spill list
    back; every other group draws from a pool of 5,000 addresses (the oracle's cost is the distinct
    addresses: 1.7 s for the 4.4M records, where test_gpu_fused_ring's spill case, every group past
    the table, takes 8.5 s)."""
    c = _cus()
    k = -(-17000 // 192)
    n, gn = 3 * c * 64 * k, 192 * k
    assert _fusable(n, c) and 16384 < gn < 65536
    g0 = (c // 2) * gn
    rng = np.random.default_rng(13)
    addr, out = _remote(rng.integers(0, 5000, n)), np.arange(n) % 3 == 0
    addr[g0:g0 + gn] = (20 << 24) + (1 << 20) + np.arange(gn)
    wins = _check(oracle, SMALL + [_rows(addr, out, _t(2), step_us=1).tobytes()], *THIRD)
    assert wins[2]["packets"]["events"] == n + 400
