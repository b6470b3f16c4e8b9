"""BGP handler on the CPU: the product's segment extraction (pv_bgp.h) and host manager
(pv_bgp.cpp), compiled for the host by tests/native_bgp, against the reference's known answers
(tests/golden/kat_bgp.json) and the Python model (tests/bgp_ref.py). No GPU."""
import ctypes
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import pktvisor_amd as pa
from pktvisor_amd import config as pvcfg
from tests import bgp_cases as bc
from tests import bgp_ref, schema_check

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE_DIR = os.path.join(ROOT, "tests", "native_bgp")
NATIVE = os.path.join(NATIVE_DIR, "libpvbgp_host.so")
GOLDEN = os.path.join(ROOT, "tests", "golden")
KAT = json.load(open(os.path.join(GOLDEN, "kat_bgp.json")))
T0 = bc.T0
STREAMS = 2000  # random streams per seed


class Seg(ctypes.Structure):
    _fields_ = [("rec", ctypes.c_uint32), ("sec", ctypes.c_uint32), ("nsec", ctypes.c_uint32), ("tcp_sec_before", ctypes.c_uint32),
                ("fkey", ctypes.c_uint32), ("seq", ctypes.c_uint32), ("plen", ctypes.c_uint32), ("caplen", ctypes.c_uint32),
                ("off", ctypes.c_uint32), ("sport", ctypes.c_uint16), ("dport", ctypes.c_uint16), ("flags", ctypes.c_uint8),
                ("pad", ctypes.c_uint8 * 7), ("src", ctypes.c_uint8 * 16)]


class Ev(ctypes.Structure):
    _fields_ = [("sec", ctypes.c_int64), ("nsec", ctypes.c_int64), ("type", ctypes.c_uint32), ("len", ctypes.c_uint32)]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(NATIVE):
        subprocess.check_call(["make", "-C", NATIVE_DIR])
    h = ctypes.CDLL(NATIVE)
    P, U32, I64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int64
    assert ctypes.sizeof(Seg) == 64
    h.bg_new.argtypes = [U32] * 4
    h.bg_new.restype = P
    h.bg_free.argtypes = [P]
    h.bg_reset.argtypes = [P]
    h.bg_extract.argtypes = [P, ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(ctypes.POINTER(Seg)),
                             ctypes.POINTER(ctypes.POINTER(ctypes.c_uint8)), ctypes.POINTER(U32)]
    h.bg_extract.restype = U32
    h.bg_feed.argtypes = [P, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int]
    h.bg_set_end.argtypes = [P, I64, I64]
    h.bg_check_period_shift.argtypes = [P, I64, I64]
    for f in (h.bg_periods, h.bg_open_connections, h.bg_known_connections):
        f.argtypes = [P]
        f.restype = U32
    h.bg_events.argtypes = [P, ctypes.POINTER(ctypes.POINTER(Ev))]
    h.bg_events.restype = U32
    h.bg_json.argtypes = [P, U32, ctypes.c_int]
    h.bg_json.restype = P
    h.bg_stamps.argtypes = [P, U32, ctypes.POINTER(I64)]
    h.bg_free_str.argtypes = [P]
    return h


class Native:
    """the harness next to a bgp_ref.Manager with the same config"""

    def __init__(self, lib, linktype=1, ts_nano=0, num_periods=5, rate=100):
        self.lib, self.lt, self.ns = lib, linktype, ts_nano
        self.h = lib.bg_new(linktype, ts_nano, num_periods, rate)
        self.ref = bgp_ref.Manager(num_periods, rate)

    def feed(self, recs: bytes, eoc=False):
        self.lib.bg_feed(self.h, recs, len(recs), int(eoc))
        self.ref.feed(recs, self.lt, self.ns, eoc)

    def reset(self):
        self.lib.bg_reset(self.h)
        self.ref.reset()

    def events(self):
        p = ctypes.POINTER(Ev)()
        n = self.lib.bg_events(self.h, ctypes.byref(p))
        return [(p[i].sec, p[i].nsec, p[i].type, p[i].len) for i in range(n)]

    def json(self, period=0, merged=False):
        p = self.lib.bg_json(self.h, period, int(merged))
        txt = ctypes.string_at(p).decode()
        self.lib.bg_free_str(p)
        assert not txt.startswith("!"), txt
        return json.loads(txt)["bgp"]

    def check(self, period=0, merged=False):
        assert self.events() == self.ref.events
        assert self.lib.bg_open_connections(self.h) == self.ref.open_connections()
        assert self.lib.bg_known_connections(self.h) == self.ref.known_connections()
        got = self.json(period, merged)
        assert got == self.ref.window(period, merged)
        return got

    def close(self):
        self.lib.bg_free(self.h)


def run(lib, batches, eoc=False, **kw):
    """the batches through a fresh harness and model: (window, events)"""
    n = Native(lib, **kw)
    try:
        for i, b in enumerate(batches):
            n.feed(b, eoc and i == len(batches) - 1)
        return n.check(), n.events()
    finally:
        n.close()


# ---------------------------------------------------------------- 1. known answers
def test_fixture_known_answers(lib):
    kat = KAT["bgp.pcap"]
    lt, ns, recs = pa.read_pcap(os.path.join(GOLDEN, "bgp.pcap"))
    rs = bgp_ref.records(recs)
    assert len(rs) == 22
    n = Native(lib, lt, ns, num_periods=1)
    n.feed(recs, eoc=True)
    end = (rs[-1][1], rs[-1][2] if ns else rs[-1][2] * 1000)
    lib.bg_set_end(n.h, *end)
    n.ref.set_end(*end)
    win = n.check()
    assert win["period"] == {"start_ts": kat["start"][0], "length": kat["length"]}
    assert win["wire_packets"]["events"] == kat["events"] == win["wire_packets"]["deep_samples"]
    for k, v in kat["counters"].items():
        assert win["wire_packets"][k] == v, k
    st = (ctypes.c_int64 * 4)()
    assert lib.bg_stamps(n.h, 0, st) == 0
    assert list(st) == kat["start"] + kat["end"] and lib.bg_periods(n.h) == kat["periods"]
    schema = json.load(open(os.path.join(GOLDEN, "bgp_window-schema.json")))
    assert schema_check.errors(schema, {"bgp": win}) == []
    # each of the nine payloads is one message, and an event's stamp is the connection's endTime
    assert sorted(e[2] for e in n.events()) == [1, 1, 2, 2, 2, 2, 4, 4, 4]
    assert all(e[1] % 1000 == 0 for e in n.events())
    n.close()


# ---------------------------------------------------------------- extraction
def segs_equal(g: Seg, arena: bytes, m: dict):
    assert (g.rec, g.sec, g.nsec, g.tcp_sec_before, g.fkey, g.seq) == (m["rec"], m["sec"], m["nsec"], m["tcp_sec_before"], m["fkey"],
                                                                      m["seq"])
    assert (g.sport, g.dport) == (m["sport"], m["dport"])
    assert (bool(g.flags & 1), bool(g.flags & 2), bool(g.flags & 4), bool(g.flags & 8)) == (m["fin"], m["syn"], m["rst"], m["side"][0])
    assert bytes(g.src) == m["side"][1].ljust(16, b"\0")
    assert g.plen == g.caplen == len(m["data"]) and arena[g.off:g.off + g.caplen] == m["data"]
    assert bytes(g.pad) == bytes(7)


def extract_both(lib, recs, linktype=1):
    h = lib.bg_new(linktype, 0, 1, 100)
    try:
        p, a, nb = ctypes.POINTER(Seg)(), ctypes.POINTER(ctypes.c_uint8)(), ctypes.c_uint32()
        n = lib.bg_extract(h, recs, len(recs), ctypes.byref(p), ctypes.byref(a), ctypes.byref(nb))
        arena = ctypes.string_at(a, nb.value) if nb.value else b""
        want, _ = bgp_ref.extract(recs, linktype)
        assert n == len(want)
        for i in range(n):
            segs_equal(p[i], arena, want[i])
        return want
    finally:
        lib.bg_free(h)


SHAPES = bc.shapes()


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_extraction_shapes(lib, name):
    linktype, recs, n = SHAPES[name]
    got = extract_both(lib, recs, linktype)
    assert len(got) == n
    if name == "caplen_cut":
        assert len(got[0]["data"]) == len(bc.bgp_msg(2, b"shape")) - 9
    if name == "v4_in_v6_tunnel":
        assert got[0]["side"][0] and got[0]["side"][1] == bc.A6  # the side is the first IP layer's address


# ---------------------------------------------------------------- 2. random streams
@pytest.fixture(scope="module")
def corpora():
    return {seed: bc.corpus(STREAMS, seed) for seed in (11, 12)}


@pytest.mark.parametrize("seed", [11, 12])
def test_random_streams_event_by_event(lib, corpora, seed):
    rng = np.random.default_rng(seed + 100)
    n = Native(lib, num_periods=3)
    events = held = closed = 0
    try:
        for i, recs in enumerate(corpora[seed]):
            n.reset()
            if i % 50 == 0:
                extract_both(lib, b"".join(recs))
            # one batch, or cut at random records
            cuts = sorted(set(int(x) for x in rng.integers(0, len(recs) + 1, int(rng.integers(0, 4))))) if i % 2 else []
            parts = [recs[a:b] for a, b in zip([0] + cuts, cuts + [len(recs)]) if a < b]
            for k, part in enumerate(parts):
                n.feed(b"".join(part), eoc=(i % 3 == 0 and k == len(parts) - 1))
            n.check()
            events += len(n.ref.events)
            held += sum(len(s.held) for c in n.ref.conns.values() for s in c.sides)
            closed += sum(c.closed_at is not None for c in n.ref.conns.values())
    finally:
        n.close()
    # the corpus reaches what it is meant to reach
    assert events > 3 * STREAMS and held > 0 and closed > STREAMS // 4


def test_batch_cuts_do_not_change_the_result(lib, corpora):
    for recs in corpora[11][:150]:
        one = run(lib, [b"".join(recs)], eoc=True)
        for cut in range(1, len(recs), max(1, len(recs) // 6)):
            assert run(lib, [b"".join(recs[:cut]), b"".join(recs[cut:])], eoc=True) == one


# ---------------------------------------------------------------- targeted reassembly cases
def counts(win):
    w = win["wire_packets"]
    return [w[k] for k in ("open", "update", "notification", "keepalive", "routerefresh")]


def test_chunk_lengths_and_type_bytes(lib):
    a, _, syn = bc.opened()
    recs = syn + b"".join([a.send(bc.bgp_msg(4)[:18], T0, 0), a.send(bc.bgp_msg(4), T0, 1), a.send(bc.bgp_msg(0), T0, 2),
                     a.send(bc.bgp_msg(6), T0, 3), a.send(bc.bgp_msg(5, b"rr"), T0, 4),
                     a.send(bc.bgp_msg(1) + bc.bgp_msg(2) + bc.bgp_msg(2), T0, 5)])
    win, ev = run(lib, [recs])
    # 18 bytes, type 0 and type 6: no event at all; three messages in one chunk: one event
    assert counts(win) == [1, 0, 0, 1, 1] and win["wire_packets"]["events"] == 3 == win["wire_packets"]["total"]
    assert [e[3] for e in ev] == [19, 21, 57]


@pytest.mark.parametrize("gap,events", [(1, 2), (10, 2), (100, 1), (12345, 1)])
def test_missing_bytes_text(lib, gap, events):
    """the flushed fragment goes out behind "[N bytes missing]": with 17 characters byte 18 is the
    fragment's second byte, with 18 its first, with 19 or more it falls in the text"""
    a, b, syn = bc.opened()
    first = a.send(bc.bgp_msg(1), T0, 0)
    a.skip(gap)
    held = a.send(bytes([3, 3]) + bytes(30), T0, 1)
    other = b.send(bc.bgp_msg(0), T0, 2)  # the side changes: A's fragment is flushed
    win, ev = run(lib, [syn + first + held + other])
    assert win["wire_packets"]["events"] == events
    if events == 2:
        assert counts(win) == [1, 0, 1, 0, 0] and ev[1][3] == len("[%d bytes missing]" % gap) + 32


@pytest.mark.parametrize("after,closes", [(29, False), (30, True), (31, True)])
def test_foreign_tcp_times_a_connection_out(lib, after, closes):
    a, _, syn = bc.opened()
    recs = syn + a.send(bc.bgp_msg(1), T0, 0) + a.send(bc.bgp_msg(4), T0 + 1, 0) + bc.foreign(T0 + 1 + after) + a.send(bc.bgp_msg(4), T0 + 1 + after, 5)
    win, _ = run(lib, [recs])
    assert win["wire_packets"]["keepalive"] == (1 if closes else 2)
    # a UDP record that late closes nothing
    a, _, syn = bc.opened()
    recs = syn + a.send(bc.bgp_msg(1), T0, 0) + a.send(bc.bgp_msg(4), T0 + 1, 0) + bc.filler(T0 + 40) + a.send(bc.bgp_msg(4), T0 + 1, 9)
    assert run(lib, [recs])[0]["wire_packets"]["keepalive"] == 2


@pytest.mark.parametrize("after,reopens", [(299, False), (300, True)])
def test_closed_key_is_reclaimed(lib, after, reopens):
    a, _, syn = bc.opened()
    recs = (syn + a.send(bc.bgp_msg(1), T0, 0) + a.send(b"", T0 + 1, 0, bc.RST) + a.send(bc.bgp_msg(2), T0 + 2, 0)
            + a.send(bc.bgp_msg(4), T0 + 1 + after, 0))
    n = Native(lib)
    n.feed(recs)
    win = n.check()
    assert counts(win) == [1, 0, 0, 1 if reopens else 0, 0]
    # (the reopened connection starts with data: delivered with endTime {0,0}, put with it, and
    # closed by the clean-up behind its own packet, as in the reference)
    assert lib.bg_open_connections(n.h) == 0
    n.close()


def test_more_than_50_held_fragments(lib):
    a, _, syn = bc.opened()
    recs = [syn, a.send(bc.bgp_msg(1), T0, 0)]
    a.skip(1)
    recs += [a.send(bc.bgp_msg(4), T0, 1 + i) for i in range(50)]
    win, _ = run(lib, [b"".join(recs)])
    assert counts(win) == [1, 0, 0, 0, 0]  # 50 held: nothing flushed
    recs.append(a.send(bc.bgp_msg(2), T0, 60))
    win, ev = run(lib, [b"".join(recs)])
    # the 51st flushes all: the first behind a 17-character text (byte 18 = 0xff: no event), 49 keepalives, the update
    assert counts(win) == [1, 1, 0, 49, 0] and len(ev) == 51


def test_sequence_wrap_overlap_and_syn_data(lib):
    a, b = bc.session(seq_a=0xFFFFFFF0, seq_b=0xFFFFFFFF)
    recs = [b.send(b"", T0, 0, bc.SYN)]
    recs.append(a.send(bc.bgp_msg(1), T0, 1, bc.SYN | bc.PSH))      # SYN carrying data: next = seq + 19 + 1 (wraps)
    assert a.seq == 4 and b.seq == 0
    recs.append(a.send(bc.bgp_msg(2), T0, 2))
    recs.append(a.send(bc.bgp_msg(2), T0, 3, seq=4))                # a retransmission: nothing new
    recs.append(a.send(bytes(5) + bc.bgp_msg(3), T0, 4, seq=a.seq - 5))  # five old bytes, then a new message
    a.skip(19)
    recs.append(b.send(bc.bgp_msg(4), T0, 5))
    win, ev = run(lib, [b"".join(recs)])
    assert counts(win) == [1, 1, 1, 1, 0]


def test_a_connection_that_starts_with_data(lib):
    """endTime is {0,0} until a connection's second packet, and a delivery puts the connection into
    the LRU list with endTime: data in the first packet is an event stamped {0,0}, and the clean-up
    behind that packet closes the connection (the reference's behaviour, not a definition of ours)"""
    a, _ = bc.session()
    win, ev = run(lib, [a.send(bc.bgp_msg(1), T0, 0) + a.send(bc.bgp_msg(4), T0, 1)])
    assert counts(win) == [1, 0, 0, 0, 0] and ev == [(0, 0, 1, 19)]


def test_fin_and_rst_in_either_order(lib):
    for first, second, late in ((bc.FIN | bc.ACK, bc.FIN | bc.ACK, 0), (bc.RST, bc.FIN | bc.ACK, 0), (bc.FIN | bc.ACK, bc.RST, 0)):
        a, b, syn = bc.opened()
        recs = syn + a.send(bc.bgp_msg(1), T0, 0) + b.send(bc.bgp_msg(1), T0, 1) + a.send(b"", T0, 2, first) + b.send(bc.bgp_msg(4), T0, 3)
        recs += b.send(b"", T0, 4, second) + a.send(bc.bgp_msg(2), T0, 5) + b.send(bc.bgp_msg(2), T0, 6)
        n = Native(lib)
        n.feed(recs)
        win = n.check()
        # a RST closes at once; after a FIN the other side still speaks; nothing after the close counts
        assert counts(win) == [2, 0, 0, 0 if first == bc.RST else 1, 0]
        assert lib.bg_open_connections(n.h) == 0
        n.close()


# ---------------------------------------------------------------- 3. sanitizer run
def test_sanitizers_standalone(lib, corpora, tmp_path):
    """the corpus through extraction and manager under ASan + UBSan, as a program of its own"""
    cxx = shutil.which("g++")
    assert cxx
    exe = str(tmp_path / "bgp_asan")
    csrc = os.path.join(ROOT, "pktvisor_amd", "csrc")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan", "-o", exe,
                           os.path.join(NATIVE_DIR, "bgp_asan_main.cpp"), os.path.join(NATIVE_DIR, "bgp_harness.cpp"),
                           os.path.join(csrc, "pv_bgp.cpp")])
    path = str(tmp_path / "corpus.recs")
    with open(path, "wb") as f:
        for seed in sorted(corpora):
            for recs in corpora[seed]:
                f.write(b"".join(recs) + bc.MARKER)
        for _lt, recs, _n in (v for v in SHAPES.values() if v[0] == 1):
            f.write(recs + bc.MARKER)
    # (the runtimes are linked statically and the program runs with the inherited environment)
    for batch in ("7", "100000"):
        out = subprocess.run([exe, "1", batch, path], capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
        assert out.stderr == ""
        assert out.stdout.startswith("%d streams" % (2 * (2 * STREAMS + sum(v[0] == 1 for v in SHAPES.values()))))


# ---------------------------------------------------------------- 4. manager cases
def test_period_shifts_on_own_events(lib):
    recs = bc.keepalive_stream(700, step_us=300000)  # 210 s: three shifts
    n = Native(lib, num_periods=3)
    n.feed(recs)
    assert lib.bg_periods(n.h) == 3
    wins = [n.check(p) for p in range(3)]
    assert [w["period"]["length"] for w in wins] == [0, 60, 60]
    assert wins[0]["period"]["start_ts"] == T0 + 180 and sum(w["wire_packets"]["events"] for w in wins) == 698 - 198
    merged = n.check(3, merged=True)
    assert merged["wire_packets"]["events"] == 500 and merged["period"]["length"] == 120
    # a foreign record 60 s later shifts nothing; the heartbeat does
    n.feed(bc.filler(T0 + 400) + bc.foreign(T0 + 400, 1))
    assert n.check()["period"]["start_ts"] == T0 + 180
    lib.bg_check_period_shift(n.h, T0 + 400, 0)
    n.ref.check_period_shift(T0 + 400, 0)
    assert n.check()["period"]["start_ts"] == T0 + 400 and n.check(1)["period"]["length"] == 220
    n.close()


def test_sampling_follows_the_pinned_generator(lib):
    g = json.load(open(os.path.join(GOLDEN, "jsf32_seed1.json")))["first"]
    k = min(len(g), 200)
    recs = bc.keepalive_stream(k + 2)
    n = Native(lib, num_periods=1, rate=50)
    n.feed(recs)
    win = n.check()
    assert win["wire_packets"]["events"] == k and win["wire_packets"]["deep_samples"] == sum(x % 100 < 50 for x in g[:k])
    # a reset restores the seed and forgets the connection
    n.reset()
    n.feed(recs)
    assert n.check() == win
    n.close()


def test_start_and_end_stamps(lib):
    a, _, syn = bc.opened()
    recs = bc.filler(T0 - 5, 123) + syn + a.send(bc.bgp_msg(1), T0, 7) + a.send(bc.bgp_msg(4), T0 + 2, 999999)
    n = Native(lib, num_periods=1)
    n.feed(recs)
    assert n.check()["period"] == {"start_ts": T0 - 5, "length": 0}  # the input's first record, any protocol
    lib.bg_set_end(n.h, T0 + 9, 5)
    n.ref.set_end(T0 + 9, 5)
    assert n.check()["period"]["length"] == 14
    st = (ctypes.c_int64 * 4)()
    assert lib.bg_stamps(n.h, 0, st) == 0 and list(st) == [T0 - 5, 123000, T0 + 9, 5]
    assert n.events() == [(T0, 7000, 1, 19), (T0 + 2, 999999000, 4, 19)]
    n.close()


def test_end_of_capture_flushes_held_fragments(lib):
    a, b, syn = bc.opened()
    c, _, syn2 = bc.opened(port=40002)
    recs = syn + syn2 + a.send(bc.bgp_msg(1), T0, 0)
    a.skip(1)
    recs += a.send(bytes([0, 2]) + bytes(20), T0, 1) + c.send(bc.bgp_msg(1), T0, 2)
    c.skip(10)
    recs += c.send(bytes([5]) + bytes(20), T0, 3)
    assert run(lib, [recs])[0]["wire_packets"]["events"] == 2
    win, ev = run(lib, [recs], eoc=True)
    assert counts(win) == [2, 1, 0, 0, 1]
    # closeAllConnections visits the connections in ascending flow key
    keys = {s["sport"]: s["fkey"] for s in bgp_ref.extract(recs)[0]}
    assert [e[2] for e in ev[2:]] == ([2, 5] if keys[40001] < keys[40002] else [5, 2])


# ---------------------------------------------------------------- 5. config
def test_config_validation():
    assert pvcfg.bgp_start({}) == {"recorded_stream": False}
    assert pvcfg.bgp_start({"recorded_stream": True, "num_periods": 3, "deep_sample_rate": 50})["recorded_stream"] is True
    with pytest.raises(pvcfg.StreamHandlerException) as e:
        pvcfg.bgp_start({"xact_ttl_ms": 5})
    assert str(e.value) == ("xact_ttl_ms is an invalid/unsupported config or filter. The valid configs/filters are: "
                            "recorded_stream, " + ", ".join(pvcfg.WINDOW_CONFIG_DEFS))


def test_header_and_bindings_agree():
    hdr = open(os.path.join(ROOT, "include", "pvgpu.h")).read()
    assert "#define PV_HANDLER_BGP 8u" in hdr and pa.PV_HANDLER_BGP == 8
    assert "pv_set_bgp" in pa.EXPORTS and "pv_bgp_timing" in pa.EXPORTS
    assert ctypes.sizeof(pa.pv_bgp_config) == 8
