"""Flow handler on the CPU: the product's datagram check and decoder (pv_flow.h) and host manager
(pv_flow.cpp), compiled for the host by tests/native_flow, against the reference's known answers
(tests/golden/kat_flow.json) and the Python model (tests/flow_ref.py). No GPU."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

import pktvisor_amd as pa
from pktvisor_amd import config as pvcfg
from tests import flow_cases as fc
from tests import flow_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native_flow", "libpvflow_host.so")
GOLDEN = os.path.join(ROOT, "tests", "golden")
KAT = json.load(open(os.path.join(GOLDEN, "kat_flow.json")))["nf5.pcap"]
REF_SKETCH = os.path.join(ROOT, "oracle", "_ref", "ref_sketch")
CSV = os.path.join(GOLDEN, "flow_ports.csv")
T0 = fc.T0


class Row(ctypes.Structure):
    _fields_ = [("last", ctypes.c_uint16), ("first", ctypes.c_uint16), ("protocol", ctypes.c_uint32), ("name", ctypes.c_char_p)]


def port_rows():
    return pvcfg.iana_port_rows(open(CSV, newline="").read())


@pytest.fixture(scope="module")
def lib():
    subprocess.check_call(["make", "-s", "-C", os.path.dirname(NATIVE)])
    h = ctypes.CDLL(NATIVE)
    P, U32, I64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int64
    h.fl_new.argtypes = [U32] * 7 + [ctypes.POINTER(ctypes.c_uint16), U32, ctypes.POINTER(Row), U32]
    h.fl_new.restype = P
    h.fl_free.argtypes = [P]
    h.fl_feed.argtypes = [P, ctypes.c_char_p, ctypes.c_size_t]
    h.fl_set_end.argtypes = [P, I64, I64]
    h.fl_check_period_shift.argtypes = [P, I64, I64]
    h.fl_periods.argtypes = [P]
    h.fl_periods.restype = U32
    h.fl_stats.argtypes = [P, ctypes.POINTER(ctypes.c_uint64)]
    h.fl_json.argtypes = [P, U32, ctypes.c_int]
    h.fl_json.restype = P
    h.fl_service.argtypes = [P, U32, ctypes.c_int]
    h.fl_service.restype = P
    h.fl_free_str.argtypes = [P]
    h.fl_coupon.argtypes = [ctypes.c_int, U32, ctypes.c_char_p]
    h.fl_coupon.restype = U32
    h.fl_estimate.argtypes = [ctypes.c_int, ctypes.POINTER(U32), ctypes.c_char_p, U32, ctypes.c_int]
    h.fl_estimate.restype = ctypes.c_double
    return h


class Native:
    """the harness next to a flow_ref.Manager with the same config"""

    def __init__(self, lib, cfg=None, linktype=1, ts_nano=0, num_periods=5, rate=100, rows=(), topn=10, pct=0):
        cfg = cfg or {}
        self.lib, self.lt, self.ns = lib, linktype, ts_nano
        start = pvcfg.flow_start(cfg)
        ports = (ctypes.c_uint16 * 8)(*start["ports"])
        self._rows = (Row * max(1, len(rows)))(*[Row(l, f, p, n.encode()) for l, f, p, n in rows])
        self.h = lib.fl_new(linktype, ts_nano, num_periods, rate, start["groups"] & 0x7ff, topn, pct, ports, len(start["ports"]),
                            self._rows, len(rows))
        self.ref = flow_ref.Manager(num_periods, rate, cfg, rows, topn, pct)

    def feed(self, recs: bytes):
        self.lib.fl_feed(self.h, recs, len(recs))
        self.ref.feed(recs, self.lt, self.ns)

    def set_end(self, sec, nsec=0):
        self.lib.fl_set_end(self.h, sec, nsec)
        self.ref.set_end(sec, nsec)

    def text(self, p):
        txt = ctypes.string_at(p).decode()
        self.lib.fl_free_str(p)
        return txt

    def json(self, period=0, merged=False):
        txt = self.text(self.lib.fl_json(self.h, period, int(merged)))
        assert not txt.startswith("!"), txt
        return json.loads(txt)["flow"]

    def stats(self):
        out = (ctypes.c_uint64 * 3)()
        self.lib.fl_stats(self.h, out)
        return {"datagrams": out[0], "invalid": out[1], "invalid_v9_v10": out[2]}

    def check(self, period=0, merged=False):
        got = self.json(period, merged)
        assert got == self.ref.window(period, merged)
        assert self.stats() == self.ref.stats
        return got

    def close(self):
        self.lib.fl_free(self.h)


def check_kat(win: dict):
    assert win["period"]["start_ts"] == KAT["start_ts"]
    assert win["wire_packets"] == {"events": KAT["events"], "deep_samples": KAT["deep_samples"]}
    dev = win["devices"][KAT["device"]]
    assert dev["records_flows"] == KAT["records_flows"]
    ifc = dev["interfaces"][KAT["interface"]]
    assert ifc["cardinality"] == KAT["cardinality"]
    for name, want in KAT["top0"].items():
        for k, v in want.items():
            assert ifc[name][0][k] == v, (name, k)


def fixture():
    return pa.read_pcap(os.path.join(GOLDEN, "nf5.pcap"))


def test_fixture_known_answers(lib):
    lt, ns, recs = fixture()
    n = Native(lib, {"enable": ["top_tos"]}, lt, ns, num_periods=1, rows=port_rows())
    n.feed(recs)
    check_kat(n.check())
    assert n.stats() == {"datagrams": 2, "invalid": 0, "invalid_v9_v10": 0}
    n.close()


@pytest.mark.parametrize("cfg", [{}, {"enable": ["all"]}, {"ports": [2055]}, {"ports": [2056]}, {"disable": ["by_bytes", "counters"]},
                                 {"disable": ["all"], "enable": ["top_interfaces", "by_packets"]}],
                         ids=["defaults", "all", "port", "other-port", "packets-only", "interfaces"])
def test_fixture_groups_and_ports(lib, cfg):
    lt, ns, recs = fixture()
    n = Native(lib, cfg, lt, ns, num_periods=1, rows=port_rows())
    n.feed(recs)
    n.check()
    n.close()


def test_fixture_mutations_against_the_model(lib):
    """seeded byte flips in the NetFlow header and count, truncations, lengths one short and one over"""
    lt, ns, recs = fixture()
    seen = set()
    for m in fc.fixture_mutations(recs, 200):
        n = Native(lib, {"enable": ["all"]}, lt, ns, num_periods=2, rate=50)
        n.feed(m)
        n.check()
        seen.add(tuple(n.stats().values()))
        n.close()
    assert len(seen) > 2  # accepted, refused and version 9 / 10 outcomes all occur


def synthetic():
    """the shapes the GPU cases use, as one stream"""
    out = []
    for v in (1, 5, 7):
        out.append(fc.packet(fc.datagram(v, fc.flows_n(fc.MAXFLOWS[v], v)), T0, v))
        out.append(fc.packet(fc.datagram(v, fc.flows_n(1, 40 + v)), T0 + 1, v, vlan=5))
        out.append(fc.packet(fc.datagram(v, fc.flows_n(2, 50 + v), time=(0, 0)), T0 + 2, v, v6=True))
        out.append(fc.packet(fc.datagram(v, fc.flows_n(3, 60 + v)), T0 + 3, v, ihl=6))
        out.append(fc.packet(fc.datagram(v, fc.flows_n(2), count=fc.MAXFLOWS[v] + 1), T0 + 4))
        out.append(fc.packet(fc.datagram(v, fc.flows_n(2), cut=1), T0 + 4))
        out.append(fc.packet(fc.datagram(v, fc.flows_n(2), extra=b"\0"), T0 + 4))
    out.append(fc.packet(fc.datagram(9, []), T0 + 5))
    out.append(fc.packet(b"\0\x0a", T0 + 5))
    out.append(fc.packet(fc.datagram(5, [fc.flow(src="0.0.0.0", sport=0), fc.flow(dst="0.0.0.0", dport=0)]), T0 + 6))
    out.append(fc.packet(fc.datagram(5, fc.flows_n(4)), T0 + 70, caplen=100))
    out.append(fc.packet(fc.datagram(5, fc.flows_n(4), time=(T0 + 70, 1)), T0 + 7, dp=9995))
    out.append(fc.filler(T0 + 7))
    return b"".join(out)


@pytest.mark.parametrize("cfg", [{"enable": ["all"]}, {"enable": ["all"], "ports": [2055]}, {}], ids=["all", "port", "defaults"])
def test_synthetic_stream_against_the_model(lib, cfg):
    n = Native(lib, cfg, num_periods=3, rows=port_rows())
    n.feed(synthetic())
    n.check()
    # (the one datagram stamped a minute on goes to port 9995: no shift where 2055 alone is configured)
    assert lib.fl_periods(n.h) == len(n.ref.buckets) == (1 if cfg.get("ports") else 2)
    if not cfg.get("ports"):
        n.check(1)
    n.check(3, merged=True)
    assert n.ref.stats["invalid_v9_v10"] == 1 and n.ref.stats["invalid"] >= 10
    n.close()


def test_deep_sampling_and_two_batches(lib):
    n = Native(lib, {"enable": ["all"]}, num_periods=2, rate=50)
    a = b"".join(fc.packet(fc.datagram(5, fc.flows_n(3, i), time=(T0 + i, 0)), T0 + i) for i in range(40))
    b = b"".join(fc.packet(fc.datagram(7, fc.flows_n(2, i), time=(T0 + 55 + i, 0)), T0 + 55 + i) for i in range(20))
    n.feed(a)
    n.feed(b)
    w = n.check()
    assert 0 < w["wire_packets"]["deep_samples"] < w["wire_packets"]["events"]
    assert lib.fl_periods(n.h) == 2
    n.check(1)
    n.check(2, merged=True)
    n.close()


def test_decoder_and_manager_under_address_and_undefined_sanitizers(tmp_path):
    """the fixture, its mutations and the synthetic stream through a stand-alone program built with
    -fsanitize=address,undefined: exit 0, no report"""
    exe = str(tmp_path / "flow_asan")
    nd = os.path.join(ROOT, "tests", "native_flow")
    csrc = os.path.join(ROOT, "pktvisor_amd", "csrc")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan", "-o", exe, os.path.join(nd, "flow_asan_main.cpp"),
                           os.path.join(nd, "flow_harness.cpp"), os.path.join(csrc, "pv_flow.cpp"), os.path.join(csrc, "pv_dhcp.cpp")])
    _, _, recs = fixture()
    files = []
    for name, data in [("nf5", recs), ("synthetic", synthetic())] + [("m%d" % i, m) for i, m in enumerate(fc.fixture_mutations(recs, 60))]:
        p = tmp_path / (name + ".recs")
        p.write_bytes(data)
        files.append(str(p))
    r = subprocess.run([exe, "1"] + files, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stderr == "" and r.stdout.startswith("read ")


def test_set_end_before_the_first_batch_is_ignored(lib):
    n = Native(lib, {}, num_periods=2)
    n.set_end(T0 + 5)
    assert n.check()["period"] == {"start_ts": 0, "length": 0}
    n.feed(fc.packet(fc.datagram(5, fc.flows_n(2)), T0))
    n.set_end(T0 + 7)
    assert n.check()["period"] == {"start_ts": T0, "length": 7}
    n.close()


def test_top_geo_without_a_database_writes_empty_lists(lib):
    """FlowMetricsBucket::to_json (:1186-1216) writes the four geo lists whatever they hold; nothing fills them here"""
    geo = {"top_geo_loc_bytes", "top_asn_bytes", "top_geo_loc_packets", "top_asn_packets"}
    for cfg, want in (({"enable": ["top_geo"]}, geo), ({"enable": ["all"]}, geo), ({}, set()),
                      ({"enable": ["top_geo"], "disable": ["by_packets"]}, {"top_geo_loc_bytes", "top_asn_bytes"}),
                      ({"disable": ["all"], "enable": ["top_geo", "by_packets"]}, {"top_geo_loc_packets", "top_asn_packets"})):
        n = Native(lib, cfg)
        n.feed(fc.packet(fc.datagram(5, fc.flows_n(6)), T0))
        ifs = n.check()["devices"]["10.0.0.2"]["interfaces"]
        assert len(ifs) == 5
        for ifc in ifs.values():
            assert {k for k in ifc if "geo" in k or "asn" in k} == want
            assert all(ifc[k] == [] for k in want)
        n.close()


# ---------------------------------------------------------------- config
def test_invalid_config_text():
    # src/handlers/flow/test_flows.cpp:568
    with pytest.raises(pa.StreamHandlerException) as e:
        pvcfg.flow_start({"invalid_config": True})
    assert str(e.value) == (
        "invalid_config is an invalid/unsupported config or filter. The valid configs/filters are: device_map, enrichment, "
        "only_device_interfaces, only_ips, only_ports, only_directions, geoloc_notfound, asn_notfound, summarize_ips_by_asn, "
        "subnets_for_summarization, exclude_asns_from_summarization, exclude_unknown_asns_from_summarization, "
        "exclude_ips_from_summarization, sample_rate_scaling, recorded_stream, deep_sample_rate, num_periods, topn_count, "
        "topn_percentile_threshold")


def test_invalid_group_text():
    with pytest.raises(pa.StreamHandlerException) as e:
        pvcfg.flow_start({"enable": ["top_nothing"]})
    assert str(e.value) == ("top_nothing is an invalid/unsupported metric group. The valid groups are: all, by_bytes, by_packets, "
                            "cardinality, conversations, counters, top_geo, top_interfaces, top_ips, top_ips_ports, top_ports, top_tos")


@pytest.mark.parametrize("key", pvcfg.FLOW_NOT_BUILT)
def test_keys_not_built_raise(key):
    with pytest.raises(pvcfg.ConfigException, match=f"^{key} is not supported by the GPU flow handler$"):
        pvcfg.flow_start({key: True})


def test_defaults_and_own_keys():
    s = pvcfg.flow_start({"sample_rate_scaling": False, "recorded_stream": True, "ports": [2055, 9995]})
    want = 0
    for g in pvcfg.FLOW_DEFAULT_GROUPS:
        want |= pvcfg.FLOW_GROUP_DEFS[g]
    assert s == {"groups": want | pvcfg.GROUPS_SET, "recorded_stream": True, "ports": [2055, 9995]}
    assert flow_ref.groups_of({}) == set(pvcfg.FLOW_DEFAULT_GROUPS)
    for bad in ([70000], ["2055"], list(range(9)), 2055):
        with pytest.raises(pvcfg.ConfigException):
            pvcfg.flow_start({"ports": bad})


# ---------------------------------------------------------------- port names
def test_port_csv_rows():
    rows = port_rows()
    assert (23, 23, 6, "telnet") in rows and (520, 520, 17, "router") in rows and (6063, 6000, 6, "x11") in rows
    assert all(r[2] in (6, 17) for r in rows) and not any(r[0] == 24 for r in rows)  # sctp and the nameless row are dropped


def test_port_csv_bad_row_takes_the_next_line_with_it():
    text = ("Service Name,Port Number,Transport Protocol,Description\n"
            "a,1,tcp,ok\n"
            "b,2,tcp,a description, with a comma\n"
            "c,3,tcp,lost with the row before it\n"
            "d,x4,udp,no number\n"
            "e,5,udp,lost too\n"
            " f , 6-8 , udp ,blanks are trimmed\n"
            "g,9,tcp\n")
    assert pvcfg.iana_port_rows(text) == [(1, 1, 6, "a"), (8, 6, 17, "f")]


def test_port_names_and_the_range_quirk(lib):
    rows = port_rows()
    n = Native(lib, {}, rows=rows)
    names = flow_ref.PortNames(rows)
    for port, udp in [(23, False), (23, True), (520, True), (520, False), (2048, False), (6000, False), (6030, True), (6063, False),
                      (5999, False), (6064, False), (1, False), (100, True), (4000, False), (65535, True), (81, False), (444, True)]:
        got = n.text(lib.fl_service(n.h, port, int(udp)))
        assert got == names.service(port, udp), port
    # lower_bound on the rows' last ports: a port inside a range takes the range's name, one below it
    # stays a number, and so does one above every row
    assert n.text(lib.fl_service(n.h, 6030, 0)) == "x11" and n.text(lib.fl_service(n.h, 5999, 0)) == "5999"
    assert n.text(lib.fl_service(n.h, 6064, 0)) == "6064" and n.text(lib.fl_service(n.h, 520, 0)) == "efs"
    n.close()
    # the quirk: a single-port row is found for its own port only, but a row whose first port is 0 names
    # every unlisted port below it
    q = Native(lib, {}, rows=[(100, 0, 6, "low"), (200, 150, 6, "mid")])
    assert [q.text(lib.fl_service(q.h, p, 0)) for p in (50, 100, 120, 150, 200, 201)] == ["low", "low", "120", "mid", "mid", "201"]
    qn = flow_ref.PortNames([(100, 0, 6, "low"), (200, 150, 6, "mid")])
    assert [qn.service(p, False) for p in (50, 100, 120, 150, 200, 201)] == ["low", "low", "120", "mid", "mid", "201"]
    q.close()


# ---------------------------------------------------------------- the model's exact counts
@pytest.mark.skipif(not os.path.exists(REF_SKETCH), reason="oracle/_ref not built")
def test_sketch_estimates_of_the_cases_are_their_distinct_counts():
    """the model counts distinct values exactly; the reference's sketch, fed the very values of the
    cases, rounds to the same number"""
    def ref(cmd):
        return float(subprocess.run([REF_SKETCH], input=cmd.encode(), capture_output=True, check=True).stdout.decode().split()[0])

    m = flow_ref.Manager(1, 100, {"enable": ["all"]})
    m.feed(synthetic())
    m.feed(fixture()[2])
    # every flow of the sequence the cases take theirs from (tests/flow_cases.py flows_n), and the zero-field flows
    m.feed(b"".join(fc.packet(fc.datagram(5, fc.flows_n(30, b)), T0) for b in range(0, 360, 30)))
    m.feed(fc.packet(fc.datagram(5, fc.zero_flows()), T0))
    checked = 0
    for dev in m.buckets[0].devices.values():
        for ifc in dev.ifs.values():
            for q, vals in enumerate(ifc.card):
                if not vals:
                    continue
                assert len(vals) <= 64
                for merged in (0, 1):
                    if q == 0:
                        est = ref(f"cpc_str {merged} {len(vals)} " + " ".join(sorted(vals)) + "\n")
                    else:
                        ints = [int.from_bytes(v, "little") if isinstance(v, bytes) else v for v in vals]
                        est = ref(f"cpc_u32 {merged} {len(ints)} " + " ".join(map(str, ints)) + "\n")
                    assert round(est) == len(vals)
                checked += 1
    assert checked > 10


# ---------------------------------------------------------------- the manager's coupons
def coupon_items():
    """(kind, value, text) of the known-answer items: addresses with the top bit clear and set, ports below and
    from 32768 (update(uint16_t) widens through int16), strings of 1, 15, 16, 17 and 40 bytes (Murmur's tail and blocks)"""
    return ([(0, v, b"") for v in (0, 1, 0x0100007F, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF, 0x0201A8C0)] +
            [(1, v, b"") for v in (1, 23, 2055, 32767, 32768, 40000, 65535)] +
            [(2, 0, t) for t in (b"a", b"10.0.0.1:80/10.0.0.2:1024", b"x" * 15, b"y" * 16, b"z" * 17, b"192.168.12.1:21509/10.0.0.2:23" + b"!" * 10)])


def test_coupon_known_answers(lib):
    """tests/golden/kat_flow.json "coupons": taken from this code once the test below had compared it with the
    reference's own sketch"""
    kat = json.load(open(os.path.join(GOLDEN, "kat_flow.json")))["coupons"]
    got = [lib.fl_coupon(k, v, t) for k, v, t in coupon_items()]
    assert got == kat
    # a port from 32768 on is not hashed as its unsigned value, an address with the top bit set neither
    assert lib.fl_coupon(1, 40000, b"") == lib.fl_coupon(0, 40000 + 0xFFFF0000, b"") != lib.fl_coupon(0, 40000, b"")


@pytest.mark.skipif(not os.path.exists(REF_SKETCH), reason="oracle/_ref not built")
@pytest.mark.parametrize("merged", [0, 1])
def test_coupons_against_the_reference_sketch(lib, merged):
    """3,000 distinct items of each kind through the manager's coupons and estimator, and through the reference's
    cpc_sketch: the same estimate to the last bits only if seed, tail handling, widening and coupon are the same.
    (update(uint16_t v) is update(int16_t(v)), which is what update(uint32_t) makes of v sign-extended to 32 bits:
    cpc_sketch_impl.hpp:124-150.)"""
    def ref(cmd):
        return float(subprocess.run([REF_SKETCH], input=cmd.encode(), capture_output=True, check=True).stdout.decode().split()[0])

    rng = np.random.default_rng(5)
    n = 3000
    addrs = [int(x) for x in rng.choice(1 << 32, n, replace=False)]
    ports = [int(x) for x in rng.choice(1 << 16, n, replace=False)]
    texts = ["%d.%d.%d.%d:%d/%s" % (a & 255, (a >> 8) & 255, (a >> 16) & 255, a >> 24, p, "c" * (i % 23)) for i, (a, p) in enumerate(zip(addrs, ports))]
    arr = lambda v: (ctypes.c_uint32 * len(v))(*v)  # noqa: E731
    want = ref(f"cpc_u32 {merged} {n} " + " ".join(map(str, addrs)) + "\n")
    assert lib.fl_estimate(0, arr(addrs), None, n, merged) == pytest.approx(want, rel=1e-12)
    want = ref(f"cpc_u32 {merged} {n} " + " ".join(str(p if p < 32768 else p + 0xFFFF0000) for p in ports) + "\n")
    assert lib.fl_estimate(1, arr(ports), None, n, merged) == pytest.approx(want, rel=1e-12)
    want = ref(f"cpc_str {merged} {n} " + " ".join(texts) + "\n")
    assert lib.fl_estimate(2, None, b"".join(t.encode() + b"\0" for t in texts), n, merged) == pytest.approx(want, rel=1e-12)
