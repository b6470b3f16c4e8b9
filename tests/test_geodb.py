"""The host GeoIP / ASN database reader (pv_geodb_*): known answers of the reference's
test_geoip.cpp, agreement with an independent Python reader on every leaf of the fixture and
synthetic trees, refusals of malformed files, and a sanitizer run of the stand-alone reader."""
import ipaddress
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import pktvisor_amd as pa
from tests import geo_cases
from tests import mmdb_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
CITY = os.path.join(GOLD, "GeoIP2-City-Test.mmdb")
ISP = os.path.join(GOLD, "GeoIP2-ISP-Test.mmdb")
KAT = json.load(open(os.path.join(GOLD, "kat_geo.json"), encoding="utf-8"))


@pytest.fixture(scope="module")
def cases():
    return geo_cases.build()


def test_city_known_answers():
    db = pa.GeoDB(CITY, "city")
    assert db.entries[0] == ("Unknown", "", "")
    for k in KAT["city"]:
        name, lat, lon = db.lookup(k["address"])
        assert name == k["location"], k
        if k["lat"] is not None:
            assert (lat, lon) == (k["lat"], k["lon"]), k


def test_asn_known_answers():
    db = pa.GeoDB(ISP, "asn")
    for k in KAT["asn"]:
        assert db.lookup(k["address"]) == (k["asn"], "", ""), k
    # the empty string (an entry with neither field) is a key of its own, not "Unknown"
    assert db.entries.index(("", "", "")) != 0


def test_open_from_bytes_and_ids_are_a_function_of_the_file():
    data = open(CITY, "rb").read()
    a, b = pa.GeoDB(data, "city"), pa.GeoDB(CITY, "city")
    assert a.entries == b.entries and len(set(a.entries)) == len(a.entries)
    # ordered by the first data offset that renders each string
    rd = R.Reader(data)
    offs = sorted({r - rd.node_count - 16 for _, _, r in rd.leaves() if r > rd.node_count})
    want = [("Unknown", "", "")]
    for o in offs:
        t = R.render_city(rd.data_at(o))
        if t not in want:
            want.append(t)
    assert a.entries == want


def _agree(data, kind, n_random, seed):
    db = pa.GeoDB(data, kind)
    rd = R.Reader(data)
    probes = geo_cases.probe_addresses(data, n_random, seed)
    total = 0
    for alen in (4, 16):
        ids = db.lookup_ids(probes[alen], alen)
        assert ids.size == len(probes[alen]) and int(ids.max(initial=0)) < len(db.entries)
        cache = {}
        for addr, i in zip(probes[alen], ids):
            off = rd.find(addr)
            if off not in cache:
                cache[off] = R.lookup(rd, kind, addr)
            assert db.entries[int(i)] == cache[off], (ipaddress.ip_address(addr), kind)
        total += ids.size
    return total


@pytest.mark.parametrize("path,kind", [(CITY, "city"), (ISP, "asn")])
def test_every_leaf_and_random_addresses_agree_with_python_reader(path, kind):
    assert _agree(open(path, "rb").read(), kind, 10000, 7) > 20000


def test_synthetic_trees_agree_with_python_reader(cases):
    for name, (data, kind) in cases.items():
        _agree(data, kind, 300, 11)


def test_synthetic_tree_answers(cases):
    for rs in (24, 28, 32):
        for fam in ("v4", "v6"):
            db = pa.GeoDB(cases[f"{fam}_rs{rs}"][0], "asn")
            assert db.lookup("128.0.0.0")[0] == "1/half" and db.lookup("255.1.2.3")[0] == "1/half"
            assert db.lookup("127.255.255.255")[0] == "Unknown"
            assert db.lookup("10.200.0.1")[0] == "8/eight" and db.lookup("11.0.0.0")[0] == "Unknown"
            assert db.lookup("11.22.33.77")[0] == "24" and db.lookup("11.22.32.255")[0] == "Unknown"
            assert db.lookup("12.1.2.3")[0] == "32/host" and db.lookup("12.1.2.2")[0] == "Unknown"
        db = pa.GeoDB(cases[f"v6_rs{rs}"][0], "asn")
        assert db.lookup("2001:db8:8000::")[0] == "33/v6 33" and db.lookup("2001:db8:ffff::9")[0] == "33/v6 33"
        assert db.lookup("2001:db8:3fff::")[0] == "Unknown" and db.lookup("2001:db8:7fff::")[0] == "64500/text number"
        assert db.lookup("2001:db8::1")[0] == "128/v6 host" and db.lookup("2001:db8::")[0] == "Unknown"
        assert db.lookup("2001:db8:4000::1")[0] == "64500/text number"
        assert db.lookup("fe80::1")[0] == "7" and db.lookup("fd00::1")[0] == "-5"
        assert db.lookup("ff02::1")[0] == f"{1 << 40}/big"
        # an IPv6 address in an ip_version 4 tree has no entry
        assert pa.GeoDB(cases[f"v4_rs{rs}"][0], "asn").lookup("2001:db8::1")[0] == "Unknown"
    db = pa.GeoDB(cases["v6_no_v4_subtree"][0], "asn")
    assert db.lookup("10.0.0.1")[0] == "Unknown" and db.lookup("2001:db8::1")[0] == "128/v6 host"
    db = pa.GeoDB(cases["v6_early_leaf"][0], "asn")  # ::/96 ends in a leaf after 8 bits: every IPv4 address
    assert db.lookup("10.0.0.1")[0] == "96/early" and db.lookup("200.1.1.1")[0] == "96/early"
    assert db.lookup("::1")[0] == "96/early" and db.lookup("fe80::1")[0] == "7"
    db = pa.GeoDB(cases["one_node_empty"][0], "asn")
    assert db.entries == [("Unknown", "", "")]
    assert db.lookup("1.2.3.4")[0] == "Unknown" and db.lookup("::")[0] == "Unknown"


def test_equal_city_triples_share_an_id(cases):
    db = pa.GeoDB(cases["city_shared_id"][0], "city")
    ids = db.lookup_ids([ipaddress.ip_address(a).packed for a in ("10.1.1.1", "20.1.1.1", "30.1.1.1", "40.1.1.1", "50.1.1.1")], 4)
    assert ids[0] == ids[1] != 0 and ids[2] not in (0, ids[0])
    assert db.entries[ids[0]] == ("EU/Sweden", "58.416700", "15.616700")
    assert db.entries[ids[2]] == ("EU/Sweden", "58.416700", "15.500000")  # same name, another longitude: another key
    assert db.entries[ids[3]] == ("NA/Canada", "", "")
    # no continent, iso_code when names.en is absent, a latitude that is not a double
    assert db.entries[ids[4]] == ("/ZZ/Q/Town", "", "2.500000")
    assert len(db.entries) == 5


# ---------------------------------------------------------------- refusals
def _refused(data, kind="asn"):
    with pytest.raises(pa.PvError) as e:
        pa.GeoDB(bytes(data), kind)
    msg = str(e.value)
    assert "pv_geodb_open failed (-1): " in msg and not msg.endswith(": ")
    return msg


@pytest.mark.parametrize("path,kind", [(CITY, "city"), (ISP, "asn")])
def test_truncated_files_are_refused(path, kind):
    data = open(path, "rb").read()
    # (the metadata is the file's tail: every proper prefix loses part of it or the marker)
    for k in range(64):
        _refused(data[: len(data) * k // 64], kind)
    _refused(data[:-1], kind)


def test_malformed_files_are_refused(cases):
    good = cases["v6_rs24"][0]
    rd = R.Reader(good)
    assert "node_count" in _refused(R.write_mmdb(geo_cases.V4, 24, 6, meta_override={"node_count": 1 << 30}))
    assert "node_count" in _refused(R.write_mmdb(geo_cases.V4, 24, 6, meta_override={"node_count": rd.node_count * 50}))
    assert "record_size 20" in _refused(R.write_mmdb(geo_cases.V4, 24, 6, meta_override={"record_size": R.U16(20)}))
    assert "ip_version 5" in _refused(R.write_mmdb(geo_cases.V4, 24, 6, meta_override={"ip_version": R.U16(5)}))
    _refused(R.write_mmdb(geo_cases.V4, 24, 6, meta_override={"record_size": "24"}))
    # fewer nodes than the tree has: a child index at or past node_count is a data pointer that
    # lands in the tree or outside the data section, or the records decode as no map at all
    short = R.write_mmdb(geo_cases.V4, 32, 4, meta_override={"node_count": 3})
    try:
        db = pa.GeoDB(short, "asn")
        assert int(db.lookup_ids(np.random.default_rng(1).integers(0, 256, 4000, dtype=np.uint8), 4).max()) < len(db.entries)
    except pa.PvError:
        pass
    # a record that points past the data section
    data = bytearray(R.write_mmdb([("128.0.0.0/1", geo_cases.asn(1))], 32, 4))
    data[4:8] = (0x7FFFFFF0).to_bytes(4, "big")  # node 0's right record
    assert "outside the data section" in _refused(data)
    data[4:8] = (1 + 8).to_bytes(4, "big")  # into the 16-byte separator
    assert "outside the data section" in _refused(data)


def test_pointer_to_pointer_is_refused():
    # record -> pointer -> pointer -> map
    target = R.enc(geo_cases.asn(9, "behind two pointers"))
    blob = R.enc(R.RawPtr(5)) + R.enc(R.RawPtr(10)) + target
    data = R.write_mmdb([], 24, 4, raw_data={"10.0.0.0/8": blob})
    assert "pointer to a pointer" in _refused(data)
    # one pointer is followed
    blob = R.enc(R.RawPtr(5)) + target
    db = pa.GeoDB(R.write_mmdb([], 24, 4, raw_data={"10.0.0.0/8": blob}), "asn")
    assert db.lookup("10.9.9.9")[0] == "9/behind two pointers"
    # a pointer past the end of the data section
    assert "pointer past the end" in _refused(R.write_mmdb([], 24, 4, raw_data={"10.0.0.0/8": R.enc(R.RawPtr(4000))}))


def test_nesting_beyond_the_cap_is_refused():
    def nested(depth):
        v = {"autonomous_system_number": R.U32(3)}
        inner = "leaf"
        for _ in range(depth):
            inner = {"m": inner}
        v["deep"] = inner
        return v
    ok = pa.GeoDB(R.write_mmdb([("10.0.0.0/8", nested(20))], 24, 4), "asn")
    assert ok.lookup("10.0.0.1")[0] == "3"
    assert "nested too deep" in _refused(R.write_mmdb([("10.0.0.0/8", nested(40))], 24, 4))
    # far beyond (a recursion the cap must stop early)
    raw = b"\xe2" + R.enc("autonomous_system_number") + R.enc(R.U32(3)) + R.enc("deep") + \
        (b"\xe1" + R.enc("m")) * 100000 + R.enc("leaf")
    assert "nested too deep" in _refused(R.write_mmdb([], 24, 4, raw_data={"10.0.0.0/8": raw}))


def test_bad_arguments():
    with pytest.raises(pa.PvError):
        pa.GeoDB(os.path.join(GOLD, "no_such_file.mmdb"), "city")
    with pytest.raises(pa.PvError):
        pa.GeoDB(CITY, "country")
    db = pa.GeoDB(CITY, "city")
    with pytest.raises(pa.PvError):
        db.lookup_ids(b"\x01\x02\x03", 4)
    lib = pa.load_library()
    assert lib.pv_geodb_entry(db.ptr, len(db.entries), None, None, None) == -1
    assert db.lookup_ids(b"", 4).size == 0


# ---------------------------------------------------------------- sanitizer run
@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_reader_under_address_and_undefined_sanitizers(tmp_path, cases):
    """pv_geodb.cpp and a stand-alone driver built with -fsanitize=address,undefined, run over the
    fixtures, the synthetic trees and 300 seeded byte mutations of each file: exit 0, no report."""
    exe = str(tmp_path / "geodb_asan")
    # (the runtimes linked statically: the binary does not depend on the order libraries load in)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-o", exe,
                           os.path.join(ROOT, "tests", "native", "geodb_asan_main.cpp"),
                           os.path.join(ROOT, "pktvisor_amd", "csrc", "pv_geodb.cpp")])
    files = [CITY, ISP]
    for name in ("v6_rs28", "v6_early_leaf", "city_shared_id"):
        p = tmp_path / (name + ".mmdb")
        p.write_bytes(cases[name][0])
        files.append(str(p))
    r = subprocess.run([exe, "300"] + files, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stderr == "" and r.stdout.startswith("opened ")
