"""CPU differential fuzz of the L2-L4 frame walk: the product's parse_record (pv_parse.h, compiled
for the host by tests/native) against the oracle's parse_packet + set_direction, row by row, over
a seeded corpus built from layers (tests/parse_corpus.py). Every handler stands on this walk."""
import ctypes
import os
import random
import shutil
import socket
import struct
import subprocess

import numpy as np
import pytest

from tests import parse_corpus as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE_DIR = os.path.join(ROOT, "tests", "native")
NATIVE = os.path.join(NATIVE_DIR, "libpvparse_host.so")
COLS = ("l3", "l4", "has4", "has6", "syn", "dir", "v4", "v6", "l4off", "l4len")
U32P = ctypes.POINTER(ctypes.c_uint32)


def split_spec(spec):
    """host spec -> ([(s_addr, cidr)], [(16 bytes, cidr)]), as the product's host code reads it"""
    v4, v6 = [], []
    for host in filter(None, spec.split(",")):
        ipstr, cidr = host.split("/")
        if ":" in ipstr:
            v6.append((socket.inet_pton(socket.AF_INET6, ipstr), int(cidr)))
        else:
            v4.append((struct.unpack("<I", socket.inet_aton(ipstr))[0], int(cidr)))
    return v4, v6


@pytest.fixture(scope="module")
def harness():
    subprocess.check_call(["make", "-s", "-C", NATIVE_DIR])
    h = ctypes.CDLL(NATIVE)
    h.h_parse_records.argtypes = [ctypes.c_char_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, U32P,
                                  U32P, ctypes.c_uint32, ctypes.c_char_p, U32P, ctypes.c_void_p, ctypes.c_uint64]
    h.h_parse_records.restype = ctypes.c_uint64
    return h


def product_rows(h, blob, n, linktype, spec, ts_nano=0):
    v4, v6 = split_spec(spec)
    a4 = (ctypes.c_uint32 * max(1, len(v4)))(*[a for a, _ in v4])
    c4 = (ctypes.c_uint32 * max(1, len(v4)))(*[c for _, c in v4])
    a6 = b"".join(a for a, _ in v6)
    c6 = (ctypes.c_uint32 * max(1, len(v6)))(*[c for _, c in v6])
    rows = np.full((n, len(COLS)), -99, dtype=np.int64)
    got = h.h_parse_records(blob + bytes(16), len(blob), linktype, ts_nano, len(v4), a4, c4, len(v6), a6, c6,
                            rows.ctypes.data, n)
    assert got == n
    return rows


def oracle_rows(oracle, blob, n, linktype, spec):
    lib = oracle.lib
    lib.pvo_parse_packets.argtypes = [ctypes.c_char_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_char_p, ctypes.c_void_p,
                                      ctypes.c_uint64]
    lib.pvo_parse_packets.restype = ctypes.c_int64
    rows = np.full((n, len(COLS)), -98, dtype=np.int64)
    got = lib.pvo_parse_packets(blob, len(blob), linktype, spec.encode(), rows.ctypes.data, n)
    assert got == n
    return rows


# ---------------------------------------------------------------- corpus
def build_corpus():
    """[(family, linktype, host_spec, [records])], seeded"""
    rng = random.Random(20240607)
    groups = []
    specs = [pc.DEFAULT_SPEC, pc.FIVE_V4_SPEC, "192.168.1.7/32,0.0.0.0/0", "2001:db8::1/7"]
    for fam in ("l2", "ipv4", "ipv6", "tunnel", "l4"):
        for spec in specs:
            groups.append((fam, 1, spec, [pc.record(f) for f in pc.frames_of(rng, fam, 5000)]))
    for spec in specs[:2]:
        groups.append(("sll", 113, spec, [pc.record(f) for f in pc.frames_of(rng, "mixed", 5000, linktype=113)]))
    for lt in pc.RAW_LINKTYPES:
        groups.append(("raw", lt, specs[lt % 2], [pc.record(f) for f in pc.frames_of(rng, "mixed", 2000, linktype=lt)]))
    # direction: the same frames under every host spec
    for lt in (1, 101):
        frames = pc.frames_of(rng, "mixed", 600, linktype=lt) + pc.frames_of(rng, "l2" if lt == 1 else "l4", 200, linktype=lt)
        recs = [pc.record(f) for f in frames]
        for spec in pc.HOST_SPECS:
            groups.append(("dir", lt, spec, recs))
    # truncation: every caplen from 0 to the frame's length, for a few hundred base frames
    for lt, n in ((1, 400), (113, 90), (101, 90)):
        base = []
        for fam in ("l2", "ipv4", "ipv6", "tunnel", "l4") if lt == 1 else ("ipv4", "ipv6", "tunnel"):
            base += pc.frames_of(rng, fam, n // (5 if lt == 1 else 3), linktype=lt, maxlen=260)
        # half of them with a trailer behind the IP packet (padding), so the L4 layer stays whole
        # over a range of captured lengths
        base = [f + rng.randbytes(rng.randrange(8, 72)) if rng.random() < 0.5 else f for f in base]
        recs = [pc.record(f, cap) for f in base for cap in range(len(f) + 1)]
        groups.append(("trunc", lt, pc.DEFAULT_SPEC, recs))
    return groups


@pytest.fixture(scope="module")
def corpus():
    return build_corpus()


@pytest.fixture(scope="module")
def oracle_table(oracle, corpus):
    """the oracle's rows of every group, computed once"""
    return [oracle_rows(oracle, b"".join(recs), len(recs), lt, spec) for _, lt, spec, recs in corpus]


def test_corpus_coverage(corpus, oracle_table):
    """a condition on the inputs, from the oracle's rows alone: every family has frames with and
    without an L4 layer, and every value of dir, l4 and l3 occurs"""
    per = {}
    for (fam, _, _, _), rows in zip(corpus, oracle_table):
        a = per.setdefault(fam, [0, 0])
        a[0] += int((rows[:, 1] != 0).sum())
        a[1] += len(rows)
    for fam, (with_l4, n) in per.items():
        print(f"{fam}: {n} records, {with_l4 / n:.1%} with an L4 layer")
        assert 0.05 <= with_l4 / n <= 0.95, (fam, with_l4, n)
    allrows = np.concatenate(oracle_table)
    assert set(np.unique(allrows[:, 5])) == {0, 1, 2}
    assert set(np.unique(allrows[:, 1])) == {0, 6, 17}
    assert set(np.unique(allrows[:, 0])) == {0, 4, 6}
    assert set(np.unique(allrows[:, 4])) == {0, 1}
    assert len(allrows) > 50000


def test_parse_record_matches_oracle(harness, corpus, oracle_table):
    bad = 0
    for (fam, lt, spec, recs), want in zip(corpus, oracle_table):
        got = product_rows(harness, b"".join(recs), len(recs), lt, spec)
        for i in np.nonzero((got != want).any(axis=1))[0][:5]:
            print(f"{fam} linktype {lt} spec '{spec}' record {i}: {recs[i].hex()}")
            print("  oracle ", dict(zip(COLS, want[i].tolist())))
            print("  product", dict(zip(COLS, got[i].tolist())))
        bad += int((got != want).any(axis=1).sum())
    assert bad == 0, f"{bad} records differ"


def test_timestamp_modes_do_not_change_the_walk(harness, corpus):
    """ts_nano only scales the fraction: the rows are the same"""
    fam, lt, spec, recs = corpus[0]
    blob = b"".join(recs)
    assert (product_rows(harness, blob, len(recs), lt, spec, 0) == product_rows(harness, blob, len(recs), lt, spec, 1)).all()


# ---------------------------------------------------------------- the frames that separated the two walks
SPEC = "10.0.0.0/8,2001:db8::/32"  # 10.1.2.3 -> 8.8.8.8 and 2001:db8::1 -> 2101:db8::1: from the host


def row(**kw):
    r = dict(l3=0, l4=0, has4=0, has6=0, syn=0, dir=2, v4=-1, v6=-1, l4off=-1, l4len=0)
    r.update(kw)
    return [r[c] for c in COLS]


@pytest.mark.parametrize("n", [6, 7, 8, 9, 10, 11])
def test_extension_header_chain(harness, oracle, n):
    """Eth + IPv6 + n 8-byte destination-option headers + TCP: the walk is bounded by the length
    alone, so the TCP layer is found behind 9 and more headers as behind 8"""
    f = pc.ext_chain_frame(n)
    assert len(f) == 79 + 8 * n  # 143 bytes at 8 headers, 151 at 9
    want = row(l3=6, l4=6, has6=1, dir=1, v6=14, l4off=54 + 8 * n, l4len=25)
    rec = pc.record(f)
    assert oracle_rows(oracle, rec, 1, 1, SPEC)[0].tolist() == want
    assert product_rows(harness, rec, 1, 1, SPEC)[0].tolist() == want


@pytest.mark.parametrize("k", [2, 3, 4, 5, 6, 7, 8])
def test_nested_ipv4_headers(harness, oracle, k):
    """Eth + k IPv4 headers + TCP: five IP headers are walked, a sixth is not"""
    f = pc.nested_v4_frame(k)
    assert len(f) == 39 + 20 * k  # 119 bytes at 4 headers, 139 at 5, 159 at 6
    if k <= 5:
        want = row(l3=4, l4=6, has4=1, dir=1, v4=14, l4off=14 + 20 * k, l4len=25)
    else:
        want = row(l3=4, has4=1, dir=1, v4=14)
    rec = pc.record(f)
    assert oracle_rows(oracle, rec, 1, 1, SPEC)[0].tolist() == want
    assert product_rows(harness, rec, 1, 1, SPEC)[0].tolist() == want


@pytest.mark.parametrize("tags", [7, 8, 9])
def test_vlan_tag_bound(harness, oracle, tags):
    """eight VLAN tags are walked in both, a ninth ends the walk"""
    rng = random.Random(3)
    f = pc.eth(rng, pc.v4hdr(rng, pc.tcp25(True), 6, src="8.8.8.8", dst="10.1.2.3"), 0x0800, ([0x8100, 0x88A8] * 5)[:tags])
    off = 14 + 4 * tags
    want = row(l3=4, l4=6, has4=1, syn=1, dir=0, v4=off, l4off=off + 20, l4len=25) if tags <= 8 else row()
    rec = pc.record(f)
    assert oracle_rows(oracle, rec, 1, 1, SPEC)[0].tolist() == want
    assert product_rows(harness, rec, 1, 1, SPEC)[0].tolist() == want


# ---------------------------------------------------------------- sanitizer run
def test_parse_record_under_address_and_undefined_sanitizers(tmp_path, corpus):
    """the corpus through a stand-alone program built with -fsanitize=address,undefined, every
    record parsed from a heap copy of exactly 16 + caplen bytes: exit 0, no report"""
    cxx = shutil.which("g++")
    assert cxx
    exe = str(tmp_path / "parse_asan")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-DPV_PARSE_BOUNDED", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-o", exe,
                           os.path.join(NATIVE_DIR, "parse_asan_main.cpp"), os.path.join(NATIVE_DIR, "parse_harness.cpp")])
    path = str(tmp_path / "corpus.bin")
    total = 0
    with open(path, "wb") as f:
        for _, lt, spec, recs in corpus:
            v4, v6 = split_spec(spec)
            f.write(struct.pack("<II", lt, len(v4)) + b"".join(struct.pack("<II", a, c) for a, c in v4))
            f.write(struct.pack("<I", len(v6)) + b"".join(a + struct.pack("<I", c) for a, c in v6))
            blob = b"".join(recs)
            f.write(struct.pack("<Q", len(blob)) + blob)
            total += len(recs)
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.startswith(f"{total} records in {len(corpus)} groups"), r.stdout
