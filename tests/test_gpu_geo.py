"""The device walker of a compiled GeoIP / ASN tree (pv_geo_walk through pv_geodb_lookup_device)
equals the host walk (pv_geodb_lookup) for both fixture databases and the synthetic trees of
tests/geo_cases.py, at batch sizes around a wave and past one launch's first grid pass."""
import os

import numpy as np
import pytest

import pktvisor_amd as pa
from tests import geo_cases

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CITY = os.path.join(GOLD, "GeoIP2-City-Test.mmdb")
ISP = os.path.join(GOLD, "GeoIP2-ISP-Test.mmdb")
BATCHES = (1, 63, 64, 65, 4097)


@pytest.fixture(scope="module")
def handlers():
    h = pa.PvHandlers(host_spec="192.168.0.0/24", num_periods=1, max_records=1 << 12)
    yield h
    h.close()


def _batches(data, alen, seed):
    """per batch size: packed addresses, leaf range ends first (they exercise every depth), then random"""
    probes = geo_cases.probe_addresses(data, 0, seed)[alen]
    rng = np.random.default_rng(seed)
    for n in BATCHES:
        rnd = rng.integers(0, 256, size=(n, alen), dtype=np.uint8)
        rng.shuffle(probes)
        take = probes[: n - n // 4]
        if take:
            rnd[: len(take)] = np.frombuffer(b"".join(take), dtype=np.uint8).reshape(-1, alen)
        yield n, rnd


def _check(h, db, kind, data, seed):
    for alen in (4, 16):
        for n, addrs in _batches(data, alen, seed + alen):
            want = db.lookup_ids(addrs, alen)
            got = h.geo_lookup_device(kind, addrs, alen)
            assert got.shape == (n,) and np.array_equal(got, want), (kind, alen, n)


def test_fixture_databases(handlers):
    city, isp = pa.GeoDB(CITY, "city"), pa.GeoDB(ISP, "asn")
    handlers.set_geodb(city, isp)
    _check(handlers, city, "city", open(CITY, "rb").read(), 1)
    _check(handlers, isp, "asn", open(ISP, "rb").read(), 2)
    # the known answers of the reference's test_geoip.cpp through the device
    import ipaddress
    for db, kind, ip, name in ((city, "city", "89.160.20.112", "EU/Sweden/E/Linköping"), (city, "city", "2a02:dac0::", "EU/Russia"),
                               (isp, "asn", "1.128.0.0", "1221/Telstra Pty Ltd"), (isp, "asn", "12.81.92.0", "7018"),
                               (isp, "asn", "8.8.8.8", ""), (isp, "asn", "6.6.6.6", "Unknown")):
        raw = ipaddress.ip_address(ip).packed
        assert db.entries[int(handlers.geo_lookup_device(kind, raw, len(raw))[0])][0] == name


def test_attach_by_path_and_one_database_only():
    h = pa.PvHandlers(host_spec="192.168.0.0/24", num_periods=1, max_records=1 << 12, geo_city_db=CITY)
    try:
        db = pa.GeoDB(CITY, "city")
        addrs = np.random.default_rng(5).integers(0, 256, size=(257, 4), dtype=np.uint8)
        assert np.array_equal(h.geo_lookup_device("city", addrs, 4), db.lookup_ids(addrs, 4))
        with pytest.raises(pa.PvError, match="no ASN database attached"):
            h.geo_lookup_device("asn", addrs, 4)
        with pytest.raises(pa.PvError, match="opened as the other kind"):
            h.set_geodb(None, db)
    finally:
        h.close()


def test_synthetic_trees(handlers):
    for seed, (name, (data, kind)) in enumerate(sorted(geo_cases.build().items())):
        db = pa.GeoDB(data, kind)
        handlers.set_geodb(db if kind == "city" else None, db if kind == "asn" else None)
        _check(handlers, db, kind, data, 100 + seed)
