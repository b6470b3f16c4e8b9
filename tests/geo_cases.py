"""Synthetic MMDB trees shared by the CPU and GPU GeoIP tests (built with tests/mmdb_ref.py's writer):
name -> (file bytes, kind). Every record size and ip_version, prefixes /1 /8 /24 /32 (/33 and
/128 for IPv6), a v6 tree without an IPv4 subtree, one whose ::/96 path ends in a leaf early, a
one-node tree with both records empty, and two data records that render one City triple."""
import ipaddress
import random

from tests import mmdb_ref as R


def asn(n, org=None):
    d = {"autonomous_system_number": R.U32(n)}
    if org is not None:
        d["autonomous_system_organization"] = org
    return d


def city(cont, country, lat=None, lon=None, extra=None):
    d = {"continent": {"code": cont}, "country": {"iso_code": country[:2].upper(), "names": {"en": country}}}
    if lat is not None:
        d["location"] = {"latitude": lat, "longitude": lon}
    d.update(extra or {})
    return d


V4 = [("128.0.0.0/1", asn(1, "half")), ("10.0.0.0/8", asn(8, "eight")), ("11.22.33.0/24", asn(24)),
      ("12.1.2.3/32", asn(32, "host"))]
V6 = [("2001:db8:8000::/33", asn(33, "v6 33")), ("2001:db8::1/128", asn(128, "v6 host")),
      ("2001:db8:4000::/34", {"autonomous_system_number": "64500", "autonomous_system_organization": "text number"}),
      ("fe80::/10", {"autonomous_system_number": R.U16(7), "x": [1, {"y": True}]}),
      ("fc00::/7", {"autonomous_system_number": R.I32(-5)}),
      ("ff00::/8", {"autonomous_system_number": R.U64(1 << 40), "autonomous_system_organization": "big"})]


def build():
    cases = {}
    for rs in (24, 28, 32):
        cases[f"v4_rs{rs}"] = (R.write_mmdb(V4, rs, 4), "asn")
        cases[f"v6_rs{rs}"] = (R.write_mmdb(V4 + V6, rs, 6), "asn")
    cases["v6_no_v4_subtree"] = (R.write_mmdb(V6, 24, 6), "asn")
    cases["v6_early_leaf"] = (R.write_mmdb([("::/8", asn(96, "early"))] + V6, 28, 6), "asn")
    cases["one_node_empty"] = (R.write_mmdb([], 24, 6), "asn")
    same = city("EU", "Sweden", 58.4167, 15.6167)
    cases["city_shared_id"] = (R.write_mmdb(
        [("10.0.0.0/8", same), ("20.0.0.0/8", dict(same, extra_field="other record")),
         ("30.0.0.0/8", city("EU", "Sweden", 58.4167, 15.5)), ("40.0.0.0/8", city("NA", "Canada")),
         ("50.0.0.0/8", {"country": {"iso_code": "ZZ"}, "subdivisions": [{"iso_code": "Q"}],
                         "city": {"names": {"en": "Town", "de": "Stadt"}}, "location": {"latitude": 1, "longitude": 2.5}})],
        32, 4), "city")
    return cases


def probe_addresses(data: bytes, n_random: int, seed: int):
    """{4: [...], 16: [...]} packed addresses: both ends of every leaf's range and random ones"""
    rd = R.Reader(data)
    rng = random.Random(seed)
    out = {4: [], 16: []}
    width = 32 if rd.ip_version == 4 else 128
    for bits, depth, _ in rd.leaves():
        lo = bits << (width - depth)
        hi = lo | ((1 << (width - depth)) - 1)
        for v in (lo, hi):
            if width == 32:
                out[4].append(v.to_bytes(4, "big"))
            else:
                out[16].append(v.to_bytes(16, "big"))
                if v >> 32 == 0:
                    out[4].append(v.to_bytes(16, "big")[12:])
    for _ in range(n_random):
        out[4].append(rng.getrandbits(32).to_bytes(4, "big"))
        out[16].append(rng.getrandbits(128).to_bytes(16, "big"))
    for text in ("0.0.0.0", "255.255.255.255", "10.255.255.255", "11.22.33.255", "11.22.34.0", "12.1.2.3", "12.1.2.2"):
        out[4].append(ipaddress.ip_address(text).packed)
    for text in ("::", "ffff:ffff:ffff:ffff:ffff:ffff:ffff:ffff", "2001:db8::1", "2001:db8::2", "2001:db8:8000::",
                 "2001:db8:7fff:ffff::", "::ffff:10.0.0.1", "::10.0.0.1"):
        out[16].append(ipaddress.ip_address(text).packed)
    return out
