#!/usr/bin/env python3
"""Write a synthetic MaxMind DB of a chosen size, for timing the GeoIP walker on a tree that does
not fit in L2 (the two test databases under tests/golden are a few KiB of nodes).

An ip_version 4 tree, complete to `--depth` levels (2^depth - 1 nodes, 32-bit records, so
8 bytes a node: depth 22 is 4.2 M nodes, 32 MiB); the records of the last level point at
`--records` distinct ASN data records picked at random (seeded). Every IPv4 address resolves after
exactly `depth` node loads, the worst case of a real database's IPv4 part.

    python tools/gen_mmdb.py --depth 22 --records 4096 -o big.mmdb
"""
import argparse
import struct

import numpy as np

MARKER = b"\xab\xcd\xefMaxMind.com"


def _str(s):
    b = s.encode()
    assert len(b) < 29 + 256
    if len(b) < 29:
        return bytes([(2 << 5) | len(b)]) + b
    return bytes([(2 << 5) | 29, len(b) - 29]) + b


def _u32(v):
    return bytes([(6 << 5) | 4]) + struct.pack(">I", v)


def _u16(v):
    return bytes([(5 << 5) | 2]) + struct.pack(">H", v)


def _map(pairs):
    assert len(pairs) < 29
    return bytes([(7 << 5) | len(pairs)]) + b"".join(_str(k) + v for k, v in pairs)


def build(depth: int, records: int, seed: int) -> bytes:
    assert 1 <= depth <= 26 and records >= 1
    nc = (1 << depth) - 1
    data, offs = b"", []
    for i in range(records):
        offs.append(len(data))
        data += _map([("autonomous_system_number", _u32(64512 + i)),
                      ("autonomous_system_organization", _str(f"Synthetic Org {i}"))])
    offs = np.asarray(offs, dtype=np.uint64)
    idx = np.arange(nc, dtype=np.uint64)
    tree = np.empty((nc, 2), dtype=np.uint64)
    tree[:, 0] = 2 * idx + 1
    tree[:, 1] = 2 * idx + 2
    first_last = (1 << (depth - 1)) - 1  # the last level: both records are data pointers
    rng = np.random.default_rng(seed)
    pick = rng.integers(0, records, size=(nc - first_last, 2))
    tree[first_last:] = nc + 16 + offs[pick]
    assert int(tree.max()) < 1 << 32
    meta = _map([("node_count", _u32(nc)), ("record_size", _u16(32)), ("ip_version", _u16(4)),
                 ("database_type", _str("Synthetic-ASN")), ("binary_format_major_version", _u16(2)),
                 ("binary_format_minor_version", _u16(0))])
    return tree.astype(">u4").tobytes() + b"\0" * 16 + data + MARKER + meta


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--depth", type=int, default=22)
    ap.add_argument("--records", type=int, default=4096)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("-o", "--output", required=True)
    a = ap.parse_args()
    blob = build(a.depth, a.records, a.seed)
    with open(a.output, "wb") as f:
        f.write(blob)
    print(f"{a.output}: {(1 << a.depth) - 1} nodes, {a.records} data records, {len(blob)} bytes")


if __name__ == "__main__":
    main()
