"""Seeded corpus of DNS messages placed so that they cross the edges of the device decode's LDS
windows: the DNS pass's 128-byte window per message (a message is decoded from LDS alone when it
ends within byte 124 of the window, else in the range's long pass) and the names kernel's 192-byte
window per record. Shared by tests/test_dns_corpus.py (conditions on the inputs),
tests/test_decoder_fuzz.py (pv_parse.h on the CPU against the oracle) and
tests/test_gpu_dns_decode.py (the same records through the DNS pass and the names kernels).

Every generator yields Items: (frame, msg_off, msg) plus how the frame is to be captured. assemble()
turns a list of Items into classic-pcap records and says where each message lies (roff, moff, mlen,
mcap), from the builder's own arithmetic, never from the code under test.

Every name of a batch is distinct (a query and its response share theirs, as do the cuts of one
captured frame in `junk`): its first label carries the family letter and a counter, so one wrong
decode changes the set of names in the top lists."""
import random
import struct
from collections import namedtuple

from tests import parse_corpus as pc

HOST = "10.0.0.0/8,2001:db8::/32"
CLIENT4, RESOLVER4 = "10.1.2.3", "8.8.8.8"
CLIENT6, RESOLVER6 = "2001:db8::1", "2101:db8::1"
T0 = 1_700_000_040  # a minute's start: a batch of a few thousand records stays inside one period
WIN, NWIN = 128, 192  # PV_WIN, PV_NWIN (pv_kernels.hip)
LAYERS = ("v4", "vlan", "opt", "v6")

# frame: without trailing pad; steer: the next record's start residue (roff & 15) this frame's pad
# is chosen for; pad: a fixed pad; cap: captured length (None: whole); long: the tile shapes' flag
Item = namedtuple("Item", "frame msg_off msg fam steer pad cap long", defaults=(None, None, None, None))
# one record of an assembled batch (dns: a UDP port-53 payload whose UDP header is captured whole)
Rec = namedtuple("Rec", "roff moff mlen mcap msg fam dns")
Batch = namedtuple("Batch", "name blob recs")


def fits(moff, mlen, mcap):
    """the DNS pass's rule for decoding a message from its LDS window alone (pv_dns_kernel)"""
    return (moff & 15) + max(mlen, mcap) <= WIN - 4


def enc(labels):
    return b"".join(bytes([len(x)]) + x for x in labels) + b"\0"


def header(txid, flags=0x0100, qd=1, an=0, ns=0, ar=0):
    return struct.pack(">HHHHHH", txid & 0xFFFF, flags, qd, an, ns, ar)


def rr(name, rtype, rdata, rdlen=None, ttl=60):
    return name + struct.pack(">HHIH", rtype, 1, ttl, len(rdata) if rdlen is None else rdlen) + rdata


PLAIN = b"abcdefghijklmnopqrstuvwxyz0123456789-_"
KINDS = ("plain", "upper", "nul", "dot", "high")
TAILS = ([b"com"], [b"co", b"uk"], [], [b"k12", b"ak", b"us"], [b"ORG"], [])
SUFFIXES = [".co.uk", "ak.us", ".t"]  # only_qname_suffix: three suffixes that occur in every family

# The GPU cases: the handler's config and the oracle's keys for the same (tests/test_gpu_dns_decode.py
# runs both; tests/test_dns_corpus.py checks on the oracle that no top list is cut)
V1 = {"enable": ["all"]}
V2_ALL = ["cardinality", "counters", "quantiles", "top_ecs", "top_qtypes", "top_rcodes", "top_size", "top_qnames", "top_ports",
          "xact_times"]
CASES = {
    "v1": (dict(dns_config=V1), dict(dns_groups=0x1ff)),
    "v1_psl": (dict(dns_config=dict(V1, public_suffix_list=True)), dict(dns_groups=0x1ff, public_suffix_list=1)),
    "v1_suffix": (dict(dns_config=dict(V1, only_qname_suffix=SUFFIXES)), dict(dns_groups=0x1ff, only_qname_suffix=",".join(SUFFIXES))),
    "v1_dnssec": (dict(dns_config=dict(V1, only_dnssec_response=True)), dict(dns_groups=0x1ff, only_dnssec_response=1)),
    "v1_qtype": (dict(dns_config=dict(V1, only_qtype=["A", "AAAA"])), dict(dns_groups=0x1ff, only_qtype="1,28")),
    "v2": (dict(dns2_config={"enable": V2_ALL}), dict(dns2_groups=0x3ff)),
    "v2_qtype": (dict(dns2_config={"enable": V2_ALL, "only_qtype": ["A", "AAAA"]}), dict(dns2_groups=0x3ff, only_qtype="1,28")),
}


def topn_for(batch):
    """topn_count above the batch's record count, so every top list comes back whole"""
    return 1024 if len(batch.recs) < 1000 else 8192


class Gen:
    """one batch's generator state: the random stream and the name counter"""

    def __init__(self, seed):
        self.rng = random.Random(seed)
        self.k = 0

    def first(self, fam):
        """the counter label: family letter + five digits"""
        self.k += 1
        return b"%s%05d" % (fam[:1].encode(), self.k)

    def text(self, n, kind="plain"):
        rng = self.rng
        b = bytearray(rng.choice(PLAIN) for _ in range(n))
        if not n:
            return bytes(b)
        if kind == "upper":
            for i in range(n):
                if rng.random() < 0.5:
                    b[i] = ord(chr(b[i]).upper())
        elif kind == "nul":
            b[rng.randrange(n)] = 0
        elif kind == "dot":
            b[rng.randrange(n)] = ord(".")
        elif kind == "high":
            for i in range(n):
                if rng.random() < 0.3:
                    b[i] = rng.randrange(0x80, 0x100)
        return bytes(b)

    def labels(self, fam, total, dots=None, kind="plain", greedy=False):
        """labels of a name whose decoded text has `total` bytes with `dots` inner dots (moved into the
        feasible range), the counter label first; greedy: 63-byte labels first. Where there is room
        the name ends in one of TAILS (suffixes the public suffix list and the suffix filter know)."""
        tail = TAILS[self.k % len(TAILS)]
        tl = sum(len(x) + 1 for x in tail)
        if tail and total - tl >= 12 and (dots is None or dots >= len(tail)):
            return self.plain_labels(fam, total - tl, None if dots is None else dots - len(tail), kind, greedy) + tail
        return self.plain_labels(fam, total, dots, kind, greedy)

    def plain_labels(self, fam, total, dots, kind, greedy):
        rng = self.rng
        first = self.first(fam)
        if total <= len(first):
            return [first[:max(1, total)]]
        if dots is None:
            dots = rng.randrange(1, 6)
        rest = total - len(first)  # bytes behind the first label, dots included
        if dots == 0:
            return [first + self.text(rest, kind)]
        dots = max(dots, -(-rest // 64))
        dots = min(dots, rest // 2)
        if dots == 0:
            return [first + self.text(rest, kind)]
        room = rest - dots  # label bytes for `dots` labels, each 1..63
        lens = [1] * dots
        room -= dots
        order = list(range(dots))
        if not greedy:
            rng.shuffle(order)
        for i in order:
            take = min(62, room) if greedy else min(62, room, rng.randrange(0, 63))
            lens[i] += take
            room -= take
        i = 0
        while room > 0:
            take = min(63 - lens[i], room)
            lens[i] += take
            room -= take
            i += 1
        return [first] + [self.text(n, kind) for n in lens]

    # ------------------------------------------------------------ placement
    def place(self, msg, fam, layer="v4", response=False, cport=None, **kw):
        """the message behind Ethernet / IP / UDP (port 53), without trailing pad; a response travels
        the other way, so with its query's cport and transaction id the two make a transaction"""
        rng = self.rng
        cport = 1024 + self.k % 60000 if cport is None else cport
        sp, dp = (53, cport) if response else (cport, 53)
        udp = struct.pack(">HHHH", sp, dp, 8 + len(msg), 0) + msg
        a4, b4 = (RESOLVER4, CLIENT4) if response else (CLIENT4, RESOLVER4)
        a6, b6 = (RESOLVER6, CLIENT6) if response else (CLIENT6, RESOLVER6)
        if layer == "v6":
            f = pc.eth(rng, pc.v6hdr(rng, udp, 17, src=a6, dst=b6), 0x86DD)
        elif layer == "vlan":
            f = pc.eth(rng, pc.v4hdr(rng, udp, 17, src=a4, dst=b4), 0x0800, [0x8100])
        elif layer == "opt":
            f = pc.eth(rng, pc.v4hdr(rng, udp, 17, ihl=rng.randrange(6, 16), src=a4, dst=b4), 0x0800)
        else:
            f = pc.eth(rng, pc.v4hdr(rng, udp, 17, src=a4, dst=b4), 0x0800)
        return Item(f, len(f) - len(msg), msg, fam, **kw)

    def pair(self, msg, fam, layer="v4"):
        """a query and the same message sent back with the QR and RA bits set: one transaction, and the
        response is as long and ends where the query does"""
        cport = 1024 + self.k % 60000
        back = msg[:2] + bytes([msg[2] | 0x80, 0x80]) + msg[4:]
        return [self.place(msg, fam, layer=layer, cport=cport), self.place(back, fam, layer=layer, response=True, cport=cport)]

    def query(self, labels, qtype=1, txid=None, flags=0x0100, tail=b"", an=0, ns=0, ar=0):
        txid = self.k if txid is None else txid
        return header(txid, flags, 1, an, ns, ar) + enc(labels) + struct.pack(">HH", qtype, 1) + tail

    def short(self, fam="s", **kw):
        """a query of about 30 bytes: it fits whatever its place"""
        return self.place(self.query([self.first(fam), b"t"]), fam, **kw)

    def of_len(self, fam, mlen, **kw):
        """a valid query of exactly mlen bytes (at least 26), the name padded to hit the length"""
        return self.place(self.query(self.labels(fam, mlen - 18)), fam, **kw)


V4_MSG_OFF = 42  # Ethernet + IPv4 + UDP


# ---------------------------------------------------------------- families
def edge_len(g):
    """valid queries whose length sweeps 90..170: they cross the `fits` edge at 124 - (moff & 15);
    then, for every residue of moff & 15, messages that end exactly at chosen bytes around 124"""
    out = []
    for mlen in range(90, 171):
        for layer in ("v4", "v6" if mlen % 2 else "v4"):
            out += g.pair(g.query(g.labels("e", mlen - 18)), "e", layer)
    for m in range(16):
        for end in (116, 120, 121, 124, 125, 128, 129, 140):
            # (roff + 16 + 42) & 15 == m; no pad of its own: mcap == mlen == end - m
            out.append(g.short("f", steer=(m - 16 - V4_MSG_OFF) & 15))
            out.append(g.of_len("e", end - m, pad=0))
    return out


def edge_name(g):
    """queries and responses whose decoded name sweeps 90..255 bytes: the 63-byte label and 255-byte
    name limits, 0..12 inner dots, upper case, NUL, '.' inside a label and bytes >= 0x80, behind
    Ethernet/IPv4, a VLAN tag, IPv4 options and IPv6; then, for every residue of roff & 15, names
    that end exactly at chosen bytes around 192 of the record's window"""
    out = []
    for v, total in enumerate(range(90, 256)):
        labels = g.labels("n", total, dots=v % 13, kind=KINDS[v % 5], greedy=v % 7 == 0)
        txid, cport = g.k, 1024 + g.k % 60000
        for resp in (False, True):  # a query and its response: one transaction
            msg = g.query(labels, qtype=(1, 28, 15, 16)[v % 4], txid=txid, flags=0x8180 if resp else 0x0100)
            out.append(g.place(msg, "n", layer=LAYERS[v % 4], response=resp, cport=cport))
    for r in range(16):
        for end in (180, 184, 185, 192, 193, 200, 201, 215):
            # name end from the record's aligned start: r + 16 + 42 + 12 + encoded length
            out.append(g.short("f", steer=r))
            out.append(g.place(g.query(g.labels("n", end - r - 16 - V4_MSG_OFF - 12 - 2, kind=KINDS[(r + end) % 5])), "n", pad=0))
    return out


def ptr(g):
    """question names with compression pointers: forward and backward targets, targets beyond byte
    124, inside the header, at or beyond the message length, self-pointers, chains deeper than 20,
    a pointer after labels; and responses whose answers use 0xC00C"""
    rng = g.rng
    out = []

    def p(target):
        return bytes([0xC0 | ((target >> 8) & 0x3F), target & 0xFF])

    for i in range(210):
        kind = i % 14
        first = g.first("p")
        lab = bytes([len(first)]) + first
        q = struct.pack(">HH", 1, 1)
        hdr = header(g.k)
        if kind in (0, 1):  # a pointer after labels, forward to labels behind the question (short and long gaps)
            gap = rng.randrange(0, 20) if kind == 0 else rng.randrange(60, 140)
            t = 12 + len(lab) + 2 + 4 + gap
            msg = hdr + lab + p(t) + q + rng.randbytes(gap) + enc([b"fwd", g.text(rng.randrange(1, 30))])
        elif kind == 2:  # backward into the first label's own bytes, which read as labels there
            inner = b"\x02bk\x00"
            first2 = first + inner
            msg = hdr + bytes([len(first2)]) + first2 + p(12 + 1 + len(first)) + q
        elif kind == 3:  # inside the header
            msg = hdr + lab + p(rng.randrange(0, 12)) + q
        elif kind == 4:  # at or beyond the message length (the message itself short or long)
            body = lab + b"\xc0\x00" + q + rng.randbytes(rng.choice((0, 0, 90)))
            n = 12 + len(body)
            t = rng.choice((n, n + 1, 124, 125, 128, 200, 0x3FFF, n - 1))
            msg = hdr + lab + p(t) + body[len(lab) + 2:]
        elif kind == 5:  # self-pointer, after the label and bare at offset 12
            msg = hdr + lab + p(12 + len(lab)) + q if i % 28 < 14 else hdr + p(12) + q
        elif kind in (6, 7, 8):  # a chain of 1..25 hops, each a one-byte label and a pointer on
            hops = rng.choice((1, 2, 5, 18, 19, 20, 21, 25)) if kind < 8 else rng.randrange(1, 26)
            base = 12 + len(lab) + 2 + 4
            body = b""
            for hop in range(hops):
                nxt = base + 4 * (hop + 1)
                body += b"\x01" + bytes([97 + hop % 26]) + p(nxt)
            body += enc([b"end"])
            msg = hdr + lab + p(base) + q + body
        elif kind == 9:  # the name opens with a pointer: the labels (counter first) lie behind the question
            gap = rng.choice((0, 3, 70, 100))
            t = 12 + 2 + 4 + gap
            msg = hdr + p(t) + q + rng.randbytes(gap) + enc([first, b"tail", g.text(rng.randrange(1, 40))])
        elif kind == 10:  # a pointer to a pointer to labels, the last hop beyond byte 124
            gap = rng.randrange(90, 130)
            a = 12 + len(lab) + 2 + 4
            msg = hdr + lab + p(a) + q + p(a + 2 + gap) + rng.randbytes(gap) + enc([b"far", b"x"])
        elif kind == 11:  # a pointer in the middle of a long name, backward onto its own second label (a loop)
            l2 = g.text(rng.randrange(1, 63))
            msg = hdr + lab + bytes([len(l2)]) + l2 + p(12 + len(lab)) + q
        else:  # responses whose answers use 0xC00C, the name long or short
            labels = [first] + [g.text(rng.randrange(1, 50)) for _ in range(rng.randrange(1, 4))]
            n_an = rng.randrange(1, 4)
            ans = b"".join(rr(b"\xc0\x0c", 1, rng.randbytes(4)) for _ in range(n_an))
            msg = header(g.k, 0x8180, 1, n_an) + enc(labels) + q + ans
            cport = 1024 + g.k % 60000
            out.append(g.place(g.query(labels), "p", layer=LAYERS[i % 4], cport=cport))
            out.append(g.place(msg, "p", layer=LAYERS[i % 4], response=True, cport=cport))
            continue
        out += g.pair(msg, "p", LAYERS[(i // 14) % 4])
    return out


def ecs_option(code, family, alen, rng, optlen=None):
    body = struct.pack(">HBB", family, 8 * min(alen, 16), 0) + rng.randbytes(alen)
    return struct.pack(">HH", code, len(body) if optlen is None else optlen) + body


def ecs(g):
    """queries with 0..3 answer or authority records in front of the OPT record, so its offset
    sweeps across 124: CSUBNET families 0..3, address lengths 0..19, other option codes, dlen 0..12,
    an rdlength that lies, the OPT record as second additional, arcount larger than present"""
    rng = g.rng
    out = []
    for i in range(240):
        labels = [g.first("c"), b"ecs", g.text(rng.randrange(1, 12))]
        n_front = i % 4
        front = b""
        for _ in range(n_front):
            nm = b"\xc0\x0c" if rng.random() < 0.6 else enc([g.text(rng.randrange(1, 9))])
            front += rr(nm, rng.choice((1, 2, 5, 46)), rng.randbytes(rng.choice((0, 4, 4, 16, 31))))
        an = rng.randrange(0, n_front + 1)
        ns = n_front - an
        family = i % 4 if i % 16 < 12 else rng.choice((1, 2))
        alen = (i // 4) % 20
        code = 8 if i % 11 else rng.choice((0, 3, 10, 0x0800))
        data = ecs_option(code, family, alen, rng)
        mode = i % 9
        rdlen = None
        ar = 1
        extra = b""
        if mode == 1:  # data cut to 0..12 bytes, rdlength to match
            data = data[: rng.randrange(0, 13)]
        elif mode == 2:  # rdlength that lies
            rdlen = max(0, len(data) + rng.choice((-5, -1, 1, 2, 9, 40)))
        elif mode == 3:  # the OPT record second
            extra = rr(enc([b"ns1"]), 1, rng.randbytes(4))
        elif mode == 4:  # arcount larger than what is there
            ar = rng.choice((2, 3, 50))
        elif mode == 5:  # data cut, rdlength not
            rdlen = len(data)
            data = data[: rng.randrange(0, len(data) + 1)]
        opt = b"\x00" + struct.pack(">HHIH", 41, 4096, 0, len(data) if rdlen is None else rdlen) + data
        tail = front + extra + opt
        if extra:
            ar += 1
        out += g.pair(g.query(labels, tail=tail, an=an, ns=ns, ar=ar), "c", LAYERS[(i // 5) % 4])
    return out


def rcode(g):
    """queries and their responses with rcode 0, 2, 3 and 5, no answer or a few, and long names: the SRVFAIL, NX,
    REFUSED and NODATA lists take their names from records past the names kernel's window; some
    answers are RRSIG (type 46) for the DNSSEC filter"""
    rng = g.rng
    out = []
    for i in range(200):
        rc = (0, 2, 3, 5)[i % 4]
        total = rng.randrange(100, 251) if i % 5 else rng.randrange(8, 60)
        labels = g.labels("r", total, kind=KINDS[(i // 4) % 5] if i % 3 == 0 else "plain")
        n_an = (0, 0, 1, 3)[(i // 4) % 4]
        ans = b""
        for j in range(n_an):
            t = 46 if (i // 16) % 2 == 0 and j == n_an - 1 else rng.choice((1, 28, 5))
            ans += rr(b"\xc0\x0c", t, rng.randbytes(rng.choice((4, 16, 24))))
        opt = b"\x00" + struct.pack(">HHIH", 41, 4096, 0x8000, 0) if i % 6 == 0 else b""
        qtype, layer = (1, 28, 15, 48)[(i // 2) % 4], LAYERS[(i // 3) % 4]
        txid, cport = g.k, 1024 + g.k % 60000
        # the query in front of its response: one transaction
        out.append(g.place(g.query(labels, qtype=qtype, txid=txid), "r", layer=layer, cport=cport))
        msg = g.query(labels, qtype=qtype, txid=txid, flags=0x8180 | rc, tail=ans + opt, an=n_an, ar=1 if opt else 0)
        out.append(g.place(msg, "r", layer=layer, response=True, cport=cport))
    return out


def junk(g):
    """test_decoder_fuzz.random_message behind UDP port 53, and whole captures cut at every length
    from 0 to the frame's, so that mcap < 12 and mcap < the UDP length occur"""
    import numpy as np

    from tests.test_decoder_fuzz import random_message
    nrng = np.random.default_rng(g.rng.getrandbits(32))
    out = []
    for i in range(220):
        g.k += 1
        out.append(g.place(random_message(nrng), "j", layer=LAYERS[i % 4], response=i % 3 == 0))
    for layer, total in (("v4", 20), ("v4", 75), ("v6", 40)):
        it = g.place(g.query(g.labels("j", total)), "j", layer=layer, pad=g.rng.randrange(16))
        for cap in range(len(it.frame) + it.pad + 1):
            out.append(it._replace(cap=cap))
    return out


FAMILIES = {"edge_len": edge_len, "edge_name": edge_name, "ptr": ptr, "ecs": ecs, "rcode": rcode, "junk": junk}


# ---------------------------------------------------------------- tile shapes
def long_msg(g):
    """a query of 130..160 bytes: at least 125 bytes from its window base wherever it lies"""
    return g.of_len("l", g.rng.randrange(130, 161))._replace(long=True)


def shape(g, name):
    """the DNS pass walks the messages 64 to a tile in record order: [Item] with Item.long set on the
    messages that must go to the long list"""
    short = lambda: g.short()._replace(long=False)  # noqa: E731
    if name.startswith("n"):  # n1, n63, n64, n65, n129: every fifth message long
        return [long_msg(g) if i % 5 == 0 else short() for i in range(int(name[1:]))]
    if name == "all_long":
        return [long_msg(g) for _ in range(64)]
    if name == "one_long_first":
        return [long_msg(g)] + [short() for _ in range(63)]
    if name == "one_long_last":
        return [short() for _ in range(63)] + [long_msg(g)]
    if name == "long_tile":
        return [short() for _ in range(64)] + [long_msg(g) for _ in range(64)] + [short() for _ in range(70)]
    raise KeyError(name)


SHAPES = ("n1", "n63", "n64", "n65", "n129", "all_long", "one_long_first", "one_long_last", "long_tile")


# ---------------------------------------------------------------- batches
def assemble(name, items, seed=1, step_us=100):
    """Items -> records. Each frame gets 0..15 trailing pad bytes behind the IP packet (random bytes;
    Item.steer / Item.pad fix the amount), so successive records drift through every residue."""
    rng = random.Random(seed)
    recs, parts, off = [], [], 0
    for i, it in enumerate(items):
        if it.steer is not None:
            pad = (it.steer - (off + 16 + len(it.frame))) & 15
        elif it.pad is not None:
            pad = it.pad
        else:
            pad = rng.randrange(16)
        f = it.frame + rng.randbytes(pad)
        cap = len(f) if it.cap is None else it.cap
        us = i * step_us
        rec = pc.record(f, cap, T0 + us // 1_000_000, us % 1_000_000)
        # the IP length trims the UDP payload to the message and the capture bounds both: the frame walk
        # starts from caplen (parse_record, like the oracle's parse_packet), so the L4 length it hands
        # the DNS pass never exceeds the capture (test_dns_corpus.py checks these figures on the oracle)
        dns = cap >= it.msg_off
        mcap = cap - it.msg_off if dns else 0
        recs.append(Rec(off, off + 16 + it.msg_off, min(len(it.msg), mcap), mcap, it.msg, it.fam, dns))
        parts.append(rec)
        off += len(rec)
    return Batch(name, b"".join(parts), recs)


def family_items(seed=7):
    """{family: [Item]} with one generator, so the names are distinct across the families too"""
    g = Gen(seed)
    return {fam: fn(g) for fam, fn in FAMILIES.items()}


def family_batches(seed=7):
    return {fam: assemble(fam, items, seed) for fam, items in family_items(seed).items()}


def mixed_batches(seed=7):
    """all families shuffled, and the same records in reverse order"""
    items = [it for fam in family_items(seed).values() for it in fam]
    random.Random(seed + 1).shuffle(items)
    return assemble("mixed", items, seed), assemble("mixed_reversed", items[::-1], seed)


def large_batch(seed=11, rounds=2):
    """about 6,800 records in one shuffle: about a hundred 64-message tiles. (On a device with more
    ranges than that each range is one tile and only the first wave of a workgroup decodes: the
    waves of a workgroup are waves_batch's subject.)"""
    g = Gen(seed)
    items = []
    for _ in range(rounds):
        for fn in FAMILIES.values():
            items += fn(g)
    for name in SHAPES:
        items += shape(g, name)
    random.Random(seed).shuffle(items)
    return assemble("large", items, seed)


def waves_batch(ranges, tiles_per_range=10, seed=13):
    """A batch that gives every one of `ranges` ranges of the DNS pass tiles_per_range tiles of 64 DNS
    messages, so that all eight waves of a workgroup stage and decode, some a second tile (the
    descriptor and window prefetch rotation), and each range's long list fills several tiles of the
    long pass. The families and tile shapes once, without the captures cut in front of the DNS
    message (every record is a DNS message), repeated in fresh shuffles with fresh pads: the names
    repeat, so the top lists stay short and a wrong decode shows as a new name or a wrong count."""
    g = Gen(seed)
    base = [it for fn in FAMILIES.values() for it in fn(g)]
    for name in SHAPES:
        base += shape(g, name)
    base = [it for it in base if it.cap is None or it.cap >= it.msg_off]
    rng = random.Random(seed)
    n = ranges * tiles_per_range * 64
    items = []
    while len(items) < n:
        rng.shuffle(base)
        items += base
    return assemble("waves", items[:n], seed, step_us=50)


def pass_partition(n_records, cus, wg_per_cu, max_grid=1024):
    """(ranges, tiles per range) of a batch, the host's rule (pv_process: grid = min(tiles,
    cus * wg_per_cu, PV_MAX_GRID), wt_per_block = ceil(tiles / grid), then grid again from it)"""
    tiles = (n_records + 63) // 64
    grid = min(tiles, cus * wg_per_cu, max_grid)
    wt = -(-tiles // grid)
    return -(-tiles // wt), wt


def shape_batches(seed=5):
    g = Gen(seed)
    out = {}
    for name in SHAPES:
        items = shape(g, name)
        out[name] = (assemble(name, items, seed), [i for i, it in enumerate(items) if it.long])
    return out


def pcap_of(batch):
    return pc.pcap([batch.blob])


def all_messages(seed=7):
    """every message of the family corpus and the tile shapes, as the decoder is handed it: the first
    mlen bytes (the capture may have cut it)"""
    out = []
    for b in list(family_batches(seed).values()) + [b for b, _ in shape_batches().values()]:
        out += [(r.fam, r.msg[: r.mlen]) for r in b.recs if r.dns]
    return out


# ---------------------------------------------------------------- DNS over TCP
def tcp_records(messages, seed=3, step_us=100):
    """each message as DNS over TCP in a flow of its own: SYN, the 2-byte length and the message in one
    or two segments cut at a random byte, FIN. Returns the records."""
    from pktvisor_amd.synth import _frame
    import socket
    rng = random.Random(seed)
    src, dst = socket.inet_aton(CLIENT4), socket.inet_aton(RESOLVER4)
    src6, dst6 = socket.inet_pton(socket.AF_INET6, CLIENT6), socket.inet_pton(socket.AF_INET6, RESOLVER6)
    recs, t = [], 0

    def put(frame):
        nonlocal t
        recs.append(pc.record(frame, None, T0 + t // 1_000_000, t % 1_000_000))
        t += step_us

    for k, msg in enumerate(messages):
        v6 = k % 5 == 0
        a, b = (src6, dst6) if v6 else (src, dst)
        port, seq = 2000 + k, rng.getrandbits(32)
        data = struct.pack(">H", len(msg)) + msg
        put(_frame(a, b, port, 53, seq, 0x02, b"", v6))
        seq += 1
        cut = rng.randrange(1, len(data)) if k % 2 and len(data) > 1 else len(data)
        for part in (data[:cut], data[cut:]):
            if part:
                put(_frame(a, b, port, 53, seq, 0x18, part, v6))
                seq += len(part)
        put(_frame(a, b, port, 53, seq, 0x11, b"", v6))
    return recs
