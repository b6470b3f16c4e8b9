"""The BPF filter's fuzz material, shared by tests/test_bpf_fuzz.py (CPU: the host machine and the
checker) and tests/test_gpu_bpf_fuzz.py (the device machine and the compaction): an independent
restatement of the checker, a seeded generator of valid programs and of single-field mutations,
hand-built programs around the device's LDS / HBM program split, and a corpus of records.

valid() restates bpf_check_classic (net/core/filter.c) as its table of allowed opcodes plus its
rules, with the project's one documented deviation: a constant shift of 32 or more is accepted
(the machine takes the count mod 32, as libpcap's C shift does on x86) where the kernel refuses it."""
import random
import struct

from tests import parse_corpus as pc

M32 = 0xFFFFFFFF
MAXINSNS = 4096
MEMWORDS = 16
PV_BPF_LDS = 1024  # instructions the device keeps in LDS (pv_kernels.hip)

# ---------------------------------------------------------------- the checker, restated
LD_PKT = (0x20, 0x28, 0x30, 0x40, 0x48, 0x50)  # ld / ldh / ldb [k], [x + k]
ALU_K = (0x04, 0x14, 0x24, 0x34, 0x44, 0x54, 0x64, 0x74, 0x94, 0xA4)  # add sub mul div or and lsh rsh mod xor #k
ALU_X = tuple(c | 8 for c in ALU_K)
JMP_K = (0x15, 0x25, 0x35, 0x45)  # jeq jgt jge jset #k
JMP_X = tuple(c | 8 for c in JMP_K)
ALLOWED = frozenset(
    (0x00, 0x80, 0x60)            # ld #k, ld len, ld M[k]
    + LD_PKT
    + (0x01, 0x81, 0x61, 0xB1)    # ldx #k, ldx len, ldx M[k], ldxb 4*([k]&0xf)
    + (0x02, 0x03)                # st, stx
    + ALU_K + ALU_X + (0x84,)     # neg
    + (0x05,) + JMP_K + JMP_X     # ja
    + (0x06, 0x16)                # ret #k, ret a
    + (0x07, 0x87))               # tax, txa
assert len(ALLOWED) == 49


def valid(prog) -> bool:
    n = len(prog)
    if not 1 <= n <= MAXINSNS:
        return False
    for pc_, (code, jt, jf, k) in enumerate(prog):
        if code not in ALLOWED:
            return False
        if code in (0x60, 0x61, 0x02, 0x03) and k >= MEMWORDS:
            return False
        if code in (0x34, 0x94) and k == 0:
            return False
        if code == 0x05:
            if pc_ + 1 + k >= n:
                return False
        elif code & 7 == 5:
            if pc_ + 1 + jt >= n or pc_ + 1 + jf >= n:
                return False
    return prog[-1][0] & 7 == 6


# ---------------------------------------------------------------- the corpus
CAPLENS = (0, 1, 13, 14, 15, 33, 34, 35, 47, 48, 49, 111, 112, 113, 1500, 9000, 65535)
BASE_SEC = 1_700_000_000
# what the frames carry in their headers: ethertypes, protocols, ports, version / length bytes
HEADER_VALUES = (0x0800, 0x86DD, 0x8100, 0x88A8, 17, 6, 4, 41, 44, 53, 443, 0x45, 0x60, 0x1FFF, 0x4000, 14, 20, 40, 64)
CONSTS = (0, 1, 31, 32, 33, 0xFFFF, 0xFFFFFFFF)


def caplen_frame(rng, caplen, k):
    """caplen bytes of an Ethernet + IPv4 (or IPv6) + UDP / TCP frame with random payload"""
    proto = 17 if k & 1 else 6
    l4 = struct.pack(">HHHH", 1024 + rng.randrange(4000), 53 if k & 2 else 443, 8, 0)
    kind = 6 if k % 5 == 4 else 4
    f = pc.eth(rng, pc.ip(rng, l4, kind, proto), pc.ET[kind])
    if len(f) < caplen:
        f += rng.randbytes(caplen - len(f))
    return f[:caplen]


def corpus(seed=20240611):
    """(records blob, [(record offset, caplen, wirelen)]): about 1,000 classic-pcap records. The
    adversarial frames of tests/parse_corpus.py (every fourth cut by its caplen), then records of
    every CAPLENS length, half of them with len > caplen. Seconds rise every few records and step
    back twice, so a kept run's change points and its monotone flag depend on what is kept."""
    rng = random.Random(seed)
    frames = []
    for l4gen in (pc.fuzz_l4, pc.dns_l4):
        for family in ("l2", "ipv4", "ipv6", "tunnel", "l4", "mixed"):
            for f in pc.frames_of(rng, family, 50, l4gen):
                cap = len(f) if rng.randrange(4) else rng.randrange(0, len(f) + 1)
                frames.append((f[:cap], len(f)))
    for cap in CAPLENS:
        for k in range(26 if cap < 1000 else 12 if cap == 1500 else 4 if cap == 9000 else 2):
            frames.append((caplen_frame(rng, cap, k), cap if k & 1 else cap + rng.choice((1, 4, 100, 1400))))
    rng.shuffle(frames)
    out, index = bytearray(), []
    for i, (f, wirelen) in enumerate(frames):
        sec = BASE_SEC + i // 7 - (30 if i in (400, 401, 402, 800) else 0)
        index.append((len(out), len(f), wirelen))
        out += struct.pack("<IIII", sec, (i * 7919) % 1_000_000, len(f), wirelen) + f
    return bytes(out), index


# ---------------------------------------------------------------- the generator
LENGTHS = (1, 2, 5, 12, 30, 60, 200)


# ethertype, IPv4 total length and fragment word, IPv6 next header; version / IHL byte, protocol, TTL
HEADER_LOADS = ((0x28, 0, 0, 12), (0x28, 0, 0, 16), (0x28, 0, 0, 20), (0x30, 0, 0, 14), (0x30, 0, 0, 23), (0x30, 0, 0, 20),
                (0x30, 0, 0, 22))


def load_offset(rng, size, wild):
    """wild: also the offsets that hardly any capture of the corpus reaches (a program with one such
    load on its path drops nearly everything, so only some programs draw them)"""
    r = rng.random()
    if r < 0.62:
        return rng.randrange(0, 81)
    if r < 0.88 or not wild:  # a capture's last load that passes and its first that fails
        return (rng.choice(CAPLENS if wild else CAPLENS[:14]) - size + rng.randrange(2)) & M32
    return (M32 - rng.randrange(0, 70)) if rng.random() < 0.7 else rng.getrandbits(32)


def constant(rng):
    r = rng.random()
    if r < 0.45:
        return rng.choice(CONSTS)
    if r < 0.85:
        return rng.choice(HEADER_VALUES)
    return rng.getrandbits(rng.choice((4, 8, 16, 32)))


def jump_offset(rng, room):
    """a forward jump offset of at most `room` (the last instruction), often small or onto the tail"""
    r = rng.random()
    if r < 0.5:
        return min(room, rng.randrange(0, 4))
    if r < 0.8:
        return max(0, room - rng.randrange(0, 2))
    return rng.randrange(0, room + 1)


def ret_insn(rng, keep=None):
    if keep is None:
        keep = rng.random() < 0.5
    if not keep:
        return (0x06, 0, 0, 0)
    return (0x16, 0, 0, 0) if rng.random() < 0.3 else (0x06, 0, 0, rng.choice((1, 262144, 0xFFFF, M32)))


def random_insn(rng, room, wild):
    """one instruction that is not a return; room: how far a jump may reach"""
    r = rng.random()
    if r < 0.30:  # packet loads
        code = rng.choice(LD_PKT + (0xB1,) + (0x28, 0x30))
        size = 1 if code == 0xB1 else {0x00: 4, 0x08: 2, 0x10: 1}[code & 0x18]
        if code in (0x28, 0x30) and rng.random() < 0.5:  # a header field the corpus carries
            return rng.choice(HEADER_LOADS)
        return (code, 0, 0, load_offset(rng, size, wild))
    if r < 0.40:  # the other loads
        code = rng.choice((0x00, 0x80, 0x60, 0x01, 0x81, 0x61))
        if code in (0x60, 0x61):
            return (code, 0, 0, rng.randrange(MEMWORDS))
        if code == 0x01 and rng.random() < 0.5:  # X for an indexed load: small, or near 2^32
            return (code, 0, 0, rng.choice((0, 1, 14, 34, M32, M32 - 13, M32 - 33, 1 << 31) if wild else (0, 1, 14, 34)))
        return (code, 0, 0, constant(rng))
    if r < 0.46:
        return (rng.choice((0x02, 0x03)), 0, 0, rng.randrange(MEMWORDS))
    if r < 0.70:  # ALU
        code = rng.choice(ALU_K + ALU_X + (0x84,))
        if code in (0x3C, 0x9C) and not wild:  # (X is often 0, and the program then drops everything)
            code = rng.choice(ALU_K)
        k = constant(rng)
        if code in (0x34, 0x94) and k == 0:
            k = rng.choice((1, 2, 3, 1000, M32))
        return (code, 0, 0, k)
    if r < 0.94:  # jumps
        if rng.random() < 0.15:
            return (0x05, 0, 0, jump_offset(rng, room))
        return (rng.choice(JMP_K + JMP_X), min(255, jump_offset(rng, room)), min(255, jump_offset(rng, room)), constant(rng))
    return (rng.choice((0x07, 0x87)), 0, 0, 0)


def random_program(rng, n):
    """a program of n instructions that valid() accepts: forward jumps only (classic BPF has no
    others), so it ends; every allowed opcode is drawn"""
    prog = []
    wild = rng.random() < 0.4
    for i in range(n - 1):
        room = n - 2 - i  # the offset that reaches the last instruction
        if i and rng.random() < 0.06:
            prog.append(ret_insn(rng))
        elif i and prog[-1] in HEADER_LOADS and rng.random() < 0.7:  # a test of the field just loaded
            prog.append((rng.choice(JMP_K), min(255, jump_offset(rng, room)), min(255, jump_offset(rng, room)),
                         rng.choice(HEADER_VALUES)))
        else:
            prog.append(random_insn(rng, room, wild))
    keep = rng.random() < 0.5
    if n >= 3 and rng.random() < 0.7:  # two returns at the tail, one keeps and one drops
        prog[n - 2] = ret_insn(rng, not keep)
    prog.append(ret_insn(rng, keep))
    assert valid(prog), prog
    return prog


def random_programs(seed, count):
    rng = random.Random(seed)
    return [random_program(rng, rng.choice(LENGTHS)) for _ in range(count)]


# ---------------------------------------------------------------- programs around pc 1024 and the length limit
FILL = (0x06, 0, 0, 0xDEAD)  # where no path leads: a jump gone wrong answers 0xdead


def long_programs():
    """{name: program}; "n4097" is the one the checker must refuse"""
    out = {}
    # a chain that executes pc 1022, 1023, 1024 and 1025 in one run: A = (ethertype + 3) * 5, kept if > 0x3000
    p = [FILL] * 1029
    p[0] = (0x28, 0, 0, 12)
    p[1] = (0x05, 0, 0, 1020)        # ja -> 1022
    p[1022] = (0x04, 0, 0, 3)
    p[1023] = (0x35, 0, 0, 0)        # jge #0: always, offset 0 -> 1024
    p[1024] = (0x24, 0, 0, 5)
    p[1025] = (0x05, 0, 0, 0)        # ja 0 -> 1026
    p[1026] = (0x25, 0, 1, 0x3000)
    p[1027] = (0x16, 0, 0, 0)
    p[1028] = (0x06, 0, 0, 0)
    out["chain_1024"] = p
    # jt = 255 from the LDS part into the HBM part; jf into the LDS part
    p = [FILL] * 1158
    p[0] = (0x30, 0, 0, 14)
    p[1] = (0x05, 0, 0, 898)         # ja -> 900
    p[900] = (0x45, 255, 0, 1)       # jset #1: -> 1156, else 901
    p[901] = (0x06, 0, 0, 0)
    p[1156] = (0x44, 0, 0, 0x100)
    p[1157] = (0x16, 0, 0, 0)
    out["jt255_across"] = p
    # 4096 instructions, A += k through scratch memory, every k another one: the answer needs every
    # instruction on both sides of 1024
    out["n4096"] = accumulate(4096)
    out["n4097"] = [(0x07, 0, 0, 0)] + accumulate(4096)
    return out


def accumulate(n):
    p = [(0x28, 0, 0, 12), (0x02, 0, 0, 0)]
    g = 0
    while len(p) + 3 <= n - 2:
        g += 1
        p += [(0x60, 0, 0, 0), (0x04, 0, 0, (g * 2654435761) & M32), (0x02, 0, 0, 0)]
    p += [(0x07, 0, 0, 0)] * (n - 2 - len(p))
    p += [(0x60, 0, 0, 0), (0x16, 0, 0, 0)]
    assert len(p) == n
    return p


# ---------------------------------------------------------------- mutations for the checker
def random_anything(rng):
    return (rng.getrandbits(16) if rng.random() < 0.5 else rng.choice(sorted(ALLOWED)), rng.randrange(256), rng.randrange(256),
            rng.choice((0, 1, 15, 16, 31, 32, rng.getrandbits(32))))


def mutate(rng, prog):
    """prog with one field changed: (field, program); about half of them stay valid"""
    p = list(prog)
    n = len(p)
    field = rng.choice(("code", "code", "jt", "jf", "k", "k", "final", "length"))
    i = rng.randrange(n)
    code, jt, jf, k = p[i]
    room = n - 2 - i
    if field == "code":
        r = rng.random()
        code = rng.getrandbits(16) if r < 0.3 else code ^ (1 << rng.randrange(16)) if r < 0.7 else rng.choice(sorted(ALLOWED))
        p[i] = (code, jt, jf, k)
    elif field in ("jt", "jf"):
        js = [j for j in range(n) if p[j][0] & 7 == 5 and p[j][0] != 0x05]
        if js:
            i = rng.choice(js)
            code, jt, jf, k = p[i]
            room = n - 2 - i
        v = rng.choice((max(0, min(255, room)), max(0, min(255, room + 1)), rng.randrange(256), 0, 255))
        p[i] = (code, v, jf, k) if field == "jt" else (code, jt, v, k)
    elif field == "k":
        p[i] = (code, jt, jf, rng.choice((0, 1, 15, 16, 17, 31, 32, max(0, room), room + 1, M32, rng.getrandbits(32))))
    elif field == "final":
        p[-1] = random_anything(rng)
    else:
        r = rng.random()
        if r < 0.4:
            p = p[: rng.randrange(0, n)]
        elif r < 0.8:
            p = p + [random_anything(rng) if rng.random() < 0.5 else ret_insn(rng) for _ in range(rng.randrange(1, 4))]
        else:
            p = p[:i] + p[i + 1:]
    return field, p
