"""CPU fuzz of the BPF filter's host side: the library's classic-BPF machine (pv_bpf_run,
pv_bpf_filter_records) against the restatement in tests/bpf_progs.py, and its checker
(pv_bpf_validate) against the restatement in tests/bpf_fuzz.py, over seeded random programs, the
programs around the device's LDS / HBM split and the 4096-instruction limit, and a corpus of
adversarial and capture-cut records. The conditions at the end keep the fuzz from being vacuous;
each is counted by the Python restatement alone. tests/test_gpu_bpf_fuzz.py runs the same programs
and corpus through the device machine.

Pinned: the machine's semantics among three implementations (host, device, restatement). Unpinned:
parity with libpcap's bpf_filter, which no image of this project holds."""
import ctypes
import os
import random
import shutil
import struct
import subprocess

import numpy as np
import pytest

import pktvisor_amd as pa
from tests import bpf_fuzz as bf
from tests import bpf_progs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 53
N_PROGRAMS = 2000


@pytest.fixture(scope="module")
def corpus():
    return bf.corpus()


@pytest.fixture(scope="module")
def programs():
    longs = bf.long_programs()
    return bf.random_programs(SEED, N_PROGRAMS), {k: v for k, v in longs.items() if k != "n4097"}, longs["n4097"]


@pytest.fixture(scope="module")
def answers(corpus, programs):
    """the restatement's answer for every program on every frame, and what the runs did"""
    recs, index = corpus
    rand, longs, _ = programs
    frames = [(recs[o + 16:o + 16 + c], w) for o, c, w in index]
    trace = bpf_progs.new_trace()
    out = []
    for p in rand + list(longs.values()):
        out.append([bpf_progs.run(p, f, w, trace) for f, w in frames])
    return out, trace


def validate(lib, prog):
    return lib.pv_bpf_validate(pa.bpf_program(prog) if prog else None, len(prog))


def test_machine_matches_restatement(corpus, programs, answers):
    """pv_bpf_run's full 32-bit answer per program and frame, and pv_bpf_filter_records' bytes"""
    recs, index = corpus
    rand, longs, _ = programs
    want, _ = answers
    lib = pa.load_library()
    buf = np.frombuffer(recs, dtype=np.uint8)
    base = buf.ctypes.data
    run = lib.pv_bpf_run
    for pi, p in enumerate(rand + list(longs.values())):
        assert bf.valid(p)
        arr = pa.bpf_program(p)
        assert lib.pv_bpf_validate(arr, len(p)) == 0, p
        got = [run(arr, base + o + 16, w, c) for o, c, w in index]
        if got != want[pi]:
            k = next(i for i in range(len(index)) if got[i] != want[pi][i])
            o, c, w = index[k]
            raise AssertionError(f"program {pi} {p} on frame {k} (caplen {c}, len {w}, {recs[o + 16:o + 16 + c].hex()}): "
                                 f"pv_bpf_run {got[k]:#x}, restatement {want[pi][k]:#x}")
        kept = b"".join(recs[o:o + 16 + c] for (o, c, w), a in zip(index, want[pi]) if a)
        assert pa.bpf_filter(recs, p) == kept, (pi, p)
    # filter_records of the restatement itself, on a sample (the join above is the same rule)
    for pi in range(0, len(rand), 97):
        kept = b"".join(recs[o:o + 16 + c] for (o, c, w), a in zip(index, want[pi]) if a)
        assert bpf_progs.filter_records(recs, rand[pi]) == kept


def test_long_programs(programs, answers, corpus):
    """the hand-built programs do what they are built for: each keeps some frames and drops others,
    and the 4096-instruction sum is the sum of all its constants"""
    _, longs, too_long = programs
    want, _ = answers
    lib = pa.load_library()
    for name, a in zip(longs, want[N_PROGRAMS:]):
        assert 0 < sum(1 for v in a if v) < len(a), name
    assert len(longs["n4096"]) == 4096 and len(too_long) == 4097
    recs, index = corpus
    total = sum(k for c, _, _, k in longs["n4096"] if c == 0x04)
    for (o, c, w), a in zip(index, want[N_PROGRAMS + list(longs).index("n4096")]):
        assert a == ((int.from_bytes(recs[o + 28:o + 30], "big") + total) & bf.M32 if c >= 14 else 0)
    assert not bf.valid(too_long) and validate(lib, too_long) != 0
    assert bf.valid(too_long[1:]) and validate(lib, too_long[1:]) == 0


def test_checker_every_opcode():
    """every 16-bit code as a one-instruction program in front of a return, k in {0, 15, 16, 31, 32}"""
    lib = pa.load_library()
    arr = pa.bpf_program([(0, 0, 0, 0), (0x06, 0, 0, 0)])
    accepted = set()
    for code in range(1 << 16):
        for k in (0, 15, 16, 31, 32):
            arr[0].code, arr[0].k = code, k
            want = bf.valid([(code, 0, 0, k), (0x06, 0, 0, 0)])
            assert (lib.pv_bpf_validate(arr, 2) == 0) == want, (hex(code), k)
            if want:
                accepted.add(code)
    assert accepted == set(bf.ALLOWED)
    # alone, only a return is a program
    for code in range(1 << 16):
        arr[0].code, arr[0].k = code, 1
        assert (lib.pv_bpf_validate(arr, 1) == 0) == bf.valid([(code, 0, 0, 1)]) == (code in (0x06, 0x16)), hex(code)


def mutations(programs, count):
    rand, _, _ = programs
    rng = random.Random(SEED + 1)
    out = []
    while len(out) < count:
        out.append(bf.mutate(rng, rng.choice(rand)))
    return out


def test_checker_mutations(programs):
    """pv_bpf_validate accepts exactly what valid() accepts over 24,000 single-field mutations of
    valid programs; every field's mutations hold both accepted and refused programs"""
    lib = pa.load_library()
    seen = {}
    for field, p in mutations(programs, 24000):
        want = bf.valid(p)
        assert (validate(lib, p) == 0) == want, (field, p)
        seen.setdefault(field, set()).add(want)
    assert seen == {f: {True, False} for f in ("code", "jt", "jf", "k", "final", "length")}, seen


@pytest.mark.parametrize("n", [2, 3, 200, 258, 4096])
def test_checker_jump_range_edges(n):
    """a target at n - 1 is accepted and one at n refused, for ja, jt and jf, from every distance
    the fields can hold"""
    lib = pa.load_library()
    ret = (0x06, 0, 0, 1)
    for pc_ in sorted({0, max(0, n - 258), max(0, n - 257), max(0, n - 256), n - 2}):
        room = n - 2 - pc_  # the offset onto the last instruction
        cases = [((0x05, 0, 0, room), True), ((0x05, 0, 0, room + 1), False), ((0x05, 0, 0, bf.M32), False),
                 ((0x05, 0, 0, bf.M32 - pc_), False)]
        if room <= 255:
            cases += [((0x15, room, 0, 0), True), ((0x15, 0, room, 0), True)]
        if room + 1 <= 255:
            cases += [((0x15, room + 1, 0, 0), False), ((0x15, 0, room + 1, 0), False)]
        for ins, ok in cases:
            p = [ret] * n
            p[pc_] = ins
            assert bf.valid(p) == ok, (n, pc_, ins)
            assert (validate(lib, p) == 0) == ok, (n, pc_, ins)


def test_conditions(programs, answers):
    """the fuzz reached what it is for (counted by the restatement alone)"""
    rand, longs, _ = programs
    want, trace = answers
    counts = {k: trace[k] for k in bpf_progs.TRACE_COUNTS}
    mixed = sum(1 for a in want[:N_PROGRAMS] if 0 < sum(1 for v in a if v) < len(a))
    big = sum(1 for a in want for v in a if v not in (0, 1, 262144, 0xFFFF, bf.M32))
    print(f"opcodes executed: {len(trace['ops'] & bf.ALLOWED)} of {len(bf.ALLOWED)}; {counts}; "
          f"programs that keep and drop: {mixed} of {N_PROGRAMS}; computed answers (ret a): {big}")
    assert trace["ops"] == set(bf.ALLOWED), sorted(bf.ALLOWED - trace["ops"])
    assert counts["edge_pass"] > 0 and counts["edge_fail"] > 0
    assert counts["div0_x"] > 0
    assert counts["ind_wrap"] > 0
    assert mixed >= 0.2 * N_PROGRAMS, mixed
    assert big > 0
    # the long programs reach both sides of the LDS / HBM split
    for name in longs:
        assert len(longs[name]) > bf.PV_BPF_LDS + 2


def test_host_machine_under_address_and_undefined_sanitizers(tmp_path, corpus, programs, answers):
    """pv_bpf.cpp in a stand-alone program built with -fsanitize=address,undefined: every program
    on every record from a heap block of exactly caplen bytes, the checker on the mutated programs
    from blocks of exactly their length: exit 0, nothing on stderr, the restatement's totals"""
    recs, index = corpus
    rand, longs, too_long = programs
    want, _ = answers
    cxx = shutil.which("g++")
    assert cxx
    exe = str(tmp_path / "bpf_asan")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan", "-o", exe,
                           os.path.join(ROOT, "tests", "native_bpf", "bpf_asan_main.cpp"),
                           os.path.join(ROOT, "pktvisor_amd", "csrc", "pv_bpf.cpp")])
    run_progs = rand + list(longs.values())
    muts = [p for _, p in mutations(programs, 24000)] + [too_long]
    with open(tmp_path / "programs.bin", "wb") as f:
        for flag, ps in ((1, run_progs), (0, muts)):
            for p in ps:
                f.write(struct.pack("<II", flag, len(p)) + b"".join(struct.pack("<HBBI", *i) for i in p))
    (tmp_path / "records.bin").write_bytes(recs)
    r = subprocess.run([exe, str(tmp_path / "programs.bin"), str(tmp_path / "records.bin")], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    n_valid = len(run_progs) + sum(1 for p in muts if bf.valid(p))
    kept = sum(1 for a in want for v in a if v)
    kept_bytes = sum(16 + c for a in want for (o, c, w), v in zip(index, a) if v)
    assert r.stdout.strip() == (f"{len(run_progs) + len(muts)} programs, {n_valid} valid, {len(run_progs)} run on {len(index)} records: "
                                f"sum {sum(sum(a) for a in want)}, kept {kept} records, {kept_bytes} bytes"), r.stdout
