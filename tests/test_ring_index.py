"""pv_ring.h: the index arithmetic of pv_net_combine_ring's hand-over ring (section of a tile, slot
of a lane's tile, sections and so barriers of a range) against a brute-force walk for every range
size from 1 to 64 tiles, as a stand-alone program under ASan + UBSan (tests/native/ring_check_main.cpp)."""
import os
import shutil
import subprocess

NATIVE_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native")


def test_ring_index_arithmetic_under_sanitizers(tmp_path):
    cxx = shutil.which("g++")
    assert cxx
    exe = str(tmp_path / "ring_check")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan", "-o", exe, os.path.join(NATIVE_DIR, "ring_check_main.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.strip().endswith("ring index check: 0 errors")
