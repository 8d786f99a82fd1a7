"""AddressSanitizer + UndefinedBehaviorSanitizer over the frame ingest's read
contract (tests/sanitize/ingest_asan.cpp, a stand-alone program): the per-tile
code k_ingest's lanes run loops over frames whose planes are heap blocks of
exactly pitch * (rows - 1) + row bytes, so a read past a plane's last row is a
heap-buffer-overflow.  The program checks its outputs itself; the sanitizers
must report nothing.
"""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
ASAN_BIN = os.path.join(HERE, "sanitize", "ingest_asan")


def test_ingest_reads_only_the_rows():
    if not os.path.exists(ASAN_BIN):  # build() makes it; a bare pytest run builds it here
        subprocess.run(["make", "-C", ROOT, "tests/sanitize/ingest_asan"], check=True, capture_output=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1")
    r = subprocess.run([ASAN_BIN], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.stdout + r.stderr)[-3000:]
    assert "ingest ok" in r.stdout
