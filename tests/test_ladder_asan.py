"""AddressSanitizer + UndefinedBehaviorSanitizer over the rendition ladder's
fan-out behind the frame ingest (tests/sanitize/ladder_asan.cpp, a stand-alone
program): source planes that are heap blocks of exactly pitch * (rows - 1) +
row bytes, an intermediate buffer, an LDS image sized for the launch's maximum
and every rung's planes of exactly their sizes go through the ingest's tiles
and k_scale_fan's host loop (ladders L1 and L3, two frames per launch), so a
read or write outside any of them is a heap-buffer-overflow.  The program
checks every output sample of every rung against a scalar statement of the
definition; the sanitizers must report nothing.
"""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
ASAN_BIN = os.path.join(HERE, "sanitize", "ladder_asan")


def test_ladder_stays_inside_its_buffers():
    if not os.path.exists(ASAN_BIN):  # build() makes it; a bare pytest run builds it here
        subprocess.run(["make", "-C", ROOT, "tests/sanitize/ladder_asan"], check=True, capture_output=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1")
    r = subprocess.run([ASAN_BIN], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.stdout + r.stderr)[-3000:]
    assert "ladder ok" in r.stdout
