"""ThreadSanitizer over the pipelined run's pop protocol
(tests/sanitize/pop_tsan.cpp, a stand-alone program): 16 threads run the
functions pop_task calls (hartallo_amd/csrc/hl_sched.h) with task_deps /
task_succ over four 8 x 3-MB pictures of zero-cost tasks.  The program checks
the end state itself (every task once, every head at its tail, every pushed
slot taken); TSan must report nothing.
"""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
TSAN_BIN = os.path.join(HERE, "sanitize", "pop_tsan")


def test_pop_protocol_under_tsan():
    if not os.path.exists(TSAN_BIN):  # build() makes it; a bare pytest run builds it here
        subprocess.run(["make", "-C", ROOT, "tests/sanitize/pop_tsan"], check=True, capture_output=True)
    env = dict(os.environ, TSAN_OPTIONS="history_size=7:halt_on_error=1")
    r = subprocess.run([TSAN_BIN], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ThreadSanitizer" not in r.stderr, (r.stdout + r.stderr)[-3000:]
    assert "pop ok" in r.stdout
