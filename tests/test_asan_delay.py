"""The stream delays' host half (aidax_delay_book.h: DelayBook — the capacity and what fits it, the records and parameters, which delays
are on, the runs of streams that restart and the dirty range, against a restatement over seeded random sets by parameters and by
records, offs, records beyond the capacity and flushes, on pools of 1, 2, 7 and 70 streams) under AddressSanitizer +
UndefinedBehaviorSanitizer: `make asan_delay` builds tests/asan_delay_harness.cpp around the product's own header. CPU suite only, like
tests/test_asan_gate.py."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_delays_bookkeeping_under_sanitizers():
    r = subprocess.run(["make", "-s", "-C", ROOT, "asan_delay"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([os.path.join(ROOT, "build", "asan", "asan_delay_harness")], capture_output=True, text=True, timeout=600, env=env)
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-6000:]
    assert r.returncode == 0, (r.returncode, r.stdout[-1000:], r.stderr[-3000:])
    assert "steps, 0 failures" in r.stdout and int(r.stdout.split("asan_delay_harness:")[1].split("steps")[0]) >= 1000, r.stdout
