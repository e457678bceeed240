"""The bus reverbs' host half (aidax_reverb_stage.h: ReverbBook — the buses' records and parameters, the delay capacity and what it
refuses, the dirty range and what a pass uploads, the position per pass, prefix pass and pass of no frames, which changes move a bus's
epoch, and the epoch refresh that keeps the device's modulo-2^32 comparison right from positions just below 2^31 and 2^32, which a book
without the refresh fails — against a restatement over seeded random steps on 1, 3 and 70 buses) under AddressSanitizer +
UndefinedBehaviorSanitizer: `make asan_reverb` builds tests/asan_reverb_harness.cpp with the product's own sources, a program of its own.
CPU suite only, like tests/test_asan_reverb.py."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_bus_reverbs_bookkeeping_under_sanitizers():
    r = subprocess.run(["make", "-s", "-C", ROOT, "asan_reverb"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([os.path.join(ROOT, "build", "asan", "asan_reverb_harness")], capture_output=True, text=True, timeout=600, env=env)
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-6000:]
    assert r.returncode == 0, (r.returncode, r.stdout[-1000:], r.stderr[-3000:])
    assert "steps, 0 failures" in r.stdout and int(r.stdout.split("asan_reverb_harness:")[1].split("steps")[0]) >= 1000, r.stdout
