"""The model bank's host half (aidax_model_bank.cpp: ModelBank — who plays which slot, the per-stream records, the dirty range and the
commit rules, against a restatement over seeded random slot commits, assignments, pool-model commits and flushes) under AddressSanitizer +
UndefinedBehaviorSanitizer: `make asan_bank` builds tests/asan_bank_harness.cpp with the product's own sources. CPU suite only, like
tests/test_asan_ir.py."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_model_banks_bookkeeping_under_sanitizers():
    r = subprocess.run(["make", "-s", "-C", ROOT, "asan_bank"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([os.path.join(ROOT, "build", "asan", "asan_bank_harness")], capture_output=True, text=True, timeout=600, env=env)
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-6000:]
    assert r.returncode == 0, (r.returncode, r.stdout[-1000:], r.stderr[-3000:])
    assert "steps, 0 failures" in r.stdout and int(r.stdout.split("asan_bank_harness:")[1].split("steps")[0]) >= 1000, r.stdout
