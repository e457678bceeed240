"""The host side of the cabinet IR stage (aidax_ir.cpp: aidax_ir_resample, the fragment packer at 65536 taps, and IrPlan, the stage's plan
builder, against a restatement of its rules over seeded random assignments, commits and passes) under AddressSanitizer +
UndefinedBehaviorSanitizer: `make asan_ir` builds tests/asan_ir_harness.cpp with the product's own sources. CPU suite only, like
tests/test_asan.py."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ir_resample_and_the_packer_under_sanitizers():
    r = subprocess.run(["make", "-s", "-C", ROOT, "asan_ir"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([os.path.join(ROOT, "build", "asan", "asan_ir_harness")], capture_output=True, text=True, timeout=600, env=env)
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-6000:]
    assert r.returncode == 0, (r.returncode, r.stdout[-1000:], r.stderr[-3000:])
    assert "0 failures" in r.stdout and int(r.stdout.split("asan_ir_harness:")[1].split("resample")[0]) > 500, r.stdout
    assert int(r.stdout.split("checksum")[1].split(",")[1].split("plan rebuilds")[0]) > 1000, r.stdout
