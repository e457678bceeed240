"""The IR blend's host side (IrPlan's second assignment, ramps, blend section and blend list, driven as the stage drives it over seeded
random sequences, against a restatement of the rules of include/aidax.h) under AddressSanitizer + UndefinedBehaviorSanitizer:
`make asan_ir_blend` builds tests/asan_ir_blend_harness.cpp, a program of its own, with the product's own host sources. CPU suite only,
like tests/test_asan_ir.py."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_blend_plan_under_sanitizers():
    r = subprocess.run(["make", "-s", "-C", ROOT, "asan_ir_blend"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([os.path.join(ROOT, "build", "asan", "asan_ir_blend_harness")], capture_output=True, text=True, timeout=600, env=env)
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-6000:]
    assert r.returncode == 0, (r.returncode, r.stdout[-1000:], r.stderr[-3000:])
    assert ", 0 failures" in r.stdout, r.stdout
    assert int(r.stdout.split("asan_ir_blend_harness:")[1].split("plan rebuilds")[0]) > 1000, r.stdout
