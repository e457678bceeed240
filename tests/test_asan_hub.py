"""The hub's host half (aidax_hub_book.h: HubBook — who is attached and has submitted, the rotating staging buffers and the pass each
holds, the pass that carried a seat's latest block, when a period is closed early, what a failed launch drops, which passes a k_mfma_lp
give-up condemns — against a restatement over literal rows and seeded random scripts on hubs of 1, 3 and 70 seats) under
AddressSanitizer + UndefinedBehaviorSanitizer: `make asan_hub` builds tests/asan_hub_harness.cpp, a program of its own that includes
nothing but that header. CPU suite only, like tests/test_asan_limit.py."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_hubs_bookkeeping_under_sanitizers():
    r = subprocess.run(["make", "-s", "-C", ROOT, "asan_hub"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([os.path.join(ROOT, "build", "asan", "asan_hub_harness")], capture_output=True, text=True, timeout=600, env=env)
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-6000:]
    assert r.returncode == 0, (r.returncode, r.stdout[-1000:], r.stderr[-3000:])
    assert "steps, 0 failures" in r.stdout and int(r.stdout.split("asan_hub_harness:")[1].split("steps")[0]) >= 1000, r.stdout
