"""The owning types of aidax_hip_host.h (DevBuf, PinnedBuf, Event, Stream: move-construct, move-assign over a full and over an empty
target, self-move, reset twice, swap, a failed alloc; each resource freed exactly once and an empty owner calling nothing) and the
all-or-nothing builds made from them (SnapshotRing::alloc and GateStage::enable with every one of their calls failing in turn) under
AddressSanitizer + UndefinedBehaviorSanitizer: `make asan_own` builds tests/asan_own_harness.cpp, which defines the runtime entry
points itself and links no HIP library. CPU suite only, like tests/test_asan_gate.py."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_owning_types_under_sanitizers():
    r = subprocess.run(["make", "-s", "-C", ROOT, "asan_own"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([os.path.join(ROOT, "build", "asan", "asan_own_harness")], capture_output=True, text=True, timeout=600, env=env)
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-6000:]
    assert r.returncode == 0, (r.returncode, r.stdout[-1000:], r.stderr[-3000:])
    assert "checks, 0 failures" in r.stdout and int(r.stdout.split("asan_own_harness:")[1].split("checks")[0]) >= 90, r.stdout
